"""Numpy references of unbatched_mesh_to_spc (helper, not collected; no project code).

``dense``   every voxel of every level against every triangle: no proposal lists, no sort.  A voxel is live for a triangle if it
            and all its ancestors pass the 13-axis test; a voxel's face is the smallest live triangle index.
``subtree`` one stage of the walker: the voxels of ``level_to`` below every proposal, in proposal order.
``build``   stable sort of (Morton code, triangle) pairs, first pair of every run, the octree bottom-up.

The voxel test is the reference's (kaolin/csrc/ops/conversions/mesh_to_spc/mesh_to_spc_cuda.cu:98-200) in the precisions of
DESIGN.md's arithmetic contract: vertex minus voxel centre in float32, the rest in float64, unfused, left to right, the comparison on
float32-rounded values.  The voxel size is a power of two, so fmaf(g, size, half - 1) is float32(g * size + (half - 1)) with the
product and the sum exact in float64.  Slow and plain on purpose."""
import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
MAX_LEVEL = 15


def to_point(morton):
    """Morton layout of spc_math.h:98-126: bit 3i = z_i, 3i + 1 = y_i, 3i + 2 = x_i"""
    m = np.asarray(morton, dtype=I64)
    x, y, z = np.zeros_like(m), np.zeros_like(m), np.zeros_like(m)
    for i in range(MAX_LEVEL):
        x |= ((m >> (3 * i + 2)) & 1) << i
        y |= ((m >> (3 * i + 1)) & 1) << i
        z |= ((m >> (3 * i)) & 1) << i
    return x, y, z


def to_morton(x, y, z):
    x, y, z = (np.asarray(a, dtype=I64) for a in (x, y, z))
    m = np.zeros(np.broadcast(x, y, z).shape, dtype=I64)
    for i in range(MAX_LEVEL):
        m |= ((z >> i) & 1) << (3 * i)
        m |= ((y >> i) & 1) << (3 * i + 1)
        m |= ((x >> i) & 1) << (3 * i + 2)
    return m


def centres(morton, level):
    """-> float32 centres (..., 3) of the voxels `morton` of `level`, and the float32 half size"""
    size = F32(2.0) / F32(1 << int(level))
    half = F32(0.5 * F64(size))
    shift = F64(half - F32(1.0))                                             # float32 difference
    c = np.stack([(g.astype(F32).astype(F64) * F64(size) + shift).astype(F32) for g in to_point(morton)], -1)
    return c, half


def _sat(v, half, ax, ay, az):
    d = [v[k][..., 0] * ax + v[k][..., 1] * ay + v[k][..., 2] * az for k in range(3)]
    maxd = np.fmax(d[0], np.fmax(d[1], d[2]))                                # fmax / fmin: a NaN operand is ignored, as in C
    mind = np.fmin(d[0], np.fmin(d[1], d[2]))
    r = F64(half) * (np.abs(ax) + np.abs(ay) + np.abs(az))
    return np.fmax(-maxd, mind).astype(F32) <= np.asarray(r).astype(F32)     # NaN <= x is False


def _normalize(a, b):
    d = b - a
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    inv = 1.0 / np.sqrt(x * x + y * y + z * z)
    return inv * x, inv * y, inv * z


def passes(tv, centre, half):
    """tv (..., 3, 3) float32 triangles, centre (..., 3) float32 (broadcast against each other) -> bool (...): all 13 axes"""
    tv = np.asarray(tv, dtype=F32)
    with np.errstate(all='ignore'):
        v = [(tv[..., k, :] - centre).astype(F64) for k in range(3)]         # float32 differences, then double
        zero, one = F64(0.0), F64(1.0)
        ab, bc, ca = _normalize(v[0], v[1]), _normalize(v[1], v[2]), _normalize(v[2], v[0])
        ok = np.ones(np.broadcast(v[0][..., 0]).shape, dtype=bool)
        for e in (ab, bc, ca):
            ok &= _sat(v, half, zero, -e[2], e[1])
        for e in (ab, bc, ca):
            ok &= _sat(v, half, e[2], zero, -e[0])
        for e in (ab, bc, ca):
            ok &= _sat(v, half, -e[1], e[0], zero)
        ok &= _sat(v, half, one, zero, zero)
        ok &= _sat(v, half, zero, one, zero)
        ok &= _sat(v, half, zero, zero, one)
        ok &= _sat(v, half, ab[1] * bc[2] - ab[2] * bc[1], ab[2] * bc[0] - ab[0] * bc[2], ab[0] * bc[1] - ab[1] * bc[0])
    return ok


def dense(face_vertices, level):
    """-> (morton int64 ascending, face_id int64) of the occupied voxels of `level`.  F * 8^level tests at the deepest level:
    keep that at or below about 1.5 million."""
    fv = np.ascontiguousarray(face_vertices, dtype=F32).reshape(-1, 3, 3)
    F = fv.shape[0]
    if F == 0:
        return np.zeros(0, I64), np.zeros(0, I64)
    live = np.ones((F, 1), dtype=bool)
    for l in range(int(level) + 1):
        c, half = centres(np.arange(8 ** l, dtype=I64), l)                   # the voxel index at a level IS its Morton code
        if l > 0:
            live = np.repeat(live, 8, axis=1)                                # the parent of code m is m >> 3
        live = live & passes(fv[:, None], c[None], half)
    morton = np.nonzero(live.any(axis=0))[0].astype(I64)
    return morton, np.argmax(live[:, morton], axis=0).astype(I64)            # argmax of bools: the smallest passing index


def subtree(face_vertices, morton, tri, level_from, level_to, tested):
    """One stage.  Proposal i is the voxel morton[i] of `level_from` with the triangle tri[i].
    -> (counts (n), morton_out, tri_out): for every proposal, in proposal order, the ascending Morton codes at `level_to` that pass
    with all their ancestors down from `level_from` (its own level included unless `tested`), and the proposal's triangle."""
    fv = np.ascontiguousarray(face_vertices, dtype=F32).reshape(-1, 3, 3)
    code = np.asarray(morton, dtype=I64).copy()
    tri = np.asarray(tri, dtype=I64)
    owner = np.arange(code.shape[0], dtype=I64)

    def keep(code, owner, l):
        if code.shape[0] == 0:
            return code, owner
        c, half = centres(code, l)
        ok = passes(fv[tri[owner]], c, half)
        return code[ok], owner[ok]

    if not tested:
        code, owner = keep(code, owner, level_from)
    for l in range(int(level_from) + 1, int(level_to) + 1):
        code = (code[:, None] * 8 + np.arange(8, dtype=I64)[None]).reshape(-1)   # child k: x = bit 2, y = bit 1, z = bit 0
        owner = np.repeat(owner, 8)
        code, owner = keep(code, owner, l)
    counts = np.bincount(owner, minlength=len(tri)).astype(I64)
    return counts, code, tri[owner]


def build(morton, tri, level):
    """pairs in any order -> (sizes [voxels, nodes per octree level root first], octree uint8, voxel codes, voxel triangles):
    a stable sort by code, the FIRST pair (in input order) of every run of equal codes, then per level the parents of the codes
    below and a byte of their children."""
    morton, tri = np.asarray(morton, dtype=I64), np.asarray(tri, dtype=I64)
    order = np.argsort(morton, kind='stable')
    sm, st = morton[order], tri[order]
    head = np.ones(sm.shape[0], dtype=bool)
    head[1:] = sm[1:] != sm[:-1]
    um, ut = sm[head], st[head]
    levels, cur = [], um
    for _ in range(int(level)):
        parent = cur >> 3
        first = np.ones(cur.shape[0], dtype=bool)
        first[1:] = parent[1:] != parent[:-1]
        bits = (1 << (cur & 7)).astype(I64)
        levels.append(np.add.reduceat(bits, np.nonzero(first)[0]).astype(np.uint8))   # distinct children: a sum is an or
        cur = parent[first]
    levels.reverse()
    sizes = [int(um.shape[0])] + [int(b.shape[0]) for b in levels]
    octree = np.concatenate(levels) if levels else np.zeros(0, np.uint8)
    return sizes, octree, um, ut
