"""Numpy oracle of gs_to_voxelgrid (helper, not collected): the reference's expressions
(kaolin/csrc/ops/conversions/gs_to_spc/gs_to_spc_cuda.cu) in its operand order, unfused, in the precisions of DESIGN.md's
arithmetic contract.  Every float32 three-term sum is spelled out (no ``@``: BLAS may reorder it); one octree level per round, a
stable sort by Morton code, the integral in float64.  Slow and plain on purpose."""
import numpy as np

F32, F64 = np.float32, np.float64
FLT_MAX = np.finfo(np.float32).max


def _voxel_size(level):
    return F32(2.0) / F32(1 << int(level))


def prepare(means, scales, rots, iso, tol, level):
    """-> cov3d_invs (G, 6), ab0 (G, 3), ab1 (G, 3), contact points (G, 3, 3), all float32"""
    means, scales, rots = (np.ascontiguousarray(a, dtype=F32) for a in (means, scales, rots))
    G = means.shape[0]
    one, two, zero = F32(1), F32(2), np.zeros(G, F32)
    with np.errstate(all='ignore'):
        s = np.fmax(scales, F32(tol) * _voxel_size(level))
        det_s = s[:, 0].astype(F64) * s[:, 1].astype(F64) * s[:, 2].astype(F64)
        r, x, y, z = (rots[:, k] for k in range(4))
        R = [[one - two * (y * y + z * z), two * (x * y + r * z), two * (x * z - r * y)],
             [two * (x * y - r * z), one - two * (x * x + z * z), two * (y * z + r * x)],
             [two * (x * z + r * y), two * (y * z - r * x), one - two * (x * x + y * y)]]
        S = [[(one / s[:, i]) if i == k else zero for k in range(3)] for i in range(3)]
        M = [[S[i][0] * R[0][j] + S[i][1] * R[1][j] + S[i][2] * R[2][j] for j in range(3)] for i in range(3)]
        Sg = [[M[0][i] * M[0][j] + M[1][i] * M[1][j] + M[2][i] * M[2][j] for j in range(3)] for i in range(3)]
        cov = np.stack([Sg[0][0], Sg[0][1], Sg[0][2], Sg[1][1], Sg[1][2], Sg[2][2]], 1).astype(F32)
        c0, c1, c2, c3, c4, c5 = (cov[:, k].astype(F64) for k in range(6))
        h0 = c3 * c5 - c4 * c4
        h1 = c2 * c4 - c1 * c5
        h2 = c1 * c4 - c2 * c3
        h3 = c0 * c5 - c2 * c2
        h4 = c1 * c2 - c0 * c4
        h5 = c0 * c3 - c1 * c1
        iso64 = F64(F32(iso))
        w = [det_s * np.sqrt(iso64 / h0), det_s * np.sqrt(iso64 / h3), det_s * np.sqrt(iso64 / h5)]
        Q = [[h0, h1, h2], [h1, h3, h4], [h2, h4, h5]]
        cp = np.stack([np.stack([(w[i] * Q[i][k]).astype(F32) for k in range(3)], 1) for i in range(3)], 1)   # (G, 3, 3)
        pmin = np.full((G, 3), FLT_MAX, F32)
        pmax = np.full((G, 3), -FLT_MAX, F32)
        for i in range(3):
            for p in (cp[:, i], F32(-1.0) * cp[:, i]):
                pmin = np.fmin(pmin, p)
                pmax = np.fmax(pmax, p)
        return cov, pmin + means, pmax + means, cp


def _edge_test(c0, c1, c2, c3, c4, c5, iso, s, t, lo, hi):
    two = F32(2)
    a = c0.astype(F64)
    b = (two * (c1 * s + c2 * t)).astype(F64)
    c = (((c3 * s * s + two * c4 * s * t) + c5 * t * t) - F32(iso)).astype(F64)
    d = np.fmax(b * b - 4.0 * a * c, 0.0)
    b2a = -0.5 * b / a
    rd = 0.5 * np.sqrt(d) / a
    r0, r1 = b2a - rd, b2a + rd
    return (d > 0) & ~((hi.astype(F64) <= r0) | (r1 <= lo.astype(F64)))


def _face_test(p, q, vs, i, j, k, o, operands=None):
    t = ((q[:, i] - (p[:, i] + o)).astype(F64) / (2.0 * q[:, i].astype(F64))).astype(F32)
    if operands is not None:
        operands.append(t)
    ok = (F32(0) <= t) & (t <= F32(1))
    f = 1.0 - 2.0 * t.astype(F64)
    hj = (f * q[:, j].astype(F64)).astype(F32)
    hk = (f * q[:, k].astype(F64)).astype(F32)
    return ok & (p[:, j] <= hj) & (hj <= p[:, j] + vs) & (p[:, k] <= hk) & (hk <= p[:, k] + vs)


def decide(g, gid, level, means, cov, ab0, ab1, cp, iso, face_operands=None):
    """GSVoxelInOut for the voxels g (n, 3) at `level` against the Gaussians gid (n) -> bool (n).  `face_operands`: a list that
    receives the operand t of the six face tests, float32 (n) each, axis by axis, the lower face first"""
    vs = _voxel_size(level)
    with np.errstate(all='ignore'):
        v = g.astype(F32) * vs + F32(-1.0)          # == fmaf(g, vs, -1): g * vs is exact (vs is a power of two)
        mean, a0, a1 = means[gid], ab0[gid], ab1[gid]
        inside = np.all(v <= a0, 1) & np.all(v + vs >= a1, 1)
        overlap = ~(np.any(a1 < v, 1) | np.any(a0 > v + vs, 1))
        p = v - mean
        face = np.zeros(len(g), bool)
        for i, j, k in ((0, 1, 2), (1, 0, 2), (2, 0, 1)):
            for o in (F32(0), vs):
                face |= _face_test(p, cp[gid, i], vs, i, j, k, o, face_operands)
        C = [cov[gid, k] for k in range(6)]
        edge = np.zeros(len(g), bool)
        for i in range(4):
            o1, o2 = (vs if i // 2 else F32(0)), (vs if i % 2 else F32(0))
            edge |= _edge_test(C[0], C[1], C[2], C[3], C[4], C[5], iso, p[:, 1] + o1, p[:, 2] + o2, p[:, 0], p[:, 0] + vs)
            edge |= _edge_test(C[3], C[1], C[4], C[0], C[2], C[5], iso, p[:, 0] + o1, p[:, 2] + o2, p[:, 1], p[:, 1] + vs)
            edge |= _edge_test(C[5], C[2], C[4], C[0], C[1], C[3], iso, p[:, 0] + o1, p[:, 1] + o2, p[:, 2], p[:, 2] + vs)
        return inside | (overlap & (face | edge))


def morton(g):
    g = g.astype(np.int64)
    m = np.zeros(len(g), np.int64)
    for b in range(15):
        m |= ((g[:, 0] >> b) & 1) << (3 * b + 2)
        m |= ((g[:, 1] >> b) & 1) << (3 * b + 1)
        m |= ((g[:, 2] >> b) & 1) << (3 * b)
    return m


_CHILD = np.array([[i >> 2, (i >> 1) & 1, i & 1] for i in range(8)], np.int64)


def gs_to_spc(means, scales, rots, iso, tol, level):
    """-> points int16 (N, 3), gaus_id int64 (N,), pack_boundary bool (N,), cov3d_invs float32 (G, 6)"""
    means = np.ascontiguousarray(means, dtype=F32)
    cov, ab0, ab1, cp = prepare(means, scales, rots, iso, tol, level)
    G = means.shape[0]
    g = np.zeros((G, 3), np.int64)
    gid = np.arange(G, dtype=np.int64)
    for l in range(level + 1):
        keep = decide(g, gid, l, means, cov, ab0, ab1, cp, iso) if len(g) else np.zeros(0, bool)
        g, gid = g[keep], gid[keep]
        if l < level:
            g = (2 * g[:, None, :] + _CHILD[None]).reshape(-1, 3)
            gid = np.repeat(gid, 8)
    m = morton(g)
    order = np.argsort(m, kind='stable')
    m, g, gid = m[order], g[order], gid[order]
    boundary = np.ones(len(m), bool)
    boundary[1:] = m[1:] != m[:-1]
    return g.astype(np.int16), gid, boundary, cov


def subtree(means, cov, ab0, ab1, cp, iso, codes, gid, level_from, level_to, tested):
    """One stage.  Proposal i is the voxel codes[i] (Morton) of `level_from` with the Gaussian gid[i]; cov, ab0, ab1, cp come from
    ``prepare`` at the target level of the whole conversion (the clamp does not follow the stage).
    -> (counts (n), out_codes, out_gid): for every proposal, in proposal order, the ascending Morton codes at `level_to` that pass
    ``decide`` with all their ancestors down from `level_from` (its own level included unless `tested`), and the proposal's Gaussian."""
    means = np.ascontiguousarray(means, dtype=F32)
    code = np.asarray(codes, dtype=np.int64).copy()
    gid = np.asarray(gid, dtype=np.int64)
    owner = np.arange(len(code), dtype=np.int64)

    def keep(code, owner, l):
        if len(code) == 0:
            return code, owner
        g = np.zeros((len(code), 3), np.int64)
        for b in range(15):
            for axis in range(3):
                g[:, axis] |= ((code >> (3 * b + 2 - axis)) & 1) << b
        ok = decide(g, gid[owner], l, means, cov, ab0, ab1, cp, iso)
        return code[ok], owner[ok]

    if not tested:
        code, owner = keep(code, owner, int(level_from))
    for l in range(int(level_from) + 1, int(level_to) + 1):
        code = (code[:, None] * 8 + np.arange(8, dtype=np.int64)[None]).reshape(-1)   # child k: x = bit 2, y = bit 1, z = bit 0
        owner = np.repeat(owner, 8)
        code, owner = keep(code, owner, l)
    counts = np.bincount(owner, minlength=len(gid)).astype(np.int64)
    return counts, code, gid[owner]


def integrate_gs(points, gaus_id, means, cov, opacities, level, step, chunk=4096):
    """-> float64 (N,): the value the reference rounds to float32, alpha * sum / step^3 (before the final rounding)"""
    means = np.ascontiguousarray(means, dtype=F32)
    opac = np.ascontiguousarray(opacities, dtype=F32).reshape(-1)
    vs = _voxel_size(level)
    step = int(step)
    step_size = vs / F32(step - 1 if step > 1 else 1)
    idx = np.arange(step, dtype=np.int64).astype(F32)
    out = np.zeros(len(points), F64)
    with np.errstate(all='ignore'):
        for s in range(0, len(points), chunk):
            e = min(s + chunk, len(points))
            gid = gaus_id[s:e]
            fp = (vs * points[s:e].astype(F32)).astype(F64) - 1.0
            fp = fp.astype(F32)
            mean = means[gid]
            c0, c1, c2, c3, c4, c5 = (cov[gid, k].astype(F64)[:, None, None, None] for k in range(6))
            off = [((fp[:, a, None] + idx[None, :] * step_size) - mean[:, a, None]).astype(F64) for a in range(3)]
            vx, vy, vz = off[0][:, :, None, None], off[1][:, None, :, None], off[2][:, None, None, :]
            a = c0 * vx * vx
            inter = a + 2.0 * c1 * vx * vy + c3 * vy * vy
            c = 2.0 * c2 * vx * vz
            ee = 2.0 * c4 * vy * vz
            f = c5 * vz * vz
            total = np.exp(-0.5 * (inter + c + ee + f)).sum(axis=(1, 2, 3))
            out[s:e] = opac[gid].astype(F64) * total / F64(step * step * step)
    return out


def merge(integral32, boundary):
    """1 - the sequential float32 product of (1 - integral) over every pack -> float32 (V,)"""
    one_minus = (F32(1) - integral32.astype(F32)).astype(F32)
    starts = np.flatnonzero(boundary)
    ends = np.append(starts[1:], len(one_minus))
    prod = np.ones(len(starts), F32)
    k = 0
    live = np.arange(len(starts))
    while len(live):
        prod[live] = prod[live] * one_minus[starts[live] + k]
        k += 1
        live = live[starts[live] + k < ends[live]]
    return (F32(1) - prod).astype(F32)


def gs_to_voxelgrid(means, scales, rots, opacities, level, iso=11.345, tol=1. / 8., step=10):
    points, gid, boundary, cov = gs_to_spc(means, scales, rots, iso, tol, level)
    integral = integrate_gs(points, gid, means, cov, opacities, level, step).astype(F32)
    return points[boundary], merge(integral, boundary)
