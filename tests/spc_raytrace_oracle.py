"""The oracle of tests/test_render_spc_cpu.py and tests/test_render_spc_gpu.py: a numpy restatement of the ray-trace contract
("SPC ray tracing") and of the packed ray operators, written from the contract and not from the package.

Tracing is a recursive descent per ray with scalar float32 arithmetic; fmaf is emulated exactly (float64 product, the TwoSum error
term of the sum, round to odd, then one rounding to float32).  The pack scans and reductions are plain sequential loops in the
features' dtype.  tests/golden/render_spc_examples.json pins it to the reference's recorded answers.  Scenes come from
tests/spc_bruteforce.py, or from raw octree bytes through `scene_from_octree`.  It must not import kaolin_amd.render."""
import struct

import numpy as np

F = np.float32
D = np.float64


class Scene:
    """level, octree (uint8), exsum (int32), points (n, 3) int16, pyramid (2, level + 2) int32"""

    def __init__(self, level, octree, exsum, points, pyramid):
        self.level, self.octree, self.exsum, self.points, self.pyramid = level, octree, exsum, points, pyramid


def scene_from_cube(cube):
    import spc_bruteforce as bf
    d = bf.decode(cube)
    return Scene(d.level, d.octree, d.exsum, d.points, d.pyramid)


def scene_from_octree(octree, level):
    """raw bytes, levels root first (a byte may be 0: a node without children)"""
    octree = np.asarray(octree, dtype=np.uint8)
    levels, used = [[(0, 0, 0)]], 0
    for l in range(level):
        nxt = []
        for x, y, z in levels[l]:
            b = int(octree[used])
            used += 1
            nxt += [(2 * x + (j >> 2), 2 * y + ((j >> 1) & 1), 2 * z + (j & 1)) for j in range(8) if (b >> j) & 1]
        levels.append(nxt)
    assert used == len(octree)
    counts = [len(p) for p in levels]
    pyramid = np.zeros((2, level + 2), dtype=np.int32)
    pyramid[0, :level + 1] = counts
    pyramid[1, 1:] = np.cumsum(counts)
    exsum = np.cumsum([bin(int(b)).count('1') for b in octree]).astype(np.int32).reshape(-1)
    points = np.array([p for lv in levels for p in lv], dtype=np.int16).reshape(-1, 3)
    return Scene(level, octree, exsum, points, pyramid)


# ---- exact float32 arithmetic ----------------------------------------------------------------------------------------------------
def fmaf(a, b, c):
    """fmaf(a, b, c) on float32 values, rounded once"""
    with np.errstate(all='ignore'):
        p = D(a) * D(b)                       # exact: 24 + 24 bits
        c = D(c)
        s = p + c
        if np.isfinite(s):
            t = s - p
            e = (p - (s - t)) + (c - t)       # TwoSum: p + c = s + e exactly
            if np.isfinite(e) and e != 0:
                bits = struct.unpack('<q', struct.pack('<d', float(s)))[0]
                if bits & 1 == 0:             # round to odd: the neighbour on the side of the exact sum
                    bits += 1 if (e > 0) == (s > 0) else -1
                    s = D(struct.unpack('<d', struct.pack('<q', bits))[0])
        return F(s)


def box(o, d, inv, sgn, r):
    """the box test: o = origin - centre; > 0 distance, < 0 origin inside, 0 miss"""
    with np.errstate(all='ignore'):
        if np.fmax(np.fmax(abs(o[0]), abs(o[1])), abs(o[2])) < r:
            return F(-r)
        for k in range(3):
            dk = F(fmaf(r, sgn[k], -o[k]) * inv[k])
            a, b = [x for x in range(3) if x != k]
            if dk >= 0 and abs(fmaf(d[a], dk, o[a])) <= r and abs(fmaf(d[b], dk, o[b])) <= r:
                return dk if dk != 0 else F(0)
        return F(0)


def trace(scene, origin, direction, level, with_exit=False):
    """-> (nuggets (n, 2) int32, entry (n) float32, exit (n) float32): depth-first per ray, rays in input order.  with_exit: a hit
    also needs exit > 0 (what the reference does when it returns both depths)."""
    origin = np.asarray(origin, dtype=F).reshape(-1, 3)
    direction = np.asarray(direction, dtype=F).reshape(-1, 3)
    octree, exsum, points = scene.octree, scene.exsum, scene.points
    nuggets, entry, leave = [], [], []
    for ray in range(len(origin)):
        org, d = origin[ray], direction[ray]
        with np.errstate(all='ignore'):
            inv = [F(D(1.0) / D(d[k])) for k in range(3)]
        sgn = [F(1.0) if np.signbit(d[k]) else F(-1.0) for k in range(3)]
        neg = [F(-s) for s in sgn]

        def visit(pidx, l):
            if pidx >= len(points):
                return
            p = points[pidx]
            r = F(2.0 ** -l)
            o = [F(org[k] - fmaf(r, fmaf(F(2), F(p[k]), F(1)), F(-1))) for k in range(3)]
            dist = box(o, d, inv, sgn, r)
            if l == level:
                if dist > 0:
                    out = box(o, d, inv, neg, r)
                    if not with_exit or out > 0:
                        nuggets.append((ray, pidx))
                        entry.append(dist)
                        leave.append(out)
                return
            if dist == 0 or pidx >= len(octree):
                return
            b = int(octree[pidx])
            s = int(exsum[pidx - 1]) if pidx else 0
            c = 0
            for k in range(3):
                x = D(fmaf(F(0.5), org[k], F(0.5))) - D(2.0 ** -l) * (D(p[k]) + D(0.5))
                c = 2 * c + (1 if x > 0 else 0)
            for j in sorted(range(8), key=lambda j: (bin(j ^ c).count('1'), j)):
                if (b >> j) & 1:
                    visit(s + bin(b & ((2 << j) - 1)).count('1'), l + 1)

        visit(0, 0)
    return (np.array(nuggets, dtype=np.int32).reshape(-1, 2), np.array(entry, dtype=F).reshape(-1),
            np.array(leave, dtype=F).reshape(-1))


# ---- packs: sequential loops in the features' dtype ----------------------------------------------------------------------------
def packs(boundaries):
    """[(first, last + 1)] of every pack; element 0 starts one"""
    b = np.asarray(boundaries).astype(bool).reshape(-1)
    starts = [i for i in range(len(b)) if i == 0 or b[i]]
    return list(zip(starts, starts[1:] + [len(b)]))


def pack_scan(feats, boundaries, prod=False, exclusive=False, reverse=False):
    feats = np.asarray(feats)
    out = np.empty_like(feats)
    identity = feats.dtype.type(1 if prod else 0)
    with np.errstate(all='ignore'):
        for first, end in packs(boundaries):
            idx = list(range(first, end))
            if reverse:
                idx = idx[::-1]
            acc = np.full(feats.shape[1], identity) if exclusive else feats[idx[0]].copy()
            out[idx[0]] = acc
            for prev, i in zip(idx, idx[1:]):
                term = feats[prev] if exclusive else feats[i]
                acc = term * acc if prod else term + acc
                out[i] = acc
    return out


def pack_reduce(feats, boundaries, prod=False):
    feats = np.asarray(feats)
    rows = []
    with np.errstate(all='ignore'):
        for first, end in packs(boundaries):
            acc = feats[first].copy()
            for i in range(first + 1, end):
                acc = acc * feats[i] if prod else acc + feats[i]
            rows.append(acc)
    return np.array(rows, dtype=feats.dtype).reshape(-1, feats.shape[1])
