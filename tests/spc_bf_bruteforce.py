"""numpy restatement of the Bayesian-fusion operators of csrc/spc_bf.hip under their arithmetic contract: float32
arrays, one rounding per operation in the order written, no FMA -- numpy's float32 arithmetic is exactly that, so the HIP kernels
and the torch formulations must reproduce every output here bit for bit.

``oracleB`` and ``oracleB_final`` also run in float64 (``dtype=np.float64``) on the same float32 inputs and the same float32 ``T``;
they then return, per point, the MARGIN of the decision: over every comparison (and truncation to a pixel) the decision rests on,
the smallest ``|a - b| / (roundings * scale)``, where ``scale`` bounds the magnitude of the terms the operands were summed from
and ``roundings`` counts the float32 roundings on the longest path to them, so that ``roundings * scale * 2^-24`` bounds the float32
error of ``a - b`` (an exact operand contributes nothing).  A margin above ``U = 2^-24`` therefore means that float32 rounding
cannot change the decision: tests/test_spc_bf_cpu.py compares the float32 decisions with the float64 ones on those cases."""
import numpy as np

NEAR = 0.15
U = 2.0 ** -24
CURVE_B = np.array([[0, 0, 0, 2], [2, 4, 8, 16], [16, 24, 36, 48], [48, 60, 72, 79], [79, 86, 88, 86], [86, 84, 78, 72],
                    [72, 66, 60, 56], [56, 52, 50, 49], [49, 48, 48, 48]], dtype=np.float32)
# roundings on the longest path to a compared value: 3 products and 3 sums for [x y z 1] T, 3 corner sums, the divide, the
# difference of two such values (the extent), and one for the second-order terms of (1 + u)^11
ROUNDINGS_GEOMETRY = 12
# ... then the depth difference, the scaling by 3 / sigma (itself one rounding) and x + 3: the argument of the curve; the curve
# itself is 14 more (t, s, 4 products and a sum per half, 2 products, the sum, the factor)
ROUNDINGS_CURVE = ROUNDINGS_GEOMETRY + 4 + 14


def transform(cam, level):
    """T = M cam in float32: every element the sum over k = 0..3, in that order, of rounded products"""
    c = np.asarray(cam, dtype=np.float32).reshape(4, 4)
    s = np.float32(2.0 ** (1 - level))
    M = np.array([[s, 0, 0, 0], [0, s, 0, 0], [0, 0, s, 0], [-1, -1, -1, 1]], dtype=np.float32)
    T = np.zeros((4, 4), dtype=np.float32)
    for i in range(4):
        for j in range(4):
            acc = np.float32(M[i, 0] * c[0, j])
            for k in range(1, 4):
                acc = np.float32(acc + np.float32(M[i, k] * c[k, j]))
            T[i, j] = acc
    return T


class Margin:
    """per point, the smallest relative distance of a comparison from equality (float64 evaluation only)"""

    def __init__(self, n, on):
        self.on = on
        self.value = np.full(n, np.inf)

    def cmp(self, a, b, scale, active=None, roundings=None):
        """self.value has the shape of the operands: one margin per point, or per corner"""
        if not self.on:
            return
        with np.errstate(all='ignore'):
            m = np.abs(np.asarray(a, dtype=np.float64) - b) / np.maximum(scale * (roundings or ROUNDINGS_GEOMETRY), 1e-300)
        m = np.where(np.isnan(m), 0.0, m)
        if active is not None:
            m = np.where(active, m, np.inf)
        self.value = np.minimum(self.value, m)

    def pixel(self, v, scale, active=None):
        """truncation to a pixel index: the distance to the nearest integer"""
        if self.on:
            self.cmp(v, np.round(v), scale, active)


def corners(points, T, dt):
    """-> q (n, 8, 3) = (x / z, y / z, z) of the eight corners, and the scale of every entry"""
    T = T.astype(dt)
    p = points.astype(dt)
    x, y, z = p[:, 0:1], p[:, 1:2], p[:, 2:3]
    O = ((x * T[0] + y * T[1]) + z * T[2]) + T[3]
    S0 = np.abs(x) * np.abs(T[0]) + np.abs(y) * np.abs(T[1]) + np.abs(z) * np.abs(T[2]) + np.abs(T[3])
    q = np.zeros((len(p), 8, 3), dtype=dt)
    scale = np.zeros((len(p), 8, 3))
    with np.errstate(all='ignore'):
        for i in range(8):
            P, S = O[:, :3], S0[:, :3]
            for bit, row in ((4, 0), (2, 1), (1, 2)):
                if i & bit:
                    P = P + T[row, :3]
                    S = S + np.abs(T[row, :3])
            q[:, i, 0], q[:, i, 1], q[:, i, 2] = P[:, 0] / P[:, 2], P[:, 1] / P[:, 2], P[:, 2]
            az = np.abs(P[:, 2]).astype(np.float64)
            for j in range(2):
                scale[:, i, j] = np.abs(q[:, i, j]) + S[:, j] / az + np.abs(q[:, i, j]) * S[:, 2] / az
            scale[:, i, 2] = S[:, 2]
    return q, np.where(np.isfinite(scale), scale, np.inf)


def build_mip2d(depth, intrinsics, mip_levels, max_depth, true_depth):
    """-> (mip (size, 2) float32 coarsest level first, the depth map as the operator leaves it)"""
    d = np.array(depth, dtype=np.float32)
    h, w = d.shape
    k = np.asarray(intrinsics, dtype=np.float32).reshape(-1)
    fx, fy, cx, cy = k[0], k[5], k[8], k[9]
    if true_depth:
        u = (np.arange(w, dtype=np.float32) - cx) / fx
        v = (np.arange(h, dtype=np.float32) - cy) / fy
        factor = np.float32(1.0) / np.sqrt((u[None, :] * u[None, :] + v[:, None] * v[:, None]) + np.float32(1.0))
        d = np.where(d == np.float32(max_depth), d, d * factor).astype(np.float32)
    levels, lo, hi = [], d, d
    for _ in range(mip_levels):
        lo = np.fmin(np.fmin(lo[0::2, 0::2], lo[1::2, 0::2]), np.fmin(lo[0::2, 1::2], lo[1::2, 1::2]))
        hi = np.fmax(np.fmax(hi[0::2, 0::2], hi[1::2, 0::2]), np.fmax(hi[0::2, 1::2], hi[1::2, 1::2]))
        levels.append(np.stack([lo.reshape(-1), hi.reshape(-1)], axis=1))
    return np.concatenate(levels[::-1]).astype(np.float32), d


def oracleB(points, level, sigma, cam, depth, mips, mip_levels, dtype=np.float32):
    """-> (occupancy, state, branch, margin): branch names the path of every point -- 'mip0', 'mid', 'top' (miplevel ==
    mip_levels), 'high' (above mip_levels), 'straddle', 'outside' (wholly outside the image), 'behind' (the near plane)"""
    n, dt, f64 = len(points), dtype, dtype == np.float64
    if level == 0 or n == 0:
        return np.ones(n, np.int32), np.full(n, 2, np.int32), np.full(n, 'level0', dtype=object), np.full(n, np.inf)
    h, w = depth.shape
    L = mip_levels
    hw = (h >> L) * (w >> L)
    q, sc = corners(points, transform(cam, level), dt)
    with np.errstate(all='ignore'):
        lo, hi = q[:, 0].copy(), q[:, 0].copy()
        for c in range(1, 8):
            lo, hi = np.fmin(lo, q[:, c]), np.fmax(hi, q[:, c])
        lo, hi = np.fmin(lo, np.finfo(np.float32).max), np.fmax(hi, -np.finfo(np.float32).max)
    S = sc.max(axis=1)                                        # (n, 3): a min / max is one of the corners' values
    near = dt(np.float32(NEAR))
    mg = Margin(n, f64)
    with np.errstate(all='ignore'):
        ordered = (lo <= hi).all(axis=1)                      # a coordinate that is NaN at every corner: the voxel is kept
    inside = ordered & (lo[:, 0] >= 0) & (hi[:, 0] < w) & (lo[:, 1] >= 0) & (hi[:, 1] < h) & (lo[:, 2] > near)
    outside = ordered & ~inside & ((hi[:, 0] < 0) | (lo[:, 0] > w) | (hi[:, 1] < 0) | (lo[:, 1] > h) | (hi[:, 2] < near))
    for j, size in ((0, w), (1, h)):
        mg.cmp(lo[:, j], 0, S[:, j]), mg.cmp(hi[:, j], size, S[:, j])
        mg.cmp(hi[:, j], 0, S[:, j], ~inside), mg.cmp(lo[:, j], size, S[:, j], ~inside)
    mg.cmp(lo[:, 2], near, S[:, 2]), mg.cmp(hi[:, 2], near, S[:, 2], ~inside)
    with np.errstate(all='ignore'):
        extent = np.fmax(hi[:, 0] - lo[:, 0], hi[:, 1] - lo[:, 1])
    m = np.zeros(n, dtype=np.int64)
    for k in range(L + 1):
        with np.errstate(all='ignore'):
            m += (dt(2.0 ** k) < extent)
        if f64:
            with np.errstate(all='ignore'):
                mg.cmp(hi[:, 0] - lo[:, 0], 2.0 ** k, 2 * S[:, 0], inside), mg.cmp(hi[:, 1] - lo[:, 1], 2.0 ** k, 2 * S[:, 1], inside)
    occ, state = np.ones(n, np.int32), np.full(n, 2, np.int32)
    branch = np.where(inside, np.where(m > L, 'high', np.where(m == L, 'top', np.where(m == 0, 'mip0', 'mid'))),
                      np.where(outside, np.where(hi[:, 2] < near, 'behind', 'outside'), 'straddle')).astype(object)
    occ[outside], state[outside] = 0, 1
    sig = dt(np.float32(sigma))
    flat = depth.reshape(-1).astype(dt)
    mipd = mips.astype(dt)
    for i in np.nonzero(inside & (m <= L))[0]:
        mi = int(m[i])
        inv = dt(2.0 ** -mi)
        vals = [inv * lo[i, 0], inv * lo[i, 1], inv * hi[i, 0], inv * hi[i, 1]]
        if f64:
            for v, j in zip(vals, (0, 1, 0, 1)):
                mg.value[i] = min(mg.value[i], abs(v - np.round(v)) / max(float(inv) * S[i, j] * ROUNDINGS_GEOMETRY, 1e-300))
        xmin, ymin, xmax, ymax = (int(v) for v in vals)
        stride, rows = w >> mi, h >> mi
        if not (0 <= xmin <= xmax < stride and 0 <= ymin <= ymax < rows):
            continue
        at = [ymin * stride + xmin, ymin * stride + xmax, ymax * stride + xmin, ymax * stride + xmax]
        if mi > 0:
            off = hw * ((4 ** (L - mi) - 1) // 3)
            zmin, zmax = [mipd[off + a, 0] for a in at], [mipd[off + a, 1] for a in at]
        else:
            zmin = zmax = [flat[a] for a in at]
        with np.errstate(all='ignore'):
            z0 = dt(np.fmin(np.fmin(zmin[0], zmin[1]), np.fmin(zmin[2], zmin[3])) - sig)
            z1 = dt(np.fmax(np.fmax(zmax[0], zmax[1]), np.fmax(zmax[2], zmax[3])) + dt(2.0) * sig)
        v0, v1 = lo[i, 2], hi[i, 2]
        occ[i] = 1 if (z0 <= v1 and v0 <= z1) else 0
        state[i] = 0 if z0 > v1 else (1 if z1 < v0 else 2)
        if f64:
            for a, b in ((z0, v1), (z1, v0)):
                if np.isfinite(a):
                    mg.value[i] = min(mg.value[i], abs(a - b) / max((abs(a) + S[i, 2]) * ROUNDINGS_GEOMETRY, 1e-300))
    return occ, state, branch, mg.value


def profile(x, dt=np.float32):
    """the published curve: 0 for x <= -3, 0.5 for x >= 6, nine cubic Bezier segments between"""
    x = np.asarray(x, dtype=dt)
    curve = (CURVE_B / np.float32(255.0)).astype(dt)
    with np.errstate(all='ignore'):
        mid = (x > -3) & (x < 6)
        xs = np.where(mid, x, dt(0))
        u = xs + dt(3)
        iu = np.trunc(u)
        t = u - iu
        s = dt(1) - t
        c = curve[np.clip(iu, 0, 8).astype(np.int64)]
        c0, c1, c2, c3 = c[..., 0], c[..., 1], c[..., 2], c[..., 3]
        val = dt(2.65625) * (s * s * (s * c0 + (dt(3) * t) * c1) + t * t * ((dt(3) * s) * c2 + t * c3))
        return np.where(mid, val, np.where(x >= 6, dt(0.5), dt(0))).astype(dt)


def profile_derivative(x, dt=np.float32):
    x = np.asarray(x, dtype=dt)
    curve = (CURVE_B / np.float32(255.0)).astype(dt)
    with np.errstate(all='ignore'):
        mid = (x > -3) & (x < 6)
        xs = np.where(mid, x, dt(0))
        u = xs + dt(3)
        iu = np.trunc(u)
        t = u - iu
        s = dt(1) - t
        c = curve[np.clip(iu, 0, 8).astype(np.int64)]
        a0, a1, a2 = s * c[..., 0] + t * c[..., 1], s * c[..., 1] + t * c[..., 2], s * c[..., 2] + t * c[..., 3]
        b0, b1 = s * a0 + t * a1, s * a1 + t * a2
        return np.where(mid, dt(7.96875) * (b1 - b0), dt(0)).astype(dt)


def oracleB_final(points, level, sigma, cam, depth, dtype=np.float32):
    """-> (occupancy, state, probabilities, margin)"""
    n, dt, f64 = len(points), dtype, dtype == np.float64
    if level == 0 or n == 0:
        return np.ones(n, np.int32), np.full(n, 2, np.int32), np.zeros(n, np.float32), np.full(n, np.inf)
    h, w = depth.shape
    q, sc = corners(points, transform(cam, level), dt)
    near = dt(np.float32(NEAR))
    scale = dt(np.float32(3.0) / np.float32(sigma))
    flat = depth.reshape(-1).astype(dt)
    mg = Margin((n, 8), f64)                                  # per corner
    clear_mid = np.zeros((n, 8), dtype=bool)
    with np.errstate(all='ignore'):
        inb = (q[..., 0] >= 0) & (q[..., 0] < w) & (q[..., 1] >= 0) & (q[..., 1] < h) & (q[..., 2] > near)
        for j, size in ((0, w), (1, h)):
            mg.cmp(q[..., j], 0, sc[..., j]), mg.cmp(q[..., j], size, sc[..., j])
            mg.pixel(q[..., j], sc[..., j], inb)
        mg.cmp(q[..., 2], near, sc[..., 2])
        x, y = np.where(inb, q[..., 0], 0).astype(np.int64), np.where(inb, q[..., 1], 0).astype(np.int64)
        d = flat[y * w + x]
        diff = q[..., 2] - d
        arg = scale * diff
        prob = np.where(inb, profile(arg, dt), dt(0.5)).astype(dt)
        if f64:
            # the argument against the ends of the curve, and the curve's value against the two exact states
            arg_scale = np.abs(scale) * (sc[..., 2] + np.abs(d))
            finite = inb & np.isfinite(arg)
            mg.cmp(arg, -3.0, arg_scale + 3.0, finite, ROUNDINGS_GEOMETRY + 4)
            mg.cmp(arg, 6.0, arg_scale + 6.0, finite, ROUNDINGS_GEOMETRY + 4)
            mid = finite & (arg > -3) & (arg < 6)
            # the curve's terms sum to at most 2.65625 * 88 / 255 < 1; its slope is at most 2.65625 * 3 * 12 / 255 < 0.4, which
            # carries the argument's error into the value
            value_scale = 1.0 + 0.4 * arg_scale
            mg.cmp(prob, 0.5, value_scale, mid, ROUNDINGS_CURVE), mg.cmp(prob, 0.0, value_scale, mid, ROUNDINGS_CURVE)
            clear_mid = mid & (mg.value > U)
    # a corner that is clearly on the curve, away from both exact values, makes the cell occupied whatever the others do;
    # otherwise the decision rests on every corner
    margin = np.maximum(np.where(clear_mid, mg.value, 0.0).max(axis=1), mg.value.min(axis=1)) if f64 else np.full(n, np.inf)
    pmin, pmax = prob.min(axis=1), prob.max(axis=1)
    empty, unseen = pmax == 0, (pmin == 0.5) & (pmax == 0.5)
    occ = (~(empty | unseen)).astype(np.int32)
    state = np.where(empty, 0, np.where(unseen, 1, 2)).astype(np.int32)
    return occ, state, prob[:, 0].astype(np.float32), margin


def _to_byte(v):
    with np.errstate(all='ignore'):
        return np.where(v > 0, np.minimum(v, np.float32(255.0)), np.float32(0)).astype(np.int64)


def colorsB_final(points, level, cam, sigma, image, depth, probs):
    """-> (colors (n, 4) uint8 in B, G, R, 0 order, normals (n, 3) float32; a normal that is not finite is a zero row)"""
    f = np.float32
    n = len(points)
    h, w = depth.shape
    T = transform(cam, level)
    p = points.astype(f)
    Q = ((p[:, 0:1] * T[0] + p[:, 1:2] * T[1]) + p[:, 2:3] * T[2]) + T[3]
    colors, normals = np.full((n, 4), 64, np.uint8), np.zeros((n, 3), f)
    scale = f(1.0) / f(sigma)
    flat, img = depth.reshape(-1), image.reshape(-1, 3)
    with np.errstate(all='ignore'):
        qx, qy, qz = Q[:, 0] / Q[:, 2], Q[:, 1] / Q[:, 2], Q[:, 2]
        inb = (qx >= 1) & (qx < w - 1) & (qy >= 1) & (qy < h - 1) & (qz > f(NEAR))
        for i in np.nonzero(inb)[0]:
            if probs[i] == 0:
                colors[i] = 0
                continue
            if probs[i] == f(0.5):
                continue
            at = int(qy[i]) * w + int(qx[i])
            r, g, b = (int(_to_byte(f(255.0) * img[at, c])) for c in range(3))
            colors[i] = (b, g, r, 0)
            du = f(0.5) * (flat[at + 1] - flat[at - 1])
            dv = f(0.5) * (flat[at + w] - flat[at - w])
            dprob = profile_derivative(scale * (qz[i] - flat[at]))
            zi = f(1.0) / qz[i]
            wgt = (scale * dprob) * zi
            hz = (wgt * zi) * ((qz[i] * qz[i] + Q[i, 0] * du) + Q[i, 1] * dv)
            hx, hy = (-wgt) * du, (-wgt) * dv
            g3 = np.array([(T[k, 0] * hx + T[k, 1] * hy) + T[k, 2] * hz for k in range(3)], dtype=f)
            nrm = g3 / np.sqrt((g3[0] * g3[0] + g3[1] * g3[1]) + g3[2] * g3[2])
            if np.isfinite(nrm).all():
                normals[i] = nrm
    return colors, normals


def inclusive_sum(values):
    return np.cumsum(np.asarray(values, dtype=np.int64)).astype(np.int32)


def subdivide(points, insum):
    kept = [i for i in range(len(points)) if (insum[i - 1] if i else 0) != insum[i]]
    out = np.zeros((len(kept), 8, 3), np.int16)
    for s, i in enumerate(kept):
        for c in range(8):
            out[s, c] = 2 * points[i] + np.array([c >> 2, (c >> 1) & 1, c & 1])
    return out.reshape(-1, 3), np.array(kept, dtype=np.int32)


def compactify(points, insum):
    kept = [i for i in range(len(points)) if (insum[i - 1] if i else 0) != insum[i]]
    return points[kept].reshape(-1, 3).astype(np.int16), np.array(kept, dtype=np.int64)


def process_final_voxels(num_nodes, total_nodes, state, nvsum, occupancies, prev_state, octree, empty):
    """-> copies of (octree, empty, occupancies, prev_state) after the operator's in-place writes"""
    octree, empty, occupancies, prev_state = octree.copy(), empty.copy(), occupancies.copy(), prev_state.copy()
    at = len(octree) - total_nodes
    for i in range(num_nodes):
        o = sum(1 << c for c in range(8) if state[8 * i + c] == 2)
        e = sum(1 << c for c in range(8) if state[8 * i + c] in (1, 2))
        octree[at + i], empty[at + i], occupancies[at + i] = o, e, 1 if o else 0
        prev_state[nvsum[i]] = 2 if o else (1 if e else 0)
    return octree, empty, occupancies, prev_state


def compactify_nodes(total_nodes, insum, octree, empty):
    kept = [i for i in range(total_nodes) if (insum[i - 1] if i else 0) != insum[i]]
    return octree[kept].astype(np.uint8), empty[kept].astype(np.uint8)


def exsum_of(octree):
    return np.cumsum([bin(int(b)).count('1') for b in octree]).astype(np.int32)


def identify(k, level, octree, empty, exsum):
    """>= 0 the point index, -1 empty or outside, -2 - depth unseen"""
    if min(k) < 0 or max(k) > (1 << level) - 1:
        return -1
    ord_ = 0
    for l in range(level):
        depth = level - l - 1
        child = (((k[0] >> depth) & 1) << 2) | (((k[1] >> depth) & 1) << 1) | ((k[2] >> depth) & 1)
        if ord_ >= len(octree):
            return -1
        bits = int(octree[ord_])
        if not (bits >> child) & 1:
            return -2 - depth if (int(empty[ord_]) >> child) & 1 else -1
        ord_ = (int(exsum[ord_ - 1]) if ord_ else 0) + bin(bits & ((2 << child) - 1)).count('1')
    return ord_


def merge_empty(points, level, tree0, tree1):
    """tree = (octree, empty, exsum) -> (occupancy, state)"""
    occ, state = np.zeros(len(points), np.int32), np.zeros(len(points), np.int32)
    for i, p in enumerate(points):
        a, b = identify([int(v) for v in p], level, *tree0), identify([int(v) for v in p], level, *tree1)
        if a == -1 or b == -1:
            continue
        occ[i], state[i] = (0, 1) if (a < -1 and b < -1) else (1, 2)
    return occ, state


def bq_merge(points, level, tree0, tree1, offset0, offset1, probs0, probs1, colors0, colors1):
    n, f = len(points), np.float32
    occ, state = np.zeros(n, np.int32), np.zeros(n, np.int32)
    probs, colors = np.zeros(n, f), np.zeros((n, 4), np.uint8)
    for i, p in enumerate(points):
        a, b = identify([int(v) for v in p], level, *tree0), identify([int(v) for v in p], level, *tree1)
        if a == -1 or b == -1:
            continue
        if a < -1 and b < -1:
            state[i] = 1
            continue
        p0 = probs0[a - offset0] if a >= 0 else f(0.5)
        p1 = probs1[b - offset1] if b >= 0 else f(0.5)
        occ[i], state[i] = 1, 2
        probs[i] = (p0 * p1) / (p0 * p1 + (f(1.0) - p0) * (f(1.0) - p1))
        colors[i] = colors0[a - offset0] if a >= 0 else colors1[b - offset1]
    return occ, state, probs, colors


def query_empty(octree, empty, exsum, coords, level):
    out = np.zeros(len(coords), np.int32)
    for i, c in enumerate(np.asarray(coords, dtype=np.float64)):
        v = np.floor((2 ** level) * (c * 0.5 + 0.5))
        out[i] = identify([int(x) for x in v], level, octree, empty, exsum) if np.all((v >= -32768) & (v <= 32767)) else -1
    return out
