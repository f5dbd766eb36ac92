"""Brute-force dual octree, trinkets and trilinear interpolation in numpy: the oracle of tests/test_spc_dual_cpu.py and
tests/test_spc_dual_gpu.py.

From a cube decoded by tests/spc_bruteforce.py it derives, without any of the package's code: per level the set of the cells'
corners, sorted by their Morton code with l + 1 bits an axis; trinkets and parents through dictionaries; and, in float64 from the
closed forms, the trilinear coefficients, the interpolated features and both gradients (by the features, and by the LOCAL cell
coordinate u = 2^level (c / 2 + 1 / 2) - p -- the convention of the reference's backward).  tests/golden/spc_dual_examples.json
pins it to the reference's documented answer.  It must not import kaolin_amd.ops.spc."""
import numpy as np

import spc_bruteforce as bf

CORNERS = [(j >> 2, (j >> 1) & 1, j & 1) for j in range(8)]


class Dual:
    """level_points (list of (n_l, 3) int16), points (n, 3) int16, pyramid (2, L + 2) int32, trinkets (num_points, 8) int32 relative
    to the level, parents (num_points) int32 absolute"""


def make_dual(d):
    """d: a spc_bruteforce.Decoded -> Dual"""
    L = d.level
    out = Dual()
    out.level_points, index = [], []
    for l in range(L + 1):
        corners = {(int(x) + a, int(y) + b, int(z) + c) for x, y, z in d.level_points[l] for a, b, c in CORNERS}
        ordered = sorted(corners, key=lambda p: bf.morton_code(*p, bits=l + 1))
        out.level_points.append(np.array(ordered, dtype=np.int16).reshape(-1, 3))
        index.append({p: i for i, p in enumerate(ordered)})
    counts = [len(p) for p in out.level_points]
    out.points = np.concatenate(out.level_points)
    out.pyramid = np.zeros((2, L + 2), dtype=np.int32)
    out.pyramid[0, :L + 1] = counts
    out.pyramid[1, 1:] = np.cumsum(counts)
    trinkets, parents = [], []
    for l in range(L + 1):
        for x, y, z in d.level_points[l].astype(np.int64):
            trinkets.append([index[l][(x + a, y + b, z + c)] for a, b, c in CORNERS])
            parents.append(-1 if l == 0 else d.index[(l - 1, x >> 1, y >> 1, z >> 1)])
    out.trinkets = np.array(trinkets, dtype=np.int32).reshape(-1, 8)
    out.parents = np.array(parents, dtype=np.int32)
    return out


def local(coords, points, level):
    """u (..., 3) float64: the local coordinate of every coordinate in its cell"""
    return 2.0 ** level * (np.asarray(coords, dtype=np.float64) * 0.5 + 0.5) - np.asarray(points, dtype=np.float64)


def coefficients(u):
    """(..., 8) float64: c000, c001, ..., c111, z fastest"""
    w = np.stack([1.0 - u, u], axis=-2)                              # (..., 2, 3): [bit, axis]
    return np.stack([w[..., a, 0] * w[..., b, 1] * w[..., c, 2] for a, b, c in CORNERS], axis=-1)


def coefficient_jacobian(u):
    """(..., 8, 3) float64: d c_k / d u_axis"""
    w = np.stack([1.0 - u, u], axis=-2)
    s = (-1.0, 1.0)
    return np.stack([np.stack([s[a] * w[..., b, 1] * w[..., c, 2], w[..., a, 0] * s[b] * w[..., c, 2],
                               w[..., a, 0] * w[..., b, 1] * s[c]], axis=-1) for a, b, c in CORNERS], axis=-2)


def gather(pidx, points, trinkets, feats):
    """(hit (N) bool, cell (N, 3) float64, corner features (N, 8, D) float64): zeros for a miss"""
    pidx = np.asarray(pidx, dtype=np.int64)
    hit = pidx >= 0
    safe = np.where(hit, pidx, 0)
    f = np.asarray(feats, dtype=np.float64)[np.asarray(trinkets, dtype=np.int64)[safe]]
    return hit, np.asarray(points, dtype=np.float64)[safe], np.where(hit[:, None, None], f, 0.0)


def interpolate(coords, pidx, points, trinkets, feats, level):
    """coords (N, S, 3), pidx (N) with -1 for a miss -> ((N, S, D) float64, corner features (N, 8, D))"""
    hit, cell, f = gather(pidx, points, trinkets, feats)
    c = coefficients(local(coords, cell[:, None, :], level))          # (N, S, 8)
    return np.where(hit[:, None, None], np.einsum('nsk,nkd->nsd', c, f), 0.0), f


def interpolate_backward(coords, pidx, points, trinkets, feats, level, grad_out):
    """-> (grad_feats (num_feats, D), grad_u (N, S, 3), both float64; for the error bounds: sum_i |g_i| per feature row
    (num_feats, D), the number of contributing samples per row (num_feats), and sum_d |g_d| max_k |f_kd| per sample (N, S))"""
    feats64 = np.asarray(feats, dtype=np.float64)
    g = np.asarray(grad_out, dtype=np.float64)
    hit, cell, f = gather(pidx, points, trinkets, feats)
    u = local(coords, cell[:, None, :], level)
    c, J = coefficients(u), coefficient_jacobian(u)
    g = np.where(hit[:, None, None], g, 0.0)
    grad_feats, abs_sum = np.zeros_like(feats64), np.zeros_like(feats64)
    count = np.zeros(len(feats64), dtype=np.int64)
    tr = np.asarray(trinkets, dtype=np.int64)[np.where(hit, np.asarray(pidx, dtype=np.int64), 0)]
    S = g.shape[1]
    for k in range(8):
        np.add.at(grad_feats, tr[hit, k], np.einsum('ns,nsd->nd', c[hit][:, :, k], g[hit]))
        np.add.at(abs_sum, tr[hit, k], np.abs(g[hit]).sum(axis=1))
        np.add.at(count, tr[hit, k], S)
    grad_u = np.einsum('nsd,nkd,nska->nsa', g, f, J)
    scale = np.einsum('nsd,nd->ns', np.abs(g), np.abs(f).max(axis=1))
    return grad_feats, grad_u, abs_sum, count, scale
