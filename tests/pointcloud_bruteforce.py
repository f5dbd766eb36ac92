"""A numpy / pure-Python restatement of the contracts of kaolin.ops.conversions.pointcloud, written from their text: dictionaries from
cell to member list, exact means with fractions.  Shares no code with the package."""
import math
from fractions import Fraction

import numpy as np

UNIT_ROUNDOFF = {np.dtype(np.float16): Fraction(1, 2 ** 11), np.dtype(np.float32): Fraction(1, 2 ** 24), np.dtype(np.float64): Fraction(0)}
SMALLEST_SUBNORMAL = {np.dtype(np.float16): Fraction(1, 2 ** 24), np.dtype(np.float32): Fraction(1, 2 ** 149),
                      np.dtype(np.float64): Fraction(1, 2 ** 1074)}


# ---- unbatched_pointcloud_to_spc ------------------------------------------------------------------------------------------------------
def quantize(points, level):
    """(N, 3) half / float / double -> (N, 3) ints: x + 1 rounded in the dtype, times 2^level, halved, clamped to [0, 2^level - 1],
    floored; NaN -> 0.  numpy rounds every operation in the array's dtype (half: computed in float, rounded to half)."""
    dt = points.dtype.type
    res = 2 ** level
    with np.errstate(all='ignore'):
        t = (points + dt(1)) * dt(res) / dt(2)
    out = np.zeros(points.shape, dtype=np.int64)
    for idx in np.ndindex(points.shape):
        v = float(t[idx])
        if math.isnan(v):
            out[idx] = 0
        else:
            out[idx] = int(math.floor(min(max(v, 0.0), float(res - 1))))
    return out


def morton(x, y, z, level):
    code = 0
    for i in range(level):
        code |= ((z >> i) & 1) << (3 * i) | ((y >> i) & 1) << (3 * i + 1) | ((x >> i) & 1) << (3 * i + 2)
    return code


def cells_of(points, level):
    """{Morton code: [input indices, ascending]} of the quantised points"""
    members = {}
    for i, (x, y, z) in enumerate(quantize(points, level).tolist()):
        members.setdefault(morton(x, y, z, level), []).append(i)
    return members


def octree_of(codes, level):
    """uint8 bytes, levels root first: per level the occupied nodes in Morton order, a bit per child ``x << 2 | y << 1 | z``"""
    levels = []
    cur = sorted(set(codes))
    for _ in range(level):
        parents = {}
        for c in cur:
            parents[c >> 3] = parents.get(c >> 3, 0) | (1 << (c & 7))
        cur = sorted(parents)
        levels.append([parents[p] for p in cur])
    return np.array([b for lv in reversed(levels) for b in lv], dtype=np.uint8)


def to_fraction(value):
    return Fraction(int(value)) if isinstance(value, (bool, np.bool_, int, np.integer)) else Fraction(float(value))


class Oracle:
    """octree (uint8), codes (the cells in Morton order), members (per cell), and with features: mean[r][d] (Fraction, exact),
    abs_sum[r][d] (Fraction: the sum of |f_i| over the members)."""

    def __init__(self, points, level, features=None):
        members = cells_of(points, level)
        self.codes = sorted(members)
        self.members = [members[c] for c in self.codes]
        self.octree = octree_of(self.codes, level)
        self.mean = self.abs_sum = None
        if features is not None:
            rows = [[to_fraction(v) for v in row] for row in features.tolist()]
            D = features.shape[1]
            self.mean = [[sum((rows[i][d] for i in m), Fraction(0)) / len(m) for d in range(D)] for m in self.members]
            self.abs_sum = [[sum((abs(rows[i][d]) for i in m), Fraction(0)) for d in range(D)] for m in self.members]

    def integer_features(self, dtype):
        """the means rounded half to even (Python's round of a Fraction), as `dtype`; bool: non-zero"""
        vals = [[round(v) for v in row] for row in self.mean]
        if np.dtype(dtype) == np.dtype(bool):
            return np.array(vals) != 0
        return np.array(vals, dtype=np.int64).astype(dtype)

    def float_bound(self, r, d, dtype):
        """|got - mean| <= (gamma_n sum|f_i| / n + u_out |mean|) (1 + 2^-10) + s_out / 2: n double additions in any order, one
        division, one cast (half through float: the 2^-10 pays for the double rounding)"""
        n = len(self.members[r])
        gamma = Fraction(n, 2 ** 53) / (1 - Fraction(n, 2 ** 53))
        dt = np.dtype(dtype)
        return (gamma * self.abs_sum[r][d] / n + UNIT_ROUNDOFF[dt] * abs(self.mean[r][d])) * (1 + Fraction(1, 2 ** 10)) + \
            SMALLEST_SUBNORMAL[dt] / 2

    def worst_share(self, got):
        """max over the entries of |got - mean| / bound (must be <= 1); `got` (U, D) numpy of a float dtype"""
        assert got.shape == (len(self.members), len(self.mean[0])), (got.shape, len(self.members))
        worst = Fraction(0)
        for r in range(got.shape[0]):
            for d in range(got.shape[1]):
                g = float(got[r, d])
                assert math.isfinite(g), (r, d, g)
                worst = max(worst, abs(Fraction(g) - self.mean[r][d]) / self.float_bound(r, d, got.dtype))
        return float(worst)


# ---- pointclouds_to_voxelgrids --------------------------------------------------------------------------------------------------------
def voxelgrids(points, resolution, origin, scale):
    """(B, P, 3), origin (B, 3), scale (B) of one float dtype -> (B, R, R, R) bool: round_half_even(((p - origin) / scale) (R - 1)),
    every operation rounded in the dtype, kept when all three lie in [0, R - 1] (NaN and inf do not)."""
    dt = points.dtype.type
    B, R = points.shape[0], resolution
    with np.errstate(all='ignore'):
        v = np.rint(((points - origin[:, None, :]) / scale[:, None, None]) * (np.ones(1, dtype=points.dtype) * dt(R - 1)))
    grid = np.zeros((B, R, R, R), dtype=bool)
    for b in range(B):
        for x, y, z in v[b].astype(np.float64).tolist():
            if all(math.isfinite(c) and 0 <= c <= R - 1 for c in (x, y, z)):
                grid[b, int(x), int(y), int(z)] = True
    return grid
