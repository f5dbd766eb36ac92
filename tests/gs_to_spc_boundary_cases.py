"""The inputs of the gs_to_voxelgrid boundary suite (helper, not collected; shared by tests/test_gs_to_spc_boundaries_cpu.py and
tests/test_gs_to_spc_boundaries_gpu.py).  Every builder is seeded and returns (means, scales, rots, opacities) as float32 numpy
arrays; its docstring says which branch of the pipeline it aims at.  CASES lists them with the level, iso and tol they run at; the
oracle's result of a case is computed once (``oracle_pairs``, ``oracle_integral``) and handed out read-only."""
import functools

import numpy as np

import gs_to_spc_bruteforce as bf
from test_gs_to_spc_cpu import ISO, TOL, centred_gaussians, random_gaussians

F32 = np.float32
MAX_PAIRS = 60000


def _voxel(level):
    return 2.0 / (1 << level)


def _unit(q):
    q = np.asarray(q, dtype=np.float64)
    return (q / np.linalg.norm(q)).astype(F32)


def deep(level):
    """levels 8 - 15: three to five stages of the walker with last stages of span 1, 2 and 3 behind full ones, Morton codes beyond
    32 bits from level 11, five and six sort passes (both parities of the ping-pong)"""
    return random_gaussians(5, level, level)


def extreme_cells(level):
    """one pair per Gaussian at the cells (0, 0, 0) and (2^level - 1,) * 3 -- code 0, the all-ones code and the int16 maximum as a
    point coordinate -- and at about 40 random cells, some of them twice or three times: packs of more than one pair"""
    rng = np.random.RandomState(1000 + level)
    top = (1 << level) - 1
    cells = rng.randint(0, 1 << level, (40, 3))
    cells = np.concatenate([[[0, 0, 0], [top, top, top]], cells, cells[:8], cells[:3], [[top, top, top], [0, 0, 0]]])
    return centred_gaussians(cells[rng.permutation(len(cells))], level)


def needles(level, ratio):
    """one axis `ratio` times the other two: long thin ellipsoids that most voxels meet through an edge only, contact points far
    outside the voxels they cross, inverse covariances whose entries differ by ratio^2"""
    means, scales, rots, opacities = random_gaussians(6, level, 3, voxels=(0.3, 0.6))
    scales[:, 0] *= F32(ratio)
    return means, scales, rots, opacities


def big(scale):
    """one rotated ellipsoid from a fraction of the cube to far larger than it (level 4): the root and whole layers pass through
    the AABB-inside test alone, up to every voxel of the grid"""
    means = np.array([[0.1, -0.05, 0.2]], F32)
    scales = (scale * np.array([[1.0, 0.8, 0.6]])).astype(F32)
    rots = _unit([0.8, 0.3, -0.4, 0.33])[None]
    return means, scales, rots, np.array([0.7], F32)


def straddle():
    """24 ellipsoids of 1 - 3 voxels (level 5) centred exactly on the cube's faces x = 1, y = -1 and just inside z = 1: half of
    every ellipsoid is outside, cells of the outermost layers, the AABB reaches beyond [-1, 1]"""
    means, scales, rots, opacities = random_gaussians(24, 5, 21, voxels=(1.0, 3.0))
    means[0:8, 0] = 1.0
    means[8:16, 1] = -1.0
    means[16:24, 2] = 0.999
    return means, scales, rots, opacities


def _exact_axis_scales(mult, level, iso):
    """axis-aligned scales near mult * voxel / sqrt(iso), moved by a few ulps until the oracle's contact points are exactly
    mult * voxel (the extents then lie on cell faces bit for bit); the nearest candidate if no such triple exists"""
    vs = F32(_voxel(level))
    base = (np.asarray(mult, dtype=np.float64) * float(vs) / np.sqrt(float(F32(iso)))).astype(F32)
    steps = np.array([(a, b, c) for a in range(-3, 4) for b in range(-3, 4) for c in range(-3, 4)])
    steps = steps[np.argsort(np.abs(steps).sum(1), kind='stable')]
    cand = np.tile(base, (len(steps), 1))
    for _ in range(3):
        up = np.nextafter(cand, F32(np.inf))
        down = np.nextafter(cand, F32(0))
        cand = np.where(steps > 0, up, np.where(steps < 0, down, cand))
        steps = steps - np.sign(steps)
    rots = np.tile(np.array([[1, 0, 0, 0]], F32), (len(cand), 1))
    cp = bf.prepare(np.zeros((len(cand), 3), F32), cand, rots, iso, 0.0, level)[3]
    err = np.abs(np.stack([cp[:, k, k] for k in range(3)], 1).astype(np.float64) - np.asarray(mult) * float(vs)).sum(1)
    return cand[int(np.argmin(err))]


CORNER_MULTS = [(1, 1, 1), (2, 1, 1), (1, 2, 3), (2, 2, 2), (1, 3, 1), (3, 1, 2)]
CORNER_AT = [(8, 8, 8), (3, 5, 12), (10, 4, 6), (13, 13, 3), (1, 9, 14), (6, 12, 2)]      # cell corners of level 4, as cell indices


def corner_ties():
    """identity rotations, means exactly on cell corners (level 4), extents of a whole number of voxels: the ellipsoid touches
    cell faces in single points, so the operands of every <= of the AABB, overlap and face tests are equal (t is exactly 0 or 1)"""
    vs = _voxel(4)
    means = (-1.0 + np.array(CORNER_AT, dtype=np.float64) * vs).astype(F32)
    scales = np.stack([_exact_axis_scales(m, 4, ISO) for m in CORNER_MULTS]).astype(F32)
    rots = np.tile(np.array([[1, 0, 0, 0]], F32), (len(means), 1))
    return means, scales, rots, np.linspace(0.2, 0.9, len(means)).astype(F32)


TANGENT_ISO = 25.0


def tangent_edges():
    """a case of this suite's own (level 4, iso 25): axis-aligned spheres of exactly 5 voxels radius whose centre lies on a cell
    corner in two axes and on a cell centre in the third, so cell edges at (3, 4) voxels from the axis are tangent to the sphere
    in their interior: the discriminant of the edge test is exactly 0 there (every operand is exact), and 0 must not count"""
    vs = _voxel(4)
    at = np.array([[8, 8.5, 8], [7.5, 9, 7], [8, 6, 8.5]], dtype=np.float64)
    means = (-1.0 + at * vs).astype(F32)
    scales = np.full((3, 3), vs, F32)
    rots = np.tile(np.array([[1, 0, 0, 0]], F32), (3, 1))
    return means, scales, rots, np.array([0.3, 0.6, 0.9], F32)


DEGENERATE = ['zero quaternion', 'quaternion times 3', 'quaternion (0, 0, 0, 1)', 'NaN mean', 'inf scales', 'one zero scale',
              'NaN scales', 'NaN quaternion']


def degenerate():
    """level 4, one splat per entry of DEGENERATE.  fmaxf / fminf drop a NaN: a NaN scale becomes the clamp, NaN or inf * 0 contact
    points leave the AABB at (FLT_MAX, -FLT_MAX) + mean, which the inside test takes for 'the voxel holds it': every voxel; a NaN
    mean fails every comparison: nothing"""
    means, scales, rots, opacities = random_gaussians(len(DEGENERATE), 4, 31, voxels=(0.5, 1.5))
    rots[0] = 0.0
    rots[1] *= F32(3.0)
    rots[2] = (0.0, 0.0, 0.0, 1.0)
    means[3] = np.nan
    scales[4] = np.inf
    scales[5, 1] = 0.0
    scales[6] = np.nan
    rots[7] = np.nan
    return means, scales, rots, opacities


ISO_TOL = [(1.0, 0.5), (11.345, 0.0), (25.0, 0.125), (0.01, 0.125)]


def iso_tol():
    """scales from far below the clamp to two voxels (level 5), run at every (iso, tol) of ISO_TOL: a clamp that takes most
    splats, no clamp at all, a shell of 5 sigma, and a shell far smaller than a voxel (the inside test decides)"""
    return random_gaussians(12, 5, 4, voxels=(0.05, 2.0))


def zero_scales():
    """level 4: scales (0, 0, 0), one component 0 and (1e-30,) * 3.  With tol = 1/8 all are clamped to an eighth of a voxel; with
    tol = 0 nothing is: 1 / 0 = inf and 1e30^2 = inf in cov3d_invs, inf * 0 = NaN behind them"""
    means, scales, rots, opacities = random_gaussians(3, 4, 41)
    scales[0] = 0.0
    scales[1, 2] = 0.0
    scales[2] = 1e-30
    return means, scales, rots, opacities


# a clamp of tol * voxel = 1.25e-20 at level 4: 1 / s^2 overflows in float, so cov3d_invs is inf / NaN, the contact points are NaN
# and every splat takes the whole grid.  The same tol times the voxel of levels 0 - 2 does not overflow: a clamp that followed the
# level under test would narrow the tree with a finite ellipsoid first and end with 512 pairs of a splat instead of 4096
TINY_TOL = 1e-19


def deep_corner(level):
    """``deep`` with its last mean moved into the cube's far corner: a deep walk (five stages at level 15) that ends at the int16
    maximum as a point coordinate, next to an AABB that reaches beyond the cube on three sides"""
    means, scales, rots, opacities = deep(level)
    means[-1] = 0.99999
    return means, scales, rots, opacities


# name -> (builder, arguments, level, iso, tol)
CASES = {}
for _level in (8, 9, 10, 11, 12, 13, 15):
    CASES[f'deep-{_level}'] = (deep, (_level,), _level, ISO, TOL)
for _level in (11, 15):
    CASES[f'extreme_cells-{_level}'] = (extreme_cells, (_level,), _level, ISO, TOL)
CASES['needles-5-30'] = (needles, (5, 30), 5, ISO, TOL)
CASES['needles-7-100'] = (needles, (7, 100), 7, ISO, TOL)
for _scale in (0.1, 0.25, 0.4, 1.0, 5.0):
    CASES[f'big-{_scale}'] = (big, (_scale,), 4, ISO, TOL)
CASES['straddle'] = (straddle, (), 5, ISO, TOL)
CASES['corner_ties'] = (corner_ties, (), 4, ISO, TOL)
CASES['tangent_edges'] = (tangent_edges, (), 4, TANGENT_ISO, TOL)
CASES['degenerate'] = (degenerate, (), 4, ISO, TOL)
for _iso, _tol in ISO_TOL:
    CASES[f'iso_tol-{_iso}-{_tol}'] = (iso_tol, (), 5, _iso, _tol)
for _tol in (0.0, TINY_TOL, 0.125):
    CASES[f'zero_scales-{_tol}'] = (zero_scales, (), 4, ISO, _tol)
CASES['deep_corner-15'] = (deep_corner, (15,), 15, ISO, TOL)
NAMES = list(CASES)
NOT_FINITE = ['degenerate', 'zero_scales-0.0', f'zero_scales-{TINY_TOL}']    # cases with NaN in cov3d_invs and in the integral
FINITE = [name for name in NAMES if name not in NOT_FINITE]
STEP = 10


def frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> ((means, scales, rots, opacities), level, iso, tol), the arrays read-only"""
    builder, args, level, iso, tol = CASES[name]
    return frozen(builder(*args)), level, iso, tol


@functools.lru_cache(maxsize=None)
def oracle_pairs(name):
    """-> the oracle's (points, gaus_id, pack_boundary, cov3d_invs) of the case, read-only"""
    (means, scales, rots, _), level, iso, tol = case(name)
    return frozen(bf.gs_to_spc(means, scales, rots, iso, tol, level))


@functools.lru_cache(maxsize=None)
def oracle_integral(name, step=STEP):
    """-> the oracle's float64 integral over the oracle's pairs of the case, read-only"""
    (means, _, _, opacities), level, _, _ = case(name)
    points, gid, _, cov = oracle_pairs(name)
    return frozen([bf.integrate_gs(points, gid, means, cov, opacities, level, step)])[0]


def to_morton(points):
    return bf.morton(np.asarray(points).astype(np.int64))


def to_point(codes):
    codes = np.asarray(codes, dtype=np.int64)
    g = np.zeros((len(codes), 3), np.int64)
    for b in range(15):
        for axis in range(3):
            g[:, axis] |= ((codes >> (3 * b + 2 - axis)) & 1) << b
    return g


def face_operands(name):
    """the operand t of the oracle's face test, as ``bf.decide`` hands it out, for every pair of the case's result at the case's
    level, every axis and both faces -> float32 (pairs, 3, 2)"""
    (means, scales, rots, _), level, iso, tol = case(name)
    points, gid, _, _ = oracle_pairs(name)
    operands = []
    prepared = bf.prepare(means, scales, rots, iso, tol, level)
    keep = bf.decide(points.astype(np.int64), gid, level, np.asarray(means, dtype=F32), *prepared, iso, face_operands=operands)
    assert keep.all() and len(operands) == 6
    return np.stack(operands, 1).reshape(len(points), 3, 2)
