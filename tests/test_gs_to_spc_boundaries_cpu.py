"""gs_to_voxelgrid at its boundaries, without a GPU: the cases of tests/gs_to_spc_boundary_cases.py (deep levels, needles, splats
larger than the cube or across its faces, exact ties, degenerate quaternions / scales / means, iso and tol varied) through the
torch formulation against the numpy oracle -- the integer results and cov3d_invs bit for bit, the integral within one float32 ulp
of the oracle's float64 value, NaN exactly where the oracle's value is NaN -- and the oracle against itself and against geometry:
its stage-wise form ``subtree`` chained over any split of the levels gives the pairs of ``gs_to_spc``, and every voxel that a
float64 sample of a splat's iso surface falls in is paired with that splat."""
import numpy as np
import pytest
import torch

import gs_to_spc_bruteforce as bf
import gs_to_spc_boundary_cases as cases
from test_gs_to_spc_cpu import C, ISO, TOL, check_against_oracle, check_integral, check_merged, kal, random_gaussians, t, ulp_share


# --------------------------------------------------------------------------------------- the cases are what they claim to be
@pytest.mark.parametrize('name', cases.NAMES)
def test_case_yields_pairs_within_the_cap(name):
    (means, _, _, _), level, _, _ = cases.case(name)
    points, gid, boundary, cov = cases.oracle_pairs(name)
    assert 1 <= len(points) <= cases.MAX_PAIRS
    assert gid.min() >= 0 and gid.max() < len(means) and points.min() >= 0 and points.max() < (1 << level)


def test_whole_grid_splats_stay_at_level_4():
    """a splat whose AABB is (FLT_MAX, -FLT_MAX) + mean, or larger than the cube, is paired with all 8^level voxels"""
    per_splat = np.bincount(cases.oracle_pairs('degenerate')[1], minlength=len(cases.DEGENERATE))
    print('degenerate: pairs per splat', dict(zip(cases.DEGENERATE, per_splat.tolist())))
    assert cases.case('degenerate')[1] == 4 and cases.case('big-5.0')[1] == 4
    assert per_splat[cases.DEGENERATE.index('NaN quaternion')] == 4096
    assert per_splat[cases.DEGENERATE.index('inf scales')] == 4096
    assert per_splat[cases.DEGENERATE.index('NaN mean')] == 0
    # the clamp took it: a sphere of sqrt(iso) / 8 = 0.42 voxels radius touches one to eight voxels
    assert 1 <= per_splat[cases.DEGENERATE.index('NaN scales')] <= 8
    for k in (0, 1, 2, 5):
        assert 0 < per_splat[k] < 4096
    assert len(cases.oracle_pairs('big-5.0')[0]) == 4096
    sizes = [len(cases.oracle_pairs(f'big-{s}')[0]) for s in (0.1, 0.25, 0.4, 1.0, 5.0)]
    print('big: pairs', sizes)
    assert sizes[0] < 200 and sizes == sorted(sizes)


def test_zero_scales_without_a_clamp_are_not_finite():
    assert np.isinf(cases.oracle_pairs('zero_scales-0.0')[3]).any() and np.isnan(cases.oracle_pairs('zero_scales-0.0')[3]).any()
    assert np.isfinite(cases.oracle_pairs('zero_scales-0.125')[3]).all()
    # a clamp so small that 1 / s^2 overflows at the target level (not with the voxel of level 0): the whole grid for every splat
    tiny = cases.oracle_pairs(f'zero_scales-{cases.TINY_TOL}')
    assert np.isinf(tiny[3]).any(1).all() and np.bincount(tiny[1]).tolist() == [4096] * 3
    coarse = bf.prepare(*cases.case(f'zero_scales-{cases.TINY_TOL}')[0][:3], cases.ISO, cases.TINY_TOL, 0)[0]
    assert np.isfinite(coarse).all()
    assert np.isnan(cases.oracle_pairs('degenerate')[3]).any()
    for name in cases.FINITE:
        assert np.isfinite(cases.oracle_pairs(name)[3]).all() and np.isfinite(cases.oracle_integral(name)).all(), name


def test_deep_cases_reach_the_wide_codes():
    for name in ('deep-15', 'deep_corner-15', 'extreme_cells-15'):
        codes = cases.to_morton(cases.oracle_pairs(name)[0])
        assert ((codes >> 44) & 1).any(), name
    # the int16 maximum: deep's means stay within 0.9 of the centre (coordinates up to 31 130), so deep_corner moves one mean there
    for name in ('deep_corner-15', 'extreme_cells-15'):
        assert cases.oracle_pairs(name)[0].max() == 32767 == np.iinfo(np.int16).max, name
    assert (cases.oracle_pairs('deep_corner-15')[0] == 32767).all(1).any()           # the corner voxel itself
    assert cases.oracle_pairs('extreme_cells-15')[0].min() == 0
    assert cases.to_morton(cases.oracle_pairs('deep-11')[0]).max() >= 2 ** 32
    assert cases.to_morton(cases.oracle_pairs('extreme_cells-11')[0]).max() == 8 ** 11 - 1
    for name in ('extreme_cells-11', 'extreme_cells-15'):
        packs = np.diff(np.append(np.flatnonzero(cases.oracle_pairs(name)[2]), len(cases.oracle_pairs(name)[2])))
        assert packs.max() >= 3 and (packs == 1).any(), name


def test_corner_ties_has_exact_face_operands():
    tt = cases.face_operands('corner_ties')
    zeros, ones = int((tt == 0).sum()), int((tt == 1).sum())
    print(f'corner_ties: {tt.size} face operands, {zeros} exactly 0, {ones} exactly 1')
    assert zeros > 0 and ones > 0


def test_tangent_edges_has_a_zero_discriminant_inside_an_edge():
    """for the first splat the cell edge along y at (-3, -4) voxels from the centre: b = 0 and c = 9 + 16 - 25 = 0 in floats"""
    (means, scales, rots, _), level, iso, tol = cases.case('tangent_edges')
    cov = cases.oracle_pairs('tangent_edges')[3]
    vs = np.float32(2.0 / 16)
    s, u = np.float32(-3) * vs, np.float32(-4) * vs
    c = ((cov[0, 0] * s * s + np.float32(2) * cov[0, 2] * s * u) + cov[0, 5] * u * u) - np.float32(iso)
    assert c == 0 and cov[0, 1] == 0 and cov[0, 4] == 0
    # the voxel outside that edge is not paired with the splat, its three neighbours around the edge are
    points, gid, _, _ = cases.oracle_pairs('tangent_edges')
    mine = {tuple(p) for p in points[gid == 0].tolist()}
    assert (4, 8, 3) not in mine and {(5, 8, 4), (4, 8, 4), (5, 8, 3)} <= mine


# ------------------------------------------------------------------------------------ the torch formulation against the oracle
@pytest.mark.parametrize('name', cases.NAMES)
def test_torch_formulation_equals_oracle(name):
    data, level, iso, tol = cases.case(name)
    want, _ = check_against_oracle(data, level, 'cpu', iso, tol)
    assert all(np.array_equal(w, o, equal_nan=True) for w, o in zip(want, cases.oracle_pairs(name)))


def check_integral_with_nan(name, device, step=cases.STEP):
    """the integral over the oracle's pairs: NaN exactly where the oracle's float64 value is NaN, within the one-ulp bound elsewhere"""
    (means, _, _, opacities), level, _, _ = cases.case(name)
    points, gid, _, cov = cases.oracle_pairs(name)
    w = cases.oracle_integral(name, step)
    got = C.integrate_gs_cuda(t(points, device), t(gid, device), t(means, device), t(cov, device), t(opacities, device), level, step)
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == w.shape
    nan = np.isnan(w)
    assert np.array_equal(np.isnan(got), nan)
    share = ulp_share(got[~nan], w[~nan]).max()
    print(f'integrate_gs {device} {name} step {step}: {len(w)} pairs, {int(nan.sum())} NaN, worst share of the bound {share:.3f}')
    assert nan.any() and share <= 1.0
    return share


@pytest.mark.parametrize('name', cases.FINITE)
def test_integral_within_one_ulp(name):
    data, level, _, _ = cases.case(name)
    check_integral(data, level, cases.STEP, 'cpu', pairs=cases.oracle_pairs(name))


@pytest.mark.parametrize('name', cases.NOT_FINITE)
def test_integral_is_nan_where_the_oracle_is(name):
    check_integral_with_nan(name, 'cpu')


@pytest.mark.parametrize('name', ['straddle', 'needles-5-30', 'extreme_cells-11'])
def test_merged_opacities(name):
    data, level, iso, tol = cases.case(name)
    assert (iso, tol) == (ISO, TOL)
    voxels, merged = kal.ops.conversions.gs_to_voxelgrid(*(t(a) for a in data), level)
    check_merged(data, level, voxels, merged)


# ------------------------------------------------------------------------------------------------- the oracle against itself
SPLITS = [(3,), (1,), (2, 3, 1), (0, 3)]      # spans of the stages, the last one repeated; (0, 3): a stage that only tests the root


def chain(data, level, iso, tol, split):
    means, scales, rots, _ = data
    cov, ab0, ab1, cp = bf.prepare(means, scales, rots, iso, tol, level)
    codes, gid = np.zeros(len(means), np.int64), np.arange(len(means), dtype=np.int64)
    level_from, tested, k = 0, 0, 0
    while True:
        level_to = min(level_from + split[min(k, len(split) - 1)], level)
        counts, codes, gid = bf.subtree(means, cov, ab0, ab1, cp, iso, codes, gid, level_from, level_to, tested)
        assert counts.sum() == len(codes)
        if level_to == level:
            return codes, gid
        level_from, tested, k = level_to, 1, k + 1


@pytest.mark.parametrize('split', SPLITS, ids=lambda s: '-'.join(map(str, s)))
@pytest.mark.parametrize('level', [7, 13])
def test_subtree_chained_over_any_split_gives_the_pairs(level, split):
    data = random_gaussians(5, level, level)
    points, gid, _, _ = bf.gs_to_spc(*data[:3], ISO, TOL, level)
    order = np.argsort(gid, kind='stable')                   # (code, Gaussian) -> (Gaussian, code): the order before the sort
    codes, ids = chain(data, level, ISO, TOL, split)
    assert len(codes) > 0
    assert np.array_equal(codes, cases.to_morton(points)[order]) and np.array_equal(ids, gid[order])


def test_subtree_counts_follow_the_proposals():
    """proposals repeated and out of order; `tested` skips the proposal's own level only"""
    data = random_gaussians(5, 4, 4)
    prep = bf.prepare(*data[:3], ISO, TOL, 4)
    root = np.zeros(5, np.int64)
    _, codes, gid = bf.subtree(data[0], *prep, ISO, root, np.arange(5), 0, 2, 0)
    pick = np.array([3, 0, 3, len(codes) - 1, 1])
    counts, out, out_gid = bf.subtree(data[0], *prep, ISO, codes[pick], gid[pick], 2, 4, 1)
    single = [bf.subtree(data[0], *prep, ISO, codes[[i]], gid[[i]], 2, 4, 1) for i in pick]
    assert counts.tolist() == [len(s[1]) for s in single] and counts.sum() > 0
    assert np.array_equal(out, np.concatenate([s[1] for s in single])) and np.array_equal(out_gid, np.repeat(gid[pick], counts))
    assert all((np.diff(s[1]) > 0).all() for s in single)
    far = codes[pick] ^ 63                                   # the opposite cells of level 2: most fail their own test
    ok = bf.decide(cases.to_point(far), gid[pick], 2, data[0], *prep, ISO)
    assert not ok.all()
    assert bf.subtree(data[0], *prep, ISO, far, gid[pick], 2, 2, 1)[0].tolist() == [1] * 5
    assert bf.subtree(data[0], *prep, ISO, far, gid[pick], 2, 2, 0)[0].tolist() == ok.astype(int).tolist()


# ------------------------------------------------------------------------------------------------- the oracle against geometry
SAMPLES = 4000
NEAR_FACE = 1e-3           # voxels: samples this close to a cell face are not judged (either side may round away)
DROPPED_CAP = 0.02


def anchor_inputs(name):
    if name == 'wide':
        return random_gaussians(12, 5, 4, voxels=(0.05, 6.0)), 5, ISO, TOL
    return cases.case(name)


@pytest.mark.parametrize('name', ['deep-12', 'needles-5-30', 'straddle', 'wide'])
def test_oracle_holds_every_voxel_the_iso_surface_passes_through(name):
    """an anchor that shares nothing with the reference's tests: the quadric x^T A x = iso of every splat in float64 from the
    clamped scales and the quaternion as given (M = S^-1 R, A = M^T M), sampled through its eigen-decomposition"""
    (means, scales, rots, _), level, iso, tol = anchor_inputs(name)
    points, gid, _, cov = bf.gs_to_spc(means, scales, rots, iso, tol, level)
    vs = 2.0 / (1 << level)
    iso64 = float(np.float32(iso))
    rng = np.random.RandomState(7)
    judged = dropped = 0
    for g in range(len(means)):
        s = np.maximum(scales[g], np.float32(tol) * np.float32(vs)).astype(np.float64)
        r, x, y, z = rots[g].astype(np.float64)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)],
                      [2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)],
                      [2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)]])
        M = np.diag(1.0 / s) @ R
        A = M.T @ M
        got = cov[g].astype(np.float64)
        want = np.array([A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2]])
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()          # relative to the matrix: small entries are sums
        lam, V = np.linalg.eigh(A)
        u = rng.normal(size=(SAMPLES, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        surface = means[g].astype(np.float64) + (u * np.sqrt(iso64 / lam)) @ V.T
        f = (surface[np.all(np.abs(surface) < 1.0, 1)] + 1.0) / vs            # in voxels
        clear = np.all(np.abs(f - np.round(f)) > NEAR_FACE, 1)
        dropped += int((~clear).sum())
        judged += len(f)
        cells = np.unique(np.floor(f[clear]).astype(np.int64), axis=0)
        paired = {tuple(p) for p in points[gid == g].tolist()}
        missing = [tuple(c) for c in cells.tolist() if tuple(c) not in paired]
        assert not missing, f'splat {g}: the surface passes through {missing[:5]}, unpaired'
    share = dropped / max(judged, 1)
    print(f'{name}: {judged} samples inside the cube, {dropped} within {NEAR_FACE} voxel of a face ({100 * share:.2f} %)')
    assert judged > SAMPLES and share <= DROPPED_CAP
