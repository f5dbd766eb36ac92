"""ops.conversions.gs_to_voxelgrid through the HIP path (csrc/gs_to_spc.hip, spc_stage.h with GsPrim, sort_scan.h) at the boundaries of its
pipeline, against the numpy oracle of tests/gs_to_spc_bruteforce.py.  Integer results and cov3d_invs are compared bit for bit, the
integral against the bound 2^-23 |w| + 2^-149 of tests/test_gs_to_spc_cpu.py.

(a) the whole operator on the cases of tests/gs_to_spc_boundary_cases.py: levels 8 - 15, needles, splats larger than the cube and
    across its faces, exact ties, degenerate quaternions / scales / means, iso and tol varied;
(b) one stage through the C ABI (prepare, stage_count, stage_emit) on synthetic proposal lists against ``subtree``;
(c) the spans and levels a stage refuses before any launch;
(d) kamd_gs_to_spc_finish on synthetic pair lists: 0 - 6 sort passes, pair counts around the sort's block, packs over blocks;
(e) the integral on pair lists built by hand: 31 / 32 / 33 pairs, steps that divide among the eight lanes or not, long columns,
    levels 11 and 15, values that are float denormals and exact zeros.
Every test asserts on the reference side that its input has the property it aims at.  No test gives a kernel a span above
kamd_gs_to_spc_stage_levels(), a Gaussian id outside the tables or a Morton code beyond the level."""
import functools

import numpy as np
import pytest
import torch

import gs_to_spc_bruteforce as bf
import gs_to_spc_boundary_cases as cases
from test_gs_to_spc_boundaries_cpu import check_integral_with_nan
from test_gs_to_spc_cpu import (C, ISO, TOL, check_against_oracle, check_integral, check_merged, kal, random_gaussians, t,
                                ulp_share)

pytestmark = pytest.mark.gpu

GROUPS_PER_WAVE = 8        # proposals per wavefront of spc_stage_kernel (eight lanes each)
PROPOSALS_PER_BLOCK = 32   # proposals per 256-thread block of spc_stage_kernel; pairs per block of gs_integrate_kernel
SCAN_BLOCK = 1024          # entries per block of ss_scan
SORT_BLOCK = 2048          # pairs per block of the radix sort (SS_SORT_BLOCK)
STAGE_LEVELS = 3
GS_PREP = 15               # floats per Gaussian of the prepared table: AABB min, AABB max, three contact points

STAGE_COUNTS = [1, GROUPS_PER_WAVE - 1, GROUPS_PER_WAVE, GROUPS_PER_WAVE + 1, PROPOSALS_PER_BLOCK - 1, PROPOSALS_PER_BLOCK,
                PROPOSALS_PER_BLOCK + 1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1]
PAIR_COUNTS = [1, SORT_BLOCK - 1, SORT_BLOCK, SORT_BLOCK + 1, 2 * SORT_BLOCK + 1]
SENTINEL = -7
PAD = 64                   # sentinel entries behind every output


def api():
    from kaolin_amd import _lib
    return _lib, _lib.load()


def cuda(a, dtype=None):
    return torch.as_tensor(np.array(a), dtype=dtype).cuda()


def filled(n, dtype=torch.long):
    return torch.full((n + PAD,), SENTINEL, dtype=dtype, device='cuda')


def untouched(x, n):
    return bool((x[n:] == SENTINEL).all())


def test_the_counts_are_the_ones_the_kernels_split_at():
    assert STAGE_COUNTS == [1, 7, 8, 9, 31, 32, 33, 1023, 1024, 1025] and PAIR_COUNTS == [1, 2047, 2048, 2049, 4097]
    _, lib = api()
    assert lib.kamd_gs_to_spc_stage_levels() == STAGE_LEVELS
    assert lib.kamd_gs_to_spc_prepare_workspace(7) == 7 * GS_PREP * 4


# ---- (a) the whole operator --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', cases.NAMES)
def test_case_equals_oracle(name):
    data, level, iso, tol = cases.case(name)
    want, _ = check_against_oracle(data, level, 'cuda', iso, tol)
    assert len(want[0]) == len(cases.oracle_pairs(name)[0]) > 0


@pytest.mark.parametrize('name', cases.FINITE)
def test_case_integral_within_one_ulp(name):
    data, level, _, _ = cases.case(name)
    check_integral(data, level, cases.STEP, 'cuda', pairs=cases.oracle_pairs(name))


@pytest.mark.parametrize('name', cases.NOT_FINITE)
def test_case_integral_is_nan_where_the_oracle_is(name):
    check_integral_with_nan(name, 'cuda')


@pytest.mark.parametrize('name', ['straddle', 'needles-5-30', 'extreme_cells-11'])
def test_case_merged_opacities(name):
    data, level, _, _ = cases.case(name)
    voxels, merged = kal.ops.conversions.gs_to_voxelgrid(*(t(a, 'cuda') for a in data), level)
    check_merged(data, level, voxels, merged)


@pytest.mark.parametrize('name', ['deep-15', 'needles-7-100'])
def test_hip_equals_cpu_and_two_runs_give_the_same_bits(name):
    data, level, iso, tol = cases.case(name)
    host = [t(a) for a in data]
    dev = [a.cuda() for a in host]
    cpu = C.gs_to_spc_cuda(*host[:3], iso, tol, level)

    def run():
        out = C.gs_to_spc_cuda(*dev[:3], iso, tol, level)
        return list(out) + [C.integrate_gs_cuda(out[0], out[1], dev[0], out[3], dev[3], level, cases.STEP)]

    first, second = run(), run()
    assert first[0].size(0) == len(cases.oracle_pairs(name)[0])
    for a, b in zip(cpu, first):
        assert b.is_cuda and not a.is_cuda and torch.equal(a, b.cpu())
    for a, b in zip(first, second):
        bits = (lambda x: x.view(torch.int32)) if a.dtype == torch.float32 else (lambda x: x)
        assert a.dtype == b.dtype and torch.equal(bits(a), bits(b))
    for a, b in zip(host, dev):
        assert torch.equal(a, b.cpu())                                       # the inputs are only read


# ---- (b) one stage through the C ABI ---------------------------------------------------------------------------------------------
STAGE_BASE = (1000, 2000, 3000)   # level-12 cell whose 2 x 2 x 2 neighbourhood holds the proposals of the stages from level 12


def stage_gaussians():
    """0 a large splat through the neighbourhood (full subtrees), 1 a small one elsewhere in the cube (fails at once from level 12,
    a sparse subtree from level 0), 2 inside one level-15 voxel, 3 a few level-15 voxels wide, 4 a NaN mean, 5 outside the cube
    -> (means, scales, rots)"""
    size = 2.0 / (1 << 12)
    p = (np.array(STAGE_BASE, dtype=np.float64) + 1.0) * size - 1.0          # the corner the eight cells share
    s15 = size / 8.0
    r = 1.0 / np.sqrt(np.float64(np.float32(ISO)))                           # scale of an extent of 1
    means = np.stack([p + size * np.array([0.05, -0.1, 0.08]),
                      np.array([0.33, 0.32, -0.5]),
                      p + s15 * np.array([0.5, 0.5, 0.5]),
                      p + s15 * np.array([0.3, -0.4, 0.2]),
                      np.array([np.nan, np.nan, np.nan]),
                      p + 5.0])
    scales = np.stack([size * r * np.array([0.95, 0.85, 0.75]),
                       np.array([0.02, 0.03, 0.025]),
                       np.full(3, 1e-7),
                       s15 * r * np.array([3.0, 2.0, 1.3]),
                       size * r * np.array([0.9, 0.9, 0.9]),
                       size * r * np.array([0.95, 0.85, 0.75])])
    rots = random_gaussians(6, 1, 61)[2]
    return means.astype(np.float32), scales.astype(np.float32), rots


def stage_target(level_from):
    """the level of the conversion the stage belongs to: prepare clamps by its voxel"""
    return 15 if level_from else 3


@functools.lru_cache(maxsize=None)
def stage_prepared(level_from):
    means, scales, rots = stage_gaussians()
    return bf.prepare(means, scales, rots, ISO, TOL, stage_target(level_from))


@functools.lru_cache(maxsize=None)
def stage_pool(level_from, span, tested):
    """every (voxel, Gaussian) of the pool with its reference subtree, computed once
    -> (codes, Gaussians, counts, [emitted codes of every pool entry])"""
    means = stage_gaussians()[0]
    if level_from == 0:
        voxels = np.zeros(1, np.int64)
    else:
        b = np.array(STAGE_BASE)
        voxels = cases.to_morton(np.array([b + [i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)]))
    m = np.repeat(voxels, len(means))
    g = np.tile(np.arange(len(means), dtype=np.int64), len(voxels))
    counts, out, _ = bf.subtree(means, *stage_prepared(level_from), ISO, m, g, level_from, level_from + span, tested)
    return m, g, counts, np.split(out, np.cumsum(counts)[:-1])


def prepare_on_gpu(level_from):
    """kamd_gs_to_spc_prepare on the pool, compared with the oracle's -> (means, cov3d_invs, prepared) on the GPU"""
    _lib, lib = api()
    means, scales, rots = stage_gaussians()
    G = len(means)
    dm, ds, dr = cuda(means), cuda(scales), cuda(rots)
    cov = filled(6 * G, torch.float32)
    prep = filled(GS_PREP * G, torch.float32)
    assert lib.kamd_gs_to_spc_prepare_workspace(G) == GS_PREP * G * 4
    status = lib.kamd_gs_to_spc_prepare(_lib.stream_ptr(dm.device), G, _lib.ptr(dm), _lib.ptr(ds), _lib.ptr(dr), ISO, TOL,
                                        stage_target(level_from), _lib.ptr(cov), _lib.ptr(prep))
    assert status == 0
    want_cov, ab0, ab1, cp = stage_prepared(level_from)
    want_prep = np.concatenate([ab0, ab1, cp.reshape(G, 9)], 1)
    assert np.array_equal(cov[:6 * G].cpu().numpy().reshape(G, 6), want_cov, equal_nan=True)
    assert np.array_equal(prep[:GS_PREP * G].cpu().numpy().reshape(G, GS_PREP), want_prep, equal_nan=True)
    assert untouched(cov, 6 * G) and untouched(prep, GS_PREP * G)
    assert np.array_equal(dm.cpu().numpy(), means, equal_nan=True) and np.array_equal(ds.cpu().numpy(), scales)
    return dm, cov, prep


@pytest.mark.parametrize('level_from, tested', [(0, 0), (0, 1), (12, 0), (12, 1)])
@pytest.mark.parametrize('span', [0, 1, 2, 3])
@pytest.mark.parametrize('n', STAGE_COUNTS)
def test_one_stage_against_subtree(n, span, level_from, tested):
    _lib, lib = api()
    means, cov, prep = prepare_on_gpu(level_from)
    G = means.size(0)
    sp = _lib.stream_ptr(means.device)
    assert span <= STAGE_LEVELS
    pm, pg, pc, pout = stage_pool(level_from, span, tested)
    assert pg.min() >= 0 and pg.max() < G and pm.max() < 8 ** level_from
    if span == 3 and level_from:
        assert pc.max() >= 64                                            # a full layer of the subtree next to ...
    if span >= 1:
        assert (pc == 0).any() and (pc > 1).any()                        # ... proposals that fail at once or below the first level
    if span == 0:
        assert set(pc.tolist()) == ({1} if tested else {0, 1})
    pick = np.random.RandomState(1000 * n + span).permutation(np.resize(np.arange(len(pm)), n))   # repeated and shuffled
    assert len(pick) == n
    want_counts = pc[pick]
    want_offsets = np.concatenate([[0], np.cumsum(want_counts)])
    want_codes = np.concatenate([pout[i] for i in pick])
    want_ids = np.repeat(pg[pick], want_counts)
    total = int(want_offsets[-1])
    morton, gid = cuda(pm[pick]), cuda(pg[pick])
    counts, offsets = filled(n, torch.int32), filled(n + 1)
    scan_ws = torch.empty(lib.kamd_gs_to_spc_scan_workspace(n), dtype=torch.uint8, device='cuda')
    head = (sp, n, G, _lib.ptr(means), _lib.ptr(cov), _lib.ptr(prep), ISO, _lib.ptr(morton), _lib.ptr(gid), level_from,
            level_from + span, tested)
    assert lib.kamd_gs_to_spc_stage_count(*head, _lib.ptr(counts), _lib.ptr(offsets), _lib.ptr(scan_ws)) == 0
    assert np.array_equal(counts[:n].cpu().numpy(), want_counts)
    assert np.array_equal(offsets[:n + 1].cpu().numpy(), want_offsets)
    assert untouched(counts, n) and untouched(offsets, n + 1)
    morton_out, gid_out = filled(total), filled(total)
    assert lib.kamd_gs_to_spc_stage_emit(*head, _lib.ptr(offsets), total, _lib.ptr(morton_out), _lib.ptr(gid_out)) == 0
    assert np.array_equal(morton_out[:total].cpu().numpy(), want_codes)
    assert np.array_equal(gid_out[:total].cpu().numpy(), want_ids)
    assert untouched(morton_out, total) and untouched(gid_out, total)
    assert np.array_equal(morton.cpu().numpy(), pm[pick]) and np.array_equal(gid.cpu().numpy(), pg[pick])


# ---- (c) refusals before any launch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('level_from, level_to', [(0, 4), (11, 15), (0, 15), (3, 2), (13, 16), (-1, 2)])
def test_a_stage_rejects_what_the_walker_cannot_hold(level_from, level_to):
    """the walker keeps 8 bits per depth in one 32-bit word: spans above kamd_gs_to_spc_stage_levels(), a negative span and levels
    outside [0, 15] return an error before any launch and leave the outputs alone"""
    _lib, lib = api()
    assert level_from < 0 or level_to < level_from or level_to > 15 or level_to - level_from > lib.kamd_gs_to_spc_stage_levels()
    n = GROUPS_PER_WAVE + 1
    means, cov, prep = prepare_on_gpu(12)
    G = means.size(0)
    sp = _lib.stream_ptr(means.device)
    morton, gid = torch.zeros(n, dtype=torch.long, device='cuda'), torch.zeros(n, dtype=torch.long, device='cuda')
    counts, offsets = filled(n, torch.int32), filled(n + 1)
    scan_ws = torch.empty(lib.kamd_gs_to_spc_scan_workspace(n), dtype=torch.uint8, device='cuda')
    for tested in (0, 1):
        head = (sp, n, G, _lib.ptr(means), _lib.ptr(cov), _lib.ptr(prep), ISO, _lib.ptr(morton), _lib.ptr(gid), level_from, level_to,
                tested)
        assert lib.kamd_gs_to_spc_stage_count(*head, _lib.ptr(counts), _lib.ptr(offsets), _lib.ptr(scan_ws)) != 0
        given = torch.arange(n + 1, dtype=torch.long, device='cuda')         # one slot per proposal: `total` > 0 reaches the check
        morton_out, gid_out = filled(n), filled(n)
        assert lib.kamd_gs_to_spc_stage_emit(*head, _lib.ptr(given), n, _lib.ptr(morton_out), _lib.ptr(gid_out)) != 0
        torch.cuda.synchronize()
        assert untouched(counts, 0) and untouched(offsets, 0) and untouched(morton_out, 0) and untouched(gid_out, 0)


# ---- (d) finish on synthetic pair lists ------------------------------------------------------------------------------------------
SORT_PASSES = {0: 0, 1: 1, 3: 2, 6: 3, 11: 5, 15: 6}       # level -> passes of eight bits over its 3 * level key bits


def pair_list(n, level, seed):
    """n pairs over about 20 distinct codes of `level` (0 and 8^level - 1 among them) in random order, so every pack is spread over
    all sort blocks of the input; ids: about 50 distinct non-negative int64 values up to 2^62, with repeats"""
    rs = np.random.RandomState(seed)
    space = 8 ** level
    codes = np.unique(np.concatenate([[0, space - 1], rs.randint(0, space, 18, dtype=np.int64)]))
    ids = rs.randint(0, 2 ** 62, 50, dtype=np.int64)
    return codes[rs.randint(0, len(codes), n)], ids[rs.randint(0, len(ids), n)]


def finish(morton, ids, level, shrink=0):
    """kamd_gs_to_spc_finish on the pairs -> (status, points, ids, boundary) padded with sentinels"""
    _lib, lib = api()
    n = len(morton)
    m, g = cuda(morton), cuda(ids)
    nbytes = lib.kamd_gs_to_spc_finish_workspace(n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    points, ids_out, boundary = filled(3 * n, torch.int16), filled(n), filled(n, torch.int8)
    status = lib.kamd_gs_to_spc_finish(_lib.stream_ptr(m.device), n, level, _lib.ptr(m), _lib.ptr(g), _lib.ptr(ws), nbytes - shrink,
                                       _lib.ptr(points), _lib.ptr(ids_out), _lib.ptr(boundary))
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy(), morton) and np.array_equal(g.cpu().numpy(), ids)     # the inputs are only read
    return status, points, ids_out, boundary


@pytest.mark.parametrize('level', list(SORT_PASSES))
@pytest.mark.parametrize('n', PAIR_COUNTS)
def test_finish_pair_counts_around_the_sort_block(n, level):
    assert (3 * level + 7) // 8 == SORT_PASSES[level]
    morton, ids = pair_list(n, level, 100 * level + n)
    assert len(morton) == n and morton.min() >= 0 and morton.max() < 8 ** level and ids.min() >= 0
    order = np.argsort(morton, kind='stable')
    sm = morton[order]
    heads = np.ones(n, bool)
    heads[1:] = sm[1:] != sm[:-1]
    if n > SORT_BLOCK:
        assert heads.sum() <= 20
        hot = np.flatnonzero(morton == sm[SORT_BLOCK])                       # the pack that lies over position 2048 once sorted ...
        if n > 2 * SORT_BLOCK:
            assert hot.min() < SORT_BLOCK <= hot.max()                       # ... comes from more than one block of the input
        assert (np.diff(ids[order])[~heads[1:]] < 0).any()                   # input order inside a pack is not id order
    status, points, ids_out, boundary = finish(morton, ids, level)
    assert status == 0
    assert np.array_equal(points[:3 * n].cpu().numpy().reshape(n, 3), cases.to_point(sm).astype(np.int16))
    assert np.array_equal(ids_out[:n].cpu().numpy(), ids[order])
    assert np.array_equal(boundary[:n].cpu().numpy().astype(bool), heads) and set(boundary[:n].tolist()) <= {0, 1}
    assert untouched(points, 3 * n) and untouched(ids_out, n) and untouched(boundary, n)
    if level == 15 and n > 1:
        assert int(sm.max()) >> 44 == 1 and points[:3 * n].max().item() == 32767


@pytest.mark.parametrize('n', [1, SORT_BLOCK + 1])
def test_finish_refuses_a_workspace_one_byte_short(n):
    morton, ids = pair_list(n, 6, n)
    status, points, ids_out, boundary = finish(morton, ids, 6, shrink=1)
    assert status != 0
    assert untouched(points, 0) and untouched(ids_out, 0) and untouched(boundary, 0)


# ---- (e) the integral on pair lists built by hand --------------------------------------------------------------------------------
INTEGRAL_PAIRS = 33
DENORMAL, ZERO = slice(24, 29), slice(29, 33)              # positions of the tail pairs in the list


@functools.lru_cache(maxsize=None)
def hand_pairs(level, step):
    """33 (voxel, Gaussian) pairs around eight splats of about one voxel near the centre of the grid: 24 within two voxels of their
    mean, five at 14 voxels (-q / 2 in [-110, -88]: opacity times the mean is a float denormal) and four at 41 voxels (below
    -800: exp gives 0 in double) -> (points, gaus_id, means, cov3d_invs, opacities, the oracle's float64 integral), read-only"""
    rs = np.random.RandomState(level)
    G = 8
    vs = 2.0 / (1 << level)
    cell = rs.randint((1 << level) // 2 - 100, (1 << level) // 2 + 100, (G, 3))
    means = (-1.0 + (cell + rs.uniform(0.2, 0.8, (G, 3))) * vs).astype(np.float32)
    scales = np.full((G, 3), vs, np.float32)
    rots = np.tile(np.array([[1, 0, 0, 0]], np.float32), (G, 1))
    opacities = np.linspace(0.35, 0.95, G).astype(np.float32)
    cov = bf.prepare(means, scales, rots, ISO, TOL, level)[0]
    gid = rs.randint(0, G, INTEGRAL_PAIRS).astype(np.int64)
    offset = rs.randint(-2, 3, (INTEGRAL_PAIRS, 3))
    offset[DENORMAL] = [[14, 0, 0], [0, -14, 0], [0, 0, 14], [-14, 1, 0], [10, 10, 0]]
    offset[ZERO] = [[41, 0, 0], [0, -41, 0], [29, 29, 0], [0, 30, -30]]
    points = (cell[gid] + offset).astype(np.int16)
    w = bf.integrate_gs(points, gid, means, cov, opacities, level, step)
    return cases.frozen([points, gid, means, cov, opacities, w])


@pytest.mark.parametrize('level', [11, 15])
@pytest.mark.parametrize('step', [1, 3, 8, 9, 33, 64])
def test_integral_on_hand_built_pairs(step, level):
    """step 8: the 64 columns divide exactly among the eight lanes; 9: one lane gets an 11th column; 1 and 3: fewer columns than lanes or
    one lane with two; 33 and 64: long columns.  31 / 32 / 33 pairs: around the 32 pairs of a block"""
    points, gid, means, cov, opacities, w = hand_pairs(level, step)
    assert points.min() >= 0 and points.max() < (1 << level) and gid.max() < len(means)
    assert (step * step) % 8 == 0 if step in (8, 64) else (step * step) % 8 == 1
    assert ((w[DENORMAL] > 0) & (w[DENORMAL] < 2.0 ** -126)).all() and (w[ZERO] == 0).all()
    assert (w[:24] > 2.0 ** -126).all()
    dev = [t(a, 'cuda') for a in (means, cov, opacities)]
    for n in (PROPOSALS_PER_BLOCK - 1, PROPOSALS_PER_BLOCK, PROPOSALS_PER_BLOCK + 1):
        p, g = filled(3 * n, torch.int16), filled(n)
        p[:3 * n] = t(points[:n], 'cuda').reshape(-1)
        g[:n] = t(gid[:n], 'cuda')
        got = C.integrate_gs_cuda(p[:3 * n].view(n, 3), g[:n], *dev, level, step)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n,)
        got = got.cpu().numpy()
        share = ulp_share(got, w[:n])
        print(f'integrate_gs cuda level {level} step {step}: {n} hand-built pairs, worst share of the bound {share.max():.3f}, '
              f'among the denormals {share[DENORMAL].max():.3f}')
        assert share.max() <= 1.0
        assert (got[ZERO] == 0).all() and not np.signbit(got[ZERO]).any()
        assert np.array_equal(p[:3 * n].cpu().numpy().reshape(n, 3), points[:n]) and np.array_equal(g[:n].cpu().numpy(), gid[:n])
