"""unbatched_pointcloud_to_spc at the chunk, run and lane-group edges of its segmented mean, without a GPU: every layout of
tests/pointcloud_boundary_cases.py is shown to be what it claims (through ``describe``, the model of the bookkeeping of
csrc/pointcloud.hip, and through the oracle's member lists), and the torch formulation is compared with the oracle on them -- the
octree and the integer means with torch.equal, the float means against ``Oracle.float_bound`` -- so that the cases and the oracle
agree before any kernel runs.  The helpers take a device: tests/test_pointcloud_boundaries_gpu.py runs them on CUDA tensors."""
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import pointcloud_bruteforce as bf
import pointcloud_boundary_cases as cases
from test_pointcloud_cpu import check_spc_case, conv

C = cases.C
SMALL = [name for name in cases.NAMES if name not in cases.LARGEST]
LANE_NAMES = [name for name, _, _, _ in cases.LANE_CASES]
SMALL_LANE_NAMES = [name for name in LANE_NAMES if name not in cases.LARGEST]
INT_TIE_DTYPES = list(cases.TIE_VALUES)
NP_FLOAT = {torch.float16: np.float16, torch.float32: np.float32, torch.float64: np.float64}
SWEEP = [(level, torch.float32) for level in range(1, 16)] + [(level, torch.float16) for level in range(1, 12)]
BORDERS = [(level, dtype) for dtype in (torch.float32, torch.float64) for level in (1, 8, 15)] + [(1, torch.float16), (11, torch.float16)]


# ---- helpers shared with the GPU suite -----------------------------------------------------------------------------------------------
def check_layout_case(name, device, dtype=torch.float32, strided=False, D=None, scale=1):
    """the layout is what it claims, its runs are the oracle's cells, and the operator agrees with the oracle -> the Spc"""
    case = cases.case(name, dtype, D, scale)
    cases.check_layout(name, case[2])
    spc, share = check_spc_case(case, f'layout {name}', cases.LEVEL, device, strided)
    cases.record(device, dtype, name, share)
    return spc


def check_ties(dtype, device):
    pts, feats, orc, want = cases.tie_case(dtype)
    d = cases.describe(cases.TIES, 2)
    assert [len(m) for m in orc.members] == cases.TIES
    assert d.runs[cases.TIE_CROSSING].owner == 1 and d.kinds == ['last', 'first'] and max(cases.TIES[:10]) <= 4
    not_a_tie = cases.NOT_A_TIE.get(dtype, (8, 9))
    for r in want:                                              # the exact means really are x.5
        assert (orc.mean[r][0].denominator == 2) == (r not in not_a_tie), (r, orc.mean[r][0])
    assert cases.TIES[7] == 4 and orc.mean[7][0] * 4 == 2       # a run of four that sums to 2
    expected = orc.integer_features(feats.numpy().dtype)
    assert [int(expected[r, 0]) for r in sorted(want)] == [want[r] for r in sorted(want)]       # the oracle and the hand-written means
    spc, _ = check_spc_case((pts, feats, orc), f'ties {dtype}', cases.LEVEL, device)
    assert [int(spc.features[r, 0]) for r in sorted(want)] == [want[r] for r in sorted(want)]


INT64_SCALE = 2 ** 40
INT64_LAYOUTS = ['short_crossing', 'aligned_middle', 'first_runs_last', 'lanes_d8_m7']


def check_int64(name, device):
    """features k 2^40, |k| <= 100: every sum is a multiple of 2^40 below 2^62, exact in double; the quotient is rounded to a double
    (an error of at most half an ulp) before rint, so the case must keep every exact mean further than an ulp from a tie"""
    pts, feats, orc = cases.case(name, torch.int64, None, INT64_SCALE)
    assert feats.dtype == torch.int64 and 2 ** 32 < int(feats.abs().max()) <= 100 * INT64_SCALE and bool((feats % INT64_SCALE == 0).all())
    for row in orc.mean:
        for mean in row:
            ulp = Fraction(2) ** (max(int(abs(mean)).bit_length(), 1) - 53)
            assert abs(mean) < 2 ** 47 and abs(mean - math.floor(mean) - Fraction(1, 2)) > ulp, mean
    for sums, count in zip(orc.abs_sum, map(len, orc.members)):
        assert all(s < 2 ** 62 and s % INT64_SCALE == 0 for s in sums)
    spc = check_layout_case(name, device, torch.int64, scale=INT64_SCALE)
    assert int(spc.features.abs().max()) > 2 ** 32              # the means themselves need more than 32 bits


def check_sweep(level, dtype, device):
    pts, feats, orc = cases.sweep_case(level, dtype)
    q = bf.quantize(np.array(cases.TOP_BIT_PAIR, dtype=NP_FLOAT[dtype]), level).tolist()
    low, high = (bf.morton(x, y, z, level) for x, y, z in q)
    assert high - low == 1 << (3 * level - 1) and low < 1 << (3 * level - 1)     # they differ in the x bit of the top level only
    assert low in orc.codes and high in orc.codes
    check_spc_case((pts, feats, orc), f'sweep {dtype}', level, device)
    return (3 * level + 7) // 8                                 # passes of eight bits over the 3 * level key bits


def check_borders(level, dtype, device):
    pts, _, orc = cases.border_case(level, dtype)
    res = 1 << level
    npdt = NP_FLOAT[dtype]
    borders = np.array([-1.0 + 2.0 * k / res for k in (0, 1, res // 2, res - 1, res)], dtype=npdt)
    assert bf.quantize(borders, level).tolist() == [0, 1, res // 2, res - 1, res - 1]           # a border belongs to the cell above
    below = bf.quantize(np.nextafter(borders, npdt(-np.inf)), level).tolist()
    assert below[0] == 0 and below[4] == res - 1 and (level == 1 or below[1] == 0)
    # just below 0, x + 1 rounds to 1: the point lands in the cell above the border
    assert float(np.nextafter(npdt(0), npdt(-1)) + npdt(1)) == 1.0 and below[2] == res // 2
    vals = set(cases.border_values(level, npdt).tolist())
    assert len(vals) >= 9 and all(set(pts[:, a].tolist()) == vals for a in range(3))
    check_spc_case((pts, None, orc), f'borders {dtype}', level, device)


def check_voxelgrid_beyond_int32(device):
    """R = 1291: R^3 > 2^31, a bit grid of 270 MB on the GPU; sparse only, the dense grid is never allocated"""
    R = 1291
    assert R ** 3 > 2 ** 31 and 0.5 * (R - 1) == 645.0
    pts = torch.tensor([[[0, 0, 0], [1, 1, 1], [0.5, 0.5, 0.5], [1, 0, 0.5]]], dtype=torch.float32, device=device)
    sp = conv().pointclouds_to_voxelgrids(pts, R, origin=torch.zeros((1, 3), device=device), scale=torch.ones(1, device=device),
                                          return_sparse=True)
    want = torch.tensor([[0, 0, 0, 0], [0, 645, 1290, 1290], [0, 645, 0, 1290], [0, 645, 645, 1290]])
    assert (want[1, -1] * R + want[2, -1]) * R + want[3, -1] > 2 ** 31 and (want[1, 2] * R + want[2, 2]) * R + want[3, 2] > 2 ** 31
    assert sp.is_sparse and tuple(sp.shape) == (1, R, R, R) and sp.dtype == torch.float32 and sp.device.type == device
    assert sp.is_coalesced() and sp.indices().dtype == torch.int64
    assert torch.equal(sp.indices().cpu(), want)
    assert torch.equal(sp.values().cpu(), torch.ones(4))


# ---- the layouts are what they claim -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', cases.NAMES)
def test_layout_is_what_it_claims(name):
    lay = cases.LAYOUTS[name]
    assert lay.__doc__ and lay.__doc__ != cases.Layout.__doc__
    pts = cases.points_of(name)
    assert pts.dtype == torch.float64 and torch.equal(pts.float().double(), pts) and float(pts.abs().max()) < 1
    orc = bf.Oracle(pts.float().numpy(), cases.LEVEL)
    d = cases.check_layout(name, orc)
    assert orc.codes == sorted(orc.codes) and len(set(orc.codes)) == len(lay.lengths)
    cell = np.empty(d.n, dtype=np.int64)
    for r, m in enumerate(orc.members):
        cell[m] = r
    assert len(lay.lengths) == 1 or (np.diff(cell) < 0).any()   # the permutation scatters the members: the input is not in cell order
    print(f'{name}: {lay.__doc__}\n    lengths {lay.lengths if len(lay.lengths) < 9 else str(lay.lengths[:3]) + " ..."} n {d.n} chunks '
          f'{"".join(k[0] for k in d.kinds) if d.nchunks < 20 else d.nchunks} D {lay.D} DL {d.DL} G {d.G} crossing '
          f'{[(r, run.k0, run.k1, run.owner, run.pieces) for r, run in enumerate(d.runs) if run.owner][:3]}')


def test_single_chunk_layouts_do_not_launch_the_runs_kernel():
    for name in ('chunk_one_run', 'chunk_127_1', 'chunk_singles'):
        d = cases.check_layout(name)
        assert d.nchunks == 1 and not d.runs_kernel and d.kinds == ['none'] and all(run.owner is None for run in d.runs)
    for name in cases.NAMES[3:]:
        assert cases.check_layout(name).runs_kernel


def test_one_boundary_layouts():
    d = cases.check_layout('tail_129')
    assert d.n == C + 1 and d.kinds == ['last', 'first'] and d.runs[0].pieces[0] == 1 and d.runs[0].on_start
    d = cases.check_layout('ends_on_boundary')
    assert d.runs[0].on_end and d.runs[0].owner is None and (d.runs[1].s, d.runs[1].e) == (C, C + 1) and d.n == C + 1
    d = cases.check_layout('one_each_side')
    assert (d.runs[1].s, d.runs[1].e) == (C - 1, C + 1) and d.runs[1].owner == 1
    d = cases.check_layout('single_127_single')
    assert d.runs[1].on_end and not d.runs[1].on_start and all(run.owner is None for run in d.runs)
    d = cases.check_layout('every_run_a_chunk')
    assert all(run.on_start and run.on_end and run.owner is None for run in d.runs) and d.kinds == ['none'] * 3
    d = cases.check_layout('open_last_run')
    assert d.n == 2 * C and d.runs[1].e == d.n and d.runs[1].on_end and d.runs[1].owner == 1


def test_aligned_and_interior_layouts():
    for name, r in (('aligned_256', 0), ('aligned_384', 0), ('aligned_middle', 1)):
        run = cases.check_layout(name).runs[r]
        assert run.on_start and run.on_end and run.s == run.k0 * C and run.owner == run.k0 + 1     # s == k0 * 128: not `<`
    d = cases.check_layout('aligned_384')
    assert d.kinds[1] == 'first' and d.runs[0].k1 - d.runs[0].k0 == 2                              # a headless interior chunk
    d = cases.check_layout('mid_start_mid_end')
    run = d.runs[1]
    assert not run.on_start and not run.on_end and (run.k0, run.k1) == (0, 3) and d.runs[2].k0 == d.runs[2].k1 == 3
    assert d.runs[2].e == d.n == 4 * C                         # the last chunk: a `first` piece, then a complete run up to n
    d = cases.check_layout('first_runs_last')
    assert d.kinds[1] == 'both' and [run.k0 == run.k1 == 1 for run in d.runs] == [False, True, True, False]
    d = cases.check_layout('two_crossing')
    assert d.kinds[1] == 'both' and d.runs[1].k1 == d.runs[2].k0 == 1 and (d.runs[1].owner, d.runs[2].owner) == (1, 2)
    d = cases.check_layout('short_crossing')
    assert cases.LAYOUTS['short_crossing'].lengths == [120, 16, 120] and d.runs[1].owner == 1 and d.runs[2].owner is None


def test_ownership_layout_crosses_five_boundaries():
    d = cases.check_layout('ownership')
    run = d.runs[1]
    inside = [b for b in range(1, d.nchunks) if run.s < b * C < run.e]
    assert inside == [1, 2, 3, 4, 5] and run.owner == 1 and [run.s < (b - 1) * C for b in inside] == [False] + [True] * 4


@pytest.mark.parametrize('name, D, G, m', cases.LANE_CASES)
def test_lane_layouts_spread_their_pieces(name, D, G, m):
    d = cases.check_layout(name)
    run = d.runs[1]
    assert (d.DL, d.G, d.DL * d.G) == (cases.lanes(D), G, 64) and cases.LAYOUTS[name].D == D
    assert (run.s, run.e, run.k0, run.k1, run.owner) == (37, 37 + 91 + C * m + 5, 0, m + 1, 1) and d.nchunks == m + 2
    q, rem = divmod(m + 1, G)                                   # m + 1 pieces dealt to G partials in turn
    assert run.pieces == [q + 1] * rem + [q] * (G - rem)


def test_lane_layouts_cover_every_width_and_piece_count():
    assert [(D, cases.lanes(D), 64 // cases.lanes(D)) for D, _ in cases.LANE_WIDTHS] == \
        [(1, 1, 64), (2, 2, 32), (3, 4, 16), (8, 8, 8), (32, 32, 2), (64, 64, 1)]
    assert len(cases.LANE_CASES) == 7 + 7 + 7 + 7 + 6 + 4
    for D, G in cases.LANE_WIDTHS:
        seen = set()
        for name, D1, _, m in cases.LANE_CASES:
            if D1 == D:
                seen |= set(cases.describe(cases.LAYOUTS[name].lengths, D).runs[1].pieces)
        assert seen >= ({0, 1, 2, 3} if G > 1 else {1, 2, 3}), (D, seen)
        assert [off for off in (32, 16, 8, 4, 2, 1) if off >= 64 // G] == [32, 16, 8, 4, 2, 1][:int(math.log2(G))]    # butterfly steps
    assert max(sum(cases.LAYOUTS[name].lengths) for name in LANE_NAMES) == sum(cases.LAYOUTS['lanes_d1_m129'].lengths) == 193 + C * 129


def test_wide_layouts_take_several_d0_iterations():
    for D in cases.WIDE:
        for name in (f'wide_lanes_d{D}', f'wide_first_runs_last_d{D}'):
            d = cases.check_layout(name)
            assert (d.DL, d.G) == (64, 1) and cases.LAYOUTS[name].D == D
            iterations = len(range(0, D, d.DL))
            live_in_last = D - (iterations - 1) * d.DL
            assert iterations == (2 if D <= 128 else 3) and live_in_last == {65: 1, 128: 64, 129: 1, 130: 2}[D]
    assert cases.check_layout('wide_lanes_d65').runs[1].pieces == [3]


def test_block_edge_layouts():
    d = cases.check_layout('runs_block_edge')
    assert d.n == 5 * C + 4 and d.runs[1].owner == 5 and cases.runs_kernel_slot(5) == (1, 0) and cases.runs_kernel_slot(4) == (0, 3)
    assert d.runs[0].owner == 1 and d.runs[0].k1 == 4
    d = cases.check_layout('runs_block_last_wave')
    assert [run.owner for run in d.runs] == [1, 4, 5] and (d.runs[1].s, d.runs[1].e) == (4 * C - 1, 4 * C + 1)
    d = cases.check_layout('chunks_block_edge_d64')
    assert d.chunks_per_block == 4 and d.nchunks == 6 and d.runs[1].k0 // 4 == 0 and d.runs[1].k1 // 4 == 1
    d = cases.check_layout('chunks_block_edge_d1')
    assert d.chunks_per_block == 256 and d.n == 32900 and d.nchunks == 258 and len(d.runs) == 328
    last = d.runs[-1]
    assert last.s < 256 * C < last.e and (last.k0, last.k1, last.owner) == (255, 257, 256) and cases.runs_kernel_slot(256) == (63, 3)
    assert last.pieces[:3] == [1, 1, 0] and sum(run.owner is not None for run in d.runs) > 200


# ---- the torch formulation on the layouts --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', SMALL)
def test_layout_float32(name):
    check_layout_case(name, 'cpu')


@pytest.mark.parametrize('name', SMALL_LANE_NAMES + ['first_runs_last'])
def test_layout_float64(name):
    check_layout_case(name, 'cpu', torch.float64)


def test_layout_float16():
    check_layout_case('first_runs_last', 'cpu', torch.float16)


@pytest.mark.parametrize('name', ['mid_start_mid_end', 'two_crossing'])
def test_layout_strided(name):
    check_layout_case(name, 'cpu', strided=True)


@pytest.mark.parametrize('dtype', INT_TIE_DTYPES, ids=str)
def test_integer_ties(dtype):
    check_ties(dtype, 'cpu')


@pytest.mark.parametrize('name', INT64_LAYOUTS)
def test_int64_beyond_32_bits(name):
    check_int64(name, 'cpu')


# ---- keys and sort -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('level, dtype', SWEEP, ids=str)
def test_every_level(level, dtype):
    check_sweep(level, dtype, 'cpu')


def test_the_levels_cross_every_pass_count():
    assert sorted({(3 * level + 7) // 8 for level, _ in SWEEP}) == [1, 2, 3, 4, 5, 6]
    assert [(3 * level + 7) // 8 for level in (1, 2, 3, 8, 11, 15)] == [1, 1, 2, 3, 5, 6]      # the levels of tests/test_pointcloud_gpu.py


@pytest.mark.parametrize('level, dtype', BORDERS, ids=str)
def test_cell_borders(level, dtype):
    check_borders(level, dtype, 'cpu')


def test_voxelgrid_beyond_int32():
    check_voxelgrid_beyond_int32('cpu')


def test_worst_shares():
    """(last: prints what the tests above recorded)"""
    cases.report('cpu')
    assert all(share <= 1.0 for share, _ in cases.WORST.values())
