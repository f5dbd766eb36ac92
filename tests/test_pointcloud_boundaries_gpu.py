"""unbatched_pointcloud_to_spc through the HIP path (csrc/pointcloud.hip) at the chunk, run and lane-group edges of its segmented
mean: the layouts of tests/pointcloud_boundary_cases.py and the checks of tests/test_pointcloud_boundaries_cpu.py on CUDA tensors.
Octrees and integer means are compared with torch.equal, float means with the oracle's derived bound
    |got - m| <= (gamma_n sum|f_i| / n + u_out |m|) (1 + 2^-10) + s_out / 2
of which every test prints the share used and the last test the worst share per dtype.  The result rows are torch.empty and the
`first` / `last` pieces live in scratch that the allocator hands back from earlier calls, so a run that no boundary finishes or a
piece that is read without being written shows as a value of an earlier call: (c) poisons both on purpose.

(a) every layout in float32, the lane-group layouts in float64, one in half, strided inputs, integer ties, int64 beyond 32 bits;
(b) a NaN stays in its row and column, every other entry keeps its bits;
(c) recycled result memory, a stale workspace, run-to-run equality;
(d) every level 1 - 15 (every pass count of the sort), coordinates on and next to the cell borders;
(e) a sparse voxel grid of more than 2^31 voxels."""
import pytest
import torch

import pointcloud_boundary_cases as cases
from test_pointcloud_boundaries_cpu import (BORDERS, INT64_LAYOUTS, INT_TIE_DTYPES, LANE_NAMES, SWEEP, check_borders, check_int64,
                                            check_layout_case, check_sweep, check_ties, check_voxelgrid_beyond_int32)
from test_pointcloud_cpu import check_spc, conv

pytestmark = pytest.mark.gpu

C = cases.C
BITS = {torch.float16: torch.int16, torch.float32: torch.int32, torch.float64: torch.int64}


def bits(x):
    return x.view(BITS[x.dtype]) if x.dtype in BITS else x


def mean_on_gpu(pts, feats):
    spc = conv().unbatched_pointcloud_to_spc(pts.cuda(), cases.LEVEL, feats.cuda())
    return spc.octrees, spc.features


def poison_free_blocks():
    """fill the allocator's free blocks with -1 bits (NaN as floats) and give them back"""
    junk = [torch.full((n,), -1, dtype=torch.int32, device='cuda') for n in (1024, 16384, 131072, 1048576) for _ in range(4)]
    del junk


# ---- (a) the layouts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', cases.NAMES)
def test_layout_float32(name):
    check_layout_case(name, 'cuda')


@pytest.mark.parametrize('name', LANE_NAMES + ['first_runs_last'])
def test_layout_float64(name):
    """u_out = 0: the bound is the pure summation bound"""
    check_layout_case(name, 'cuda', torch.float64)


def test_layout_float16():
    check_layout_case('first_runs_last', 'cuda', torch.float16)


@pytest.mark.parametrize('name', ['mid_start_mid_end', 'two_crossing'])
def test_layout_strided(name):
    check_layout_case(name, 'cuda', strided=True)


@pytest.mark.parametrize('dtype', INT_TIE_DTYPES, ids=str)
def test_integer_ties(dtype):
    check_ties(dtype, 'cuda')


@pytest.mark.parametrize('name', INT64_LAYOUTS)
def test_int64_beyond_32_bits(name):
    check_int64(name, 'cuda')


# ---- (b) a NaN stays where it is -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize('name, r, chunk, d', [('first_runs_last', 3, 3, 1), ('lanes_d8_m9', 1, 4, 7)])
def test_a_nan_stays_in_its_row_and_column(name, r, chunk, d, dtype):
    """one NaN feature at a member of run r that lies in an interior chunk of the run: entry (r, d) is NaN, every other entry has
    the bits of the call without it (the order of the sum is fixed: two calls give the same bits)"""
    pts, feats, orc = cases.case(name, dtype)
    desc = cases.check_layout(name, orc)
    run = desc.runs[r]
    assert run.k0 < chunk < run.k1 and 0 <= d < feats.shape[1]
    if desc.G > 1:
        assert (chunk - run.k0 - 1) % desc.G != 0               # a piece that a partial sum other than 0 adds
    position = chunk * C + 17
    row = orc.members[r][position - run.s]                      # the stable sort keeps the members in ascending input index
    octree, clean = mean_on_gpu(pts, feats)
    dirty = feats.clone()
    dirty[row, d] = float('nan')
    octree_dirty, got = mean_on_gpu(pts, dirty)
    assert torch.equal(octree, octree_dirty) and not torch.isnan(clean).any()
    assert bool(torch.isnan(got[r, d]))
    same = torch.ones_like(got, dtype=torch.bool)
    same[r, d] = False
    assert torch.equal(bits(got)[same], bits(clean)[same]) and int(torch.isnan(got).sum()) == 1


# ---- (c) leaks across calls ------------------------------------------------------------------------------------------------------------
LEAK_CASES = [('first_runs_last', torch.float32), ('lanes_d8_m9', torch.float64), ('runs_block_edge', torch.float32),
              ('wide_first_runs_last_d129', torch.float32), ('lanes_d1_m65', torch.float64)]


@pytest.mark.parametrize('name, dtype', LEAK_CASES, ids=str)
def test_results_do_not_depend_on_recycled_memory(name, dtype):
    """the result rows and the scratch are torch.empty: with the allocator's free blocks full of NaN bits before the call the result
    stays within the bound and keeps the bits of the unpoisoned call"""
    clean = check_layout_case(name, 'cuda', dtype)
    for _ in range(2):
        poison_free_blocks()
        again = check_layout_case(name, 'cuda', dtype)
        assert torch.equal(clean.octrees, again.octrees) and torch.equal(bits(clean.features), bits(again.features))


@pytest.mark.parametrize('name, dtype', LEAK_CASES, ids=str)
def test_a_stale_workspace_is_not_read(name, dtype):
    """a call with the same n, D and layout but features times 2^20 leaves its `first` / `last` pieces and its rows in the blocks
    that the next call gets: an entry read without being written in this call is off by a factor of 2^20"""
    pts, feats, orc = cases.case(name, dtype)
    mean_on_gpu(pts, feats * 2.0 ** 20)
    after_same_size = check_layout_case(name, 'cuda', dtype)
    check_spc('random_2049', 3, 'cuda', D=5)                    # an unrelated call of a different size
    after_other_size = check_layout_case(name, 'cuda', dtype)
    assert torch.equal(bits(after_same_size.features), bits(after_other_size.features))
    assert torch.equal(after_same_size.octrees, after_other_size.octrees)


@pytest.mark.parametrize('name, dtype', [('ownership', torch.float32), ('lanes_d3_m33', torch.float64), ('two_crossing', torch.float16)],
                         ids=str)
def test_two_runs_give_the_same_bits(name, dtype):
    first = check_layout_case(name, 'cuda', dtype)
    second = check_layout_case(name, 'cuda', dtype)
    assert torch.equal(first.octrees, second.octrees) and torch.equal(bits(first.features), bits(second.features))


# ---- (d) keys and sort -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('level, dtype', SWEEP, ids=str)
def test_every_level(level, dtype):
    """1 - 6 passes of the pair sort over 3 * level key bits, with two cells that differ in the most significant key bit only"""
    assert 1 <= check_sweep(level, dtype, 'cuda') <= 6


@pytest.mark.parametrize('level, dtype', BORDERS, ids=str)
def test_cell_borders(level, dtype):
    check_borders(level, dtype, 'cuda')


# ---- (e) a voxel grid of more than 2^31 voxels -----------------------------------------------------------------------------------------
def test_voxelgrid_beyond_int32():
    check_voxelgrid_beyond_int32('cuda')


def test_worst_shares():
    """(last: prints the worst share of the bound per dtype that the tests above recorded)"""
    cases.report('cuda')
    assert all(share <= 1.0 for (device, _), (share, _) in cases.WORST.items() if device == 'cuda')
