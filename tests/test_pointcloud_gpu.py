"""kaolin.ops.conversions.pointcloud through the HIP path (csrc/pointcloud.hip): the checks of tests/test_pointcloud_cpu.py on CUDA
tensors, at the smallest shapes at which each stage can go wrong.  Octrees, integer features and voxel grids are compared with
torch.equal; float features with the oracle's derived bound
    |got - m| <= (gamma_n sum|f_i| / n + u_out |m|) (1 + 2^-10) + s_out / 2
(any order of n double additions, one division, one cast), of which every test prints the worst share used."""
import pytest
import torch

from test_pointcloud_cpu import (FLOAT_DTYPES, INT_DTYPES, VOXEL_DTYPES, check_reference_examples, check_spc, check_spc_errors,
                                 check_spc_fields, check_voxel_case, check_voxelgrids_errors, conv, golden_case, golden_cases)

pytestmark = pytest.mark.gpu

CHUNK = 128             # sorted positions per chunk of the mean (csrc/pointcloud.hip PC_CHUNK)
SORT_BLOCK = 2048       # pairs per block of the pair sort (csrc/sort_scan_host.h SS_SORT_BLOCK)


# ---- SPC -------------------------------------------------------------------------------------------------------------------------------
# one_cell_300: a run longer than a wavefront, a chunk and a 256-thread workgroup; one_cell_5000 (40 chunks): with D = 3 the 16
# partial sums of the run take two or three chunks each, with D = 1 (64 partial sums) some take none
@pytest.mark.parametrize('name, level, D', [('one', 8, 3), ('two_same', 8, 3), ('one_cell_300', 15, 3), ('one_cell_300', 8, 64),
                                            ('one_cell_5000', 15, 3), ('one_cell_5000', 15, 1), ('distinct_257', 8, 3),
                                            ('random_2049', 8, 3)])
def test_spc_sizes(name, level, D):
    assert 300 > 2 * CHUNK and 2049 == SORT_BLOCK + 1
    check_spc(name, level, 'cuda', D=D)


@pytest.mark.parametrize('level', [1, 8, 15])
def test_spc_levels(level):
    """level 1: at most 8 runs of ~256 members, each over several chunks; level 15: 45 key bits, six sort passes"""
    check_spc('random_2049', level, 'cuda')
    check_spc('random_2049', level, 'cuda', D=0)


@pytest.mark.parametrize('D', [1, 3, 64, 65])
def test_spc_feature_widths(D):
    check_spc('random_2049', 3, 'cuda', D=D)
    check_spc('random_2049', 1, 'cuda', D=D, feature_dtype=torch.int32)


def test_spc_special_coordinates():
    check_spc('special', 4, 'cuda')
    check_spc('special', 15, 'cuda', point_dtype=torch.float64)
    check_spc('special', 11, 'cuda', point_dtype=torch.float16)


def test_spc_nan_quantises_to_zero():
    pts = torch.tensor([[float('nan'), 0.5, 0.5], [0.5, float('nan'), float('nan')]], device='cuda')
    for p in (pts, pts.double()):
        assert conv().unbatched_pointcloud_to_spc(p, 2).point_hierarchies[-2:].tolist() == [[0, 3, 3], [3, 0, 0]]


@pytest.mark.parametrize('dtype, level', [(torch.float32, 8), (torch.float64, 15), (torch.float16, 11), (torch.float16, 3)], ids=str)
def test_spc_point_dtypes(dtype, level):
    check_spc('random_2049', level, 'cuda', point_dtype=dtype, strided=True)


@pytest.mark.parametrize('dtype', INT_DTYPES + FLOAT_DTYPES, ids=str)
def test_spc_feature_dtypes(dtype):
    check_spc('random_2049', 2, 'cuda', feature_dtype=dtype, strided=True)
    check_spc('random_2049', 1, 'cuda', feature_dtype=dtype)


@pytest.mark.parametrize('name, level, D, dtype', [('random_2049', 1, 3, torch.float32), ('random_2049', 3, 65, torch.float64),
                                                   ('one_cell_5000', 15, 3, torch.float16), ('random_2049', 2, 3, torch.int16)], ids=str)
def test_spc_gpu_cpu_and_repeat(name, level, D, dtype):
    """GPU and CPU paths: equal octrees, lengths and integer features, float features within the bound (both are checked against
    the oracle); two GPU runs give the same bits"""
    gpu, _ = check_spc(name, level, 'cuda', D=D, feature_dtype=dtype)
    cpu, _ = check_spc(name, level, 'cpu', D=D, feature_dtype=dtype)
    assert torch.equal(gpu.octrees.cpu(), cpu.octrees) and torch.equal(gpu.lengths, cpu.lengths)
    if not dtype.is_floating_point:
        assert torch.equal(gpu.features.cpu(), cpu.features)
    again, _ = check_spc(name, level, 'cuda', D=D, feature_dtype=dtype)
    assert torch.equal(gpu.octrees, again.octrees) and torch.equal(gpu.features, again.features)


def test_spc_fields_and_examples():
    check_spc_fields('cuda')
    check_reference_examples('cuda')


def test_spc_errors_before_any_launch():
    check_spc_errors('cuda')


# ---- voxel grids -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', sorted(VOXEL_DTYPES))
def test_voxelgrids_goldens(tag):
    for case in golden_cases(tag):
        got = check_voxel_case(case, 'cuda')
        pts, R, origin, scale, _, _ = golden_case(case)
        assert torch.equal(got.cpu(), conv().pointclouds_to_voxelgrids(pts, R, origin=origin, scale=scale)), case


def test_voxelgrids_errors_before_any_launch():
    check_voxelgrids_errors('cuda')
