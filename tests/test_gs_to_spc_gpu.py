"""ops.conversions.gs_to_voxelgrid through the HIP path (csrc/gs_to_spc.hip): the helpers of tests/test_gs_to_spc_cpu.py on CUDA
tensors, at the shapes where the pipeline can go wrong -- the stage boundaries of the three-level walker, the blocks of the prepare
kernel (256), of the scan (1024) and of the sort (2048), one voxel whose pack spans sort blocks -- and the reference's recorded
level-7 result.  The integer results and cov3d_invs equal the numpy oracle bit for bit; the integral lies within one float32 ulp of
the oracle's float64 value (bound in test_gs_to_spc_cpu.py); merged opacities within (n + 2) 2^-24 of the oracle's sequential
float product for a pack of n pairs.  No test feeds the kernels an out-of-range index."""
import numpy as np
import pytest
import torch

import gs_to_spc_bruteforce as bf
from test_gs_to_spc_cpu import (C, ISO, REF_TOL, TOL, bad_arguments, centred_gaussians, check_against_oracle, check_empty_cases,
                                check_integral, check_merged, golden, kal, oracle_level7, random_gaussians, reference_inputs, t,
                                ulp_share)

pytestmark = pytest.mark.gpu

PREPARE_BLOCK = 256     # Gaussians per block of gs_prepare_kernel
SCAN_BLOCK = 1024       # entries per block of ss_scan
SORT_BLOCK = 2048       # pairs per block of the radix sort (SS_SORT_BLOCK)


def random_cells(count, level, seed):
    return np.random.RandomState(seed).randint(0, 1 << level, (count, 3))


@pytest.mark.parametrize('level', [0, 1, 2, 3, 4, 6, 7])
def test_levels_around_the_stage_boundaries(level):
    """a stage finishes three levels: levels 0-3 take one stage, 4 and 6 two, 7 three"""
    want, _ = check_against_oracle(random_gaussians(5, level, level), level, 'cuda')
    assert len(want[0]) > 0


@pytest.mark.parametrize('G', [1, PREPARE_BLOCK - 1, PREPARE_BLOCK, PREPARE_BLOCK + 1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1])
def test_gaussian_counts_around_the_blocks(G):
    want, _ = check_against_oracle(random_gaussians(G, 4, G, voxels=(0.2, 0.6)), 4, 'cuda')
    assert len(want[0]) >= G


@pytest.mark.parametrize('total', [SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1, SORT_BLOCK - 1, SORT_BLOCK, SORT_BLOCK + 1])
def test_pair_totals_around_the_scan_and_sort_blocks(total):
    """every Gaussian sits inside one cell of level 4 and yields exactly one pair; cells repeat, so packs have several pairs"""
    want, _ = check_against_oracle(centred_gaussians(random_cells(total, 4, total), 4), 4, 'cuda')
    assert len(want[0]) == total and int(want[2].sum()) < total


def test_one_voxel_whose_pack_spans_sort_blocks():
    """3 000 Gaussians with one mean at level 2: one pack of 3 000 pairs over two sort blocks, Gaussian ids ascending inside it"""
    case = centred_gaussians(np.tile([[1, 2, 3]], (3000, 1)), 2)
    want, got = check_against_oracle(case, 2, 'cuda')
    assert len(want[0]) == 3000 > SORT_BLOCK and int(got[2].sum()) == 1
    assert torch.equal(got[1].cpu(), torch.arange(3000))
    voxels, merged = kal.ops.conversions.gs_to_voxelgrid(*(t(a, 'cuda') for a in case), 2)
    assert check_merged(case, 2, voxels, merged).tolist() == [3000]


def test_reference_record_at_level_7():
    g = golden()
    points, gid, boundary, cov, integral = oracle_level7()
    args = [t(a, 'cuda') for a in reference_inputs()]
    got = C.gs_to_spc_cuda(*args[:3], ISO, TOL, 7)
    for name, w, x in zip(('points', 'gaus_id', 'pack_boundary', 'cov3d_invs'), (points, gid, boundary, cov), got):
        assert np.array_equal(w, x.cpu().numpy()), name
    values = C.integrate_gs_cuda(got[0], got[1], args[0], got[3], args[3], 7, 10)
    share = ulp_share(values.cpu().numpy(), integral).max()
    print(f'integrate_gs cuda level 7: {len(points)} pairs, worst share of the bound {share:.3f}')
    assert share <= 1.0
    voxels, merged = kal.ops.conversions.gs_to_voxelgrid(*args, level=7)
    assert voxels.dtype == torch.int16 and np.array_equal(voxels.cpu().numpy(), g['voxels_7'])
    k = int(g['opacity_stride'])
    recorded = t(g['opacities_7'], 'cuda')
    print('level 7: worst opacity difference to the record', float((merged[::k] - recorded).abs().max()))
    assert torch.allclose(merged[::k], recorded, **REF_TOL)


@pytest.mark.parametrize('level', [0, 1])
def test_reference_expectations(level):
    g = golden()
    voxels, merged = kal.ops.conversions.gs_to_voxelgrid(*(t(a, 'cuda') for a in reference_inputs()), level=level)
    assert torch.equal(voxels.cpu(), t(g[f'voxels_{level}']))
    assert torch.allclose(merged.cpu(), t(g[f'opacities_{level}']), **REF_TOL)


@pytest.mark.parametrize('step', [1, 2, 7, 10])
def test_integrate_gs_within_one_ulp(step):
    """step 7: the 49 columns do not divide among the eight lanes of a pair; steps 1 and 2: fewer columns than lanes"""
    check_integral(random_gaussians(64, 4, 5), 4, step, 'cuda')


def test_merged_opacities_against_the_sequential_product():
    case = random_gaussians(64, 4, 7, voxels=(1.0, 2.0))
    voxels, merged = kal.ops.conversions.gs_to_voxelgrid(*(t(a, 'cuda') for a in case), 4)
    assert check_merged(case, 4, voxels, merged).max() > 1


def test_two_runs_are_bit_identical():
    means, scales, rots, opacities = (t(a, 'cuda') for a in random_gaussians(300, 5, 11, voxels=(0.5, 2.0)))

    def run():
        out = C.gs_to_spc_cuda(means, scales, rots, ISO, TOL, 5)
        values = C.integrate_gs_cuda(out[0], out[1], means, out[3], opacities, 5, 10)
        return list(out) + [values] + list(kal.ops.conversions.gs_to_voxelgrid(means, scales, rots, opacities, 5))

    first, second = run(), run()
    assert first[0].size(0) > SORT_BLOCK
    for a, b in zip(first, second):
        bits = (lambda x: x.view(torch.int32)) if a.dtype == torch.float32 else (lambda x: x)
        assert a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def test_hip_and_cpu_paths_agree():
    case = random_gaussians(100, 5, 13, voxels=(0.5, 2.0))
    cpu = C.gs_to_spc_cuda(*(t(a) for a in case[:3]), ISO, TOL, 5)
    hip = C.gs_to_spc_cuda(*(t(a, 'cuda') for a in case[:3]), ISO, TOL, 5)
    assert cpu[0].size(0) > 0
    for a, b in zip(cpu, hip):
        assert b.is_cuda and not a.is_cuda and torch.equal(a, b.cpu())
    pairs = tuple(x.numpy() for x in cpu)
    check_integral(case, 5, 10, 'cpu', pairs=pairs)
    check_integral(case, 5, 10, 'cuda', pairs=pairs)


def test_argument_checks_on_gpu_tensors():
    for call, what in bad_arguments('cuda'):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f'{what}: no error')


def test_empty_cases_on_gpu():
    check_empty_cases('cuda')


def test_integrate_gs_is_capturable():
    case = random_gaussians(64, 4, 17)
    points, gid, _, cov = bf.gs_to_spc(*case[:3], ISO, TOL, 4)
    args = [t(a, 'cuda') for a in (points, gid, case[0], cov, case[3])]
    eager = C.integrate_gs_cuda(*args, 4, 10)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        C.integrate_gs_cuda(*args, 4, 10)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = C.integrate_gs_cuda(*args, 4, 10)
    out.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert eager.size(0) > 0 and torch.equal(out, eager)
