"""farthest_point_sampling on the GPU (csrc/fps.hip), both kernel designs, bit-exact against the numpy oracle of
tests/test_fps_cpu.py: `block` keeps a cloud in the registers of one workgroup, thread t owning points t + 1024 j in tiers of
1024 P points up to the limit L; `rounds` launches once per selected point, a workgroup per slice of 2048 points."""
import math

import pytest
import torch

from kaolin_amd import _C, _lib
from kaolin_amd.ops import pointcloud as pc
from test_fps_cpu import fps_oracle, lattice, oracle_batch, special

pytestmark = pytest.mark.gpu

L = _lib.load().kamd_fps_block_limit()
SLICE = 2048
TIERS = [1024 * P + e for P in (1, 2, 4, 8, 16) for e in (0, 1) if 1024 * P + e <= L]

CASES = [('block', N, N, 1) for N in (1, 2, 63, 64, 65)]
CASES += [('block', N, min(N, 300), 1) for N in (1023, 1024, 1025)]
CASES += [('block', N, 64, 1) for N in TIERS]
CASES += [('block', 3000, 32, 3), ('block', 3000, 0, 1)]
CASES += [('rounds', 1, 1, 1), ('rounds', 65, 65, 1), ('rounds', SLICE, 64, 1), ('rounds', SLICE + 1, 64, 3),
          ('rounds', 2 * SLICE + 1, 64, 3), ('rounds', 3000, 0, 1)]
CASES += [(None, L + 1, 64, 1)]


def run(points, k, path):
    """`path` None: the public function; else that design, forced through the shim"""
    dev = points.cuda()
    out = pc.farthest_point_sampling(dev, k) if path is None else _C.ops.farthest_point_sampling_cuda(dev, k, path=path)
    assert out.dtype == torch.int64 and out.device == dev.device and out.shape == (points.shape[0], k)
    return out.cpu()


@pytest.mark.parametrize('path,N,k,B', CASES)
def test_lattice(path, N, k, B):
    points = lattice(B, N, seed=N)
    assert torch.equal(run(points, k, path), oracle_batch(points, k))


@pytest.mark.parametrize('path', ['block', 'rounds'])
@pytest.mark.parametrize('N,k', [(20, 15), (3000, 32)])
@pytest.mark.parametrize('kind', ['nan', 'inf', 'dup', 'overflow'])
def test_special_values(path, N, k, kind):
    points = special(N, kind)
    out = run(points, k, path)
    assert torch.equal(out, oracle_batch(points, k))
    if k == 32 and kind in ('nan', 'inf'):
        assert torch.isfinite(points[0, out[0]]).all()


@pytest.mark.parametrize('path', ['block', 'rounds'])
def test_generic_floats(path):
    """The centre of generic floats depends on the order of the sum, so the first index is held to the reference's own tolerance
    (tests/python/kaolin/ops/test_pointcloud.py:72) and the rest to the oracle replayed from that index: the unfused float32 d."""
    points = torch.rand(2, 3000, 3, generator=torch.Generator().manual_seed(7))
    out = run(points, 64, path)
    for cloud, idx in zip(points.double(), out):
        from_centre = (cloud - cloud.mean(dim=0)).norm(dim=1)
        assert math.isclose(from_centre[idx[0]], from_centre.max(), rel_tol=1e-5, abs_tol=1e-5)
        assert idx.tolist() == fps_oracle(cloud.numpy(), 64, first=int(idx[0]))


def test_forced_block_above_its_limit_is_an_error():
    with pytest.raises(RuntimeError):
        _C.ops.farthest_point_sampling_cuda(torch.zeros(1, L + 1, 3, device='cuda'), 1, path='block')
