"""ops.conversions.voxelgrids_to_trianglemeshes on the GPU: the HIP pipeline (csrc/mcube.hip) against the numpy oracle
(tests/mcube_bruteforce.py), the reference's recorded cases and the torch formulation on the same device -- bit for bit -- and its
one-launch backward against the torch formulation's autograd in float64 within a derived bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mcube_bruteforce as bf
from kaolin_amd import _C
from kaolin_amd.ops.conversions import voxelgrids_to_trianglemeshes
from kaolin_amd.ops.conversions.voxelgrid import _trianglemeshes_torch
from test_mcube_cpu import GOLDEN, all_cases_batch, assert_equals_oracle, check_golden, check_variations

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
HIP_DTYPES = [torch.bool, torch.uint8, torch.float16, torch.float32]          # read in place by the kernels
CAST_DTYPES = [torch.int32, torch.int64, torch.float64, torch.bfloat16]       # cast once with .float()


def rand(shape, seed, binary=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(shape, generator=g)
    return (x < 0.5) if binary else x.half().float()                           # (exact in half: one input for every dtype)


def gpu(x, iso=0.5):
    return voxelgrids_to_trianglemeshes(x.to(DEV), iso)


def torch_formulation(x, iso=0.5):
    """The torch formulation on the device of x, as lists."""
    verts, faces, nv, nf = _trianglemeshes_torch(F.pad(x.float(), (1,) * 6), iso)
    return list(torch.split(verts, nv)), list(torch.split(faces, nf))


def assert_same(got, want, equal_nan=False):
    assert len(got[0]) == len(got[1]) == len(want[0]) == len(want[1])
    for (v, f, wv, wf) in zip(*got, *want):
        assert v.dtype == torch.float32 and f.dtype == torch.int64 and v.shape == wv.shape and f.shape == wf.shape
        if equal_nan:
            assert np.array_equal(v.cpu().numpy(), wv.cpu().numpy(), equal_nan=True)
        else:
            assert torch.equal(v, wv.to(v.device))
        assert torch.equal(f, wf.to(f.device))


@pytest.mark.parametrize('n', range(14))
def test_golden(n):
    check_golden(gpu, GOLDEN[n])
    check_variations(gpu, GOLDEN[n])


def test_all_256_cases():
    x = all_cases_batch()
    assert_equals_oracle(x, got=gpu(x))
    # 258 items: the prefix over the batch walks it in rounds of 256, so items 256 (empty) and 257 start after a carried round
    more = torch.cat([x, x[:1], x[105:106]])
    assert more.shape == (258, 2, 2, 2) and not more[256].any() and more[257].any()
    assert_equals_oracle(more, got=gpu(more))


@pytest.mark.parametrize('dtype', HIP_DTYPES + CAST_DTYPES, ids=lambda d: str(d).split('.')[-1])
def test_dtypes(dtype):
    binary = not dtype.is_floating_point or dtype == torch.bfloat16
    x = rand((2, 5, 6, 7), 21, binary=binary).to(dtype)
    for iso in (0.5, 0.3):
        assert_equals_oracle(x, iso, got=gpu(x, iso))
        assert_same(gpu(x, iso), torch_formulation(x.to(DEV), iso))


def test_non_contiguous():
    x = rand((2, 5, 6, 7), 22).to(DEV)
    want = gpu(x.contiguous())
    permuted = x.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)           # Z is the slowest axis in memory
    assert not permuted.is_contiguous()
    assert_same(gpu(permuted), want)
    padded = torch.full((2, 5 + 2, 6 + 3, 2 * 7 + 1), 7., device=DEV)
    sliced = padded[:, 1:-1, 2:-1, 1::2]                                        # offsets and a step of 2 along Z
    sliced.copy_(x)
    assert not sliced.is_contiguous()
    assert_same(gpu(sliced), want)
    half = padded.half()[:, 1:-1, 2:-1, 1::2]
    assert_same(gpu(half), want)
    assert_equals_oracle(x.cpu(), got=want)
    flipped = x.flip(1, 3)
    assert_equals_oracle(flipped.cpu(), got=gpu(flipped))
    one = x[:1, :, :, :1].expand(2, -1, -1, 5)                                   # strides of 0 along the batch and Z
    assert_equals_oracle(one.cpu(), got=gpu(one))


@pytest.mark.parametrize('shape', [(1, 3, 5, 2), (1, 1, 1, 7), (2, 1, 9, 1), (1, 2, 1, 1)])
def test_non_cubic(shape):
    for binary in (False, True):
        x = rand(shape, 23, binary)
        assert_equals_oracle(x, got=gpu(x))


def test_empty_item_between_two_and_empty_batch():
    x = rand((3, 4, 5, 6), 24)
    x[1] = 0
    got = gpu(x)
    assert got[0][1].shape == (0, 3) and got[1][1].shape == (0, 3) and got[0][1].dtype == torch.float32
    assert got[1][1].dtype == torch.int64 and got[0][1].device.type == 'cuda'
    assert_equals_oracle(x, got=got)
    assert_equals_oracle(torch.zeros((2, 3, 3, 3)), got=gpu(torch.zeros((2, 3, 3, 3))))
    assert gpu(torch.zeros((0, 4, 4, 4))) == ([], [])
    assert _C.ops.conversions.voxelgrids_to_trianglemeshes_cuda(torch.zeros((0, 4, 4, 4), device=DEV)) == ([], [])


# the classify workgroup holds 256 cells of the (X+1)(Y+1)(Z+1) lattice: exactly one workgroup (8 * 8 * 4 = 256), a few cells more
# (2 * 3 * 43 = 258: 257 is prime, no lattice has it), 320, and several workgroups with a partial last one (6 * 8 * 72 = 3456 =
# 13.5 workgroups; 72 crosses a 64-lane wavefront inside a row)
@pytest.mark.parametrize('shape', [(2, 7, 7, 3), (2, 1, 2, 42), (2, 7, 7, 4), (2, 5, 7, 71)])
def test_workgroup_boundaries(shape):
    x = rand(shape, 25)
    assert_equals_oracle(x, got=gpu(x))
    b = rand(shape, 26, binary=True)
    assert_same(gpu(b), torch_formulation(b.to(DEV)))


def test_scan_crosses_its_chunk():
    """One round of the scan covers 1024 * 8 workgroup counts = 2 097 152 cells: a lattice of 128 * 128 * 130 cells (8320
    workgroups) needs a second round.  Sparse: a few blobs, one of them in the last workgroups.  Torch formulation only."""
    x = torch.zeros((1, 127, 127, 129), device=DEV)
    x[0, 3:6, 10:13, 100:104] = 1
    x[0, 60, 64, 1] = 0.75
    x[0, 125:127, 120:127, 127:129] = 1
    x[0, 126, 126, 0] = 0.625
    got = gpu(x)
    assert got[0][0].shape[0] > 100
    assert_same(got, torch_formulation(x))


def test_value_equal_to_iso():
    x = torch.zeros((1, 3, 3, 3))
    x[0, 1, 1, 1], x[0, 1, 1, 2], x[0, 0, 1, 1] = 0.5, 1, 0.5                    # not below: the vertex sits ON the lattice point
    got = gpu(x)
    assert_equals_oracle(x, got=got)
    v = got[0][0]
    assert ((v == v.round()).all(1)).any()


def test_nan_voxel():
    x = rand((1, 3, 4, 3), 27)
    x[0, 1, 2, 1] = float('nan')
    got = gpu(x)
    assert torch.isnan(got[0][0]).any()
    want_v, want_f = bf.marching_cubes(x[0].numpy())
    assert np.array_equal(got[0][0].cpu().numpy(), want_v, equal_nan=True) and np.array_equal(got[1][0].cpu().numpy(), want_f)
    assert_same(got, torch_formulation(x.to(DEV)), equal_nan=True)


def test_closed_and_oriented():
    x = rand((1, 12, 12, 12), 28, binary=True)
    verts, faces = gpu(x)
    assert bf.closed_oriented(faces[0].cpu().numpy())
    assert int(faces[0].max()) == verts[0].shape[0] - 1


def test_deterministic_and_side_stream():
    x = rand((2, 9, 10, 11), 29).to(DEV)
    first = gpu(x)
    assert_same(gpu(x), first)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        on_side = gpu(x)
    side.synchronize()
    assert_same(on_side, first)


def test_unbatched_operator():
    x = rand((1, 4, 6, 5), 30).to(DEV)
    want = gpu(x)
    v, f = _C.ops.conversions.unbatched_mcube_forward_cuda(F.pad(x[0], (1,) * 6), 0.5)
    assert_same(([v], [f]), want)
    # as given, without the border: the cells between the points only
    raw_v, raw_f = _C.ops.conversions.unbatched_mcube_forward_cuda(x[0], 0.5)
    want_v, want_f = bf.marching_cubes(x[0].cpu().numpy(), 0.5, border=False)
    assert np.array_equal(raw_v.cpu().numpy(), want_v) and np.array_equal(raw_f.cpu().numpy(), want_f)
    flat_v, flat_f = _C.ops.conversions.unbatched_mcube_forward_cuda(x[0, :1], 0.5)
    assert flat_v.shape == (0, 3) and flat_f.shape == (0, 3)


def test_operators_reject_cpu_tensors():
    x = rand((1, 3, 3, 3), 31)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        _C.ops.conversions.voxelgrids_to_trianglemeshes_cuda(x, 0.5)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        _C.ops.conversions.unbatched_mcube_forward_cuda(x[0], 0.5)


# ---- the gradient --------------------------------------------------------------------------------------------------------------
# The backward kernel computes, per grid value, sum over its <= 6 crossed lattice edges of  +-g * ((iso - f_other) / (d * d)),
# d = f_B - f_A.  Rounded float32 operations in one term: iso - f_other (1), d (1), d * d (2 + 1 = 3), the quotient (1 + 3 + 1 = 5),
# times g (6); the sign is exact.  The <= 6 terms are added in sequence: <= 5 further roundings on the first.  So
# |kernel - exact| <= gamma_11 * sum |term| with u = 2^-24.  The yardstick is the torch formulation's autograd run in float64 on the
# same float32 values; its own error is that of at most 16 operations at u = 2^-53 on its intermediate quantities g / d and
# g n / d^2, each at most |g / d| (iso lies between the two values): <= gamma_16(2^-53) * 2 sum |g / d|, some 1e-9 of the bound.
K_KERNEL = 11
K_YARDSTICK = 16
SHARES = {}


def gradient_check(x, iso, name):
    x = x.to(DEV).requires_grad_()
    verts, _ = voxelgrids_to_trianglemeshes(x, iso)
    assert all(v.requires_grad and v.dtype == torch.float32 for v in verts)
    gen = torch.Generator().manual_seed(5)
    weights = [torch.rand(v.shape, generator=gen) * 2 - 1 for v in verts]
    sum((v * w.to(DEV)).sum() for v, w in zip(verts, weights)).backward()
    assert x.grad.dtype == x.dtype and x.grad.shape == x.shape

    y = x.detach().float().double().requires_grad_()
    v64 = _trianglemeshes_torch(F.pad(y, (1,) * 6), iso)[0]
    (v64 * torch.cat(weights).double().to(DEV)).sum().backward()
    worst = 0.0
    for b in range(x.shape[0]):
        exact, magnitude, edges = bf.vertex_gradient_terms(x[b].detach().float().cpu().numpy(), iso, weights[b].numpy())
        yard = y.grad[b].cpu().numpy()
        yard_error = bf.gamma(K_YARDSTICK, 2.0 ** -53) * 2 * edges
        assert np.all(np.abs(yard - exact) <= yard_error)                          # the yardstick is the closed form
        bound = bf.gamma(K_KERNEL) * magnitude
        err = np.abs(x.grad[b].double().cpu().numpy() - yard)
        share = float(np.max(np.where(magnitude > 0, err / np.where(magnitude > 0, bound, 1), 0)))
        worst = max(worst, share)
        print(f'mcube gradient {name} item {b}: worst share of the bound {share:.3f}')
        assert np.all(err <= bound + yard_error)
        assert np.all(x.grad[b].cpu().numpy()[magnitude == 0] == 0)
    SHARES[name] = worst
    return x.grad.clone()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64], ids=['float32', 'float64'])
@pytest.mark.parametrize('iso', [0.5, 0.3])
def test_gradient(dtype, iso):
    g = torch.Generator().manual_seed(41)
    x = torch.rand((2, 6, 5, 7), generator=g, dtype=dtype)
    first = gradient_check(x, iso, f'{dtype}-{iso}')
    assert torch.equal(gradient_check(x, iso, f'{dtype}-{iso}'), first)            # bit-equal across two runs


def test_gradient_six_crossed_edges():
    """A single voxel above iso among zeros: all six of its lattice edges are crossed, every other value has at most one."""
    x = torch.zeros((1, 3, 3, 3))
    x[0, 1, 1, 1] = 0.8125
    grad = gradient_check(x, 0.5, 'six')
    assert grad[0, 1, 1, 1] != 0
    x = torch.full((1, 1, 1, 1), 0.9)                                           # ... all six reach into the border
    assert gradient_check(x, 0.5, 'six-border')[0, 0, 0, 0] != 0


def test_gradient_half_and_strided():
    x = rand((1, 4, 5, 6), 42).to(DEV)
    a = x.clone().requires_grad_()
    verts, _ = voxelgrids_to_trianglemeshes(a)
    verts[0].sum().backward()
    t = x.permute(0, 3, 2, 1).contiguous().permute(0, 3, 2, 1).requires_grad_()
    verts_t, _ = voxelgrids_to_trianglemeshes(t)
    verts_t[0].sum().backward()
    assert torch.equal(t.grad, a.grad)
    h = x.half().requires_grad_()
    verts_h, _ = voxelgrids_to_trianglemeshes(h)
    verts_h[0].sum().backward()
    assert h.grad.dtype == torch.float16 and torch.equal(h.grad, a.grad.half())  # (x is exact in half: the same float32 sums)
    with torch.no_grad():
        assert not voxelgrids_to_trianglemeshes(a)[0][0].requires_grad
