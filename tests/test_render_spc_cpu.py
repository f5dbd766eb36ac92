"""render.spc on CPU tensors (the torch formulations) against the numpy oracle of tests/spc_raytrace_oracle.py, and the oracle
against the reference's recorded answers (tests/golden/render_spc_examples.json).  Traces and scans are compared with torch.equal:
the contract fixes every bit.  The scenes, the rays and the check functions are shared with tests/test_render_spc_gpu.py, which
runs them through the HIP path."""
import functools
import json
import os
import warnings

import numpy as np
import pytest
import torch

import spc_bruteforce as bf
import spc_raytrace_oracle as ro
from conftest import GOLDEN_DIR


def rspc():
    import kaolin_amd as kal
    return kal.render.spc


def fixture():
    with open(os.path.join(GOLDEN_DIR, 'render_spc_examples.json')) as f:
        return json.load(f)


def t(array, device, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(array), dtype=dtype).to(device)


def scene_args(scene, device):
    """(octree, point_hierarchy, pyramid (CPU), exsum) of a scene"""
    return t(scene.octree, device), t(scene.points, device), t(scene.pyramid, 'cpu'), t(scene.exsum, device)


# ------------------------------------------------------------------------------------------------------------------ scenes and rays
def golden_scene():
    doc = fixture()
    return ro.scene_from_octree(doc['octree'], doc['level'])


def golden_rays(doc, name):
    """the reference's 4 x 4 orthographic grid: ray = 4 * (index of x) + (index of y)"""
    g, ex = doc['grid'], doc[name]
    origin = np.array([[x, y, ex['z']] for x in g for y in g], dtype=np.float32)
    return origin, np.tile(np.array(ex['direction'], dtype=np.float32), (len(origin), 1))


def dense_scene(level):
    return ro.scene_from_cube(np.ones((2 ** level,) * 3, dtype=bool))


@functools.lru_cache(maxsize=None)
def random_scene():
    return ro.scene_from_cube(bf.random_cube(4, 3, 0.08))


def perspective_rays(n, seed):
    """origins in [-1.5, 1.5]^3 (about a quarter inside the volume), each aimed at a random point of the volume"""
    rng = np.random.RandomState(seed)
    origin = rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)
    target = rng.uniform(-1.0, 1.0, (n, 3)).astype(np.float32)
    direction = target - origin
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    return origin, direction.astype(np.float32)


def edge_rays(n=1025):
    """rays from outside aimed at the volume; every third one is turned round and misses, so the offsets cross empty rays"""
    rng = np.random.RandomState(11)
    origin = rng.normal(size=(n, 3))
    origin = (2.5 * origin / np.linalg.norm(origin, axis=1, keepdims=True)).astype(np.float32)
    target = rng.uniform(-0.9, 0.9, (n, 3)).astype(np.float32)
    direction = target - origin
    direction /= np.linalg.norm(direction, axis=1, keepdims=True)
    direction[::3] *= -1
    return origin, direction.astype(np.float32)


def _case(name):
    """-> (scene, origin, direction, level)"""
    f32 = np.float32
    if name in ('positive', 'negative', 'none', 'coarser'):
        doc = fixture()
        return (golden_scene(),) + golden_rays(doc, name) + (doc[name].get('level', doc['level']),)
    if name == 'level0':        # one ray that hits the root, one whose origin is inside it, one that misses
        return (golden_scene(), np.array([[0.25, 0.5, -3], [0.25, 0.5, 0.125], [3, 3, -3]], dtype=f32),
                np.array([[0, 0, 1]] * 3, dtype=f32), 0)
    if name == 'chain15':       # 15 levels of the last child: one voxel of 2^-14 at the (1, 1, 1) corner
        return (ro.scene_from_octree([128] * 15, 15), np.array([[-2, -2, -2], [-2, -2, -2.5]], dtype=f32),
                np.array([[1, 1, 1], [1, 1, 1]], dtype=f32), 15)
    if name == 'dense3':        # dyadic coordinates: all the arithmetic is exact and the tie order is the contract's
        origin = np.array([[-2, 0.125, -0.375],      # along +x through 8 voxels
                           [0.625, 2, 0.375],        # along -y, the other components -0.0
                           [-2, -2, -2],             # the main diagonal: through voxel corners
                           [2, 2, -2],               # another diagonal
                           [-2, 0, 0],               # on the centre planes y = 0 and z = 0 of the root
                           [0, 0, -3],               # on x = 0 and y = 0
                           [-2, 0.5, -0.25],         # on centre planes of deeper levels
                           [0, 0, 0],                # inside, on every centre plane of the root
                           [0.125, 0.125, 0.125]],   # inside a voxel
                          dtype=f32)
        direction = np.array([[1, 0, 0], [-0.0, -1, -0.0], [1, 1, 1], [-1, -1, 1], [1, 0, 0], [0, 0, 1], [1, 0, 0], [1, 0.5, 0.25],
                              [-1, 0.5, 0]], dtype=f32)
        return dense_scene(3), origin, direction, 3
    if name == 'random600':
        return (random_scene(),) + perspective_rays(600, 5) + (4,)
    if name == 'edges1025':
        return (random_scene(),) + edge_rays() + (4,)
    if name == 'all_miss':
        origin, direction = perspective_rays(70, 9)
        origin = (origin + np.array([4, 0, 0])).astype(f32)
        direction = np.abs(direction) * np.array([1, 1, 1], dtype=f32)          # from x >= 2.5 towards +x
        return random_scene(), origin, direction, 4
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (scene, origin, direction, level, (nuggets, entry, exit) of the oracle); computed once and shared"""
    scene, origin, direction, level = _case(name)
    return scene, origin, direction, level, ro.trace(scene, origin, direction, level)


def check_trace(name, device, rays=None):
    """all three forms of the call on the first `rays` rays of a case against the oracle, bit for bit"""
    R = rspc()
    scene, origin, direction, level, (nuggets, entry, leave) = case(name)
    n = len(origin) if rays is None else rays
    rows = nuggets[:, 0] < n                                         # rays are independent: a prefix of the rays = a prefix of the result
    nuggets, entry, leave = nuggets[rows], entry[rows], leave[rows]
    args = scene_args(scene, device) + (t(origin[:n], device), t(direction[:n], device), level)
    ridx, pidx = R.unbatched_raytrace(*args, return_depth=False)
    assert ridx.dtype == torch.int32 and pidx.dtype == torch.int32 and ridx.device.type == device
    assert ridx.shape == (len(nuggets),) and pidx.shape == (len(nuggets),)
    assert torch.equal(torch.stack([ridx, pidx], 1).cpu(), t(nuggets, 'cpu').reshape(-1, 2))
    ridx1, pidx1 = R.unbatched_raytrace(*args, return_depth=False, with_exit=True)      # without depths with_exit does nothing
    assert torch.equal(ridx1, ridx) and torch.equal(pidx1, pidx)
    ridx2, pidx2, depth = R.unbatched_raytrace(*args)
    assert torch.equal(ridx2, ridx) and torch.equal(pidx2, pidx)
    assert depth.dtype == torch.float32 and depth.shape == (len(nuggets), 1)
    assert torch.equal(depth.cpu()[:, 0], t(entry, 'cpu'))
    out = leave > 0                                                  # with both depths a hit also needs a positive exit
    ridx3, pidx3, depth2 = R.unbatched_raytrace(*args, return_depth=True, with_exit=True)
    assert depth2.shape == (int(out.sum()), 2)
    assert torch.equal(torch.stack([ridx3, pidx3], 1).cpu(), t(nuggets[out], 'cpu').reshape(-1, 2))
    assert torch.equal(depth2.cpu(), t(np.stack([entry[out], leave[out]], 1), 'cpu').reshape(-1, 2))
    return nuggets


# ------------------------------------------------------------------------------------------------------------------------ pack cases
PACK_LAYOUTS = {'single': [70], 'each': [1] * 67, 'mixed': [1, 2, 63, 64, 65, 1025, 1]}


@functools.lru_cache(maxsize=None)
def pack_case(layout, dtype_name, C):
    """-> (feats (n, C) numpy, boundaries (n) bool numpy); values near 1 so that a product of 1025 of them stays finite"""
    lengths = PACK_LAYOUTS[layout]
    n = sum(lengths)
    rng = np.random.RandomState(n + C)
    feats = rng.uniform(0.9, 1.1, (n, C)).astype(dtype_name)
    boundaries = np.zeros(n, dtype=bool)
    boundaries[np.cumsum([0] + lengths[:-1])] = True
    return feats, boundaries


def check_pack_ops(layout, dtype_name, C, device):
    R = rspc()
    feats_np, b_np = pack_case(layout, dtype_name, C)
    feats, b = t(feats_np, device), t(b_np, device)
    for exclusive in (False, True):
        for reverse in (False, True):
            for fn, prod in ((R.cumsum, False), (R.cumprod, True)):
                got = fn(feats, b, exclusive=exclusive, reverse=reverse)
                want = ro.pack_scan(feats_np, b_np, prod, exclusive, reverse)
                assert got.dtype == feats.dtype and got.device == feats.device
                assert torch.equal(got.cpu(), t(want, 'cpu')), (fn.__name__, exclusive, reverse)
    for fn, prod in ((R.sum_reduce, False), (R.prod_reduce, True)):
        got = fn(feats, b)
        assert got.shape == (int(b_np.sum()), C)
        assert torch.equal(got.cpu(), t(ro.pack_reduce(feats_np, b_np, prod), 'cpu')), fn.__name__
        assert torch.equal(fn(feats, b), got)                        # bit-identical run to run


def check_pack_backward(dtype_name, device):
    """the backward passes are scans and gathers themselves: compared with the oracle's, bit for bit"""
    R = rspc()
    feats_np, b_np = pack_case('mixed', dtype_name, 3)
    rng = np.random.RandomState(2)
    g_np = rng.uniform(-1, 1, feats_np.shape).astype(dtype_name)
    b, g = t(b_np, device), t(g_np, device)
    for exclusive in (False, True):
        for reverse in (False, True):
            feats = t(feats_np, device).requires_grad_()
            R.cumsum(feats, b, exclusive=exclusive, reverse=reverse).backward(g)
            want = ro.pack_scan(g_np, b_np, False, exclusive, not reverse)
            assert torch.equal(feats.grad.cpu(), t(want, 'cpu')), ('cumsum', exclusive, reverse)
            feats = t(feats_np, device).requires_grad_()
            R.cumprod(feats, b, exclusive=exclusive, reverse=reverse).backward(g)
            prod = ro.pack_scan(feats_np, b_np, True, exclusive, reverse)
            want = ro.pack_scan(prod * g_np, b_np, False, exclusive, not reverse) / feats_np
            assert torch.equal(feats.grad.cpu(), t(want, 'cpu')), ('cumprod', exclusive, reverse)
    feats = t(feats_np, device).requires_grad_()
    out = R.sum_reduce(feats, b)
    go = rng.uniform(-1, 1, tuple(out.shape)).astype(dtype_name)
    out.backward(t(go, device))
    assert torch.equal(feats.grad.cpu(), t(go[np.cumsum(b_np) - 1], 'cpu'))
    with pytest.raises(RuntimeError):                               # prod_reduce has no backward pass
        R.prod_reduce(t(feats_np, device).requires_grad_(), b).sum().backward()


def check_exponential_integration(dtype_name, device):
    """the reference's composition: alpha = 1 - exp(-tau), transmittance = exp(-cumsum(tau)) * alpha, the sum of transmittance *
    feats over every pack -- exp by torch on the same device, the scan and the reduction by the oracle"""
    R = rspc()
    feats_np, b_np = pack_case('mixed', dtype_name, 3)
    tau_np = np.random.RandomState(4).uniform(0, 0.3, (len(b_np), 1)).astype(dtype_name)
    feats, tau, b = t(feats_np, device), t(tau_np, device), t(b_np, device)
    for exclusive in (True, False):
        out, transmittance = R.exponential_integration(feats, tau, b, exclusive=exclusive)
        want = torch.exp(-1.0 * t(ro.pack_scan(tau_np, b_np, False, exclusive, False), device)) * (1.0 - torch.exp(-tau))
        assert torch.equal(transmittance, want)
        weighted = (want * feats).cpu().numpy()
        assert torch.equal(out.cpu(), t(ro.pack_reduce(weighted, b_np, False), 'cpu'))


# ---------------------------------------------------------------------------------------------------------- the oracle is pinned
def test_oracle_matches_reference_goldens():
    doc = fixture()
    for name in ('positive', 'negative', 'none', 'coarser'):
        nuggets, entry, leave = case(name)[4]
        assert nuggets.tolist() == doc[name]['nuggets'], name
    _, entry, leave = case('negative')[4]
    assert entry.tolist() == doc['negative']['entry'] and leave.tolist() == doc['negative']['exit']
    assert (leave > 0).all()


# (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is a float32 tie; + 2^-60 lifts it above the tie, but float64 drops the 2^-60, lands on the tie
# and float32 then rounds to even: the double-rounding case.  Rows: (a, b, c, fmaf(a, b, c)).
FMAF_ROWS = [(1 + 2.0 ** -12, 1 + 2.0 ** -12, 2.0 ** -60, 1 + 2.0 ** -11 + 2.0 ** -23),
             (1 + 2.0 ** -12, 1 + 2.0 ** -12, 0.0, 1 + 2.0 ** -11),
             (1 + 2.0 ** -12, 1 + 2.0 ** -12, -2.0 ** -60, 1 + 2.0 ** -11),
             (-1 - 2.0 ** -12, 1 + 2.0 ** -12, -2.0 ** -60, -1 - 2.0 ** -11 - 2.0 ** -23),
             (2.0 ** -12, 2.0 ** -12, 1.0, 1.0),
             (2.0 ** -12 + 2.0 ** -35, 2.0 ** -12, 1.0, 1 + 2.0 ** -23)]


def test_oracle_fmaf_rounds_once():
    f = np.float32
    for a, b, c, want in FMAF_ROWS:
        assert f(a) == a and f(b) == b and f(c) == c and f(want) == want
        assert ro.fmaf(f(a), f(b), f(c)) == f(want), (a, b, c)
    a, b, c, want = FMAF_ROWS[0]
    assert f(np.float64(a) * np.float64(b) + np.float64(c)) != f(want)       # the trap is real: plain float64 rounds twice


def test_fmaf_of_the_package_matches_the_oracle():
    """the torch emulation on the double-rounding rows, on non-finite operands and on random operands of mixed magnitude"""
    from kaolin_amd.render.spc.raytrace import _fmaf
    rng = np.random.RandomState(0)
    n = 4000
    a, b, c = ((rng.uniform(-1, 1, n) * 2.0 ** rng.randint(-30, 5, n)).astype(np.float32) for _ in range(3))
    k = len(FMAF_ROWS)
    a[:k], b[:k], c[:k] = [r[0] for r in FMAF_ROWS], [r[1] for r in FMAF_ROWS], [r[2] for r in FMAF_ROWS]
    a[k:k + 3], b[k:k + 3], c[k:k + 3] = [np.inf, 0.0, 1.0], [0.0, 3.0, np.inf], [1.0, -0.0, -np.inf]
    want = np.array([ro.fmaf(x, y, z) for x, y, z in zip(a, b, c)], dtype=np.float32)
    got = _fmaf(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(c)).numpy()
    assert np.isnan(want[k]) and np.isnan(want[k + 2]) and np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert np.array_equal(got.view(np.int32)[ok], want.view(np.int32)[ok])
    assert got[:k].tolist() == [np.float32(r[3]) for r in FMAF_ROWS]


def test_mark_pack_boundaries_docstring_example():
    R, ex = rspc(), fixture()['mark_pack_boundaries']
    got = R.mark_pack_boundaries(torch.tensor(ex['pack_ids'], dtype=torch.int32))
    assert got.dtype == torch.bool and got.tolist() == ex['boundaries']
    for dtype in (torch.uint8, torch.int16, torch.int64):
        assert R.mark_pack_boundaries(torch.tensor(ex['pack_ids'], dtype=dtype)).tolist() == ex['boundaries']
    assert R.mark_pack_boundaries(torch.zeros(0, dtype=torch.int32)).shape == (0,)


def test_mark_first_hit_warns():
    R = rspc()
    with pytest.warns(UserWarning, match='mark_first_hit has been deprecated'):
        got = R.mark_first_hit(torch.tensor([0, 0, 3], dtype=torch.int32))
    assert got.tolist() == [True, False, True]


# ------------------------------------------------------------------------------------------------------------- tracing on the CPU
@pytest.mark.parametrize('name', ['positive', 'negative', 'none', 'coarser', 'level0', 'chain15', 'dense3', 'random600', 'all_miss'])
def test_trace_cpu(name):
    nuggets = check_trace(name, 'cpu')
    if name == 'chain15':
        assert nuggets.tolist() == [[0, 15]]
    if name == 'level0':
        assert nuggets.tolist() == [[0, 0]]
    if name in ('none', 'all_miss'):
        assert len(nuggets) == 0
    if name == 'dense3':
        assert (nuggets[:, 0] == 0).sum() == 8                      # the axis ray goes through 8 voxels


def test_trace_cpu_golden_shapes_and_views():
    R, doc = rspc(), fixture()
    scene = golden_scene()
    origin, direction = golden_rays(doc, 'none')
    ridx, pidx, depth = R.unbatched_raytrace(*scene_args(scene, 'cpu'), t(origin, 'cpu'), t(direction, 'cpu'), 2, with_exit=True)
    assert [list(ridx.shape), list(pidx.shape), list(depth.shape)] == doc['none']['shapes']
    origin, direction = golden_rays(doc, 'positive')
    ridx, pidx = R.unbatched_raytrace(*scene_args(scene, 'cpu'), t(origin, 'cpu'), t(direction, 'cpu'), 2, return_depth=False)
    assert ridx.stride() == (2,) and ridx.data_ptr() + 4 == pidx.data_ptr()      # the two columns of one tensor
    empty = torch.zeros((0, 3))
    ridx, pidx, depth = R.unbatched_raytrace(*scene_args(scene, 'cpu'), empty, empty, 2)
    assert ridx.shape == (0,) and pidx.shape == (0,) and depth.shape == (0, 1)


def test_trace_prefixes_share_one_oracle_run():
    for n in (1, 63, 65):
        check_trace('edges1025', 'cpu', rays=n)


def test_trace_depths_are_front_to_back():
    nuggets, entry, _ = case('random600')[4]
    assert len(nuggets) > 600
    for ray in np.unique(nuggets[:, 0]):
        assert (np.diff(entry[nuggets[:, 0] == ray]) >= 0).all()


def test_trace_value_errors():
    R = rspc()
    scene, origin, direction, level, _ = case('positive')
    octree, points, pyramid, exsum = scene_args(scene, 'cpu')
    o, d = t(origin, 'cpu'), t(direction, 'cpu')
    for bad in (-1, 3, 16):
        with pytest.raises(ValueError, match='level'):
            R.unbatched_raytrace(octree, points, pyramid, exsum, o, d, bad)
    with pytest.raises(ValueError, match='float32'):
        R.unbatched_raytrace(octree, points, pyramid, exsum, o.double(), d, 2)
    with pytest.raises(ValueError, match='num_rays, 3'):
        R.unbatched_raytrace(octree, points, pyramid, exsum, o[:, :2], d, 2)
    with pytest.raises(ValueError, match='origins for'):
        R.unbatched_raytrace(octree, points, pyramid, exsum, o[:5], d, 2)
    legacy = torch.cat([exsum.new_zeros(1), exsum])
    with pytest.raises(ValueError, match='legacy'):
        R.unbatched_raytrace(octree, points, pyramid, legacy, o, d, 2)


def test_trace_has_no_gradient():
    R = rspc()
    scene, origin, direction, level, _ = case('negative')
    o, d = t(origin, 'cpu').requires_grad_(), t(direction, 'cpu').requires_grad_()
    _, _, depth = R.unbatched_raytrace(*scene_args(scene, 'cpu'), o, d, level)
    assert not depth.requires_grad


# ------------------------------------------------------------------------------------------------------------------ packs on the CPU
@pytest.mark.parametrize('dtype_name', ['float32', 'float64'])
@pytest.mark.parametrize('layout,C', [('single', 3), ('each', 1), ('mixed', 3), ('mixed', 65)])
def test_pack_ops_cpu(layout, C, dtype_name):
    check_pack_ops(layout, dtype_name, C, 'cpu')


@pytest.mark.parametrize('dtype_name', ['float32', 'float64'])
def test_pack_backward_cpu(dtype_name):
    check_pack_backward(dtype_name, 'cpu')


@pytest.mark.parametrize('dtype_name', ['float32', 'float64'])
def test_exponential_integration_cpu(dtype_name):
    check_exponential_integration(dtype_name, 'cpu')


def _loop_scan(feats, lengths, prod, exclusive, reverse):
    """per pack, with torch's own differentiable cumsum / cumprod"""
    pieces, first = [], 0
    for n in lengths:
        x = feats[first:first + n]
        first += n
        if reverse:
            x = x.flip(0)
        y = torch.cumprod(x, 0) if prod else torch.cumsum(x, 0)
        if exclusive:
            y = torch.cat([torch.ones_like(x[:1]) if prod else torch.zeros_like(x[:1]), y[:-1]])
        pieces.append(y.flip(0) if reverse else y)
    return torch.cat(pieces)


@pytest.mark.parametrize('exclusive', [False, True])
@pytest.mark.parametrize('reverse', [False, True])
def test_pack_autograd_against_a_per_pack_loop(exclusive, reverse):
    R = rspc()
    lengths = [3, 1, 5, 2]
    n = sum(lengths)
    b = torch.zeros(n, dtype=torch.bool)
    b[np.cumsum([0] + lengths[:-1])] = True
    gen = torch.Generator().manual_seed(1)
    x0 = torch.rand((n, 2), generator=gen, dtype=torch.float64) + 0.5
    g = torch.rand((n, 2), generator=gen, dtype=torch.float64)
    for fn, prod in ((R.cumsum, False), (R.cumprod, True)):
        x = x0.clone().requires_grad_()
        got = fn(x, b, exclusive=exclusive, reverse=reverse)
        got.backward(g)
        y = x0.clone().requires_grad_()
        want = _loop_scan(y, lengths, prod, exclusive, reverse)
        want.backward(g)
        assert torch.allclose(got, want, rtol=1e-13, atol=0) and torch.allclose(x.grad, y.grad, rtol=1e-12, atol=1e-15)
        assert torch.autograd.gradcheck(lambda v: fn(v, b, exclusive=exclusive, reverse=reverse), (x0.clone().requires_grad_(),))
    x = x0.clone().requires_grad_()
    got = R.sum_reduce(x, b)
    want = torch.stack([p.sum(0) for p in torch.split(x0, lengths)])
    assert torch.allclose(got, want, rtol=1e-13, atol=0)
    assert torch.autograd.gradcheck(lambda v: R.sum_reduce(v, b), (x0.clone().requires_grad_(),))


def test_diff_and_other_dtypes():
    R = rspc()
    feats = torch.tensor([[1.0], [4.0], [9.0], [16.0], [2.0], [3.0]])
    b = torch.tensor([True, False, False, True, True, False])
    assert R.diff(feats, b)[:, 0].tolist() == [3.0, 5.0, 0.0, 0.0, 1.0, 0.0]
    # half runs the torch formulation: 6 elements of size <= 16, one rounding of 2^-11 relative per step
    half = R.cumsum(feats.half(), b)
    assert half.dtype == torch.float16
    assert torch.allclose(half.float(), torch.tensor([[1.0], [5.0], [14.0], [16.0], [2.0], [5.0]]), rtol=3 * 2.0 ** -11, atol=0)
    assert R.sum_reduce(feats.half(), b).float()[:, 0].tolist() == [14.0, 16.0, 5.0]
    with pytest.raises(ValueError):
        R.cumsum(feats, b[:3])
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        R.cumsum(feats, b)


def test_install_as_kaolin_provides_render_spc():
    import importlib
    import kaolin_amd as kal
    kal.install_as_kaolin()
    mod = importlib.import_module('kaolin.render.spc')
    assert mod.unbatched_raytrace is kal.render.spc.unbatched_raytrace
    names = ('raytrace_cuda', 'mark_pack_boundaries_cuda', 'diff_cuda', 'inclusive_sum_cuda', 'sum_reduce_cuda', 'prod_reduce_cuda',
             'cumsum_cuda', 'cumprod_cuda')
    assert all(hasattr(kal._C.render.spc, n) for n in names)
