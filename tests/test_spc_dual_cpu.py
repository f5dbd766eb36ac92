"""ops.spc feature grids on CPU tensors (the torch formulations): dual octree, trinkets, trilinear coefficients and interpolation against
the brute force of tests/spc_dual_bruteforce.py, and the brute force against the reference's documented answer
(tests/golden/spc_dual_examples.json).  Hierarchies, trinkets and parents are compared with torch.equal; interpolated values and
gradients within bounds derived from the arithmetic (see `forward_bound`, `feats_bound`, `coords_bound`).  The `check_*` helpers
take a device: tests/test_spc_dual_gpu.py runs them through the HIP path."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import spc_bruteforce as bf
import spc_dual_bruteforce as dbf
from conftest import GOLDEN_DIR

EPS32, EPS16, EPS64 = 2.0 ** -24, 2.0 ** -11, 2.0 ** -53


def half_rounding(result):
    """the final rounding of a half output: 2^-11 |result| -- and, a term a purely relative bound misses, half a spacing of the
    subnormal halves, 2^-25, where |result| < 2^-14 (there 2^-11 |result| < 2^-25; a coefficient near 0 gives such results)"""
    return np.maximum(EPS16 * np.abs(result), 2.0 ** -25)


def spc():
    import kaolin_amd as kal
    return kal.ops.spc


def t(array, device, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(array), dtype=dtype).to(device)


def fixture():
    with open(os.path.join(GOLDEN_DIR, 'spc_dual_examples.json')) as f:
        return json.load(f)['make_dual_example']


def cube_with_points(level, num_points, seed):
    """a random cube of `level` whose hierarchy has exactly `num_points` points over all its levels: cells are added while they
    do not overshoot; a cell next to an occupied one adds a single point, so the target is always reached"""
    assert num_points >= level + 1
    rng = np.random.RandomState(seed)
    seen = [set() for _ in range(level + 1)]
    cube = np.zeros((2 ** level,) * 3, dtype=bool)
    total = 0
    while total < num_points:
        p = rng.randint(0, 2 ** level, 3)
        new = [l for l in range(level + 1) if tuple(p >> (level - l)) not in seen[l]]
        if new and total + len(new) <= num_points:
            for l in new:
                seen[l].add(tuple(p >> (level - l)))
            total += len(new)
            cube[tuple(p)] = True
    return cube


# ------------------------------------------------------------------------------------------------------ the brute force is pinned
def test_bruteforce_matches_the_reference_example():
    ex = fixture()
    dual = dbf.make_dual(bf.decode(bf.cube_of_points(ex['points'], ex['level'])))
    assert dual.level_points[0].tolist() == ex['dual_level_0'] and len(ex['dual_level_0']) == 8
    assert dual.level_points[1].tolist() == ex['dual_level_1'] and len(ex['dual_level_1']) == 16
    assert dual.pyramid.tolist() == ex['pyramid_dual']


# ------------------------------------------------------------------------------------------------------- dual, trinkets, parents
def check_invariant(S, points, pyramid, dual, pyramid_dual, trinkets, parents):
    """the invariant of the reference's own trinket test: the dual points a level's trinkets name are the corners of the level's
    points, and the points the parents name are the points halved"""
    L = pyramid.shape[1] - 2
    assert trinkets.dtype == torch.int32 and parents.dtype == torch.int32
    assert tuple(trinkets.shape) == (points.shape[0], 8) and tuple(parents.shape) == (points.shape[0],)
    for l in range(L + 1):
        lo, hi = int(pyramid[1, l]), int(pyramid[1, l + 1])
        named = dual[int(pyramid_dual[1, l]) + trinkets[lo:hi].long()]
        assert torch.equal(named, S.points_to_corners(points[lo:hi]))
        if l > 0:
            assert torch.equal(points[parents[lo:hi].long()], points[lo:hi] >> 1)
    assert parents[0].item() == -1


def check_dual(cube, device):
    """dual, trinkets and parents of the octree of `cube` against the brute force -> (Decoded, Dual, the package's tensors)"""
    S = spc()
    d = bf.decode(cube)
    want = dbf.make_dual(d)
    points, pyramid = t(d.points, device), t(d.pyramid, 'cpu')
    dual, pyramid_dual = S.unbatched_make_dual(points, pyramid)
    assert dual.dtype == torch.int16 and dual.device.type == device
    assert pyramid_dual.dtype == pyramid.dtype and pyramid_dual.device.type == 'cpu' and pyramid_dual.shape == pyramid.shape
    assert torch.equal(pyramid_dual, t(want.pyramid, 'cpu'))
    assert torch.equal(dual.cpu(), t(want.points, 'cpu'))
    trinkets, parents = S.unbatched_make_trinkets(points, pyramid, dual, pyramid_dual)
    assert torch.equal(trinkets.cpu(), t(want.trinkets, 'cpu')) and torch.equal(parents.cpu(), t(want.parents, 'cpu'))
    check_invariant(S, points, pyramid, dual, pyramid_dual, trinkets, parents)
    return d, want, (points, pyramid, dual, pyramid_dual, trinkets, parents)


def check_fixture(device):
    S, ex = spc(), fixture()
    octree = S.unbatched_points_to_octree(torch.tensor(ex['points'], dtype=torch.int16, device=device), ex['level'])
    _, pyramids, exsum = S.scan_octrees(octree, torch.tensor([len(octree)], dtype=torch.int32))
    points = S.generate_points(octree, pyramids, exsum)
    dual, pyramid_dual = S.unbatched_make_dual(points, pyramids[0])
    assert S.unbatched_get_level_points(dual, pyramid_dual, 0).tolist() == ex['dual_level_0']
    assert S.unbatched_get_level_points(dual, pyramid_dual, 1).tolist() == ex['dual_level_1']
    assert pyramid_dual.tolist() == ex['pyramid_dual']


def check_dense(device):
    _, want, _ = check_dual(np.ones((8, 8, 8), dtype=bool), device)
    assert want.pyramid[0].tolist() == [(2 ** l + 1) ** 3 for l in range(4)] + [0]


TOUCHING = [([1, 1, 1], 1), ([1, 1, 0], 2), ([1, 0, 0], 4)]         # the second cell: at a corner, along an edge, across a face


def check_touching(device):
    for second, shared in TOUCHING:
        _, _, (_, pyramid, _, pyramid_dual, trinkets, _) = check_dual(bf.cube_of_points([[0, 0, 0], second], 1), device)
        assert pyramid_dual[0].tolist() == [8, 16 - shared, 0]
        a, b = (set(row) for row in trinkets[int(pyramid[1, 1]):].tolist())
        assert len(a) == 8 and len(b) == 8 and len(a & b) == shared


def test_fixture_cpu():
    check_fixture('cpu')


@pytest.mark.parametrize('level', [1, 4, 6])
def test_dual_of_random_cubes(level):
    check_dual(bf.random_cube(level, 20 + level), 'cpu')


def test_dual_of_the_dense_octree():
    check_dense('cpu')


def test_dual_of_touching_cells():
    check_touching('cpu')


def test_level_15_has_no_dual():
    S = spc()
    points = torch.tensor([[2 ** l - 1] * 3 for l in range(16)], dtype=torch.int16)
    pyramid = torch.tensor([[1] * 16 + [0], list(range(17))], dtype=torch.int32)
    with pytest.raises(ValueError, match='level 15'):
        S.unbatched_make_dual(points, pyramid)
    with pytest.raises(ValueError, match='level 15'):
        S.unbatched_make_trinkets(points, pyramid, points, pyramid)
    dual, pyramid_dual = S.unbatched_make_dual(points[:15], pyramid[:, :16].contiguous())      # level 14 is the deepest
    assert pyramid_dual[0].tolist() == [8] * 15 + [0] and dual[-1].tolist() == [16384] * 3


def test_a_pyramid_that_does_not_describe_the_points_is_rejected():
    S = spc()
    d = bf.decode(bf.random_cube(2, 3))
    points, pyramid = t(d.points, 'cpu'), t(d.pyramid, 'cpu')
    dual, pyramid_dual = S.unbatched_make_dual(points, pyramid)
    with pytest.raises(ValueError, match='does not describe'):
        S.unbatched_make_dual(points[:-1], pyramid)
    swapped = pyramid.clone()
    swapped[1, 1], swapped[1, 2] = pyramid[1, 2], pyramid[1, 1]                    # row 1 decreases, and disagrees with row 0
    with pytest.raises(ValueError, match='does not describe'):
        S.unbatched_make_dual(points, swapped)
    with pytest.raises(ValueError, match='does not describe'):
        S.unbatched_make_trinkets(points, swapped, dual, pyramid_dual)
    with pytest.raises(ValueError, match='pyramid_dual does not describe'):
        S.unbatched_make_trinkets(points, pyramid, dual[:-1], pyramid_dual)
    with pytest.raises(ValueError, match='no points'):
        S.unbatched_make_dual(points[:0], pyramid)
    with pytest.raises(ValueError, match='no points'):
        S.unbatched_make_trinkets(points, pyramid, dual[:0], pyramid_dual)


# --------------------------------------------------------------------------------------------------------------- coefficients
def test_coefficients_against_the_closed_form_and_the_alias():
    S = spc()
    rng = np.random.RandomState(5)
    level = 3
    points = rng.randint(0, 8, (50, 3)).astype(np.int16)
    for dtype, eps in ((torch.float32, EPS32), (torch.float64, EPS64)):
        coords = t(((points + rng.rand(50, 3)) / 8.0) * 2.0 - 1.0, 'cpu', dtype)
        want = dbf.coefficients(dbf.local(coords.numpy(), points, level))
        got = S.coords_to_trilinear_coeffs(coords, t(points, 'cpu'), level)
        assert got.dtype == dtype and tuple(got.shape) == (50, 8)
        assert np.abs(got.double().numpy() - want).max() <= 4 * eps                  # u, 1 - u and two products: four roundings
        assert abs(float(got.sum(dim=1).double().sub(1).abs().max())) <= 32 * eps
        shaped = S.coords_to_trilinear_coeffs(coords.reshape(5, 10, 3), t(points, 'cpu').reshape(5, 10, 3), level)
        assert tuple(shaped.shape) == (5, 10, 8) and torch.equal(shaped.reshape(50, 8), got)
    with pytest.warns(DeprecationWarning, match='coords_to_trilinear_coeffs'):
        old = S.coords_to_trilinear(coords, t(points, 'cpu'), level)
    assert torch.equal(old, got)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        S.coords_to_trilinear_coeffs(coords, t(points, 'cpu'), level)


def test_coefficients_gradcheck():
    S = spc()
    rng = np.random.RandomState(6)
    points = rng.randint(0, 4, (6, 3)).astype(np.int16)
    coords = t(((points + 0.1 + 0.8 * rng.rand(6, 3)) / 4.0) * 2.0 - 1.0, 'cpu', torch.float64).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda c: S.coords_to_trilinear_coeffs(c, t(points, 'cpu'), 2), (coords,))


# -------------------------------------------------------------------------------------------------------------- interpolation
class Case:
    """inputs of one interpolation, in numpy: coords (N, S, 3) float32, pidx (N) int32, feats (num_feats, D) in `dtype`, level"""


def make_case(d, dual, N, S, D, dtype, seed, misses='some', level=None):
    """N cells of `level` picked with repetition, S samples inside each; misses: 'none', 'some' (every third voxel) or 'all'"""
    rng = np.random.RandomState(seed)
    c = Case()
    c.level = d.level if level is None else level
    cells = d.level_points[c.level]
    first = int(d.pyramid[1, c.level])
    pick = rng.randint(0, len(cells), N)
    c.pidx = (first + pick).astype(np.int32)
    u = rng.rand(N, S, 3)
    c.coords = (((cells[pick][:, None, :] + u) / 2.0 ** c.level) * 2.0 - 1.0).astype(np.float32)
    if misses == 'all':
        c.pidx[:] = -1
    elif misses == 'some':
        c.pidx[::3] = -1
    num_feats = int(dual.pyramid[0, c.level])
    c.feats = (rng.rand(num_feats, D) * 2.0 - 1.0).astype({torch.float16: np.float16, torch.float32: np.float32,
                                                          torch.float64: np.float64}[dtype])
    c.grad = (rng.rand(N, S, D) * 2.0 - 1.0).astype(c.feats.dtype)
    c.dtype, c.points, c.trinkets = dtype, d.points, dual.trinkets
    return c


def forward_bound(corner_feats, result, dtype):
    """per output element: 64 * 2^-24 * max_k |f_k| (+ `half_rounding` for half).  Each float coefficient is off by at most 4 * 2^-24
    absolutely (u, 1 - u and two products), there are eight of them and they sum to one: 32 * 2^-24 * max |f|; the eight products
    and the seven additions add at most 8 * 2^-24 * max |f|; the rest is slack."""
    bound = 64 * EPS32 * np.abs(corner_feats).max(axis=1)[:, None, :]
    return bound + (half_rounding(result) if dtype == torch.float16 else 0.0)


def feats_bound(abs_sum, count, result, dtype):
    """per feature row and channel: (K + 8) * 2^-24 * sum_i |g_i| over the K contributing samples -- the error of a coefficient
    and of its product with g per term, plus the accumulation of K terms in any order.  Half adds `half_rounding`; double
    accumulates with 2^-53 but keeps the float coefficients."""
    if dtype == torch.float64:
        return (8 * EPS32 + count[:, None] * EPS64) * abs_sum
    bound = (count[:, None] + 8) * EPS32 * abs_sum
    return bound + (half_rounding(result) if dtype == torch.float16 else 0.0)


def coords_bound(scale, D):
    """per sample and axis: (D + 48) * 2^-24 * sum_d |g_d| max_k |f_kd|"""
    return ((D + 48) * EPS32 * scale)[..., None]


def tensors(c, device):
    return (t(c.coords, device), t(c.pidx, device), t(c.points, device), t(c.trinkets, device), t(c.feats, device))


def check_forward(c, device):
    """the public forward against the brute force (within `forward_bound`) and against the torch formulation run on the same
    tensors (torch.equal: the same unfused arithmetic; half after the one rounding of the float result) -> the result, on the CPU"""
    S = spc()
    coords, pidx, points, trinkets, feats = tensors(c, device)
    out = S.unbatched_interpolate_trilinear(coords, pidx, points, trinkets, feats, c.level)
    N, Sn, D = c.coords.shape[0], c.coords.shape[1], c.feats.shape[1]
    assert out.dtype == c.dtype and tuple(out.shape) == (N, Sn, D) and out.device.type == device
    want, corner_feats = dbf.interpolate(c.coords, c.pidx, c.points, c.trinkets, c.feats, c.level)
    err = np.abs(out.double().cpu().numpy() - want)
    bound = forward_bound(corner_feats, want, c.dtype)
    print(f'forward {c.dtype} N={N} S={Sn} D={D}: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0:.3f}')
    assert (err <= bound).all()
    assert (out[t(c.pidx, device) < 0] == 0).all()
    formulation = S.points._torch_interpolate_forward(coords, pidx, points, trinkets, feats, c.level)
    assert torch.equal(out, formulation)
    return out.cpu()


def check_backward(c, device, which=('coords', 'feats')):
    """both gradients of the public function against the brute force within `feats_bound` / `coords_bound`; exact zeros for
    misses and untouched rows -> (grad_coords, grad_feats) on the CPU (None where not asked for)"""
    S = spc()
    coords, pidx, points, trinkets, feats = tensors(c, device)
    coords.requires_grad_('coords' in which)
    feats.requires_grad_('feats' in which)
    out = S.unbatched_interpolate_trilinear(coords, pidx, points, trinkets, feats, c.level)
    out.backward(t(c.grad, device))
    D = c.feats.shape[1]
    want_feats, want_u, abs_sum, count, scale = dbf.interpolate_backward(c.coords, c.pidx, c.points, c.trinkets, c.feats, c.level,
                                                                         c.grad)
    if 'feats' in which:
        assert feats.grad.dtype == c.dtype and feats.grad.shape == feats.shape
        got = feats.grad.double().cpu().numpy()
        err, bound = np.abs(got - want_feats), feats_bound(abs_sum, count, want_feats, c.dtype)
        print(f'grad_feats {c.dtype} D={D}: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0:.3f}')
        assert (err <= bound).all() and (got[count == 0] == 0).all()
    else:
        assert feats.grad is None
    if 'coords' in which:
        assert coords.grad.dtype == torch.float32 and coords.grad.shape == coords.shape
        got = coords.grad.double().cpu().numpy()
        err, bound = np.abs(got - want_u), coords_bound(scale, D)
        print(f'grad_coords {c.dtype} D={D}: max err / bound = {float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0:.3f}')
        assert (err <= bound).all() and (got[c.pidx < 0] == 0).all()
    else:
        assert coords.grad is None
    return (coords.grad.cpu() if 'coords' in which else None, feats.grad.cpu() if 'feats' in which else None)


def check_exact_corners(device, dtype=torch.float32):
    """coordinates exactly on the low corner of a cell return that corner's row exactly, coordinates on the high faces the
    opposite corners: there every coefficient is exactly 0 or 1"""
    S = spc()
    d = bf.decode(bf.random_cube(3, 31))
    dual = dbf.make_dual(d)
    c = make_case(d, dual, 40, 1, 5, dtype, 32, misses='none')
    cells = c.points[c.pidx].astype(np.float64)
    for corner in range(8):
        offset = np.array([corner >> 2, (corner >> 1) & 1, corner & 1], dtype=np.float64)
        c.coords = (((cells + offset) / 8.0) * 2.0 - 1.0).astype(np.float32)[:, None, :]          # exact in float
        coords, pidx, points, trinkets, feats = tensors(c, device)
        out = S.unbatched_interpolate_trilinear(coords, pidx, points, trinkets, feats, c.level)
        assert torch.equal(out[:, 0], feats[trinkets[pidx.long()][:, corner].long()])


@pytest.fixture(scope='module')
def grid():
    d = bf.decode(bf.random_cube(4, 41))
    return d, dbf.make_dual(d)


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32, torch.float64])
@pytest.mark.parametrize('S', [1, 3])
def test_interpolate_forward_cpu(grid, S, dtype):
    for D in (1, 16, 33):
        check_forward(make_case(*grid, 50, S, D, dtype, 100 + D), 'cpu')
    check_forward(make_case(*grid, 0, S, 3, dtype, 1), 'cpu')
    check_forward(make_case(*grid, 7, S, 3, dtype, 2, misses='all'), 'cpu')
    check_forward(make_case(*grid, 20, S, 4, dtype, 3, level=2), 'cpu')


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32, torch.float64])
@pytest.mark.parametrize('S', [1, 3])
def test_interpolate_backward_cpu(grid, S, dtype):
    for D in (1, 16, 33):
        check_backward(make_case(*grid, 50, S, D, dtype, 200 + D), 'cpu')
    check_backward(make_case(*grid, 20, S, 4, dtype, 4, level=2), 'cpu')


def test_interpolate_needs_input_grad_cpu(grid):
    check_backward(make_case(*grid, 9, 2, 3, torch.float32, 5), 'cpu', which=('feats',))
    check_backward(make_case(*grid, 9, 2, 3, torch.float32, 6), 'cpu', which=('coords',))


def test_interpolate_exact_corners_cpu():
    check_exact_corners('cpu')


def test_interpolate_gradcheck(grid):
    """float64 coordinates and features on the torch formulation.  The gradient by coords is the derivative by the LOCAL coordinate:
    at level 1 that is the derivative by coords itself (2^(level - 1) = 1), which gradcheck can see; at other levels
    `check_backward` compares it with the closed form."""
    S = spc()
    d, dual = grid
    c = make_case(d, dual, 6, 2, 3, torch.float64, 7)
    args = [t(c.pidx, 'cpu'), t(c.points, 'cpu'), t(c.trinkets, 'cpu')]
    coords, feats = t(c.coords, 'cpu', torch.float64), t(c.feats, 'cpu').requires_grad_(True)
    assert torch.autograd.gradcheck(lambda f: S.unbatched_interpolate_trilinear(coords, *args, f, c.level), (feats,))
    d1 = bf.decode(np.ones((2, 2, 2), dtype=bool))
    c = make_case(d1, dbf.make_dual(d1), 6, 2, 3, torch.float64, 8)
    inside = ((c.points[np.maximum(c.pidx, 0)][:, None, :] + 0.1 + 0.8 * np.random.RandomState(9).rand(6, 2, 3)) / 2.0) * 2.0 - 1.0
    coords = t(inside, 'cpu', torch.float64).requires_grad_(True)
    args = [t(c.pidx, 'cpu'), t(c.points, 'cpu'), t(c.trinkets, 'cpu')]
    feats = t(c.feats, 'cpu')
    assert torch.autograd.gradcheck(lambda x: S.unbatched_interpolate_trilinear(x, *args, feats, 1), (coords,))


def test_out_of_range_indices_are_misses(grid):
    """a stale pidx / trinkets pair: zeros and zero gradients, nothing else changes.  On the CPU only."""
    S = spc()
    d, dual = grid
    c = make_case(d, dual, 12, 2, 4, torch.float32, 10, misses='none')
    coords, pidx, points, trinkets, feats = tensors(c, 'cpu')
    good = S.unbatched_interpolate_trilinear(coords, pidx, points, trinkets, feats, c.level)
    bad_pidx = pidx.clone()
    bad_pidx[0], bad_pidx[1], bad_pidx[2] = points.shape[0], -5, 2 ** 31 - 1
    bad_trinkets = trinkets.clone()
    bad_trinkets[pidx[3].long(), 7] = feats.shape[0]
    bad_trinkets[pidx[4].long(), 0] = -1
    stale = (bad_pidx[:5] != pidx[:5]) | torch.tensor([False, False, False, True, True])
    stale = torch.cat([stale, torch.zeros(7, dtype=torch.bool)]) | (pidx == pidx[3]) | (pidx == pidx[4])
    coords.requires_grad_(True)
    feats.requires_grad_(True)
    out = S.unbatched_interpolate_trilinear(coords, bad_pidx, points, bad_trinkets, feats, c.level)
    assert (out[stale] == 0).all() and torch.equal(out[~stale], good[~stale])
    out.sum().backward()
    assert (coords.grad[stale] == 0).all() and torch.isfinite(feats.grad).all()
    kept = torch.zeros(feats.shape[0], dtype=torch.bool)
    kept[trinkets[pidx[~stale].long()].long().reshape(-1)] = True
    assert (feats.grad[~kept] == 0).all()


def test_arguments_are_checked():
    S = spc()
    d = bf.decode(bf.random_cube(2, 11))
    c = make_case(d, dbf.make_dual(d), 4, 1, 2, torch.float32, 12)
    coords, pidx, points, trinkets, feats = tensors(c, 'cpu')
    with pytest.raises(ValueError, match='pidx'):
        S.unbatched_interpolate_trilinear(coords, pidx.long(), points, trinkets, feats, c.level)
    with pytest.raises(ValueError, match='coords'):
        S.unbatched_interpolate_trilinear(coords[:, 0], pidx, points, trinkets, feats, c.level)
    with pytest.raises(ValueError, match='trinkets'):
        S.unbatched_interpolate_trilinear(coords, pidx, points, trinkets[:-1], feats, c.level)
    with pytest.raises(ValueError, match='feats'):
        S.unbatched_interpolate_trilinear(coords, pidx, points, trinkets, feats.long(), c.level)
