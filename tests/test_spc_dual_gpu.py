"""ops.spc feature grids through the HIP path (csrc/spc_trilinear.hip): the `check_*` helpers of tests/test_spc_dual_cpu.py on CUDA
tensors, at the smallest shapes at which each kernel can go wrong.  Dual, trinkets and parents are compared with torch.equal;
float32 / float64 forwards with torch.equal against the torch formulation on the same tensors and against the CPU path; everything
against the float64 brute force within the derived bounds of test_spc_dual_cpu.py.  No out-of-range index, malformed hierarchy or
level-15 dual is launched on the GPU."""
import numpy as np
import pytest
import torch

import spc_bruteforce as bf
import spc_dual_bruteforce as dbf
from test_spc_dual_cpu import (check_backward, check_dense, check_dual, check_exact_corners, check_fixture, check_forward,
                               check_invariant, check_touching, cube_with_points, feats_bound, forward_bound, make_case, spc, t,
                               tensors)

pytestmark = pytest.mark.gpu

SORT_TILE = 2048        # keys per block of the radix sort (csrc/sort_scan_host.h SS_SORT_BLOCK): 8 keys a point -> 256 points
BLOCK_POINTS = 32       # points per 256-thread block of the trinket kernel: a thread per (point, corner)


@pytest.fixture(scope='module')
def grid():
    d = bf.decode(bf.random_cube(4, 41))
    return d, dbf.make_dual(d)


# ------------------------------------------------------------------------------------------------------------ dual and trinkets
def test_fixture_gpu():
    check_fixture('cuda')


def test_dual_of_a_single_cell():
    _, want, _ = check_dual(bf.cube_of_points([[1, 0, 1]], 1), 'cuda')
    assert want.pyramid[0].tolist() == [8, 8, 0]


@pytest.mark.parametrize('num_points', [SORT_TILE // 8 - 1, SORT_TILE // 8, SORT_TILE // 8 + 1])
def test_dual_across_the_sort_tile(num_points):
    d, _, _ = check_dual(cube_with_points(4, num_points, num_points), 'cuda')
    assert len(d.points) == num_points


@pytest.mark.parametrize('num_points', [BLOCK_POINTS - 1, BLOCK_POINTS, BLOCK_POINTS + 1, 2 * BLOCK_POINTS - 1, 2 * BLOCK_POINTS,
                                        2 * BLOCK_POINTS + 1])
def test_trinkets_around_the_block(num_points):
    """hierarchies that end just before, on and just after a block of the trinket kernel; the starts of their levels fall inside
    the blocks, so that one block searches the ranges of several levels"""
    d, _, _ = check_dual(cube_with_points(3, num_points, num_points), 'cuda')
    assert len(d.points) == num_points


def test_dual_of_a_chain_to_level_14():
    """one cell per level down to (16383, 16383, 16383): the corners reach 16384, the 15th bit of a coordinate.  The 8 corners
    of an all-ones cell are in Morton order as they stand."""
    S = spc()
    points = torch.tensor([[2 ** l - 1] * 3 for l in range(15)], dtype=torch.int16, device='cuda')
    pyramid = torch.tensor([[1] * 15 + [0], list(range(16))], dtype=torch.int32)
    dual, pyramid_dual = S.unbatched_make_dual(points, pyramid)
    assert pyramid_dual.tolist() == [[8] * 15 + [0], [8 * l for l in range(16)]]
    assert torch.equal(dual, S.points_to_corners(points).reshape(-1, 3)) and dual[-1].tolist() == [16384] * 3
    trinkets, parents = S.unbatched_make_trinkets(points, pyramid, dual, pyramid_dual)
    assert trinkets.tolist() == [list(range(8))] * 15 and parents.tolist() == list(range(-1, 14))
    check_invariant(S, points, pyramid, dual, pyramid_dual, trinkets, parents)


def test_dual_of_the_dense_octree_gpu():
    check_dense('cuda')


def test_dual_of_touching_cells_gpu():
    check_touching('cuda')


@pytest.mark.parametrize('level', [1, 4, 6])
def test_dual_of_random_cubes_gpu(level):
    check_dual(bf.random_cube(level, 20 + level), 'cuda')


@pytest.fixture(scope='module')
def sphere():
    """the octree of unbatched_mesh_to_spc for the geodesic sphere at level 7, with its dual and trinkets"""
    import kaolin_amd as kal
    from kaolin_amd.utils.testing import geodesic_sphere
    S = spc()
    v, f = geodesic_sphere(8)
    octree = kal.ops.conversions.unbatched_mesh_to_spc((v.float() * 1.2)[f].contiguous().cuda(), 7)[0]
    _, pyramids, exsum = S.scan_octrees(octree, torch.tensor([octree.numel()], dtype=torch.int32))
    points = S.generate_points(octree, pyramids, exsum)
    dual, pyramid_dual = S.unbatched_make_dual(points, pyramids[0])
    trinkets, parents = S.unbatched_make_trinkets(points, pyramids[0], dual, pyramid_dual)
    return octree, exsum, points, pyramids[0], dual, pyramid_dual, trinkets, parents


def test_sphere_octree_invariant(sphere):
    octree, exsum, points, pyramid, dual, pyramid_dual, trinkets, parents = sphere
    S = spc()
    assert pyramid.shape[1] == 9 and int(pyramid_dual[1, 8]) == dual.shape[0] > points.shape[0]
    check_invariant(S, points, pyramid, dual, pyramid_dual, trinkets, parents)
    cpu_dual, cpu_pyramid_dual = S.unbatched_make_dual(points.cpu(), pyramid)                    # ... and the CPU path
    assert torch.equal(cpu_pyramid_dual, pyramid_dual) and torch.equal(cpu_dual, dual.cpu())


# -------------------------------------------------------------------------------------------------------- interpolation, forward
@pytest.mark.parametrize('dtype', [torch.float16, torch.float32, torch.float64])
@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('D', [1, 3, 16, 32, 33])
def test_interpolate_forward(grid, D, S, dtype):
    for N in (0, 1, 255, 256, 257):
        c = make_case(*grid, N, S, D, dtype, 1000 + N + D)
        assert torch.equal(check_forward(c, 'cuda'), check_forward(c, 'cpu'))


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32, torch.float64])
def test_interpolate_forward_all_misses_and_inner_level(grid, dtype):
    out = check_forward(make_case(*grid, 70, 2, 16, dtype, 3, misses='all'), 'cuda')
    assert (out == 0).all()
    c = make_case(*grid, 70, 2, 6, dtype, 4, misses='none', level=2)
    assert torch.equal(check_forward(c, 'cuda'), check_forward(c, 'cpu'))


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32, torch.float64])
def test_interpolate_exact_corners(dtype):
    check_exact_corners('cuda', dtype)


def test_interpolate_with_pidx_of_query_and_raytrace(sphere):
    """pidx as unbatched_query (cast to int32) and unbatched_raytrace return it, on the sphere's octree at level 7: against the
    brute-force interpolation, and the torch formulation on the same tensors"""
    import kaolin_amd as kal
    S = spc()
    octree, exsum, points, pyramid, dual, pyramid_dual, trinkets, _ = sphere
    level, D = 7, 16
    gen = torch.Generator().manual_seed(0)
    feats = (torch.rand((int(pyramid_dual[0, level]), D), generator=gen) * 2 - 1).cuda()
    leaves = S.unbatched_get_level_points(points, pyramid, level)
    pick = torch.randint(0, leaves.shape[0], (500,), generator=gen).cuda()
    inside = ((leaves[pick].float() + torch.rand((500, 3), generator=gen).cuda()) / 2 ** level) * 2 - 1
    coords = torch.cat([inside, (torch.rand((500, 3), generator=gen) * 2 - 1).cuda()])
    pidx = S.unbatched_query(octree, exsum, coords, level).int()
    assert int((pidx >= 0).sum()) >= 490 and int((pidx < 0).sum()) > 0
    origin = torch.tensor([[0.0, 0.0, -3.0]]).repeat(300, 1).cuda()
    target = (torch.rand((300, 3), generator=gen) * 1.6 - 0.8).cuda()
    direction = torch.nn.functional.normalize(target - origin, dim=1)
    ridx, ray_pidx, depth = kal.render.spc.unbatched_raytrace(octree, points, pyramid, exsum, origin, direction, level)
    assert ray_pidx.dtype == torch.int32 and ray_pidx.numel() > 0
    hits = origin[ridx.long()] + direction[ridx.long()] * depth[:, :1]
    for c, p in ((coords[:, None, :], pidx), (hits[:, None, :].contiguous(), ray_pidx.contiguous())):
        out = S.unbatched_interpolate_trilinear(c, p, points, trinkets, feats, level)
        assert torch.equal(out, S.points._torch_interpolate_forward(c, p, points, trinkets, feats, level))
        want, corner = dbf.interpolate(c.cpu().numpy(), p.cpu().numpy(), points.cpu().numpy(), trinkets.cpu().numpy(),
                                       feats.cpu().numpy(), level)
        # (the entry point of a ray lies on its cell's face, up to rounding: the bound's coefficients may leave [0, 1] by that much)
        assert (np.abs(out.double().cpu().numpy() - want) <= forward_bound(corner, want, torch.float32)).all()


# ------------------------------------------------------------------------------------------------------- interpolation, backward
@pytest.mark.parametrize('dtype', [torch.float16, torch.float32, torch.float64])
@pytest.mark.parametrize('S', [1, 3])
@pytest.mark.parametrize('D', [1, 16, 33])
def test_interpolate_backward(grid, D, S, dtype):
    for N in (0, 1, 255, 256, 257):
        check_backward(make_case(*grid, N, S, D, dtype, 2000 + N + D), 'cuda')


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32, torch.float64])
def test_interpolate_backward_contention(grid, dtype):
    """4096 samples in ONE voxel: all of them add into the same eight rows -- as 4096 voxels of one sample (one atomic per voxel
    and row) and as one voxel of 4096 samples (summed in registers first)"""
    d, dual = grid
    for N, S in ((4096, 1), (1, 4096)):
        c = make_case(d, dual, N, S, 16, dtype, 5, misses='none')
        cell = int(c.pidx[0])
        u = np.random.RandomState(6).rand(N, S, 3)
        c.pidx[:] = cell
        c.coords = (((d.points[cell][None, None, :] + u) / 2.0 ** c.level) * 2.0 - 1.0).astype(np.float32)
        check_backward(c, 'cuda')


def test_interpolate_backward_all_misses(grid):
    grad_coords, grad_feats = check_backward(make_case(*grid, 70, 2, 16, torch.float32, 7, misses='all'), 'cuda')
    assert (grad_coords == 0).all() and (grad_feats == 0).all()


def test_interpolate_needs_input_grad(grid):
    check_backward(make_case(*grid, 100, 2, 16, torch.float32, 8), 'cuda', which=('feats',))
    check_backward(make_case(*grid, 100, 2, 16, torch.float32, 9), 'cuda', which=('coords',))


# ------------------------------------------------------------------------------------------------------------------ graph capture
def test_interpolate_replays_in_a_graph(grid):
    """forward + gradient by feats captured on one stream and replayed: the forward equals the eager one, the gradient stays within
    its bound (float atomics).  The eager reference runs on its own leaf and keeps no autograd graph: a graph built on the default
    stream keeps the leaf's AccumulateGrad node bound to that stream, and a capture that reuses the node makes the default
    stream wait for the capturing one -- a capture that can never be joined."""
    S = spc()
    c = make_case(*grid, 300, 2, 16, torch.float32, 10)
    coords, pidx, points, trinkets, feats = tensors(c, 'cuda')
    grad_out = t(c.grad, 'cuda')

    def make_step(leaf, out):
        def step():
            res = S.unbatched_interpolate_trilinear(coords, pidx, points, trinkets, leaf, c.level)
            (grad,) = torch.autograd.grad(res, [leaf], grad_out)
            for k, v in (('out', res), ('grad', grad)):
                if k in out:
                    out[k].copy_(v.detach())
                else:
                    out[k] = v.detach().clone()
        return step
    eager = {}
    make_step(feats.clone().requires_grad_(), eager)()
    out = {}
    step = make_step(feats.clone().requires_grad_(), out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for k in out:
        out[k].fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out['out'], eager['out'])
    want, _, abs_sum, count, _ = dbf.interpolate_backward(c.coords, c.pidx, c.points, c.trinkets, c.feats, c.level, c.grad)
    for got in (out['grad'], eager['grad']):
        assert (np.abs(got.double().cpu().numpy() - want) <= feats_bound(abs_sum, count, want, torch.float32)).all()


# ---------------------------------------------------------------------------------------------------------------------- shims
def test_coefficients_gpu():
    S = spc()
    rng = np.random.RandomState(11)
    for n in (0, 1, 255, 256, 257):
        points = rng.randint(0, 32, (n, 3)).astype(np.int16)
        for dtype in (torch.float16, torch.float32, torch.float64):
            coords = t(((points + rng.rand(n, 3)) / 32.0) * 2.0 - 1.0, 'cpu', dtype)
            got = S.coords_to_trilinear_coeffs(coords.cuda(), t(points, 'cuda'), 5)
            assert got.dtype == dtype and torch.equal(got.cpu(), S.coords_to_trilinear_coeffs(coords, t(points, 'cpu'), 5))


def test_shims_reject_cpu_tensors(grid):
    import kaolin_amd as kal
    C = kal._C.ops.spc
    d, dual = grid
    c = make_case(d, dual, 4, 1, 2, torch.float32, 12)
    coords, pidx, points, trinkets, feats = tensors(c, 'cpu')
    pyramid, pyramid_dual, dual_points = t(d.pyramid, 'cpu'), t(dual.pyramid, 'cpu'), t(dual.points, 'cpu')
    grad = t(c.grad, 'cpu')
    for call in (lambda: C.make_dual_cuda(points, pyramid), lambda: C.make_trinkets_cuda(points, pyramid, dual_points, pyramid_dual),
                 lambda: C.coords_to_trilinear_cuda(coords[:, 0], points[:4], 4),
                 lambda: C.interpolate_trilinear_cuda(coords, pidx, points, trinkets, feats, 4),
                 lambda: C.interpolate_trilinear_backward_feats_cuda(coords, pidx, points, trinkets, feats, 4, grad),
                 lambda: C.interpolate_trilinear_backward_coords_cuda(coords, pidx, points, trinkets, feats, 4, grad)):
        with pytest.raises(RuntimeError, match='CUDA'):
            call()


def test_level_15_is_refused_before_any_launch():
    S = spc()
    points = torch.zeros((16, 3), dtype=torch.int16, device='cuda')
    pyramid = torch.tensor([[1] * 16 + [0], list(range(17))], dtype=torch.int32)
    with pytest.raises(ValueError, match='level 15'):
        S.unbatched_make_dual(points, pyramid)


def test_bad_arguments_are_refused_before_any_launch(grid):
    """the public checks are the same for both devices: a pyramid that does not describe its hierarchy, and float64 coords (which
    only the CPU path takes), raise ValueError"""
    S = spc()
    d, dual = grid
    c = make_case(d, dual, 4, 1, 2, torch.float32, 13)
    coords, pidx, points, trinkets, feats = tensors(c, 'cuda')
    with pytest.raises(ValueError, match='does not describe'):
        S.unbatched_make_dual(points[:-1], t(d.pyramid, 'cpu'))
    with pytest.raises(ValueError, match='no points'):
        S.unbatched_make_dual(points[:0], t(d.pyramid, 'cpu'))
    with pytest.raises(ValueError, match='float32'):
        S.unbatched_interpolate_trilinear(coords.double(), pidx, points, trinkets, feats, c.level)


def test_half_gradient_does_not_depend_on_recycled_memory(grid):
    """the float32 sums of the half gradient live in a buffer of the call: with the allocator's free blocks full of NaN bits before
    each call, two calls give gradients within the bound of each other's reference"""
    c = make_case(*grid, 257, 3, 33, torch.float16, 14)
    for _ in range(2):
        junk = [torch.full((n,), -1, dtype=torch.int32, device='cuda') for n in (1024, 16384, 131072) for _ in range(4)]
        del junk
        check_backward(c, 'cuda', which=('feats',))
