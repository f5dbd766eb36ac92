"""render.spc through the HIP path (csrc/spc_raytrace.hip) against the numpy oracle of tests/spc_raytrace_oracle.py: the cases of
tests/test_render_spc_cpu.py on CUDA tensors, plus the smallest shapes at which each kernel can go wrong.  Every comparison is
torch.equal.  No malformed octree is run on the GPU."""
import numpy as np
import pytest
import torch

import spc_raytrace_oracle as ro
from test_render_spc_cpu import (case, check_exponential_integration, check_pack_backward, check_pack_ops, check_trace, dense_scene,
                                 fixture, golden_rays, golden_scene, pack_case, rspc, scene_args, t)

pytestmark = pytest.mark.gpu

SCAN_BLOCK = 1024       # counts per block of the scan of the hit counts (csrc/sort_scan.h)


# ------------------------------------------------------------------------------------------------------------------------ tracing
@pytest.mark.parametrize('name', ['positive', 'negative', 'none', 'coarser'])
def test_trace_golden_scenes(name):
    doc = fixture()
    nuggets = check_trace(name, 'cuda')
    assert nuggets.tolist() == doc[name]['nuggets']


def test_trace_golden_depths_shapes_and_views():
    R, doc = rspc(), fixture()
    scene = golden_scene()
    origin, direction = golden_rays(doc, 'negative')
    args = scene_args(scene, 'cuda') + (t(origin, 'cuda'), t(direction, 'cuda'), 2)
    ridx, pidx, depth = R.unbatched_raytrace(*args, with_exit=True)
    assert depth[:, 0].tolist() == doc['negative']['entry'] and depth[:, 1].tolist() == doc['negative']['exit']
    assert ridx.stride() == (2,) and ridx.data_ptr() + 4 == pidx.data_ptr()      # the two columns of one tensor
    origin, direction = golden_rays(doc, 'none')
    out = R.unbatched_raytrace(*scene_args(scene, 'cuda'), t(origin, 'cuda'), t(direction, 'cuda'), 2, with_exit=True)
    assert [list(x.shape) for x in out] == doc['none']['shapes']
    empty = torch.zeros((0, 3), device='cuda')
    ridx, pidx, depth = R.unbatched_raytrace(*scene_args(scene, 'cuda'), empty, empty, 2)
    assert ridx.shape == (0,) and pidx.shape == (0,) and depth.shape == (0, 1) and depth.is_cuda


def test_trace_level_0():
    assert check_trace('level0', 'cuda').tolist() == [[0, 0]]       # the root is hit; the origin inside it gives nothing


def test_trace_deepest_walk_state():
    assert check_trace('chain15', 'cuda').tolist() == [[0, 15]]     # 15 levels of state; the parallel ray misses


def test_trace_dense_level_3_ties():
    nuggets = check_trace('dense3', 'cuda')
    assert (nuggets[:, 0] == 0).sum() == 8 and (nuggets[:, 0] == 1).sum() == 8


def test_trace_random_perspective_rays():
    nuggets = check_trace('random600', 'cuda')
    assert len(nuggets) > 600


@pytest.mark.parametrize('rays', [1, 63, 64, 65, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1])
def test_trace_at_the_wave_and_scan_block_edges(rays):
    nuggets = check_trace('edges1025', 'cuda', rays=rays)
    assert rays < 3 or len(np.unique(nuggets[:, 0])) < rays         # some rays are empty


def test_trace_all_rays_miss():
    assert len(check_trace('all_miss', 'cuda')) == 0


def test_trace_second_level_of_the_scan():
    """more scan blocks than a block has threads: copies of one axis ray through the dense octree of level 1 -- two hits each"""
    R = rspc()
    scene = dense_scene(1)
    n = SCAN_BLOCK * SCAN_BLOCK + SCAN_BLOCK + 1
    one = ro.trace(scene, [[-2, 0.5, 0.5]], [[1, 0, 0]], 1)[0]
    assert one.tolist() == [[0, 4], [0, 8]]                         # the children (0, 1, 1) and (1, 1, 1) of the root, front to back
    origin = torch.tensor([[-2, 0.5, 0.5]], device='cuda').expand(n, 3).contiguous()
    direction = torch.tensor([[1.0, 0, 0]], device='cuda').expand(n, 3).contiguous()
    ridx, pidx = R.unbatched_raytrace(*scene_args(scene, 'cuda'), origin, direction, 1, return_depth=False)
    assert torch.equal(ridx, torch.arange(n, dtype=torch.int32, device='cuda').repeat_interleave(2))
    assert torch.equal(pidx, torch.tensor(one[:, 1].tolist(), dtype=torch.int32, device='cuda').repeat(n))


def test_trace_value_errors_of_the_shim():
    R = rspc()
    scene, origin, direction, level, _ = case('positive')
    octree, points, pyramid, exsum = scene_args(scene, 'cuda')
    o, d = t(origin, 'cuda'), t(direction, 'cuda')
    for bad in (-1, 3, 16):
        with pytest.raises(ValueError, match='level'):
            R.unbatched_raytrace(octree, points, pyramid, exsum, o, d, bad)
    with pytest.raises(ValueError, match='float32'):
        R.unbatched_raytrace(octree, points, pyramid, exsum, o.double(), d, 2)
    with pytest.raises(ValueError, match='origins for'):
        R.unbatched_raytrace(octree, points, pyramid, exsum, o[:5], d, 2)
    with pytest.raises(ValueError, match='one GPU'):
        R.unbatched_raytrace(octree, points, pyramid, exsum, o.cpu(), d, 2)
    with pytest.raises(ValueError, match='legacy'):
        R.unbatched_raytrace(octree, points, pyramid, torch.cat([exsum.new_zeros(1), exsum]), o, d, 2)


# -------------------------------------------------------------------------------------------------------------------- pack operators
@pytest.mark.parametrize('dtype_name', ['float32', 'float64'])
@pytest.mark.parametrize('C', [1, 3, 65])
@pytest.mark.parametrize('layout', ['single', 'each', 'mixed'])
def test_pack_ops(layout, C, dtype_name):
    check_pack_ops(layout, dtype_name, C, 'cuda')


@pytest.mark.parametrize('dtype_name', ['float32', 'float64'])
def test_pack_backward(dtype_name):
    check_pack_backward(dtype_name, 'cuda')


@pytest.mark.parametrize('dtype_name', ['float32', 'float64'])
def test_exponential_integration(dtype_name):
    check_exponential_integration(dtype_name, 'cuda')


def test_reference_operator_signatures():
    """the reference's Python layer passes the list of pack starts and the inclusive sum"""
    import kaolin_amd as kal
    C = kal._C.render.spc
    feats_np, b_np = pack_case('mixed', 'float32', 3)
    feats, b = t(feats_np, 'cuda'), t(b_np, 'cuda')
    starts = torch.nonzero(b).int().contiguous()[..., 0]
    assert torch.equal(C.cumsum_cuda(feats, starts, True, False).cpu(), t(ro.pack_scan(feats_np, b_np, False, True, False), 'cpu'))
    assert torch.equal(C.cumprod_cuda(feats, starts, False, True).cpu(), t(ro.pack_scan(feats_np, b_np, True, False, True), 'cpu'))
    isum = C.inclusive_sum_cuda(b.int())
    assert isum.dtype == torch.int32 and isum.tolist() == np.cumsum(b_np).tolist()
    assert torch.equal(C.sum_reduce_cuda(feats, isum).cpu(), t(ro.pack_reduce(feats_np, b_np, False), 'cpu'))
    assert C.mark_pack_boundaries_cuda(isum).dtype == torch.int32
    assert torch.equal(C.diff_cuda(feats, torch.nonzero(b)[..., 0]), kal.render.spc.diff(feats, b))


def test_cumsum_graph_capture():
    R = rspc()
    feats_np, b_np = pack_case('mixed', 'float32', 3)
    feats, b = t(feats_np, 'cuda'), t(b_np, 'cuda')
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        R.cumsum(feats, b, exclusive=True)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = R.cumsum(feats, b, exclusive=True)
        out_reverse = R.cumprod(feats, b, reverse=True)
    fresh = np.random.RandomState(8).uniform(0.9, 1.1, feats_np.shape).astype(np.float32)
    feats.copy_(t(fresh, 'cuda'))
    out.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), t(ro.pack_scan(fresh, b_np, False, True, False), 'cpu'))
    assert torch.equal(out_reverse.cpu(), t(ro.pack_scan(fresh, b_np, True, False, True), 'cpu'))


# ------------------------------------------------------------------------------------------------------------------------ integration
def test_mesh_to_image_integration():
    """mesh -> octree -> scan -> points -> trace over a 32 x 32 camera -> exponential integration"""
    import kaolin_amd as kal
    from kaolin_amd.utils import testing as T
    level = 5
    vertices, faces = T.geodesic_sphere(8, radius=0.8)
    face_vertices = vertices[faces].float().cuda().contiguous()
    octree = kal._C.ops.conversions.mesh_to_spc_cuda(face_vertices, level)[0]
    lengths = torch.tensor([octree.numel()], dtype=torch.int32)
    max_level, pyramids, exsum = kal.ops.spc.scan_octrees(octree, lengths)
    assert max_level == level
    points = kal.ops.spc.generate_points(octree, pyramids, exsum)
    ii, jj = torch.meshgrid(torch.linspace(-0.6, 0.6, 32), torch.linspace(-0.6, 0.6, 32), indexing='ij')
    origin = torch.tensor([0.3, -0.2, -3.0]).expand(1024, 3).contiguous().cuda()
    direction = torch.stack([ii.reshape(-1), jj.reshape(-1), torch.zeros(1024)], dim=1).cuda() - origin      # towards the plane z = 0
    direction = (direction / direction.norm(dim=1, keepdim=True)).contiguous()
    ridx, pidx, depth = kal.render.spc.unbatched_raytrace(octree, points, pyramids[0], exsum, origin, direction, level)
    assert len(ridx) > 1024                                           # the sphere fills most of the view, front and back
    first, last = int(pyramids[0, 1, level]), int(pyramids[0, 1, level + 1])
    assert int(pidx.min()) >= first and int(pidx.max()) < last       # every hit is a point of `level`
    assert (ridx[1:] >= ridx[:-1]).all()
    # the entry point lies in the hit voxel, to within one voxel
    entry = origin[ridx.long()] + depth * direction[ridx.long()]
    centre = (points[pidx.long()].float() + 0.5) * (2.0 / 2 ** level) - 1.0
    assert float((entry - centre).abs().max()) <= 2.0 / 2 ** level
    boundaries = kal.render.spc.mark_pack_boundaries(ridx)
    tau = torch.full((len(ridx), 1), 0.5, device='cuda')
    colour = centre * 0.5 + 0.5
    image, transmittance = kal.render.spc.exponential_integration(colour, tau, boundaries)
    assert image.shape == (int(boundaries.sum()), 3) and transmittance.shape == (len(ridx), 1)
    assert torch.isfinite(image).all() and float(image.min()) >= 0 and float(image.max()) <= 1
