"""ops.spc through the HIP path (csrc/spc.hip) against the brute-force decoder of tests/spc_bruteforce.py: the cases of
tests/test_spc_cpu.py on CUDA tensors, plus the smallest shapes at which each kernel can go wrong.  Every comparison is
torch.equal.  No malformed octree is run on the GPU."""
import numpy as np
import pytest
import torch

import oracle
import spc_bruteforce as bf
from test_spc_cpu import (check_feature_grid_round_trip, check_fixture, check_pipeline, check_queries, check_to_dense_backward,
                          cubes_for, spc, t)

pytestmark = pytest.mark.gpu

SCAN_BLOCK = 1024       # bytes per block of the scan (csrc/spc.hip SP_SCAN_BLOCK)
SORT_TILE = 2048        # keys per block of the radix sort (csrc/sort_scan_host.h SS_SORT_BLOCK)


def cube_with_bytes(level, num_bytes, seed):
    """a random cube of `level` whose octree has exactly `num_bytes` bytes (= occupied cells above the last level): cells are
    added while they do not overshoot; a cell next to an occupied one adds a single byte, so the target is always reached"""
    rng = np.random.RandomState(seed)
    seen = [set() for _ in range(level)]
    cube = np.zeros((2 ** level,) * 3, dtype=bool)
    total = 0
    while total < num_bytes:
        p = rng.randint(0, 2 ** level, 3)
        new = [l for l in range(level) if tuple(p >> (level - l)) not in seen[l]]
        if total + len(new) <= num_bytes:
            for l in new:
                seen[l].add(tuple(p >> (level - l)))
            total += len(new)
            cube[tuple(p)] = True
    return cube


def check_scan_generate(cubes):
    S = spc()
    ds, octrees_np, lengths_np, pyramids_np, exsum_np, points_np = bf.decode_batch(cubes)
    octrees, lengths = t(octrees_np, 'cuda'), t(lengths_np, 'cpu')
    max_level, pyramids, exsum = S.scan_octrees(octrees, lengths)
    assert max_level == ds[0].level and torch.equal(pyramids, t(pyramids_np, 'cpu'))
    assert exsum.dtype == torch.int32 and torch.equal(exsum.cpu(), t(exsum_np, 'cpu'))
    points = S.generate_points(octrees, pyramids, exsum)
    assert points.dtype == torch.int16 and torch.equal(points.cpu(), t(points_np, 'cpu'))
    return lengths_np


def test_fixture_gpu():
    check_fixture('cuda')


# ------------------------------------------------------------------------------------------------------------------------ scan
@pytest.mark.parametrize('num_bytes', [SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1])
def test_scan_at_the_block_size(num_bytes):
    assert check_scan_generate([cube_with_bytes(5, num_bytes, num_bytes)]).tolist() == [num_bytes]


def test_scan_item_boundaries_inside_and_on_a_block():
    lengths = check_scan_generate([cube_with_bytes(5, n, n) for n in (SCAN_BLOCK - 1, SCAN_BLOCK + 1, 300)])
    assert lengths.tolist() == [SCAN_BLOCK - 1, SCAN_BLOCK + 1, 300]      # boundaries at 1023 (inside a block) and 2048 (on one)


def test_scan_second_level_of_block_sums():
    """more blocks than a block has threads: the dense octree of level 8 (2 396 745 bytes); its answers are closed forms"""
    S = spc()
    octree, lengths = S.create_dense_spc(8, 'cuda')
    assert int(lengths[0]) > SCAN_BLOCK * SCAN_BLOCK
    max_level, pyramids, exsum = S.scan_octrees(octree, lengths)
    assert max_level == 8
    assert pyramids[0, 0].tolist() == [8 ** l for l in range(9)] + [0]
    assert pyramids[0, 1].tolist() == [sum(8 ** k for k in range(l)) for l in range(10)]
    assert torch.equal(exsum, torch.arange(1, int(lengths[0]) + 1, dtype=torch.int32, device='cuda') * 8)


def test_scan_one_byte_octree():
    check_pipeline([bf.cube_of_points([[1, 0, 1]], 1)], 'cuda')
    check_pipeline([bf.cube_of_points([[1, 0, 1]], 1), np.ones((2, 2, 2), dtype=bool)], 'cuda')


# ------------------------------------------------------------------------------------------------------------- generate_points
def test_generate_points_dense():
    S = spc()
    octree, lengths = S.create_dense_spc(3, 'cuda')
    d = bf.decode(np.ones((8, 8, 8), dtype=bool))
    assert torch.equal(octree.cpu(), t(d.octree, 'cpu'))
    max_level, pyramids, exsum = S.scan_octrees(octree, lengths)
    assert max_level == 3 and torch.equal(S.generate_points(octree, pyramids, exsum).cpu(), t(d.points, 'cpu'))


def test_generate_points_chain_to_depth_15():
    """a single chain to the deepest level, ending at the int16 maximum: child 7 (bit 7) of every node"""
    S = spc()
    octree = torch.full((15,), 128, dtype=torch.uint8, device='cuda')
    max_level, pyramids, exsum = S.scan_octrees(octree, torch.tensor([15], dtype=torch.int32))
    assert max_level == 15 and pyramids[0, 0].tolist() == [1] * 16 + [0] and pyramids[0, 1].tolist() == list(range(17))
    assert exsum.tolist() == list(range(1, 16))
    points = S.generate_points(octree, pyramids, exsum)
    assert points.tolist() == [[2 ** l - 1] * 3 for l in range(16)] and points[15].tolist() == [32767] * 3
    q = torch.tensor([[32767, 32767, 32767], [32767, 32767, 32766]], dtype=torch.int16, device='cuda')
    assert S.unbatched_query(octree, exsum, q, 15).tolist() == [15, -1]
    assert S.unbatched_query(octree, exsum, q, 15, with_parents=True).tolist() == [list(range(16)), list(range(15)) + [-1]]


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('level', [1, 4, 7])
def test_pipeline_gpu(level, B):
    check_pipeline(cubes_for(level, B), 'cuda', query_dtypes=(torch.float16, torch.float32, torch.float64))


# ------------------------------------------------------------------------------------------------------------------ octree build
def test_octree_single_point_and_extreme_levels():
    S = spc()
    one = torch.tensor([[1, 0, 1]], dtype=torch.int16, device='cuda')
    assert S.unbatched_points_to_octree(one, 1).tolist() == [1 << 5]
    assert S.unbatched_points_to_octree(one, 1, sorted=True).tolist() == [1 << 5]
    assert S.unbatched_points_to_octree(one, 0).shape == (0,)
    deep = torch.tensor([[32767, 32767, 32767], [0, 0, 0], [32767, 32767, 32767]], dtype=torch.int16, device='cuda')
    assert S.unbatched_points_to_octree(deep[:1], 15).tolist() == [128] * 15
    assert S.unbatched_points_to_octree(deep, 15).tolist() == [129] + [1, 128] * 14          # two chains: children 0 and 7
    assert S.unbatched_points_to_octree(deep[1:], 15, sorted=True).tolist() == [129] + [1, 128] * 14
    with pytest.raises(ValueError, match='no points'):
        S.unbatched_points_to_octree(deep[:0], 3)


@pytest.mark.parametrize('n', [SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 2 * SORT_TILE + 1])
def test_octree_build_across_the_sort_tile(n):
    S = spc()
    points = np.random.RandomState(n).randint(0, 64, (n, 3)).astype(np.int16)
    d = bf.decode(bf.cube_of_points(points, 6))
    assert torch.equal(S.unbatched_points_to_octree(t(points, 'cuda'), 6).cpu(), t(d.octree, 'cpu'))
    assert torch.equal(S.unbatched_points_to_octree(t(d.level_points[6], 'cuda'), 6, sorted=True).cpu(), t(d.octree, 'cpu'))


# ------------------------------------------------------------------------------------------------------------------------ query
@pytest.mark.parametrize('dtype', [torch.float16, torch.float32, torch.float64])
def test_query_at_and_beyond_the_borders(dtype):
    """the dense octree of level 3, queries (q, 0.1, 0.1): q = -1 is cell 0, q = 1 is cell 8 -- outside; floor (without parents)
    against truncation toward zero (with parents) just below -1; far outside, infinite and NaN coordinates miss"""
    S = spc()
    octree, lengths = S.create_dense_spc(3, 'cuda')
    _, _, exsum = S.scan_octrees(octree, lengths)
    d = bf.decode(np.ones((8, 8, 8), dtype=bool))
    eps = 2.0 ** -9                                                # exact in half next to 1
    big = 60000.0 if dtype == torch.float16 else 1e30
    qs = [-1.0, 1.0, -1.0 - eps, 1.0 + eps, 1.0 - eps, big, -big, float('inf'), float('-inf'), float('nan')]
    floor_cell = [0, 8, -1, 8, 7, None, None, None, None, None]      # floor(4 (q + 1))
    trunc_cell = [0, 8, 0, 8, 7, None, None, None, None, None]       # trunc(8 (q / 2 + 1 / 2)): -2^-7 -> 0
    other = 4                                                      # 0.1 -> floor(4 * 1.1) = trunc(8 * 0.55) = 4
    for axis in range(3):
        coords = torch.full((len(qs), 3), 0.1, dtype=torch.float64)
        coords[:, axis] = torch.tensor(qs, dtype=torch.float64)
        coords = coords.to(dtype).cuda()

        def cell(c):
            p = [other] * 3
            p[axis] = c
            return p
        want = [bf.query(d, 3, cell(c)) if c is not None and 0 <= c < 8 else -1 for c in floor_cell]
        assert S.unbatched_query(octree, exsum, coords, 3).tolist() == want
        want = [bf.ancestors(d, 3, cell(c)) if c is not None else [-1] * 4 for c in trunc_cell]
        assert S.unbatched_query(octree, exsum, coords, 3, with_parents=True).tolist() == want


def test_query_sizes_around_the_block():
    S = spc()
    d = bf.decode(bf.random_cube(4, 11))
    octree, exsum = t(d.octree, 'cuda'), t(d.exsum, 'cuda')
    leaves = d.level_points[4]
    empty = S.unbatched_query(octree, exsum, torch.zeros((0, 3), device='cuda'), 4)
    assert empty.shape == (0,) and empty.dtype == torch.long
    assert S.unbatched_query(octree, exsum, torch.zeros((0, 3), device='cuda'), 4, with_parents=True).shape == (0, 5)
    for Q in (255, 256, 257):
        pick = np.arange(Q) % len(leaves)
        got = S.unbatched_query(octree, exsum, t(leaves[pick], 'cuda'), 4)
        assert torch.equal(got.cpu(), torch.as_tensor(pick) + int(d.pyramid[1, 4]))
        got = S.unbatched_query(octree, exsum, t(leaves[pick], 'cuda'), 4, with_parents=True)
        assert got.tolist() == [bf.ancestors(d, 4, leaves[i]) for i in pick]


def test_query_int16_and_inner_levels():
    S = spc()
    d = bf.decode(bf.random_cube(5, 12))
    octree, exsum = t(d.octree, 'cuda'), t(d.exsum, 'cuda')
    for level in (0, 2, 5):
        check_queries(S, d, octree, exsum, level, 'cuda', (torch.float16, torch.float32, torch.float64))


def test_query_replays_in_a_graph():
    S = spc()
    d = bf.decode(bf.random_cube(5, 13))
    octree, exsum = t(d.octree, 'cuda'), t(d.exsum, 'cuda')
    g = torch.Generator().manual_seed(0)
    coords = (torch.rand((1000, 3), generator=g) * 2.2 - 1.1).cuda()
    leaves = torch.as_tensor((d.level_points[5].astype(np.float32) + 0.5) / 16.0 - 1.0).cuda()
    coords[:len(leaves)] = leaves[:1000]
    eager = S.unbatched_query(octree, exsum, coords, 5)
    eager_parents = S.unbatched_query(octree, exsum, coords, 5, with_parents=True)
    assert int((eager >= 0).sum()) >= min(len(leaves), 1000)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        S.unbatched_query(octree, exsum, coords, 5)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = S.unbatched_query(octree, exsum, coords, 5)
        out_parents = S.unbatched_query(octree, exsum, coords, 5, with_parents=True)
    out.fill_(-7)
    out_parents.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager) and torch.equal(out_parents, eager_parents)


# --------------------------------------------------------------------------------------------------------------------- to_dense
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('level', [-1, 1])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('C', [1, 4])
def test_to_dense_forward_and_backward(C, B, level, dtype):
    cubes = cubes_for(3, B)
    out, grad = check_to_dense_backward(cubes, 'cuda', level, C, dtype)              # HIP against index_put autograd on the GPU
    cpu_out, cpu_grad = check_to_dense_backward(cubes, 'cpu', level, C, dtype)       # ... and against the CPU path: same seeds
    assert torch.equal(out.cpu(), cpu_out) and torch.equal(grad.cpu(), cpu_grad)


def test_to_dense_other_dtypes_take_the_torch_formulation():
    S = spc()
    _, _, _, pyramids_np, _, points_np = bf.decode_batch(cubes_for(2, 2))
    pyramids, points = t(pyramids_np, 'cpu'), t(points_np, 'cuda')
    rows = int(pyramids[:, 0, 2].sum())
    x = torch.arange(rows * 2, dtype=torch.float32).reshape(rows, 2).cuda()
    assert torch.equal(S.to_dense(points, pyramids, x.half()), S.to_dense(points, pyramids, x).half())
    with pytest.raises(TypeError, match='unexpected keyword'):
        S.to_dense(points, pyramids, x, features=x)


@pytest.mark.parametrize('with_masks', [False, True])
@pytest.mark.parametrize('C', [1, 3])
def test_feature_grid_round_trip_gpu(C, with_masks):
    check_feature_grid_round_trip(C, with_masks, 'cuda')


# ------------------------------------------------------------------------------------------------------ the point of the feature
def sphere_soup(level=8, radius=0.6):
    from kaolin_amd.utils.testing import geodesic_sphere
    v, f = geodesic_sphere(level)
    return (v.float() * (radius / 0.5))[f].contiguous()


@pytest.mark.parametrize('level', [3, 7])
def test_mesh_to_spc_octree_is_consumed(level):
    import kaolin_amd as kal
    S = spc()
    fv = sphere_soup()
    octree = kal.ops.conversions.unbatched_mesh_to_spc(fv.cuda(), level)[0]
    mortons = oracle.mesh_to_spc(fv, level, omp=True, return_mortons=True)[3].numpy().astype(np.int64)
    voxels = np.zeros((len(mortons), 3), dtype=np.int64)           # the oracle's voxels, decoded here
    for i in range(level):
        voxels[:, 2] |= ((mortons >> (3 * i)) & 1) << i
        voxels[:, 1] |= ((mortons >> (3 * i + 1)) & 1) << i
        voxels[:, 0] |= ((mortons >> (3 * i + 2)) & 1) << i
    voxels = voxels.astype(np.int16)
    max_level, pyramids, exsum = S.scan_octrees(octree, torch.tensor([octree.numel()], dtype=torch.int32))
    assert max_level == level and int(pyramids[0, 0, level]) == len(voxels)
    points = S.generate_points(octree, pyramids, exsum)
    assert torch.equal(S.unbatched_get_level_points(points, pyramids[0], level).cpu(), t(voxels, 'cpu'))
    centres = t((voxels.astype(np.float32) + 0.5) / 2 ** level * 2.0 - 1.0, 'cuda')
    got = S.unbatched_query(octree, exsum, centres, level)
    assert torch.equal(got.cpu() - int(pyramids[0, 1, level]), torch.arange(len(voxels)))


# ---------------------------------------------------------------------------------------------------------------------- shims
def test_shims_reject_cpu_tensors():
    import kaolin_amd as kal
    C = kal._C.ops.spc
    points = torch.zeros((2, 3), dtype=torch.int16)
    octree, exsum = torch.tensor([255], dtype=torch.uint8), torch.tensor([8], dtype=torch.int32)
    pyramid = torch.tensor([[[1, 8, 0], [0, 1, 9]]], dtype=torch.int32)
    for call in (lambda: C.points_to_morton_cuda(points), lambda: C.morton_to_points_cuda(torch.zeros(2, dtype=torch.long)),
                 lambda: C.points_to_corners_cuda(points), lambda: C.points_to_octree(points, 1),
                 lambda: C.morton_to_octree(torch.zeros(2, dtype=torch.long), 1),
                 lambda: C.scan_octrees_cuda(octree, torch.tensor([1], dtype=torch.int32)),
                 lambda: C.generate_points_cuda(octree, pyramid, exsum), lambda: C.query_cuda(octree, exsum, torch.zeros(1, 3), 1),
                 lambda: C.query_multiscale_cuda(octree, exsum, torch.zeros(1, 3), 1),
                 lambda: C.to_dense_forward(torch.zeros((9, 3), dtype=torch.int16), 1, pyramid, torch.zeros(8, 1)),
                 lambda: C.to_dense_backward(torch.zeros((9, 3), dtype=torch.int16), 1, pyramid, torch.zeros(8, 1),
                                             torch.zeros(1, 1, 2, 2, 2))):
        with pytest.raises(RuntimeError, match='CUDA'):
            call()
