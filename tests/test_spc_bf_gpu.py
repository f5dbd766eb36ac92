"""The Bayesian-fusion operators, ``bf_recon`` and ``sample_points_in_volume`` through the HIP path (csrc/spc_bf.hip): the cases of
tests/test_spc_bf_cpu.py on CUDA tensors -- every operator ``torch.equal`` to the numpy restatement at point counts around the
kernels' blocks, on every branch of oracleB, with and without the in-place depth conversion; the octree, query, bf_cells and
fuseBF pins; one frame against geometry; the densifier end to end (20 000 Gaussians, 256 x 256 depth maps; also with the default
viewpoints) -- and what only
the GPU can show: two runs are bit-identical, the one-launch operators replay in a captured graph, and a frame calls the
operators of ``_C.ops.spc`` in the reference's sequence.  No test feeds the kernels an out-of-range index."""
import collections
import types

import numpy as np
import pytest
import torch

import spc_bf_bruteforce as bf
import test_spc_bf_cpu as C
from test_spc_bf_cpu import COUNTS, MAX_DEPTH, SCENES, SIGMA, bfr, kal, level_points, scene, t

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('true_depth', [False, True])
@pytest.mark.parametrize('name', ['front32', 'cell64'])
def test_build_mip2d(name, true_depth):
    C.check_build_mip2d(DEV, name, true_depth)


def test_oracleB_equals_the_oracle_on_every_branch():
    seen = set()
    for name, level, points in C.oracleB_cases():
        seen |= set(C.check_oracleB(DEV, name, level, points)[2].tolist())
    assert seen >= {'mip0', 'mid', 'top', 'high', 'straddle', 'outside', 'behind'}, seen


@pytest.mark.parametrize('name', list(SCENES))
def test_final_operators_equal_the_oracle(name):
    for level in range(1, 6):
        C.check_final(DEV, name, level, level_points(level) if level < 5 else level_points(5, 1025, 1))


@pytest.mark.parametrize('n', COUNTS)
def test_point_counts_around_the_blocks(n):
    points = level_points(5, n, 3)
    C.check_oracleB(DEV, 'front32', 5, points)
    C.check_final(DEV, 'front32', 5, points)
    C.check_scan_ops(DEV, n)
    C.check_process_final_voxels(DEV, n)
    C.check_merges(DEV, 3, n)


def test_empty_inputs_return_empty_tensors_of_the_right_types():
    o, s = kal._C.ops.spc, scene('front32')
    none = torch.zeros((0, 3), dtype=torch.int16, device=DEV)
    depth, mips = t(s['depth'], DEV), t(s['mips'], DEV)
    occ, state = o.oracleB(none, 3, SIGMA, s['cam'], depth, mips, 3)
    assert occ.shape == state.shape == (0,) and occ.dtype == state.dtype == torch.int32
    occ, state, probs = o.oracleB_final(none, 3, SIGMA, s['cam'], depth)
    assert probs.shape == (0,) and probs.dtype == torch.float32 and occ.dtype == torch.int32
    colors, normals = o.colorsB_final(none, 3, s['cam'], SIGMA, t(s['image'], DEV), depth, probs)
    assert colors.shape == (0, 4) and colors.dtype == torch.uint8 and normals.shape == (0, 3) and normals.dtype == torch.float32
    insum = o.inclusive_sum(torch.zeros(0, dtype=torch.int32, device=DEV))
    assert insum.shape == (0,) and insum.dtype == torch.int32
    pts, nvsum = o.subdivide(none, insum)
    assert pts.shape == (0, 3) and pts.dtype == torch.int16 and nvsum.dtype == torch.int32
    pts, nvsum = o.compactify(none, insum)
    assert pts.shape == (0, 3) and nvsum.dtype == torch.long


def test_degenerate_cams():
    C.check_degenerate_cams(DEV)


def test_level_zero_is_occupied():
    s = scene('front32')
    root = torch.zeros((1, 3), dtype=torch.int16, device=DEV)
    occ, state = kal._C.ops.spc.oracleB(root, 0, SIGMA, s['cam'], t(s['depth'], DEV), t(s['mips'], DEV), 3)
    assert occ.tolist() == [1] and state.tolist() == [2]
    occ, state, probs = kal._C.ops.spc.oracleB_final(root, 0, SIGMA, s['cam'], t(s['depth'], DEV))
    assert occ.tolist() == [1] and state.tolist() == [2] and probs.tolist() == [0.0]


@pytest.mark.parametrize('level', [1, 2, 3, 4])
def test_query_agrees_with_the_dense_expansion(level):
    C.check_query(DEV, level, 10 + level)


@pytest.mark.parametrize('level', [1, 2, 3, 4, 5, 6])
def test_bf_cells_equals_the_dense_query(level):
    sparse = dict(p_occ=0.45, p_unseen=0.25) if level < 5 else dict(p_occ=0.3, p_unseen=0.1)
    octree, empty = C.build_tree(level, 20 + level, **sparse)
    assert 0 < len(C.check_cells(DEV, octree, empty, level)) < 8 ** level
    octree, empty = C.build_tree(level, 30 + level, unseen=False, p_occ=sparse['p_occ'])          # no unseen bit at all
    C.check_cells(DEV, octree, empty, level)
    assert len(C.check_cells(DEV, np.array([0], np.uint8), np.array([255], np.uint8), level)) == 8 ** level   # the root all unseen


@pytest.mark.parametrize('level', [1, 3, 4])
def test_merges_equal_the_oracle(level):
    C.check_merges(DEV, level)


def test_octree_pin_and_fuse_laws():
    C.check_fuse_laws(DEV, C.check_octree_pin(DEV))


def test_frame_geometry():
    C.check_frame_geometry(DEV, res=8)


def test_bad_arguments_raise_value_error():
    o, s = kal._C.ops.spc, scene('front32')
    depth = t(s['depth'], DEV)
    pts = torch.zeros((2, 3), dtype=torch.int16, device=DEV)
    with pytest.raises(ValueError):
        o.build_mip2d(torch.zeros((30, 30), device=DEV), s['intrinsics'], 3, MAX_DEPTH, True)
    with pytest.raises(ValueError):
        o.build_mip2d(depth.cpu(), s['intrinsics'], 3, MAX_DEPTH, True)                    # a CPU tensor
    with pytest.raises(ValueError):
        o.oracleB(pts, 3, SIGMA, s['cam'], depth, t(s['mips'], DEV)[:-1], 3)               # a pyramid of the wrong size
    with pytest.raises(ValueError):
        o.oracleB(pts.int(), 3, SIGMA, s['cam'], depth, t(s['mips'], DEV), 3)
    with pytest.raises(ValueError):
        o.oracleB_final(pts, 3, 0.0, s['cam'], depth)
    with pytest.raises(ValueError):
        o.colorsB_final(pts, 3, s['cam'], SIGMA, t(s['image'], DEV), depth, torch.zeros(3, device=DEV))
    with pytest.raises(ValueError):
        o.subdivide(pts, torch.tensor([1, 5], dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError):
        o.process_final_voxels(4, 2, *(torch.zeros(k, dtype=d, device=DEV) for k, d in (
            (32, torch.int32), (4, torch.int32), (8, torch.int32), (4, torch.int32), (8, torch.uint8), (8, torch.uint8))))
    with pytest.raises(ValueError):
        o.compactify_nodes(9, torch.zeros(8, dtype=torch.int32, device=DEV), torch.zeros(8, dtype=torch.uint8, device=DEV),
                           torch.zeros(8, dtype=torch.uint8, device=DEV))
    two = torch.tensor([1, 1], dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        o.bf_cells_cuda(two, two, 1)                                                        # a byte too many for one level
    with pytest.raises(ValueError):
        o.query_cuda_empty(two, two, torch.zeros(3, dtype=torch.int32, device=DEV), torch.zeros((1, 3), device=DEV), 1)
    with pytest.raises(ValueError):
        o.merge_empty(pts, 16, two, two, two, two, torch.zeros(2, dtype=torch.int32, device=DEV),
                      torch.zeros(2, dtype=torch.int32, device=DEV))


def test_fill_is_solid():
    C.check_fill_is_solid(DEV)


def test_clipped_samples_lie_on_a_grid_inside_the_bbox():
    C.check_clipped(DEV)


def test_jitter_moves_every_point_by_at_most_two_diagonals():
    C.check_jitter(DEV)


def test_num_samples_and_the_level_assertion():
    C.check_num_samples(DEV)


def test_masked_call_returns_at_least_the_thresholded_points():
    C.check_mask(DEV)


def test_custom_viewpoints():
    C.check_custom_viewpoints(DEV)


def test_default_viewpoints_and_a_second_run():
    """the densifier's own 86 viewpoints at full resolution; and a run repeated is bit-identical"""
    centre, must, key, lo, hi = C.e2e_geometry(DEV)
    default = kal.ops.gaussians.sample_points_in_volume(*C.e2e_model(DEV)[0], octree_level=6, jitter=False)
    assert torch.isin(key(must), key(default)).all() and ((default > lo) & (default < hi)).all()
    assert torch.equal(C.e2e_sample(DEV, jitter=False, clip_samples_to_input_bbox=False), C.e2e_free(DEV))


def test_sample_points_in_volume_failure_paths(caplog):
    C.check_failure_paths(DEV, caplog)


def test_two_runs_are_bit_identical():
    ds = C.frames(DEV, [[4.0, 0.0, 0.0], [2.3, 2.3, 2.3], [0.0, -4.0, 0.0]], 7)
    runs = [bfr.bf_recon(ds, 6, 0.0005) for _ in range(2)]
    assert runs[0][0] is not None and len(runs[0][0]) > 0
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_one_launch_operators_replay_in_a_graph():
    """query_cuda_empty and oracleB_final inside one capture (a linear one: no parallel branches)"""
    octree, empty = C.build_tree(4, 14)
    to, te = t(octree, DEV), t(empty, DEV)
    _, _, exsum = kal.ops.spc.scan_octrees(to, torch.tensor([len(octree)], dtype=torch.int32))
    coords = (torch.rand((1000, 3), generator=torch.Generator().manual_seed(0)) * 2.2 - 1.1).to(DEV)
    s = scene('front32')
    points, depth = t(level_points(4), DEV), t(s['depth'], DEV)
    o = kal._C.ops.spc
    eager_q = o.query_cuda_empty(to, te, exsum, coords, 4)
    eager_f = o.oracleB_final(points, 4, SIGMA, s['cam'], depth)
    assert len(set(eager_q.tolist())) > 3
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        o.query_cuda_empty(to, te, exsum, coords, 4)
        o.oracleB_final(points, 4, SIGMA, s['cam'], depth)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_q = o.query_cuda_empty(to, te, exsum, coords, 4)
        out_f = o.oracleB_final(points, 4, SIGMA, s['cam'], depth)
    out_q.fill_(-7)
    for x in out_f:
        x.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_q, eager_q)
    for a, b in zip(out_f, eager_f):
        assert torch.equal(a, b)


def test_a_frame_calls_the_operators_in_the_reference_sequence(monkeypatch):
    """processFrame at final level L with start level 4: build_mip2d; per level 4 .. L - 1 oracleB, inclusive_sum, subdivide;
    oracleB_final, inclusive_sum, compactify, colorsB_final; process_final_voxels for L .. 1; inclusive_sum, compactify_nodes.
    fuseBF: merge_empty, inclusive_sum, subdivide per level; bq_merge, inclusive_sum, compactify; process_final_voxels and
    inclusive_sum for L .. 1; inclusive_sum, compactify_nodes."""
    calls = []
    real = kal._C.ops.spc
    names = ['build_mip2d', 'oracleB', 'oracleB_final', 'colorsB_final', 'inclusive_sum', 'subdivide', 'compactify',
             'process_final_voxels', 'compactify_nodes', 'merge_empty', 'bq_merge', 'query_cuda_empty', 'bf_cells_cuda']

    def wrap(name):
        def call(*a, **kw):
            calls.append(name)
            return getattr(real, name)(*a, **kw)
        return call
    wrapped = types.SimpleNamespace(**{**vars(real), **{n: wrap(n) for n in names}})
    monkeypatch.setattr(kal._C.ops, 'spc', wrapped)
    L = 6
    ds = C.frames(DEV, [[4.0, 0.0, 0.0], [2.3, 2.3, 2.3]], 7)
    a = bfr.processFrame(ds[0], L, 0.0005)
    frame = ['build_mip2d'] + ['oracleB', 'inclusive_sum', 'subdivide'] * (L - 4) + \
        ['oracleB_final', 'inclusive_sum', 'compactify', 'colorsB_final'] + ['process_final_voxels'] * L + \
        ['inclusive_sum', 'compactify_nodes']
    assert calls == frame, calls
    assert collections.Counter(calls)['process_final_voxels'] == L
    b = bfr.processFrame(ds[1], L, 0.0005)
    del calls[:]
    bfr.fuseBF(a, b)
    fuse = ['merge_empty', 'inclusive_sum', 'subdivide'] * (L - 4) + ['bq_merge', 'inclusive_sum', 'compactify'] + \
        ['process_final_voxels', 'inclusive_sum'] * L + ['inclusive_sum', 'compactify_nodes']
    assert calls == fuse, calls
