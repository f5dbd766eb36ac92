"""unbatched_mesh_to_spc through the HIP path (csrc/mesh_to_spc.hip, spc_stage.h, spc_octree.h, sort_scan.h) at the block boundaries of its
pipeline, against the numpy references of tests/mesh_to_spc_bruteforce.py and the oracle.  Everything is compared bit for bit.

(a) the whole operator: levels 10 - 15 (codes beyond 32 bits, four and five stages, five and six sort passes), triangle counts around
    the eight proposals of a wavefront and the 32 of a block of the stage kernel and around a block of the scan, degenerate triangles;
(b) one stage through the C ABI on synthetic proposal lists: counts, offsets and emitted pairs against ``subtree``;
(c) kamd_mesh_to_spc_build + kamd_mesh_to_spc_results on synthetic pair lists against ``build``: pair counts around the sort's
    block, runs of equal codes over wavefronts, rounds and blocks, voxel and inner node counts around the scan's block;
(d) two runs give the same bits;
and the spans a stage rejects.  Every test asserts on the reference side that its input has the count it aims at.  No test gives a
kernel a span above kamd_mesh_to_spc_stage_levels(), an out-of-range triangle id or a Morton code beyond the level."""
import functools

import numpy as np
import pytest
import torch

import mesh_to_spc_bruteforce as bf
import oracle
from test_mesh_to_spc import assert_matches_oracle, random_soup
from test_mesh_to_spc_cpu import (DEEP_CASES, YIELDS_NOTHING, MIXED_AT, compose, deep_scene, degenerate, mixed_soup, tie_soup)

pytestmark = pytest.mark.gpu

GROUPS_PER_WAVE = 8        # proposals per wavefront of spc_stage_kernel (eight lanes each)
PROPOSALS_PER_BLOCK = 32   # proposals per 256-thread block of spc_stage_kernel
SCAN_BLOCK = 1024          # entries per block of ss_scan
SORT_BLOCK = 2048          # pairs per block of the radix sort (SS_SORT_BLOCK): eight rounds of 256
SORT_ROUND = 256
WAVE = 64
STAGE_LEVELS = 3

STAGE_COUNTS = [1, GROUPS_PER_WAVE - 1, GROUPS_PER_WAVE, GROUPS_PER_WAVE + 1, PROPOSALS_PER_BLOCK - 1, PROPOSALS_PER_BLOCK,
                PROPOSALS_PER_BLOCK + 1, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1]
PAIR_COUNTS = [1, SORT_BLOCK - 1, SORT_BLOCK, SORT_BLOCK + 1, 2 * SORT_BLOCK + 1]
SENTINEL = -7
PAD = 64                   # sentinel entries behind every output


def api():
    from kaolin_amd import _lib
    return _lib, _lib.load()


def cuda(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda()


def filled(n, dtype=torch.long):
    return torch.full((n + PAD,), SENTINEL, dtype=dtype, device='cuda')


def untouched(t, n):
    return bool((t[n:] == SENTINEL).all())


def test_the_counts_are_the_ones_the_kernels_split_at():
    assert STAGE_COUNTS == [1, 7, 8, 9, 31, 32, 33, 1023, 1024, 1025] and PAIR_COUNTS == [1, 2047, 2048, 2049, 4097]
    _, lib = api()
    assert lib.kamd_mesh_to_spc_stage_levels() == STAGE_LEVELS


# ---- (a) the whole operator --------------------------------------------------------------------------------------------------------
def assert_matches_oracle_nan(fv, level):
    """assert_matches_oracle for scenes with a triangle of no area: its voxels' weights are 0 * inf = NaN on either side, and a NaN
    has no bits to agree on.  Octree and face ids equal; weights NaN in the same places and equal everywhere else"""
    import kaolin_amd as kal
    got = kal.ops.conversions.unbatched_mesh_to_spc(fv.cuda(), level)
    ref = oracle.mesh_to_spc(fv, level, omp=True)
    assert got[0].shape == ref[0].shape and got[1].shape == ref[1].shape and got[2].shape == ref[2].shape
    assert torch.equal(got[0].cpu(), ref[0]) and torch.equal(got[1].cpu(), ref[1])
    nan = torch.isnan(ref[2])
    assert torch.equal(torch.isnan(got[2]).cpu(), nan) and torch.equal(got[2].cpu()[~nan], ref[2][~nan])
    return got, nan


def assert_matches_dense(fv, level, got):
    morton, face = bf.dense(fv.numpy(), level)
    assert np.array_equal(got[1].cpu().numpy(), face)
    return morton, face


@pytest.mark.parametrize('kind, level', DEEP_CASES)
def test_deep_levels(kind, level):
    """10: four stages, the last of one level; 12: four; 13: five, the last of one level; 15: five, 45 key bits and six sort passes"""
    fv = deep_scene(kind, level)
    codes = oracle.mesh_to_spc(fv, level, return_mortons=True)[3].numpy()
    assert 10 <= len(codes) <= 2000
    x, y, z = bf.to_point(codes)
    if kind == 'top_bit':
        assert ((codes >> (3 * level - 1)) & 1).all() and (level != 15 or int(codes.max()) >> 44 == 1)
    if kind == 'centre':
        for g in (x, y, z):
            assert g.min() < (1 << (level - 1)) <= g.max()
    assert_matches_oracle(fv, level)


@pytest.mark.parametrize('F', STAGE_COUNTS)
def test_triangle_counts_around_the_blocks(F):
    """level 2: one stage whose proposals are the F triangles themselves"""
    fv = random_soup(F, F)
    got = assert_matches_oracle(fv, 2)
    morton, _ = assert_matches_dense(fv, 2, got)
    assert len(morton) > 0


@pytest.mark.parametrize('name', YIELDS_NOTHING)
def test_point_and_two_equal_vertices_alone(name):
    import kaolin_amd as kal
    for level in (0, 1, 3, 12):
        octree, face_idx, bary = kal.ops.conversions.unbatched_mesh_to_spc(degenerate(name).cuda(), level)
        assert octree.shape == (0,) and face_idx.shape == (0,) and bary.shape == (0, 3)
        assert oracle.mesh_to_spc(degenerate(name), level)[1].shape == (0,)


def test_collinear_triangle_alone():
    for level, voxels in ((0, 1), (1, 8), (3, 24), (4, 40)):
        got, nan = assert_matches_oracle_nan(degenerate('collinear'), level)
        assert_matches_dense(degenerate('collinear'), level, got)
        assert got[1].numel() == voxels and bool(nan.all())                  # no area: every weight is 0 * inf
    assert assert_matches_oracle_nan(degenerate('collinear') * 2.0 ** -8, 12)[0][1].numel() == 40


def test_in_plane_triangle_alone():
    for level, voxels in ((0, 1), (1, 8), (3, 46), (4, 116)):
        got = assert_matches_oracle(degenerate('in_plane'), level)
        assert_matches_dense(degenerate('in_plane'), level, got)
        assert got[1].numel() == voxels
    assert assert_matches_oracle(degenerate('in_plane') * 2.0 ** -8, 12)[1].numel() == 116


def test_degenerates_mixed_into_a_soup():
    fv, soup, kept = mixed_soup()
    got, nan = assert_matches_oracle_nan(fv, 4)
    morton, face = assert_matches_dense(fv, 4, got)
    assert torch.equal(nan.all(1), torch.from_numpy(face == MIXED_AT[2])) and bool(nan.any())   # only the collinear triangle's voxels
    plain = oracle.mesh_to_spc(soup, 4, return_mortons=True)
    at = np.searchsorted(morton, plain[3].numpy())
    gpu_face = got[1].cpu().numpy()[at]
    undisturbed = kept.numpy()[plain[1].numpy()]
    mine = np.isin(gpu_face, kept.numpy())
    assert not np.isin(gpu_face, [MIXED_AT[0], MIXED_AT[1]]).any()
    assert mine.sum() > 100 and np.array_equal(gpu_face[mine], undisturbed[mine])
    assert (gpu_face[~mine] < undisturbed[~mine]).all()


def test_equal_triangles_report_the_smallest_index():
    got = assert_matches_oracle(tie_soup(), 4)
    _, face = assert_matches_dense(tie_soup(), 4, got)
    assert (face == 3).sum() > 10 and not np.isin(face, [11, 12, 29, 30]).any()


def test_nothing_inside_at_deep_levels():
    import kaolin_amd as kal
    fv = deep_scene('random', 13)
    for case, level in ((fv + 5., 13), (fv[:0], 15)):
        octree, face_idx, bary = kal.ops.conversions.unbatched_mesh_to_spc(case.cuda(), level)
        assert octree.shape == (0,) and face_idx.shape == (0,) and bary.shape == (0, 3)


# ---- (b) one stage through the C ABI ---------------------------------------------------------------------------------------------
STAGE_BASE = (1000, 2000, 3000)   # level-12 cell whose 2 x 2 x 2 neighbourhood holds the proposals of the stages from level 12


def stage_triangles():
    """0 a large triangle through the neighbourhood (full subtrees), 1 a small one elsewhere in the cube (fails at once from level 12,
    a sparse subtree from level 0), 2 inside one level-15 voxel, 3 a few level-15 voxels wide, 4 two equal vertices, 5 outside"""
    size = 2.0 / (1 << 12)
    p = (np.array(STAGE_BASE, dtype=np.float64) + 1.0) * size - 1.0          # the corner the eight cells share
    s15 = size / 8.0
    tris = [p + np.array([[-0.5, -0.4, 0.03], [0.6, -0.3, -0.05], [-0.1, 0.7, 0.02]]),
            np.array([[0.30, 0.31, -0.52], [0.36, 0.30, -0.50], [0.33, 0.37, -0.47]]),
            p + s15 * np.array([[0.2, 0.3, 0.4], [0.6, 0.3, 0.5], [0.4, 0.7, 0.3]]),
            p + s15 * np.array([[-2.3, -1.2, 0.4], [2.6, 0.3, -1.5], [0.4, 2.7, 1.3]]),
            np.array([[0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [0.5, 0.5, 0.5]]),
            p + 5.0 + np.array([[-0.5, -0.4, 0.03], [0.6, -0.3, -0.05], [-0.1, 0.7, 0.02]])]
    return np.stack(tris).astype(np.float32)


@functools.lru_cache(maxsize=None)
def stage_pool(level_from, span, tested):
    """every (voxel, triangle) of the pool with its reference subtree, computed once
    -> (codes, triangles, counts, [emitted codes of every pool entry])"""
    fv = stage_triangles()
    if level_from == 0:
        voxels = np.zeros(1, np.int64)
    else:
        b = np.array(STAGE_BASE)
        voxels = np.array([bf.to_morton(*(b + [i, j, k])) for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.int64)
    m = np.repeat(voxels, fv.shape[0])
    t = np.tile(np.arange(fv.shape[0], dtype=np.int64), len(voxels))
    counts, out, _ = bf.subtree(fv, m, t, level_from, level_from + span, tested)
    return m, t, counts, np.split(out, np.cumsum(counts)[:-1])


@pytest.mark.parametrize('level_from, tested', [(0, 0), (0, 1), (12, 0), (12, 1)])
@pytest.mark.parametrize('n', STAGE_COUNTS)
def test_one_stage_against_subtree(n, level_from, tested):
    _lib, lib = api()
    fv = cuda(stage_triangles())
    sp = _lib.stream_ptr(fv.device)
    for span in (0, 1, 2, 3):
        assert span <= STAGE_LEVELS
        pm, pt, pc, pout = stage_pool(level_from, span, tested)
        if span == 3:
            assert pc.max() >= (64 if level_from else 16)                    # a full layer of the subtree next to ...
        if span >= 1:
            assert (pc == 0).any()                                           # ... proposals that fail at once or below the first level
        if span == 0:
            assert set(pc.tolist()) == ({1} if tested else {0, 1})
        pick = np.random.RandomState(1000 * n + span).permutation(np.resize(np.arange(len(pm)), n))   # repeated and shuffled
        assert len(pick) == n
        want_counts = pc[pick]
        want_offsets = np.concatenate([[0], np.cumsum(want_counts)])
        want_codes = np.concatenate([pout[i] for i in pick])
        want_tris = np.repeat(pt[pick], want_counts)
        total = int(want_offsets[-1])
        morton, tri = cuda(pm[pick]), cuda(pt[pick])
        counts, offsets = filled(n, torch.int32), filled(n + 1)
        scan_ws = torch.empty(lib.kamd_mesh_to_spc_scan_workspace(n), dtype=torch.uint8, device='cuda')
        status = lib.kamd_mesh_to_spc_stage_count(sp, n, _lib.ptr(fv), _lib.ptr(morton), _lib.ptr(tri), level_from, level_from + span,
                                                  tested, _lib.ptr(counts), _lib.ptr(offsets), _lib.ptr(scan_ws))
        assert status == 0
        assert np.array_equal(counts[:n].cpu().numpy(), want_counts), span
        assert np.array_equal(offsets[:n + 1].cpu().numpy(), want_offsets), span
        assert untouched(counts, n) and untouched(offsets, n + 1)
        morton_out, tri_out = filled(total), filled(total)
        status = lib.kamd_mesh_to_spc_stage_emit(sp, n, _lib.ptr(fv), _lib.ptr(morton), _lib.ptr(tri), level_from, level_from + span,
                                                 tested, _lib.ptr(offsets), _lib.ptr(morton_out), _lib.ptr(tri_out))
        assert status == 0
        assert np.array_equal(morton_out[:total].cpu().numpy(), want_codes), span
        assert np.array_equal(tri_out[:total].cpu().numpy(), want_tris), span
        assert untouched(morton_out, total) and untouched(tri_out, total)
        assert np.array_equal(morton.cpu().numpy(), pm[pick]) and np.array_equal(tri.cpu().numpy(), pt[pick])


@pytest.mark.parametrize('level_from, level_to', [(0, 4), (11, 15), (0, 5), (10, 15), (0, 15), (3, 2), (13, 16), (-1, 2)])
def test_a_stage_rejects_what_the_walker_cannot_hold(level_from, level_to):
    """the walker keeps 8 bits per depth in one 32-bit word: spans above kamd_mesh_to_spc_stage_levels(), a negative span and levels
    outside [0, 15] return an error before any launch and leave the outputs alone (the rule of kamd_gs_to_spc_stage_*)"""
    _lib, lib = api()
    assert level_from < 0 or level_to < level_from or level_to > 15 or level_to - level_from > lib.kamd_mesh_to_spc_stage_levels()
    n = GROUPS_PER_WAVE + 1
    fv = cuda(stage_triangles())
    sp = _lib.stream_ptr(fv.device)
    morton, tri = torch.zeros(n, dtype=torch.long, device='cuda'), torch.zeros(n, dtype=torch.long, device='cuda')
    counts, offsets = filled(n, torch.int32), filled(n + 1)
    scan_ws = torch.empty(lib.kamd_mesh_to_spc_scan_workspace(n), dtype=torch.uint8, device='cuda')
    for tested in (0, 1):
        status = lib.kamd_mesh_to_spc_stage_count(sp, n, _lib.ptr(fv), _lib.ptr(morton), _lib.ptr(tri), level_from, level_to, tested,
                                                  _lib.ptr(counts), _lib.ptr(offsets), _lib.ptr(scan_ws))
        assert status != 0
        given = torch.zeros(n + 1, dtype=torch.long, device='cuda')
        morton_out, tri_out = filled(n), filled(n)
        status = lib.kamd_mesh_to_spc_stage_emit(sp, n, _lib.ptr(fv), _lib.ptr(morton), _lib.ptr(tri), level_from, level_to, tested,
                                                 _lib.ptr(given), _lib.ptr(morton_out), _lib.ptr(tri_out))
        assert status != 0
        torch.cuda.synchronize()
        assert untouched(counts, 0) and untouched(offsets, 0) and untouched(morton_out, 0) and untouched(tri_out, 0)


# ---- (c) build + results on synthetic pair lists ---------------------------------------------------------------------------------
TRIANGLES = 16   # the triangle table of the synthetic lists: any valid one (the barycentric weights are checked through (a))


def distinct_codes(count, level, rs):
    space = 8 ** level
    if space <= 1 << 20:
        return np.sort(rs.permutation(space)[:count]).astype(np.int64)
    codes = np.unique(rs.randint(0, space, 2 * count + 16, dtype=np.int64))
    assert len(codes) >= count
    return np.sort(rs.permutation(codes)[:count])


def check_build(morton, tri, level):
    """build + results of the C ABI on the pairs -> the reference's (sizes, octree, voxel codes, voxel triangles), all compared"""
    _lib, lib = api()
    morton, tri = np.asarray(morton, dtype=np.int64), np.asarray(tri, dtype=np.int64)
    n = len(morton)
    assert tri.min() >= 0 and tri.max() < TRIANGLES and morton.min() >= 0 and morton.max() < 8 ** level
    want_sizes, want_octree, um, ut = bf.build(morton, tri, level)
    fv = random_soup(TRIANGLES, 1).cuda()
    sp = _lib.stream_ptr(fv.device)
    m, t = cuda(morton), cuda(tri)
    nbytes = lib.kamd_mesh_to_spc_build_workspace(n, level)
    ws = torch.empty(nbytes, dtype=torch.uint8, device='cuda')
    sizes = filled(1 + level)
    assert lib.kamd_mesh_to_spc_build(sp, n, level, _lib.ptr(m), _lib.ptr(t), _lib.ptr(ws), nbytes, _lib.ptr(sizes)) == 0
    assert sizes[:1 + level].tolist() == want_sizes and untouched(sizes, 1 + level)
    assert np.array_equal(m.cpu().numpy(), morton) and np.array_equal(t.cpu().numpy(), tri)     # the inputs are only read
    # the results are sized by the reference: the sizes above are equal
    num_voxels, octree_bytes = want_sizes[0], sum(want_sizes[1:])
    octree, face_ids = filled(octree_bytes, torch.int8), filled(num_voxels)
    bary = torch.empty((num_voxels, 2), dtype=torch.float32, device='cuda')
    assert lib.kamd_mesh_to_spc_results(sp, n, level, _lib.ptr(fv), _lib.ptr(ws), num_voxels, octree_bytes, _lib.ptr(octree),
                                        _lib.ptr(face_ids), _lib.ptr(bary)) == 0
    assert np.array_equal(octree[:octree_bytes].view(torch.uint8).cpu().numpy(), want_octree)
    assert np.array_equal(face_ids[:num_voxels].cpu().numpy(), ut)
    assert untouched(octree, octree_bytes) and untouched(face_ids, num_voxels)
    return want_sizes, want_octree, um, ut


# runs of equal codes, as [first, last) positions of the list in code order: over a wavefront (64), over a round of the sort (256),
# inside a wavefront, over the first sort block (2048), over the second one, and up to the end of the longest list
RUNS = [(WAVE - 4, WAVE + 6), (SORT_ROUND - 6, SORT_ROUND + 6), (1000, 1003), (SORT_BLOCK - 148, SORT_BLOCK + 152),
        (2 * SORT_BLOCK - 10, 2 * SORT_BLOCK + 1)]


def pair_list(n, level, shuffled, seed):
    """n pairs over distinct random codes of `level` in ascending order, the positions of RUNS merged into one voxel each, random
    triangle ids; `shuffled`: in random order, so that every run is spread over all blocks of the input"""
    rs = np.random.RandomState(seed)
    group = np.arange(n)
    for a, b in RUNS:
        if a < n:
            group[a:min(b, n)] = a
    morton = distinct_codes(n, level, rs)[group]
    tri = rs.randint(0, TRIANGLES, n)
    if shuffled:
        order = rs.permutation(n)
        morton, tri = morton[order], tri[order]
    return morton, tri


@pytest.mark.parametrize('level', [5, 15])
@pytest.mark.parametrize('shuffled', [False, True], ids=['in_order', 'shuffled'])
@pytest.mark.parametrize('n', PAIR_COUNTS)
def test_build_pair_counts_around_the_sort_block(n, shuffled, level):
    """level 5: two sort passes; level 15: six.  The first pair of a run in input order wins, not the smallest triangle"""
    morton, tri = pair_list(n, level, shuffled, n + level)
    assert len(morton) == n
    if n > SORT_BLOCK:
        hot = np.nonzero(morton == np.sort(morton)[SORT_BLOCK])[0]           # the run that lies over position 2048 once sorted
        assert len(hot) == min(SORT_BLOCK + 152, n) - (SORT_BLOCK - 148)
        if not shuffled or n > 2 * SORT_BLOCK:
            assert hot.min() < SORT_BLOCK <= hot.max()                       # and over two blocks of the input
        if not shuffled:
            assert morton[WAVE - 1] == morton[WAVE] and morton[SORT_ROUND - 1] == morton[SORT_ROUND]
    sizes, octree, um, ut = check_build(morton, tri, level)
    if n > 1:
        run_min = np.array([tri[morton == c].min() for c in um[:400]])
        run_last = np.array([tri[morton == c][-1] for c in um[:400]])
        assert (ut[:400] != run_min).any() and (ut[:400] != run_last).any()
    assert sizes[0] == len(np.unique(morton))


@pytest.mark.parametrize('voxels', [SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1])
def test_build_voxel_counts_around_the_scan_block(voxels):
    rs = np.random.RandomState(voxels)
    codes = distinct_codes(voxels, 6, rs)
    morton = rs.permutation(np.concatenate([codes, codes[rs.randint(0, voxels, 200)]]))
    sizes, _, _, _ = check_build(morton, rs.randint(0, TRIANGLES, len(morton)), 6)
    assert sizes[0] == voxels and voxels in (1023, 1024, 1025)


@pytest.mark.parametrize('nodes', [SCAN_BLOCK, SCAN_BLOCK + 1])
def test_build_inner_node_counts_around_the_scan_block(nodes):
    """`nodes` cells of level 4 hold the voxels of level 6: the scans above the leaves read their length on the device and run on a
    grid sized by the pair count, here over more than one block of it"""
    rs = np.random.RandomState(nodes)
    cells = distinct_codes(nodes, 4, rs)
    below = np.repeat(cells, rs.randint(1, 4, nodes)) * 64
    morton = rs.permutation(below + rs.randint(0, 64, len(below)))
    sizes, _, _, _ = check_build(morton, rs.randint(0, TRIANGLES, len(morton)), 6)
    assert sizes[1 + 4] == nodes and nodes in (1024, 1025) and len(morton) > SCAN_BLOCK + 1
    assert sizes[1 + 5] > SCAN_BLOCK and sizes[0] > SCAN_BLOCK


def test_build_one_parent_chain_at_level_15():
    rs = np.random.RandomState(15)
    parent = int(rs.randint(0, 8 ** 14, dtype=np.int64)) | (1 << 41)         # the children's codes use bit 44
    morton = rs.permutation(np.repeat(parent * 8 + np.array([0, 2, 5, 7]), 5))
    sizes, octree, um, _ = check_build(morton, rs.randint(0, TRIANGLES, 20), 15)
    assert sizes == [4] + [1] * 15 and octree[-1] == 0b10100101 and int(um.max()) >> 44 == 1
    assert all(bin(int(b)).count('1') == 1 for b in octree[:-1])


@pytest.mark.parametrize('n', [1, 5, SORT_BLOCK + 1])
def test_build_level_0(n):
    """no key bits: the sort is a copy; one voxel, no octree bytes, the first triangle"""
    tri = np.random.RandomState(n).randint(1, TRIANGLES, n)
    sizes, octree, um, ut = check_build(np.zeros(n, np.int64), tri, 0)
    assert sizes == [1] and len(octree) == 0 and ut.tolist() == [tri[0]]


# ---- (d) two runs give the same bits ---------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical():
    import kaolin_amd as kal
    fv = random_soup(300, 5)
    sizes, _, _, _, pairs = compose(fv, 5)
    assert pairs == 3926 > SORT_BLOCK                                        # pairs that reach the sort
    first = kal.ops.conversions.unbatched_mesh_to_spc(fv.cuda(), 5)
    second = kal.ops.conversions.unbatched_mesh_to_spc(fv.cuda(), 5)
    assert first[1].numel() == sizes[0]
    for a, b in zip(first, second):
        bits = (lambda x: x.view(torch.int32)) if a.dtype == torch.float32 else (lambda x: x)
        assert a.dtype == b.dtype and torch.equal(bits(a), bits(b))
