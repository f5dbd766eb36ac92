"""unbatched_mesh_to_spc on the CPU: the references the GPU tests lean on, checked against each other.

oracle/mesh_to_spc_oracle.inc is the proposal-list algorithm of the HIP path in the same arithmetic, with a sort whose tie-break
rests on the C library.  tests/mesh_to_spc_bruteforce.py says independently what a voxel must report:
  * ``dense`` (every voxel x every triangle, argmax over the triangle axis) against the oracle, Morton codes and face ids
    ``array_equal``, on the reference's 4-triangle case, random soups, ties between equal triangles and the scenes of
    tests/test_mesh_to_spc_boundaries_gpu.py that fit its size limit;
  * ``subtree`` and ``build``, composed stage after stage as kaolin_amd/_C/ops.py composes the C ABI, against the oracle at levels
    0, 1, 3, 4, 12, 13 and 15 -- beyond the reach of ``dense``;
  * degenerate triangles: a point and a triangle with two equal vertices (NaN edge axes) yield nothing, a collinear triangle and a
    triangle inside a voxel-boundary plane yield voxels.
Also the scenes shared with the GPU file.  No GPU, no project code besides the oracle."""
import numpy as np
import pytest
import torch

import mesh_to_spc_bruteforce as bf
import oracle
from test_mesh_to_spc import random_soup, reference_case

STAGE_LEVELS = 3        # levels a stage finishes below its proposals (kamd_mesh_to_spc_stage_levels)
DENSE_LIMIT = 1_500_000  # triangle x voxel tests at the deepest level that `dense` may take


# ---- scenes (shared with tests/test_mesh_to_spc_boundaries_gpu.py) ---------------------------------------------------------------
def small_triangles(level, cells, seed, width=3.0):
    """one triangle per cell (x, y, z) of `level`: the cell's centre plus offsets of up to `width` voxels per coordinate"""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 1, 3)
    off = (np.random.RandomState(seed).rand(cells.shape[0], 3, 3) * 2.0 - 1.0) * width
    size = 2.0 / (1 << level)
    return torch.from_numpy(((cells + 0.5 + off) * size - 1.0).astype(np.float32)).contiguous()


def deep_scene(kind, level):
    """a handful of triangles a few voxels wide at `level`.  'random': anywhere; 'top_bit': x in the upper half, so the codes use
    bit 3 level - 1 (bit 44 at level 15); 'centre': around the origin, so x, y and z all carry across their top bit"""
    n = 1 << level
    rs = np.random.RandomState(100 + level)
    if kind == 'random':
        return small_triangles(level, rs.randint(8, n - 8, (5, 3)), level)
    if kind == 'top_bit':
        cells = rs.randint(8, n - 8, (4, 3))
        cells[:, 0] = rs.randint(n // 2 + 8, n - 8, 4)
        return small_triangles(level, cells, level + 1)
    assert kind == 'centre'
    fv = small_triangles(level, np.full((3, 3), n // 2), level + 2, width=2.0)
    fv[0] = torch.tensor([[-1.5, -1.0, -1.2], [1.4, 1.1, -0.6], [0.3, -0.7, 1.6]]) * (2.0 / n)   # through all eight octants
    return fv.contiguous()


DEEP_CASES = [('random', 10), ('random', 12), ('centre', 12), ('random', 13), ('centre', 13), ('random', 15), ('top_bit', 15),
              ('centre', 15)]

DEGENERATE = {
    'point': [[0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [0.1, 0.2, 0.3]],
    'two_equal': [[0.1, 0.2, 0.3], [0.1, 0.2, 0.3], [0.5, 0.5, 0.5]],
    'collinear': [[-0.5, 0.0, 0.0], [0.0, 0.0, 0.0], [0.5, 0.0, 0.0]],
    'in_plane': [[0.0, -0.5, -0.25], [0.0, 0.5, -0.25], [0.0, 0.25, 0.75]],       # all x = 0: the boundary plane of every level
}
YIELDS_NOTHING = ('point', 'two_equal')


def degenerate(name):
    return torch.tensor([DEGENERATE[name]])


MIXED_AT = (0, 7, 20, 43)   # where the four degenerate triangles sit in `mixed_soup`: first, inside, last


def mixed_soup(seed=5):
    """random_soup(40) with the four degenerate triangles inserted -> (44 triangles, indices of the 40 in the result)"""
    soup = random_soup(40, seed)
    rows, kept, it = [], [], iter(range(40))
    for i in range(44):
        if i in MIXED_AT:
            rows.append(degenerate(list(DEGENERATE)[MIXED_AT.index(i)])[0])
        else:
            rows.append(soup[next(it)])
            kept.append(i)
    return torch.stack(rows).contiguous(), soup, torch.tensor(kept)


def tie_soup():
    """one triangle four times, at indices 3, 11, 12 and 29 of a 33-triangle soup, and a second one twice (17, 30) crossing it: in
    the proposal list the winner of a shared voxel is neither the first nor the last entry"""
    fv = random_soup(33, 9, size=0.5)
    fv[[3, 11, 12, 29]] = torch.tensor([[-0.6, -0.5, -0.1], [0.7, -0.4, 0.2], [0.0, 0.6, 0.1]])
    fv[[17, 30]] = torch.tensor([[-0.5, 0.1, -0.6], [0.6, 0.0, -0.5], [0.1, 0.2, 0.7]])
    return fv.contiguous()


# ---- the composed reference -------------------------------------------------------------------------------------------------------
def compose(face_vertices, level, depth=STAGE_LEVELS):
    """the host sequence of kaolin_amd/_C/ops.py:mesh_to_spc_cuda on the numpy stage references
    -> (sizes, octree, voxel codes, face ids, number of pairs before the sort), or None where nothing is occupied"""
    fv = face_vertices.numpy()
    morton, tri = np.zeros(fv.shape[0], np.int64), np.arange(fv.shape[0], dtype=np.int64)
    level_from, tested = 0, 0
    while True:
        level_to = min(level_from + depth, level)
        counts, morton, tri = bf.subtree(fv, morton, tri, level_from, level_to, tested)
        assert int(counts.sum()) == len(morton) == len(tri)
        if len(morton) == 0:
            return None
        if level_to == level:
            break
        level_from, tested = level_to, 1
    return bf.build(morton, tri, level) + (len(morton),)


def assert_dense_matches_oracle(fv, level):
    assert fv.shape[0] * 8 ** level <= DENSE_LIMIT
    morton, face = bf.dense(fv.numpy(), level)
    ref = oracle.mesh_to_spc(fv, level, return_mortons=True)
    assert np.array_equal(morton, ref[3].numpy())
    assert np.array_equal(face, ref[1].numpy())
    return morton, face


def assert_compose_matches_oracle(fv, level):
    ref = oracle.mesh_to_spc(fv, level, return_mortons=True)
    got = compose(fv, level)
    if got is None:
        assert ref[1].shape == (0,) and ref[0].shape == (0,)
        return None
    sizes, octree, um, ut, pairs = got
    assert np.array_equal(um, ref[3].numpy()) and np.array_equal(ut, ref[1].numpy())
    assert np.array_equal(octree, ref[0].numpy()) and sizes[0] == len(um) and sum(sizes[1:]) == len(octree)
    return got


# ---- dense against the oracle -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name, level, voxels', [('reference', 3, 65), ('soup40', 5, 526), ('soup300', 4, 1311)])
def test_dense_matches_oracle(name, level, voxels):
    fv = {'reference': reference_case, 'soup40': lambda: random_soup(40, 3), 'soup300': lambda: random_soup(300, 4)}[name]()
    morton, _ = assert_dense_matches_oracle(fv, level)
    assert len(morton) == voxels


def test_dense_matches_oracle_on_ties():
    fv = tie_soup()
    morton, face = assert_dense_matches_oracle(fv, 4)
    c, half = bf.centres(morton, 4)
    live = bf.passes(fv.numpy()[:, None], c[None], half)                     # leaf test only: a superset of the live triangles
    assert set(np.unique(face)) >= {3, 17}
    for first, copies in ((3, [11, 12, 29]), (17, [30])):
        mine = face == first
        assert mine.sum() > 10 and live[copies][:, mine].all()               # every copy touches the voxel, the first one wins
    assert not np.isin(face, [11, 12, 29, 30]).any()
    assert (live[:, face == 17].sum(0) >= 3).any() and (face[live[3] & live[17]] == 3).all()


@pytest.mark.parametrize('F', [1, 7, 8, 9, 31, 32, 33, 1023, 1024, 1025])
def test_dense_matches_oracle_on_the_triangle_counts(F):
    morton, face = assert_dense_matches_oracle(random_soup(F, F), 2)
    assert len(morton) > 0


def test_dense_matches_oracle_on_the_mixed_soup():
    fv, soup, kept = mixed_soup()
    morton, face = assert_dense_matches_oracle(fv, 4)
    plain = oracle.mesh_to_spc(soup, 4, return_mortons=True)
    # the point and the two-equal-vertices triangle emit nothing; the other two may add voxels, never take one from a smaller index
    assert not np.isin(face, [MIXED_AT[0], MIXED_AT[1]]).any()
    assert np.isin(plain[3].numpy(), morton).all()
    at = np.searchsorted(morton, plain[3].numpy())
    undisturbed = kept.numpy()[plain[1].numpy()]
    mine = np.isin(face[at], kept.numpy())
    assert mine.sum() > 100 and np.array_equal(face[at][mine], undisturbed[mine])
    assert (face[at][~mine] < undisturbed[~mine]).all()                      # only a smaller index may take a voxel over


# ---- subtree and build against the oracle ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('level', [0, 1, 3, 4])
def test_composed_stages_match_oracle_on_a_soup(level):
    got = assert_compose_matches_oracle(random_soup(40, level), level)
    assert got[0][0] > 0


@pytest.mark.parametrize('kind, level', DEEP_CASES)
def test_composed_stages_match_oracle_at_deep_levels(kind, level):
    """levels 12 / 13 / 15: four, five and five stages, level 13 ends on a one-level stage; codes beyond 32 bits"""
    sizes, octree, um, ut, pairs = assert_compose_matches_oracle(deep_scene(kind, level), level)
    assert 10 <= sizes[0] <= 2000 and len(np.unique(ut)) >= 2
    x, y, z = bf.to_point(um)
    if kind == 'top_bit':
        assert ((um >> (3 * level - 1)) & 1).all() and (level != 15 or int(um.max()) >> 44 == 1)
    if kind == 'centre':
        for g in (x, y, z):
            assert g.min() < (1 << (level - 1)) <= g.max()
    if level >= 11:
        assert int(um.max()) >= 1 << 32


def test_composed_stages_match_oracle_on_ties_and_mixed():
    assert_compose_matches_oracle(tie_soup(), 4)
    assert_compose_matches_oracle(mixed_soup()[0], 4)


def test_composed_stages_match_dense():
    fv = random_soup(40, 3)
    sizes, octree, um, ut, pairs = compose(fv, 5)
    morton, face = bf.dense(fv.numpy(), 5)
    assert np.array_equal(um, morton) and np.array_equal(ut, face) and pairs > len(um)


def test_build_keeps_the_first_pair_of_a_run():
    """not the minimum: the first in input order"""
    sizes, octree, um, ut = bf.build([9, 8, 9, 8, 15], [5, 7, 1, 2, 0], 2)
    assert um.tolist() == [8, 9, 15] and ut.tolist() == [7, 5, 0]
    assert sizes == [3, 1, 1] and octree.tolist() == [0b10, 0b10000011]


# ---- degenerate triangles through the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', YIELDS_NOTHING)
@pytest.mark.parametrize('level', [0, 1, 3, 12])
def test_point_and_two_equal_vertices_yield_nothing(name, level):
    octree, face_idx, bary = oracle.mesh_to_spc(degenerate(name), level)
    assert octree.shape == (0,) and face_idx.shape == (0,) and bary.shape == (0, 3)
    assert compose(degenerate(name), level) is None
    if level <= 3:
        assert len(bf.dense(degenerate(name).numpy(), level)[0]) == 0


def test_collinear_triangle_yields_voxels():
    """three distinct collinear vertices: every edge axis is finite, the normal axis is the zero vector and separates nothing.
    24 voxels at level 3; at level 0 the root voxel itself (and an octree of no bytes)"""
    fv = degenerate('collinear')
    morton, face = assert_dense_matches_oracle(fv, 3)
    assert len(morton) == 24
    x, y, z = bf.to_point(morton)
    assert set(x.tolist()) == {1, 2, 3, 4, 5, 6} and set(y.tolist()) == {3, 4} and set(z.tolist()) == {3, 4}
    octree, face_idx, bary = oracle.mesh_to_spc(fv, 0)
    assert octree.shape == (0,) and face_idx.tolist() == [0] and len(bf.dense(fv.numpy(), 0)[0]) == 1
    assert_compose_matches_oracle(fv, 3)
    assert_compose_matches_oracle(fv, 12)


@pytest.mark.parametrize('level', [1, 3, 4])
def test_triangle_in_a_boundary_plane_yields_both_sides(level):
    """x = 0 is a face of the voxels on either side at every level, and `<=` keeps both: the result is symmetric in x"""
    fv = degenerate('in_plane')
    morton, face = assert_dense_matches_oracle(fv, level)
    x, y, z = bf.to_point(morton)
    h = 1 << (level - 1)
    assert set(x.tolist()) == {h - 1, h}
    left, right = x == h - 1, x == h
    assert left.sum() == right.sum() > 0
    assert sorted(zip(y[left].tolist(), z[left].tolist())) == sorted(zip(y[right].tolist(), z[right].tolist()))
    assert_compose_matches_oracle(fv, level)


def test_triangle_in_a_boundary_plane_at_level_12():
    sizes, octree, um, ut, pairs = assert_compose_matches_oracle(degenerate('in_plane') * 2.0 ** -8, 12)
    x, _, _ = bf.to_point(um)
    assert set(x.tolist()) == {2047, 2048}
