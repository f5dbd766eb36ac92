"""CPU side of the voxelizer's boundary suite: every case of voxelgrid_boundary_cases.py has the property it is named for,
measured in the oracle (oracle/voxelgrid.py), never in the code under test; the oracle itself is pinned to the reference-made
fixture tests/golden/voxelgrid_edges.npz (NaN vertices, coinciding vertices); and the package's torch path (CPU tensors, half
precision: ops/conversions/trianglemesh.py ``_torch_dense``) is checked against the reference's goldens and against the oracle.
No GPU."""
import os

import numpy as np
import pytest
import torch

import voxelgrid_boundary_cases as cases
from conftest import GOLDEN_DIR
from oracle import voxelgrid as vox_oracle
from test_voxelgrid import CASES as GOLDEN_CASES, load_case


def torch_path(*args, **kwargs):
    from kaolin_amd.ops.conversions import trianglemeshes_to_voxelgrids
    return trianglemeshes_to_voxelgrids(*args, **kwargs)


@pytest.fixture(scope='module')
def edges():
    return np.load(cases.edges_path(GOLDEN_DIR))


@pytest.fixture(scope='module')
def gold():
    return np.load(os.path.join(GOLDEN_DIR, 'voxelgrid.npz'))


# ---------------------------------------------------------------------------------------------------- A
def test_l0_rule_and_thresholds():
    """The restated rule: the documented values, every L0 of 0 .. 9 among the cases, and both sides of every threshold"""
    assert [cases.l0_of(1, n) for n in (1, 2, 3, 9, 10, 624, 625, 159999, 160000, 10 ** 7)] == [9, 9, 8, 8, 7, 5, 4, 1, 0, 0]
    assert cases.l0_of(8, 20480) == 0 and cases.l0_of(2000, 80) == 0 and cases.l0_of(1, 0) == 0
    for below, above in cases.BF_THRESHOLDS:
        assert cases.l0_of(1, below) == cases.l0_of(1, above) + 1
    counts = {count for _, count in cases.A_CASES}
    assert {cases.l0_of(1, n) for n in counts} == set(range(10))
    for below, above in cases.BF_THRESHOLDS:
        assert below in counts and above in counts, (below, above)
    for dtype in cases.DTYPES:
        assert {cases.l0_of(1, n) for _, n in cases.a_cases(dtype)} >= set(cases.A_BOTH_DTYPES_L0)


@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_a_trees_against_every_l0(dtype):
    """Per L0, the unique faces of the cases that run it hold a tree of no level, one at least two levels shallower (L0 >= 2), one
    of exactly L0 levels and one at least two levels deeper; every tree is full (4^r triangles kept in round r), so each of its
    branches has that depth; and no call walks more than 10^9 nodes"""
    for name, spec in cases.A_BASES.items():
        kept = cases.a_depths(name, dtype)
        assert tuple(len(k) for k in kept) == spec['depths'], (name, kept)
        assert all(k == tuple(4 ** r for r in range(len(k))) for k in kept), (name, kept)
    by_l0 = {}
    for name, count in cases.A_CASES:
        depths = cases.A_BASES[name]['depths']
        assert count >= len(depths)
        by_l0.setdefault(cases.l0_of(1, count), set()).update(depths)
        nodes = -(-count // len(depths)) * sum((4 ** (d + 1) - 1) // 3 for d in depths)
        assert nodes <= 10 ** 9, (name, count, nodes)
        if cases.A_BASES[name]['resolution'] == 256 and len(depths) > 3:
            assert count <= 624
    for l0 in range(10):
        depths = by_l0[l0]
        assert 0 in depths and l0 in depths and any(d >= l0 + 2 for d in depths), (l0, depths)
        # (at L0 = 2 the tree two levels shallower is the empty one; from L0 = 3 on there is one that subdivides first)
        assert l0 < 3 or any(0 < d <= l0 - 2 for d in depths), (l0, depths)
    assert any(d > 9 for d in by_l0[9])
    for name in cases.A_BASES:
        expected = cases.a_expected(name, dtype)
        assert expected.shape[1] <= 256 and int(expected.sum()) > 3 * len(cases.A_BASES[name]['depths'])


# ---------------------------------------------------------------------------------------------------- B
def test_sphere_batch_subdivides_at_96_and_not_at_32():
    vertices, faces = cases.sphere_batch(cases.B8_LEVEL, cases.B8_BATCH, torch.float32, 80)
    assert cases.l0_of(vertices.shape[0], faces.shape[0]) == 0 and vertices.shape[0] * faces.shape[0] == 163840
    normed = cases.normalised(vertices, None, None)
    for b in range(vertices.shape[0]):
        assert cases.kept_per_round(normed[b], faces.numpy(), cases.B8_RES_FLAT) == []
        assert cases.kept_per_round(normed[b], faces.numpy(), cases.B8_RES)[0] > faces.shape[0] // 2
    for res in (cases.B8_RES, cases.B8_RES_FLAT):
        grids = cases.b_expected(cases.B8_LEVEL, cases.B8_BATCH, torch.float32, 80, res, False)
        assert all(not torch.equal(grids[b], grids[b + 1]) for b in range(cases.B8_BATCH - 1))


@pytest.mark.parametrize('given', [False, True])
def test_many_small_meshes_differ_from_their_neighbours(given):
    """2 000 meshes of 42 vertices and 80 faces: a workgroup of 256 threads spans more than two of them in the vertex part and in
    the face part (L0 = 0), and every mesh's grid differs from both neighbours': a normalisation taken from the mesh before or
    after cannot pass"""
    vertices, faces = cases.sphere_batch(cases.MANY_LEVEL, cases.MANY_BATCH, torch.float32, 81)
    B, V, F = vertices.shape[0], vertices.shape[1], faces.shape[0]
    assert (V, F) == (42, 80) and cases.l0_of(B, F) == 0 and 256 > 2 * V and 256 > 2 * F * 4 ** cases.l0_of(B, F)
    # the first launch is sized by its B * VOX_NP extent workgroups, not by the 16-byte stores of the fill (256 per workgroup)
    assert B > 128 and -(-(B * cases.MANY_RES ** 3 * 4 // 16) // 256) < B * cases.VOX_NP
    for dtype in cases.DTYPES:
        grids = cases.b_expected(cases.MANY_LEVEL, cases.MANY_BATCH, dtype, 81, cases.MANY_RES, given)
        flat = grids.reshape(B, -1)
        assert bool((flat[1:] != flat[:-1]).any(dim=1).all())
        assert bool((flat[2:] != flat[:-2]).any(dim=1).all())   # (s_n[1] read for mesh b0 + 2, or the other way round)
        assert int(flat.sum(dim=1).min()) > 8


# ---------------------------------------------------------------------------------------------------- C
def test_tiny_batches_span_workgroups():
    vertices, faces = cases.tet_batch(torch.float32)
    assert vertices.shape == (7, 4, 3) and cases.l0_of(7, 4) == 7 and vertices.shape[1] < 128 and vertices.shape[0] >= 3
    grids = vox_oracle.trianglemeshes_to_voxelgrids(vertices, faces, cases.TET_RES)
    assert all(not torch.equal(grids[b], grids[b + 1]) for b in range(6))
    points, none = cases.points_only(torch.float32)
    only = vox_oracle.trianglemeshes_to_voxelgrids(points, none, 8)
    assert none.shape == (0, 3) and [int(g.sum()) for g in only] == [5, 5]


# ---------------------------------------------------------------------------------------------------- D
@pytest.mark.parametrize('V', cases.EXTENT_V)
def test_extent_cases_hinge_on_one_vertex(V):
    """The minimum of every axis is held by vertex lo_at alone and the maximum by hi_at alone, at the indices asked for, and the
    oracle's grid changes when either is taken away"""
    step = cases.VOX_NP * cases.VOX_SLICE                # a slice's thread t reads vertices slice * 256 + t + k * 8192
    assert cases.EXTENT_AT == (0, cases.VOX_SLICE - 1, cases.VOX_SLICE, step - 1, step)
    places = cases.extent_places(V)
    at = {i for i in cases.EXTENT_AT if i < V} | {V - 1}
    assert {p[0] for p in places} == at and {p[1] for p in places} == at
    for lo_at, hi_at in places:
        for dtype in cases.DTYPES:
            vertices, faces = cases.extent_mesh(V, lo_at, hi_at, dtype)
            assert vertices.shape == (V, 3)
            lo, hi = vertices.min(dim=0)[0], vertices.max(dim=0)[0]
            assert bool(((vertices == lo).sum(dim=0) == 1).all()) and torch.equal(vertices[lo_at], lo)
            assert bool(((vertices == hi).sum(dim=0) == 1).all()) and torch.equal(vertices[hi_at], hi)
            grid = vox_oracle.trianglemeshes_to_voxelgrids(vertices[None], faces, cases.EXTENT_RES)
            for index in (lo_at, hi_at):
                other = vox_oracle.trianglemeshes_to_voxelgrids(cases.without_vertex(vertices, index)[None], faces, cases.EXTENT_RES)
                assert not torch.equal(grid, other), (V, lo_at, hi_at, index)


# ---------------------------------------------------------------------------------------------------- E
@pytest.mark.parametrize('dtype', cases.DTYPES)
@pytest.mark.parametrize('name', cases.EDGE_CASES)
def test_oracle_and_torch_path_vs_reference_edges(edges, name, dtype):
    v, f, res, org, sc, expected = cases.load_edge_case(edges, name, dtype)
    out = vox_oracle.trianglemeshes_to_voxelgrids(v, f, res, org, sc)
    assert out.dtype == dtype and torch.equal(out, expected)
    for sparse in (False, True):
        got = torch_path(v, f, res, org, sc, return_sparse=sparse)
        assert got.is_sparse == sparse and got.dtype == dtype
        assert torch.equal(got.to_dense() if sparse else got, expected)


def test_edge_fixture_holds_the_cases_it_is_named_for(edges):
    inputs = cases.edge_case_inputs()
    assert set(inputs) == set(cases.EDGE_CASES)
    for name, (v, f, res, org, sc) in inputs.items():
        gv, gf, gres, gorg, gsc, _ = cases.load_edge_case(edges, name, torch.float32)
        assert torch.equal(torch.nan_to_num(gv, nan=7.0), torch.nan_to_num(v, nan=7.0)) and torch.equal(gf, f) and gres == res
        assert (org is None) == (gorg is None) and (org is None or (torch.equal(org, gorg) and torch.equal(sc, gsc)))
    for dtype in cases.DTYPES:
        # the lone faces: the reference marks the three vertices' voxels at most -- no midpoint -- although the finite edge is
        # long enough to subdivide: a rule that ignores a NaN edge marks more
        for name in cases.NAN_LONE:
            v, f, res, org, sc, expected = cases.load_edge_case(edges, name, dtype)
            assert int(expected.sum()) == 3 and int(torch.isnan(v).any(dim=2).sum()) == 1
            finite = [i for i in f[0].tolist() if not bool(torch.isnan(v[0, i]).any())]
            edge2 = float(((v[0, finite[0]] - v[0, finite[1]]) ** 2).sum())
            assert edge2 > 100 * ((res - 1) / res ** 2) ** 2
            pair = torch.tensor([[finite[0], finite[1], finite[1]]])
            assert int(vox_oracle.trianglemeshes_to_voxelgrids(torch.nan_to_num(v, nan=0.5), pair, res, org, sc).sum()) > 4
        v, f, res, org, sc, expected = cases.load_edge_case(edges, 'nan_batch3', dtype)
        assert int(expected[1].sum()) == 0 and bool(torch.isnan(v[1]).any()) and not bool(torch.isnan(v[[0, 2]]).any())
        for b in (0, 2):
            assert torch.equal(expected[b:b + 1], vox_oracle.trianglemeshes_to_voxelgrids(v[b:b + 1], f, res))
            assert int(expected[b].sum()) > 50
        v, f, res, org, sc, expected = cases.load_edge_case(edges, 'coincide', dtype)
        assert int(expected.sum()) == 0 and bool((v == v[:, :1]).all())
        v, f, res, org, sc, expected = cases.load_edge_case(edges, 'nan_closed', dtype)
        assert int(expected.sum()) > 100 and int(torch.isnan(v).any(dim=2).sum()) == 1


# ---------------------------------------------------------------------------------------------------- F
def test_tail_shapes():
    for res, batch in cases.DENSE_TAILS:
        assert (batch * res ** 3 * 4) % 16 != 0 and batch * res ** 3 * 4 > 10 ** 6
    for res, batch in cases.SPARSE_TAILS:
        assert res ** 3 % 32 != 0 and batch >= 2
    for res, batch in cases.DENSE_TAILS + cases.SPARSE_TAILS:
        vertices, faces = cases.tail_mesh(batch)
        grids = vox_oracle.trianglemeshes_to_voxelgrids(vertices, faces, res)
        # the mesh that sets the tail of the whole allocation reaches the last plane of its longest axis
        assert bool(grids[-1].nonzero().max(dim=0)[0].max() == res - 1)


# ---------------------------------------------------------------------------------------------------- G: the torch path
@pytest.mark.parametrize('name', GOLDEN_CASES)
def test_torch_path_vs_reference_golden(gold, name):
    v, f, res, org, sc, expected = load_case(gold, name)
    out = torch_path(v, f, res, org, sc)
    assert out.dtype == v.dtype and out.device.type == 'cpu' and torch.equal(out, expected)
    sparse = torch_path(v, f, res, org, sc, return_sparse=True)
    assert sparse.is_sparse and torch.equal(sparse.to_dense(), expected)


@pytest.mark.parametrize('dtype', cases.DTYPES)
def test_torch_path_vs_oracle_small_cases(dtype):
    for name, count in (('shallow', 7), ('shallow', 625), ('deep_pair_short', 2), ('deep_pair', 2)):
        vertices, faces, res, origin, scale = cases.a_base(name, dtype)
        assert torch.equal(torch_path(vertices, cases.cycled(faces, count), res, origin, scale), cases.a_expected(name, dtype))
    vertices, faces = cases.tet_batch(dtype)
    assert torch.equal(torch_path(vertices, faces, cases.TET_RES), vox_oracle.trianglemeshes_to_voxelgrids(vertices, faces, cases.TET_RES))
    origin, scale = cases.given_norm(vertices, 5)
    assert torch.equal(torch_path(vertices, faces, cases.TET_RES, origin, scale),
                       vox_oracle.trianglemeshes_to_voxelgrids(vertices, faces, cases.TET_RES, origin, scale))
    points, none = cases.points_only(dtype)
    assert torch.equal(torch_path(points, none, 8), vox_oracle.trianglemeshes_to_voxelgrids(points, none, 8))
    wide, cols = cases.strided_inputs(dtype)
    vertices, faces = wide[:, ::2], cols[:, ::2]
    assert not vertices.is_contiguous() and not faces.is_contiguous()
    assert torch.equal(torch_path(vertices, faces, 24), vox_oracle.trianglemeshes_to_voxelgrids(vertices, faces, 24))


def test_torch_path_half_precision_vs_oracle():
    """float16 goes through the torch path on any device; the oracle carries its arithmetic out in float16 as well"""
    vertices, faces = cases.tet_batch(torch.float32)
    vertices = vertices.half()
    out = torch_path(vertices, faces, cases.TET_RES)
    assert out.dtype == torch.float16 and torch.equal(out, vox_oracle.trianglemeshes_to_voxelgrids(vertices, faces, cases.TET_RES))
