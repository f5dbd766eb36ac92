"""The voxelizer's HIP pass (csrc/voxelgrid.hip) at the boundaries of its thread split, its normalisation cache, its extent
reduction and its grid fill, and on NaN vertices: every comparison is torch.equal against oracle/voxelgrid.py (or against the
reference-made fixture tests/golden/voxelgrid_edges.npz, to which the oracle is pinned as well).  The cases and what makes each a
boundary are in voxelgrid_boundary_cases.py; test_voxelgrid_boundary_cases_cpu.py proves the properties without a GPU.

Out of scope, on purpose: infinite coordinates (the reference never terminates on them and the kernel would walk every tree to its
depth cap), and a caller's ``scale`` small enough to bring a tree near the cap of L0 + 20 levels (4^20 nodes in one thread)."""
import numpy as np
import pytest
import torch

import voxelgrid_boundary_cases as cases
from conftest import GOLDEN_DIR
from oracle import voxelgrid as vox_oracle

pytestmark = pytest.mark.gpu
IDS = {torch.float32: 'f32', torch.float64: 'f64'}
dtypes = pytest.mark.parametrize('dtype', cases.DTYPES, ids=IDS.values())


def conv(vertices, faces, resolution, origin=None, scale=None, return_sparse=False):
    from kaolin_amd.ops.conversions import trianglemeshes_to_voxelgrids
    dev = [None if t is None else t.cuda() for t in (origin, scale)]
    return trianglemeshes_to_voxelgrids(vertices.cuda(), faces.cuda(), resolution, *dev, return_sparse=return_sparse)


def check(vertices, faces, resolution, origin=None, scale=None, expected=None, sparse=(False,)):
    if expected is None:
        expected = vox_oracle.trianglemeshes_to_voxelgrids(vertices, faces, resolution, origin, scale)
    for return_sparse in sparse:
        out = conv(vertices, faces, resolution, origin, scale, return_sparse)
        assert out.is_sparse == return_sparse and out.dtype == vertices.dtype and out.shape == expected.shape
        if return_sparse:
            assert out.is_coalesced()
            out = out.to_dense()
        assert torch.equal(out.cpu(), expected), int((out.cpu() != expected).sum())


@pytest.fixture(scope='module')
def edges():
    return np.load(cases.edges_path(GOLDEN_DIR))


# ---------------------------------------------------------------------------------------------------- A
@pytest.mark.parametrize('dtype,name,count', [(dt, n, c) for dt in cases.DTYPES for n, c in cases.a_cases(dt)],
                         ids=lambda v: IDS.get(v, str(v)))
def test_every_l0_against_shallower_equal_and_deeper_trees(dtype, name, count):
    """A base mesh's unique faces cycled to `count` rows: the same grid whatever the count (and so whatever L0), the oracle's on
    the unique faces"""
    vertices, faces, resolution, origin, scale = cases.a_base(name, dtype)
    check(vertices, cases.cycled(faces, count), resolution, origin, scale, expected=cases.a_expected(name, dtype))


@dtypes
def test_l0_9_sparse_result(dtype):
    """The deepest tree (11 levels under L0 = 9) through the bit grid"""
    vertices, faces, resolution, origin, scale = cases.a_base('deep_single', dtype)
    check(vertices, faces, resolution, origin, scale, expected=cases.a_expected('deep_single', dtype), sparse=(True,))


# ---------------------------------------------------------------------------------------------------- B
@pytest.mark.parametrize('resolution', [cases.B8_RES, cases.B8_RES_FLAT])
def test_l0_0_eight_spheres(resolution):
    """163 840 faces in 8 meshes: L0 = 0.  At R = 96 most faces subdivide once, at R = 32 none does"""
    vertices, faces = cases.sphere_batch(cases.B8_LEVEL, cases.B8_BATCH, torch.float32, 80)
    check(vertices, faces, resolution, expected=cases.b_expected(cases.B8_LEVEL, cases.B8_BATCH, torch.float32, 80, resolution, False))


@dtypes
@pytest.mark.parametrize('given', [False, True], ids=['default', 'given'])
def test_two_thousand_small_meshes(dtype, given):
    """More than two meshes per workgroup in the vertex part and in the face part, B * 32 extent workgroups"""
    vertices, faces = cases.sphere_batch(cases.MANY_LEVEL, cases.MANY_BATCH, dtype, 81)
    origin, scale = cases.given_norm(vertices, 82) if given else (None, None)
    expected = cases.b_expected(cases.MANY_LEVEL, cases.MANY_BATCH, dtype, 81, cases.MANY_RES, given)
    check(vertices, faces, cases.MANY_RES, origin, scale, expected=expected, sparse=(False, True))


# ---------------------------------------------------------------------------------------------------- C
@dtypes
@pytest.mark.parametrize('given', [False, True], ids=['default', 'given'])
def test_seven_tetrahedra(dtype, given):
    vertices, faces = cases.tet_batch(dtype)
    origin, scale = cases.given_norm(vertices, 5) if given else (None, None)
    check(vertices, faces, cases.TET_RES, origin, scale, sparse=(False, True))


@dtypes
def test_empty_face_list_marks_the_vertices(dtype):
    vertices, faces = cases.points_only(dtype)
    assert faces.shape == (0, 3)
    check(vertices, faces, 8, sparse=(False, True))
    origin, scale = cases.given_norm(vertices, 6)
    check(vertices, faces, 8, origin, scale)


@dtypes
def test_strided_vertices_and_faces(dtype):
    wide, cols = cases.strided_inputs(dtype)
    expected = vox_oracle.trianglemeshes_to_voxelgrids(wide[:, ::2], cols[:, ::2], 24)
    v, f = wide.cuda()[:, ::2], cols.cuda()[:, ::2]
    assert not v.is_contiguous() and not f.is_contiguous()
    from kaolin_amd.ops.conversions import trianglemeshes_to_voxelgrids
    for return_sparse in (False, True):
        out = trianglemeshes_to_voxelgrids(v, f, 24, return_sparse=return_sparse)
        assert torch.equal((out.to_dense() if return_sparse else out).cpu(), expected)


# ---------------------------------------------------------------------------------------------------- D
@dtypes
@pytest.mark.parametrize('V', cases.EXTENT_V)
def test_extent_reduction_extremes_at_slice_edges(V, dtype):
    """The vertex that alone holds the minimum (maximum) of every axis at index 0, 255, 256, 8191, 8192 and V - 1: one mesh per
    placement, then the first two and the first three placements as one batch"""
    meshes = [cases.extent_mesh(V, lo_at, hi_at, dtype) for lo_at, hi_at in cases.extent_places(V)]
    grids = [vox_oracle.trianglemeshes_to_voxelgrids(v[None], f, cases.EXTENT_RES) for v, f in meshes]
    for (vertices, faces), expected in zip(meshes, grids):
        check(vertices[None], faces, cases.EXTENT_RES, expected=expected)
    # a batch shares its faces: the vertex sets of the first placements under the faces of the first.  Every mesh keeps its
    # extremes at its own indices (as vertices no face uses, in the later meshes), and they alone set its origin and scale
    for batch in (2, 3):
        if len(meshes) >= batch:
            vertices = torch.stack([m[0] for m in meshes[:batch]])
            check(vertices, meshes[0][1], cases.EXTENT_RES)


# ---------------------------------------------------------------------------------------------------- E
@dtypes
@pytest.mark.parametrize('name', cases.EDGE_CASES)
def test_nan_and_coinciding_vertices_vs_reference(edges, name, dtype):
    """A face with a NaN corner is never subdivided, whichever corner it is (torch.max of its edges is NaN); a NaN under the
    default origin empties its own mesh only; coinciding vertices (scale 0) mark nothing"""
    v, f, res, org, sc, expected = cases.load_edge_case(edges, name, dtype)
    check(v, f, res, org, sc, expected=expected, sparse=(False, True))


# ---------------------------------------------------------------------------------------------------- F
def _dirty_allocator():
    """Leaves torch's cached free blocks full of 0xFF: the next torch.empty gets them"""
    junk = [torch.full((1 << 25,), -1, dtype=torch.int32, device='cuda')]                # 128 MiB, split for large requests
    junk += [torch.full((n,), -1, dtype=torch.int32, device='cuda') for n in (64, 1024, 16384, 131072, 1 << 20) for _ in range(4)]
    del junk


@pytest.mark.parametrize('resolution,batch', cases.DENSE_TAILS)
def test_dense_tail_on_dirty_memory(resolution, batch):
    """float32 grids whose size is no multiple of 16 bytes, after a long 16-byte body: the tail is cleared as well"""
    vertices, faces = cases.tail_mesh(batch)
    expected = vox_oracle.trianglemeshes_to_voxelgrids(vertices, faces, resolution)
    v, f = vertices.cuda(), faces.cuda()
    from kaolin_amd.ops.conversions import trianglemeshes_to_voxelgrids
    for _ in range(2):
        _dirty_allocator()
        out = trianglemeshes_to_voxelgrids(v, f, resolution)
        assert torch.equal(out.cpu(), expected)
        out.fill_(float('nan'))
        del out


@pytest.mark.parametrize('resolution,batch', cases.SPARSE_TAILS)
def test_sparse_tail_on_dirty_memory(resolution, batch):
    """Bit grids whose last word has padding bits: no index at or beyond R, the indices of dense.to_sparse()"""
    vertices, faces = cases.tail_mesh(batch)
    expected = vox_oracle.trianglemeshes_to_voxelgrids(vertices, faces, resolution)
    v, f = vertices.cuda(), faces.cuda()
    from kaolin_amd.ops.conversions import trianglemeshes_to_voxelgrids
    want = trianglemeshes_to_voxelgrids(v, f, resolution).to_sparse()
    assert torch.equal(want.to_dense().cpu(), expected)
    for _ in range(2):
        _dirty_allocator()
        got = trianglemeshes_to_voxelgrids(v, f, resolution, return_sparse=True)
        assert got.is_sparse and got.is_coalesced() and got.shape == want.shape and got.dtype == want.dtype
        assert int(got.indices()[1:].max()) < resolution and int(got.indices().min()) >= 0 and int(got.indices()[0].max()) < batch
        assert torch.equal(got.indices(), want.indices()) and torch.equal(got.values(), want.values())
        del got
