"""kaolin.ops.mesh.subdivide_tetmesh / inverse_vertices_offset without a GPU: the package's torch formulation against every case
the reference recorded (tests/golden/subdivide_tetmesh.npz, written by make_golden_subdivide_tetmesh.py), the argument checks,
and the host-only parts of the HIP path (index-range check, workspace query)."""
import builtins
import re

import pytest
import torch

import kaolin_amd as kal
from kaolin_amd import _C, _lib
from kaolin_amd.ops.mesh import inverse_vertices_offset, subdivide_tetmesh, tetmesh
from subdivide_tetmesh_golden import (CASES, DTYPES, G, case_inputs, check_gradients, child_blocks, cotangents, expected, same,
                                      tensor)


def raises_like(name):
    kind, text = (str(x) for x in G[f'err_{name}'])
    return pytest.raises(getattr(builtins, kind), match=re.escape(text))


@pytest.mark.parametrize('tag,dtype', DTYPES)
@pytest.mark.parametrize('case', CASES)
def test_matches_reference(case, tag, dtype):
    vertices, tets, features = case_inputs(case)
    want_vertices, want_tets, want_features = expected(case, tag, dtype)
    out = subdivide_tetmesh(vertices.to(dtype), tets, features.to(dtype))
    assert isinstance(out, tuple) and len(out) == 3
    assert same(out[0], want_vertices) and same(out[1], want_tets) and same(out[2], want_features), case
    two = subdivide_tetmesh(vertices.to(dtype), tets)
    assert isinstance(two, tuple) and len(two) == 2 and same(two[0], want_vertices) and same(two[1], want_tets)
    if case == 'grid9':
        one = subdivide_tetmesh(vertices.to(dtype), tets, features[..., :1].to(dtype))
        assert same(one[2][:, 1000:], tensor(f'grid9_d1_mid_features_{tag}')) and same(one[2][:, :1000], features[..., :1].to(dtype))


def test_reference_test_expectations():
    """The tensors the reference's own unit test expects (its bound: torch.equal)."""
    for case in ('kat1', 'kat2'):
        vertices, tets, features = case_inputs(case)
        new_vertices, new_tets, new_features = subdivide_tetmesh(vertices, tets, features)
        assert torch.equal(new_vertices, tensor('kat_expected_vertices')) and torch.equal(new_features, tensor('kat_expected_features'))
        assert torch.equal(new_tets, tensor(f'{case}_expected_tets'))


def test_child_table_matches_blocks():
    """The module's CHILD_TETS against the eight blocks spelled out next to the goldens."""
    tets = torch.tensor([[0, 1, 2, 3], [3, 1, 0, 2]])
    slots = torch.arange(12).reshape(2, 6) + 10
    columns = torch.cat([tets, slots], dim=1)
    assert torch.equal(columns[:, torch.tensor(tetmesh.CHILD_TETS)].permute(1, 0, 2).reshape(-1, 4), child_blocks(tets, slots))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.half])
def test_no_tetrahedrons(dtype):
    vertices, tets, features = case_inputs('grid9')
    new_vertices, new_tets, new_features = subdivide_tetmesh(vertices.to(dtype), tets[:0], features.to(dtype))
    assert same(new_vertices, vertices.to(dtype)) and same(new_features, features.to(dtype))
    assert same(new_tets, tensor('empty_new_tets')) and new_tets.shape == (0, 4) and new_tets.dtype == torch.long
    assert len(subdivide_tetmesh(vertices.to(dtype), tets[:0])) == 2


@pytest.mark.parametrize('tag,dtype', DTYPES)
@pytest.mark.parametrize('case', ['grid9', 'sparse_ids'])
def test_gradients_match_reference(case, tag, dtype):
    vertices, tets, features = case_inputs(case)
    cot_v, cot_f = cotangents(case)
    p, f = vertices.to(dtype).requires_grad_(), features.to(dtype).requires_grad_()
    new_vertices, new_tets, new_features = subdivide_tetmesh(p, tets, f)
    assert new_vertices.requires_grad and new_features.requires_grad and not new_tets.requires_grad
    ((new_vertices * cot_v.to(dtype)).sum() + (new_features * cot_f.to(dtype)).sum()).backward()
    check_gradients(case, tag, p.grad, f.grad, cot_v, cot_f)


def test_other_dtypes():
    """half, int32 tetrahedrons, float32 vertices with float64 features: the reference's dtypes (its ``cat`` promotes)."""
    vertices, tets, features = case_inputs('grid9')
    _, want_tets, _ = expected('grid9', 'f64', torch.float64)
    for name, args in (('half', (vertices.half(), tets, features.half())), ('int32_tets', (vertices, tets.int(), features)),
                       ('mixed', (vertices, tets, features.double()))):
        out = subdivide_tetmesh(*args)
        assert [str(o.dtype) for o in out] == [str(x) for x in G[f'dtypes_{name}']], name
        assert same(out[1], want_tets)
    mixed = subdivide_tetmesh(vertices, tets, features.double())
    want = expected('grid9', 'f64', torch.float64)
    assert same(mixed[0], want[0]) and same(mixed[2], want[2])        # float32 values widen exactly


def test_recorded_errors():
    vertices, _, features = case_inputs('grid9')
    vertices, features, tets = vertices[:, :8], features[:, :8], torch.tensor([[0, 1, 2, 3], [4, 5, 6, 7]])
    with raises_like('tets_width'):
        subdivide_tetmesh(vertices, tets[:, :3], features)
    with raises_like('tets_float'):
        subdivide_tetmesh(vertices, tets.float(), features)
    with raises_like('features_rows'):
        subdivide_tetmesh(vertices, tets, features[:, :7])


def test_index_range_check():
    tets = torch.tensor([[0, 1, 2, 3], [4, 5, 6, 7]])
    vertices, features = torch.rand(1, 8, 3), torch.rand(1, 8, 2)
    assert subdivide_tetmesh(vertices, tets, features)[1].shape == (16, 4)
    with pytest.raises(IndexError, match='outside'):
        subdivide_tetmesh(vertices[:, :7], tets, features[:, :7])      # an entry equal to V
    low = tets.clone()
    low[1, 2] = -1
    with pytest.raises(IndexError, match='-1'):
        subdivide_tetmesh(vertices, low)
    with pytest.raises(IndexError, match='outside'):
        _C.ops.mesh.subdivide_tetmesh_cuda(tets, 7)                     # the range check comes before every other
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        _C.ops.mesh.subdivide_tetmesh_cuda(tets, 8)
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        _C.ops.mesh.tetmesh_midpoints_forward_cuda(vertices, features, torch.zeros(0, 2, dtype=torch.long))


def test_inverse_vertices_offset():
    got = inverse_vertices_offset(tensor('ivo_tet_vertices'))
    assert got.shape == (1, 1, 3, 3) and torch.allclose(got, tensor('ivo_reference'), rtol=1e-5, atol=1e-4)
    assert torch.allclose(got, tensor('ivo_known'), rtol=1e-4)
    for name, bad in (('ivo_ndim', torch.zeros(2, 2)), ('ivo_dim2', torch.zeros(1, 2, 3, 3)), ('ivo_dim3', torch.zeros(1, 2, 4, 2))):
        with raises_like(name):
            inverse_vertices_offset(bad)


def test_workspace_query():
    ws = _lib.load().kamd_subdivide_tetmesh_workspace
    assert ws(0, 1000) == 0 and ws(1, 0) == 0 and ws(1, 1) > 0 and ws(-1, 5) == 0 and ws(5, 2 ** 32) == 0
    assert ws(12582912, 2146689) > ws(4444, 1000) > ws(1, 4)
    assert ws(4444, 70001) == ws(4444, 1000)                    # the sort skips passes for a small V; the buffers are the same
    assert ws(2 ** 31 // 6 + 1, 2 ** 32 - 1) > 6 * (2 ** 31 // 6 + 1) * 20


def test_public_names():
    kaolin = kal.install_as_kaolin()
    assert kaolin.ops.mesh.subdivide_tetmesh is subdivide_tetmesh
    assert kaolin.ops.mesh.tetmesh.subdivide_tetmesh is subdivide_tetmesh
    assert kaolin.ops.mesh.inverse_vertices_offset is inverse_vertices_offset
    assert 'subdivide_tetmesh' in kaolin.ops.mesh.__all__ and 'inverse_vertices_offset' in kaolin.ops.mesh.__all__
    for name in ('subdivide_tetmesh_cuda', 'tetmesh_midpoints_forward_cuda', 'tetmesh_midpoints_backward_cuda'):
        assert callable(getattr(_C.ops.mesh, name))
