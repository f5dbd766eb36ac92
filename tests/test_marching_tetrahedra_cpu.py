"""kaolin.ops.conversions.marching_tetrahedra without a GPU: the package's torch formulation against every case the reference
recorded (tests/golden/marching_tetrahedra.npz, written by make_golden_marching_tetrahedra.py), the sign-case table rebuilt
from those records, the argument checks, and the host-only parts of the HIP path (index-range helper, workspace queries)."""
import builtins
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
import kaolin_amd as kal
from kaolin_amd import _C, _lib
from kaolin_amd.ops.conversions import marching_tetrahedra, tetmesh
from kaolin_amd.utils.testing import elementwise_mismatch, kuhn_grid

G = np.load(os.path.join(GOLDEN_DIR, 'marching_tetrahedra.npz'))
DTYPES = [('f32', torch.float32), ('f64', torch.float64)]
CASES = ['cases16', 'doc', 'kat', 'zeros_nan', 'grid9', 'sparse_ids']
SPARSE_V = 70001


def tensor(name):
    return torch.from_numpy(G[name])


def case_inputs(case):
    if case != 'sparse_ids':
        return tensor(f'{case}_vertices'), tensor(f'{case}_tets'), tensor(f'{case}_sdf')
    ids = tensor('sparse_ids_map')
    vertices, sdf = torch.zeros(SPARSE_V, 3), torch.full((SPARSE_V,), -1.0)
    vertices[ids], sdf[ids] = tensor('grid9_vertices')[0], tensor('grid9_sdf')[0]
    return vertices[None], tensor('sparse_ids_tets'), sdf[None]


def same(a, b, equal_nan=False):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if equal_nan:
        a, b = torch.nan_to_num(a, nan=12345.), torch.nan_to_num(b, nan=12345.)
    return torch.equal(a, b)


def raises_like(name):
    kind, text = (str(x) for x in G[f'err_{name}'])
    return pytest.raises(getattr(builtins, kind), match=re.escape(text))


@pytest.mark.parametrize('tag,dtype', DTYPES)
@pytest.mark.parametrize('case', CASES)
def test_matches_reference(case, tag, dtype):
    vertices, tets, sdf = case_inputs(case)
    out = marching_tetrahedra(vertices.to(dtype), tets, sdf.to(dtype), True)
    assert isinstance(out, list) and len(out) == 3 and all(len(o) == vertices.shape[0] for o in out)
    for b in range(vertices.shape[0]):
        assert same(out[0][b], tensor(f'{case}_verts_{b}_{tag}'), equal_nan=(case == 'zeros_nan')), (case, b)
        assert same(out[1][b], tensor(f'{case}_faces_{b}')) and same(out[2][b], tensor(f'{case}_tet_idx_{b}')), (case, b)
    two = marching_tetrahedra(vertices.to(dtype), tets, sdf.to(dtype))
    assert len(two) == 2 and all(same(x, y, True) for x, y in zip(two[0], out[0])) and all(same(x, y) for x, y in zip(two[1], out[1]))
    if case == 'zeros_nan':
        assert bool(torch.isnan(out[0][0]).any())


def test_reference_test_expectations():
    """The tensors the reference's own unit test expects (its bound: allclose(atol=1e-4) on the vertices)."""
    vertices, tets, sdf = case_inputs('kat')
    verts, faces, tet_idx = marching_tetrahedra(vertices, tets, sdf, True)
    for b in range(4):
        assert torch.allclose(verts[b], tensor(f'kat_expected_verts_{b}'), atol=1e-4)
        assert torch.equal(faces[b], tensor(f'kat_expected_faces_{b}')) and torch.equal(tet_idx[b], tensor(f'kat_expected_tet_idx_{b}'))


def test_empty_conventions():
    vertices, tets, sdf = case_inputs('grid9')
    for dtype in (torch.float32, torch.float64, torch.half):
        for out in (marching_tetrahedra(vertices.to(dtype), tets, sdf.abs().to(dtype) + 1, True),
                    marching_tetrahedra(vertices.to(dtype), tets[:0], sdf.to(dtype), True)):
            for b in range(2):
                assert out[0][b].shape == (0, 3) and out[0][b].dtype == dtype
                assert out[1][b].shape == (0, 3) and out[1][b].dtype == torch.long
                assert out[2][b].shape == (0,) and out[2][b].dtype == torch.long
    assert marching_tetrahedra(vertices[:0], tets, sdf[:0]) == []
    assert same(tensor('cases16_verts_0_f32'), torch.zeros(0, 3)) and same(tensor('cases16_faces_15'), torch.zeros(0, 3, dtype=torch.long))


def test_other_dtypes():
    """int32 tets, and vertices / sdf of different types (the result takes the promoted type, as the reference's does)."""
    vertices, tets, sdf = case_inputs('grid9')
    verts, faces = marching_tetrahedra(vertices.double(), tets.int(), sdf)
    assert verts[0].dtype == torch.float64 and same(faces[0], tensor('grid9_faces_0'))
    assert same(verts[0], tensor('grid9_verts_0_f64'))       # float32 sdf values widen exactly
    half = marching_tetrahedra(vertices.half(), tets, sdf.half())
    assert half[0][0].dtype == torch.half and half[1][0].dtype == torch.long


def test_case_table_derived_from_records():
    """One tet with ids 0..3: its crossing edges, ascending, are its crossing edge slots in slot order, so the recorded faces
    of sign case c name the slots of the table's row c."""
    for c in range(16):
        occupied = [(c >> k) & 1 for k in range(4)]
        slots = [i for i, (a, b) in enumerate(tetmesh.EDGE_CORNERS) if occupied[a] != occupied[b]]
        assert G[f'cases16_verts_{c}_f64'].shape[0] == len(slots)
        row = [slots[r] for r in G[f'cases16_faces_{c}'].reshape(-1)]
        assert len(row) == 3 * tetmesh.NUM_TRIANGLES[c]
        assert list(tetmesh.TRIANGLE_SLOTS[c][:len(row)]) == row, c
    hip = open(os.path.join(os.path.dirname(GOLDEN_DIR), '..', 'kaolin_amd', 'csrc', 'marching_tetrahedra.hip')).read()
    body = re.search(r'mt_tri\[16\]\[6\] = \{(.*?)\};', hip, flags=re.S).group(1)
    assert [int(x) for x in re.findall(r'\d+', body)] == [s for row in tetmesh.TRIANGLE_SLOTS for s in row]


@pytest.mark.parametrize('tag,dtype', DTYPES)
@pytest.mark.parametrize('case', ['grid9', 'sparse_ids'])
def test_gradients_match_reference(case, tag, dtype):
    vertices, tets, sdf = case_inputs(case)
    p, s = vertices[:1].to(dtype).requires_grad_(), sdf[:1].to(dtype).requires_grad_()
    verts, faces = marching_tetrahedra(p, tets, s)
    assert verts[0].requires_grad and not faces[0].requires_grad
    (verts[0] * tensor(f'grads_{case}_cotangent').to(dtype)).sum().backward()
    grad_p, grad_s = p.grad[0], s.grad[0]
    if case == 'sparse_ids':
        ids = tensor('sparse_ids_map')
        rest = torch.ones(SPARSE_V, dtype=torch.bool)
        rest[ids] = False
        assert not bool(grad_p[rest].any()) and not bool(grad_s[rest].any())
        grad_p, grad_s = grad_p[ids], grad_s[ids]
    for got, name in ((grad_p, 'vertices'), (grad_s, 'sdf')):
        msg = elementwise_mismatch(got, tensor(f'grads_{case}_{name}_{tag}'), tol=1e-5,
                                   term_abs_sum=tensor(f'grads_{case}_{name}_tas'))
        assert msg is None, msg


def test_recorded_errors():
    vertices, _, sdf = case_inputs('grid9')
    vertices, sdf, tets = vertices[:, :8], sdf[:, :8], torch.tensor([[0, 1, 2, 3], [4, 5, 6, 7]])
    with raises_like('sdf_unbatched'):
        marching_tetrahedra(vertices, tets, sdf[0])
    with raises_like('sdf_batch'):
        marching_tetrahedra(vertices, tets, sdf[:1])
    with raises_like('tets_width'):
        marching_tetrahedra(vertices, tets[:, :3], sdf)
    with raises_like('tets_float'):
        marching_tetrahedra(vertices, tets.float(), sdf)


def test_index_range_check():
    check = _C.ops.check_tets_in_range
    tets = torch.tensor([[0, 1, 2, 3], [4, 5, 6, 7]])
    check(tets, 8)
    check(tets[:0], 0)
    with pytest.raises(IndexError, match='outside'):
        check(tets, 7)                                       # an entry equal to V
    low = tets.clone()
    low[1, 2] = -1
    with pytest.raises(IndexError, match='-1'):
        check(low, 8)
    with pytest.raises(RuntimeError):
        check(tets[:, :3], 8)
    with pytest.raises(RuntimeError):
        check(tets.float(), 8)
    vertices, sdf = torch.rand(1, 8, 3), torch.randn(1, 8)
    with pytest.raises(IndexError):
        marching_tetrahedra(vertices[:, :7], tets, sdf[:, :7])
    with pytest.raises(IndexError):
        marching_tetrahedra(vertices, low, sdf)
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        _C.ops.conversions.marching_tetrahedra_cuda(vertices[0], tets, sdf[0])


def test_workspace_queries():
    lib = _lib.load()
    ws = lib.kamd_marching_tetrahedra_workspace
    assert ws(0, 1000) == 0 and ws(4374, 1000) > 0
    assert ws(12582912, 2146689) > ws(303918, 54872) > ws(4374, 1000)
    assert ws(4374, 70001) > ws(4374, 1000)
    assert ws(12582912, 2146689) < 2 * 12582912              # a byte per tet and a bit per vertex, not a key per tet
    edges = lib.kamd_marching_tetrahedra_edges_workspace
    assert edges(0, 0) == 0 and edges(100, 0) > 0 and edges(100, 100) > edges(100, 0) and edges(1000, 1000) > edges(100, 100)


def test_public_names():
    kaolin = kal.install_as_kaolin()
    assert kaolin.ops.conversions.marching_tetrahedra is marching_tetrahedra
    assert kaolin.ops.conversions.tetmesh.marching_tetrahedra is marching_tetrahedra
    assert callable(_C.ops.conversions.marching_tetrahedra_cuda) and callable(_C.ops.conversions.marching_tetrahedra_backward_cuda)
    vertices, tets = kuhn_grid(1)
    assert vertices.shape == (8, 3) and tets.shape == (6, 4) and torch.unique(tets.sort(dim=1).values, dim=0).shape[0] == 6
