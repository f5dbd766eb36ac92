"""kaolin.ops.conversions.marching_tetrahedra on the GPU: the HIP pipeline (csrc/marching_tetrahedra.hip) against the
reference's recorded answers (tests/golden/marching_tetrahedra.npz, written by make_golden_marching_tetrahedra.py) and, at a
size no golden holds, against the package's torch formulation on the CPU (which test_marching_tetrahedra_cpu.py pins to the
same records).  Integer results and vertices are compared with torch.equal: both sides evaluate the same four correctly
rounded operations per coordinate.  No test here passes an out-of-range index (the CPU file covers that check)."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from kaolin_amd.ops.conversions import marching_tetrahedra, tetmesh
from kaolin_amd.utils.testing import elementwise_mismatch, kuhn_grid

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = np.load(os.path.join(GOLDEN_DIR, 'marching_tetrahedra.npz'))
DTYPES = [('f32', torch.float32), ('f64', torch.float64)]
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


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=12345.), torch.nan_to_num(b, nan=12345.))


@pytest.fixture(autouse=True)
def hip_path_only(monkeypatch):
    """A float32 / float64 GPU call that reached the torch formulation would pass these tests without running a kernel."""
    monkeypatch.setattr(tetmesh, '_torch_unbatched', None)


@pytest.mark.parametrize('tag,dtype', DTYPES)
@pytest.mark.parametrize('case', ['cases16', 'doc', 'kat', 'zeros_nan', 'grid9', 'sparse_ids'])
def test_matches_reference(case, tag, dtype):
    vertices, tets, sdf = case_inputs(case)
    out = marching_tetrahedra(vertices.to(DEV, dtype), tets.to(DEV), sdf.to(DEV, dtype), True)
    assert isinstance(out, list) and len(out) == 3 and all(len(o) == vertices.shape[0] for o in out)
    assert len(marching_tetrahedra(vertices.to(DEV, dtype), tets.to(DEV), sdf.to(DEV, dtype))) == 2
    for b in range(vertices.shape[0]):
        verts, faces, tet_idx = out[0][b], out[1][b], out[2][b]
        assert verts.device == faces.device == tet_idx.device == torch.device(DEV)
        assert same(verts.cpu(), tensor(f'{case}_verts_{b}_{tag}')), (case, b)      # (NaN where the reference has NaN)
        assert same(faces.cpu(), tensor(f'{case}_faces_{b}')), (case, b)
        assert same(tet_idx.cpu(), tensor(f'{case}_tet_idx_{b}')), (case, b)
    if case == 'zeros_nan':
        assert bool(torch.isnan(out[0][0]).any())


@pytest.mark.parametrize('tag,dtype', DTYPES)
@pytest.mark.parametrize('case', ['grid9', 'sparse_ids'])
def test_gradients_match_reference(case, tag, dtype):
    vertices, tets, sdf = case_inputs(case)
    p = vertices[:1].to(DEV, dtype).requires_grad_()
    s = sdf[:1].to(DEV, dtype).requires_grad_()
    verts, faces = marching_tetrahedra(p, tets.to(DEV), s)
    assert verts[0].requires_grad and not faces[0].requires_grad
    (verts[0] * tensor(f'grads_{case}_cotangent').to(DEV, dtype)).sum().backward()
    grad_p, grad_s = p.grad[0].cpu(), s.grad[0].cpu()
    if case == 'sparse_ids':
        ids = tensor('sparse_ids_map')
        rest = torch.ones(SPARSE_V, dtype=torch.bool)
        rest[ids] = False
        assert not bool(grad_p[rest].any()) and not bool(grad_s[rest].any())
        grad_p, grad_s = grad_p[ids], grad_s[ids]
    for got, name in ((grad_p, 'vertices'), (grad_s, 'sdf')):
        msg = elementwise_mismatch(got, tensor(f'grads_{case}_{name}_{tag}'), tol=1e-5,
                                   term_abs_sum=tensor(f'grads_{case}_{name}_tas'))
        print(case, tag, name, 'slack use', elementwise_mismatch.last_slack_use, msg)
        assert msg is None, msg


def test_gradcheck():
    vertices, tets = kuhn_grid(2, dtype=torch.double)
    g = torch.Generator().manual_seed(3)
    vertices = (vertices + (torch.rand(vertices.shape, generator=g, dtype=torch.double) - 0.5) * 0.1)
    sdf = 0.5 - (vertices - torch.tensor([0.4, 0.55, 0.45], dtype=torch.double)).norm(dim=-1)
    assert tets.shape == (48, 4) and float(sdf.abs().min()) > 1e-2
    p, s, t = vertices[None].to(DEV).requires_grad_(), sdf[None].to(DEV).requires_grad_(), tets.to(DEV)
    assert marching_tetrahedra(p, t, s)[0][0].shape[0] > 8
    assert torch.autograd.gradcheck(lambda a, b: marching_tetrahedra(a, t, b)[0][0], (p, s), nondet_tol=1e-12)


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_non_contiguous_inputs(tag, dtype):
    vertices, tets, sdf = case_inputs('grid9')
    wide_v = torch.randn(2, 1000, 7, dtype=dtype, device=DEV)
    wide_v[:, :, 2:5] = vertices.to(DEV, dtype)
    wide_s = torch.randn(2, 1000, 3, dtype=dtype, device=DEV)
    wide_s[:, :, 1] = sdf.to(DEV, dtype)
    wide_t = torch.zeros(tets.shape[0], 6, dtype=torch.long, device=DEV)
    wide_t[:, 1:5] = tets.to(DEV)
    p, s, t = wide_v[:, :, 2:5], wide_s[:, :, 1], wide_t[:, 1:5]
    assert not p.is_contiguous() and not s.is_contiguous() and not t.is_contiguous()
    verts, faces, tet_idx = marching_tetrahedra(p, t, s, True)
    for b in range(2):
        assert same(verts[b].cpu(), tensor(f'grid9_verts_{b}_{tag}'))
        assert same(faces[b].cpu(), tensor(f'grid9_faces_{b}')) and same(tet_idx[b].cpu(), tensor(f'grid9_tet_idx_{b}'))


def test_grid37_matches_torch_formulation(monkeypatch):
    """303 918 tets: 297 chunks of 1 024 for the count scan, and more crossing-edge instances than one block of the key scan
    and of the radix sort hold."""
    vertices, tets = kuhn_grid(37)
    assert tets.shape == (303918, 4)
    sdf = 0.37 - (vertices - torch.tensor([0.48, 0.53, 0.5])).norm(dim=-1)
    monkeypatch.undo()                                           # the CPU side of this test IS the torch formulation
    ref_verts, ref_faces, ref_idx = marching_tetrahedra(vertices[None], tets, sdf[None], True)
    monkeypatch.setattr(tetmesh, '_torch_unbatched', None)
    verts, faces, tet_idx = marching_tetrahedra(vertices[None].to(DEV), tets.to(DEV), sdf[None].to(DEV), True)
    assert ref_verts[0].shape[0] > 2048 * 4
    assert same(verts[0].cpu(), ref_verts[0]) and same(faces[0].cpu(), ref_faces[0]) and same(tet_idx[0].cpu(), ref_idx[0])
    assert int(faces[0].max()) == verts[0].shape[0] - 1
    occupied = (sdf > 0)[tets].sum(-1)
    assert bool(((occupied > 0) & (occupied < 4))[tet_idx[0].cpu()].all())


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_empty_results(tag, dtype):
    vertices, tets, sdf = case_inputs('grid9')
    p, s, t = vertices[:1].to(DEV, dtype), sdf[:1].to(DEV, dtype), tets.to(DEV)
    for out in (marching_tetrahedra(p, t[:0], s, True), marching_tetrahedra(p, t, -s.abs() - 1, True)):
        verts, faces, tet_idx = out[0][0], out[1][0], out[2][0]
        assert verts.shape == (0, 3) and verts.dtype == dtype and verts.device == torch.device(DEV)
        assert faces.shape == (0, 3) and faces.dtype == torch.long and tet_idx.shape == (0,) and tet_idx.dtype == torch.long
    assert marching_tetrahedra(p[:0], t, s[:0]) == []
    q = p.clone().requires_grad_()
    marching_tetrahedra(q, t, -s.abs() - 1)[0][0].sum().backward()
    assert q.grad.shape == q.shape and not bool(q.grad.any())


def test_half_takes_the_torch_path(monkeypatch):
    monkeypatch.undo()
    vertices, tets, sdf = case_inputs('grid9')
    calls = []
    inner = tetmesh._torch_unbatched
    monkeypatch.setattr(tetmesh, '_torch_unbatched', lambda *a: calls.append(1) or inner(*a))
    verts, faces = marching_tetrahedra(vertices.to(DEV).half(), tets.to(DEV), sdf.to(DEV).half())
    assert len(calls) == 2 and verts[0].dtype == torch.half and verts[0].device == torch.device(DEV)
    cpu_verts, cpu_faces = marching_tetrahedra(vertices.half(), tets, sdf.half())
    assert same(faces[0].cpu(), cpu_faces[0]) and same(faces[1].cpu(), cpu_faces[1])
    assert verts[0].shape == cpu_verts[0].shape
