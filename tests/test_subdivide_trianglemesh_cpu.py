"""kaolin.ops.mesh.subdivide_trianglemesh without a GPU: the package's torch formulation against every case the reference recorded
(tests/golden/subdivide_trianglemesh.npz, written by make_golden_subdivide_trianglemesh.py), the rules the reference does not
have (batches, float64, unused vertices), the argument checks and the host-only parts of the HIP path."""
import builtins
import re

import pytest
import torch

import kaolin_amd as kal
from kaolin_amd import _C, _lib
from kaolin_amd.ops.mesh import subdivide_trianglemesh, trianglemesh
from subdivide_trianglemesh_golden import (FORWARD_CASES, G, GRAD_CASES, SETTINGS, case_inputs, check_forward, check_gradients,
                                           child_faces, tensor)


def raises_like(name):
    kind, text = (str(x) for x in G[f'err_{name}'])
    return pytest.raises(getattr(builtins, kind), match=re.escape(text))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('setting', SETTINGS)
@pytest.mark.parametrize('case,iterations', FORWARD_CASES)
def test_matches_reference(case, iterations, setting, dtype):
    """float32, and float64 against the same float32 records at the same bound"""
    vertices, faces, alpha = case_inputs(case)
    new_vertices, new_faces = subdivide_trianglemesh(vertices.to(dtype), faces, iterations,
                                                     alpha.to(dtype) if setting == 'alpha' else None)
    assert new_vertices.dtype == dtype
    check_forward(case, iterations, setting, new_vertices, new_faces)


def test_reference_test_expectations():
    """The tensors the reference's own unit test expects, at its bound (atol = 1e-4)"""
    vertices, faces, _ = case_inputs('ico')
    for alpha, name in ((None, 'default'), (torch.zeros(1, 12), 'zero')):
        new_vertices, new_faces = subdivide_trianglemesh(vertices, faces, 1, alpha)
        assert torch.allclose(new_vertices, tensor(f'ico_expected_{name}_vertices'), rtol=1e-5, atol=1e-4)
        assert torch.equal(new_faces, tensor('ico_expected_faces'))


def test_child_table_matches_rows():
    """The module's CHILD_FACES against the four rows spelled out next to the goldens."""
    faces = torch.tensor([[0, 1, 2], [2, 1, 3]])
    slots = torch.arange(6).reshape(2, 3) + 10
    columns = torch.cat([faces, slots], dim=1)
    assert torch.equal(columns[:, torch.tensor(trianglemesh.CHILD_FACES)].reshape(-1, 3), child_faces(faces, slots))


@pytest.mark.parametrize('setting', SETTINGS)
def test_batch_equals_items(setting):
    vertices, faces, alpha = case_inputs('sphere6')
    a = alpha if setting == 'alpha' else None
    both, both_faces = subdivide_trianglemesh(vertices, faces, 2, a)
    for b in range(2):
        one, one_faces = subdivide_trianglemesh(vertices[b:b + 1], faces, 2, None if a is None else a[b:b + 1])
        assert torch.equal(both[b:b + 1], one) and torch.equal(both_faces, one_faces)


def test_alpha_with_a_trailing_dimension():
    vertices, faces, alpha = case_inputs('sphere6')
    want = subdivide_trianglemesh(vertices, faces, 2, alpha)
    got = subdivide_trianglemesh(vertices, faces, 2, alpha.unsqueeze(-1))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert [str(o.dtype) for o in got] == [str(x) for x in G['dtypes_alpha3']]


def test_no_iterations_and_no_faces():
    vertices, faces, alpha = case_inputs('sphere6')
    out = subdivide_trianglemesh(vertices, faces, 0, alpha)
    assert out[0] is vertices and out[1] is faces
    for a in (None, alpha):
        new_vertices, new_faces = subdivide_trianglemesh(vertices, faces[:0], 2, a)
        assert torch.equal(new_vertices, vertices) and new_faces.shape == (0, 3) and new_faces.dtype == torch.long


@pytest.mark.parametrize('setting', SETTINGS)
def test_unused_vertices_pass_through(setting):
    """Three vertices nobody uses among the doc tetrahedron's: position and alpha kept, over two iterations; the used ones move
    as without them.  (The reference returns NaN for the unused rows.)"""
    vertices, faces, _ = case_inputs('doc')
    g = torch.Generator().manual_seed(3)
    alpha = torch.rand(1, 4, generator=g)
    keep = torch.tensor([1, 3, 4, 6])
    wide, wide_alpha = torch.rand(1, 7, 3, generator=g), torch.rand(1, 7, generator=g)
    wide[0, keep], wide_alpha[0, keep] = vertices[0], alpha[0]
    a, wa = (alpha, wide_alpha) if setting == 'alpha' else (None, None)
    want, want_faces = subdivide_trianglemesh(vertices, faces, 2, a)
    p, q = wide.clone().requires_grad_(), (wa.clone().requires_grad_() if wa is not None else None)
    got, got_faces = subdivide_trianglemesh(p, keep[faces], 2, q)
    rest = torch.tensor([0, 2, 5])
    assert torch.equal(got[0, rest], wide[0, rest]) and not bool(torch.isnan(got).any())
    assert torch.equal(got[0, keep], want[0, :4]) and torch.equal(got[0, 7:], want[0, 4:])
    assert got_faces.shape == want_faces.shape
    got.sum().backward()
    assert torch.equal(p.grad[0, rest], torch.ones(3, 3)) and not bool(torch.isnan(p.grad).any())
    if q is not None:
        assert torch.equal(q.grad[0, rest], torch.zeros(3)) and not bool(torch.isnan(q.grad).any())


@pytest.mark.parametrize('case', GRAD_CASES)
def test_gradients_match_reference(case):
    vertices, faces, alpha = case_inputs(case)
    p, a = vertices.clone().requires_grad_(), alpha.clone().requires_grad_()
    new_vertices, new_faces = subdivide_trianglemesh(p, faces, 2, a)
    assert new_vertices.requires_grad and not new_faces.requires_grad
    (new_vertices * tensor(f'grads_{case}_cot')).sum().backward()
    check_gradients(case, p.grad, a.grad)


@pytest.mark.parametrize('case', GRAD_CASES)
def test_term_magnitudes_bound_the_gradient(case):
    vertices, faces, alpha = case_inputs(case)
    p, a = vertices.double().requires_grad_(), alpha.double().requires_grad_()
    (subdivide_trianglemesh(p, faces, 2, a)[0] * tensor(f'grads_{case}_cot').double()).sum().backward()
    assert bool((tensor(f'grads_{case}_vertices_tas') + 1e-300 >= p.grad.abs() * (1 - 1e-9)).all())
    assert bool((tensor(f'grads_{case}_alpha_tas') + 1e-300 >= a.grad.abs() * (1 - 1e-9)).all())


def test_gradcheck():
    vertices, faces, _ = case_inputs('doc')
    g = torch.Generator().manual_seed(11)
    p = (vertices.double() + torch.rand(1, 4, 3, generator=g, dtype=torch.double) * 0.1).requires_grad_()
    a = torch.rand(1, 4, generator=g, dtype=torch.double).requires_grad_()
    assert torch.autograd.gradcheck(lambda x, y: subdivide_trianglemesh(x, faces, 2, y)[0], (p, a))
    assert torch.autograd.gradcheck(lambda x: subdivide_trianglemesh(x, faces, 2)[0], (p,))


def test_other_dtypes():
    """What the reference rejects and this takes: half, float64, a batch, int32 faces, mixed dtypes"""
    vertices, faces, alpha = case_inputs('sphere6')
    for name in ('double', 'half', 'batch2', 'int32_faces'):
        assert str(G[f'err_{name}'][0]) == 'RuntimeError'                       # (the reference's limits, as recorded)
    want = subdivide_trianglemesh(vertices, faces, 1, alpha)
    half = subdivide_trianglemesh(vertices.half(), faces, 1, alpha.half())
    assert half[0].dtype == torch.half and torch.equal(half[1], want[1])
    assert torch.allclose(half[0].float(), want[0], atol=4e-3)
    ints = subdivide_trianglemesh(vertices, faces.int(), 1, alpha)
    assert ints[1].dtype == torch.long and torch.equal(ints[0], want[0]) and torch.equal(ints[1], want[1])
    mixed = subdivide_trianglemesh(vertices, faces, 1, alpha.double())
    assert mixed[0].dtype == torch.double
    assert torch.equal(mixed[0], subdivide_trianglemesh(vertices.double(), faces, 1, alpha.double())[0])


def test_argument_errors():
    vertices, faces, alpha = case_inputs('doc')
    with raises_like('faces_1d'):
        subdivide_trianglemesh(vertices, faces.reshape(-1), 1, alpha)
    with raises_like('faces_float'):
        subdivide_trianglemesh(vertices, faces.float(), 1, alpha)
    with raises_like('iterations_float'):
        subdivide_trianglemesh(vertices, faces, 1.0, alpha)
    with pytest.raises(RuntimeError, match='faces must of size'):
        subdivide_trianglemesh(vertices, torch.tensor([[0, 1, 2, 3]]), 1)
    with pytest.raises(RuntimeError, match='alpha must of size'):
        subdivide_trianglemesh(vertices, faces, 1, alpha[:, :3])
    with pytest.raises(RuntimeError, match='alpha must of size'):
        subdivide_trianglemesh(vertices, faces, 1, alpha.expand(2, -1))
    with pytest.raises(RuntimeError, match='vertices must of size'):
        subdivide_trianglemesh(vertices[0], faces, 1)


def test_index_range_check():
    vertices, faces, alpha = case_inputs('doc')
    with pytest.raises(IndexError, match='outside'):
        subdivide_trianglemesh(vertices[:, :3], faces, 1)                     # an entry equal to V
    low = faces.clone()
    low[1, 2] = -1
    with pytest.raises(IndexError, match='-1'):
        subdivide_trianglemesh(vertices, low, 1, alpha)
    with pytest.raises(IndexError, match='outside'):
        _C.ops.mesh.subdivide_trianglemesh_cuda(faces, 3)                      # the range check comes before every other
    with pytest.raises(RuntimeError, match='CUDA tensor'):
        _C.ops.mesh.subdivide_trianglemesh_cuda(faces, 4)


def test_workspace_query():
    ws = _lib.load().kamd_subdivide_trianglemesh_workspace
    assert ws(0, 1000) == 0 and ws(1, 0) == 0 and ws(1, 1) > 0 and ws(-1, 5) == 0 and ws(5, 2 ** 32) == 0
    assert ws(327680, 163842) > ws(720, 362) > ws(1, 3)
    assert ws(720, 70001) == ws(720, 362)                       # the sort skips passes for a small V; the buffers are the same
    assert ws(2 ** 31 // 3 + 1, 2 ** 32 - 1) > 3 * (2 ** 31 // 3 + 1) * 28


def test_public_names():
    kaolin = kal.install_as_kaolin()
    assert kaolin.ops.mesh.subdivide_trianglemesh is subdivide_trianglemesh
    assert kaolin.ops.mesh.trianglemesh.subdivide_trianglemesh is subdivide_trianglemesh
    assert 'subdivide_trianglemesh' in kaolin.ops.mesh.__all__
    for name in ('subdivide_trianglemesh_cuda', 'trianglemesh_loop_forward_cuda', 'trianglemesh_loop_backward_cuda'):
        assert callable(getattr(_C.ops.mesh, name))
