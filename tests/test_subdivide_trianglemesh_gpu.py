"""kaolin.ops.mesh.subdivide_trianglemesh on the GPU: the HIP pipeline (csrc/subdivide_trianglemesh.hip) against the reference's
recorded answers (tests/golden/subdivide_trianglemesh.npz, written by make_golden_subdivide_trianglemesh.py) in float32 and, in
float64 and at shapes no golden holds, against the package's torch formulation on the CPU (which
test_subdivide_trianglemesh_cpu.py pins to the same records)."""
import pytest
import torch

from kaolin_amd.ops.mesh import subdivide_trianglemesh, trianglemesh
from kaolin_amd.utils.testing import elementwise_mismatch
from subdivide_trianglemesh_golden import (FORWARD_CASES, GRAD_CASES, SETTINGS, case_inputs, check_forward, check_gradients,
                                           expected_faces, tensor)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TORCH_ITERATION = trianglemesh._torch_iteration     # (the autouse fixture hides the module attribute)


def _refuse(*args):
    raise AssertionError('a float32 / float64 GPU call reached the torch formulation')


@pytest.fixture(autouse=True)
def hip_path_only(monkeypatch):
    """A float32 / float64 GPU call that reached the torch formulation would pass these tests without running a kernel."""
    monkeypatch.setattr(trianglemesh, '_torch_iteration', _refuse)


_CPU64 = {}


def cpu_float64(case, iterations, setting):
    """The torch formulation in float64 on the CPU (computed once per case; do not modify)"""
    key = (case, iterations, setting)
    if key not in _CPU64:
        vertices, faces, alpha = case_inputs(case)
        for _ in range(iterations):
            vertices, faces, alpha = TORCH_ITERATION(vertices.double(), faces, alpha.double() if setting == 'alpha' else None)
        _CPU64[key] = (vertices, faces)
    return _CPU64[key]


@pytest.mark.parametrize('setting', SETTINGS)
@pytest.mark.parametrize('case,iterations', FORWARD_CASES)
def test_matches_reference(case, iterations, setting):
    vertices, faces, alpha = case_inputs(case)
    new_vertices, new_faces = subdivide_trianglemesh(vertices.to(DEV), faces.to(DEV), iterations,
                                                     alpha.to(DEV) if setting == 'alpha' else None)
    assert new_vertices.dtype == torch.float32 and new_vertices.device == new_faces.device == torch.device(DEV)
    check_forward(case, iterations, setting, new_vertices, new_faces, verbose=True)


@pytest.mark.parametrize('setting', SETTINGS)
@pytest.mark.parametrize('case,iterations', FORWARD_CASES)
def test_float64_matches_torch_formulation(case, iterations, setting):
    vertices, faces, alpha = case_inputs(case)
    want_vertices, want_faces = cpu_float64(case, iterations, setting)
    new_vertices, new_faces = subdivide_trianglemesh(vertices.to(DEV).double(), faces.to(DEV), iterations,
                                                     alpha.to(DEV).double() if setting == 'alpha' else None)
    assert new_vertices.dtype == torch.float64 and torch.equal(new_faces.cpu(), want_faces)
    assert torch.equal(want_faces, expected_faces(case, iterations))
    msg = elementwise_mismatch(new_vertices.cpu(), want_vertices, tol=1e-12)
    assert msg is None, msg
    if case == 'sparse_ids':                                      # the rows nobody uses: the inputs, bit for bit
        used = torch.zeros(vertices.shape[1], dtype=torch.bool)
        used[faces.reshape(-1)] = True
        assert torch.equal(new_vertices.cpu()[0, :vertices.shape[1]][~used], vertices.double()[0, ~used])


def test_forward_is_bit_reproducible():
    vertices, faces, alpha = (t.to(DEV) for t in case_inputs('open_messy'))
    first = subdivide_trianglemesh(vertices, faces, 2, alpha)
    second = subdivide_trianglemesh(vertices, faces, 2, alpha)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])
    first, second = subdivide_trianglemesh(vertices, faces, 2), subdivide_trianglemesh(vertices, faces, 2)
    assert torch.equal(first[0], second[0])


@pytest.mark.parametrize('case', GRAD_CASES)
def test_gradients_match_reference(case):
    vertices, faces, alpha = case_inputs(case)
    p, a = vertices.to(DEV).requires_grad_(), alpha.to(DEV).requires_grad_()
    new_vertices, new_faces = subdivide_trianglemesh(p, faces.to(DEV), 2, a)
    assert new_vertices.requires_grad and not new_faces.requires_grad
    (new_vertices * tensor(f'grads_{case}_cot').to(DEV)).sum().backward()
    check_gradients(case, p.grad, a.grad, verbose=True)


def test_gradient_of_vertices_alone():
    """alpha given but constant, and no alpha: only `vertices` gets a gradient.  float64 against the torch formulation on the CPU:
    both sum a few dozen terms of magnitude <= 1 per element, so they differ by some 1e-15, far inside 1e-12 of the typical
    magnitude."""
    vertices, faces, alpha = case_inputs('open_messy')
    vertices, alpha, cot = vertices.double(), alpha.double(), tensor('grads_open_messy_cot').double()
    for a in (alpha, None):
        q = vertices.clone().requires_grad_()
        x, f, al = q, faces, a
        for _ in range(2):
            x, f, al = TORCH_ITERATION(x, f, al)
        (x * cot).sum().backward()
        p = vertices.to(DEV).requires_grad_()
        (subdivide_trianglemesh(p, faces.to(DEV), 2, None if a is None else a.to(DEV))[0] * cot.to(DEV)).sum().backward()
        msg = elementwise_mismatch(p.grad.cpu(), q.grad, tol=1e-12)
        assert msg is None, msg


STRIP = torch.tensor([[0, 1, 2], [2, 1, 3]])      # two triangles: one interior edge, four boundary edges


@pytest.mark.parametrize('mesh', ['doc', 'strip'])
def test_gradcheck(mesh):
    g = torch.Generator().manual_seed(11)
    faces = (case_inputs('doc')[1] if mesh == 'doc' else STRIP).to(DEV)
    p = torch.rand(1, 4, 3, generator=g, dtype=torch.double).to(DEV).requires_grad_()
    a = torch.rand(1, 4, generator=g, dtype=torch.double).to(DEV).requires_grad_()
    assert torch.autograd.gradcheck(lambda x, y: subdivide_trianglemesh(x, faces, 2, y)[0], (p, a), nondet_tol=1e-12)
    assert torch.autograd.gradcheck(lambda x: subdivide_trianglemesh(x, faces, 2)[0], (p,), nondet_tol=1e-12)


def test_batch_views():
    """An expanded (stride-0) batch and a `vertices` view that is not contiguous"""
    vertices, faces, alpha = (t.to(DEV) for t in case_inputs('sphere6'))
    want, want_faces = subdivide_trianglemesh(vertices[1:], faces, 2, alpha[1:])
    expanded, expanded_alpha = vertices[1:].expand(3, -1, -1), alpha[1:].expand(3, -1)
    assert expanded.stride(0) == 0
    got, got_faces = subdivide_trianglemesh(expanded, faces, 2, expanded_alpha)
    assert torch.equal(got_faces, want_faces) and all(torch.equal(got[b], want[0]) for b in range(3))
    wide = torch.zeros(2, 362, 5, device=DEV)
    wide[..., 1:4] = vertices
    view = wide[..., 1:4]
    assert not view.is_contiguous()
    both = subdivide_trianglemesh(view, faces, 2, alpha)[0]
    assert torch.equal(both[1], want[0])
    assert torch.equal(both, subdivide_trianglemesh(vertices, faces, 2, alpha)[0])
    shifted = torch.zeros(faces.numel() + 1, dtype=torch.long, device=DEV)[1:].view(-1, 3)     # storage 8 bytes off 16
    shifted.copy_(faces)
    assert torch.equal(subdivide_trianglemesh(vertices[1:], shifted, 2, alpha[1:])[0], want)


def test_current_stream_is_honoured():
    vertices, faces, alpha = (t.to(DEV) for t in case_inputs('sphere6'))
    want = subdivide_trianglemesh(vertices, faces, 2, alpha)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        # the inputs are produced on the side stream right before the call: a kernel on another stream would not wait for them
        v, a = vertices * 1.0, alpha * 1.0
        got = subdivide_trianglemesh(v, faces, 2, a)
    stream.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_half_takes_the_torch_path(monkeypatch):
    monkeypatch.undo()
    vertices, faces, alpha = case_inputs('sphere6')
    calls = []
    monkeypatch.setattr(trianglemesh, '_torch_iteration', lambda *a: calls.append(1) or TORCH_ITERATION(*a))
    out = subdivide_trianglemesh(vertices.to(DEV).half(), faces.to(DEV), 1, alpha.to(DEV).half())
    assert len(calls) == 1 and out[0].dtype == torch.half and out[0].device == torch.device(DEV)
    assert torch.equal(out[1].cpu(), expected_faces('sphere6', 1))


def test_index_out_of_range_raises_before_any_launch():
    vertices, faces, alpha = (t.to(DEV) for t in case_inputs('doc'))
    with pytest.raises(IndexError, match='outside'):
        subdivide_trianglemesh(vertices[:, :3], faces, 1)
    bad = faces.clone()
    bad[2, 1] = -1
    with pytest.raises(IndexError, match='-1'):
        subdivide_trianglemesh(vertices, bad, 1, alpha)
    from kaolin_amd import _C
    with pytest.raises(IndexError, match='outside'):
        _C.ops.mesh.subdivide_trianglemesh_cuda(faces, 3)
