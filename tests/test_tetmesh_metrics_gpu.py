"""kaolin.metrics.tetmesh on the GPU: the fused kernels of csrc/tetmesh_metrics.hip against the reference's recorded float64
answers (tests/golden/tetmesh_metrics.npz, written by make_golden_tetmesh_metrics.py) and, at shapes no record holds, against the
package's torch formulations in float64 on the CPU (which test_tetmesh_metrics_cpu.py pins to the same records).  Tolerances
(tests/tetmesh_metrics_golden.py): per element elementwise_mismatch(tol = 1e-5 float32 / 2e-14 float64) with the sums of term
magnitudes; losses |hip - ref64| <= max(4 |ref32 - ref64|, 64 eps sum|terms| / T).  No test passes non-finite inputs."""
import contextlib

import pytest
import torch

from kaolin_amd.metrics import tetmesh
from kaolin_amd.metrics.tetmesh import amips, equivolume, tetrahedron_volume
from kaolin_amd.ops.mesh import inverse_vertices_offset
from kaolin_amd.utils.testing import kuhn_grid
from tetmesh_metrics_golden import (DTYPES, amips_grad_terms, check_elements, check_scalars, equivolume_grad_terms, jittered_grid,
                                    known_answers, records_amips, records_equivolume, records_volume, volume_grad_terms,
                                    volume_terms)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FORMULATIONS = {n: getattr(tetmesh, n) for n in ('_torch_volume', '_torch_equivolume', '_torch_amips')}


@pytest.fixture(autouse=True)
def hip_path_only(monkeypatch):
    """A float32 / float64 GPU call that reached a torch formulation would pass these tests without running a kernel."""
    for name in FORMULATIONS:
        monkeypatch.setattr(tetmesh, name, None)


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_known_answers(tag, dtype, monkeypatch):
    monkeypatch.undo()      # (the docstring's equivolume example is B == T == 2 with the mean computed: the torch formulation's)
    known_answers(DEV, tag, dtype)


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_volume_records(tag, dtype):
    records_volume(DEV, tag, dtype)


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_equivolume_records(tag, dtype):
    records_equivolume(DEV, tag, dtype)


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_amips_records(tag, dtype):
    records_amips(DEV, tag, dtype)


def _case(n, batch, dtype, num_tets=None, seed=3):
    """-> tet_vertices (batch, T, 4, 3) of the jittered kuhn_grid(n) (its first `num_tets` tets) and the inverse offset matrices
    (1, T, 3, 3) of the rest shape, on the CPU; every 5th tet has corners 2 and 3 swapped (negative volume, det < 0)"""
    vertices, tets = jittered_grid(n, batch, dtype, seed)
    rest = kuhn_grid(n, dtype=dtype)[0][None]
    tets = tets[:num_tets]
    swapped = tets.clone()
    swapped[1::5, 2], swapped[1::5, 3] = tets[1::5, 3], tets[1::5, 2]
    return vertices[:, swapped].contiguous(), inverse_vertices_offset(rest[:, tets]).contiguous()


@contextlib.contextmanager
def _formulations():
    """The torch formulations back in place (they call each other through the module) while the CPU side of a test runs"""
    hidden = {n: getattr(tetmesh, n) for n in FORMULATIONS}
    for n, f in FORMULATIONS.items():
        setattr(tetmesh, n, f)
    try:
        yield
    finally:
        for n, f in hidden.items():
            setattr(tetmesh, n, f)


def _reference(tv, inv, mean, power):
    """float64 on the CPU through the torch formulations: volumes, both losses and every gradient (cotangents: ones)"""
    x, m, mu = (t.detach().double().requires_grad_() for t in (tv, inv, mean))
    with _formulations():
        volumes = FORMULATIONS['_torch_volume'](x)
        equi = FORMULATIONS['_torch_equivolume'](x, mu, power)
        am = FORMULATIONS['_torch_amips'](x, m)
    gv, = torch.autograd.grad(volumes.sum(), x)
    ge, gmu = torch.autograd.grad(equi.sum(), (x, mu))
    ga, gm = torch.autograd.grad(am.sum(), (x, m))
    return volumes.detach(), equi.detach(), am.detach(), gv, ge, gmu, ga, gm


def _compare(name, tv, inv, tag, dtype, power=2, mean=1e-4, make_inputs=None):
    """All three operators, forward and backward, at tv / inv (CPU, `dtype`) against the float64 formulation.  `make_inputs`
    turns the contiguous device copies into the views under test."""
    mean = torch.tensor([mean], dtype=dtype)
    want = _reference(tv, inv, mean, power)
    x, m, mu = tv.to(DEV), inv.to(DEV), mean.to(DEV)
    if make_inputs is not None:
        x, m = make_inputs(x, m)
    x, m, mu = x.detach().requires_grad_(), m.detach().requires_grad_(), mu.requires_grad_()
    volumes, equi, am = tetrahedron_volume(x), equivolume(x, mu, pow=power), amips(x, m)
    gv, = torch.autograd.grad(volumes.sum(), x)
    ge, gmu = torch.autograd.grad(equi.sum(), (x, mu))
    ga, gm = torch.autograd.grad(am.sum(), (x, m))
    B, T = tv.shape[:2]
    ones = torch.ones(B, T)
    eterms, mterms = equivolume_grad_terms(tv, mean, power, False)
    aterms, iterms = amips_grad_terms(tv, inv)
    check_elements(f'{name}_volume', volumes, tag, want[0], volume_terms(tv))
    check_elements(f'{name}_volume_grad', gv, tag, want[3], volume_grad_terms(tv, ones))
    check_elements(f'{name}_equi_grad', ge, tag, want[4], eterms)
    check_elements(f'{name}_equi_grad_mean', gmu, tag, want[5], mterms.reshape(1))
    check_elements(f'{name}_amips_grad', ga, tag, want[6], aterms)
    check_elements(f'{name}_amips_grad_inv', gm, tag, want[7], iterms.sum(0, keepdim=True) if inv.shape[0] != B else iterms)
    # losses: the float32 formulation's own deviation from float64 stands in for the recorded ref32_dev
    with _formulations():
        dev32 = [FORMULATIONS[f](tv.float(), *a).double() - w for f, a, w in
                 (('_torch_equivolume', (mean.float(), power), want[1]), ('_torch_amips', (inv.float(),), want[2]))]
    check_scalars(f'{name}_equi', equi, tag, want[1], dev32[0], want[1])
    check_scalars(f'{name}_amips', am, tag, want[2], dev32[1], want[2])
    return x, m


@pytest.mark.parametrize('tag,dtype', DTYPES)
@pytest.mark.parametrize('num_tets', [1, 63, 64, 65, 255, 256, 257])
def test_small_shapes(num_tets, tag, dtype):
    tv, inv = _case(4, 2, dtype, num_tets)
    assert tv.shape == (2, num_tets, 4, 3)
    _compare(f'T{num_tets}', tv, inv, tag, dtype)


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_grid16_three_items(tag, dtype):
    """24 576 tets: 96 partials per batch item in the reductions; B = 3 against one item of inverse matrices; pow = 3"""
    tv, inv = _case(16, 3, dtype)
    assert tv.shape == (3, 24576, 4, 3) and inv.shape[0] == 1
    _compare('grid16', tv, inv, tag, dtype, power=3)
    _compare('grid16_own_inverse', tv, inv.expand(3, -1, -1, -1).contiguous(), tag, dtype, power=1, mean=0.0)


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_views(tag, dtype):
    tv, inv = _case(3, 2, dtype)

    def expanded(x, m):
        x = x[:1].expand(2, -1, -1, -1)
        assert x.stride(0) == 0
        return x, m
    _compare('expanded', tv[:1].expand(2, -1, -1, -1), inv, tag, dtype, make_inputs=expanded)

    def offset(x, m):
        """storage offsets that leave the data only element-aligned: the scalar-load variant"""
        views = []
        for t in (x, m):
            flat = torch.zeros(t.numel() + 1, dtype=t.dtype, device=DEV)
            flat[1:] = t.reshape(-1)
            views.append(flat[1:].view(t.shape))
        assert views[0].data_ptr() % 16 != 0 and views[0].is_contiguous()
        return views
    _compare('offset', tv, inv, tag, dtype, make_inputs=offset)

    def sliced(x, m):
        wide = torch.zeros(x.shape[:3] + (5,), dtype=x.dtype, device=DEV)
        wide[..., 1:4] = x
        wide_m = torch.zeros(m.shape[:3] + (4,), dtype=m.dtype, device=DEV)
        wide_m[..., :3] = m
        assert not wide[..., 1:4].is_contiguous() and not wide_m[..., :3][0].is_contiguous()
        return wide[..., 1:4], wide_m[..., :3]
    _compare('sliced', tv, inv, tag, dtype, make_inputs=sliced)

    # a cotangent that is not contiguous
    x = tv.to(DEV).requires_grad_()
    cot = torch.ones(2, 2 * tv.shape[1], dtype=dtype, device=DEV)[:, ::2]
    assert not cot.is_contiguous()
    got, = torch.autograd.grad(tetrahedron_volume(x), x, cot)
    want, = torch.autograd.grad(tetrahedron_volume(x).sum(), x)
    assert torch.equal(got, want)
    loss_cot = torch.ones(2, 2, dtype=dtype, device=DEV)[:, :1]
    got, = torch.autograd.grad(amips(x, inv.to(DEV)), x, loss_cot)
    want, = torch.autograd.grad(amips(x, inv.to(DEV)).sum(), x)
    assert torch.equal(got, want)


def test_gradcheck():
    vertices, tets = jittered_grid(2, 1, torch.double)
    assert tets.shape == (48, 4)
    inv = inverse_vertices_offset(kuhn_grid(2, dtype=torch.double)[0][None][:, tets]).to(DEV).requires_grad_()
    p, t = vertices.to(DEV).requires_grad_(), tets.to(DEV)
    m = torch.tensor([1e-3], dtype=torch.double, device=DEV, requires_grad=True)
    # (the losses are scaled to order one, so that gradcheck's absolute tolerance means something)
    assert torch.autograd.gradcheck(lambda x: tetrahedron_volume(x[:, t]), (p,), nondet_tol=0)
    assert torch.autograd.gradcheck(lambda x: equivolume(x[:, t], pow=4) * 1e12, (p,), nondet_tol=0)
    assert torch.autograd.gradcheck(lambda x, y: equivolume(x[:, t], y, pow=2) * 1e6, (p, m), nondet_tol=0)
    assert torch.autograd.gradcheck(lambda x, y: amips(x[:, t], y), (p, inv), nondet_tol=0)


def test_deterministic():
    tv, inv = _case(16, 2, torch.float32)
    mean = torch.tensor([1e-4], device=DEV)
    runs = []
    for _ in range(2):
        x, m, mu = tv.to(DEV).requires_grad_(), inv.to(DEV).requires_grad_(), mean.clone().requires_grad_()
        outs = (tetrahedron_volume(x), equivolume(x, mu, pow=4), equivolume(x[:1], pow=2), amips(x, m))
        grads = torch.autograd.grad([o.sum() for o in outs], (x, m, mu))
        runs.append([o.detach() for o in outs] + list(grads))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_gradients_only_where_needed():
    tv, inv = _case(3, 2, torch.float32)
    x, m = tv.to(DEV).requires_grad_(), inv.to(DEV)
    amips(x, m).sum().backward()
    assert m.grad is None and x.grad is not None
    x, m = tv.to(DEV), inv.to(DEV).requires_grad_()
    amips(x, m).sum().backward()
    assert x.grad is None and m.grad is not None and m.grad.shape == inv.shape
    x, mu = tv.to(DEV), torch.tensor([1e-4], device=DEV, requires_grad=True)
    equivolume(x, mu).sum().backward()
    assert x.grad is None and mu.grad.shape == (1,)
    x, mu = tv.to(DEV).requires_grad_(), torch.tensor(1e-4, device=DEV)
    loss = equivolume(x, mu)                                     # a 0-d mean
    loss.sum().backward()
    assert mu.grad is None and x.grad is not None and loss.shape == (2, 1)
    assert not tetrahedron_volume(tv.to(DEV)).requires_grad


def test_other_inputs_take_the_torch_path(monkeypatch):
    monkeypatch.undo()
    tv, inv = _case(3, 2, torch.float32)
    x, m = tv.to(DEV), inv.to(DEV)
    calls = []

    def counted(name):
        inner = FORMULATIONS[name]
        monkeypatch.setattr(tetmesh, name, lambda *a: calls.append(name) or inner(*a))
    for name in FORMULATIONS:
        counted(name)
    assert tetrahedron_volume(x.half()).dtype == torch.half and calls == ['_torch_volume']
    del calls[:]
    assert equivolume(x[:1], pow=2.5).shape == (1, 1) and calls == ['_torch_equivolume', '_torch_volume']       # a float pow
    del calls[:]
    given = torch.linspace(0, 1e-3, x.shape[1], device=DEV)                                                    # M == T
    assert equivolume(x, given).shape == (2, 1) and calls == ['_torch_equivolume', '_torch_volume']
    del calls[:]
    assert amips(x[:, :0], m[:, :0]).shape == (2, 1) and tetrahedron_volume(x[:, :0]).shape == (2, 0)          # T == 0
    assert calls == ['_torch_amips', '_torch_volume']
    del calls[:]
    try:                                                       # (whatever torch's det does for half: the formulation was reached)
        assert amips(x.half(), m.half()).device == x.device
    except (RuntimeError, NotImplementedError):
        pass
    assert calls == ['_torch_amips']
    del calls[:]
    with pytest.raises(RuntimeError, match='must match the size of tensor b'):
        equivolume(x.reshape(1, -1, 4, 3)[:, :15].reshape(3, 5, 4, 3))                                         # B = 3, mean computed
    del calls[:]
    tetrahedron_volume(x), equivolume(x[:1]), equivolume(x, given[:1]), amips(x, m)                            # the HIP path:
    assert calls == []                                                                                         # no formulation runs


def test_graph_capture():
    """Forward and backward of the three operators in one captured graph; the replay equals the eager results bit for bit."""
    tv, inv = _case(8, 2, torch.float32)
    x, m = tv.to(DEV).requires_grad_(), inv.to(DEV).requires_grad_()
    mu = torch.tensor([1e-4], device=DEV, requires_grad=True)

    def step():
        volumes = tetrahedron_volume(x)
        losses = (equivolume(x, mu, pow=4), equivolume(x[:1], pow=2), amips(x, m))
        total = volumes.sum() * 1e-3 + losses[0].sum() * 1e12 + losses[1].sum() * 1e6 + losses[2].sum()
        return (volumes,) + losses + torch.autograd.grad(total, (x, m, mu))

    eager = [t.detach().clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                   # (warm the allocator on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.detach().zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b.detach()) for a, b in zip(eager, captured))
