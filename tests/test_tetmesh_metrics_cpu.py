"""kaolin.metrics.tetmesh without a GPU: the torch formulations of kaolin_amd/metrics/tetmesh.py (what every input outside the
HIP path runs, and what test_tetmesh_metrics_gpu.py compares the kernels with at shapes no record holds) against the reference's
recorded answers (tests/golden/tetmesh_metrics.npz, written by make_golden_tetmesh_metrics.py): results, gradients, error types and
texts, dtypes, and the reference's quirks."""
import pytest
import torch

from kaolin_amd.metrics import tetmesh
from kaolin_amd.metrics.tetmesh import amips, equivolume, tetrahedron_volume
from tetmesh_metrics_golden import (DTYPES, golden, grid9, jittered_grid, known_answers, records_amips, records_equivolume,
                                    records_volume, tensor)


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_known_answers(tag, dtype):
    known_answers('cpu', tag, dtype)


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_volume_records(tag, dtype):
    records_volume('cpu', tag, dtype)


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_equivolume_records(tag, dtype):
    records_equivolume('cpu', tag, dtype)


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_amips_records(tag, dtype):
    records_amips('cpu', tag, dtype)


def _raises(name, fn):
    kind, text = golden()[f'err_{name}']
    with pytest.raises(Exception) as info:
        fn()
    assert type(info.value).__name__ == kind and str(info.value) == text, (name, info.value)


def test_errors_match_reference():
    for name, fn in (('tetrahedron_volume', tetrahedron_volume), ('equivolume', equivolume),
                     ('amips', lambda x: amips(x, torch.zeros(1, 2, 3, 3)))):
        _raises(f'{name}_ndim', lambda: fn(torch.zeros(2, 2)))
        _raises(f'{name}_dim2', lambda: fn(torch.zeros(1, 2, 3, 3)))
        _raises(f'{name}_dim3', lambda: fn(torch.zeros(1, 2, 4, 2)))
    gv, gt = grid9()
    five = gv[:1, gt[:15]].reshape(3, 5, 4, 3)
    _raises('equivolume_batch3x5', lambda: equivolume(five))
    _raises('equivolume_mean3_t5', lambda: equivolume(five, torch.zeros(3)))


def test_equivolume_broadcasts_along_the_tet_axis():
    """B == T: the mean of item j is subtracted from tet j (what the reference returns for its docstring's example, not what its
    docstring means); M == T with a given mean likewise."""
    tv = tensor('kat_equivolume_in0').double()
    v = tetrahedron_volume(tv)
    want = ((v - v.mean(-1).reshape(1, 2)).abs() ** 4).mean(-1, keepdim=True)
    assert torch.equal(equivolume(tv), want)
    per_item = ((v - v.mean(-1, keepdim=True)).abs() ** 4).mean(-1, keepdim=True)
    assert not torch.allclose(want, per_item, rtol=1e-3, atol=0)
    given = torch.tensor([1e-3, -2e-3], dtype=torch.double)
    assert torch.equal(equivolume(tv, given, pow=2), ((v - given.reshape(1, 2)).abs() ** 2).mean(-1, keepdim=True))


def test_no_tetrahedrons():
    empty = torch.zeros(2, 0, 4, 3)
    assert tetrahedron_volume(empty).shape == (2, 0)
    loss = equivolume(empty[:1])
    assert loss.shape == (1, 1) and bool(torch.isnan(loss).all())           # the mean of nothing, as the reference's
    loss = amips(empty, torch.zeros(2, 0, 3, 3))
    assert loss.shape == (2, 1) and bool(torch.isnan(loss).all())


def test_float_pow():
    tv, tets = jittered_grid(2, 1, torch.double)
    tv = tv[:, tets]
    v = tetrahedron_volume(tv)
    assert torch.equal(equivolume(tv, pow=2.5), ((v - v.mean()).abs() ** 2.5).mean(-1, keepdim=True))


def test_dtypes_match_reference():
    g = golden()
    tets = jittered_grid(6, 1, torch.float)[1]
    from tetmesh_metrics_golden import amips_tet_vertices
    small, small_inv = amips_tet_vertices(tensor('amips_vertices'), tets)[:, :8], tensor('amips_inv_f32')[:, :8]
    cases = {'volume_half': lambda: tetrahedron_volume(small.half()), 'equivolume_half': lambda: equivolume(small[:1].half()),
             'amips_half': lambda: amips(small.half(), small_inv.half()),
             'equivolume_mixed': lambda: equivolume(small, torch.tensor([1e-3], dtype=torch.float64)),
             'amips_mixed': lambda: amips(small, small_inv.double()), 'amips_f64': lambda: amips(small.double(), small_inv.double())}
    for name, fn in cases.items():
        record = list(g[f'dtypes_{name}'])
        if record[0] == 'raises':
            with pytest.raises(Exception) as info:
                fn()
            assert [type(info.value).__name__, str(info.value)] == record[1:], name
        else:
            assert str(fn().dtype) == record[0], name


def test_gradcheck_of_the_formulations():
    vertices, tets = jittered_grid(2, 1, torch.double)
    assert tets.shape == (48, 4)
    rest = jittered_grid(2, 1, torch.double, jitter=0.0)[0][:, tets]
    inv = torch.inverse(rest[:, :, 1:] - rest[:, :, :1]).requires_grad_()
    p = vertices.clone().requires_grad_()
    m = torch.tensor([1e-3], dtype=torch.double, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x: tetmesh._torch_volume(x[:, tets]), (p,))
    assert torch.autograd.gradcheck(lambda x: tetmesh._torch_equivolume(x[:, tets], None, 4) * 1e12, (p,))
    assert torch.autograd.gradcheck(lambda x, y: tetmesh._torch_equivolume(x[:, tets], y, 2) * 1e6, (p, m))
    assert torch.autograd.gradcheck(lambda x, y: tetmesh._torch_amips(x[:, tets], y), (p, inv))
