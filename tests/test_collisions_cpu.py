"""kaolin_amd.physics.collisions without a GPU: the torch formulation of the detection contract against the all-pairs numpy
oracle, bit for bit, and of the contact terms against float64 autograd of the reference test's analytic energy
(tests/collisions_bruteforce.py).  Every figure is printed before it is asserted (pytest -s)."""
import functools

import pytest
import torch

import collisions_bruteforce as bf
from kaolin_amd.physics import Collision, collisions

# what each case must contain for its rule to bite
BITES = {
    'n257': lambda col, total: total > 100,
    'one_cell': lambda col, total: total > 100,
    'exact': lambda col, total: total == 1,
    'duplicates': lambda col, total: (col.collision_normals == 0).all(dim=1).sum() == 2,
    'nan': lambda col, total: total > 10 and not {11, 30} & set(col.collision_indices_a.tolist() + col.collision_indices_b.tolist()),
    'immune': lambda col, total: 0 < (col.collision_indices_a % 2 == col.collision_indices_b % 2).sum() < total,
    'static': lambda col, total: (col.collision_indices_a == -1).any() and (col.collision_indices_b >= 20).all() and total > 3,
    'none': lambda col, total: total == 0 and col.object_pairs == [] and col.collision_normals.shape == (0, 3),
}


@pytest.mark.parametrize('name', bf.DETECTION_CASES)
def test_detection(name, caplog):
    col, total = bf.check_detection(name, 'cpu', caplog)
    assert BITES.get(name, lambda *_: True)(col, total)


def test_detection_overflow_keeps_the_smallest_pairs(caplog):
    assert bf.check_detection('n257', 'cpu', caplog, max_pairs=37)[1] > 37


def test_object_pairs_and_jacobian():
    """The static scene: object 0 static against object 1 -> the reference's four pairs; J against the LBS rows of the points"""
    dx, x0, obj, static, kw = bf.detection_case('static')
    col = Collision(dt=0.01, **kw)
    col.detect_collisions(*(torch.from_numpy(t) for t in (dx, x0, obj, static)))
    assert col.object_pairs.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]
    w, x = torch.rand(42, 3, dtype=torch.float64), torch.from_numpy(x0).double()
    col.calculate_jacobian(w, x)
    B = torch.einsum('ph,pn,bc->pbhcn', w, torch.cat([x, torch.ones(42, 1)], dim=1).double(), torch.eye(3).double()).reshape(42, 3, 36)
    rows = lambda i: torch.where((i >= 0)[:, None, None], B[i.long().clamp(min=0)], torch.zeros(1).double())
    assert torch.equal(col.collision_J_dense, (rows(col.collision_indices_a) - rows(col.collision_indices_b)).reshape(-1, 36))
    with pytest.raises(NotImplementedError):
        col.get_bounds(None, None, None)


@functools.lru_cache(maxsize=None)
def contacts():
    d = bf.synthetic(300, 50, 3, seed=5, static=True)
    return d, bf.terms64(d)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_terms_against_autograd(dtype):
    """float64: the formulation is the energy's derivative up to the limit form of the first regime; float32: within the
    yardstick's own limit, e_def < 1e-4, on the inputs the GPU test uses"""
    d, (G64, H64) = contacts()
    col, dx, w, x0 = bf.collision_of(d, dtype, 'cpu')
    E, G, Hs = col.energy(dx, x0, bf.COEFF), col.gradient(dx, x0, bf.COEFF), col.hessian(dx, x0, bf.COEFF)
    offset = collisions._contact_offsets(d['dx'], d['dx0'], d['gaps'], d['ia'], d['ib'])
    E64 = bf.energy64(offset, d['normals'], torch.where(d['ib'] < 0, 1.0, 2.0).double() * bf.RADIUS)
    assert E.shape == (1,) and G.shape == (300, 3) and Hs.shape == (300, 3, 3) and E.dtype == G.dtype == Hs.dtype == dtype
    bound = bf.LIMIT_FORM if dtype == torch.float64 else 1e-4
    for name, got, ref in (('energy', E, E64.sum().reshape(1)), ('gradient', G, G64), ('hessian', Hs, H64)):
        e = (got.double() - ref).abs().max().item() / ref.abs().max().item()
        print(f'{name} {dtype}: e {e:.3e}')
        assert e < bound
    inactive = E64 == 0
    assert inactive.sum() > 30 and (G[inactive] == 0).all() and (Hs[inactive] == 0).all() and (G[~inactive] != 0).any(dim=1).all()
    total = torch.ones(1, dtype=dtype)
    assert col.energy(dx, x0, bf.COEFF, energy=total) is total and torch.equal(total, 1 + E)


def test_reduced_terms_cpu():
    d, _ = contacts()
    col, dx, w, x0 = bf.collision_of(d, torch.float64, 'cpu')
    E, g, K = col.reduced_terms(dx, w, x0, bf.COEFF)
    col.calculate_jacobian(w, x0)
    J, G, Hs = col.collision_J_dense, col.gradient(dx, x0, bf.COEFF), col.hessian(dx, x0, bf.COEFF)
    assert torch.equal(E, col.energy(dx, x0, bf.COEFF)) and torch.allclose(g, J.T @ G.reshape(-1), rtol=1e-12, atol=0)
    assert torch.allclose(K, J.T @ torch.block_diag(*Hs) @ J, rtol=1e-10, atol=1e-12 * K.abs().max().item())
    E2, g2, K2 = col.reduced_terms(dx, w, x0, bf.COEFF, hessian=False)
    assert K2 is None and torch.equal(E2, E) and torch.equal(g2, g)
    col.num_contacts, col.collision_indices_a = 0, col.collision_indices_a[:0]
    assert [t.abs().sum().item() for t in col.reduced_terms(dx, w, x0, bf.COEFF)] == [0, 0, 0]
