"""kaolin_amd.physics, the torch definition path in float64 on the CPU, against autograd of the one scalar energy.  Both sides
are float64 and differ by rounding only: 1e-9 of the largest entry."""
import pytest
import torch

from kaolin_amd.physics import materials, simplicits

COEFF = 0.7


def make_inputs(N, H, seed=0, dtype=torch.float64):
    """Seeded: softmax weights, 0.5 randn weight gradients, points in [-1, 1]^3, z = 0.1 randn (F near I, J > 0), positive
    mu, lam, vol that differ per point"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    d = dict(z=0.1 * r(H, 3, 4), pts=2 * torch.rand(N, 3, generator=gen, dtype=torch.float64) - 1,
             weights=torch.softmax(r(N, H), dim=1), weights_jac=0.5 * r(N, H, 3), mu=1 + r(N).abs(), lam=2 + 3 * r(N).abs(),
             vol=0.1 + 0.05 * r(N).abs())
    return {k: v.to(dtype) for k, v in d.items()}


def close(a, b, rtol=1e-9):
    return (a - b).abs().max() <= rtol * b.abs().max()


def energy(F, mu, lam, vol):
    """The one scalar everything is derived from, written out with torch.det for autograd"""
    J = torch.det(F)
    return COEFF * (vol * (mu / 2 * ((F * F).sum(dim=(1, 2)) - 3) + lam / 2 * (J - 1) ** 2 - mu * (J - 1))).sum()


@pytest.mark.parametrize('reparameterize', [False, True])
@pytest.mark.parametrize('N', [1, 5])
def test_material_against_autograd(N, reparameterize):
    d = make_inputs(N, 2, seed=N)
    mat = materials.NeohookeanElasticMaterial(d['mu'], d['lam'], d['vol'], reparameterize_lame=reparameterize)
    F = simplicits.get_defo_grad(d['z'], d['weights'], d['weights_jac'], d['pts'])
    of_F = lambda F: energy(F, d['mu'], d['lam'] + d['mu'] if reparameterize else d['lam'], d['vol'])
    assert mat.energy(F, COEFF).shape == (1,) and close(mat.energy(F, COEFF)[0], of_F(F))
    assert close(mat.gradient(F, COEFF), torch.autograd.functional.jacobian(of_F, F))
    full = torch.autograd.functional.hessian(of_F, F).reshape(N, 9, N, 9)
    assert close(mat.hessian(F, COEFF), torch.stack([full[p, :, p, :] for p in range(N)]))


@pytest.mark.parametrize('H', [1, 3])
def test_reduced_terms_against_autograd(H):
    d = make_inputs(7, H, seed=H)
    rest = {k: d[k] for k in ('pts', 'weights', 'weights_jac', 'mu', 'lam', 'vol')}
    dF = simplicits.dFdz_matrix(d['weights'], d['weights_jac'], d['pts'])
    F = simplicits.get_defo_grad(d['z'], d['weights'], d['weights_jac'], d['pts'])
    assert dF.shape == (63, 12 * H)
    assert close((dF @ d['z'].flatten()).reshape(7, 3, 3) + torch.eye(3, dtype=torch.float64), F)

    of_z = lambda z: energy((dF @ z).reshape(7, 3, 3) + torch.eye(3, dtype=torch.float64), d['mu'], d['lam'], d['vol'])
    E, g, K = simplicits.reduced_neohookean_terms(d['z'].flatten(), coeff=COEFF, **rest)
    assert E.shape == (1,) and g.shape == (12 * H,) and K.shape == (12 * H, 12 * H)
    assert close(E[0], of_z(d['z'].flatten()))
    assert close(g, torch.autograd.functional.jacobian(of_z, d['z'].flatten()))
    assert close(K, torch.autograd.functional.hessian(of_z, d['z'].flatten()))
    E2, g2, K2 = simplicits.reduced_neohookean_terms(d['z'], coeff=COEFF, hessian=False, **rest)
    assert torch.equal(E2, E) and torch.equal(g2, g) and K2 is None


def test_singular_deformation_gradient():
    """F = 0: everything finite, and the limit of the closed form: P = 0, H = mu I9 vol coeff"""
    one, mu = torch.ones(1, dtype=torch.float64), torch.tensor([1.5], dtype=torch.float64)
    z = torch.cat([-torch.eye(3, dtype=torch.float64), torch.zeros(3, 1, dtype=torch.float64)], dim=1)[None]
    args = dict(weights=one[:, None], weights_jac=torch.zeros(1, 1, 3, dtype=torch.float64), pts=torch.rand(1, 3, dtype=torch.float64))
    F = simplicits.get_defo_grad(z, **args)
    assert torch.equal(F, torch.zeros(1, 3, 3, dtype=torch.float64))
    mat = materials.NeohookeanElasticMaterial(mu, 4 * one, 0.5 * one)
    assert torch.isfinite(mat.energy(F, COEFF)).all()
    assert torch.equal(mat.gradient(F, COEFF), torch.zeros_like(F))
    assert torch.allclose(mat.hessian(F, COEFF)[0], 1.5 * 0.5 * COEFF * torch.eye(9, dtype=torch.float64), rtol=1e-15, atol=0)
    E, g, K = simplicits.reduced_neohookean_terms(z, mu=mu, lam=4 * one, vol=0.5 * one, coeff=COEFF, **args)
    assert torch.isfinite(E).all() and torch.equal(g, torch.zeros(12, dtype=torch.float64)) and torch.isfinite(K).all()


@pytest.mark.parametrize('change,error', [
    (dict(z=torch.zeros(3, 3, 4, dtype=torch.float64)), ValueError),              # another H
    (dict(z=torch.zeros(2, 12, dtype=torch.float64)), ValueError),                # wrong rank
    (dict(pts=torch.zeros(4, 3, dtype=torch.float64)), ValueError),               # another N
    (dict(weights=torch.zeros(5, dtype=torch.float64)), ValueError),
    (dict(weights_jac=torch.zeros(5, 2, dtype=torch.float64)), ValueError),
    (dict(mu=torch.ones(6, dtype=torch.float64)), ValueError),
    (dict(vol=torch.ones(5, dtype=torch.int64)), TypeError),
    (dict(pts=torch.zeros(5, 3, dtype=torch.int32)), TypeError),
    (dict(lam=torch.ones(5, dtype=torch.float32)), TypeError),                    # mixed dtypes
])
def test_bad_arguments_raise(change, error):
    d = {**make_inputs(5, 2), **change}
    with pytest.raises(error):
        simplicits.reduced_neohookean_terms(**d)


def test_bad_material_arguments_raise():
    with pytest.raises(ValueError):
        materials.NeohookeanElasticMaterial(torch.ones(5), torch.ones(4), torch.ones(5))
    with pytest.raises(TypeError):
        materials.NeohookeanElasticMaterial(torch.ones(5), torch.ones(5), torch.ones(5, dtype=torch.int64))
    with pytest.raises(ValueError):
        materials.NeohookeanElasticMaterial(torch.ones(5), torch.ones(5), torch.ones(5)).gradient(torch.zeros(5, 9))


def test_no_points():
    d = make_inputs(0, 2)
    E, g, K = simplicits.reduced_neohookean_terms(**d)
    assert torch.equal(E, torch.zeros(1, dtype=torch.float64)) and torch.equal(g, torch.zeros(24, dtype=torch.float64))
    assert torch.equal(K, torch.zeros(24, 24, dtype=torch.float64))
    assert materials.to_lame(torch.tensor(1e5), torch.tensor(0.45))[0] == pytest.approx(1e5 / 2.9)
