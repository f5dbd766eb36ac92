"""The torch definition of the Simplicits training losses (kaolin_amd/physics/simplicits.py), in float64 on the CPU: the oracle of
tests/test_simplicits_training_gpu.py."""
import pytest
import torch

from kaolin_amd.physics import simplicits

N, B, HP = 3, 2, 2


def inputs(requires_grad=False):
    torch.manual_seed(7)
    w = torch.randn(N, HP, dtype=torch.float64, requires_grad=requires_grad)
    jac = torch.randn(N, HP, 3, dtype=torch.float64, requires_grad=requires_grad)
    pts, tfms = torch.rand(N, 3, dtype=torch.float64), 0.1 * torch.randn(B, HP, 3, 4, dtype=torch.float64)
    mus, lams = 1 + torch.rand(N, dtype=torch.float64), 2 + torch.rand(N, dtype=torch.float64)
    return w, jac, pts, tfms, mus, lams


@pytest.mark.parametrize('s', [0.0, 0.5, 1.0])
def test_gradcheck_in_weights_and_jacobian(s):
    w, jac, *rest = inputs(requires_grad=True)
    assert torch.autograd.gradcheck(lambda w, jac: simplicits.training_losses(w, jac, *rest, s, 0.7, 1.3), (w, jac))
    assert torch.autograd.gradcheck(simplicits.loss_ortho, (w,))


def test_zero_transforms_and_orthonormal_weights():
    w, jac, pts, tfms, mus, lams = inputs()
    for s in (0.0, 0.5, 1.0):
        assert simplicits.training_losses(w, jac, pts, torch.zeros_like(tfms), mus, lams, s)[0].item() == 0.0
    q = torch.linalg.qr(torch.randn(5, HP, dtype=torch.float64))[0]
    assert simplicits.loss_ortho(q).item() <= 1e-30
    with pytest.raises(ValueError):
        simplicits.loss_elastic(None, pts, mus, lams, mus, tfms, 1.0, 0.5, elasticity_type='linear')


def test_closed_form_F_is_the_derivative_of_standard_lbs():
    """loss_elastic at (mu, lam) = (1, 0), s = 0 is (vol / N) sum |eps(F)|^2: the closed-form F against a central difference of
    standard_lbs, whose truncation is delta^2 / 6 times a third derivative of order one"""
    torch.manual_seed(3)
    model = simplicits.SimplicitsMLP(3, 16, HP + 1, 1).double()
    w_, jac, pts, tfms, mus, lams = inputs()
    delta = 1e-4
    skin = lambda x: simplicits.standard_lbs(x, tfms, model(x))[:, :, 0]                    # (N, B, 3)
    cols = [(skin(pts + delta * e) - skin(pts - delta * e)) / (2 * delta) for e in torch.eye(3, dtype=torch.float64)]
    F = torch.stack(cols, dim=-1)                                                             # (N, B, 3, 3), d x_i / d x0_j
    eps = (F + F.transpose(-1, -2)) / 2 - torch.eye(3, dtype=torch.float64)
    want = (2.0 / N) * (eps * eps).sum()
    with torch.no_grad():
        got = simplicits.loss_elastic(model, pts, 2 * torch.ones(N, 1, dtype=torch.float64), torch.zeros(N, dtype=torch.float64), None,
                                      tfms, 2.0, 0.0)
    assert abs(got.item() - want.item()) <= 10 * delta ** 2 * want.item()
