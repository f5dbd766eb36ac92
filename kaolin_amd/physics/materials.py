"""Elastic materials on torch tensors (the reference's classes, kaolin/physics/materials, take Warp arrays of the same shapes).

With :math:`J = \\det F` and :math:`C = \\operatorname{cof} F = \\partial J / \\partial F`, the Neo-Hookean terms per point are

.. math::
    \\Psi = \\tfrac{\\mu}{2} (\\|F\\|^2 - 3) + \\tfrac{\\lambda}{2} (J - 1)^2 - \\mu (J - 1), \\quad
    \\frac{\\partial \\Psi}{\\partial F} = \\mu F + (\\lambda (J - 1) - \\mu) C, \\quad
    \\frac{\\partial^2 \\Psi}{\\partial F^2} = \\mu I_9 + \\lambda \\operatorname{vec}(C) \\operatorname{vec}(C)^T
        + (\\lambda (J - 1) - \\mu) \\frac{\\partial C}{\\partial F}

each scaled by the point's volume and ``coeff``; :math:`\\operatorname{vec}` is row-major and :math:`\\partial C / \\partial F`
is the cross-product operator, linear in :math:`F`.  :math:`C` is computed from 2x2 minors, never from ``inverse(F)``: the same
function as the reference's :math:`J F^{-T}` wherever :math:`F` is invertible, and finite for a singular or inverted :math:`F`,
where the reference returns NaN.  The difference is deliberate.

float32 tensors on a GPU run csrc/physics.hip; everything else (CPU, float64) runs the torch definition in this file.  These
are a solver's forward quantities: nothing here records an autograd graph.
"""
import torch

from .. import _C

__all__ = ['to_lame', 'NeohookeanElasticMaterial']


def to_lame(yms, prs):
    r"""Converts Young's moduli and Poisson ratios to the Lame parameters :math:`(\mu, \lambda)`.

    Args:
        yms (torch.Tensor): Young's moduli.
        prs (torch.Tensor): Poisson ratios, of the same shape.

    Returns:
        (torch.Tensor, torch.Tensor): :math:`\mu = E / (2 (1 + \nu))` and :math:`\lambda = E \nu / ((1 + \nu) (1 - 2 \nu))`.
    """
    return yms / (2 * (1 + prs)), yms * prs / ((1 + prs) * (1 - 2 * prs))


def _check_floating(**tensors):
    """Tensors of one floating dtype on one device"""
    first = None
    for name, t in tensors.items():
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise TypeError(f'{name} must be a floating-point tensor, got {getattr(t, "dtype", type(t))}')
        if first is not None and (t.dtype != first.dtype or t.device != first.device):
            raise TypeError(f'{name} is {t.dtype} on {t.device}, expected {first.dtype} on {first.device}')
        first = t if first is None else first


def _on_hip(*tensors):
    return all(t.is_cuda and t.dtype == torch.float32 for t in tensors)


def _levi_civita(ref):
    eps = torch.zeros(3, 3, 3, dtype=ref.dtype, device=ref.device)
    for i, j, k in ((0, 1, 2), (1, 2, 0), (2, 0, 1)):
        eps[i, j, k], eps[i, k, j] = 1, -1
    return eps


def _cofactor(F):
    """(N, 3, 3) -> cof F (each row the cross product of F's other two rows) and det F"""
    r0, r1, r2 = F[:, 0], F[:, 1], F[:, 2]
    C = torch.stack([torch.linalg.cross(r1, r2), torch.linalg.cross(r2, r0), torch.linalg.cross(r0, r1)], dim=1)
    return C, (r0 * C[:, 0]).sum(dim=-1)


def _neohookean_terms(F, mu, lam, scale, energy=True, gradient=True, hessian=True):
    """The definition: (sum of scale * Psi (1,), scale * dPsi/dF (N, 3, 3), scale * d2Psi/dF2 (N, 9, 9)), None where not asked"""
    C, J = _cofactor(F)
    a = lam * (J - 1) - mu
    E = P = Hs = None
    if energy:
        E = (scale * (mu / 2 * ((F * F).sum(dim=(1, 2)) - 3) + lam / 2 * (J - 1) ** 2 - mu * (J - 1))).sum().reshape(1)
    if gradient:
        P = scale[:, None, None] * (mu[:, None, None] * F + a[:, None, None] * C)
    if hessian:
        eps = _levi_civita(F)
        dCdF = torch.einsum('ikx,jly,nxy->nijkl', eps, eps, F).reshape(-1, 9, 9)
        c = C.reshape(-1, 9)
        Hs = mu[:, None, None] * torch.eye(9, dtype=F.dtype, device=F.device) + lam[:, None, None] * c[:, :, None] * c[:, None, :]
        Hs = scale[:, None, None] * (Hs + a[:, None, None] * dCdF)
    return E, P, Hs


class NeohookeanElasticMaterial:
    r"""Neo-Hookean elastic material over :math:`N` integration points (see the module's text for the terms).

    Args:
        mu (torch.Tensor): Lame coefficient :math:`\mu`, of shape :math:`(N,)`.
        lam (torch.Tensor): Lame coefficient :math:`\lambda`, of shape :math:`(N,)`.
        integration_pt_volume (torch.Tensor): the volume each point stands for, of shape :math:`(N,)`.
        reparameterize_lame (bool): use :math:`\lambda + \mu` for :math:`\lambda`, so that the linearised energy matches
            linear elasticity (Stable Neo-Hookean Flesh Simulation).  Default: False.
    """

    def __init__(self, mu, lam, integration_pt_volume, reparameterize_lame=False):
        _check_floating(mu=mu, lam=lam, integration_pt_volume=integration_pt_volume)
        if not (mu.dim() == 1 and mu.shape == lam.shape == integration_pt_volume.shape):
            raise ValueError(f'mu, lam and integration_pt_volume must be of one shape (N,), got {tuple(mu.shape)}, '
                             f'{tuple(lam.shape)}, {tuple(integration_pt_volume.shape)}')
        self.mu = mu.detach().contiguous()
        self.lam = (lam + mu if reparameterize_lame else lam).detach().contiguous()
        self.integration_pt_volume = integration_pt_volume.detach().contiguous()

    def __str__(self):
        return 'NeohookeanElasticMaterial'

    def _terms(self, defo_grads, coeff, energy=False, gradient=False, hessian=False):
        _check_floating(mu=self.mu, defo_grads=defo_grads)
        if defo_grads.dim() != 3 or tuple(defo_grads.shape) != (self.mu.shape[0], 3, 3):
            raise ValueError(f'defo_grads must be of shape ({self.mu.shape[0]}, 3, 3), got {tuple(defo_grads.shape)}')
        F = defo_grads.detach()
        if _on_hip(F):
            return _C.physics.neohookean_cuda(F.contiguous(), self.mu, self.lam, self.integration_pt_volume, coeff,
                                              energy=energy, gradient=gradient, hessian=hessian)
        return _neohookean_terms(F, self.mu, self.lam, self.integration_pt_volume * coeff, energy, gradient, hessian)

    def energy(self, defo_grads, coeff=1.0):
        r"""The total energy :math:`\text{coeff} \sum_p vol_p \Psi(F_p)`, of shape :math:`(1,)`, for ``defo_grads`` of shape
        :math:`(N, 3, 3)`.  On the GPU the sum has one fixed order: the same bits on every call."""
        return self._terms(defo_grads, coeff, energy=True)[0]

    def gradient(self, defo_grads, coeff=1.0):
        r"""The energy's gradient per point :math:`\text{coeff} \cdot vol_p \, \partial \Psi / \partial F_p`, of shape
        :math:`(N, 3, 3)`."""
        return self._terms(defo_grads, coeff, gradient=True)[1]

    def hessian(self, defo_grads, coeff=1.0):
        r"""The energy's Hessian blocks :math:`\text{coeff} \cdot vol_p \, \partial^2 \Psi / \partial F_p^2`, of shape
        :math:`(N, 9, 9)`, rows and columns in row-major order of :math:`F`."""
        return self._terms(defo_grads, coeff, hessian=True)[2]
