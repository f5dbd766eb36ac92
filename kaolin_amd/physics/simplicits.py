r"""The reduced (Simplicits) degrees of freedom: :math:`H` handles with a 3x4 delta transform :math:`Z_h` each, skinned to
:math:`N` points by ``weights``; :math:`D = 12 H`, the flat index of :math:`Z_h[b][n]` is :math:`12 h + 4 b + n`.

With :math:`\tilde x_p = (x, y, z, 1)` and :math:`M_{p,h}[m][n] = \partial_m w_{p,h} \, \tilde x_p[n] + w_{p,h} \delta_{mn}`
(3x4), the rows :math:`9 p + 3 b + m` of :math:`\partial F / \partial z` hold :math:`M_{p,h}[m][n]` in the columns
:math:`12 h + 4 b + n` (the 9x12 block :math:`I_3 \otimes M_{p,h}`) and zeros elsewhere, and

.. math::
    F_p = I + \sum_h \left( w_{p,h} Z_h[:, :3] + (Z_h \tilde x_p) \otimes \nabla w_{p,h} \right)

The reference keeps :math:`\partial F / \partial z` as a sparse Warp matrix (kaolin/physics/simplicits/precomputed.py) and
densifies it for the Hessian's reduction; :func:`reduced_neohookean_terms` on a GPU never forms it (csrc/physics.hip).
These are a solver's forward quantities: nothing here records an autograd graph.
"""
import torch

from .. import _C
from .materials import _check_floating, _neohookean_terms, _on_hip

__all__ = ['dFdz_matrix', 'get_defo_grad', 'reduced_neohookean_terms']


def _check_skinning(weights, weights_jac, pts, **per_point):
    _check_floating(weights=weights, weights_jac=weights_jac, pts=pts, **per_point)
    if weights.dim() != 2:
        raise ValueError(f'weights must be of shape (N, H), got {tuple(weights.shape)}')
    N, H = weights.shape
    if H < 1:
        raise ValueError('weights must have a handle')
    for name, t, shape in [('weights_jac', weights_jac, (N, H, 3)), ('pts', pts, (N, 3))] + \
                          [(name, t, (N,)) for name, t in per_point.items()]:
        if tuple(t.shape) != shape:
            raise ValueError(f'{name} must be of shape {shape}, got {tuple(t.shape)}')
    return N, H


def _check_z(z, H, like):
    _check_floating(weights=like, z=z)
    if tuple(z.shape) not in ((H, 3, 4), (12 * H,)):
        raise ValueError(f'z must be of shape ({H}, 3, 4) or ({12 * H},), got {tuple(z.shape)}')
    return z.detach().reshape(H, 3, 4)


def _homogeneous(pts):
    return torch.cat([pts, torch.ones_like(pts[:, :1])], dim=1)


def dFdz_matrix(weights, weights_jac, pts):
    r"""The Jacobian of the deformation gradients with respect to the flat transforms, dense, in plain torch: the definition
    the fused path is tested against, and fit for small problems.

    Args:
        weights (torch.Tensor): skinning weights, of shape :math:`(N, H)`.
        weights_jac (torch.Tensor): their spatial gradients :math:`\partial w_h / \partial x`, of shape :math:`(N, H, 3)`.
        pts (torch.Tensor): the points, of shape :math:`(N, 3)`.

    Returns:
        (torch.Tensor): of shape :math:`(9 N, 12 H)`.
    """
    N, H = _check_skinning(weights, weights_jac, pts)
    weights, weights_jac, pts = weights.detach(), weights_jac.detach(), pts.detach()
    eye34 = torch.eye(3, 4, dtype=pts.dtype, device=pts.device)
    M = weights_jac[:, :, :, None] * _homogeneous(pts)[:, None, None, :] + weights[:, :, None, None] * eye34   # (N, H, m, n)
    out = torch.zeros((N, 3, 3, H, 3, 4), dtype=pts.dtype, device=pts.device)                              # (p, b, m, h, b, n)
    for b in range(3):
        out[:, b, :, :, b, :] = M.permute(0, 2, 1, 3)
    return out.reshape(9 * N, 12 * H)


def get_defo_grad(z, weights, weights_jac, pts):
    r"""The deformation gradient of every point, :math:`F_p = I + (\partial F / \partial z)_p \, z` in its closed form.

    Args:
        z (torch.Tensor): the delta transforms, of shape :math:`(H, 3, 4)` or flat :math:`(12 H,)`.
        weights, weights_jac, pts: as in :func:`dFdz_matrix`.

    Returns:
        (torch.Tensor): of shape :math:`(N, 3, 3)`.
    """
    N, H = _check_skinning(weights, weights_jac, pts)
    Z = _check_z(z, H, weights)
    Zx = torch.einsum('hbn,pn->phb', Z, _homogeneous(pts.detach()))
    return torch.eye(3, dtype=pts.dtype, device=pts.device) + torch.einsum('ph,hbm->pbm', weights.detach(), Z[:, :, :3]) + \
        torch.einsum('phb,phm->pbm', Zx, weights_jac.detach())


def _reduced_definition(Z, pts, weights, weights_jac, mu, lam, vol, coeff, hessian):
    """Dense dFdz, the per-point blocks, bmm and matmul"""
    N, D = pts.shape[0], 12 * Z.shape[0]
    dF = dFdz_matrix(weights, weights_jac, pts)
    F = get_defo_grad(Z, weights, weights_jac, pts)
    E, P, Hs = _neohookean_terms(F, mu, lam, vol * coeff, hessian=hessian)
    g = dF.T @ P.reshape(9 * N)
    K = dF.T @ torch.bmm(Hs, dF.reshape(N, 9, D)).reshape(9 * N, D) if hessian else None
    return E, g, K


def reduced_neohookean_terms(z, pts, weights, weights_jac, mu, lam, vol, coeff=1.0, hessian=True):
    r"""The Neo-Hookean energy of the skinned points, its gradient and its Hessian with respect to the flat transforms:

    .. math::
        E = \text{coeff} \sum_p vol_p \Psi(F_p), \quad g = \frac{\partial F}{\partial z}^T \operatorname{vec}(P), \quad
        K = \frac{\partial F}{\partial z}^T \operatorname{blockdiag}(H_p) \frac{\partial F}{\partial z}

    with :math:`P_p`, :math:`H_p` the gradient and Hessian of :class:`~kaolin_amd.physics.materials.NeohookeanElasticMaterial`
    (cofactor from 2x2 minors: finite for a singular or inverted :math:`F`, where the reference returns NaN).

    float32 tensors on a GPU with at most ``kaolin_amd._C.physics.max_handles()`` handles run one fused HIP kernel and a
    finishing launch: :math:`\partial F / \partial z` and the :math:`(N, 9, 9)` blocks are never allocated, :math:`K` is
    symmetric to the bit, and the same inputs give the same bits on every call.  Everything else (CPU, float64, more handles)
    runs the dense torch definition.  No autograd: these are the forward quantities of a Newton step.

    Args:
        z (torch.Tensor): the delta transforms, of shape :math:`(H, 3, 4)` or flat :math:`(12 H,)`.
        pts (torch.Tensor): the points, of shape :math:`(N, 3)`.
        weights (torch.Tensor): skinning weights, of shape :math:`(N, H)`.
        weights_jac (torch.Tensor): their spatial gradients, of shape :math:`(N, H, 3)`.
        mu, lam, vol (torch.Tensor): Lame coefficients and volume per point, each of shape :math:`(N,)`.
        coeff (float): scales all three results.
        hessian (bool): compute :math:`K`.  Default: True.

    Returns:
        (torch.Tensor, torch.Tensor, torch.Tensor or None): :math:`E` of shape :math:`(1,)`, :math:`g` of shape :math:`(D,)`
        and :math:`K` of shape :math:`(D, D)`, or None without ``hessian``.
    """
    N, H = _check_skinning(weights, weights_jac, pts, mu=mu, lam=lam, vol=vol)
    Z = _check_z(z, H, weights)
    D = 12 * H
    if N == 0:
        zeros = pts.new_zeros
        return zeros(1), zeros(D), zeros((D, D)) if hessian else None
    tensors = [t.detach() for t in (pts, weights, weights_jac, mu, lam, vol)]
    if _on_hip(Z, *tensors) and H <= _C.physics.max_handles():
        return _C.physics.reduced_neohookean_cuda(Z.reshape(D).contiguous(), *(t.contiguous() for t in tensors), coeff,
                                                  hessian=hessian)
    return _reduced_definition(Z, *tensors, coeff, hessian)
