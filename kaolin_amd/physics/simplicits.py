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

The inputs of those come from a skinning network: :class:`SkinningModule` and :class:`SimplicitsMLP` (the reference's
kaolin/physics/simplicits/network.py; state dicts interchange) give ``weights`` and ``weights_jac`` of any points, both from one
forward pass that carries the three tangents (csrc/skinning_mlp.hip on a GPU), and :func:`standard_lbs` skins points with them.
"""
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _C
from .materials import _check_floating, _neohookean_terms, _on_hip

__all__ = ['dFdz_matrix', 'get_defo_grad', 'reduced_neohookean_terms', 'SkinningModule', 'SimplicitsMLP', 'weight_function_lbs',
           'standard_lbs']


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


class SkinningModule(nn.Module):
    r"""Base class of skinning weight modules: ``forward`` maps points normalised to the bounding box, of shape :math:`(N, 3)`,
    to the weights of the learned handles, :math:`(N, H - 1)`; the methods below add the normalisation and the constant handle.

    Args:
        bb_min (torch.Tensor or array-like, optional): minimum corner of the bounding box, of shape :math:`(3,)`.
            Default: ``torch.zeros(3)``.
        bb_max (torch.Tensor or array-like, optional): maximum corner, of shape :math:`(3,)`. Default: ``torch.ones(3)``.
    """

    def __init__(self, bb_min=None, bb_max=None):
        super().__init__()
        if bb_min is None:
            bb_min = torch.zeros(3, dtype=torch.float32)
        elif not torch.is_tensor(bb_min):
            bb_min = torch.tensor(bb_min, dtype=torch.float32)
        if bb_max is None:
            bb_max = torch.ones(3, dtype=torch.float32)
        elif not torch.is_tensor(bb_max):
            bb_max = torch.tensor(bb_max, dtype=torch.float32)
        assert (bb_min < bb_max).all(), f"bb_min must be greater than bb_max, received {bb_min} and {bb_max}."
        self.register_buffer('bb_min', bb_min)
        self.register_buffer('bb_max', bb_max)

    def _offset_scale(self, pts):
        return (pts - self.bb_min.to(pts.dtype)) / (self.bb_max.to(pts.dtype) - self.bb_min.to(pts.dtype))

    def compute_skinning_weights(self, pts):
        r"""The skinning weights of ``pts`` :math:`(N, 3)`, of shape :math:`(N, H)`: the module on the normalised points and a
        trailing column of ones (the constant handle)."""
        return torch.cat([self(self._offset_scale(pts)), pts.new_ones((pts.shape[0], 1))], dim=1)

    def compute_dwdx(self, pts):
        r"""The Jacobian of the skinning weights with respect to ``pts`` :math:`(N, 3)`, of shape :math:`(N, H, 3)`, the constant
        handle's row zero: by the module's ``grad`` method on the normalised points if it has one, else by ``jacrev`` under
        ``vmap``."""
        if hasattr(self, 'grad'):
            model_grad = self.grad(self._offset_scale(pts))
            model_grad = model_grad / (self.bb_max - self.bb_min).to(model_grad.dtype)[None, None]
            return torch.cat([model_grad, model_grad.new_zeros((model_grad.shape[0], 1, model_grad.shape[2]))], dim=1)
        jac_single = torch.func.jacrev(lambda x: self.compute_skinning_weights(x[None])[0])
        return torch.vmap(jac_single)(pts)

    def compute_weights_and_dwdx(self, pts):
        r"""Both of the above, ``(weights (N, H), weights_jac (N, H, 3))``, the inputs of :func:`reduced_neohookean_terms`.  A
        :class:`SimplicitsMLP` gets them from one evaluation: the call a setup routine should make."""
        return self.compute_skinning_weights(pts), self.compute_dwdx(pts)

    @staticmethod
    def from_function(function, bb_min=0, bb_max=1):
        r"""A SkinningModule whose ``forward`` is ``function`` (normalised points :math:`(N, 3)` to :math:`(N, H - 1)`)."""
        skinning_mod = SkinningModule(bb_min=bb_min, bb_max=bb_max)
        skinning_mod.forward = types.MethodType(lambda self, pts: function(pts), skinning_mod)
        return skinning_mod


class SimplicitsMLP(SkinningModule):
    r"""The Simplicits skinning network: ``Linear(spatial_dimensions, layer_width)``, ELU, ``num_layers`` times
    (``Linear(layer_width, layer_width)``, ELU), ``Linear(layer_width, num_handles - 1)``, in ``self.linear_elu_stack``.

    The weights and their Jacobian come from one forward pass that carries the tangents :math:`T` :math:`(N, 3, W)` next to the
    values: :math:`T \leftarrow (T W^T) \cdot \operatorname{elu}'(y)`, starting from :math:`W_0 / (bb_{max} - bb_{min})`, not
    from ``jacrev``.  In torch this is differentiable in the parameters and in ``pts``, on any device and floating dtype.

    With ``spatial_dimensions == 3``, float32 parameters and ``pts`` on one GPU, ``layer_width`` a multiple of 16 in
    :math:`[16, 128]`, ``2 <= num_handles <= kaolin_amd._C.physics.max_handles()``, at least a point, and no gradient wanted
    (grad mode off, or neither ``pts`` nor a parameter requires grad), all three methods run one HIP launch
    (csrc/skinning_mlp.hip): activations stay in registers from layer to layer, no workspace, the same bits on every call.
    No autograd in HIP: the kernel gives the forward quantities of a simulation; anything that wants a gradient takes torch.

    Args:
        spatial_dimensions (int): 3, or 2 (torch only).
        layer_width (int): width of the hidden layers.
        num_handles (int): number of handles, the constant one included.
        num_layers (int): number of hidden ``Linear(layer_width, layer_width)``.
        bb_min, bb_max: as in :class:`SkinningModule`.
    """

    def __init__(self, spatial_dimensions, layer_width, num_handles, num_layers, bb_min=None, bb_max=None):
        super().__init__(bb_min=bb_min, bb_max=bb_max)
        layers = [nn.Linear(spatial_dimensions, layer_width), nn.ELU()]
        for _ in range(num_layers):
            layers += [nn.Linear(layer_width, layer_width), nn.ELU()]
        layers.append(nn.Linear(layer_width, num_handles - 1))
        self.linear_elu_stack = nn.Sequential(*layers)

    def forward(self, x):
        r"""The learned handles' weights of normalised points ``x`` :math:`(N, dim)`, of shape :math:`(N, H - 1)`."""
        return self.linear_elu_stack(x)

    def _linears(self):
        return [m for m in self.linear_elu_stack if isinstance(m, nn.Linear)]

    def _runs_hip(self, pts):
        lin = self._linears()
        W, H = lin[0].out_features, lin[-1].out_features + 1
        tensors = [pts, self.bb_min, self.bb_max] + [t for m in lin for t in (m.weight, m.bias)]
        return (lin[0].in_features == 3 and _on_hip(*tensors) and len({t.device for t in tensors}) == 1 and
                not torch._C._functorch.is_functorch_wrapped_tensor(pts) and W % 16 == 0 and 16 <= W <= 128 and
                2 <= H <= _C.physics.max_handles() and pts.shape[0] >= 1 and
                not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors)))

    def _forward_mode(self, pts):
        """The definition, in torch: values y (N, W) and tangents T (N, 3, W) through the stack"""
        lin = self._linears()
        y = F.linear(self._offset_scale(pts), lin[0].weight, lin[0].bias)
        T = (lin[0].weight / (self.bb_max - self.bb_min).to(pts.dtype)).T[None]
        for m in lin[1:]:
            T = T * torch.exp(y.clamp(max=0))[:, None, :]      # elu'(y): 1 for y > 0, exp(y) otherwise
            y, T = F.linear(F.elu(y), m.weight, m.bias), T @ m.weight.T
        N = pts.shape[0]
        return torch.cat([y, y.new_ones((N, 1))], dim=1), torch.cat([T.expand(N, -1, -1).transpose(1, 2), y.new_zeros((N, 1, 3))], dim=1)

    def compute_weights_and_dwdx(self, pts):
        if pts.dim() != 2 or pts.shape[1] != self._linears()[0].in_features:
            raise ValueError(f'pts must be of shape (N, {self._linears()[0].in_features}), got {tuple(pts.shape)}')
        if self._runs_hip(pts):
            lin = self._linears()
            return _C.physics.skinning_mlp_cuda(pts.detach().contiguous(), self.bb_min, self.bb_max,
                                                [(m.weight, m.bias) for m in lin], lin[0].out_features, len(lin) - 2,
                                                lin[-1].out_features + 1)
        return self._forward_mode(pts)

    def compute_skinning_weights(self, pts):
        if pts.dim() == 2 and pts.shape[1] == 3 and self._runs_hip(pts):
            return self.compute_weights_and_dwdx(pts)[0]
        return super().compute_skinning_weights(pts)

    def compute_dwdx(self, pts):
        return self.compute_weights_and_dwdx(pts)[1]


def weight_function_lbs(x0, tfms, fcn):
    r"""Linear blend skinning of ``x0`` :math:`(N, 3)` by a batch of transforms ``tfms`` :math:`(B, H, 3, 4)` with the weights
    ``fcn(x0)`` :math:`(N, H)`; differentiable through ``fcn``.  Returns :math:`(N, B, 1, 3)`."""
    return standard_lbs(x0, tfms, fcn(x0))


def standard_lbs(x0, tfms, w_x0):
    r"""Linear blend skinning :math:`x_i = x_{0,i} + \sum_h w_h(x_{0,i}) \, T_h \, (x_{0,i}, 1)` for every transform of a batch.

    Args:
        x0 (torch.Tensor): rest points, of shape :math:`(N, 3)`.
        tfms (torch.Tensor): delta transforms of the handles, of shape :math:`(B, H, 3, 4)`.
        w_x0 (torch.Tensor): skinning weights, of shape :math:`(N, H)`.

    Returns:
        (torch.Tensor): the transformed points, of shape :math:`(N, B, 1, 3)`.
    """
    return (x0[:, None] + torch.einsum('nh,bhij,nj->nbi', w_x0, tfms, _homogeneous(x0)))[:, :, None]
