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

Training such a network (the reference's kaolin/physics/simplicits/losses.py): :func:`loss_elastic`, :func:`loss_ortho` and
:func:`compute_losses`, over :func:`training_losses`, the two losses of given ``weights`` and ``weights_jac`` as one differentiable
function.  float32 on a GPU runs csrc/simplicits_loss.hip (losses and their gradient) and, for a :class:`SimplicitsMLP` of width
at most 64, csrc/skinning_mlp_backward.hip (the network's forward that keeps its pre-activations, and its reverse pass); everything
else runs the torch definitions in this file.  A training loop is Adam around :func:`compute_losses`::

    model = SimplicitsMLP(3, 64, num_handles, 6).cuda()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    for step in range(num_steps):
        opt.zero_grad()
        le, lo = compute_losses(model, pts, yms, prs, rhos, step / num_steps, 10, appx_vol, 1000, 1e-1, 1e6)
        (le + lo).backward()
        opt.step()
"""
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import _C
from .materials import _check_floating, _cofactor, _neohookean_terms, _on_hip, to_lame

__all__ = ['dFdz_matrix', 'get_defo_grad', 'reduced_neohookean_terms', 'SkinningModule', 'SimplicitsMLP', 'weight_function_lbs',
           'standard_lbs', 'training_losses', 'loss_ortho', 'loss_elastic', 'compute_losses']


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
    These three methods have no autograd in HIP: the kernel gives the forward quantities of a simulation, and a call of theirs
    that wants a gradient takes torch.  Training has its own path: :func:`loss_elastic` and :func:`compute_losses` evaluate the
    network (``layer_width <= 64``, ``pts`` not requiring grad) and its reverse pass in csrc/skinning_mlp_backward.hip.

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

    def _trains_hip(self, pts):
        """csrc/skinning_mlp_backward.hip serves the training losses, with or without a gradient wanted"""
        lin = self._linears()
        W, H = lin[0].out_features, lin[-1].out_features + 1
        tensors = [pts] + [t for m in lin for t in (m.weight, m.bias)]
        return (lin[0].in_features == 3 and _on_hip(*tensors) and len({t.device for t in tensors}) == 1 and
                not torch._C._functorch.is_functorch_wrapped_tensor(pts) and W % 16 == 0 and 16 <= W <= 64 and
                2 <= H <= _C.physics.max_handles() and pts.dim() == 2 and pts.shape[0] >= 1 and not pts.requires_grad)

    def _forward_mode(self, pts, box=None):
        """The definition, in torch: values y (N, W) and tangents T (N, 3, W) through the stack; box: (bb_min, bb_max) to
        normalise with, the module's own by default"""
        lin = self._linears()
        if box is None:
            xn, ext = self._offset_scale(pts), (self.bb_max - self.bb_min).to(pts.dtype)
        else:
            xn, ext = (pts - box[0]) / (box[1] - box[0]), box[1] - box[0]
        y = F.linear(xn, lin[0].weight, lin[0].bias)
        T = (lin[0].weight / ext).T[None]
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


class _SkinningMLPTraining(torch.autograd.Function):
    """(weights (N, H - 1), weights_jac (N, H - 1, 3)) of a SimplicitsMLP on pts as they are, csrc/skinning_mlp_backward.hip"""

    @staticmethod
    def forward(ctx, pts, dims, *params):
        packed = torch.cat([t.detach().reshape(-1) for t in params])
        weights, weights_jac, stash = _C.physics.skinning_mlp_forward_save_cuda(pts, packed, *dims)
        ctx.save_for_backward(pts, packed, stash)
        ctx.dims, ctx.shapes = dims, [t.shape for t in params]
        return weights, weights_jac

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_weights, grad_weights_jac):
        pts, packed, stash = ctx.saved_tensors
        flat = _C.physics.skinning_mlp_backward_cuda(pts, packed, stash, grad_weights.contiguous(), grad_weights_jac.contiguous(),
                                                     *ctx.dims)
        grads = [g.view(shape) for g, shape in zip(flat.split([shape.numel() for shape in ctx.shapes]), ctx.shapes)]
        return (None, None, *grads)


def _weights_and_jac(model, pts):
    """(weights (N, H'), weights_jac (N, H', 3)) of ``model(pts)``: the learned handles of the points as they are"""
    if isinstance(model, SimplicitsMLP):
        lin = model._linears()
        if model._trains_hip(pts):
            return _SkinningMLPTraining.apply(pts.contiguous(), (lin[0].out_features, len(lin) - 2, lin[-1].out_features + 1),
                                              *(t for m in lin for t in (m.weight, m.bias)))
        weights, weights_jac = model._forward_mode(pts, box=(0.0, 1.0))
        return weights[:, :-1], weights_jac[:, :-1]
    return model(pts), torch.vmap(torch.func.jacrev(lambda x: model(x[None])[0]))(pts)


def _losses_definition(weights, weights_jac, pts, transforms, mus, lams, interp_step, scale_le, scale_lo):
    """The two training losses in torch; transforms None: the elastic one is zero"""
    Hp = weights.shape[1]
    if transforms is None:
        le = weights.new_zeros(())
    else:
        eye = torch.eye(3, dtype=weights.dtype, device=weights.device)
        defo = eye + torch.einsum('ph,bhij->pbij', weights, transforms[..., :3]) + \
            torch.einsum('bhin,pn,phj->pbij', transforms, _homogeneous(pts), weights_jac)
        mu, lam = mus[:, None], lams[:, None]
        eps = (defo + defo.transpose(-1, -2)) / 2 - eye
        lin = mu * (eps * eps).sum(dim=(-1, -2)) + lam / 2 * eps.diagonal(dim1=-2, dim2=-1).sum(dim=-1) ** 2
        J = _cofactor(defo.reshape(-1, 3, 3))[1].reshape(defo.shape[:2])
        neo = mu / 2 * ((defo * defo).sum(dim=(-1, -2)) - 3) + lam / 2 * (J - 1) ** 2 - mu * (J - 1)
        le = scale_le * ((1 - interp_step) * lin + interp_step * neo).sum()
    gram = weights.T @ weights
    return le, scale_lo * ((gram - torch.eye(Hp, dtype=weights.dtype, device=weights.device)) ** 2).mean()


class _TrainingLosses(torch.autograd.Function):
    """(le, lo) of csrc/simplicits_loss.hip; differentiable in weights and weights_jac"""

    @staticmethod
    def forward(ctx, weights, weights_jac, pts, transforms, mus, lams, interp_step, scale_le, scale_lo):
        args = (weights, weights_jac, pts, transforms, mus, lams)
        args = tuple(t if t is None else t.detach().contiguous() for t in args) + (interp_step, scale_le, scale_lo)
        le, lo, gmi = _C.physics.simplicits_loss_cuda(*args)
        ctx.save_for_backward(gmi, *(t for t in args[:6] if t is not None))
        ctx.alone, ctx.scalars = transforms is None, args[6:]
        return le, lo

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_le, grad_lo):
        gmi, weights, *rest = ctx.saved_tensors
        rest = [None] * 5 if ctx.alone else rest
        grad_w, grad_j = _C.physics.simplicits_loss_backward_cuda(weights, *rest, *ctx.scalars, gmi, grad_le.contiguous(),
                                                                  grad_lo.contiguous())
        return (grad_w, None if ctx.alone else grad_j) + (None,) * 7


def _losses(weights, weights_jac, pts, transforms, mus, lams, interp_step, scale_le, scale_lo):
    """Dispatch of the two losses; transforms None: the orthogonality loss alone"""
    tensors = [weights] if transforms is None else [weights, weights_jac, pts, transforms, mus, lams]
    if (_on_hip(*tensors) and len({t.device for t in tensors}) == 1 and weights.shape[0] >= 1 and
            1 <= weights.shape[1] <= _C.physics.max_handles() - 1 and (transforms is None or transforms.shape[0] >= 1) and
            not any(t.requires_grad for t in tensors[2:]) and
            not any(torch._C._functorch.is_functorch_wrapped_tensor(t) for t in tensors)):
        return _TrainingLosses.apply(weights, weights_jac, pts, transforms, mus, lams, float(interp_step), float(scale_le),
                                     float(scale_lo))
    return _losses_definition(weights, weights_jac, pts, transforms, mus, lams, interp_step, scale_le, scale_lo)


def training_losses(weights, weights_jac, pts, transforms, mus, lams, interp_step, scale_le=1.0, scale_lo=1.0):
    r"""The elastic and the orthogonality loss of Simplicits training as one function of the skinning weights:

    .. math::
        le = \text{scale_le} \sum_{p, b} \left[ (1 - s) \Psi_{lin}(F_{pb}) + s \Psi_{neo}(F_{pb}) \right], \quad
        lo = \text{scale_lo} \operatorname{mean}\left( (W^T W - I)^2 \right)

    with :math:`F_{pb} = I + \sum_h ( w_{ph} T_{bh}[:, :3] + (T_{bh} \tilde x_p) \otimes \nabla w_{ph} )`,
    :math:`\Psi_{lin} = \mu \|\epsilon\|^2 + \tfrac{\lambda}{2} \operatorname{tr}(\epsilon)^2`,
    :math:`\epsilon = (F + F^T) / 2 - I`, and :math:`\Psi_{neo}` the Neo-Hookean energy of
    :mod:`kaolin_amd.physics.materials` (determinant from 2x2 minors: finite for an inverted :math:`F`).

    float32 tensors on one GPU with at most ``kaolin_amd._C.physics.max_handles() - 1`` weights a point run
    csrc/simplicits_loss.hip, forward and backward: differentiable in ``weights`` and ``weights_jac`` (once), sums in one fixed
    order, the same bits on every call.  Everything else, and a gradient wanted in any other argument, runs torch.

    Args:
        weights (torch.Tensor): skinning weights, of shape :math:`(N, H')`.
        weights_jac (torch.Tensor): their spatial gradients, of shape :math:`(N, H', 3)`.
        pts (torch.Tensor): the points, of shape :math:`(N, 3)`.
        transforms (torch.Tensor): sample transforms of the handles, of shape :math:`(B, H', 3, 4)`.
        mus, lams (torch.Tensor): Lame coefficients per point, each of shape :math:`(N,)`.
        interp_step (float): :math:`s`, from 0 (linear elasticity) to 1 (Neo-Hookean).
        scale_le, scale_lo (float): scale the two losses.

    Returns:
        (torch.Tensor, torch.Tensor): ``le`` and ``lo``, scalars.
    """
    N, Hp = _check_skinning(weights, weights_jac, pts, mus=mus, lams=lams)
    _check_floating(weights=weights, transforms=transforms)
    if transforms.dim() != 4 or tuple(transforms.shape[1:]) != (Hp, 3, 4):
        raise ValueError(f'transforms must be of shape (B, {Hp}, 3, 4), got {tuple(transforms.shape)}')
    return _losses(weights, weights_jac, pts, transforms, mus, lams, interp_step, scale_le, scale_lo)


def loss_ortho(weights):
    r"""The orthogonality loss of skinning weights, :math:`\operatorname{mean}((W^T W - I)^2)`.

    Args:
        weights (torch.Tensor): of shape :math:`(N, H')`.

    Returns:
        (torch.Tensor): a scalar; differentiable in ``weights`` (csrc/simplicits_loss.hip for float32 on a GPU).
    """
    _check_floating(weights=weights)
    if weights.dim() != 2:
        raise ValueError(f'weights must be of shape (N, H), got {tuple(weights.shape)}')
    return _losses(weights, None, None, None, None, None, 0.0, 0.0, 1.0)[1]


def _materials(yms, prs, interp_step, interp_material):
    mus, lams = to_lame(yms.reshape(-1), prs.reshape(-1))
    if interp_material:
        mus = (1 - interp_step) * mus.min() + interp_step * mus
        lams = (1 - interp_step) * lams.min() + interp_step * lams
    return mus, lams


def loss_elastic(model, pts, yms, prs, rhos, transforms, appx_vol, interp_step, elasticity_type="neohookean", interp_material=False):
    r"""The elastic loss of Simplicits training: the energy of the points skinned by ``model`` under sample transforms,
    :math:`\tfrac{\text{appx_vol}}{N} \sum_{p, b} [(1 - s) \Psi_{lin}(F_{pb}) + s \Psi_{neo}(F_{pb})]` (see
    :func:`training_losses`), ramping from linear to Neo-Hookean elasticity with ``interp_step``.

    ``model`` is applied to ``pts`` as they are: ``model(pts)`` gives the :math:`H'` learned weights, without bounding-box
    normalisation and without the constant handle, as in the reference's training.  One difference from the reference is
    deliberate: there :math:`F` comes from central finite differences of :func:`weight_function_lbs` with step
    :math:`\sqrt{10^{-7}}` in float32; here it is the closed form above with the model's own Jacobian.

    A float32 :class:`SimplicitsMLP` on a GPU (``layer_width`` a multiple of 16 up to 64, ``pts`` not requiring grad) is evaluated
    and differentiated by csrc/skinning_mlp_backward.hip; another :class:`SimplicitsMLP` by its torch forward mode, any other
    :class:`SkinningModule` by ``jacrev`` under ``vmap``.  Differentiable in the model's parameters.

    Args:
        model (SkinningModule): the skinning module.
        pts (torch.Tensor): sample points, of shape :math:`(N, 3)`.
        yms, prs, rhos (torch.Tensor): Young's moduli, Poisson ratios and densities per point, of shape :math:`(N,)` or
            :math:`(N, 1)`; ``rhos`` is not used.
        transforms (torch.Tensor): sample transforms, of shape :math:`(B, H', 3, 4)`.
        appx_vol (float): the object's volume.
        interp_step (float): :math:`s` in :math:`[0, 1]`.
        elasticity_type (str): ``"neohookean"``; anything else raises ``ValueError``.
        interp_material (bool): blend :math:`\mu, \lambda` from their minima to their values with ``interp_step``.

    Returns:
        (torch.Tensor): a scalar.
    """
    if elasticity_type != "neohookean":
        raise ValueError(f"Elasticity type {elasticity_type} not supported")
    mus, lams = _materials(yms, prs, interp_step, interp_material)
    weights, weights_jac = _weights_and_jac(model, pts)
    return training_losses(weights, weights_jac, pts, transforms, mus, lams, interp_step, appx_vol / pts.shape[0], 0.0)[0]


def compute_losses(skinning_mod, normalized_pts, yms, prs, rhos, en_interp, batch_size, appx_vol, num_samples, le_coeff, lo_coeff):
    r"""One step of Simplicits training: draws ``num_samples`` points (``torch.randint`` on the points' device) and ``batch_size``
    transforms (``0.1 * torch.randn(batch_size, H', 3, 4)``), as the reference does, and returns
    ``(le_coeff * loss_elastic, lo_coeff * loss_ortho)`` of them.  The network is evaluated once and both losses come from one
    call of :func:`training_losses`; see :func:`loss_elastic` for the one difference from the reference.

    Args:
        skinning_mod (SkinningModule): the skinning module.
        normalized_pts (torch.Tensor): the points, of shape :math:`(M, 3)`.
        yms, prs, rhos (torch.Tensor): Young's moduli, Poisson ratios and densities per point, of shape :math:`(M,)`.
        en_interp (float): the interpolation between the energies at this step.
        batch_size (int): number of sample transforms.
        appx_vol (float): the object's volume.
        num_samples (int): number of sample points.
        le_coeff, lo_coeff (float): coefficients of the two losses.

    Returns:
        (torch.Tensor, torch.Tensor): the elastic and the orthogonality term, scalars.
    """
    sample_indices = torch.randint(low=0, high=normalized_pts.shape[0], size=(num_samples,), device=normalized_pts.device)
    sample_pts = normalized_pts[sample_indices]
    mus, lams = _materials(yms[sample_indices], prs[sample_indices], en_interp, False)
    weights, weights_jac = _weights_and_jac(skinning_mod, sample_pts)
    batch_transforms = 0.1 * torch.randn(batch_size, weights.shape[-1], 3, 4, dtype=normalized_pts.dtype).to(normalized_pts.device)
    le, lo = training_losses(weights, weights_jac, sample_pts, batch_transforms, mus, lams, en_interp, appx_vol / num_samples, 1.0)
    return le_coeff * le, lo_coeff * lo
