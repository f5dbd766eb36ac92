"""``transform_gaussians`` and ``transform_shs`` (API mirror of kaolin/ops/gaussians/transforms.py): one rigid or similarity
transform for a whole splat model, or one per Gaussian, with the view-dependent colour (real SH, degrees 0..3, the 3DGS sign
convention) rotated into the new frame.

float32 / float64 CUDA tensors on one device run csrc/gaussian_transform.hip: ONE launch per direction, no host read, no atomics,
no workspace, the same bits on every call, capturable into a graph.  Inputs that are not contiguous are copied first
(``.contiguous()``).  The kernels do not build the gradient with respect to ``transform`` / ``R``: a call where that tensor requires
a gradient, and every call on CPU tensors or in half / bfloat16, runs the torch formulation below as a whole (differentiable in
everything, deterministic: D^2 and D^3 are assembled by a matrix product, not by ``scatter_add_``).

Both paths evaluate the Ivanic-Ruedenberg recurrence with its exact coefficients (generated: ``_sh_rotation_table.py``,
tools/gen_sh_rotation_table.py); the reference carries them rounded to four decimals, so its bands 2 and 3 differ from ours by up
to 2e-4 per unit coefficient.
"""
import math

import torch
from torch.autograd.function import once_differentiable

from ... import _C
from ...math import quat as quat_ops
from . import _sh_rotation_table as _table

__all__ = ['transform_gaussians', 'transform_shs']

# band 1 in the 3DGS convention (basis -y, z, -x): D^1 = R[perm][:, perm] * sign
_PERM = (1, 2, 0)
_SIGN = ((1., -1., 1.), (-1., 1., -1.), (1., -1., 1.))


# ---- the torch formulation --------------------------------------------------------------------------------------------------------
_WEIGHTS = {}


def _band_weights(l, dtype, device):
    """The term list of band l as a dense (9 (2l - 1)^2, (2l + 1)^2) matrix W: vec(D^l) = vec(D^1 (x) D^{l-1}) W"""
    key = (l, dtype, str(device))
    w = _WEIGHTS.get(key)
    if w is None:
        k, d = 2 * l - 1, 2 * l + 1
        w64 = torch.zeros(9 * k * k, d * d, dtype=torch.float64)
        for c, m, n, i, j, p, q in _table.BANDS[l]:
            w64[(i * 3 + j) * k * k + p * k + q, m * d + n] += c
        w = _WEIGHTS[key] = w64.to(device=device, dtype=dtype)
    return w


def _sh_matrices(R, degree):
    """R (n, 3, 3) -> [D^1, ..., D^degree], D^l (n, 2l + 1, 2l + 1): polynomials in the entries of R, orthogonal or not"""
    if degree == 0:
        return []
    n = R.shape[0]
    mats = [R[:, _PERM, :][:, :, _PERM] * R.new_tensor(_SIGN)]
    for l in range(2, degree + 1):
        outer = mats[0][:, :, :, None, None] * mats[-1][:, None, None, :, :]
        mats.append((outer.reshape(n, -1) @ _band_weights(l, R.dtype, R.device)).reshape(n, 2 * l + 1, 2 * l + 1))
    return mats


def _torch_transform_shs(shs_feat, R, degree):
    bands = [shs_feat[:, :1]]
    for l, D in enumerate(_sh_matrices(R, degree), start=1):
        bands.append(D @ shs_feat[:, l * l:(l + 1) * (l + 1)])
    return torch.cat(bands, dim=1)


def _torch_transform_gaussians(positions, orientations, scales, transform, sh_coeff, degree, use_log_scales, use_xyzw):
    """transform: (1 or N, 4, 4)"""
    A = transform[:, :3, :3]
    tfm_scale = torch.linalg.norm(A, dim=-2)                              # the column norms
    R = A / tfm_scale.unsqueeze(-2)
    new_positions = (A @ positions[:, :, None] + transform[:, :3, 3:]).squeeze(-1)
    unit = orientations / torch.linalg.norm(orientations, dim=-1, keepdim=True)
    if not use_xyzw:
        unit = torch.cat([unit[:, 1:], unit[:, :1]], dim=-1)
    new_orientations = quat_ops.quat_mul(quat_ops.quat_from_rot33(R), unit)
    if not use_xyzw:
        new_orientations = torch.cat([new_orientations[:, -1:], new_orientations[:, :-1]], dim=-1)
    if use_log_scales:
        new_scales = scales * (torch.log(tfm_scale) / scales + 1)
    else:
        new_scales = scales * tfm_scale
    new_sh_coeff = None if sh_coeff is None else _torch_transform_shs(sh_coeff, R, degree)
    return new_positions, new_orientations, new_scales, new_sh_coeff


# ---- the HIP path -------------------------------------------------------------------------------------------------------------------
class _TransformGaussians(torch.autograd.Function):
    """positions / orientations / scales (all three or none) and sh_coeff (or None) under `transform` ((1 or N, 4, 4), or
    (1 or N, 3, 3) with rotation_given); no gradient for `transform`"""

    @staticmethod
    def forward(ctx, positions, orientations, scales, sh_coeff, transform, use_log_scales, use_xyzw, rotation_given):
        ctx.save_for_backward(orientations, transform)
        ctx.flags = (use_log_scales, use_xyzw, rotation_given)
        ctx.has_sh = sh_coeff is not None
        ctx.set_materialize_grads(False)
        return _C.ops.gaussians.transform_gaussians_forward_cuda(positions, orientations, scales, transform, sh_coeff, use_log_scales,
                                                                use_xyzw, rotation_given)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_positions, grad_orientations, grad_scales, grad_sh):
        orientations, transform = ctx.saved_tensors
        need = list(ctx.needs_input_grad[:4])
        grads = _C.ops.gaussians.transform_gaussians_backward_cuda(
            grad_positions, grad_orientations, grad_scales, grad_sh, orientations, transform, *ctx.flags, need)
        return (*grads, None, None, None, None)


def _on_hip(transform, *tensors):
    """float32 / float64 on one GPU, and no gradient asked of the transform"""
    return (transform.is_cuda and transform.dtype in (torch.float32, torch.float64) and
            all(t.device == transform.device and t.dtype == transform.dtype for t in tensors) and
            not (torch.is_grad_enabled() and transform.requires_grad))


def _sh_degree(shs_feat):
    assert shs_feat.dim() == 3, f"sh must be of shape (N, S, 3), got sh.shape: {shs_feat.shape}"
    num_coeffs = shs_feat.shape[1]
    degree = math.isqrt(num_coeffs) - 1
    assert ((degree + 1) ** 2) == num_coeffs
    if degree > 3:
        raise NotImplementedError(f"transform_shs does not support degree > 3, got {degree}")
    assert shs_feat.shape[2] == 3, f"sh must have 3 channels, got sh.shape: {shs_feat.shape}"
    return degree


def transform_gaussians(positions, orientations, scales, transform, sh_coeff=None, use_log_scales=False, use_xyzw=False):
    r"""Apply a 4x4 affine transform to gaussian positions, orientations, and scales (reference:
    kaolin/ops/gaussians/transforms.py).  With :math:`A` the upper-left 3x3 block of the transform and :math:`t` its last column:
    positions become :math:`A p + t`; the scale of the transform is the column norms of :math:`A` and multiplies ``scales``
    (``use_log_scales``: its logarithm is added, evaluated as ``scales * (log(tfm_scale) / scales + 1)``); the rotation
    :math:`R = A / \text{tfm_scale}` (column-wise) is composed with the normalized ``orientations`` and rotates ``sh_coeff``
    (:func:`transform_shs`).

    Exact for rotation, translation and isotropic scale; under shear or anisotropic scale :math:`R` is not a rotation and the
    result is the same polynomial expression evaluated on it (applying the inverse transform does not undo it).  A zero-norm
    quaternion or a zero column of :math:`A` gives NaN / inf in that row only.

    Differentiable in ``positions``, ``orientations``, ``scales`` and ``sh_coeff`` on the HIP path (the gradient of ``scales``
    under ``use_log_scales`` is the cotangent itself: the derivative of ``scales + log(tfm_scale)``); a ``transform`` that
    requires a gradient runs the torch formulation, which is differentiable in everything.

    Args:
        positions (torch.Tensor): Splat centres of shape :math:`(N, 3)`.
        orientations (torch.Tensor):
            Quaternions, shape :math:`(N, 4)`, normalized here.
            Follow wxyz convention, or xyzw convention if ``use_xyzw`` is True.
        scales (torch.Tensor): Per-axis scale per gaussian, shape :math:`(N, 3)`.
        transform (torch.Tensor): Affine transform, shape :math:`(4, 4)`, :math:`(1, 4, 4)` or :math:`(N, 4, 4)`.
            Single transform is broadcast to all gaussians.
        sh_coeff (torch.Tensor, optional): Full SH coefficients of shape
            :math:`(N, S, 3)` where :math:`S = (sh\_degree + 1)^2`, :math:`sh\_degree \leq 3`. The band 0 (DC)
            coefficient at index 0 is rotation-invariant and passed through unchanged;
            only bands :math:`l \geq 1` are rotated. Default: None.
        use_log_scales (bool): If True, use log-based scaling for scales. Default: False.
        use_xyzw (bool): If True, use xyzw convention for quaternions. Default: False.

    Returns:
        tuple: (new_positions, new_orientations, new_scales, Optional[new_sh_coeff]) with same shapes as inputs.
    """
    assert positions.dtype == orientations.dtype == scales.dtype == transform.dtype, f"positions, orientations, scales, and transform must have the same dtype, got positions.dtype: {positions.dtype}, orientations.dtype: {orientations.dtype}, scales.dtype: {scales.dtype}, transform.dtype: {transform.dtype}"
    assert positions.device == orientations.device == scales.device == transform.device, f"positions, orientations, scales, and transform must be on the same device, got positions.device: {positions.device}, orientations.device: {orientations.device}, scales.device: {scales.device}, transform.device: {transform.device}"
    if sh_coeff is not None:
        assert sh_coeff.dtype == positions.dtype, f"sh_coeff must have the same dtype as the other inputs, got sh_coeff.dtype: {sh_coeff.dtype}, positions.dtype: {positions.dtype}"
        assert sh_coeff.device == positions.device, f"sh_coeff must be on the same device as the other inputs, got sh_coeff.device: {sh_coeff.device}, positions.device: {positions.device}"
    if len(transform.shape) == 2:  # single transform for all the gaussians
        transform = transform.unsqueeze(0)
    n = positions.shape[0]
    assert positions.shape == (n, 3), f"positions must be of shape (N, 3), got positions.shape: {positions.shape}"
    assert orientations.shape == (n, 4), f"orientations must be of shape (N, 4), got orientations.shape: {orientations.shape}"
    assert scales.shape == (n, 3), f"scales must be of shape (N, 3), got scales.shape: {scales.shape}"
    assert transform.dim() == 3 and transform.shape[0] in (1, n) and transform.shape[1:] == (4, 4), f"transform must be of shape (4, 4), (1, 4, 4) or (N, 4, 4), got transform.shape: {transform.shape}"
    degree = 0
    if sh_coeff is not None:
        degree = _sh_degree(sh_coeff)
        assert transform.shape[0] == sh_coeff.shape[0] or transform.shape[0] == 1, f"R must have the same number of batches as sh, got R.shape: {transform[:, :3, :3].shape}, sh.shape: {sh_coeff.shape}"
        assert sh_coeff.shape[0] == n, f"sh_coeff must be of shape (N, S, 3), got sh_coeff.shape: {sh_coeff.shape}"
    tensors = (positions, orientations, scales) + (() if sh_coeff is None else (sh_coeff,))
    if _on_hip(transform, *tensors):
        return _TransformGaussians.apply(positions, orientations, scales, sh_coeff, transform, bool(use_log_scales), bool(use_xyzw),
                                         False)
    return _torch_transform_gaussians(positions, orientations, scales, transform, sh_coeff, degree, use_log_scales, use_xyzw)


def transform_shs(shs_feat: torch.Tensor, R: torch.Tensor) -> torch.Tensor:
    r"""
    Rotate real SH coefficients (bands 0..3, the 3DGS sign convention) in batch (reference:
    kaolin/ops/gaussians/transforms.py). Band 0 (DC) is rotation-invariant and is passed through unchanged; band :math:`l` is
    multiplied by :math:`D^l(R)`, with :math:`D^2` and :math:`D^3` from the Ivanic-Ruedenberg recurrence with exact
    coefficients.  ``R`` is used as given: the :math:`D^l` are polynomials in its entries whether it is orthogonal or not.
    Differentiable in ``shs_feat`` on the HIP path; an ``R`` that requires a gradient runs the torch formulation.

    Args:
        shs_feat (torch.Tensor): SH coefficients for bands l=0..degree, RGB, of shape
            :math:`(N, (\text{degree}+1)^2, 3)` with the DC term at index 0.
        R (torch.Tensor): rotation matrices (SO(3)), of shape :math:`(N, 3, 3)` or :math:`(1, 3, 3)`.

    Returns:
        (torch.Tensor): rotated SH coefficients, same shape as ``shs_feat``.
    """
    assert shs_feat.dtype == R.dtype, f"sh and R must have the same dtype, got sh.dtype: {shs_feat.dtype}, R.dtype: {R.dtype}"
    assert shs_feat.device == R.device, f"sh and R must be on the same device, got sh.device: {shs_feat.device}, R.device: {R.device}"
    degree = _sh_degree(shs_feat)
    assert R.shape[0] == shs_feat.shape[0] or R.shape[0] == 1, f"R must have the same number of batches as sh, got R.shape: {R.shape}, sh.shape: {shs_feat.shape}"
    assert R.shape[1:] == (3, 3), f"R must be a rotation matrix, got R.shape: {R.shape}"
    if _on_hip(R, shs_feat):
        return _TransformGaussians.apply(None, None, None, shs_feat, R, False, False, True)[3]
    return _torch_transform_shs(shs_feat, R, degree)
