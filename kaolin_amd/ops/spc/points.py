"""``kaolin.ops.spc`` points: quantisation, Morton codes, corners, the octree of a point set and trilinear interpolation of corner
features (reference: kaolin/ops/spc/points.py).  CUDA tensors run the HIP kernels of csrc/spc.hip and csrc/spc_trilinear.hip
through ``_C.ops.spc``; CPU tensors (which the reference rejects) run the ``_torch_*`` formulations of the same pipelines below --
also the yardstick of tools/time_spc.py and tools/time_spc_trilinear.py."""
import warnings

import torch

from ... import _C

__all__ = ['points_to_morton', 'morton_to_points', 'points_to_corners', 'unbatched_points_to_octree', 'quantize_points',
           'create_dense_spc', 'coords_to_trilinear_coeffs', 'coords_to_trilinear', 'unbatched_interpolate_trilinear']

_COORD_BITS = 15        # KAOLIN_SPC_MAX_LEVELS: bits of a coordinate in a Morton code


def quantize_points(x, level):
    """Float coordinates in [-1, 1] (last dimension 3) -> int16 coordinates in [0, 2^level - 1]; points outside are clipped."""
    res = 2 ** level
    return torch.floor(torch.clamp(res * (x + 1.0) / 2.0, 0, res - 1.)).short()


def _torch_points_to_morton(points):
    p = points.long()
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    code = torch.zeros_like(x)
    for i in range(_COORD_BITS):
        code |= ((z >> i) & 1) << (3 * i)
        code |= ((y >> i) & 1) << (3 * i + 1)
        code |= ((x >> i) & 1) << (3 * i + 2)
    return code


def _torch_morton_to_points(morton):
    x, y, z = torch.zeros_like(morton), torch.zeros_like(morton), torch.zeros_like(morton)
    for i in range(_COORD_BITS):
        z |= ((morton >> (3 * i)) & 1) << i
        y |= ((morton >> (3 * i + 1)) & 1) << i
        x |= ((morton >> (3 * i + 2)) & 1) << i
    return torch.stack([x, y, z], dim=-1).short()


def _torch_morton_to_octree(morton, level):
    """Morton codes (N), any order, duplicates allowed -> octree bytes, levels root first: unique codes, then per level the
    unique parents and the OR of their children's bits."""
    cur = torch.unique(morton & ((1 << (3 * level)) - 1))
    levels = []
    for _ in range(level):
        parents, inverse = torch.unique(cur >> 3, return_inverse=True)
        byte = torch.zeros(parents.numel(), dtype=torch.long, device=morton.device)
        byte.scatter_add_(0, inverse, torch.bitwise_left_shift(torch.ones_like(cur), cur & 7))     # children are distinct: + is |
        levels.append(byte.byte())
        cur = parents
    return torch.cat(levels[::-1]) if levels else torch.empty(0, dtype=torch.uint8, device=morton.device)


def points_to_morton(points):
    """Quantised points (..., 3) int16 -> Morton codes (...) int64: bit 3i = z_i, 3i + 1 = y_i, 3i + 2 = x_i."""
    shape = list(points.shape)[:-1]
    points = points.reshape(-1, 3)
    if points.is_cuda:
        return _C.ops.spc.points_to_morton_cuda(points.contiguous()).reshape(*shape)
    return _torch_points_to_morton(points).reshape(*shape)


def morton_to_points(morton):
    """Morton codes (...) int64 -> quantised points (..., 3) int16."""
    shape = list(morton.shape) + [3]
    morton = morton.reshape(-1)
    if morton.is_cuda:
        return _C.ops.spc.morton_to_points_cuda(morton.contiguous()).reshape(*shape)
    return _torch_morton_to_points(morton).reshape(*shape)


_CORNERS = ((0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1))


def _torch_points_to_corners(points):
    return points.unsqueeze(-2) + torch.tensor(_CORNERS, dtype=points.dtype, device=points.device)


def points_to_corners(points):
    """Quantised points (..., 3) int16 -> the 8 corners of their cells (..., 8, 3), corner j = point + (j >> 2, (j >> 1) & 1, j & 1)."""
    shape = list(points.shape)
    shape.insert(-1, 8)
    if points.is_cuda:
        return _C.ops.spc.points_to_corners_cuda(points.reshape(-1, 3).contiguous()).reshape(*shape)
    return _torch_points_to_corners(points)


def unbatched_points_to_octree(points, level, sorted=False):
    """Quantised points (N, 3) int16 of ``level`` -> octree (num_bytes) uint8, levels root first.

    ``sorted=False``: any order, duplicates allowed (on the GPU: Morton codes, a radix sort over their 3 * level bits, unique, then
    every level bottom-up on the device; one host read of the level sizes).  ``sorted=True`` promises unique points in Morton
    order and skips the sort; the result for any other input is unspecified.  ``N = 0`` raises ValueError (the reference reads
    out of bounds); ``level = 0`` returns an empty tensor."""
    if points.dim() != 2 or points.size(1) != 3 or points.dtype != torch.int16:
        raise ValueError(f'unbatched_points_to_octree: points must be short, of size (num_points, 3), got {points.dtype} '
                         f'{tuple(points.shape)}')
    if points.size(0) == 0:
        raise ValueError('unbatched_points_to_octree: no points (an octree has at least its root)')
    level = int(level)
    if not 0 <= level <= _COORD_BITS:
        raise ValueError(f'unbatched_points_to_octree: level must be in [0, {_COORD_BITS}], got {level}')
    if level == 0:
        return torch.empty(0, dtype=torch.uint8, device=points.device)
    if points.is_cuda:
        return _C.ops.spc.points_to_octree(points.contiguous(), level, sorted=bool(sorted))
    return _torch_morton_to_octree(_torch_points_to_morton(points), level)


def create_dense_spc(level, device):
    """-> (octree, lengths) of the full octree of ``level``: every byte 255, sum of 8^l for l < level bytes; lengths (1) int32 CPU."""
    lengths = torch.tensor([sum(8 ** l for l in range(level))], dtype=torch.int32)
    octree = torch.full((int(lengths[0]),), 255, device=device, dtype=torch.uint8)
    return octree, lengths


# ---- trilinear interpolation ---------------------------------------------------------------------------------------------------------
def _torch_local(coords, points, level):
    """(u, 1 - u), u = 2^level (c / 2 + 1 / 2) - p: in double, rounded to float -- 1 - u from the ROUNDED u, in double, rounded to
    float.  Double coordinates keep both in double."""
    work = torch.float64 if coords.dtype == torch.float64 else torch.float32
    u = ((2 ** level) * (coords.double() * 0.5 + 0.5) - points.double()).to(work)
    return u, (1.0 - u.double()).to(work)


def _torch_coeffs(u, v):
    """c000, c001, ..., c111 (z fastest): products in the order (x y) z"""
    x, y, z = (v[..., 0], u[..., 0]), (v[..., 1], u[..., 1]), (v[..., 2], u[..., 2])
    return torch.stack([(x[k >> 2] * y[(k >> 1) & 1]) * z[k & 1] for k in range(8)], dim=-1)


def _torch_coords_to_trilinear_coeffs(coords, points, level):
    u, v = _torch_local(coords, points, level)
    return _torch_coeffs(u, v).to(coords.dtype)


def coords_to_trilinear_coeffs(coords, points, level):
    """The trilinear coefficients of coordinates in their cells: coords (..., 3) half / float / double in [-1, 1], points int16, the
    cells of ``level`` that hold them (reshaped to the same count) -> (..., 8) in coords' dtype, in the order c000, c001, ...,
    c111 -- z fastest, the corner order of ``points_to_corners``: ``(feats[trinkets] * coeffs[..., None]).sum(-2)`` interpolates.

    The local coordinate ``u = 2^level (c / 2 + 1 / 2) - p`` is evaluated in double; half and float coordinates then take the
    float arithmetic of ``unbatched_interpolate_trilinear``, double coordinates stay in double.  CUDA tensors run one HIP launch
    (not differentiable, as in the reference); CPU tensors run the torch formulation, which autograd differentiates."""
    shape = list(coords.shape)
    shape[-1] = 8
    points = points.reshape(-1, 3)
    coords = coords.reshape(-1, 3)
    if points.size(0) != coords.size(0) or points.dtype != torch.int16:
        raise ValueError(f'coords_to_trilinear_coeffs: points must be short and hold one point per coordinate, got {points.dtype} '
                         f'{tuple(points.shape)} for {coords.size(0)} coordinates')
    if coords.is_cuda:
        return _C.ops.spc.coords_to_trilinear_cuda(coords.contiguous(), points.contiguous(), level).reshape(*shape)
    return _torch_coords_to_trilinear_coeffs(coords, points, level).reshape(*shape)


def coords_to_trilinear(coords, points, level):
    """Deprecated alias of :func:`coords_to_trilinear_coeffs`."""
    warnings.warn('coords_to_trilinear is deprecated, please use kaolin.ops.spc.coords_to_trilinear_coeffs instead',
                  DeprecationWarning, stacklevel=2)
    return coords_to_trilinear_coeffs(coords, points, level)


def _torch_voxels(coords, pidx, point_hierarchy, trinkets, num_feats):
    """(hit (N) bool, points (N, 1, 3), trinkets (N, 8) long) with every index of a miss replaced by 0.  A pidx outside
    [0, num_points) or a trinket outside [0, num_feats) is a miss."""
    pi = pidx.long()
    hit = (pi >= 0) & (pi < point_hierarchy.size(0))
    pi = torch.where(hit, pi, 0)
    if point_hierarchy.size(0) == 0:
        return hit, point_hierarchy.new_zeros((pidx.size(0), 1, 3)), torch.zeros((pidx.size(0), 8), dtype=torch.long, device=pidx.device)
    tr = trinkets[pi].long()
    hit = hit & ((tr >= 0) & (tr < num_feats)).all(dim=1)
    return hit, point_hierarchy[pi][:, None, :], torch.where(hit[:, None], tr, 0)


def _acc_dtype(feats):
    return torch.float64 if feats.dtype == torch.float64 else torch.float32


def _torch_interpolate_forward(coords, pidx, point_hierarchy, trinkets, feats, level):
    """The arithmetic of the HIP kernel, operation by operation: float coefficients, the 8 products feat * coeff added in corner
    order in float (double for double features), one rounding to feats' dtype; zeros for a miss."""
    N, S, D = coords.size(0), coords.size(1), feats.size(1)
    if N == 0 or feats.size(0) == 0:
        return feats.new_zeros((N, S, D))
    hit, points, tr = _torch_voxels(coords, pidx, point_hierarchy, trinkets, feats.size(0))
    acc = _acc_dtype(feats) if coords.dtype != torch.float64 else torch.float64
    c = _torch_coeffs(*_torch_local(coords, points, level)).to(acc)                      # (N, S, 8)
    out = None
    for k in range(8):
        prod = feats[tr[:, k]].to(acc)[:, None, :] * c[:, :, k, None]                    # (N, S, D)
        out = prod if out is None else out + prod
    return torch.where(hit[:, None, None], out, 0).to(feats.dtype)


def _torch_interpolate_backward_feats(coords, pidx, point_hierarchy, trinkets, feats, level, grad_output):
    """grad_feats[trinket_k] += coeff_k * grad_output, summed over the samples of a voxel first; float sums for half features"""
    acc = _acc_dtype(feats) if coords.dtype != torch.float64 else torch.float64
    grad = torch.zeros(feats.shape, dtype=acc, device=feats.device)
    if coords.size(0) == 0 or feats.size(0) == 0:
        return grad.to(feats.dtype)
    hit, points, tr = _torch_voxels(coords, pidx, point_hierarchy, trinkets, feats.size(0))
    c = _torch_coeffs(*_torch_local(coords, points, level)).to(acc)
    per_corner = (c[..., None] * grad_output.to(acc)[:, :, None, :]).sum(dim=1)          # (N, 8, D)
    per_corner = torch.where(hit[:, None, None], per_corner, 0)
    grad.index_add_(0, tr.reshape(-1), per_corner.reshape(-1, feats.size(1)))
    return grad.to(feats.dtype)


def _torch_interpolate_backward_coords(coords, pidx, point_hierarchy, trinkets, feats, level, grad_output):
    """sum_d grad_output[d] * sum_k feats[trinket_k, d] * d coeff_k / d u: the derivative by the LOCAL coordinate u"""
    N, S = coords.size(0), coords.size(1)
    if N == 0 or feats.size(0) == 0:
        return torch.zeros_like(coords)
    acc = _acc_dtype(feats) if coords.dtype != torch.float64 else torch.float64
    hit, points, tr = _torch_voxels(coords, pidx, point_hierarchy, trinkets, feats.size(0))
    u, v = _torch_local(coords, points, level)
    u, v = u.to(acc), v.to(acc)
    f = feats[tr].to(acc)                                                                # (N, 8, D)
    w = torch.einsum('nkd,nsd->nsk', f, grad_output.to(acc))                             # (N, S, 8): sum_d g_d f_kd
    x, y, z = (v[..., 0], u[..., 0]), (v[..., 1], u[..., 1]), (v[..., 2], u[..., 2])
    sign = (-1.0, 1.0)
    gx = sum(w[..., k] * (sign[k >> 2] * y[(k >> 1) & 1] * z[k & 1]) for k in range(8))
    gy = sum(w[..., k] * (sign[(k >> 1) & 1] * x[k >> 2] * z[k & 1]) for k in range(8))
    gz = sum(w[..., k] * (sign[k & 1] * x[k >> 2] * y[(k >> 1) & 1]) for k in range(8))
    grad = torch.stack([gx, gy, gz], dim=-1)
    return torch.where(hit[:, None, None], grad, 0).to(coords.dtype)


class _InterpolateTrilinear(torch.autograd.Function):
    """forward and both backward passes: the HIP kernels for CUDA tensors, the torch formulations above for CPU tensors"""

    @staticmethod
    def forward(ctx, coords, pidx, point_hierarchy, trinkets, feats, level):
        coords, pidx, point_hierarchy = coords.contiguous(), pidx.contiguous(), point_hierarchy.contiguous()
        trinkets, feats = trinkets.contiguous(), feats.contiguous()
        ctx.save_for_backward(coords, pidx, point_hierarchy, trinkets, feats)
        ctx.level = level
        if coords.is_cuda:
            return _C.ops.spc.interpolate_trilinear_cuda(coords, pidx, point_hierarchy, trinkets, feats, level)
        return _torch_interpolate_forward(coords, pidx, point_hierarchy, trinkets, feats, level)

    @staticmethod
    def backward(ctx, grad_output):
        args = ctx.saved_tensors + (ctx.level, grad_output.contiguous())
        cuda = grad_output.is_cuda
        grad_coords = grad_feats = None
        if ctx.needs_input_grad[0]:
            op = _C.ops.spc.interpolate_trilinear_backward_coords_cuda if cuda else _torch_interpolate_backward_coords
            grad_coords = op(*args)
        if ctx.needs_input_grad[4]:
            op = _C.ops.spc.interpolate_trilinear_backward_feats_cuda if cuda else _torch_interpolate_backward_feats
            grad_feats = op(*args)
        return grad_coords, None, None, None, grad_feats, None


def unbatched_interpolate_trilinear(coords, pidx, point_hierarchy, trinkets, feats, level):
    """Trilinear interpolation of features stored on the corners of the cells of ONE octree.

    coords (N, S, 3) float32 in [-1, 1]: S samples inside each of N cells; pidx (N) int32: the index of each cell in
    ``point_hierarchy`` (``unbatched_raytrace`` returns it in this form, ``unbatched_query(...).int()`` too), -1 for a miss;
    point_hierarchy (num_points, 3) int16; trinkets (num_points, 8) int32 of ``unbatched_make_trinkets``; feats (num_feats, D) half /
    float / double, one row per dual point of ``level``; level: the level of the cells.  -> (N, S, D) in feats' dtype; the rows of
    a miss are zero.  A ``pidx`` outside [-1, num_points) or a cell with a trinket outside [0, num_feats) -- a stale pair of
    tensors -- is a miss too: zeros, zero gradients, no access.

    Arithmetic: the local coordinate ``u = 2^level (c / 2 + 1 / 2) - p`` and ``1 - u`` in double, rounded to float; float
    coefficients ``(x y) z``; the 8 products feat * coeff added in corner order, in float for half and float features and in
    double for double features; one rounding.

    Differentiable in ``feats`` and ``coords``; each gradient is computed only when asked for.  On the GPU all three passes are HIP
    kernels with lanes along D.  The gradient by ``feats`` sums the samples of a cell in registers and adds with float atomics
    (double for double features; half accumulates in float32 and is rounded once): IT MAY DIFFER IN THE LAST BITS FROM RUN TO RUN.
    The gradient by ``coords`` keeps THE REFERENCE'S CONVENTION: it is the derivative by the LOCAL cell coordinate u, WITHOUT the
    factor ``2^(level - 1)`` that the derivative by ``coords`` itself would carry; misses get zero.  Any S works (the reference's
    formulation needs S = 1).  CPU tensors run the torch formulation of the same arithmetic (and also take float64 coords, all in
    double, for gradient checks)."""
    if coords.dim() != 3 or coords.size(2) != 3 or coords.size(1) < 1 or coords.dtype not in (torch.float32, torch.float64):
        raise ValueError(f'unbatched_interpolate_trilinear: coords must be float, of size (num_voxels, num_samples, 3), got '
                         f'{coords.dtype} {tuple(coords.shape)}')
    if coords.is_cuda and coords.dtype != torch.float32:
        raise ValueError('unbatched_interpolate_trilinear: coords on a CUDA device must be float32 (float64 coords are taken on '
                         'CPU tensors only, for gradient checks)')
    if pidx.dim() != 1 or pidx.size(0) != coords.size(0) or pidx.dtype != torch.int32:
        raise ValueError(f'unbatched_interpolate_trilinear: pidx must be int, of size (num_voxels), got {pidx.dtype} '
                         f'{tuple(pidx.shape)}; unbatched_query returns int64: pass pidx.int()')
    if trinkets.dim() != 2 or trinkets.size(1) != 8 or trinkets.size(0) != point_hierarchy.size(0) or trinkets.dtype != torch.int32:
        raise ValueError(f'unbatched_interpolate_trilinear: trinkets must be int, of size (num_points, 8), got {trinkets.dtype} '
                         f'{tuple(trinkets.shape)} for {point_hierarchy.size(0)} points')
    if feats.dim() != 2 or feats.size(1) < 1 or feats.dtype not in (torch.float16, torch.float32, torch.float64):
        raise ValueError(f'unbatched_interpolate_trilinear: feats must be half, float or double, of size (num_feats, feature_dim), '
                         f'got {feats.dtype} {tuple(feats.shape)}')
    level = int(level)
    if not 0 <= level <= _COORD_BITS:
        raise ValueError(f'unbatched_interpolate_trilinear: level must be in [0, {_COORD_BITS}], got {level}')
    return _InterpolateTrilinear.apply(coords, pidx, point_hierarchy, trinkets, feats, level)
