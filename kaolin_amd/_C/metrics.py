"""Host shims for ``kaolin._C.metrics`` (bindings.cpp:103-108)."""
import os

import torch

from .. import _lib
from .._checks import (Arg, check_same_gpu, check_all_same_gpu, check_all_contiguous, check_same_type,
                       check_size, check_same_size, torch_check)

_SD_TYPES = ('f32', 'f64', 'f16', 'u8', 'i16', 'i32', 'i64')   # the reference's DISPATCH_NUM_TYPES (utils.h:50-64)


def sided_distance_forward_cuda(p1, p2):
    """reference: kaolin/csrc/metrics/sided_distance.cpp:65-89 -> [dist, idx]"""
    fn = 'sided_distance_forward_cuda'
    p1_arg, p2_arg = Arg(p1, 'p1', 1), Arg(p2, 'p2', 2)
    check_same_gpu(fn, p1_arg, p2_arg)
    check_all_contiguous(fn, [p1_arg, p2_arg])
    check_same_type(fn, p1_arg, p2_arg)
    batch_size, num_p1, num_p2 = p1.size(0), p1.size(1), p2.size(1)
    check_size(fn, p1_arg, [batch_size, num_p1, 3])
    check_size(fn, p2_arg, [batch_size, num_p2, 3])
    sfx = _lib.dtype_suffix(p1.dtype, fn, _SD_TYPES)
    lib = _lib.load()
    with _lib.on_device(p1.device):
        # the reference allocates zeros (sided_distance.cpp:80-81); every kernel path writes all B x N entries, so only
        # the degenerate "no target" case (nothing is launched) needs them
        alloc = torch.zeros if num_p2 == 0 else torch.empty
        dist = alloc((batch_size, num_p1), dtype=p1.dtype, device=p1.device)
        idx = alloc((batch_size, num_p1), dtype=torch.long, device=p1.device)
        ws = _lib.workspace(
            lib.kamd_sided_distance_forward_workspace(batch_size, num_p1, num_p2, p1.element_size()), p1.device)
        st = getattr(lib, f'kamd_sided_distance_forward_{sfx}')(
            _lib.stream_ptr(p1.device), batch_size, num_p1, num_p2,
            _lib.ptr(p1), _lib.ptr(p2), _lib.ptr(dist), _lib.ptr(idx), _lib.ptr(ws))
    _lib.check(st, fn)
    return [dist, idx]


def sided_distance_pair_forward(p1, p2):
    """Both directions of a chamfer distance from one binning pass over both clouds -> [dist1, idx1, dist2, idx2], or ``None`` when the
    shapes do not qualify (the caller then issues two ``sided_distance_forward_cuda``).  Not part of the reference's
    ``kaolin._C``: it fuses the two calls kaolin/metrics/pointcloud.py:89-136 makes; results are bit-identical."""
    fn = 'sided_distance_forward_cuda'   # argument errors read as the reference's (its chamfer_distance fails in this operator)
    p1_arg, p2_arg = Arg(p1, 'p1', 1), Arg(p2, 'p2', 2)
    check_same_gpu(fn, p1_arg, p2_arg)
    check_all_contiguous(fn, [p1_arg, p2_arg])
    check_same_type(fn, p1_arg, p2_arg)
    batch_size, num_p1, num_p2 = p1.size(0), p1.size(1), p2.size(1)
    check_size(fn, p1_arg, [batch_size, num_p1, 3])
    check_size(fn, p2_arg, [batch_size, num_p2, 3])
    if p1.dtype not in (torch.float32, torch.float64):
        return None
    lib = _lib.load()
    nbytes = lib.kamd_sided_distance_pair_forward_workspace(batch_size, num_p1, num_p2, p1.element_size())
    if nbytes == 0:
        return None
    with _lib.on_device(p1.device):
        dist1 = torch.empty((batch_size, num_p1), dtype=p1.dtype, device=p1.device)
        idx1 = torch.empty((batch_size, num_p1), dtype=torch.long, device=p1.device)
        dist2 = torch.empty((batch_size, num_p2), dtype=p1.dtype, device=p1.device)
        idx2 = torch.empty((batch_size, num_p2), dtype=torch.long, device=p1.device)
        ws = _lib.workspace(nbytes, p1.device)
        run = lib.kamd_sided_distance_pair_forward_f32 if p1.dtype == torch.float32 else lib.kamd_sided_distance_pair_forward_f64
        st = run(
            _lib.stream_ptr(p1.device), batch_size, num_p1, num_p2, _lib.ptr(p1), _lib.ptr(p2),
            _lib.ptr(dist1), _lib.ptr(idx1), _lib.ptr(dist2), _lib.ptr(idx2), _lib.ptr(ws))
    _lib.check(st, fn)
    return [dist1, idx1, dist2, idx2]


_CHAMFER_WS = {}      # (B, N, M, with_grad) -> workspace bytes (0: the shapes do not qualify)


def chamfer_distance_forward(p1, p2, w1, w2, squared, with_grad):
    """``chamfer_distance`` (kaolin/metrics/pointcloud.py:89-136) of two fp32 clouds as one operator -> (value (B), state) or
    ``None`` when the shapes do not qualify for the shared-grid search (the caller then composes it from
    ``sided_distance_forward_cuda``).  ``state`` is the workspace holding the gradient pieces for
    :func:`chamfer_distance_backward_fused` (``with_grad``).  Not part of the reference's ``kaolin._C``.
    This is a hot host path (the 100k x 100k training step is host-bound): shape checks inline, sizes cached."""
    fn = 'sided_distance_forward_cuda'   # argument errors read as the reference's (its chamfer_distance fails in this operator)
    batch_size, num_p1, num_p2 = p1.size(0), p1.size(1), p2.size(1)
    if not (p1.is_cuda and p2.is_cuda and p1.device == p2.device and p1.is_contiguous() and p2.is_contiguous() and
            p1.dtype == p2.dtype and p1.shape == (batch_size, num_p1, 3) and p2.shape == (batch_size, num_p2, 3)):
        p1_arg, p2_arg = Arg(p1, 'p1', 1), Arg(p2, 'p2', 2)      # raises the reference's message for what is wrong
        check_same_gpu(fn, p1_arg, p2_arg)
        check_all_contiguous(fn, [p1_arg, p2_arg])
        check_same_type(fn, p1_arg, p2_arg)
        check_size(fn, p1_arg, [batch_size, num_p1, 3])
        check_size(fn, p2_arg, [batch_size, num_p2, 3])
    if p1.dtype != torch.float32:
        return None
    lib = _lib.load()
    # (the library's choice of search also depends on a measurement knob read from the environment)
    key = (batch_size, num_p1, num_p2, bool(with_grad), os.environ.get('KAMD_SIDED_DISTANCE'))
    nbytes = _CHAMFER_WS.get(key)
    if nbytes is None:
        nbytes = lib.kamd_chamfer_distance_forward_workspace(batch_size, num_p1, num_p2, 1 if with_grad else 0)
        if len(_CHAMFER_WS) > 64:
            _CHAMFER_WS.clear()
        _CHAMFER_WS[key] = nbytes
    if nbytes == 0:
        return None
    device = p1.device
    with _lib.on_device(device):
        out = torch.empty((batch_size,), dtype=torch.float32, device=device)
        ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=device)
        st = lib.kamd_chamfer_distance_forward_f32(
            _lib.stream_ptr(device), batch_size, num_p1, num_p2, p1.data_ptr(), p2.data_ptr(), float(w1),
            float(w2), 1 if squared else 0, 1 if with_grad else 0, out.data_ptr(), None, None, None, None, ws.data_ptr())
    if st != 0:
        _lib.check(st, 'chamfer_distance_forward')
    return out, ws


def chamfer_distance_backward_fused(grad_output, state, batch_size, num_p1, num_p2):
    """-> [grad_p1 (B, N, 3), grad_p2 (B, M, 3)] from the state of a ``with_grad`` :func:`chamfer_distance_forward`."""
    fn = 'chamfer_distance_backward'
    if not (grad_output.is_cuda and grad_output.dtype == torch.float32 and grad_output.numel() == batch_size):
        torch_check(False, f'{fn}: grad_output must be a Float CUDA tensor of size {{batch_size}}')
    device = state.device
    lib = _lib.load()
    with _lib.on_device(device):
        g1 = torch.empty((batch_size, num_p1, 3), dtype=torch.float32, device=device)
        g2 = torch.empty((batch_size, num_p2, 3), dtype=torch.float32, device=device)
        st = lib.kamd_chamfer_distance_backward_fused_f32(
            _lib.stream_ptr(device), batch_size, num_p1, num_p2, grad_output.data_ptr(), state.data_ptr(),
            g1.data_ptr(), g2.data_ptr())
    if st != 0:
        _lib.check(st, fn)
    return [g1, g2]


def chamfer_distance_backward(grad_output, w1, w2, squared, p1, p2, idx1, idx2, dist1, dist2):
    """Gradient of ``chamfer_distance`` (kaolin/metrics/pointcloud.py:120-136) w.r.t. both clouds in one launch
    -> [grad_p1, grad_p2]; fp32 only.  Not part of the reference's ``kaolin._C`` (it evaluates the autograd chain
    weight -> mean -> [sqrt] -> two ``sided_distance_backward_cuda`` per point)."""
    fn = 'chamfer_distance_backward'
    args = [Arg(grad_output, 'grad_output', 1), Arg(p1, 'p1', 5), Arg(p2, 'p2', 6), Arg(idx1, 'idx1', 7),
            Arg(idx2, 'idx2', 8), Arg(dist1, 'dist1', 9), Arg(dist2, 'dist2', 10)]
    check_all_same_gpu(fn, args)
    check_all_contiguous(fn, args)
    batch_size, num_p1, num_p2 = p1.size(0), p1.size(1), p2.size(1)
    check_size(fn, args[0], [batch_size])
    check_size(fn, args[1], [batch_size, num_p1, 3])
    check_size(fn, args[2], [batch_size, num_p2, 3])
    check_size(fn, args[3], [batch_size, num_p1])
    check_size(fn, args[4], [batch_size, num_p2])
    check_size(fn, args[5], [batch_size, num_p1])
    check_size(fn, args[6], [batch_size, num_p2])
    torch_check(p1.dtype == torch.float32 and p2.dtype == torch.float32 and grad_output.dtype == torch.float32,
                f'{fn}: only Float clouds are supported')
    lib = _lib.load()
    with _lib.on_device(p1.device):
        g1, g2 = torch.empty_like(p1), torch.empty_like(p2)     # the kernels write every entry
        st = lib.kamd_chamfer_distance_backward_f32(
            _lib.stream_ptr(p1.device), batch_size, num_p1, num_p2, _lib.ptr(grad_output), float(w1), float(w2),
            1 if squared else 0, _lib.ptr(p1), _lib.ptr(p2), _lib.ptr(idx1), _lib.ptr(idx2), _lib.ptr(dist1),
            _lib.ptr(dist2), _lib.ptr(g1), _lib.ptr(g2))
    _lib.check(st, fn)
    return [g1, g2]


def sided_distance_backward_cuda(grad_output, p1, p2, idx):
    """reference: kaolin/csrc/metrics/sided_distance.cpp:91-122 -> [grad_p1, grad_p2]"""
    fn = 'sided_distance_backward_cuda'
    g_arg, p1_arg, p2_arg, idx_arg = (Arg(grad_output, 'grad_output', 1), Arg(p1, 'p1', 2),
                                      Arg(p2, 'p2', 3), Arg(idx, 'idx', 4))
    check_all_same_gpu(fn, [g_arg, p1_arg, p2_arg, idx_arg])
    check_all_contiguous(fn, [g_arg, p1_arg, p2_arg, idx_arg])
    batch_size, num_p1, num_p2 = p1.size(0), p1.size(1), p2.size(1)
    check_size(fn, idx_arg, [batch_size, num_p1])
    check_size(fn, p1_arg, [batch_size, num_p1, 3])
    check_size(fn, p2_arg, [batch_size, num_p2, 3])
    check_same_size(fn, idx_arg, g_arg)
    sfx = _lib.dtype_suffix(p1.dtype, fn, _SD_TYPES)
    lib = _lib.load()
    with _lib.on_device(p1.device):
        g1 = torch.zeros_like(p1)
        g2 = torch.zeros_like(p2)
        st = getattr(lib, f'kamd_sided_distance_backward_{sfx}')(
            _lib.stream_ptr(p1.device), batch_size, num_p1, num_p2,
            _lib.ptr(grad_output), _lib.ptr(p1), _lib.ptr(p2), _lib.ptr(idx), _lib.ptr(g1), _lib.ptr(g2))
    _lib.check(st, fn)
    return [g1, g2]


def _check_cuda_contig(pairs):
    # CHECK_CUDA / CHECK_CONTIGUOUS (kaolin/csrc/check.h:22-24), in the reference's order
    for name, t in pairs:
        torch_check(t.is_cuda, f'{name} must be a CUDA tensor')
    for name, t in pairs:
        torch_check(t.is_contiguous(), f'{name} must be contiguous')


def _check_sizes(name, t, sizes, spelled):
    # CHECK_SIZES (check.h:37-39)
    torch_check(list(t.shape) == list(sizes), f'{name} must of size {{{spelled}}}')


def unbatched_triangle_distance_forward_cuda(points, face_vertices, dist, face_idx, dist_type):
    """reference: kaolin/csrc/metrics/unbatched_triangle_distance.cpp:43-72 -> None (outputs are
    caller-allocated: metrics/trianglemesh.py:130-134)"""
    fn = 'unbatched_triangle_distance_forward_cuda'
    _check_cuda_contig([('points', points), ('face_vertices', face_vertices), ('dist', dist),
                        ('face_idx', face_idx), ('dist_type', dist_type)])
    num_points, num_faces = points.size(0), face_vertices.size(0)
    _check_sizes('points', points, [num_points, 3], 'num_points, 3')
    _check_sizes('face_vertices', face_vertices, [num_faces, 3, 3], 'num_faces, 3, 3')
    _check_sizes('dist', dist, [num_points], 'num_points')
    _check_sizes('face_idx', face_idx, [num_points], 'num_points')
    _check_sizes('dist_type', dist_type, [num_points], 'num_points')
    sfx = _lib.dtype_suffix(points.dtype, fn)
    torch_check(face_vertices.dtype == points.dtype and dist.dtype == points.dtype,
                'expected scalar type of points, face_vertices and dist to match')
    torch_check(face_idx.dtype == torch.long, 'expected scalar type Long but found ' + str(face_idx.dtype))
    torch_check(dist_type.dtype == torch.int32, 'expected scalar type Int but found ' + str(dist_type.dtype))
    lib = _lib.load()
    with _lib.on_device(points.device):
        ws = _lib.workspace(
            lib.kamd_triangle_distance_forward_workspace(num_points, num_faces, points.element_size()),
            points.device)
        st = getattr(lib, f'kamd_triangle_distance_forward_{sfx}')(
            _lib.stream_ptr(points.device), num_points, num_faces, _lib.ptr(points), _lib.ptr(face_vertices),
            _lib.ptr(dist), _lib.ptr(face_idx), _lib.ptr(dist_type), _lib.ptr(ws))
    _lib.check(st, fn)


def unbatched_triangle_distance_backward_cuda(grad_dist, points, face_vertices, face_idx, dist_type,
                                              grad_points, grad_face_vertices):
    """reference: kaolin/csrc/metrics/unbatched_triangle_distance.cpp:74-114 -> None; accumulates into the
    caller-zeroed grad_points / grad_face_vertices (metrics/trianglemesh.py:144-148)"""
    fn = 'unbatched_triangle_distance_backward_cuda'
    _check_cuda_contig([('grad_dist', grad_dist), ('points', points), ('face_vertices', face_vertices),
                        ('face_idx', face_idx), ('dist_type', dist_type), ('grad_points', grad_points),
                        ('grad_face_vertices', grad_face_vertices)])
    num_points, num_faces = points.size(0), face_vertices.size(0)
    _check_sizes('grad_dist', grad_dist, [num_points], 'num_points')
    _check_sizes('points', points, [num_points, 3], 'num_points, 3')
    _check_sizes('face_vertices', face_vertices, [num_faces, 3, 3], 'num_faces, 3, 3')
    _check_sizes('face_idx', face_idx, [num_points], 'num_points')
    _check_sizes('dist_type', dist_type, [num_points], 'num_points')
    _check_sizes('grad_points', grad_points, [num_points, 3], 'num_points, 3')
    _check_sizes('grad_face_vertices', grad_face_vertices, [num_faces, 3, 3], 'num_faces, 3, 3')
    sfx = _lib.dtype_suffix(points.dtype, fn)
    lib = _lib.load()
    with _lib.on_device(points.device):
        st = getattr(lib, f'kamd_triangle_distance_backward_{sfx}')(
            _lib.stream_ptr(points.device), num_points, num_faces, _lib.ptr(grad_dist), _lib.ptr(points),
            _lib.ptr(face_vertices), _lib.ptr(face_idx), _lib.ptr(dist_type), _lib.ptr(grad_points),
            _lib.ptr(grad_face_vertices))
    _lib.check(st, fn)


# ---- metrics.tetmesh (csrc/tetmesh_metrics.hip).  Not part of the reference's ``kaolin._C``: it evaluates these three losses as
# chains of torch kernels (kaolin/metrics/tetmesh.py).  Nothing below reads back or synchronises: the operators capture into a graph.
def _batch_items(t):
    """(tensor, batch stride in elements): every item contiguous, the batch stride free (0 for an expanded batch); anything
    else is copied"""
    if t.size(0) == 0 or t[0].is_contiguous():
        return t, (t.stride(0) if t.size(0) > 1 else 0)
    t = t.contiguous()
    return t, t.stride(0)


def _tetmesh_args(fn, tet_vertices, others=()):
    """tet_vertices (B, T, 4, 3) float32 / float64 on a GPU; others: ((name, tensor or None, shape), ...) of the same dtype and
    device -> (suffix, B, T)"""
    torch_check(tet_vertices.is_cuda, f'{fn}: tet_vertices must be a CUDA tensor')
    torch_check(tet_vertices.dim() == 4 and tet_vertices.shape[2:] == (4, 3),
                f'{fn}: tet_vertices must of size {{batch_size, num_tetrahedrons, 4, 3}}')
    sfx = _lib.dtype_suffix(tet_vertices.dtype, fn)
    for name, t, shape in others:
        if t is None:
            continue
        torch_check(t.is_cuda and t.device == tet_vertices.device, f'{fn}: {name} must be a CUDA tensor on the device of tet_vertices')
        torch_check(t.dtype == tet_vertices.dtype, f'{fn}: expected {name} to have the scalar type of tet_vertices')
        torch_check(tuple(t.shape) == tuple(shape), f'{fn}: {name} must of size {{{", ".join(str(s) for s in shape)}}}')
    return sfx, tet_vertices.size(0), tet_vertices.size(1)


def _tetmesh_workspace(lib, B, T, device):
    return _lib.workspace(lib.kamd_tetmesh_reduce_workspace(B, T), device)


def tetmesh_volume_forward_cuda(tet_vertices):
    """tet_vertices (B, T, 4, 3) -> volumes (B, T): ``((A - D) . ((B - D) x (C - D))) / 6``, signed."""
    fn = 'tetmesh_volume_forward_cuda'
    sfx, B, T = _tetmesh_args(fn, tet_vertices)
    dev = tet_vertices.device
    tv, bs = _batch_items(tet_vertices.detach())
    lib = _lib.load()
    with _lib.on_device(dev):
        volumes = torch.empty((B, T), dtype=tv.dtype, device=dev)
        if B > 0 and T > 0:
            _lib.check(getattr(lib, f'kamd_tetmesh_volume_forward_{sfx}')(
                _lib.stream_ptr(dev), B, T, _lib.ptr(tv), bs, _lib.ptr(volumes)), fn)
    return volumes


def tetmesh_volume_backward_cuda(grad_volumes, tet_vertices):
    """grad_volumes (B, T), any strides; tet_vertices (B, T, 4, 3) -> grad_tet_vertices (B, T, 4, 3), recomputed from the input."""
    fn = 'tetmesh_volume_backward_cuda'
    sfx, B, T = _tetmesh_args(fn, tet_vertices, (('grad_volumes', grad_volumes, (tet_vertices.size(0), tet_vertices.size(1))),))
    dev = tet_vertices.device
    tv, bs = _batch_items(tet_vertices.detach())
    g = grad_volumes.contiguous()
    lib = _lib.load()
    with _lib.on_device(dev):
        grad = torch.empty((B, T, 4, 3), dtype=tv.dtype, device=dev)
        if B > 0 and T > 0:
            _lib.check(getattr(lib, f'kamd_tetmesh_volume_backward_{sfx}')(
                _lib.stream_ptr(dev), B, T, _lib.ptr(tv), bs, _lib.ptr(g), _lib.ptr(grad)), fn)
    return grad


def _check_power(fn, power):
    torch_check(isinstance(power, int) and not isinstance(power, bool) and 1 <= power <= 16, f'{fn}: pow must be an int in [1, 16]')


def tetmesh_equivolume_forward_cuda(tet_vertices, mean, power):
    """tet_vertices (B, T, 4, 3), T >= 1; mean: ONE element; power: int in [1, 16] -> loss (B, 1): the mean over the tets of
    ``|volume - mean| ** power``.  Two launches: a partial per workgroup, then their sum in a fixed order (no atomics)."""
    fn = 'tetmesh_equivolume_forward_cuda'
    sfx, B, T = _tetmesh_args(fn, tet_vertices, (('mean', mean, (1,) * mean.dim()),))
    _check_power(fn, power)
    torch_check(T > 0, f'{fn}: no tetrahedrons')
    dev = tet_vertices.device
    tv, bs = _batch_items(tet_vertices.detach())
    lib = _lib.load()
    with _lib.on_device(dev):
        loss = torch.empty((B, 1), dtype=tv.dtype, device=dev)
        if B > 0:
            ws = _tetmesh_workspace(lib, B, T, dev)
            _lib.check(getattr(lib, f'kamd_tetmesh_equivolume_forward_{sfx}')(
                _lib.stream_ptr(dev), B, T, _lib.ptr(tv), bs, _lib.ptr(mean.detach()), power, _lib.ptr(loss), _lib.ptr(ws)), fn)
    return loss


def tetmesh_equivolume_backward_cuda(grad_loss, tet_vertices, mean, power, need_tet_vertices=True, need_mean=True):
    """grad_loss (B, 1), any strides -> (grad_tet_vertices (B, T, 4, 3) or None, grad_mean of mean's shape or None); each is
    computed only when asked for.  At ``volume == mean`` the term is 0, as ``torch.abs``'s gradient."""
    fn = 'tetmesh_equivolume_backward_cuda'
    sfx, B, T = _tetmesh_args(fn, tet_vertices, (('mean', mean, (1,) * mean.dim()), ('grad_loss', grad_loss, (tet_vertices.size(0), 1))))
    _check_power(fn, power)
    torch_check(T > 0, f'{fn}: no tetrahedrons')
    dev = tet_vertices.device
    tv, bs = _batch_items(tet_vertices.detach())
    g = grad_loss.contiguous()
    lib = _lib.load()
    with _lib.on_device(dev):
        grad_tv = torch.empty((B, T, 4, 3), dtype=tv.dtype, device=dev) if need_tet_vertices else None
        grad_mean = torch.zeros(mean.shape, dtype=tv.dtype, device=dev) if need_mean else None
        if B > 0 and (need_tet_vertices or need_mean):
            ws = _tetmesh_workspace(lib, B, T, dev) if need_mean else None
            _lib.check(getattr(lib, f'kamd_tetmesh_equivolume_backward_{sfx}')(
                _lib.stream_ptr(dev), B, T, _lib.ptr(tv), bs, _lib.ptr(mean.detach()), power, _lib.ptr(g), _lib.ptr(grad_tv),
                _lib.ptr(grad_mean), _lib.ptr(ws)), fn)
    return grad_tv, grad_mean


def _inverse_items(fn, tet_vertices, inverse_offset_matrix):
    B, T = tet_vertices.size(0), tet_vertices.size(1)
    torch_check(inverse_offset_matrix.dim() == 4 and inverse_offset_matrix.size(0) in (1, B),
                f'{fn}: inverse_offset_matrix must of size {{batch_size or 1, num_tetrahedrons, 3, 3}}')
    inv, ibs = _batch_items(inverse_offset_matrix.detach())
    return inv, (ibs if inv.size(0) > 1 else 0)     # (a batch of one against B > 1 is read B times)


def tetmesh_amips_forward_cuda(tet_vertices, inverse_offset_matrix):
    """tet_vertices (B, T, 4, 3), T >= 1; inverse_offset_matrix (B or 1, T, 3, 3) -> loss (B, 1): the mean over the tets of
    ``tr(J J^T) / (det(J)^2 + 1e-10)^(1/3) * (det(J) >= 0)``, J = (rows B - A, C - A, D - A) M.  Two launches, no atomics."""
    fn = 'tetmesh_amips_forward_cuda'
    shape = (inverse_offset_matrix.size(0) if inverse_offset_matrix.dim() else 0, tet_vertices.size(1), 3, 3)
    sfx, B, T = _tetmesh_args(fn, tet_vertices, (('inverse_offset_matrix', inverse_offset_matrix, shape),))
    torch_check(T > 0, f'{fn}: no tetrahedrons')
    dev = tet_vertices.device
    tv, bs = _batch_items(tet_vertices.detach())
    inv, ibs = _inverse_items(fn, tet_vertices, inverse_offset_matrix)
    lib = _lib.load()
    with _lib.on_device(dev):
        loss = torch.empty((B, 1), dtype=tv.dtype, device=dev)
        if B > 0:
            ws = _tetmesh_workspace(lib, B, T, dev)
            _lib.check(getattr(lib, f'kamd_tetmesh_amips_forward_{sfx}')(
                _lib.stream_ptr(dev), B, T, _lib.ptr(tv), bs, _lib.ptr(inv), ibs, _lib.ptr(loss), _lib.ptr(ws)), fn)
    return loss


def tetmesh_amips_backward_cuda(grad_loss, tet_vertices, inverse_offset_matrix, need_tet_vertices=True, need_inverse=True):
    """grad_loss (B, 1), any strides -> (grad_tet_vertices (B, T, 4, 3) or None, grad_inverse_offset_matrix of the matrix' shape
    or None); each is computed only when asked for.  A matrix batch of one against B > 1 gets the sum over the items."""
    fn = 'tetmesh_amips_backward_cuda'
    shape = (inverse_offset_matrix.size(0) if inverse_offset_matrix.dim() else 0, tet_vertices.size(1), 3, 3)
    sfx, B, T = _tetmesh_args(fn, tet_vertices, (('inverse_offset_matrix', inverse_offset_matrix, shape),
                                                 ('grad_loss', grad_loss, (tet_vertices.size(0), 1))))
    torch_check(T > 0, f'{fn}: no tetrahedrons')
    dev = tet_vertices.device
    tv, bs = _batch_items(tet_vertices.detach())
    inv, ibs = _inverse_items(fn, tet_vertices, inverse_offset_matrix)
    g = grad_loss.contiguous()
    lib = _lib.load()
    with _lib.on_device(dev):
        grad_tv = torch.empty((B, T, 4, 3), dtype=tv.dtype, device=dev) if need_tet_vertices else None
        grad_inv = torch.empty((B, T, 3, 3), dtype=tv.dtype, device=dev) if need_inverse else None
        if B > 0 and (need_tet_vertices or need_inverse):
            _lib.check(getattr(lib, f'kamd_tetmesh_amips_backward_{sfx}')(
                _lib.stream_ptr(dev), B, T, _lib.ptr(tv), bs, _lib.ptr(inv), ibs, _lib.ptr(g), _lib.ptr(grad_tv),
                _lib.ptr(grad_inv)), fn)
        if grad_inv is not None and inverse_offset_matrix.size(0) != B:
            grad_inv = grad_inv.sum(dim=0, keepdim=True)
    return grad_tv, grad_inv
