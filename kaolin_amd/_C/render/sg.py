"""Host shims of ``kaolin._C.render.sg`` (bindings.cpp:130-133): the reduced spherical-gaussian inner product,
forward and backward, over kamd_sg_reduced_inner_product_* (csrc/sg_lighting.hip).

Same names, argument order, checks and return structure as the reference's
kaolin/csrc/render/sg/unbatched_reduced_sg_inner_product.cpp; f32 and f64 (the reference: f32 only).
``reduced_sg_constant_lobe_forward`` / ``_backward`` are this package's own entry points for a row side that is one
constant lobe (cosine_lobe_sg(normal)): they read the normals alone and return only the gradient into them."""
import torch

from ... import _lib
from ..._checks import Arg, check_all_same_gpu, check_all_contiguous, check_all_same_type, check_size, torch_check

_NAMES = ('intensity', 'direction', 'sharpness', 'other_intensity', 'other_direction', 'other_sharpness')


def _check(fn, tensors, names):
    args = [Arg(t, n, k + 1) for k, (t, n) in enumerate(zip(tensors, names))]
    check_all_same_gpu(fn, args)
    check_all_contiguous(fn, args)
    check_all_same_type(fn, args)
    return args


def _check_sizes(fn, args, num_sg, num_other):
    *head, a, d, s, oa, od, os_ = args
    for g in head:                       # grad_out
        check_size(fn, g, [num_sg, 3])
    check_size(fn, a, [num_sg, 3])
    check_size(fn, d, [num_sg, 3])
    check_size(fn, s, [num_sg])
    check_size(fn, oa, [num_other, 3])
    check_size(fn, od, [num_other, 3])
    check_size(fn, os_, [num_other])


def unbatched_reduced_sg_inner_product_forward_cuda(intensity, direction, sharpness,
                                                    other_intensity, other_direction, other_sharpness):
    """-> (num_sg, 3): sum over the num_other lobes of the SG inner product of every row lobe with them."""
    fn = 'unbatched_reduced_sg_inner_product_forward_cuda'
    ts = (intensity, direction, sharpness, other_intensity, other_direction, other_sharpness)
    args = _check(fn, ts, _NAMES)
    num_sg, num_other = intensity.size(0), other_intensity.size(0)
    _check_sizes(fn, args, num_sg, num_other)
    sfx = _lib.dtype_suffix(intensity.dtype, fn)
    dev = intensity.device
    with _lib.on_device(dev):
        if num_sg == 0 or num_other == 0:
            return torch.zeros_like(intensity)
        out = torch.empty_like(intensity)
        st = getattr(_lib.load(), f'kamd_sg_reduced_inner_product_forward_{sfx}')(
            _lib.stream_ptr(dev), num_sg, num_other, _lib.ptr(intensity), _lib.ptr(direction), _lib.ptr(sharpness), 0.0,
            0.0, _lib.ptr(other_intensity), _lib.ptr(other_direction), _lib.ptr(other_sharpness), _lib.ptr(out))
    _lib.check(st, fn)
    return out


def unbatched_reduced_sg_inner_product_backward_cuda(grad_out, intensity, direction, sharpness,
                                                     other_intensity, other_direction, other_sharpness):
    """-> [grad_intensity, grad_direction, grad_sharpness, grad_other_intensity, grad_other_direction,
    grad_other_sharpness]; deterministic (no atomics)."""
    fn = 'unbatched_reduced_sg_inner_product_backward_cuda'
    ts = (grad_out, intensity, direction, sharpness, other_intensity, other_direction, other_sharpness)
    args = _check(fn, ts, ('grad_out',) + _NAMES)
    num_sg, num_other = intensity.size(0), other_intensity.size(0)
    _check_sizes(fn, args, num_sg, num_other)
    sfx = _lib.dtype_suffix(intensity.dtype, fn)
    dev = intensity.device
    with _lib.on_device(dev):
        if num_sg == 0 or num_other == 0:
            return [torch.zeros_like(t) for t in ts[1:]]
        grads = [torch.empty_like(t) for t in ts[1:]]
        lib = _lib.load()
        ws = _lib.workspace(lib.kamd_sg_reduced_inner_product_backward_workspace(num_sg, num_other, intensity.element_size()),
                            dev)
        st = getattr(lib, f'kamd_sg_reduced_inner_product_backward_{sfx}')(
            _lib.stream_ptr(dev), num_sg, num_other, _lib.ptr(grad_out), _lib.ptr(intensity), _lib.ptr(direction),
            _lib.ptr(sharpness), 0.0, 0.0, _lib.ptr(other_intensity), _lib.ptr(other_direction), _lib.ptr(other_sharpness),
            _lib.ptr(ws), *[_lib.ptr(g) for g in grads])
    _lib.check(st, fn)
    return grads


def _check_constant_lobe(fn, ts, names):
    args = _check(fn, ts, names)
    torch_check(ts[0].is_floating_point(), f'{fn}: expected a floating point dtype')
    return args


def reduced_sg_constant_lobe_forward(lobe_amplitude, lobe_sharpness, direction, other_intensity, other_direction,
                                     other_sharpness):
    """The reduced product with the row lobes (lobe_amplitude (x3), direction (num_sg, 3), lobe_sharpness): two Python
    scalars and the directions -> (num_sg, 3)."""
    fn = 'reduced_sg_constant_lobe_forward'
    ts = (direction, other_intensity, other_direction, other_sharpness)
    args = _check_constant_lobe(fn, ts, _NAMES[1:2] + _NAMES[3:])
    num_sg, num_other = direction.size(0), other_intensity.size(0)
    check_size(fn, args[0], [num_sg, 3])
    check_size(fn, args[1], [num_other, 3])
    check_size(fn, args[2], [num_other, 3])
    check_size(fn, args[3], [num_other])
    sfx = _lib.dtype_suffix(direction.dtype, fn)
    dev = direction.device
    with _lib.on_device(dev):
        if num_sg == 0 or num_other == 0:
            return torch.zeros_like(direction)
        out = torch.empty_like(direction)
        st = getattr(_lib.load(), f'kamd_sg_reduced_inner_product_forward_{sfx}')(
            _lib.stream_ptr(dev), num_sg, num_other, None, _lib.ptr(direction), None, float(lobe_amplitude),
            float(lobe_sharpness), _lib.ptr(other_intensity), _lib.ptr(other_direction), _lib.ptr(other_sharpness),
            _lib.ptr(out))
    _lib.check(st, fn)
    return out


def reduced_sg_constant_lobe_backward(grad_out, lobe_amplitude, lobe_sharpness, direction, other_intensity,
                                      other_direction, other_sharpness):
    """-> [grad_direction, grad_other_intensity, grad_other_direction, grad_other_sharpness]."""
    fn = 'reduced_sg_constant_lobe_backward'
    ts = (grad_out, direction, other_intensity, other_direction, other_sharpness)
    args = _check_constant_lobe(fn, ts, ('grad_out',) + _NAMES[1:2] + _NAMES[3:])
    num_sg, num_other = direction.size(0), other_intensity.size(0)
    check_size(fn, args[0], [num_sg, 3])
    check_size(fn, args[1], [num_sg, 3])
    check_size(fn, args[2], [num_other, 3])
    check_size(fn, args[3], [num_other, 3])
    check_size(fn, args[4], [num_other])
    sfx = _lib.dtype_suffix(direction.dtype, fn)
    dev = direction.device
    with _lib.on_device(dev):
        if num_sg == 0 or num_other == 0:
            return [torch.zeros_like(t) for t in ts[1:]]
        grads = [torch.empty_like(t) for t in ts[1:]]
        lib = _lib.load()
        ws = _lib.workspace(lib.kamd_sg_reduced_inner_product_backward_workspace(num_sg, num_other, direction.element_size()),
                            dev)
        st = getattr(lib, f'kamd_sg_reduced_inner_product_backward_{sfx}')(
            _lib.stream_ptr(dev), num_sg, num_other, _lib.ptr(grad_out), None, _lib.ptr(direction), None,
            float(lobe_amplitude), float(lobe_sharpness), _lib.ptr(other_intensity), _lib.ptr(other_direction),
            _lib.ptr(other_sharpness), _lib.ptr(ws), None, _lib.ptr(grads[0]), None, *[_lib.ptr(g) for g in grads[1:]])
    _lib.check(st, fn)
    return grads
