"""``kaolin.ops.spc`` sparse convolutions over the points of an octree level (reference: kaolin/ops/spc/convolution.py).

The contract, for input rows X at ``level`` = Q, kernel vectors v_k and weights W[k] (in, out):

* ``conv3d``: the output rows are the points of P = Q - jump, s = 2^jump, and ``Y[p] = sum_k X[point of Q at s p + v_k] W[k]`` over
  the neighbours the octree has;
* ``conv_transpose3d``: the output rows are the points of P = Q + jump and ``Y[p] = sum_k X[point of Q at (p - v_k) / s] W[k]`` over
  the k for which every component of p - v_k is non-negative and divisible by s.

A neighbour outside the grid of its level is a miss, duplicate kernel vectors each contribute, a row without neighbours is 0 (+
bias), and the coordinate arithmetic is int32 (the reference's int16 wraps for vectors near 2^15).  float32 / float64 CUDA tensors
run the HIP kernels of csrc/spc_conv.hip through ``_C.ops.spc`` (neighbour map + gather-GEMM; both gradients are gathers too: no
scan, no compaction, no host read, no atomics, bit-identical from run to run); CPU tensors (which the reference rejects), half and
bfloat16 run the ``_torch_*`` formulation of the same contract below -- also the yardstick of tools/time_spc_conv.py.

``exsum`` is accepted in the current layout only, as everywhere in this package."""
import math

import torch
from torch import nn

from ... import _C
from ..._C.ops import spc_conv_check as _check
from ...rep.spc import Spc
from .points import points_to_morton

__all__ = ['conv3d', 'Conv3d', 'conv_transpose3d', 'ConvTranspose3d']


# ---- the torch formulation ---------------------------------------------------------------------------------------------------
def _torch_neighbour_map(point_hierarchies, pyramids, kernel_vectors, row_level, target_level, transposed):
    """(K, rows at row_level) int64: the packed row at ``target_level`` of every row's neighbour under every kernel vector, -1 for
    a miss.  The points of an item's level are in Morton order: the neighbour's code is searched in that range."""
    dev = point_hierarchies.device
    p = pyramids.long()
    B, L = p.size(0), p.size(2) - 2
    jump = abs(target_level - row_level)
    npoints = p[:, 1, L + 1]
    pstart = (torch.cumsum(npoints, 0) - npoints).tolist()
    v = kernel_vectors.to(torch.int32)[:, None, :]
    maps, first_target = [], 0
    for b in range(B):
        r0, t0 = pstart[b] + int(p[b, 1, row_level]), pstart[b] + int(p[b, 1, target_level])
        rows = point_hierarchies[r0:r0 + int(p[b, 0, row_level])].to(torch.int32)[None]
        ntargets = int(p[b, 0, target_level])
        codes = points_to_morton(point_hierarchies[t0:t0 + ntargets])
        if transposed:
            u = rows - v
            c = u >> jump
            ok = ((u >= 0) & ((u & ((1 << jump) - 1)) == 0)).all(dim=-1)
        else:
            c = rows * (1 << jump) + v
            ok = torch.ones(c.shape[:-1], dtype=torch.bool, device=dev)
        ok = ok & ((c >= 0) & (c < (1 << target_level))).all(dim=-1)
        want = points_to_morton(torch.where(ok[..., None], c, 0).short().reshape(-1, 3)).reshape(ok.shape)
        at = torch.searchsorted(codes, want.reshape(-1)).reshape(ok.shape).clamp(max=ntargets - 1)
        ok = ok & (codes[at] == want)
        maps.append(torch.where(ok, at + first_target, -1))
        first_target += ntargets
    return torch.cat(maps, dim=1)


def _torch_conv(transposed, point_hierarchies, level, out_level, pyramids, input, weight, kernel_vectors):
    """One gathered matmul per kernel offset, added in the order of the offsets; half and bfloat16 accumulate in float32 and are
    rounded once.  Differentiable through torch's own autograd."""
    table = _torch_neighbour_map(point_hierarchies, pyramids, kernel_vectors, out_level, level, transposed)
    work = torch.float32 if input.dtype in (torch.float16, torch.bfloat16) else input.dtype
    x, w = input.to(work), weight.to(work)
    out = torch.zeros((table.size(1), weight.size(2)), dtype=work, device=input.device)
    for k in range(table.size(0)):
        rows = torch.nonzero(table[k] >= 0).reshape(-1)
        if rows.numel():
            out = out.index_add(0, rows, x[table[k][rows]].mm(w[k]))
    return out.to(input.dtype)


# ---- the HIP path ---------------------------------------------------------------------------------------------------------------
def _make_function(forward_op, backward_op):
    class _Function(torch.autograd.Function):
        @staticmethod
        def forward(ctx, octrees, point_hierarchies, level, pyramids, exsum, inputs, params, kernel_vectors, jump):
            tensors = [x.contiguous() for x in (octrees, point_hierarchies, pyramids, exsum, inputs, params, kernel_vectors)]
            ctx.save_for_backward(*tensors)
            ctx.jump = jump
            octrees, point_hierarchies, pyramids, exsum, inputs, params, kernel_vectors = tensors
            outputs, out_level = getattr(_C.ops.spc, forward_op)(octrees, point_hierarchies, level, pyramids, exsum, inputs, params,
                                                                kernel_vectors, jump)
            ctx.level = out_level
            return outputs

        @staticmethod
        def backward(ctx, grad_outputs):
            octrees, point_hierarchies, pyramids, exsum, inputs, params, kernel_vectors = ctx.saved_tensors
            grad_inputs, grad_params = getattr(_C.ops.spc, backward_op)(
                octrees, point_hierarchies, ctx.level, pyramids, exsum, inputs, grad_outputs.contiguous(), params, kernel_vectors,
                ctx.jump, needs=(ctx.needs_input_grad[5], ctx.needs_input_grad[6]))
            return None, None, None, None, None, grad_inputs, grad_params, None, None
    return _Function


_Conv3dFunction = _make_function('Conv3d_forward', 'Conv3d_backward')
_ConvTranspose3dFunction = _make_function('ConvTranspose3d_forward', 'ConvTranspose3d_backward')


def _conv(fn, transposed, octrees, point_hierarchies, level, pyramids, exsum, input, weight, kernel_vectors, jump, bias, kwargs):
    unexpected = kwargs.keys() - Spc.KEYS
    if unexpected:
        raise TypeError(f'{fn} got an unexpected keyword argument {list(unexpected)[0]}')
    in_level, out_level = _check(fn, transposed, octrees, point_hierarchies, level, pyramids, exsum, input, weight, kernel_vectors,
                                 jump, bias=bias)
    jump = int(jump)
    if weight.shape[0] == 1 and jump == 0:           # the reference's shortcut: whatever the one kernel vector is
        outputs, out_level = input.mm(weight[0]), level
    elif input.is_cuda and input.dtype in (torch.float32, torch.float64):
        function = _ConvTranspose3dFunction if transposed else _Conv3dFunction
        outputs = function.apply(octrees, point_hierarchies, in_level, pyramids, exsum, input, weight, kernel_vectors, jump)
    else:
        outputs = _torch_conv(transposed, point_hierarchies, in_level, out_level, pyramids, input, weight, kernel_vectors)
    if bias is not None:
        outputs = outputs + bias.unsqueeze(0)
    return outputs, int(out_level)


def conv3d(octrees, point_hierarchies, level, pyramids, exsum, input, weight, kernel_vectors, jump=0, bias=None, **kwargs):
    """Convolution over the points of a batch of octrees: ``Y[i] = sum_k X[n(i, k)] W[k] (+ bias)``.

    octrees (num_bytes) uint8, point_hierarchies (num_points, 3) int16, pyramids (B, 2, max_level + 2) int32 CPU and exsum
    (num_bytes) int32 of the batch; input (points of ``level`` in the batch, in_channels); weight (K, in_channels, out_channels);
    kernel_vectors (K, 3) int16; ``jump`` >= 0: the output lives ``jump`` levels above the input (stride 2^jump); bias
    (out_channels) -> (output (points of level - jump in the batch, out_channels), level - jump).

    Output point p takes, for every k, the input point at ``2^jump p + kernel_vectors[k]`` if the octree has it.  With K = 1 and
    jump = 0 the result is ``input.mm(weight[0])`` whatever the vector is, as in the reference.  Differentiable in input, weight
    and bias.  Keywords other than the members of ``Spc.KEYS`` raise TypeError; a bad argument raises ValueError before anything
    runs.  On the GPU (float32 / float64): 2 launches forward, 4 backward, no host read, results bit-identical from run to run."""
    return _conv('conv3d', False, octrees, point_hierarchies, level, pyramids, exsum, input, weight, kernel_vectors, jump, bias,
                 kwargs)


def conv_transpose3d(octrees, point_hierarchies, level, pyramids, exsum, input, weight, kernel_vectors, jump=0, bias=None,
                     **kwargs):
    """Transposed convolution over the points of a batch of octrees: arguments as ``conv3d`` -> (output (points of level + jump in
    the batch, out_channels), level + jump).

    Output point p takes, for every k with ``p - kernel_vectors[k]`` non-negative and divisible by 2^jump in every component, the
    input point at ``(p - kernel_vectors[k]) / 2^jump`` if the octree has it: the adjoint of ``conv3d``'s neighbourhood."""
    return _conv('conv_transpose3d', True, octrees, point_hierarchies, level, pyramids, exsum, input, weight, kernel_vectors, jump,
                 bias, kwargs)


class _ConvBase(nn.Module):
    _transposed = False

    def __init__(self, in_channels, out_channels, kernel_vectors, jump=0, bias=True):
        super().__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_vectors_size = kernel_vectors.shape[0]
        self.jump = jump
        self.register_buffer('kernel_vectors', kernel_vectors)
        self.kernel_shape = (self.kernel_vectors_size, in_channels, out_channels)
        self.weight = nn.Parameter(torch.empty(*self.kernel_shape))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        """uniform in +-1 / sqrt(fan), fan = kernel vectors x in_channels (out_channels for the transposed layer)"""
        fan = (self.out_channels if self._transposed else self.in_channels) * self.kernel_vectors_size
        bound = 1.0 / math.sqrt(fan)
        self.weight.data.uniform_(-bound, bound)
        if self.bias is not None:
            self.bias.data.uniform_(-bound, bound)

    def forward(self, octrees, point_hierarchies, level, pyramids, exsum, input, **kwargs):
        """-> (output features, their level); see ``conv3d`` / ``conv_transpose3d``"""
        name = type(self).__name__
        unexpected = kwargs.keys() - Spc.KEYS
        if unexpected:
            raise TypeError(f'{name} got an unexpected keyword argument {list(unexpected)[0]}')
        op = conv_transpose3d if self._transposed else conv3d
        return op(octrees, point_hierarchies, level, pyramids, exsum, input, self.weight, self.kernel_vectors, self.jump, self.bias)

    def __repr__(self):
        return f'{type(self).__name__}(in={self.in_channels}, out={self.out_channels}, kernel_vector_size={self.kernel_vectors_size})'


class Conv3d(_ConvBase):
    """``conv3d`` as a layer: weight (K, in_channels, out_channels), optional bias (out_channels), buffer ``kernel_vectors`` (K, 3)
    int16; ``forward(octrees, point_hierarchies, level, pyramids, exsum, input)`` -> (output, level - jump)."""


class ConvTranspose3d(_ConvBase):
    """``conv_transpose3d`` as a layer; ``forward`` -> (output, level + jump)."""
    _transposed = True
