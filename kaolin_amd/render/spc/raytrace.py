"""``kaolin.render.spc``: ray tracing of an octree and the reductions over the resulting packs of hits (reference:
kaolin/render/spc/raytrace.py).  float32 CUDA rays run the HIP walk of csrc/spc_raytrace.hip through ``_C.render.spc``; CPU tensors
(which the reference rejects) run ``_torch_raytrace`` below, a level-by-level formulation of the same contract that produces the
same bits -- device-agnostic, so tools/time_spc_raytrace.py also runs it on the GPU as its yardstick.  The packed operators run in
HIP for float32 / float64 CUDA features and as ``_torch_pack_scan`` / ``_torch_pack_reduce`` (step k of all packs at once, the same
sequential order) for everything else.

The contract of the trace ("SPC ray tracing") in short: per ray, depth-first from the root; a node above ``level`` is
descended when its box test returns d != 0 (a hit, or the origin inside), a node of ``level`` is emitted when d > 0 -- so the voxel
that holds the origin is not; children are visited in the order of (popcount(j ^ c), j), c the octant of the origin relative to
the node centre.  The box test is float32 with explicit fused multiply-adds; nuggets and depths equal the reference's bit for bit."""
import warnings

import torch

from ... import _C
from ...ops.spc.spc import _check_exsum
from ...ops.spc.uint8 import uint8_bits_sum

__all__ = ['unbatched_raytrace', 'mark_pack_boundaries', 'mark_first_hit', 'diff', 'sum_reduce', 'prod_reduce', 'cumsum', 'cumprod',
           'exponential_integration']

_MAX_LEVEL = 15
# row c: the children j of a node in the order of (popcount(j ^ c), j) -- the octant of the origin first
_ORDER = [sorted(range(8), key=lambda j, c=c: (bin(j ^ c).count('1'), j)) for c in range(8)]


# ---- ray tracing: the torch formulation ------------------------------------------------------------------------------------------
def _fmaf(a, b, c):
    """fmaf(a, b, c) of float32 tensors, bit for bit: the product is exact in float64 (48 bits), the sum is rounded to odd when it
    is inexact (its TwoSum error term is non-zero), so that narrowing to float32 rounds the exact value once."""
    p = a.double() * b.double()
    c = c.double().expand_as(p)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)
    fix = torch.isfinite(s) & torch.isfinite(e) & (e != 0) & ((s.view(torch.int64) & 1) == 0)
    away = (e > 0) == (s > 0)                                       # the exact sum lies farther from zero than s
    bits = s.view(torch.int64) + torch.where(away, 1, -1)           # the neighbour on that side: its last bit is odd
    return torch.where(fix, bits.view(torch.float64), s).float()


def _box(o, d, inv, sgn, r):
    """ray_aabb for rows of (origin relative to the box centre, direction, 1 / direction, signs) and half widths r (n, 1)"""
    a = o.abs()
    inside = torch.fmax(torch.fmax(a[:, 0], a[:, 1]), a[:, 2]) < r[:, 0]     # fmaxf: a NaN component is ignored
    dk = _fmaf(r, sgn, -o) * inv                                    # (n, 3): the distance to the entry plane of every axis
    ok = []
    for k in range(3):
        a, b = [x for x in range(3) if x != k]
        t = dk[:, k:k + 1]
        lt = _fmaf(d[:, [a, b]], t, o[:, [a, b]])
        ok.append((dk[:, k] >= 0) & (lt.abs() <= r).all(dim=1))
    zero = torch.zeros_like(dk[:, 0])
    out = torch.where(ok[0], dk[:, 0], torch.where(ok[1], dk[:, 1], torch.where(ok[2], dk[:, 2], zero)))
    out = torch.where(out != 0, out, zero)
    return torch.where(inside, -r[:, 0], out)


def _torch_raytrace(octree, points, exsum, origin, direction, level, return_depth, with_exit):
    """-> (nuggets (n, 2) int32, depths (n, 1 | 2) float32 or None): all rays level by level, the (ray, node) pairs kept in order"""
    dev, N = origin.device, origin.size(0)
    nbytes, npoints = octree.numel(), points.size(0)
    order = torch.tensor(_ORDER, dtype=torch.long, device=dev)
    inv_all = (1.0 / direction.double()).float()
    sgn_all = torch.where(torch.signbit(direction), 1.0, -1.0).float()
    half_all = _fmaf(torch.full_like(origin, 0.5), origin, torch.full_like(origin, 0.5))
    ridx = torch.arange(N, dtype=torch.long, device=dev)
    pidx = torch.zeros(N, dtype=torch.long, device=dev)
    if npoints == 0:
        ridx, pidx = ridx[:0], pidx[:0]
    depths = None
    for l in range(level + 1):
        r = torch.full((ridx.numel(), 1), 2.0 ** -l, dtype=torch.float32, device=dev)
        p = points[pidx].float()
        centre = _fmaf(r, _fmaf(torch.full_like(p, 2.0), p, torch.ones_like(p)), -torch.ones_like(p))
        o, d, inv, sgn = origin[ridx] - centre, direction[ridx], inv_all[ridx], sgn_all[ridx]
        entry = _box(o, d, inv, sgn, r)
        if l == level:
            keep = entry > 0
            if return_depth:
                depths = entry[:, None]
                if with_exit:
                    leave = _box(o, d, inv, -sgn, r)
                    keep = keep & (leave > 0)
                    depths = torch.stack([entry, leave], dim=1)
                depths = depths[keep]
            ridx, pidx = ridx[keep], pidx[keep]
            break
        keep = (entry != 0) & (pidx < nbytes)
        ridx, pidx, p = ridx[keep], pidx[keep], p[keep]
        if nbytes == 0:
            ridx, pidx = ridx[:0], pidx[:0]
            continue
        bits = octree[pidx].long()
        base = torch.where(pidx == 0, 0, exsum[(pidx - 1).clamp(min=0)].long())
        x = half_all[ridx].double() - (2.0 ** -l) * (p.double() + 0.5)
        c = 4 * (x[:, 0] > 0).long() + 2 * (x[:, 1] > 0).long() + (x[:, 2] > 0).long()
        j = order[c]                                                # (n, 8): the children in visit order
        present = ((bits[:, None] >> j) & 1) == 1
        upto = bits[:, None] & (torch.bitwise_left_shift(torch.full_like(j, 2), j) - 1)
        child = base[:, None] + uint8_bits_sum(upto.to(torch.uint8).reshape(-1)).reshape(-1, 8).long()
        present = present & (child < npoints)
        ridx = ridx[:, None].expand(-1, 8)[present]                 # row-major: a node's children stay together, in visit order
        pidx = child[present]
    return torch.stack([ridx, pidx], dim=1).int(), depths


def unbatched_raytrace(octree, point_hierarchy, pyramid, exsum, origin, direction, level, return_depth=True, with_exit=False):
    """Ray tracing over ONE octree, normalised to [-1, 1] on every axis.

    octree (num_bytes) uint8, point_hierarchy (num_points, 3) int16, pyramid (2, max_level + 2) int32 CPU and exsum (num_bytes)
    int32 of scan_octrees / generate_points; origin and direction (num_rays, 3) float32; ``level`` in 0..max_level.
    -> (ray index (n) int32, point index (n) int32[, depths (n, 1) float32, or (n, 2) with ``with_exit``: entry and exit]): every
    box of ``level`` that a ray enters, rays in input order, a ray's boxes front to back.  The two index tensors are the columns
    of one (n, 2) tensor, as in the reference.  The box that holds a ray's origin is not reported.  ``with_exit`` only acts
    together with ``return_depth`` (as in the reference) and then also drops the hits whose exit depth is not positive.

    On the GPU: one thread per ray walks its subtree depth-first, once to count and once to write -- 4 launches and one host read
    whatever the level, so the call synchronises and cannot be captured in a graph.  No gradient flows through it.  ValueError
    for a level outside the pyramid, rays that are not (N, 3) float32 of one N, tensors on different devices, an exsum of the
    legacy length, and 2^31 hits or more."""
    fn = 'unbatched_raytrace'
    _check_exsum(fn, exsum, octree.numel())
    level = int(level)
    if octree.is_cuda:
        out = _C.render.spc.raytrace_cuda(octree.contiguous(), point_hierarchy.contiguous(), pyramid.contiguous(),
                                          exsum.contiguous(), origin.detach().contiguous(), direction.detach().contiguous(), level,
                                          return_depth, with_exit)
        nuggets, depths = out[0], (out[1] if return_depth else None)
    else:
        tensors = (octree, point_hierarchy, exsum, origin, direction)
        if len({t.device for t in tensors}) != 1:
            raise ValueError(f'{fn}: expected every tensor on one device, got {[str(t.device) for t in tensors]}')
        for name, r in (('origin', origin), ('direction', direction)):
            if r.dim() != 2 or r.size(1) != 3 or r.dtype != torch.float32:
                raise ValueError(f'{fn}: {name} must be a float32 tensor of size (num_rays, 3), got {r.dtype} {tuple(r.shape)}')
        if origin.size(0) != direction.size(0):
            raise ValueError(f'{fn}: {origin.size(0)} origins for {direction.size(0)} directions')
        max_level = min(pyramid.size(-1) - 2, _MAX_LEVEL)
        if not 0 <= level <= max_level:
            raise ValueError(f'{fn}: level {level} outside [0, max_level = {max_level}]')
        nuggets, depths = _torch_raytrace(octree, point_hierarchy, exsum, origin.detach(), direction.detach(), level, return_depth,
                                          with_exit)
    if return_depth:
        return nuggets[..., 0], nuggets[..., 1], depths
    return nuggets[..., 0], nuggets[..., 1]


# ---- packs ------------------------------------------------------------------------------------------------------------------------
def mark_pack_boundaries(pack_ids):
    """pack_ids (n), any integer dtype, sorted so that the elements of a pack are adjacent (e.g. the ray index of
    unbatched_raytrace) -> bool (n): True where a pack starts.

    >>> mark_pack_boundaries(torch.IntTensor([1, 1, 1, 1, 2, 2, 2]))
    tensor([ True, False, False, False,  True, False, False])"""
    return _C.render.spc.mark_pack_boundaries_cuda(pack_ids.contiguous()).bool()


def mark_first_hit(ridx):
    """Deprecated alias of :func:`mark_pack_boundaries`."""
    warnings.warn('mark_first_hit has been deprecated, please use mark_pack_boundaries instead')
    return mark_pack_boundaries(ridx)


def diff(feats, boundaries):
    """``out[i] = feats[i + 1] - feats[i]`` inside every pack, 0 at a pack's last element.  feats (n, C), boundaries (n) bool."""
    shape = feats.shape
    feats = feats.reshape(-1, shape[-1])
    b = boundaries.reshape(-1) != 0
    last = torch.ones_like(b)
    last[:-1] = b[1:]
    return _C.render.spc._diff(feats, last).reshape(*shape)


def _pack_lengths(boundaries):
    """(starts, lengths) of the packs; element 0 starts a pack whatever boundaries[0] says"""
    n = boundaries.numel()
    b = boundaries.reshape(-1) != 0
    if n > 0:
        b = b.clone()
        b[0] = True
    starts = torch.nonzero(b)[:, 0]
    ends = torch.cat([starts[1:], starts.new_full((1,), n)]) if n > 0 else starts
    return starts, ends - starts


def _torch_pack_scan(feats, boundaries, prod, exclusive, reverse):
    """The sequential scan of every pack, step k of all packs at once, in feats' dtype (the order of the HIP kernel)."""
    out = torch.empty_like(feats)
    if feats.numel() == 0:
        return out
    starts, lens = _pack_lengths(boundaries)
    first = starts + lens - 1 if reverse else starts
    step = -1 if reverse else 1
    acc = torch.full_like(feats[first], 1.0 if prod else 0.0) if exclusive else feats[first]
    out[first] = acc
    for k in range(1, int(lens.max())):
        live = lens > k
        pos = first[live] + step * k
        term = feats[pos - step] if exclusive else feats[pos]
        acc = acc[live[lens > k - 1]]
        acc = term * acc if prod else term + acc
        out[pos] = acc
    return out


def _torch_pack_reduce(feats, boundaries, prod):
    starts, lens = _pack_lengths(boundaries)
    if boundaries.numel() > 0 and not bool(boundaries.reshape(-1)[0]):
        starts, lens = starts[1:], lens[1:]                         # elements before the first boundary belong to no pack
    acc = feats[starts]
    for k in range(1, int(lens.max()) if lens.numel() else 0):
        live = lens > k
        acc = acc.clone()
        acc[live] = acc[live] * feats[starts[live] + k] if prod else acc[live] + feats[starts[live] + k]
    return acc


def _hip(feats):
    return feats.is_cuda and feats.dtype in (torch.float32, torch.float64)


def _scan(feats, boundaries, prod, exclusive, reverse):
    if _hip(feats):
        b = boundaries if boundaries.dtype in (torch.bool, torch.uint8) else boundaries != 0
        return _C.render.spc.pack_scan(feats, b.contiguous(), prod, exclusive, reverse)
    return _torch_pack_scan(feats, boundaries, prod, exclusive, reverse)


def _reduce(feats, boundaries, prod):
    if _hip(feats):
        inclusive_sum = _C.render.spc.inclusive_sum_cuda(boundaries.int())
        op = _C.render.spc.prod_reduce_cuda if prod else _C.render.spc.sum_reduce_cuda
        return op(feats, inclusive_sum)
    return _torch_pack_reduce(feats, boundaries, prod)


class SumReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, boundaries):
        ctx.save_for_backward(boundaries)
        return _reduce(feats, boundaries, False)

    @staticmethod
    def backward(ctx, grad_output):
        boundaries, = ctx.saved_tensors
        pack = torch.cumsum(boundaries.reshape(-1) != 0, 0) - 1      # a gather: every element takes its pack's gradient
        grad = grad_output[pack.clamp(min=0)]
        return torch.where((pack >= 0)[:, None], grad, torch.zeros_like(grad)), None


class Cumsum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, boundaries, exclusive, reverse):
        ctx.save_for_backward(boundaries)
        ctx.flags = (exclusive, reverse)
        return _scan(feats, boundaries, False, exclusive, reverse)

    @staticmethod
    def backward(ctx, grad_output):
        boundaries, = ctx.saved_tensors
        exclusive, reverse = ctx.flags
        return _scan(grad_output.contiguous(), boundaries, False, exclusive, not reverse), None, None, None


class Cumprod(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, boundaries, exclusive, reverse):
        prod = _scan(feats, boundaries, True, exclusive, reverse)
        ctx.save_for_backward(feats, boundaries, prod)
        ctx.flags = (exclusive, reverse)
        return prod

    @staticmethod
    def backward(ctx, grad_output):
        feats, boundaries, prod = ctx.saved_tensors
        exclusive, reverse = ctx.flags
        out = _scan((prod * grad_output).contiguous(), boundaries, False, exclusive, not reverse)
        grad = out / feats                                          # the reference's (TensorFlow's) form: NaN -> 0
        return torch.where(grad.isnan(), torch.zeros_like(grad), grad), None, None, None


def _pack_inputs(fn, feats, boundaries):
    if feats.dim() != 2 or boundaries.dim() != 1 or boundaries.size(0) != feats.size(0):
        raise ValueError(f'{fn}: feats must be of size (n, num_feats) and boundaries of size (n), got {tuple(feats.shape)} and '
                         f'{tuple(boundaries.shape)}')
    if feats.device != boundaries.device:
        raise ValueError(f'{fn}: feats is on {feats.device}, boundaries on {boundaries.device}')
    return feats.contiguous(), boundaries.contiguous()


def sum_reduce(feats, boundaries):
    """feats (n, C), boundaries (n) bool (mark_pack_boundaries) -> (num_packs, C): the sum of every pack, accumulated from the
    pack's first element on in index order in feats' dtype -- deterministic (the reference uses float atomics).  Differentiable.
    The pack count is read back once, to size the result."""
    return SumReduce.apply(*_pack_inputs('sum_reduce', feats, boundaries))


def prod_reduce(feats, boundaries):
    """As :func:`sum_reduce` with products.  No backward pass (as in the reference)."""
    feats, boundaries = _pack_inputs('prod_reduce', feats, boundaries)
    return _reduce(feats.detach(), boundaries, True)


def cumsum(feats, boundaries, exclusive=False, reverse=False):
    """Cumulative sum inside every pack: feats (n, C), boundaries (n) bool -> (n, C).  ``exclusive``: an element's own value is left
    out (the pack's first result is 0); ``reverse``: from the pack's end.  Accumulated sequentially in feats' dtype, the
    reference's order.  On float32 / float64 GPU tensors: one launch, no host read -- graph-capturable.  Differentiable."""
    return Cumsum.apply(*_pack_inputs('cumsum', feats, boundaries), bool(exclusive), bool(reverse))


def cumprod(feats, boundaries, exclusive=False, reverse=False):
    """Cumulative product inside every pack, as :func:`cumsum`.  The gradient is the reference's: ``cumsum(prod * grad, opposite
    direction) / feats`` with NaN replaced by 0 (exact where feats has no zero)."""
    return Cumprod.apply(*_pack_inputs('cumprod', feats, boundaries), bool(exclusive), bool(reverse))


def exponential_integration(feats, tau, boundaries, exclusive=True):
    """Exponential transmittance integration over packs: feats (n, C), tau (n, 1) optical thickness, boundaries (n) bool ->
    (integrated features (num_packs, C), transmittance (n, 1)) with ``transmittance = exp(-cumsum(tau)) * (1 - exp(-tau))`` -- the
    reference's composition, in its cumsum form."""
    alpha = 1.0 - torch.exp(-tau.contiguous())
    transmittance = torch.exp(-1.0 * cumsum(tau.contiguous(), boundaries.contiguous(), exclusive=exclusive))
    transmittance = transmittance * alpha
    feats_out = sum_reduce(transmittance * feats.contiguous(), boundaries.contiguous())
    return feats_out, transmittance
