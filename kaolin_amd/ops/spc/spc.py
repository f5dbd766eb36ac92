"""``kaolin.ops.spc`` octrees: scan, point generation, query, dense conversion, dual octree and trinkets (reference:
kaolin/ops/spc/spc.py).  CUDA tensors run the HIP kernels of csrc/spc.hip and csrc/spc_trilinear.hip through ``_C.ops.spc``; CPU tensors (which the reference rejects) run the ``_torch_*`` formulations
of the same pipelines below -- device-agnostic, so tools/time_spc.py also runs them on the GPU as its yardstick.

``exsum`` is accepted in the current layout only: per octree the inclusive sum of the bit counts, ``num_bytes`` entries."""
import math
import warnings

import torch

from ... import _C
from ..._C.ops import SPC_DUAL_MAX_LEVEL as _DUAL_MAX_LEVEL, finish_scan as _finish_scan
from .points import _torch_morton_to_points, _torch_points_to_corners, _torch_points_to_morton, morton_to_points
from .uint8 import bits_to_uint8, uint8_bits_sum, uint8_to_bits

__all__ = ['feature_grids_to_spc', 'scan_octrees', 'generate_points', 'to_dense', 'unbatched_query', 'unbatched_get_level_points',
           'unbatched_make_dual', 'unbatched_make_trinkets']

_MAX_LEVEL = 15
_PYR = _MAX_LEVEL + 2


def _check_exsum(fn, exsum, num_bytes):
    if exsum.dim() != 1 or exsum.numel() != num_bytes:
        raise ValueError(f'{fn}: exsum has {exsum.numel()} entries for {num_bytes} octree bytes; only the current layout '
                         '(num_bytes entries, inclusive sums) is accepted, not the legacy one with a leading 0 per octree')


# ---- scan ------------------------------------------------------------------------------------------------------------------------
def _torch_scan_octrees(octrees, lens):
    """octrees (num_bytes) uint8, lens: list of B byte counts -> (full pyramids (B, 2, 17) int32 CPU, depths (list), exsum int32):
    the steps of the HIP pipeline -- bit counts, one inclusive sum over the batch, a walk of all items level by level through it,
    a rebase per item -- and one read-back."""
    dev, B, total = octrees.device, len(lens), octrees.numel()
    lens_t = torch.tensor(lens, dtype=torch.long, device=dev)
    starts = torch.cumsum(lens_t, 0) - lens_t
    g = torch.cumsum(uint8_bits_sum(octrees), 0)
    base = torch.where(starts > 0, g[(starts - 1).clamp(min=0)], 0)
    exsum = (g - torch.repeat_interleave(base, lens_t, output_size=total)).int()
    pyr = torch.zeros((B, 2, _PYR), dtype=torch.long, device=dev)
    pyr[:, 0, 0] = 1
    pyr[:, 1, 1] = 1
    prev = torch.zeros(B, dtype=torch.long, device=dev)
    depth = torch.zeros(B, dtype=torch.long, device=dev)
    active = torch.ones(B, dtype=torch.bool, device=dev)
    for level in range(1, _MAX_LEVEL + 1):
        active = active & (pyr[:, 1, level] <= lens_t)
        cur = g[starts + torch.minimum(prev, lens_t - 1)] - base            # the index is clamped to the item's length
        count = torch.where(active, cur - prev, 0)
        pyr[:, 0, level] = count
        pyr[:, 1, level + 1] = torch.where(active, pyr[:, 1, level] + count, 0)
        prev = torch.where(active, cur, prev)
        depth += active
    full = torch.cat([pyr.reshape(B, 2 * _PYR), depth[:, None]], dim=1).int().cpu()      # the one read-back
    return full[:, :2 * _PYR].reshape(B, 2, _PYR), full[:, 2 * _PYR].tolist(), exsum


def scan_octrees(octrees, lengths, legacy_exsum=False):
    """octrees (num_bytes) uint8: a batch of octrees packed one after the other; lengths (B) int32 CPU: bytes per octree ->
    (max_level, pyramids (B, 2, max_level + 2) int32 CPU, exsum (num_bytes) int32 on the octrees' device).

    ``pyramids[b, 0, l]`` is the number of points of level l, ``pyramids[b, 1, l]`` the number of points above it.  ``exsum`` is,
    per octree, the inclusive sum of the bit counts of its bytes.  ``legacy_exsum=True`` returns the deprecated layout instead
    (every octree's block with a leading 0, num_bytes + B entries) and warns.

    All octrees of a batch must have the same depth and account for their bytes exactly (``sum(pyramids[b, 0, :max_level]) ==
    lengths[b]``), ``sum(lengths) * 8`` must stay below 2^31 and the depth is at most 15: ValueError otherwise.  The host reads
    back once for the whole batch."""
    if octrees.is_cuda:
        max_level, pyramids, exsum = _C.ops.spc.scan_octrees_cuda(octrees.contiguous(), lengths.contiguous())
    else:
        fn = 'scan_octrees'
        if octrees.dtype != torch.uint8 or octrees.dim() != 1:
            raise ValueError(f'{fn}: octrees must be a 1D byte tensor')
        lens = [int(v) for v in lengths.tolist()]
        if len(lens) == 0 or min(lens) < 1:
            raise ValueError(f'{fn}: every octree needs at least one byte, got lengths {lens}')
        if sum(lens) != octrees.numel():
            raise ValueError(f'{fn}: lengths sum to {sum(lens)}, octrees holds {octrees.numel()} bytes')
        if sum(lens) * 8 >= 2 ** 31:
            raise ValueError(f'{fn}: {sum(lens)} bytes: sum(lengths) * 8 must stay below 2^31')
        full, depths, exsum = _torch_scan_octrees(octrees, lens)
        max_level, pyramids = _finish_scan(fn, full, depths, lens)
    if legacy_exsum:
        warnings.warn('scan_octrees(legacy_exsum=True) returns the deprecated exsum layout of size (num_bytes + batch_size); '
                      'the operators of this package accept the current layout only.', DeprecationWarning, stacklevel=2)
        blocks = torch.split(exsum, [int(v) for v in lengths.tolist()])
        exsum = torch.cat([t for block in blocks for t in (exsum.new_zeros(1), block)])
    return max_level, pyramids, exsum


# ---- generate_points -----------------------------------------------------------------------------------------------------------------
def _torch_generate_points(octrees, pyramids):
    """Level by level, all items together: the set bits of the level's bytes, in (node, bit) order, are the children
    ``2 * parent + bit`` -- Morton order inside an item.  The sizes come from the CPU pyramid."""
    dev = octrees.device
    p = pyramids.long()
    B, L = p.size(0), p.size(2) - 2
    count, above = p[:, 0, :].tolist(), p[:, 1, :].tolist()
    nbytes = [above[b][L] for b in range(B)]
    ostart = [sum(nbytes[:b]) for b in range(B)]
    levels = [torch.zeros((B, 3), dtype=torch.long, device=dev)]
    for l in range(L):
        index = torch.cat([torch.arange(ostart[b] + above[b][l], ostart[b] + above[b][l] + count[b][l]) for b in range(B)])
        node, child = torch.nonzero(uint8_to_bits(octrees[index.to(dev)]), as_tuple=True)
        levels.append(2 * levels[l][node] + torch.stack([child >> 2, (child >> 1) & 1, child & 1], dim=1))
    if B == 1:
        return torch.cat(levels).short()
    pieces = []
    for b in range(B):
        for l in range(L + 1):
            first = sum(count[i][l] for i in range(b))
            pieces.append(levels[l][first:first + count[b][l]])
    return torch.cat(pieces).short()


def generate_points(octrees, pyramids, exsum):
    """octrees (num_bytes) uint8, pyramids (B, 2, max_level + 2) int32 CPU and exsum (num_bytes) int32 of scan_octrees -> point
    hierarchies (num_points_at_all_levels, 3) int16: per octree its points level by level, root first, each level in Morton
    order.  On the GPU: max_level launches for the whole batch, no host read."""
    _check_exsum('generate_points', exsum, octrees.numel())
    if octrees.is_cuda:
        return _C.ops.spc.generate_points_cuda(octrees.contiguous(), pyramids.contiguous(), exsum.contiguous())
    return _torch_generate_points(octrees, pyramids)


# ---- query -----------------------------------------------------------------------------------------------------------------------------
def _torch_query(octree, exsum, coords, level, with_parents):
    """The walk of one thread of the HIP kernel, for all queries at once -> (Q, level + 1) int64, -1 from the first miss."""
    dev, Q, nbytes = coords.device, coords.size(0), octree.numel()
    if with_parents:        # double, truncated toward zero
        v = (2 ** level) * (coords.double() * 0.5 + 0.5)
        ok = (v > -32769.0) & (v < 32768.0)
        k = torch.where(ok, v, 0).trunc().long()
    else:                   # the coordinate's own arithmetic (float for half), floored
        c = coords.float() if coords.dtype == torch.float16 else coords
        v = torch.floor((0.5 * 2 ** level) * (c + 1.0))
        ok = (v >= -32768) & (v <= 32767)
        k = torch.where(ok, v, 0).long()
    ok = ok.all(dim=1) & ((k >= 0) & (k <= 2 ** level - 1)).all(dim=1)
    out = torch.full((Q, level + 1), -1, dtype=torch.long, device=dev)
    if nbytes == 0:
        return out
    out[:, 0] = torch.where(ok, 0, -1)
    ord_, alive = torch.zeros(Q, dtype=torch.long, device=dev), ok
    for l in range(level):
        depth = level - l - 1
        child = (((k[:, 0] >> depth) & 1) << 2) | (((k[:, 1] >> depth) & 1) << 1) | ((k[:, 2] >> depth) & 1)
        bits = octree[ord_.clamp(max=nbytes - 1)].long()
        hit = alive & (ord_ < nbytes) & (((bits >> child) & 1) == 1)
        upto = bits & (torch.bitwise_left_shift(torch.full_like(child, 2), child) - 1)
        base = torch.where(ord_ == 0, 0, exsum[(ord_ - 1).clamp(min=0, max=nbytes - 1)].long())
        ord_ = torch.where(hit, base + uint8_bits_sum(upto.byte()), ord_)
        alive = hit
        out[:, l + 1] = torch.where(alive, ord_, -1)
    return out


def unbatched_query(octree, exsum, query_coords, level, with_parents=False):
    """The index, in the point hierarchy of ``octree``, of the point of ``level`` that holds every coordinate; -1 where there is none.

    octree (num_bytes) uint8 and its exsum (num_bytes) int32; query_coords (Q, 3): floating point (half / float / double, read in
    place) in [-1, 1], or integer in [0, 2^level], converted with ``(q.float() / 2**level) * 2 - 1``.  -> int64 (Q), or with
    ``with_parents`` (Q, level + 1): the point and all its ancestors, root first.

    Quantisation follows the reference: ``floor(0.5 * 2^level * (q + 1))`` in the coordinate's arithmetic (float for half), and
    with parents ``2^level * (q * 0.5 + 0.5)`` in double, truncated toward zero.  A value no int16 holds, NaN included, is a miss.
    On the GPU: one launch, one thread per query, no host read and no allocation besides the result: graph-capturable."""
    _check_exsum('unbatched_query', exsum, octree.numel())
    level = int(level)
    if not 0 <= level <= _MAX_LEVEL:
        raise ValueError(f'unbatched_query: level must be in [0, {_MAX_LEVEL}], got {level}')
    coords = query_coords if query_coords.is_floating_point() else (query_coords.float() / (2 ** level)) * 2.0 - 1.0
    if coords.dtype not in (torch.float16, torch.float32, torch.float64):
        coords = coords.float()
    if octree.is_cuda:
        op = _C.ops.spc.query_multiscale_cuda if with_parents else _C.ops.spc.query_cuda
        return op(octree.contiguous(), exsum.contiguous(), coords.contiguous(), level)
    out = _torch_query(octree, exsum, coords, level, with_parents)
    return out if with_parents else out[:, level].contiguous()


# ---- to_dense ----------------------------------------------------------------------------------------------------------------------------
def _torch_to_dense(point_hierarchies, pyramids, input, level):
    dev = input.device
    p = pyramids.long()
    B, L, E = p.size(0), p.size(2) - 2, 1 << level
    counts, npoints = p[:, 0, level], p[:, 1, L + 1]
    first = (torch.cumsum(npoints, 0) - npoints + p[:, 1, level]).tolist()
    rows = torch.cat([torch.arange(first[b], first[b] + int(counts[b])) for b in range(B)]).to(dev)
    item = torch.repeat_interleave(torch.arange(B), counts).to(dev)
    pts = point_hierarchies[rows].long()
    out = torch.zeros((B, input.size(1), E, E, E), dtype=input.dtype, device=dev)
    out[item, :, pts[:, 0], pts[:, 1], pts[:, 2]] = input
    return out


class _ToDenseFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, point_hierarchies, level, pyramids, input):
        input = input.contiguous()
        pyramids = pyramids.contiguous()
        point_hierarchies = point_hierarchies.contiguous()
        ctx.save_for_backward(point_hierarchies, pyramids, input)
        ctx.level = level
        return _C.ops.spc.to_dense_forward(point_hierarchies, level, pyramids, input)

    @staticmethod
    def backward(ctx, grad_output):
        point_hierarchies, pyramids, input = ctx.saved_tensors
        grad = _C.ops.spc.to_dense_backward(point_hierarchies, ctx.level, pyramids, input, grad_output.contiguous())
        return None, None, None, grad


def to_dense(point_hierarchies, pyramids, input, level=-1, **kwargs):
    """Features of the points of one level -> dense grids: point_hierarchies (num_points, 3) int16 and pyramids (B, 2, max_level + 2)
    int32 CPU of a batch, input (points of ``level`` in the batch, C) -> (B, C, 2^level, 2^level, 2^level), ``out[b, :, x, y, z] =
    input[i]`` for point i = (x, y, z) of item b, zero elsewhere.  ``level = -1`` is the deepest level.  Differentiable in
    ``input``.  float32 / float64 CUDA tensors run in HIP (a zero fill and one thread per (point, channel); the backward is the
    matching gather), everything else the torch formulation.  The other members of ``Spc.KEYS`` are accepted and ignored, so that
    ``to_dense(**spc.to_dict(), input=..., level=...)`` works; any other keyword raises TypeError."""
    from ...rep.spc import Spc
    unexpected = kwargs.keys() - Spc.KEYS
    if unexpected:
        raise TypeError(f'to_dense got an unexpected keyword argument {list(unexpected)[0]!r}')
    max_level = pyramids.shape[2] - 2
    if level < 0:
        level = max_level + 1 + level
    if not 0 <= level <= max_level:
        raise ValueError(f'to_dense: level {level} outside [0, max_level = {max_level}]')
    rows = int(pyramids[:, 0, level].sum())
    if input.dim() != 2 or input.size(0) != rows:
        raise ValueError(f'to_dense: input must be of size ({rows}, feature_dim) for level {level}, got {tuple(input.shape)}')
    if input.is_cuda and input.dtype in (torch.float32, torch.float64):
        return _ToDenseFunction.apply(point_hierarchies, level, pyramids, input)
    return _torch_to_dense(point_hierarchies, pyramids, input, level)


# ---- feature grids -> SPC ------------------------------------------------------------------------------------------------------------
def feature_grids_to_spc(feature_grids, masks=None):
    """Sparse feature grids (B, C, X, Y, Z) -> (octrees (num_bytes) uint8, lengths (B) int32 CPU, features (num_points, C)): the
    octrees of the occupied cells (``masks`` (B, X, Y, Z) bool, default: any channel non-zero), padded to the next power of two,
    and the features of those cells in Morton order.  Vectorised over the batch: the grid is put into Morton order once, and a
    level is then a reshape."""
    B, C, X, Y, Z = feature_grids.shape
    dev = feature_grids.device
    L = max(int(math.ceil(math.log2(max(X, Y, Z)))), 0)
    D = 2 ** L
    padded = torch.zeros((B, D, D, D, C), dtype=feature_grids.dtype, device=dev)
    padded[:, :X, :Y, :Z] = feature_grids.permute(0, 2, 3, 4, 1)
    if masks is None:
        occupied = torch.any(padded != 0, dim=-1)
    else:
        assert masks.shape == (B, X, Y, Z)
        occupied = torch.zeros((B, D, D, D), dtype=torch.bool, device=dev)
        occupied[:, :X, :Y, :Z] = masks
    cells = morton_to_points(torch.arange(D ** 3, dtype=torch.long, device=dev)).long()
    flat = occupied[:, cells[:, 0], cells[:, 1], cells[:, 2]]                       # (B, 8^L), Morton order
    occ = [flat.reshape(B, 8 ** l, -1).any(dim=-1) for l in range(L + 1)]           # occupancy of every level
    occ[0] = torch.ones_like(occ[0])                                                # the root exists even in an empty grid
    batch = torch.arange(B, device=dev)
    pieces = []
    for l in range(L):
        byte = bits_to_uint8(occ[l + 1].reshape(B, 8 ** l, 8))
        pieces.append((byte[occ[l]], occ[l].sum(dim=1)))                            # item-major
    if not pieces:
        return (torch.empty(0, dtype=torch.uint8, device=dev), torch.zeros(B, dtype=torch.int32),
                padded[:, cells[:, 0], cells[:, 1], cells[:, 2]][flat])
    counts = torch.stack([c for _, c in pieces], dim=1)                             # (B, L)
    lengths = counts.sum(dim=1)
    item_start = torch.cumsum(lengths, 0) - lengths
    level_start = torch.cumsum(counts, 1) - counts
    total = sum(v.numel() for v, _ in pieces)
    octrees = torch.empty(total, dtype=torch.uint8, device=dev)
    for l, (values, c) in enumerate(pieces):                                        # (level, item) order -> (item, level)
        item = torch.repeat_interleave(batch, c, output_size=values.numel())
        rank = torch.arange(values.numel(), device=dev) - (torch.cumsum(c, 0) - c)[item]
        octrees[item_start[item] + level_start[item, l] + rank] = values
    features = padded[:, cells[:, 0], cells[:, 1], cells[:, 2]][flat]
    return octrees, lengths.int().cpu(), features


def unbatched_get_level_points(point_hierarchy, pyramid, level):
    """point_hierarchy (num_points, 3) and pyramid (2, max_level + 2) of ONE octree -> the points of ``level``."""
    return point_hierarchy[pyramid[1, level]:pyramid[1, level + 1]]


# ---- dual octree and trinkets ------------------------------------------------------------------------------------------------------
def _check_dual_depth(fn, pyramid, what='pyramid'):
    if pyramid.dim() != 2 or pyramid.size(0) != 2 or pyramid.size(1) < 2 or pyramid.is_cuda:
        raise ValueError(f'{fn}: {what} must be a CPU tensor of size (2, max_level + 2), got {tuple(pyramid.shape)}')
    max_level = pyramid.size(1) - 2
    if max_level > _DUAL_MAX_LEVEL:
        raise ValueError(f'{fn}: max_level {max_level}: the corners of level 15 reach 32768, which neither int16 nor the 15-bit '
                         f'Morton codes hold (the reference wraps silently); dual octrees go up to level {_DUAL_MAX_LEVEL}')
    return max_level


def _check_hierarchy(fn, points, pyramid, what_points='point_hierarchy', what='pyramid'):
    """What both devices' paths ask of a hierarchy and its pyramid (the shims of the HIP path repeat it): int16 (n, 3) points, at
    least one, and a pyramid whose rows agree, start at 0, do not decrease and end at n.  -> max_level"""
    max_level = _check_dual_depth(fn, pyramid, what)
    if points.dim() != 2 or points.size(1) != 3 or points.dtype != torch.int16:
        raise ValueError(f'{fn}: {what_points} must be short, of size (num_points, 3), got {points.dtype} {tuple(points.shape)}')
    n = points.size(0)
    if n == 0:
        raise ValueError(f'{fn}: no points in {what_points} (an octree has at least its root)')
    count, first = pyramid[0].tolist(), pyramid[1].tolist()
    if first[0] != 0 or first[max_level + 1] != n or \
            any(c < 0 or first[l] + c != first[l + 1] for l, c in enumerate(count[:max_level + 1])):
        raise ValueError(f'{fn}: {what} does not describe the {n} rows of {what_points}: {pyramid.tolist()}')
    return max_level


def _torch_make_dual(point_hierarchy, pyramid):
    """Level by level: the Morton codes of the 8 corners of every point, unique (which sorts them), decoded."""
    L = pyramid.size(1) - 2
    first = pyramid[1].tolist()
    levels = []
    for l in range(L + 1):
        corners = _torch_points_to_corners(point_hierarchy[first[l]:first[l + 1]]).reshape(-1, 3)
        levels.append(_torch_morton_to_points(torch.unique(_torch_points_to_morton(corners))))
    counts = [len(p) for p in levels]
    pyramid_dual = torch.zeros_like(pyramid)
    pyramid_dual[0, :L + 1] = torch.tensor(counts, dtype=pyramid.dtype)
    pyramid_dual[1, 1:] = torch.cumsum(torch.tensor(counts), 0).to(pyramid.dtype)
    return torch.cat(levels), pyramid_dual


def unbatched_make_dual(point_hierarchy, pyramid):
    """The dual of ONE octree: point_hierarchy (num_points, 3) int16 and pyramid (2, max_level + 2) int32 CPU -> (point_hierarchy_dual
    (num_dual_points, 3) int16, pyramid_dual (2, max_level + 2), like pyramid): per level the distinct corners of the level's
    cells (``points_to_corners``), in Morton order.  Features live on these corners; ``unbatched_make_trinkets`` maps cells to them.

    A corner of level l reaches 2^l, so the deepest octree with a dual has ``max_level = 14``: deeper raises ValueError (the
    reference wraps to -32768 silently).  On the GPU all levels go through ONE radix sort of ``level << 48 | Morton`` keys, and the
    host reads the level sizes once (the reference: a unique and an argsort with their reads per level)."""
    _check_hierarchy('unbatched_make_dual', point_hierarchy, pyramid)
    if point_hierarchy.is_cuda:
        return _C.ops.spc.make_dual_cuda(point_hierarchy.contiguous(), pyramid.contiguous())
    return _torch_make_dual(point_hierarchy, pyramid)


def _torch_make_trinkets(point_hierarchy, pyramid, point_hierarchy_dual, pyramid_dual):
    """Level by level: the corners' Morton codes searched in the level's sorted dual codes, the parents' in the previous level's."""
    dev = point_hierarchy.device
    L = pyramid.size(1) - 2
    first, first_dual = pyramid[1].tolist(), pyramid_dual[1].tolist()

    def find(codes, sorted_codes):
        if sorted_codes.numel() == 0:
            return torch.full_like(codes, -1)
        at = torch.searchsorted(sorted_codes, codes).clamp(max=sorted_codes.numel() - 1)
        return torch.where(sorted_codes[at] == codes, at, -1)
    trinkets, parents = [], []
    for l in range(L + 1):
        points = point_hierarchy[first[l]:first[l + 1]]
        dual_codes = _torch_points_to_morton(point_hierarchy_dual[first_dual[l]:first_dual[l + 1]])
        trinkets.append(find(_torch_points_to_morton(_torch_points_to_corners(points).reshape(-1, 3)), dual_codes).reshape(-1, 8))
        if l == 0:
            parents.append(torch.full((points.size(0),), -1, dtype=torch.long, device=dev))
        else:
            at = find(_torch_points_to_morton(points >> 1), _torch_points_to_morton(point_hierarchy[first[l - 1]:first[l]]))
            parents.append(torch.where(at >= 0, at + first[l - 1], -1))
    return torch.cat(trinkets).int(), torch.cat(parents).int()


def unbatched_make_trinkets(point_hierarchy, pyramid, point_hierarchy_dual, pyramid_dual):
    """The indirection from the cells of ONE octree to its dual (``unbatched_make_dual``) -> (trinkets (num_points, 8) int32,
    parents (num_points) int32).

    ``trinkets[i, j]`` is the index of corner j of point i (the corner order of ``points_to_corners``) in the dual, RELATIVE TO THE
    START OF ITS LEVEL -- the reference's convention: a feature tensor with one row per dual point of a level is indexed by the
    level's trinkets directly.  ``parents[i]`` is the absolute index in ``point_hierarchy`` of the parent ``point >> 1``, -1 for
    the root.  A corner or parent that is not there (a dual that does not belong to the hierarchy) is -1.  On the GPU: one launch,
    a binary search per (point, corner), no host read (the reference: Python dictionaries on the host)."""
    fn = 'unbatched_make_trinkets'
    if _check_hierarchy(fn, point_hierarchy, pyramid) != \
            _check_hierarchy(fn, point_hierarchy_dual, pyramid_dual, 'point_hierarchy_dual', 'pyramid_dual'):
        raise ValueError(f'{fn}: pyramid and pyramid_dual differ in depth')
    if point_hierarchy.device != point_hierarchy_dual.device:
        raise ValueError(f'{fn}: point_hierarchy is on {point_hierarchy.device}, point_hierarchy_dual on {point_hierarchy_dual.device}')
    if point_hierarchy.is_cuda:
        return _C.ops.spc.make_trinkets_cuda(point_hierarchy.contiguous(), pyramid.contiguous(), point_hierarchy_dual.contiguous(),
                                             pyramid_dual.contiguous())
    return _torch_make_trinkets(point_hierarchy, pyramid, point_hierarchy_dual, pyramid_dual)
