"""Host shims of ``kaolin._C.render.spc`` (bindings.cpp; kaolin/csrc/render/spc/raytrace.cpp:177-436): octree ray tracing and the
packed ray operators over kamd_spc_raytrace_* / kamd_spc_pack_* (csrc/spc_raytrace.hip).

The reference's operator names and argument lists, so that its Python layer binds unchanged: ``cumsum_cuda`` / ``cumprod_cuda`` take
the list of pack starts and ``sum_reduce_cuda`` / ``prod_reduce_cuda`` the inclusive sum of the boundaries.  ``pack_scan`` is this
package's own entry point: it takes the boundaries themselves, so nothing is compacted and nothing is read back."""
import ctypes

import torch

from ... import _lib
from ..._checks import torch_check

SPC_MAX_LEVEL = 15      # KAOLIN_SPC_MAX_LEVELS


def raytrace_cuda(octree, points, pyramid, exsum, ray_o, ray_d, target_level, return_depth=True, with_exit=False):
    """reference: raytrace.cpp:177-221 ``raytrace_cuda``: octree (num_bytes) uint8, points (num_points, 3) int16, pyramid
    (2, max_level + 2) int32 CPU, exsum (num_bytes) int32, ray_o / ray_d (N, 3) float32 -> [nuggets (n, 2) int32] or [nuggets,
    depths (n, 1 | 2) float32]: (ray, point) of every box of ``target_level`` a ray enters, rays in input order, front to back.
    ``with_exit`` only acts together with ``return_depth`` (as in the reference): a hit then also needs an exit depth > 0.

    4 launches and ONE host read whatever the level (the reference: 3-4 launches and a blocking read per level).  ValueError for a
    level outside the pyramid, rays that are not (N, 3) float32 of one N, tensors on different devices, an exsum in the legacy
    layout, and 2^31 hits or more."""
    fn = 'raytrace_cuda'
    tensors = (octree, points, exsum, ray_o, ray_d)
    if not all(t.is_cuda for t in tensors) or len({t.device for t in tensors}) != 1:
        raise ValueError(f'{fn}: octree, points, exsum, ray_o and ray_d must be on one GPU, got {[str(t.device) for t in tensors]}')
    for name, r in (('ray_o', ray_o), ('ray_d', ray_d)):
        if r.dim() != 2 or r.size(1) != 3 or r.dtype != torch.float32:
            raise ValueError(f'{fn}: {name} must be a float32 tensor of size (num_rays, 3), got {r.dtype} {tuple(r.shape)}')
    if ray_o.size(0) != ray_d.size(0):
        raise ValueError(f'{fn}: {ray_o.size(0)} origins for {ray_d.size(0)} directions')
    torch_check(octree.dtype == torch.uint8 and octree.dim() == 1, f'{fn}: octree must be a 1D byte tensor')
    torch_check(points.dtype == torch.int16 and points.dim() == 2 and points.size(1) == 3, f'{fn}: points must be short, Nx3')
    torch_check(exsum.dtype == torch.int32 and exsum.dim() == 1, f'{fn}: exsum must be a 1D int tensor')
    torch_check(all(t.is_contiguous() for t in tensors), f'{fn}: expected contiguous tensors')
    torch_check(not pyramid.is_cuda and pyramid.dim() == 2 and pyramid.size(0) == 2 and pyramid.size(1) >= 2,
                f'{fn}: pyramid must be a CPU tensor of size {{2, max_level + 2}}')
    if exsum.numel() != octree.numel():
        raise ValueError(f'{fn}: exsum has {exsum.numel()} entries for {octree.numel()} octree bytes; only the current layout '
                         '(num_bytes entries, inclusive sums) is accepted, not the legacy one with a leading 0 per octree')
    max_level, level = pyramid.size(1) - 2, int(target_level)
    if not 0 <= level <= min(max_level, SPC_MAX_LEVEL):
        raise ValueError(f'{fn}: level {level} outside [0, max_level = {min(max_level, SPC_MAX_LEVEL)}]')
    torch_check(int(pyramid[1, max_level]) == octree.numel() and int(pyramid[1, max_level + 1]) == points.size(0),
                f'{fn}: the pyramid describes {int(pyramid[1, max_level])} bytes and {int(pyramid[1, max_level + 1])} points, '
                f'got {octree.numel()} and {points.size(0)}')
    N, dev = ray_o.size(0), octree.device
    mode = (2 if with_exit else 1) if return_depth else 0
    lib = _lib.load()
    with _lib.on_device(dev):
        total = 0
        if N > 0:
            torch_check(N < 2 ** 31, f'{fn}: more than 2^31 - 1 rays')
            sp = _lib.stream_ptr(dev)
            nbytes = lib.kamd_spc_raytrace_workspace(N)
            ws = _lib.workspace(nbytes, dev)
            head = (sp, N, level, octree.numel(), points.size(0), _lib.ptr(octree), _lib.ptr(exsum), _lib.ptr(points),
                    _lib.ptr(ray_o), _lib.ptr(ray_d))
            host_total = ctypes.c_int64(0)
            _lib.check(lib.kamd_spc_raytrace_count(*head, int(mode == 2), _lib.ptr(ws), ctypes.byref(host_total)), fn)
            total = host_total.value                                   # data-dependent size: the one host read
            if total >= 2 ** 31:
                raise ValueError(f'{fn}: {total} hits; the result is indexed with int32 and must stay below 2^31')
        nuggets = torch.empty((total, 2), dtype=torch.int32, device=dev)
        depths = torch.empty((total, mode), dtype=torch.float32, device=dev) if mode else None
        if total > 0:
            _lib.check(lib.kamd_spc_raytrace_emit(*head, mode, _lib.ptr(ws), total, _lib.ptr(nuggets), _lib.ptr(depths)), fn)
    return [nuggets, depths] if mode else [nuggets]


def mark_pack_boundaries_cuda(pack_ids):
    """reference: raytrace.cpp:223-238: pack_ids (n) of an integer dtype -> int32 (n): 1 where a pack starts.  Elementwise torch."""
    fn = 'mark_pack_boundaries_cuda'
    torch_check(pack_ids.dim() == 1, f'{fn}: pack_ids must be 1D')
    torch_check(pack_ids.dtype in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64), f'{fn}: pack_ids must be integral')
    out = torch.ones(pack_ids.size(0), dtype=torch.int32, device=pack_ids.device)
    if pack_ids.size(0) > 1:
        out[1:] = pack_ids[1:] != pack_ids[:-1]
    return out


def diff_cuda(feats, pack_indices):
    """reference: raytrace.cpp:292-316: feats (n, C), pack_indices (num_packs) int64 = the pack starts -> out[i] = feats[i + 1] -
    feats[i] inside a pack, 0 at every pack's last element.  Elementwise torch."""
    n = feats.size(0)
    last = torch.zeros(n, dtype=torch.bool, device=feats.device)
    if n > 0:
        last[-1] = True
        starts = pack_indices[pack_indices > 0]
        last[starts - 1] = True
    return _diff(feats, last)


def _diff(feats, last):
    out = torch.zeros_like(feats)
    if feats.size(0) > 1:
        out[:-1] = torch.where(last[:-1, None], out[:-1], feats[1:] - feats[:-1])
    return out


def inclusive_sum_cuda(info):
    """reference: raytrace.cpp:318-333: int32 (n) -> its inclusive sum, int32."""
    torch_check(info.dim() == 1 and info.dtype == torch.int32, 'inclusive_sum_cuda: info must be a 1D int tensor')
    return torch.cumsum(info, 0, dtype=torch.int32)


def _pack_args(fn, feats, other, other_name, other_dtypes):
    torch_check(feats.is_cuda and other.is_cuda and feats.device == other.device, f'{fn}: feats and {other_name} must be on one GPU')
    torch_check(feats.dim() == 2 and other.dim() == 1, f'{fn}: feats must be 2D and {other_name} 1D')
    torch_check(feats.is_contiguous() and other.is_contiguous(), f'{fn}: expected contiguous tensors')
    torch_check(other.dtype in other_dtypes, f'{fn}: {other_name} must be of type {" / ".join(str(d) for d in other_dtypes)}')
    return _lib.dtype_suffix(feats.dtype, fn)


def pack_scan(feats, boundaries, prod=False, exclusive=False, reverse=False, fn='pack_scan'):
    """feats (n, C) float32 / float64, boundaries (n) bool / uint8 (element 0 starts a pack whatever boundaries[0] says) -> the
    cumulative sum (``prod``: product) inside every pack, accumulated sequentially in index order (``reverse``: from the pack's
    end) in feats' dtype; ``exclusive`` writes the identity first.  One launch, no host read: capturable."""
    sfx = _pack_args(fn, feats, boundaries, 'boundaries', (torch.bool, torch.uint8))
    torch_check(boundaries.size(0) == feats.size(0), f'{fn}: {boundaries.size(0)} boundaries for {feats.size(0)} features')
    dev = feats.device
    with _lib.on_device(dev):
        out = torch.empty_like(feats)
        if out.numel() > 0:
            _lib.check(getattr(_lib.load(), f'kamd_spc_pack_scan_{sfx}')(
                _lib.stream_ptr(dev), feats.size(0), feats.size(1), _lib.ptr(feats), _lib.ptr(boundaries), int(bool(prod)),
                int(bool(exclusive)), int(bool(reverse)), _lib.ptr(out)), fn)
    return out


def _scan_from_indices(fn, feats, pack_indices, prod, exclusive, reverse):
    torch_check(pack_indices.dim() == 1 and pack_indices.dtype == torch.int32, f'{fn}: pack_indices must be a 1D int tensor')
    boundaries = torch.zeros(feats.size(0), dtype=torch.uint8, device=feats.device)
    boundaries[pack_indices.long()] = 1
    return pack_scan(feats, boundaries, prod, exclusive, reverse, fn=fn)


def cumsum_cuda(feats, pack_indices, exclusive, reverse):
    """reference: raytrace.cpp:387-411: pack_indices (num_packs) int32 = the pack starts (scattered back into boundaries here)."""
    return _scan_from_indices('cumsum_cuda', feats, pack_indices, False, exclusive, reverse)


def cumprod_cuda(feats, pack_indices, exclusive, reverse):
    """reference: raytrace.cpp:413-436."""
    return _scan_from_indices('cumprod_cuda', feats, pack_indices, True, exclusive, reverse)


def _reduce(fn, feats, inclusive_sum, prod):
    sfx = _pack_args(fn, feats, inclusive_sum, 'inclusive_sum', (torch.int32,))
    torch_check(inclusive_sum.size(0) == feats.size(0), f'{fn}: {inclusive_sum.size(0)} sums for {feats.size(0)} features')
    n, C, dev = feats.size(0), feats.size(1), feats.device
    with _lib.on_device(dev):
        num_packs = int(inclusive_sum[-1]) if n > 0 else 0             # sizes the result: the one host read
        out = torch.full((max(num_packs, 0), C), 1.0 if prod else 0.0, dtype=feats.dtype, device=dev)
        if out.numel() > 0:
            _lib.check(getattr(_lib.load(), f'kamd_spc_pack_reduce_{sfx}')(
                _lib.stream_ptr(dev), n, C, num_packs, _lib.ptr(feats), _lib.ptr(inclusive_sum), int(prod), _lib.ptr(out)), fn)
    return out


def sum_reduce_cuda(feats, inclusive_sum):
    """reference: raytrace.cpp:335-359: feats (n, C), inclusive_sum (n) int32 = the inclusive sum of the boundaries -> (num_packs, C),
    every pack summed from its first element on in index order (the reference: float atomics): bit-identical run to run."""
    return _reduce('sum_reduce_cuda', feats, inclusive_sum, False)


def prod_reduce_cuda(feats, inclusive_sum):
    """reference: raytrace.cpp:361-385."""
    return _reduce('prod_reduce_cuda', feats, inclusive_sum, True)
