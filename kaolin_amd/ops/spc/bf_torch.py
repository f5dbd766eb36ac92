"""Torch formulations of the Bayesian-fusion operators of ``_C.ops.spc`` (csrc/spc_bf.hip): the same argument lists, the same
arithmetic contract (float32, one rounding per operation in the order written, no FMA -- which is what eager torch
gives), all points at once where the HIP kernels run one thread per point.  CPU tensors, which the reference rejects, run these;
tools/time_spc_bf.py also runs them on GPU tensors as its yardstick."""
import types

import numpy as np
import torch

from ..._C.ops import bf_transform
from .points import _torch_morton_to_points
from .uint8 import bits_to_uint8, uint8_bits_sum, uint8_to_bits

_NEAR = 0.15
_FLT_MAX = float(np.finfo(np.float32).max)
_CURVE_B = [[0, 0, 0, 2], [2, 4, 8, 16], [16, 24, 36, 48], [48, 60, 72, 79], [79, 86, 88, 86], [86, 84, 78, 72], [72, 66, 60, 56],
            [56, 52, 50, 49], [49, 48, 48, 48]]


def _f32(v, dev):
    return torch.tensor(v, dtype=torch.float32, device=dev)


def _sqrt(x):
    """the correctly rounded float32 square root the contract asks for: torch's vectorised float32 sqrt is not correctly rounded on
    every backend, the float64 one rounded to float32 is (53 >= 2 * 24 + 2 bits)"""
    return torch.sqrt(x.double()).float()


def _curve(dev):
    return _f32(_CURVE_B, dev) / _f32(255.0, dev)


def _segment(x, dev):
    u = x + 3.0
    iu = torch.trunc(u)
    t = u - iu
    s = 1.0 - t
    c = _curve(dev)[iu.clamp(0, 8).long()]
    return t, s, c


def _profile(x):
    dev = x.device
    mid = (x > -3.0) & (x < 6.0)
    t, s, c = _segment(torch.where(mid, x, 0.0), dev)
    val = 2.65625 * (s * s * (s * c[..., 0] + (3.0 * t) * c[..., 1]) + t * t * ((3.0 * s) * c[..., 2] + t * c[..., 3]))
    return torch.where(mid, val, torch.where(x >= 6.0, 0.5, 0.0).float())


def _profile_derivative(x):
    dev = x.device
    mid = (x > -3.0) & (x < 6.0)
    t, s, c = _segment(torch.where(mid, x, 0.0), dev)
    a0, a1, a2 = s * c[..., 0] + t * c[..., 1], s * c[..., 1] + t * c[..., 2], s * c[..., 2] + t * c[..., 3]
    b0, b1 = s * a0 + t * a1, s * a1 + t * a2
    return torch.where(mid, 7.96875 * (b1 - b0), 0.0)


def _origin(points, T):
    p = points.float()
    return ((p[:, 0:1] * T[0] + p[:, 1:2] * T[1]) + p[:, 2:3] * T[2]) + T[3]         # (n, 4): [x y z 1] * T, left to right


def _corners(points, T):
    """-> (n, 8, 3): (x / z, y / z, z) of corner i = O (+ row 0 if i & 4) (+ row 1 if i & 2) (+ row 2 if i & 1)"""
    O = _origin(points, T)[:, :3]
    out = []
    for i in range(8):
        P = O
        if i & 4:
            P = P + T[0, :3]
        if i & 2:
            P = P + T[1, :3]
        if i & 1:
            P = P + T[2, :3]
        out.append(torch.stack([P[:, 0] / P[:, 2], P[:, 1] / P[:, 2], P[:, 2]], dim=1))
    return torch.stack(out, dim=1)


_CHUNK = 1 << 20


def _in_chunks(fn, n, *per_point):
    """fn on at most _CHUNK points at a time (the formulations below hold dozens of (n, 8) temporaries), results concatenated"""
    if n <= _CHUNK:
        return fn(*per_point)
    parts = [fn(*(t[s:s + _CHUNK] for t in per_point)) for s in range(0, n, _CHUNK)]
    return tuple(torch.cat(column) for column in zip(*parts))


def _mat(cam, level, dev):
    T = torch.from_numpy(bf_transform(cam, int(level)))
    if not (bool(torch.isfinite(cam).all()) and bool(torch.isfinite(T).all())):
        raise ValueError('cam, and its product with the level\'s scaling, must be finite')
    return T.to(dev)


def _mip_offset(hw, l):
    return hw * ((4 ** l - 1) // 3)


def build_mip2d(depth_map, intrinsics, mip_levels, max_depth, true_depth):
    h, w = depth_map.shape
    L, s = int(mip_levels), 1 << int(mip_levels)
    if L < 1 or L > 15 or h % s or w % s:
        raise ValueError(f'build_mip2d: mip_levels must be in [1, 15] and divide the {h} x {w} depth map into whole 2^mip_levels '
                         f'blocks, got {L}')
    dev = depth_map.device
    k = intrinsics.detach().cpu().float().reshape(-1)
    fx, fy, cx, cy = (_f32(float(k[i]), dev) for i in (0, 5, 8, 9))
    if true_depth:
        u = (torch.arange(w, dtype=torch.float32, device=dev) - cx) / fx
        v = (torch.arange(h, dtype=torch.float32, device=dev) - cy) / fy
        factor = 1.0 / _sqrt((u[None, :] * u[None, :] + v[:, None] * v[:, None]) + 1.0)
        depth_map.copy_(torch.where(depth_map == _f32(float(max_depth), dev), depth_map, depth_map * factor))     # in place
    levels = []
    lo = hi = depth_map
    for _ in range(L):
        a, b, c, e = lo[0::2, 0::2], lo[0::2, 1::2], lo[1::2, 0::2], lo[1::2, 1::2]
        lo = torch.fmin(torch.fmin(a, c), torch.fmin(b, e))
        a, b, c, e = hi[0::2, 0::2], hi[0::2, 1::2], hi[1::2, 0::2], hi[1::2, 1::2]
        hi = torch.fmax(torch.fmax(a, c), torch.fmax(b, e))
        levels.append(torch.stack([lo.reshape(-1), hi.reshape(-1)], dim=1))
    return torch.cat(levels[::-1]).contiguous()


def oracleB(points, level, sigma, cam, depth_map, mips, mip_levels):
    return _in_chunks(lambda p: _oracleB(p, level, sigma, cam, depth_map, mips, mip_levels), points.size(0), points)


def _oracleB(points, level, sigma, cam, depth_map, mips, mip_levels):
    dev, n = points.device, points.size(0)
    level, L = int(level), int(mip_levels)
    if level == 0 or n == 0:
        return torch.ones(n, dtype=torch.int32, device=dev), torch.full((n,), 2, dtype=torch.int32, device=dev)
    h, w = depth_map.shape
    hw = (h >> L) * (w >> L)
    q = _corners(points, _mat(cam, level, dev))
    lo = torch.full((n, 3), _FLT_MAX, dtype=torch.float32, device=dev)
    hi = -lo
    for c in range(8):
        lo, hi = torch.fmin(lo, q[:, c]), torch.fmax(hi, q[:, c])
    near = _f32(_NEAR, dev)
    ordered = (lo <= hi).all(dim=1)        # (a coordinate that is NaN at every corner leaves lo > hi: the voxel is kept)
    inside = ordered & (lo[:, 0] >= 0) & (hi[:, 0] < w) & (lo[:, 1] >= 0) & (hi[:, 1] < h) & (lo[:, 2] > near)
    outside = ordered & ((hi[:, 0] < 0) | (lo[:, 0] > w) | (hi[:, 1] < 0) | (lo[:, 1] > h) | (hi[:, 2] < near))
    extent = torch.fmax(hi[:, 0] - lo[:, 0], hi[:, 1] - lo[:, 1])
    powers = _f32([2.0 ** k for k in range(L + 1)], dev)
    m = (powers[None, :] < extent[:, None]).sum(dim=1)                 # the smallest m with 2^m >= extent, at most L + 1
    use = inside & (m <= L)
    mc = m.clamp(max=L)
    inv = _f32([2.0 ** -k for k in range(L + 1)], dev)[mc]
    zero = torch.zeros((), dtype=torch.float32, device=dev)
    xmin, ymin = (inv * torch.where(use, lo[:, 0], zero)).long(), (inv * torch.where(use, lo[:, 1], zero)).long()
    xmax, ymax = (inv * torch.where(use, hi[:, 0], zero)).long(), (inv * torch.where(use, hi[:, 1], zero)).long()
    stride, rows = torch.full_like(mc, w) >> mc, torch.full_like(mc, h) >> mc
    use = use & (xmin >= 0) & (xmin <= xmax) & (xmax < stride) & (ymin >= 0) & (ymin <= ymax) & (ymax < rows)
    off = torch.tensor([0] + [_mip_offset(hw, L - k) for k in range(1, L + 1)], dtype=torch.long, device=dev)[mc]
    flat = depth_map.reshape(-1)
    zmin, zmax = [], []
    for y, x in ((ymin, xmin), (ymin, xmax), (ymax, xmin), (ymax, xmax)):
        at = torch.where(use, y * stride + x, 0)
        pix = flat[at.clamp(0, flat.numel() - 1)]
        row = mips[(off + at).clamp(0, mips.size(0) - 1)]
        zmin.append(torch.where(mc > 0, row[:, 0], pix))
        zmax.append(torch.where(mc > 0, row[:, 1], pix))
    sig = _f32(float(sigma), dev)
    z0 = torch.fmin(torch.fmin(zmin[0], zmin[1]), torch.fmin(zmin[2], zmin[3])) - sig
    z1 = torch.fmax(torch.fmax(zmax[0], zmax[1]), torch.fmax(zmax[2], zmax[3])) + 2.0 * sig
    keep = torch.where(use, (z0 <= hi[:, 2]) & (lo[:, 2] <= z1), ~(outside & ~inside))
    state = torch.where(use, torch.where(z0 > hi[:, 2], 0, torch.where(z1 < lo[:, 2], 1, 2)),
                        torch.where(outside & ~inside, 1, 2))
    return keep.int(), state.int()


def oracleB_final(points, level, sigma, cam, depth_map):
    if float(sigma) == 0.0:
        raise ValueError("oracleB_final: sigma can't be zero")
    return _in_chunks(lambda p: _oracleB_final(p, level, sigma, cam, depth_map), points.size(0), points)


def _oracleB_final(points, level, sigma, cam, depth_map):
    dev, n = points.device, points.size(0)
    level = int(level)
    if level == 0 or n == 0:
        return (torch.ones(n, dtype=torch.int32, device=dev), torch.full((n,), 2, dtype=torch.int32, device=dev),
                torch.zeros(n, dtype=torch.float32, device=dev))
    h, w = depth_map.shape
    q = _corners(points, _mat(cam, level, dev))
    scale = _f32(3.0, dev) / _f32(float(sigma), dev)
    flat = depth_map.reshape(-1)
    inb = (q[..., 0] >= 0) & (q[..., 0] < w) & (q[..., 1] >= 0) & (q[..., 1] < h) & (q[..., 2] > _f32(_NEAR, dev))
    x, y = torch.where(inb, q[..., 0], 0.0).long(), torch.where(inb, q[..., 1], 0.0).long()
    d = flat[y * w + x]
    prob = torch.where(inb, _profile(scale * (q[..., 2] - d)), 0.5)                  # (n, 8)
    pmin, pmax = prob.min(dim=1).values, prob.max(dim=1).values
    empty, unseen = pmax == 0.0, (pmin == 0.5) & (pmax == 0.5)
    occ = ~(empty | unseen)
    state = torch.where(empty, 0, torch.where(unseen, 1, 2))
    return occ.int(), state.int(), prob[:, 0].contiguous()


def colorsB_final(points, level, cam, sigma, image, depth_map, probabilities):
    if not float(sigma) > 0.0:
        raise ValueError('colorsB_final: sigma must be strictly positive')
    return _in_chunks(lambda p, pr: _colorsB_final(p, level, cam, sigma, image, depth_map, pr), points.size(0), points,
                      probabilities)


def _colorsB_final(points, level, cam, sigma, image, depth_map, probabilities):
    dev, n = points.device, points.size(0)
    h, w = depth_map.shape
    T = _mat(cam, level, dev)
    Q = _origin(points, T)
    qx, qy, qz = Q[:, 0] / Q[:, 2], Q[:, 1] / Q[:, 2], Q[:, 2]
    scale = _f32(1.0, dev) / _f32(float(sigma), dev)
    inb = (qx >= 1.0) & (qx < w - 1) & (qy >= 1.0) & (qy < h - 1) & (qz > _f32(_NEAR, dev))
    x, y = torch.where(inb, qx, 1.0).long(), torch.where(inb, qy, 1.0).long()
    flat = depth_map.reshape(-1)
    at = y * w + x
    rgb = image.reshape(-1, 3)[at]
    byte = torch.where(rgb > 0, (255.0 * rgb).clamp(max=255.0), 0.0).long()          # truncated, saturated, NaN -> 0
    du = 0.5 * (flat[at + 1] - flat[at - 1])
    dv = 0.5 * (flat[at + w] - flat[at - w])
    dprob = _profile_derivative(scale * (qz - flat[at]))
    zi = 1.0 / qz
    wgt = (scale * dprob) * zi
    hz = (wgt * zi) * ((qz * qz + Q[:, 0] * du) + Q[:, 1] * dv)
    hx, hy = (-wgt) * du, (-wgt) * dv
    g = torch.stack([(T[r, 0] * hx + T[r, 1] * hy) + T[r, 2] * hz for r in range(3)], dim=1)
    length = _sqrt((g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2])
    normal = g / length[:, None]
    normal = torch.where(torch.isfinite(normal).all(dim=1, keepdim=True), normal, 0.0)
    surface = inb & (probabilities != 0.0) & (probabilities != 0.5)
    colors = torch.full((n, 4), 64, dtype=torch.long, device=dev)
    colors[inb & (probabilities == 0.0)] = 0
    bgr0 = torch.cat([byte.flip(1), torch.zeros((n, 1), dtype=torch.long, device=dev)], dim=1)
    colors = torch.where(surface[:, None], bgr0, colors)
    normals = torch.where(surface[:, None], normal, 0.0)
    return colors.byte(), normals.float().contiguous()


def inclusive_sum(inputs):
    return torch.cumsum(inputs, 0).int()


def _kept(insum, n, npass):
    """the rows whose scan steps, with their slots (a slot outside [0, pass) is skipped)"""
    slot = torch.cat([insum.new_zeros(1), insum[:n - 1]]).long() if n > 0 else insum.long()
    keep = (slot != insum[:n].long()) & (slot >= 0) & (slot < npass)
    idx = torch.nonzero(keep).reshape(-1)
    return idx, slot[idx]


def _pass(fn, insum, n):
    npass = int(insum[n - 1]) if n > 0 else 0
    if not 0 <= npass <= n:
        raise ValueError(f'{fn}: insum ends at {npass} for {n} points: not an inclusive sum of 0 / 1 flags')
    return npass


def subdivide(points, insum):
    n, dev = points.size(0), points.device
    npass = _pass('subdivide', insum, n)
    idx, slot = _kept(insum, n, npass)
    new_points = torch.zeros((npass, 8, 3), dtype=torch.int16, device=dev)
    nvsum = torch.zeros(npass, dtype=torch.int32, device=dev)
    c = torch.arange(8, device=dev)
    offs = torch.stack([c >> 2, (c >> 1) & 1, c & 1], dim=1)
    new_points[slot] = (2 * points[idx].long()[:, None, :] + offs[None]).short()
    nvsum[slot] = idx.int()
    return new_points.reshape(-1, 3), nvsum


def compactify(points, insum):
    n, dev = points.size(0), points.device
    npass = _pass('compactify', insum, n)
    idx, slot = _kept(insum, n, npass)
    new_points = torch.zeros((npass, 3), dtype=torch.int16, device=dev)
    nvsum = torch.zeros(npass, dtype=torch.long, device=dev)
    new_points[slot] = points[idx]
    nvsum[slot] = idx
    return new_points, nvsum


def process_final_voxels(num_nodes, total_nodes, state, nvsum, occupancies, prev_state, octree, empty):
    num_nodes, total_nodes, size = int(num_nodes), int(total_nodes), octree.numel()
    if not (0 <= num_nodes <= total_nodes <= size and empty.numel() == size and occupancies.numel() == size and
            state.numel() >= 8 * num_nodes and nvsum.numel() >= num_nodes):
        raise ValueError(f'process_final_voxels: {num_nodes} nodes of {total_nodes} do not fit buffers of {size}, state of '
                         f'{state.numel()} and nvsum of {nvsum.numel()} entries')
    st = state[:8 * num_nodes].reshape(num_nodes, 8)
    o, e = bits_to_uint8(st == 2), bits_to_uint8((st == 1) | (st == 2))
    at = size - total_nodes
    octree[at:at + num_nodes] = o
    empty[at:at + num_nodes] = e
    occupancies[at:at + num_nodes] = (o != 0).int()
    up = nvsum[:num_nodes].long()
    ok = (up >= 0) & (up < prev_state.numel())
    prev_state[up[ok]] = torch.where(o != 0, 2, torch.where(e != 0, 1, 0)).int()[ok]
    return octree, empty, occupancies


def compactify_nodes(total_nodes, insum, octree, empty):
    n = int(total_nodes)
    if not 0 <= n <= min(insum.numel(), octree.numel(), empty.numel()):
        raise ValueError(f'compactify_nodes: total_nodes {n} exceeds insum, octree or empty')
    npass = _pass('compactify_nodes', insum, n)
    idx, slot = _kept(insum, n, npass)
    new_octree = torch.zeros(npass, dtype=torch.uint8, device=octree.device)
    new_empty = torch.zeros(npass, dtype=torch.uint8, device=octree.device)
    new_octree[slot] = octree[idx]
    new_empty[slot] = empty[idx]
    return new_octree, new_empty


def _identify(k, level, octree, empty, exsum):
    """k (n, 3) int64 -> (n) int64: the walk of one thread of the HIP kernels, for all points at once"""
    dev, n, nbytes = k.device, k.size(0), octree.numel()
    inside = ((k >= 0) & (k <= 2 ** level - 1)).all(dim=1)
    out = torch.full((n,), -1, dtype=torch.long, device=dev)
    if level == 0:
        return torch.where(inside, 0, -1)
    if nbytes == 0 or n == 0:
        return out
    ord_, alive = torch.zeros(n, dtype=torch.long, device=dev), inside
    for l in range(level):
        depth = level - l - 1
        child = (((k[:, 0] >> depth) & 1) << 2) | (((k[:, 1] >> depth) & 1) << 1) | ((k[:, 2] >> depth) & 1)
        alive = alive & (ord_ >= 0) & (ord_ < nbytes)
        at = ord_.clamp(0, nbytes - 1)
        bits, mpty = octree[at].long(), empty[at].long()
        hit = ((bits >> child) & 1) == 1
        unseen = alive & ~hit & (((mpty >> child) & 1) == 1)
        out = torch.where(unseen, -2 - depth, out)
        upto = bits & (torch.bitwise_left_shift(torch.full_like(child, 2), child) - 1)
        base = torch.where(at == 0, 0, exsum[(at - 1).clamp(min=0)].long())
        ord_ = torch.where(alive & hit, base + uint8_bits_sum(upto.byte()), ord_)
        alive = alive & hit
    return torch.where(alive, ord_, out)


def _merge_class(a, b):
    empty, unseen = (a == -1) | (b == -1), (a < -1) & (b < -1)
    return empty, unseen


def merge_empty(points, level, octree0, octree1, empty0, empty1, exsum0, exsum1):
    k = points.long()
    a, b = _identify(k, int(level), octree0, empty0, exsum0), _identify(k, int(level), octree1, empty1, exsum1)
    empty, unseen = _merge_class(a, b)
    return (~(empty | unseen)).int(), torch.where(empty, 0, torch.where(unseen, 1, 2)).int()


def bq_merge(points, level, octree0, octree1, empty0, empty1, pyramid0, pyramid1, probs0, probs1, colors0, colors1, normals0,
             normals1, exsum0, exsum1):
    dev, n, level = points.device, points.size(0), int(level)
    k = points.long()
    a, b = _identify(k, level, octree0, empty0, exsum0), _identify(k, level, octree1, empty1, exsum1)
    ra, rb = a - int(pyramid0[0, 1, level]), b - int(pyramid1[0, 1, level])
    ina, inb = (a >= 0) & (ra >= 0) & (ra < probs0.numel()), (b >= 0) & (rb >= 0) & (rb < probs1.numel())
    empty, unseen = _merge_class(a, b)
    empty = empty | ((a >= 0) & ~ina) | ((b >= 0) & ~inb)
    occ = ~(empty | unseen)
    half = torch.full((1,), 0.5, dtype=torch.float32, device=dev)
    p0 = torch.where(ina, torch.cat([probs0, half])[torch.where(ina, ra, probs0.numel())], 0.5)
    p1 = torch.where(inb, torch.cat([probs1, half])[torch.where(inb, rb, probs1.numel())], 0.5)
    p = (p0 * p1) / (p0 * p1 + (1.0 - p0) * (1.0 - p1))
    pad = torch.zeros((1, 4), dtype=torch.uint8, device=dev)
    c0 = torch.cat([colors0, pad])[torch.where(ina, ra, colors0.size(0))]
    c1 = torch.cat([colors1, pad])[torch.where(inb, rb, colors1.size(0))]
    colors = torch.where(occ[:, None], torch.where(ina[:, None], c0, c1), 0).byte()
    return (occ.int(), torch.where(empty, 0, torch.where(unseen, 1, 2)).int(), torch.where(occ, p, 0.0).float(), colors,
            torch.zeros((n, 3), dtype=torch.float32, device=dev))


def query_cuda_empty(octree, empty, exsum, query_coords, level):
    level = int(level)
    v = torch.floor((2 ** level) * (query_coords.double() * 0.5 + 0.5))
    ok = ((v >= -32768.0) & (v <= 32767.0)).all(dim=1)
    k = torch.where(ok[:, None], v, -1.0).long()
    return _identify(k, level, octree, empty, exsum).int()


def bf_cells_cuda(octree, empty, level):
    """Level by level from the root: the Morton codes of the occupied leaves and of every cell of an unseen block, sorted."""
    dev, level, nbytes = octree.device, int(level), octree.numel()
    if level == 0:
        return torch.zeros((1, 3), dtype=torch.int16, device=dev)
    if nbytes == 0:
        return torch.zeros((0, 3), dtype=torch.int16, device=dev)
    exsum = torch.cumsum(uint8_bits_sum(octree), 0)
    nodes = torch.zeros(1, dtype=torch.long, device=dev)
    prefix = torch.zeros(1, dtype=torch.long, device=dev)
    codes, used = [], 0
    eight = torch.arange(8, device=dev)
    for d in range(level):
        if nodes.numel() and int(nodes.max()) >= nbytes:
            raise ValueError(f'bf_cells_cuda: the octree of {nbytes} bytes is not {level} levels deep')
        used = max(used, int(nodes.max()) + 1 if nodes.numel() else 0)
        left = level - 1 - d
        bits, mpty = uint8_to_bits(octree[nodes]), uint8_to_bits(empty[nodes])
        child_code = prefix[:, None] * 8 + eight[None, :]
        unseen = child_code[mpty & ~bits]
        codes.append(((unseen[:, None] << (3 * left)) + torch.arange(8 ** left, device=dev)[None, :]).reshape(-1))
        prefix = child_code[bits]
        base = torch.where(nodes == 0, 0, exsum[(nodes - 1).clamp(min=0)])
        rank = torch.cumsum(bits.long(), dim=1)
        nodes = (base[:, None] + rank)[bits]
    codes.append(prefix)
    if used != nbytes:
        raise ValueError(f'bf_cells_cuda: {level} levels of the octree account for {used} bytes, it holds {nbytes}')
    return _torch_morton_to_points(torch.sort(torch.cat(codes)).values)


ops = types.SimpleNamespace(build_mip2d=build_mip2d, oracleB=oracleB, oracleB_final=oracleB_final, colorsB_final=colorsB_final,
                            inclusive_sum=inclusive_sum, subdivide=subdivide, compactify=compactify,
                            process_final_voxels=process_final_voxels, compactify_nodes=compactify_nodes, merge_empty=merge_empty,
                            bq_merge=bq_merge, query_cuda_empty=query_cuda_empty, bf_cells_cuda=bf_cells_cuda)
