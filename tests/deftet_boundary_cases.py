"""Scenes that put deftet_sparse_render (csrc/deftet.hip) on the boundaries of its pixel-grid pipeline: pixel counts on either
side of every grid resolution, faces of three sizes so that one call feeds the thread-per-face, the wavefront-per-face and the
workgroup-per-face kernels, crowded cells, pixels that overflow their rows, degenerate and non-finite extents, coordinates
beyond the float range, and caller-supplied boxes that are empty, inverted, NaN or too small.  Pure torch / numpy on the CPU,
seeded by torch.Generator; nothing here reads the reference.

The first half restates the dispatch rules of deftet.hip so that a test can say which kernel a face goes to; the second half
builds the scenes.  Every builder returns

    pix (B, P, 2), ranges (B, P, 2), z (B, F, 3), img (B, F, 3, 2) as float64 tensors holding float32 values, name

(`beyond_f32` alone holds values that are no float32; `boxes_given` also returns the boxes).  The caller casts.

test_deftet_boundary_cases_cpu.py checks that every case is what it claims to be; test_deftet_boundaries_gpu.py runs them
through the kernels."""
import numpy as np
import torch

MAX_GSHIFT, SMALL_CELLS, SMALL_CAND, WAVE_CELLS = 8, 16, 256, 1024      # csrc: DT_MAX_GSHIFT, DT_SMALL_*, DT_WAVE_CELLS

P_EDGES = (2048, 2049, 8192, 8193, 32768, 32769, 131072, 131073)
KH_EDGE = dict(B=2, P=8193, K=(255, 256))        # 2 * 8193 * 255 = 4 178 430 < 2^22 <= 4 194 816 = 2 * 8193 * 256
MIXED_FACES = (4, 60, 400)                       # full-extent, size 0.7, size 0.04
DEGENERATE = ('identical', 'line', 'no_finite', 'one_finite', 'wide_f32', 'beyond_f32')
DEGENERATE_DTYPES = {'wide_f32': (torch.float32,), 'beyond_f32': (torch.float64,)}      # (every other kind: both)
BEYOND_PIXELS = 50
F64 = torch.float64


# ---- the dispatch rules of deftet.hip, restated -------------------------------------------------------------------------
def gshift(P):
    """csrc: dt_gshift -- G = 2^gshift cells per axis, about 8 pixels a cell, 16 <= G <= 256"""
    g = 4
    while g < MAX_GSHIFT and (1 << (2 * g)) * 8 < P:
        g += 1
    return g


def scan_blocks(P):
    """csrc: dt_search, `nsb = kamd_cdiv(w.nc, 1024)` -- the blocks of the cell scan"""
    return max(1, 4 ** gshift(P) // 1024)


def sort_path(B, P, K):
    """csrc: dt_forward_fused, `n < 1 << 22`"""
    return 'one_pass' if B * P * K < 2 ** 22 else 'fill_then_rank'


def extent(pix_b):
    """csrc: dt_extent_kernel + dt_grid_setup -- (lo (2), hi (2)) of the pixels whose two coordinates are finite, as float32
    rounded outwards (dt_round_down / dt_round_up); (+inf, -inf) when there is none"""
    with np.errstate(over='ignore', invalid='ignore'):
        x = np.asarray(pix_b, dtype=np.float64).reshape(-1, 2)
        x = x[np.isfinite(x).all(axis=1)]
        if x.shape[0] == 0:
            return np.full(2, np.inf, np.float32), np.full(2, -np.inf, np.float32)
        lo, hi = x.min(axis=0), x.max(axis=0)
        lo32, hi32 = lo.astype(np.float32), hi.astype(np.float32)
        lo32 = np.where(lo32.astype(np.float64) > lo, np.nextafter(lo32, np.float32(-np.inf)), lo32)
        hi32 = np.where(hi32.astype(np.float64) < hi, np.nextafter(hi32, np.float32(np.inf)), hi32)
        return lo32.astype(np.float32), hi32.astype(np.float32)


def cell_inverse(lo, hi, G):
    """csrc: dt_grid_setup -- 1 / cell size per axis; a degenerate, empty or overflowing extent is one slab of size 1"""
    with np.errstate(over='ignore', invalid='ignore'):
        size = (hi - lo) / np.float32(G)
        size = np.where((size > 0) & np.isfinite(size), size, np.float32(1)).astype(np.float32)
        return (np.float32(1) / size).astype(np.float32)


def axis_cell(v, lo, inv, G):
    """csrc: dt_axis_cell, in float32: subtract, multiply by float32(1) / size, truncate, clamp (NaN -> 0)"""
    with np.errstate(over='ignore', invalid='ignore'):
        t = (np.asarray(v, dtype=np.float64).astype(np.float32) - np.float32(lo)) * np.float32(inv)
        inside = (t >= 0) & (t < np.float32(G))
        cell = np.where(inside, t, 0).astype(np.int64)
        return np.where(t >= 0, np.where(inside, cell, G - 1), 0)


def handover(pix_b, boxes_b, P):
    """csrc: dt_face_kernel -- which kernel walks the pixels of every face of one batch item.
    pix_b (P, 2), boxes_b (F, 4) = (x0, y0, x1, y1)  ->  kinds (F) of 'none' | 'thread' | 'wave' | 'group', ncell (F) int
    (0 for a face rejected before its cells are counted)"""
    pix_b = np.asarray(pix_b, dtype=np.float64).reshape(-1, 2)
    bb = np.asarray(boxes_b, dtype=np.float64).reshape(-1, 4)
    assert pix_b.shape[0] == P
    G = 1 << gshift(P)
    lo, hi = extent(pix_b)
    inv = cell_inverse(lo, hi, G)
    count = np.zeros((G, G), dtype=np.int64)                                # every pixel is counted, the non-finite ones too
    np.add.at(count, (axis_cell(pix_b[:, 1], lo[1], inv[1], G), axis_cell(pix_b[:, 0], lo[0], inv[0], G)), 1)
    total = np.zeros((G + 1, G + 1), dtype=np.int64)
    total[1:, 1:] = count.cumsum(axis=0).cumsum(axis=1)
    with np.errstate(invalid='ignore'):
        alive = (bb[:, 0] < bb[:, 2]) & (bb[:, 1] < bb[:, 3])               # an empty box or a NaN limit
        alive &= ~((bb[:, 2] <= lo[0]) | (bb[:, 0] > hi[0]) | (bb[:, 3] <= lo[1]) | (bb[:, 1] > hi[1]))
    cx0, cx1 = axis_cell(bb[:, 0], lo[0], inv[0], G), axis_cell(bb[:, 2], lo[0], inv[0], G)
    cy0, cy1 = axis_cell(bb[:, 1], lo[1], inv[1], G), axis_cell(bb[:, 3], lo[1], inv[1], G)
    ncell = (cx1 - cx0 + 1) * (cy1 - cy0 + 1)
    boxed = total[cy1 + 1, cx1 + 1] - total[cy0, cx1 + 1] - total[cy1 + 1, cx0] + total[cy0, cx0]
    cand = np.where(ncell <= SMALL_CELLS, boxed, SMALL_CAND + 1)
    kinds = np.where(cand > SMALL_CAND, np.where(ncell <= WAVE_CELLS, 'wave', 'group'), 'thread')
    kinds = np.where(alive & (cand > 0), kinds, 'none')
    return kinds, np.where(alive, ncell, 0)


def handover_counts(pix, boxes):
    """pix (B, P, 2), boxes (B, F, 4) -> dict kind -> the number of faces over the batch (counters[0] = 'wave', [1] = 'group')"""
    counts = dict(none=0, thread=0, wave=0, group=0)
    for b in range(pix.shape[0]):
        kinds, _ = handover(pix[b], boxes[b], pix.shape[1])
        for k in counts:
            counts[k] += int((kinds == k).sum())
    return counts


# ---- the scenes ---------------------------------------------------------------------------------------------------------
def r32(t):
    """float64 tensor holding float32 values"""
    return t.to(torch.float64).to(torch.float32).to(torch.float64)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, g):
    return torch.rand(shape, generator=g, dtype=F64)


def boxes_of(img):
    return torch.cat([img.min(dim=2)[0], img.max(dim=2)[0]], dim=2).contiguous()


def layered_ranges(B, P, g):
    """the depth ranges of test_deftet.layered_scene"""
    lo = -4. + _rand((B, P, 1), g)
    return torch.cat([lo, lo + 1. + 2. * _rand((B, P, 1), g)], dim=-1)


def features(B, F, D, seed=0):
    return r32(_rand((B, F, 3, D), _gen(1000 + seed)))


def upstream(shape, seed=0):
    return r32(_rand(tuple(shape), _gen(2000 + seed)))


def _blobs(B, n, size, g):
    return (_rand((B, n, 1, 2), g) * 1.6 - 0.8) + (_rand((B, n, 3, 2), g) - 0.5) * size


def mixed(B, P, seed, cluster=False, outlier=False):
    """Per batch item 4 faces over the whole extent (a triangle with corners near (-0.97, -0.95), (0.96, -0.9), (0.02, 0.97)
    and its three quarter turns, jittered by 0.01), 60 faces of size 0.7 and 400 of size 0.04 with centres in +-0.8, in random
    mesh order; z in [-4, -1]; pixels uniform in [-1, 1]^2; the ranges of layered_scene.
    cluster: three quarters of the pixels lie in a square 0.004 wide at (0.3, 0.3), and 8 of the small faces sit on it.
    outlier: one pixel of item 0 has x = 1e6."""
    g = _gen(seed)
    n_big, n_mid, n_small = MIXED_FACES
    base = torch.tensor([[-0.97, -0.95], [0.96, -0.9], [0.02, 0.97]], dtype=F64)
    turns = [base]
    for _ in range(3):
        turns.append(torch.stack([-turns[-1][:, 1], turns[-1][:, 0]], dim=1))
    big = torch.stack(turns)[None] + (_rand((B, n_big, 3, 2), g) - 0.5) * 0.02
    mid, small = _blobs(B, n_mid, 0.7, g), _blobs(B, n_small, 0.04, g)
    if cluster:
        small[:, :8] = 0.3 + (_rand((B, 8, 1, 2), g) - 0.5) * 0.02 + (_rand((B, 8, 3, 2), g) - 0.5) * 0.04
    img = torch.cat([big, mid, small], dim=1)
    F = img.shape[1]
    img = torch.stack([img[b][torch.randperm(F, generator=g)] for b in range(B)])
    z = -1. - _rand((B, F, 3), g) * 3.
    pix = _rand((B, P, 2), g) * 2. - 1.
    ranges = layered_ranges(B, P, g)
    name = f'mixed_B{B}_P{P}_s{seed}'
    if cluster:
        n = 3 * P // 4
        pix[:, :n] = 0.3 + (_rand((B, n, 2), g) - 0.5) * 0.004
        name += '_cluster'
    if outlier:
        pix[0, P // 2, 0] = 1e6
        name += '_outlier'
    return r32(pix), r32(ranges), r32(z), r32(img), name


def smallest_altitude(img):
    """(..., 3, 2) -> (...): twice the area over the longest edge"""
    a, b, c = img[..., 0, :], img[..., 1, :], img[..., 2, :]
    area2 = ((b - a)[..., 0] * (c - a)[..., 1] - (b - a)[..., 1] * (c - a)[..., 0]).abs()
    longest = torch.stack([(b - a).norm(dim=-1), (c - b).norm(dim=-1), (a - c).norm(dim=-1)]).max(dim=0)[0]
    return area2 / longest


def clean(B=2, F=300, P=700, seed=0):
    """The backward sweep's scene: faces drawn like layered_scene's (centre +-0.8, size 0.9), one whose smallest altitude is
    below 0.05 drawn again; no duplicates, no zero-area faces; z in [-4, -1]; the range (-10, 0) everywhere."""
    g = _gen(seed)
    img = r32(_blobs(B, 4 * F, 0.9, g))
    keep = smallest_altitude(img) >= 0.05
    img = torch.stack([img[b][keep[b]][:F] for b in range(B)])
    assert img.shape == (B, F, 3, 2)
    z = -1. - _rand((B, F, 3), g) * 3.
    pix = _rand((B, P, 2), g) * 2. - 1.
    ranges = torch.tensor([-10., 0.], dtype=F64).repeat(B, P, 1)
    return r32(pix), ranges, r32(z), img, f'clean_B{B}_F{F}_P{P}_s{seed}'


def degenerate(kind, seed=3):
    """The faces of `mixed` under pixels whose extent is degenerate:
    identical   P = 300, every pixel at (0.1, -0.2), the scene times 0.6: an extent of size 0, one slab, one crowded cell
    line        P = 700, every x = 0.25: one axis of size 0
    no_finite   P = 500, every pixel has a NaN or an infinite coordinate: no extent at all
    one_finite  no_finite with one pixel at the origin
    wide_f32    float only: scene and pixels times 1e36 -- hi - lo is finite, G * size is near the top of the float range
    beyond_f32  double only: one more triangle at (1e39, -1e39) and 50 pixels at and near its centroid, range (-10, 0), among
                the pixels of an ordinary scene -- the float extent is infinite on both axes"""
    assert kind in DEGENERATE
    P = dict(identical=300, line=700, no_finite=500, one_finite=500, wide_f32=3000, beyond_f32=3000)[kind]
    pix, ranges, z, img, _ = mixed(2, P, seed)
    g = _gen(seed + 50)
    if kind == 'identical':
        pix[:] = r32(torch.tensor([0.1, -0.2], dtype=F64))
        img = r32(img * 0.6)                                                # every box ends less than 1 from the pixel
    elif kind == 'line':
        pix[..., 0] = 0.25
    elif kind in ('no_finite', 'one_finite'):
        bad = torch.tensor([float('nan'), float('inf'), -float('inf')], dtype=F64)
        which = torch.randint(3, (2, P), generator=g)                       # x, y or both
        value = bad[torch.randint(3, (2, P, 2), generator=g)]
        pix[..., 0] = torch.where(which != 1, value[..., 0], pix[..., 0])
        pix[..., 1] = torch.where(which != 0, value[..., 1], pix[..., 1])
        if kind == 'one_finite':
            pix[1, P // 3] = 0.
    elif kind == 'wide_f32':
        pix, img = r32(pix * 1e36), r32(img * 1e36)
    else:
        tri = torch.tensor([[-0.3, -0.2], [0.4, -0.1], [0., 0.5]], dtype=F64) * 1e36 + torch.tensor([1e39, -1e39], dtype=F64)
        near = tri.mean(dim=0) + (_rand((2, BEYOND_PIXELS, 2), g) - 0.5) * 1e34
        near[:, 0] = tri.mean(dim=0)
        img = torch.cat([img[:, :200], tri.expand(2, 1, 3, 2), img[:, 200:]], dim=1)
        z = torch.cat([z[:, :200], torch.tensor([-2., -2.5, -3.], dtype=F64).expand(2, 1, 3), z[:, 200:]], dim=1)
        where = torch.randperm(P + BEYOND_PIXELS, generator=g)
        pix = torch.cat([pix, near], dim=1)[:, where]
        ranges = torch.cat([ranges, torch.tensor([-10., 0.], dtype=F64).expand(2, BEYOND_PIXELS, 2)], dim=1)[:, where]
    return pix.contiguous(), ranges.contiguous(), z.contiguous(), img.contiguous(), f'degenerate_{kind}'


BEYOND_FACE = 200                                # the index of beyond_f32's triangle


def boxes_given(seed=4):
    """mixed(2, 3000) with boxes that are not the faces' own (the C operator takes them from the caller): of every five faces
    the first has a NaN limit (each of the four in turn), the second x0 and x1 swapped, the third its max corner pulled to the
    centre of its box; face 3 has x0 == x1.  -> pix, ranges, z, img, boxes, name"""
    pix, ranges, z, img, name = mixed(2, 3000, seed)
    bb = boxes_of(img)
    F = bb.shape[1]
    for f in range(0, F, 5):
        bb[:, f, (f // 5) % 4] = float('nan')
    swap = bb[:, 1::5].clone()
    bb[:, 1::5, 0], bb[:, 1::5, 2] = swap[..., 2], swap[..., 0]
    third = bb[:, 2::5].clone()
    bb[:, 2::5, 2:] = r32((third[..., :2] + third[..., 2:]) * 0.5)
    bb[:, 3, 2] = bb[:, 3, 0]
    return pix, ranges, z, img, bb.contiguous(), name + '_boxes_given'


def hit_counts(face_idx):
    """face_idx (B, P, K) of the forward operator -> hits per pixel (B, P)"""
    return (face_idx != -1).sum(dim=-1)
