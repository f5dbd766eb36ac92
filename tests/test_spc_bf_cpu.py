"""The Bayesian-fusion operators (``_C.ops.spc`` of csrc/spc_bf.hip), ``ops.spc.bf_recon`` and ``ops.gaussians.sample_points_in_volume``
through the torch formulations that CPU tensors take; tests/test_spc_bf_gpu.py runs the same cases through the HIP path.

* every operator equals the numpy restatement of tests/spc_bf_bruteforce.py, ``torch.equal`` on every output -- integers,
  probabilities, colours and normals alike, the arithmetic contract being bit-defined;
* the float32 restatement is pinned by its float64 evaluation (test_float32_decisions_are_pinned_by_float64);
* pins that do not restate the reference's code: the assembled octree is the octree of its own occupied points, the empty-aware
  query agrees with a dense expansion of the tree, bf_cells equals the dense-query form, fuseBF is idempotent and symmetric;
* one frame of a sphere shell carves what geometry says, and sample_points_in_volume fills a sphere of Gaussians solid."""
import functools
import logging
import math

import numpy as np
import pytest
import torch

import spc_bf_bruteforce as bf
import kaolin_amd as kal
from kaolin_amd import _C
from kaolin_amd.ops.gaussians import densifier
from kaolin_amd.ops.spc import bf_recon as bfr
from kaolin_amd.ops.spc import bf_torch
from kaolin_amd.ops.spc.raytraced_spc_dataset import RayTracedSPCDataset, _camera_matrices, _pinhole

MAX_DEPTH = float(np.finfo(np.float32).max)
SIGMA = 0.05                # wide enough for the profile curve to be hit between its ends at these resolutions
COUNTS = [0, 1, 255, 256, 257, 1025]       # around the 256-thread blocks of the per-point kernels and the 1024 of the scan


def ops(device):
    return _C.ops.spc if device == 'cuda' else bf_torch.ops


def t(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def eq(got, want):
    want = torch.from_numpy(np.ascontiguousarray(want))
    got = got.cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype, got.shape, want.shape)
    assert torch.equal(got, want), f'{int((got != want).sum())} of {want.numel()} entries differ'


# ---- scenes: a pinhole view of a sphere of radius 0.6 at the origin, depth = ray length to it, max_depth where the ray misses ----
# (the cameras aim a little off the lattice points of the cube, so that no cell corner projects onto a pixel boundary exactly)
SCENES = {
    # name: (res, mip_levels, eye, at, fov)
    'front32': (32, 3, (4.0, 0.3, 0.2), (0.013, -0.021, 0.017), 0.644),         # the cube about fills the image: every oracleB branch but two
    'cell64': (64, 6, (3.5, 0.55, 0.45), (0.513, 0.487, 0.509), 0.42),         # a level-1 cell spans more than half the image: miplevel 6
    'inside32': (32, 3, (0.9, 0.2, 0.1), (0.011, 0.023, -0.019), 0.644),        # the eye inside the cube: cells behind the near plane
    'oblique32': (32, 3, (2.4, 2.1, 1.9), (-0.017, 0.012, 0.021), 0.644),
}


@functools.lru_cache(maxsize=None)
def scene(name, true_depth=True):
    res, L, eye, at, fov = SCENES[name]
    view, fx, fy, cx, cy, origins, dirs = _pinhole(eye, at, (0.0, 0.0, 1.0), fov, res, 'cpu')
    Cam, In = _camera_matrices(view, fx, fy, cx, cy)
    o, d = origins.double().numpy(), dirs.double().numpy()
    b = (o * d).sum(1)
    disc = b * b - ((o * o).sum(1) - 0.6 ** 2)
    length = np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), MAX_DEPTH)
    raw = np.where((disc > 0) & (length > 0), length, MAX_DEPTH).astype(np.float32).reshape(res, res)
    rng = np.random.RandomState(res)
    image = rng.rand(res, res, 3).astype(np.float32)
    mips, depth = bf.build_mip2d(raw, In.numpy(), L, MAX_DEPTH, true_depth)
    return dict(res=res, L=L, cam=Cam, intrinsics=In, raw=raw, depth=depth, mips=mips, image=image, true_depth=true_depth)


def level_points(level, count=None, seed=0):
    """the dense points of a level in Morton order, or ``count`` of them at random (with repeats when the level has fewer)"""
    n = 8 ** level
    codes = np.arange(n) if count is None else np.random.RandomState(seed + 31 * level).randint(0, n, count)
    return kal.ops.spc.morton_to_points(torch.from_numpy(np.asarray(codes, dtype=np.int64))).numpy().reshape(-1, 3)


def check_build_mip2d(device, name, true_depth):
    s = scene(name, true_depth)
    depth = t(s['raw'].copy(), device)
    mips = ops(device).build_mip2d(depth, s['intrinsics'], s['L'], MAX_DEPTH, true_depth)
    eq(mips, s['mips'])
    eq(depth, s['depth'])                      # converted in place (or left alone)
    missed = s['raw'] == np.float32(MAX_DEPTH)
    assert missed.any() and (depth.cpu().numpy()[missed] == np.float32(MAX_DEPTH)).all()       # max_depth pixels are left alone
    assert (depth.cpu().numpy()[~missed] != s['raw'][~missed]).any() == true_depth
    hw = (s['res'] >> s['L']) ** 2
    assert mips.shape[0] == hw * (4 ** s['L'] - 1) // 3


def check_oracleB(device, name, level, points, sigma=SIGMA):
    s = scene(name)
    want = bf.oracleB(points, level, sigma, s['cam'].numpy(), s['depth'], s['mips'], s['L'])
    occ, state = ops(device).oracleB(t(points, device), level, sigma, s['cam'], t(s['depth'], device), t(s['mips'], device), s['L'])
    eq(occ, want[0])
    eq(state, want[1])
    return want


def check_final(device, name, level, points, sigma=SIGMA):
    s = scene(name)
    o = ops(device)
    depth = t(s['depth'], device)
    want = bf.oracleB_final(points, level, sigma, s['cam'].numpy(), s['depth'])
    occ, state, probs = o.oracleB_final(t(points, device), level, sigma, s['cam'], depth)
    eq(occ, want[0])
    eq(state, want[1])
    eq(probs, want[2])
    if level > 0:
        wc, wn = bf.colorsB_final(points, level, s['cam'].numpy(), sigma, s['image'], s['depth'], want[2])
        colors, normals = o.colorsB_final(t(points, device), level, s['cam'], sigma, t(s['image'], device), depth, probs)
        eq(colors, wc)
        eq(normals, wn)
        return want, wc, wn
    return want, None, None


def oracleB_cases():
    """(scene, level, points): the dense levels 1 to 4 and 1025 points of level 5, from every scene"""
    for name in SCENES:
        for level in range(1, 6):
            yield name, level, level_points(level) if level < 5 else level_points(5, 1025, 1)


def check_degenerate_cams(device):
    """A cam that makes a coordinate NaN at every corner (a zero matrix: 0 / 0) leaves no extent to test: every voxel is kept,
    no pixel is read.  A cam with a non-finite entry is refused before any launch."""
    s = scene('front32')
    o = ops(device)
    points = level_points(3)
    depth, mips = t(s['depth'], device), t(s['mips'], device)
    for cam in (torch.zeros(4, 4), torch.diag(torch.tensor([0.0, 1.0, 1.0, 1.0]))):
        want = bf.oracleB(points, 3, SIGMA, cam.numpy(), s['depth'], s['mips'], s['L'])
        occ, state = o.oracleB(t(points, device), 3, SIGMA, cam, depth, mips, s['L'])
        eq(occ, want[0])
        eq(state, want[1])
        wf = bf.oracleB_final(points, 3, SIGMA, cam.numpy(), s['depth'])
        for got, w in zip(o.oracleB_final(t(points, device), 3, SIGMA, cam, depth), wf):
            eq(got, w)
    assert (bf.oracleB(points, 3, SIGMA, np.zeros((4, 4), np.float32), s['depth'], s['mips'], s['L'])[0] == 1).all()
    for bad in (float('nan'), float('inf')):
        cam = s['cam'].clone()
        cam[2, 0] = bad
        with pytest.raises(ValueError):
            o.oracleB(t(points, device), 3, SIGMA, cam, depth, mips, s['L'])
        with pytest.raises(ValueError):
            o.oracleB_final(t(points, device), 3, SIGMA, cam, depth)
        with pytest.raises(ValueError):
            o.colorsB_final(t(points, device), 3, cam, SIGMA, t(s['image'], device), depth, torch.zeros(len(points), device=device))


def check_scan_ops(device, n):
    """inclusive_sum, subdivide, compactify and compactify_nodes on n flags"""
    o = ops(device)
    rng = np.random.RandomState(n)
    flags = (rng.rand(n) < 0.4).astype(np.int32)
    if n > 0:
        flags[-1] = 1
    pts = level_points(4, n, 2).astype(np.int16)
    insum = o.inclusive_sum(t(flags, device))
    eq(insum, bf.inclusive_sum(flags))
    big = (rng.randint(0, 1000, n)).astype(np.int32)
    eq(o.inclusive_sum(t(big, device)), bf.inclusive_sum(big))
    for name in ('subdivide', 'compactify'):
        got = getattr(o, name)(t(pts, device), insum)
        want = getattr(bf, name)(pts, bf.inclusive_sum(flags))
        eq(got[0], want[0])
        eq(got[1], want[1])
    octree, empty = rng.randint(0, 256, n).astype(np.uint8), rng.randint(0, 256, n).astype(np.uint8)
    got = o.compactify_nodes(n, insum, t(octree, device), t(empty, device))
    want = bf.compactify_nodes(n, bf.inclusive_sum(flags), octree, empty)
    eq(got[0], want[0])
    eq(got[1], want[1])


def check_process_final_voxels(device, num_nodes):
    o = ops(device)
    rng = np.random.RandomState(num_nodes + 7)
    total, size, prev = num_nodes + 5, num_nodes + 11, num_nodes + 3
    state = rng.randint(0, 3, 8 * num_nodes).astype(np.int32)
    state[:8] = 0
    nvsum = rng.permutation(prev)[:num_nodes].astype(np.int32)
    bufs = [rng.randint(0, 256, size).astype(np.uint8), rng.randint(0, 256, size).astype(np.uint8),
            rng.randint(0, 2, size).astype(np.int32), rng.randint(0, 3, prev).astype(np.int32)]
    want = bf.process_final_voxels(num_nodes, total, state, nvsum, bufs[2], bufs[3], bufs[0], bufs[1])
    octree, empty, occ, prev_state = (t(b.copy(), device) for b in bufs)
    out = o.process_final_voxels(num_nodes, total, t(state, device), t(nvsum, device), occ, prev_state, octree, empty)
    for got, w in zip((octree, empty, occ, prev_state), want):
        eq(got, w)                                                        # written in place, the rest of the buffers untouched
    assert out[0] is octree and out[1] is empty and out[2] is occ


# ---- hand-built trees ---------------------------------------------------------------------------------------------------------------
def build_tree(level, seed, p_occ=0.45, p_unseen=0.25, unseen=True):
    """A random (octree, empty) of ``level`` levels, breadth first.  With ``unseen`` the first node of every level has bit 0
    occupied and bit 7 unseen: an unseen block at every depth."""
    rng = np.random.RandomState(seed)
    octree, empty, nodes = [], [], 1
    for d in range(level):
        nxt = 0
        for i in range(nodes):
            r = rng.rand(8)
            o = sum(1 << c for c in range(8) if r[c] < p_occ)
            e = sum(1 << c for c in range(8) if p_occ <= r[c] < p_occ + p_unseen) if unseen else 0
            if i == 0:
                o |= 1
                if unseen:
                    o &= ~128
                    e |= 128
            octree.append(o)
            empty.append(e | o)
            nxt += bin(o).count('1')
        nodes = nxt
    return np.array(octree, dtype=np.uint8), np.array(empty, dtype=np.uint8)


def dense_states(octree, empty, level):
    """the answer of the empty-aware query for every cell of the 2^level cube, by recursive region fill"""
    ex = bf.exsum_of(octree)
    cube = np.full((1 << level,) * 3, -1, dtype=np.int64)

    def fill(node, d, x, y, z):
        left = level - 1 - d
        for c in range(8):
            cx, cy, cz = 2 * x + (c >> 2), 2 * y + ((c >> 1) & 1), 2 * z + (c & 1)
            block = tuple(slice(v << left, (v + 1) << left) for v in (cx, cy, cz))
            if (octree[node] >> c) & 1:
                child = (int(ex[node - 1]) if node else 0) + bin(int(octree[node]) & ((2 << c) - 1)).count('1')
                if left == 0:
                    cube[block] = child
                else:
                    fill(child, d + 1, cx, cy, cz)
            elif (empty[node] >> c) & 1:
                cube[block] = -2 - left
    fill(0, 0, 0, 0, 0)
    return cube


def check_query(device, level, seed):
    octree, empty = build_tree(level, seed)
    cube = dense_states(octree, empty, level)
    assert {-2 - d for d in range(level)} <= set(np.unique(cube).tolist())          # an unseen block at every depth
    to, te = t(octree, device), t(empty, device)
    _, pyramid, exsum = kal.ops.spc.scan_octrees(to, torch.tensor([len(octree)], dtype=torch.int32))
    cells = kal.ops.spc.morton_to_points(torch.arange(8 ** level, device=device))
    got = bfr.unbatched_query(to, te, exsum, cells, level)
    c = cells.cpu().numpy().astype(np.int64)
    want = cube[c[:, 0], c[:, 1], c[:, 2]]
    assert got.dtype == torch.long
    eq(got, want)
    plain = kal.ops.spc.unbatched_query(to, exsum, cells, level).cpu().numpy()
    assert (plain[want >= 0] == want[want >= 0]).all() and (plain[want < 0] == -1).all()
    # float coordinates of every supported type, and coordinates outside the cube
    centres = (c + 0.5) / 2 ** (level - 1) - 1.0
    for dtype in (torch.float16, torch.float32, torch.float64):
        if dtype == torch.float16 and level > 3:
            continue                                            # (half cannot hold the cell centres of deeper levels)
        eq(bfr.unbatched_query(to, te, exsum, torch.from_numpy(centres).to(device=device, dtype=dtype), level), want)
    outside = torch.tensor([[-1.5, 0, 0], [0, 1.0, 0], [0, 0, 7.0], [float('nan'), 0, 0], [1e30, 0, 0]], device=device)
    assert (bfr.unbatched_query(to, te, exsum, outside, level) == -1).all()
    # the operator against the numpy walk
    eq(ops(device).query_cuda_empty(to, te, exsum, torch.from_numpy(centres).float().to(device), level),
       bf.query_empty(octree, empty, bf.exsum_of(octree), centres.astype(np.float32), level))
    return octree, empty, cube


def dense_cells(octree, empty, level, device):
    """the reference's final step: every cell of the level queried, the empty ones dropped"""
    to, te = t(octree, device), t(empty, device)
    cells = kal.ops.spc.morton_to_points(torch.arange(8 ** level, dtype=torch.long, device=device))
    if len(octree) == 0:
        return cells[:0]
    _, _, exsum = kal.ops.spc.scan_octrees(to, torch.tensor([len(octree)], dtype=torch.int32))
    return cells[bfr.unbatched_query(to, te, exsum, cells, level) != -1]


def check_cells(device, octree, empty, level):
    got = ops(device).bf_cells_cuda(t(octree, device), t(empty, device), level)
    want = dense_cells(octree, empty, level, device)
    assert got.dtype == torch.int16 and torch.equal(got, want), (got.shape, want.shape)
    return got


def check_merges(device, level, n=None):
    """merge_empty and bq_merge of two random trees at the dense points of the level (or n of them)"""
    o = ops(device)
    trees = []
    for seed in (level, level + 50):
        octree, empty = build_tree(level, seed)
        ex = bf.exsum_of(octree)
        rows = sum(bin(int(b)).count('1') for b in octree[_level_start(octree, level - 1):])      # the points of the level
        rng = np.random.RandomState(seed)
        trees.append(dict(octree=octree, empty=empty, exsum=ex, rows=rows,
                          probs=rng.rand(rows).astype(np.float32), colors=rng.randint(0, 256, (rows, 4)).astype(np.uint8)))
    pts = level_points(level) if n is None else level_points(level, n, 5)
    tt = []
    for tr in trees:
        to = t(tr['octree'], device)
        lvl, pyramid, exsum = kal.ops.spc.scan_octrees(to, torch.tensor([len(tr['octree'])], dtype=torch.int32))
        assert lvl == level and int(pyramid[0, 0, level]) == tr['rows']
        tr['offset'] = int(pyramid[0, 1, level])
        tt.append((to, t(tr['empty'], device), exsum, pyramid, t(tr['probs'], device), t(tr['colors'], device),
                   torch.zeros((tr['rows'], 3), device=device)))
    a, b = tt
    np_trees = [(tr['octree'], tr['empty'], tr['exsum']) for tr in trees]
    for l in range(1, level + 1):
        p = level_points(l) if n is None else level_points(l, n, 5)
        occ, state = o.merge_empty(t(p, device), l, a[0], b[0], a[1], b[1], a[2], b[2])
        want = bf.merge_empty(p, l, *np_trees)
        eq(occ, want[0])
        eq(state, want[1])
    got = o.bq_merge(t(pts, device), level, a[0], b[0], a[1], b[1], a[3], b[3], a[4], b[4], a[5], b[5], a[6], b[6], a[2], b[2])
    want = bf.bq_merge(pts, level, np_trees[0], np_trees[1], trees[0]['offset'], trees[1]['offset'], trees[0]['probs'],
                       trees[1]['probs'], trees[0]['colors'], trees[1]['colors'])
    for g, w in zip(got[:4], want):
        eq(g, w)
    assert got[4].shape == (len(pts), 3) and got[4].dtype == torch.float32 and not got[4].any()       # normals: all zero
    unoccupied = got[0] == 0
    assert not got[2][unoccupied].any() and not got[3][unoccupied].any()                               # unoccupied rows are zero
    return want


def _level_start(octree, d):
    """the first byte of level d of a breadth-first octree"""
    start, count = 0, 1
    for _ in range(d):
        below = sum(bin(int(b)).count('1') for b in octree[start:start + count])
        start, count = start + count, below
    return start


# ---- frames -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shell_octree(level=6, radius=0.5):
    """the octree of the cells of ``level`` that a sphere shell of ``radius`` crosses (analytic points)"""
    n = 200000
    i = np.arange(n) + 0.5
    phi, theta = np.arccos(1 - 2 * i / n), math.pi * (1 + 5 ** 0.5) * i
    pts = radius * np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=1)
    cells = np.unique(np.floor((pts + 1) * 2 ** (level - 1)).astype(np.int16), axis=0)
    return kal.ops.spc.unbatched_points_to_octree(torch.from_numpy(cells), level, sorted=False)


def frames(device, viewpoints, res, level=6, radius=0.5):
    octree = shell_octree(level, radius).to(device)
    return RayTracedSPCDataset(torch.tensor(viewpoints, dtype=torch.float32), octree, res=res)


def spc_level_points(octree, level):
    """the points of ``level`` of an octree, as an int64 array"""
    _, pyramid, exsum = kal.ops.spc.scan_octrees(octree, torch.tensor([len(octree)], dtype=torch.int32))
    pts = kal.ops.spc.generate_points(octree, pyramid, exsum)
    return pts[int(pyramid[0, 1, level]):int(pyramid[0, 1, level + 1])].cpu().numpy().astype(np.int64)


def spc_points(spc, level):
    """the occupied points of ``level`` of a processFrame / fuseBF result"""
    pts = kal.ops.spc.generate_points(spc['octree'], spc['pyramid'], spc['exsum'])
    return pts[int(spc['pyramid'][0, 1, level]):int(spc['pyramid'][0, 1, level + 1])]


def check_octree_pin(device, res=6):
    """(a) after process_final_voxels and compactify_nodes the octree is the octree of its own occupied final-level points"""
    ds = frames(device, [[4.0, 0.0, 0.0], [2.3, 2.3, 2.3]], res)
    out = []
    for k in range(2):
        spc = bfr.processFrame(ds[k], 6, 0.0005)
        assert spc['level'] == 6                                           # scan_octrees accepted it, at the right depth
        pts = spc_points(spc, 6)
        assert torch.equal(kal.ops.spc.unbatched_points_to_octree(pts, 6), spc['octree'])
        assert spc['empty'].shape == spc['octree'].shape and ((spc['empty'] & spc['octree']) == spc['octree']).all()
        assert spc['probabilities'].shape == (len(pts),) and spc['colors'].shape == (len(pts), 4) and \
            spc['normals'].shape == (len(pts), 3)
        out.append(spc)
    return out


def check_fuse_laws(device, spcs):
    """(d) fuseBF of a frame with itself returns the frame's octree and empty; fuseBF(a, b) and fuseBF(b, a) agree in both"""
    a, b = spcs
    aa = bfr.fuseBF(a, a)
    assert torch.equal(aa['octree'], a['octree']) and torch.equal(aa['empty'], a['empty'])
    ab, ba = bfr.fuseBF(a, b), bfr.fuseBF(b, a)
    assert torch.equal(ab['octree'], ba['octree']) and torch.equal(ab['empty'], ba['empty'])
    assert len(ab['octree']) > 0 and not torch.equal(ab['empty'], a['empty'])
    assert torch.equal(kal.ops.spc.unbatched_points_to_octree(spc_points(ab, 6), 6), ab['octree'])
    return ab


def check_frame_geometry(device, res=8, level=6, sigma=0.0005, radius=0.3):
    """One view from (4, 0, 0) of the level-6 shell of a sphere.  Among the final-level cells whose eight corners project inside
    the image: a cell wholly in front of (or beside) the shell is empty, a cell wholly behind its near side -- inside the sphere or
    in its shadow -- is unseen, and the cells at the surface are occupied: every front-most voxel of the shell on a pixel's ray (the
    visible crust).  A voxel of the shell that another one hides is unseen by the method, so the cells that the sphere passes
    through on the eye's side are, as a whole, only never empty.

    Margins.  The depth map holds the distance to the VOXELISED shell: the cells the sphere crosses, all within one cell diagonal
    ``diag`` of it, a closed surface around the ball of radius ``radius - diag``.  The depth under a corner is taken at the centre
    of its pixel, whose ray passes within a footprint ``foot = distance / focal`` (times sqrt 2, rounded up to 2) of the corner.  So
    a corner is surely seen as free space when the segment from the eye to it stays ``radius + diag + 2 foot + 3 sigma`` clear of
    the centre, and surely as hidden when the segment enters the ball of radius ``radius - diag - 2 foot - 3 sigma`` (the ray has
    then crossed the shell, by more than the 2 sigma the profile curve needs).  A cell is judged when all eight corners agree;
    the cells in between are not judged, and they may be at most 10 % of the in-image cells."""
    ds = frames(device, [[4.0, 0.0, 0.0]], res, level, radius)
    batch = ds[0]
    ray_length = batch[1].clone().reshape(-1).double().cpu().numpy()          # (processFrame converts the map in place)
    spc = bfr.processFrame(batch, level, sigma)
    cells = kal.ops.spc.morton_to_points(torch.arange(8 ** level, device=device))
    state = bfr.unbatched_query(spc['octree'], spc['empty'], spc['exsum'], cells, level).cpu().numpy()
    cell = 2.0 / 2 ** level
    diag = cell * math.sqrt(3)
    lo = cells.cpu().numpy().astype(np.float64) * cell - 1.0                 # the cells' low corners
    corners = lo[:, None, :] + cell * np.array([[c >> 2, (c >> 1) & 1, c & 1] for c in range(8)])[None]
    focal = 2 ** res / (2 * math.tan(0.644 / 2))
    zc = 4.0 - corners[..., 0]                                                # depth along the view axis (the eye is on +x)
    u, v = corners[..., 1] / zc * focal, corners[..., 2] / zc * focal
    in_image = (np.abs(u).max(1) < 2 ** res / 2) & (np.abs(v).max(1) < 2 ** res / 2)
    foot = 4.0 / focal
    margin = diag + 2 * foot + 3 * sigma
    eye = np.array([4.0, 0.0, 0.0])
    seg = corners - eye
    along = np.clip(-(seg * eye).sum(-1) / (seg * seg).sum(-1), 0.0, 1.0)     # the point of the segment closest to the centre
    clearance = np.linalg.norm(eye + along[..., None] * seg, axis=-1)
    empty_sure = in_image & (clearance.min(1) > radius + margin)
    unseen_sure = in_image & (clearance.max(1) < radius - margin)
    rc = np.linalg.norm(corners, axis=-1)
    # the cells the sphere passes through, a quarter of a cell clear of their corners, on the side of the eye: voxels of the shell
    crossing = in_image & (lo[:, 0] > 0) & (rc.min(1) < radius - 0.25 * cell) & (rc.max(1) > radius + 0.25 * cell)
    # the visible crust: the front-most voxel of the shell on every pixel's ray, from the shell's own ray traced depths -- the
    # cell that holds the point just behind the ray's first hit
    _, _, _, _, _, origins, dirs = _pinhole(eye, (0.0, 0.0, 0.0), (0.0, 0.0, 1.0), 0.644, 2 ** res, 'cpu')
    hit_ray = ray_length < 1e30
    entry = origins.double().numpy()[hit_ray] + dirs.double().numpy()[hit_ray] * (ray_length[hit_ray, None] + 1e-4)
    crust_cells = np.unique(np.floor((entry + 1.0) / cell).astype(np.int64), axis=0)
    shell = set(map(tuple, spc_level_points(shell_octree(level, radius), level).tolist()))
    assert all(tuple(c) in shell for c in crust_cells.tolist())              # (they are voxels of the shell indeed)
    code = cells.cpu().numpy().astype(np.int64) @ np.array([4096, 64, 1])
    crust = in_image & np.isin(code, crust_cells @ np.array([4096, 64, 1]))
    surface = crossing | crust
    unjudged = in_image & ~(empty_sure | unseen_sure | surface)
    print(f'in image {in_image.sum()}, empty {empty_sure.sum()}, unseen {unseen_sure.sum()}, crust {crust.sum()}, crossing '
          f'{crossing.sum()} ({(state[crossing] >= 0).sum()} occupied), unjudged {unjudged.sum()} ({unjudged.sum() / in_image.sum():.3f})')
    assert (state[empty_sure] == -1).all(), (state[empty_sure] != -1).sum()
    assert (state[unseen_sure] < -1).all(), (state[unseen_sure] >= -1).sum()
    assert (state[crust] >= 0).all(), (state[crust] < 0).sum()               # every cell of the visible crust is occupied
    assert (state[crossing] != -1).all(), (state[crossing] == -1).sum()      # a hidden voxel of the shell may be unseen, not empty
    assert empty_sure.sum() > 1000 and unseen_sure.sum() > 1000 and crust.sum() > 250 and crossing.sum() > 250
    assert unjudged.sum() <= 0.10 * in_image.sum()


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('true_depth', [False, True])
@pytest.mark.parametrize('name', ['front32', 'cell64'])
def test_build_mip2d(name, true_depth):
    check_build_mip2d('cpu', name, true_depth)
    assert (scene(name)['raw'] == np.float32(MAX_DEPTH)).any()              # pixels equal to max_depth are there, and stay


def test_oracleB_equals_the_oracle_on_every_branch():
    seen = set()
    for name, level, points in oracleB_cases():
        want = check_oracleB('cpu', name, level, points)
        seen |= set(want[2].tolist())
    assert seen >= {'mip0', 'mid', 'top', 'high', 'straddle', 'outside', 'behind'}, seen
    assert set(bf.oracleB(level_points(1), 1, SIGMA, scene('cell64')['cam'].numpy(), scene('cell64')['depth'],
                          scene('cell64')['mips'], 6)[2].tolist()) >= {'top'}          # miplevel 6 on the 64 x 64 map


@pytest.mark.parametrize('name', list(SCENES))
def test_final_operators_equal_the_oracle(name):
    states = set()
    for level in range(1, 6):
        want, colors, normals = check_final('cpu', name, level, level_points(level) if level < 5 else level_points(5, 1025, 1))
        states |= set(want[1].tolist())
    if name == 'front32':
        assert states == {0, 1, 2}
        assert np.abs(normals).sum() > 0 and (colors[:, 3] == 0).any()


@pytest.mark.parametrize('n', COUNTS)
def test_point_counts_around_the_blocks(n):
    points = level_points(5, n, 3)
    occ, state, _, _ = check_oracleB('cpu', 'front32', 5, points)
    assert occ.shape == (n,) and occ.dtype == np.int32
    check_final('cpu', 'front32', 5, points)
    check_scan_ops('cpu', n)
    check_process_final_voxels('cpu', n)


def test_degenerate_cams():
    check_degenerate_cams('cpu')


def test_level_zero_is_occupied():
    s = scene('front32')
    root = torch.zeros((1, 3), dtype=torch.int16)
    occ, state = bf_torch.ops.oracleB(root, 0, SIGMA, s['cam'], t(s['depth'], 'cpu'), t(s['mips'], 'cpu'), 3)
    assert occ.tolist() == [1] and state.tolist() == [2]
    occ, state, probs = bf_torch.ops.oracleB_final(root, 0, SIGMA, s['cam'], t(s['depth'], 'cpu'))
    assert occ.tolist() == [1] and state.tolist() == [2] and probs.shape == (1,)


def test_float32_decisions_are_pinned_by_float64():
    """The float32 oracle's occupancy and state equal the float64 evaluation's wherever the float64 margin -- the relative
    distance from equality of the closest comparison on the point's path, see spc_bf_bruteforce -- exceeds the rounding bound of
    the deciding expression: ``roundings * scale * 2^-24``, with ``roundings`` the count of float32 roundings on the longest path to
    a compared value (12 for a projected coordinate or extent, 16 for the argument of the profile curve, 30 for its value; derived
    beside the constants of spc_bf_bruteforce) and ``scale`` the magnitude of the summed terms.  The oracle reports the margin in
    units of ``roundings * scale``, so the condition is ``margin > 2^-24``.  Cases below the bound are left out; at most 1 % may
    be."""
    total = left_out = 0
    for name, level, points in oracleB_cases():
        s = scene(name)
        args = (points, level, SIGMA, s['cam'].numpy(), s['depth'], s['mips'], s['L'])
        o32, s32, _, _ = bf.oracleB(*args)
        o64, s64, _, margin = bf.oracleB(*args, dtype=np.float64)
        safe = margin > bf.U
        assert (o32[safe] == o64[safe]).all() and (s32[safe] == s64[safe]).all(), (name, level)
        total, left_out = total + len(points), left_out + int((~safe).sum())
        args = (points, level, SIGMA, s['cam'].numpy(), s['depth'])
        o32, s32, p32, _ = bf.oracleB_final(*args)
        o64, s64, p64, margin = bf.oracleB_final(*args, dtype=np.float64)
        safe = margin > bf.U
        assert (o32[safe] == o64[safe]).all() and (s32[safe] == s64[safe]).all(), (name, level)
        total, left_out = total + len(points), left_out + int((~safe).sum())
    print(f'{left_out} of {total} decisions below the bound ({left_out / total:.4%})')
    assert left_out <= 0.01 * total


@pytest.mark.parametrize('level', [1, 2, 3, 4])
def test_query_agrees_with_the_dense_expansion(level):
    check_query('cpu', level, 10 + level)


@pytest.mark.parametrize('level', [1, 2, 3, 4, 5, 6])
def test_bf_cells_equals_the_dense_query(level):
    sparse = dict(p_occ=0.45, p_unseen=0.25) if level < 5 else dict(p_occ=0.3, p_unseen=0.1)
    octree, empty = build_tree(level, 20 + level, **sparse)
    cells = check_cells('cpu', octree, empty, level)
    assert 0 < len(cells) < 8 ** level
    octree, empty = build_tree(level, 30 + level, unseen=False, p_occ=sparse['p_occ'])          # no unseen bit at all
    assert len(check_cells('cpu', octree, empty, level)) == sum(bin(int(b)).count('1') for b in octree[_level_start(octree, level - 1):])
    root_unseen = check_cells('cpu', np.array([0], np.uint8), np.array([255], np.uint8), level)   # the root byte all unseen
    assert len(root_unseen) == 8 ** level


@pytest.mark.parametrize('level', [1, 3, 4])
def test_merges_equal_the_oracle(level):
    want = check_merges('cpu', level)
    assert set(want[1].tolist()) == {0, 1, 2}


@pytest.mark.parametrize('n', COUNTS)
def test_merge_point_counts(n):
    check_merges('cpu', 3, n)


def test_octree_pin_and_fuse_laws():
    check_fuse_laws('cpu', check_octree_pin('cpu'))


def test_frame_geometry():
    check_frame_geometry('cpu', res=8)


def test_bad_arguments_raise_value_error():
    s = scene('front32')
    o = bf_torch.ops
    with pytest.raises(ValueError):
        o.build_mip2d(torch.zeros(30, 30), s['intrinsics'], 3, MAX_DEPTH, True)           # not whole 8 x 8 blocks
    with pytest.raises(ValueError):
        o.oracleB_final(torch.zeros((1, 3), dtype=torch.int16), 3, 0.0, s['cam'], t(s['depth'], 'cpu'))
    with pytest.raises(ValueError):
        o.subdivide(torch.zeros((2, 3), dtype=torch.int16), torch.tensor([1, 5], dtype=torch.int32))
    with pytest.raises(ValueError):
        o.process_final_voxels(4, 2, torch.zeros(32, dtype=torch.int32), torch.zeros(4, dtype=torch.int32),
                               torch.zeros(8, dtype=torch.int32), torch.zeros(4, dtype=torch.int32),
                               torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8))
    with pytest.raises(ValueError):
        o.bf_cells_cuda(torch.tensor([1, 1], dtype=torch.uint8), torch.tensor([1, 1], dtype=torch.uint8), 1)   # a byte too many
    with pytest.raises(ValueError):
        bfr.unbatched_query(torch.zeros(2, dtype=torch.uint8), torch.zeros(2, dtype=torch.uint8), torch.zeros(3, dtype=torch.int32),
                            torch.zeros((1, 3)), 1)                                                           # legacy exsum


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
def sphere_gaussians(device, n=20000, radius=0.5, scale=0.01, opacity=0.9):
    i = torch.arange(n, dtype=torch.float64) + 0.5
    phi, theta = torch.acos(1 - 2 * i / n), math.pi * (1 + 5 ** 0.5) * i
    xyz = radius * torch.stack([torch.cos(theta) * torch.sin(phi), torch.sin(theta) * torch.sin(phi), torch.cos(phi)], dim=1)
    return (xyz.float().to(device), torch.full((n, 3), scale, device=device),
            torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=device).repeat(n, 1), torch.full((n,), opacity, device=device))


def anchor_viewpoints():
    return densifier._generate_default_viewpoints()[:14]


def nearest_distances(p, among):
    """for the points p, the first rows of ``among``: the distance to the nearest other point of ``among``"""
    d = torch.cdist(p.double(), among.double())
    d[torch.arange(len(p)), torch.arange(len(p))] = float('inf')
    return d.min(dim=1).values


# the model per device: on the CPU, where the torch formulations of the voxeliser and the ray tracer take seconds, 10 000 Gaussians
# (still a watertight shell at level 6, checked), 64 x 64 depth maps and the 14 anchor viewpoints; on the GPU 20 000 and 256 x 256
E2E = {'cpu': dict(n=10000, res=6), 'cuda': dict(n=20000, res=8)}
E2E_LEVEL, E2E_RADIUS, E2E_SCALE = 6, 0.5, 0.01
E2E_CELL = 2 * (E2E_RADIUS + 0.05) / 2 ** E2E_LEVEL          # the densifier scales the normalised cube by dmax = radius + 0.05
# the shell's voxels reach the iso radius sqrt(11.345) * scale beyond the means, and a cell that a voxel test touches extends one
# cell diagonal further; in cells
E2E_K = math.sqrt(11.345) * E2E_SCALE / E2E_CELL + math.sqrt(3)


@functools.lru_cache(maxsize=None)
def e2e_model(device):
    return sphere_gaussians(device, n=E2E[device]['n'], radius=E2E_RADIUS, scale=E2E_SCALE), anchor_viewpoints()


def e2e_sample(device, gaussians=None, **kw):
    """sample_points_in_volume on the device's model (every call is a full run of the densifier)"""
    g, viewpoints = e2e_model(device)
    kw.setdefault('viewpoints', viewpoints)
    kw.setdefault('octree_level', E2E_LEVEL)
    real = densifier.RayTracedSPCDataset
    densifier.RayTracedSPCDataset = functools.partial(RayTracedSPCDataset, res=E2E[device]['res'])
    try:
        return kal.ops.gaussians.sample_points_in_volume(*(gaussians or g), **kw)
    finally:
        densifier.RayTracedSPCDataset = real


@functools.lru_cache(maxsize=None)
def e2e_free(device):
    return e2e_sample(device, jitter=False, clip_samples_to_input_bbox=False)


@functools.lru_cache(maxsize=None)
def e2e_clipped(device):
    return e2e_sample(device, jitter=False)


def e2e_geometry(device):
    """(centre, the cell centres that must be returned, key: a point's cell as one integer, bbox of the means)"""
    xyz = e2e_model(device)[0][0]
    lo, hi = xyz.min(0).values, xyz.max(0).values
    centre = 0.5 * (lo + hi)
    grid = torch.arange(2 ** E2E_LEVEL, device=device, dtype=torch.float32) * E2E_CELL - (E2E_RADIUS + 0.05)
    gx, gy, gz = torch.meshgrid(grid, grid, grid, indexing='ij')
    cells = torch.stack([gx, gy, gz], dim=-1).reshape(-1, 3) + centre
    must = cells[(cells - centre).norm(dim=1) / E2E_CELL <= E2E_RADIUS / E2E_CELL - E2E_K]

    def key(p):
        return (torch.round((p - centre + E2E_RADIUS + 0.05) / E2E_CELL).long() * torch.tensor([4096, 64, 1], device=device)).sum(dim=1)
    return centre, must, key, lo, hi


def check_fill_is_solid(device):
    """every returned point lies within r + k cells of the centre, and every cell centre within r - k cells is returned: the fill
    is solid, where gs_to_voxelgrid alone leaves the interior empty"""
    centre, must, key, lo, hi = e2e_geometry(device)
    free = e2e_free(device)
    assert ((free - centre).norm(dim=1) / E2E_CELL).max() <= E2E_RADIUS / E2E_CELL + E2E_K
    assert len(must) > 30000 and torch.isin(key(must), key(free)).all()


def check_clipped(device):
    centre, must, key, lo, hi = e2e_geometry(device)
    free, clipped = e2e_free(device), e2e_clipped(device)
    assert 0 < len(clipped) <= len(free) and ((clipped > lo) & (clipped < hi)).all()              # inside the bbox of the means
    assert torch.isin(key(must), key(clipped)).all()
    nn = nearest_distances(clipped[:4096], clipped)
    assert ((nn - nn.min()).abs() < 1e-5).float().mean() > 0.95                                 # a regular grid without jitter


def check_jitter(device):
    free = e2e_free(device)
    jittered = e2e_sample(device, jitter=True, clip_samples_to_input_bbox=False)
    assert len(jittered) == len(free)                       # the cells come in Morton order on every run
    moved = (jittered - free).norm(dim=1)
    assert moved.max() <= 2 * E2E_CELL * math.sqrt(3) and moved.std() > 0
    assert nearest_distances(jittered[:4096], jittered).std() > 1e-4                            # not all equal


def check_num_samples(device):
    assert len(e2e_sample(device, num_samples=500)) == 500
    with pytest.raises(AssertionError):
        e2e_sample(device, octree_level=5)


def check_mask(device):
    """the reference's mask test: the Gaussians above the threshold, unthresholded, give at least as many points"""
    opacity = e2e_model(device)[0][3]
    masked = e2e_sample(device, mask=opacity >= 0.35, opacity_threshold=0.0, jitter=False)
    assert masked.dim() == 2 and masked.shape[1] == 3 and masked.shape[0] >= e2e_clipped(device).shape[0]


def check_custom_viewpoints(device):
    centre, must, key, lo, hi = e2e_geometry(device)
    anchors = torch.tensor([[2.3, -2.3, 2.3], [0.0, 4.2, 0.0], [4.0, 0.0, 0.0], [-2.3, 2.3, 2.3], [0.0, -4.1, 0.0],
                            [2.3, 2.3, 2.3], [0.0, 0.0, 4.3]])
    custom = e2e_sample(device, viewpoints=torch.cat([anchors, -anchors]), jitter=False)
    assert len(custom) > 30000 and ((custom > lo) & (custom < hi)).all()


def check_failure_paths(device, caplog):
    g = sphere_gaussians(device, n=2000)
    with caplog.at_level(logging.WARNING):
        caplog.clear()
        out = e2e_sample(device, g, opacity_threshold=1.1)
        assert out.shape == (0, 3) and 'failed to produce a voxelized volume' in caplog.text
        caplog.clear()
        # viewpoints that look away from the shape: a shell far off-centre is behind every camera that looks at the origin
        away = torch.tensor([[0.0, 0.0, 0.5], [0.0, 0.5, 0.0]])
        small = (g[0] * 0.02 + torch.tensor([0.9, 0.9, 0.9], device=device), g[1] * 0.02, g[2], g[3])
        big = torch.cat([small[0], -small[0][:1]]), torch.cat([small[1], small[1][:1]]), torch.cat([small[2], small[2][:1]]), \
            torch.cat([small[3], small[3][:1]])
        out = e2e_sample(device, big, viewpoints=away, opacity_threshold=0.0)
        assert out.shape == (0, 3) and 'failed to produce a voxelized volume' in caplog.text


def test_fill_is_solid():
    check_fill_is_solid('cpu')


def test_clipped_samples_lie_on_a_grid_inside_the_bbox():
    check_clipped('cpu')


def test_jitter_moves_every_point_by_at_most_two_diagonals():
    check_jitter('cpu')


def test_num_samples_and_the_level_assertion():
    check_num_samples('cpu')


def test_masked_call_returns_at_least_the_thresholded_points():
    check_mask('cpu')


def test_custom_viewpoints():
    check_custom_viewpoints('cpu')


def test_sample_points_in_volume_failure_paths(caplog):
    check_failure_paths('cpu', caplog)


def test_both_spellings_are_registered():
    kaolin = kal.install_as_kaolin()
    import kaolin.ops.gaussian
    import kaolin.ops.gaussians
    from kaolin.ops.spc.bf_recon import bf_recon, unbatched_query                             # noqa: F401
    from kaolin.ops.spc.raytraced_spc_dataset import RayTracedSPCDataset as R                   # noqa: F401
    assert kaolin.ops.gaussian.sample_points_in_volume is kaolin.ops.gaussians.sample_points_in_volume
    assert kal.ops.random.sample_spherical_coords((5,))[0].shape == (5,)
