"""Meshes on the stage boundaries of the Loop subdivision pipeline (csrc/subdivide_trianglemesh.hip) and the comparison of a
forward / backward with the brute force (helper, not collected).  test_subdivide_trianglemesh_bruteforce_cpu.py runs the package's
CPU path over them, test_subdivide_trianglemesh_boundaries_gpu.py the HIP pipeline; both assert from the brute force's own counts
that a mesh sits where its parameter says.

Every generator takes a seed for the order of the faces and the rotation of their corners, so the keys arrive unsorted."""
import functools

import numpy as np
import torch

import subdivide_trianglemesh_bruteforce as bf

SORT_BLOCK, SCAN_BLOCK = 2048, 1024                       # csrc/sort_scan_host.h: SS_SORT_BLOCK, SS_SCAN_BLOCK
KEY_FACES = (1, 341, 342, 682, 683, 1365, 1366, 2730, 2731)                   # 3 F next to 1024, 2048, 4096 and 8192
KEY_COUNTS = (3, 1023, 1026, 2046, 2049, 4095, 4098, 8190, 8193)
EDGE_COUNTS = (1, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
ID_WIDTH_FULL = (256, 257, 65536, 65537)                                      # 1 | 2 | 2 | 3 radix passes per key half
ID_WIDTH_TOPOLOGY = (1 << 24, (1 << 24) + 1)                                  # 3 | 4
ID_WIDTH_SPECIAL = (255, 256, 65535, 65536, (1 << 24) - 1, 1 << 24)
BATCHES = (1023, 1024, 1025, 2049)
# faces of the two large cases.  349 526: 1 048 578 keys, 1 025 blocks of the head scan, whose last block adds up 1 024 block sums,
# one per thread.  349 868: 1 049 604 keys, 1 026 blocks, whose last adds up 1 025: the first to take the loop's second round.
BIG_FACES = (349526, 349868)
SETTINGS = ('default', 'alpha')
DTYPES = (torch.float32, torch.float64)


def cdiv(a, b):
    return -(-a // b)


def passes_per_half(V):
    """The 8-bit radix passes that sort ids below V: the digits that hold a bit of V - 1"""
    return max(1, cdiv((V - 1).bit_length(), 8))


def shuffled(faces, seed):
    """Seeded face order and, per face, seeded rotation of its corners (the orientation is kept)"""
    g = torch.Generator().manual_seed(seed)
    faces = faces[torch.randperm(faces.shape[0], generator=g)]
    turn = torch.randint(0, 3, (faces.shape[0],), generator=g)
    rows = torch.arange(faces.shape[0])
    return torch.stack([faces[rows, (turn + k) % 3] for k in range(3)], dim=1)


def strip_faces(F, first=0):
    """F faces (i, i + 1, i + 2), every other one turned round: F + 2 vertices, 2 F + 1 edges"""
    i = torch.arange(F) + first
    odd = (torch.arange(F) % 2 == 1)
    return torch.stack((i, torch.where(odd, i + 2, i + 1), torch.where(odd, i + 1, i + 2)), dim=1)


def strip(F, free=0, seed=0):
    """A strip of F faces and `free` triangles on three fresh vertices each -> faces, V.  E = 2 F + 1 + 3 free."""
    parts = [strip_faces(F)] + [torch.arange(3)[None] + (F + 2 + 3 * k) for k in range(free)]
    return shuffled(torch.cat(parts), seed), F + 2 + 3 * free


def wheel(n, hub_last=False, seed=0):
    """n rim vertices around a hub of valence n -> faces, V = n + 1"""
    rim = torch.arange(n) + (0 if hub_last else 1)
    hub = torch.full((n,), n if hub_last else 0)
    return shuffled(torch.stack((hub, rim, rim.roll(-1)), dim=1), seed), n + 1


def grid(m, k, seed=0, faces=None):
    """m x k squares cut in two, row by row; the first `faces` triangles of them -> faces, V = (m + 1) (k + 1)"""
    r, c = torch.meshgrid(torch.arange(m), torch.arange(k), indexing='ij')
    p = (r * (k + 1) + c).reshape(-1)
    both = torch.stack((p, p + 1, p + k + 2, p, p + k + 2, p + k + 1), dim=1).reshape(-1, 3)
    return shuffled(both if faces is None else both[:faces], seed), (m + 1) * (k + 1)


@functools.lru_cache(maxsize=None)
def mesh_for_keys(F):
    """F faces: a strip and, where F allows it, two free triangles"""
    return strip(F, 0, seed=F) if F <= 2 else strip(F - 2, 2, seed=F)


@functools.lru_cache(maxsize=None)
def mesh_for_edges(E):
    """E unique edges: (a, a, a) for 1, one triangle for 3, else a strip and two or three free triangles"""
    if E == 1:
        return torch.zeros(1, 3, dtype=torch.long), 1
    if E == 3:
        return strip(1, 0, seed=E)
    free = 2 + (E % 2 == 0)
    return strip((E - 1 - 3 * free) // 2, free, seed=E)


@functools.lru_cache(maxsize=None)
def mesh_for_id_width(V):
    """A 40-face strip whose 42 ids go through an increasing injection into [0, V) that uses 0, V - 1 and every id of
    ID_WIDTH_SPECIAL below V -> faces, V, the sorted ids"""
    must = sorted({0, V - 1} | {s for s in ID_WIDTH_SPECIAL if s < V})
    drawn = [int(i) for i in np.random.RandomState(V % (1 << 31)).randint(0, V, size=400)]
    ids = list(must)
    for i in drawn:
        if len(ids) == 42:
            break
        if i not in ids:
            ids.append(i)
    ids = torch.tensor(sorted(ids))
    assert ids.numel() == 42 and int(ids[0]) == 0 and int(ids[-1]) == V - 1
    faces, _ = strip(40, 0, seed=V % 1000)
    return ids[faces], V, ids


@functools.lru_cache(maxsize=None)
def big_grid(F):
    """The first F triangles of a 400 x 437 (F = BIG_FACES[0]) or 400 x 438 grid, the last row cut short"""
    return grid(400, 437 if F == BIG_FACES[0] else 438, seed=7, faces=F)


def inputs(B, V, E, dtype, seed):
    """-> x (B, V, 3) in [-1/2, 1/2), alpha (B, V) in [0, 1), and the cotangents gx (B, V + E, 3), ga (B, V + E), drawn in `dtype`"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, V, 3, generator=g, dtype=dtype) - 0.5, torch.rand(B, V, generator=g, dtype=dtype),
            torch.rand(B, V + E, 3, generator=g, dtype=dtype) - 0.5, torch.rand(B, V + E, generator=g, dtype=dtype) - 0.5)


# ---- comparisons --------------------------------------------------------------------------------------------------------------
WORST = {}                                    # (what, dtype) -> the largest share of its bound any check of this process used


def _note(what, dtype, value):
    key = (what, str(dtype))
    WORST[key] = max(WORST.get(key, 0.0), value)


def check_forward(tp, new_x, new_alpha, x, alpha, label):
    """new_x (B, V + E, 3) and new_alpha (or None) of a forward in their own dtype against the brute force, within the derived
    bound -> the brute force's result"""
    dtype = new_x.dtype
    fw = bf.forward(tp, x.cpu().numpy(), None if alpha is None else alpha.cpu().numpy())
    bound_x, bound_a = bf.forward_bound(fw, dtype, default=alpha is None)
    used = bf.share(new_x.cpu().numpy(), fw.new_x, bound_x)
    if alpha is None:
        assert new_alpha is None
    else:
        assert new_alpha.dtype == dtype
        used = max(used, bf.share(new_alpha.cpu().numpy(), fw.new_alpha, bound_a))
    _note('forward', dtype, used)
    print(f'{label} {dtype} forward: {used:.3f} of the bound')
    assert used <= 1, (label, dtype, used)
    return fw


def check_backward(tp, dx, da, x, alpha, gx, ga, label):
    """dx (B, V, 3) and da (or None) of a backward under the cotangents gx, ga (or None) against the brute force"""
    dtype = dx.dtype
    bw = bf.backward(tp, x.cpu().numpy(), None if alpha is None else alpha.cpu().numpy(), gx.cpu().numpy(),
                     None if ga is None else ga.cpu().numpy())
    bound_x, bound_a = bf.gradient_bound(bw, dtype)
    used = bf.share(dx.cpu().numpy(), bw.dx, bound_x)
    if da is not None:
        assert da.dtype == dtype and alpha is not None
        used = max(used, bf.share(da.cpu().numpy(), bw.da, bound_a))
    _note('backward', dtype, used)
    print(f'{label} {dtype} backward: {used:.3f} of the bound')
    assert used <= 1, (label, dtype, used)
    return bw


def report():
    """Printed by a module-scoped fixture of either test file once its last test has run"""
    for (what, dtype), value in sorted(WORST.items()):
        print(f'worst share of the bound in this run, {what} {dtype}: {value:.3f}')
