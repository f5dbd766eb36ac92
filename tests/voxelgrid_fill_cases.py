"""The inputs and the oracle of the ops.voxelgrid.fill boundary suite (helper, not collected; shared by
tests/test_voxelgrid_fill_boundaries_cpu.py and tests/test_voxelgrid_fill_boundaries_gpu.py).  numpy and plain Python only: no
torch, no scipy, nothing of kaolin_amd.

``fill_oracle`` is the independent definition of the operation: per batch item an explicit queue starts from the empty voxels of
the six boundary faces, grows through the six face neighbours, and the answer is NOT reached.  ``case(name)`` builds a bool
(N, X, Y, Z) grid; a name is a shape or a construction, and what makes it a boundary of csrc/voxelgrid_fill.hip is said where the
GPU suite uses it.  A case and its oracle are computed once per process and handed out read-only."""
import collections
import functools

import numpy as np

DENSITY = 0.72          # a voxel of a random case is a wall with this probability
MIN_VOLUME = 1000       # random cases of at least this volume must hold MIN_COUNT cavity voxels and MIN_COUNT outside voxels that
MIN_COUNT = 50          # are on no boundary face (test_voxelgrid_fill_boundaries_cpu.py asserts it)

# the shapes of the random cases: Z around the words (32), the chunks (64), the pack rounds and the bricks along Z (256) at X = 5,
# Y = 6; X and Y around the brick (16) at Z = 33; a batch at brick scale
Z_SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 258, 260, 287, 288, 289, 511, 512, 513)
XY_SIZES = ((1, 1), (1, 40), (40, 1), (2, 2), (15, 17), (16, 16), (17, 15), (31, 33), (32, 32), (33, 31))
BATCH_SHAPE = (3, 17, 33, 65)
RANDOM_SHAPES = {f'z{z}': (1, 5, 6, z) for z in Z_SIZES}
RANDOM_SHAPES.update({f'xy{x}x{y}': (1, x, y, 33) for x, y in XY_SIZES})
RANDOM_SHAPES['batch'] = BATCH_SHAPE

CARRY_NAMES = tuple(f'carry_{c}' for c in 'abcdef')
CORRIDOR_NAMES = ('corridor_z', 'corridor_x', 'corridor_y')
MANY_SHAPE = (4101, 3, 3, 37)      # more bricks than the pass kernel has workgroups (4096)
MANY_TAIL = range(4096, 4101)      # the items that are a workgroup's second brick
NAMES = tuple(RANDOM_SHAPES) + CARRY_NAMES + CORRIDOR_NAMES + ('many_bricks',)


# ---- the oracle --------------------------------------------------------------------------------------------------------------------
def _flood_item(empty):
    """(X, Y, Z) bool, True = empty -> (X, Y, Z) bool, True = reached from an empty voxel of a boundary face.  The item gets a rim of
    walls, so that the six neighbours of a flat index are six offsets and none leaves the array."""
    X, Y, Z = empty.shape
    padded = np.zeros((X + 2, Y + 2, Z + 2), dtype=np.uint8)
    padded[1:-1, 1:-1, 1:-1] = empty
    face = np.zeros((X, Y, Z), dtype=bool)
    face[0], face[-1], face[:, 0], face[:, -1], face[:, :, 0], face[:, :, -1] = (True,) * 6
    seeds = np.zeros(padded.shape, dtype=bool)
    seeds[1:-1, 1:-1, 1:-1] = face & empty
    sy, sx = Z + 2, (Y + 2) * (Z + 2)
    steps = (1, -1, sy, -sy, sx, -sx)
    free = bytearray(padded.tobytes())          # 1 = empty and not reached yet
    reached = bytearray(len(free))
    queue = collections.deque(np.flatnonzero(seeds.ravel()).tolist())
    for i in queue:
        free[i] = 0
        reached[i] = 1
    while queue:
        i = queue.popleft()
        for d in steps:
            j = i + d
            if free[j]:
                free[j] = 0
                reached[j] = 1
                queue.append(j)
    return np.frombuffer(bytes(reached), dtype=np.uint8).reshape(padded.shape)[1:-1, 1:-1, 1:-1].astype(bool)


def fill_oracle(grid):
    """(N, X, Y, Z), any dtype, wall = value != 0 -> bool (N, X, Y, Z): the walls and every empty voxel that no path of face-adjacent
    empty voxels joins to an empty voxel of the item's six boundary faces"""
    grid = np.asarray(grid)
    assert grid.ndim == 4
    out = np.ones(grid.shape, dtype=bool)
    if grid.size:
        for n in range(grid.shape[0]):
            out[n] = ~_flood_item(grid[n] == 0)
    return out


def off_faces(a):
    """the voxels of (N, X, Y, Z) that lie on no boundary face"""
    return a[:, 1:-1, 1:-1, 1:-1]


def counts(grid, filled):
    """(cavity voxels, outside voxels on no boundary face) per batch item, as two integer arrays of length N"""
    cavity = (filled & ~grid).reshape(len(grid), -1).sum(1)
    outside = off_faces(~filled).reshape(len(grid), -1).sum(1)
    return cavity, outside


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
def shape_seed(shape):
    n, x, y, z = shape
    return (((n * 1009 + x) * 1013 + y) * 1019 + z) % (2 ** 32)


def random_grid(shape, density=DENSITY):
    """every shape of RANDOM_SHAPES meets the condition on its first draw at DENSITY: none needed another seed or density"""
    rng = np.random.RandomState(shape_seed(shape))
    return rng.random_sample(shape) < density


def _row(z_empty, walls=()):
    """3 x 3 x 513, all wall except the row x = y = 1, which is empty on the inclusive range z_empty but for the voxels `walls`"""
    g = np.ones((1, 3, 3, 513), dtype=bool)
    g[0, 1, 1, z_empty[0]:z_empty[1] + 1] = False
    for z in walls:
        g[0, 1, 1, z] = True
    return g


CARRIES = {
    'carry_a': ((0, 512), ()),         # open at both ends
    'carry_b': ((0, 511), ()),         # open at z = 0 only: the flood climbs across both brick boundaries
    'carry_c': ((1, 512), ()),         # open at z = 512 only: the flood descends across both
    'carry_d': ((0, 511), (255,)),     # as b, stopped by a wall in the last bit of the first brick: above it a cavity
    'carry_e': ((0, 511), (256,)),     # as b, stopped by a wall in the first bit of the second brick
    'carry_f': ((250, 262), ()),       # a closed cavity that spans z = 256
}


def corridor_plane(rows, length, lo, hi):
    """(rows, length) bool, True = wall.  Row 1 is empty on [0, hi], the rows 3, 5, ..., rows - 2 on [lo, hi]; row r joins row r + 2
    through (r + 1, hi) and (r + 1, lo) in turn, starting at hi: one path, open only at (1, 0), that crosses every position between
    lo and hi once per odd row."""
    assert rows % 2 == 1 and 0 < lo < hi < length - 1
    p = np.ones((rows, length), dtype=bool)
    p[1, 0:hi + 1] = False
    for k, r in enumerate(range(3, rows - 1, 2)):
        p[r, lo:hi + 1] = False
        p[r - 1, lo if k % 2 else hi] = False
    return p


def corridor(name):
    """The plane above as the middle plane of a grid three voxels thick, all wall around it: along Z across z = 256 (3 x 67 x 260),
    along X across x = 16 (35 x 67 x 3) and along Y across y = 16 (67 x 35 x 3)"""
    if name == 'corridor_z':
        g = np.ones((1, 3, 67, 260), dtype=bool)
        g[0, 1] = corridor_plane(67, 260, 254, 258)
    elif name == 'corridor_x':
        g = np.ones((1, 35, 67, 3), dtype=bool)
        g[0, :, :, 1] = corridor_plane(67, 35, 14, 18).T
    else:
        g = np.ones((1, 67, 35, 3), dtype=bool)
        g[0, :, :, 1] = corridor_plane(67, 35, 14, 18)
    return g


def many_bricks():
    """4101 items of 3 x 3 x 37: random walls at 0.8, then the centre row x = y = 1 cleared for z in [1, 35].  The centre row is all
    that lies off the boundary faces, and cleared it is one run: outside as soon as one of its 142 neighbours is empty, so no seed
    makes a cavity of it (0.8^142).  Every odd item therefore gets a plugged stretch [a, b] of that row -- walls at a - 1 and b + 1
    in the row, and around it on [a, b] -- which is a cavity, while the rest of the row is left to the random walls."""
    rng = np.random.RandomState(shape_seed(MANY_SHAPE))
    g = rng.random_sample(MANY_SHAPE) < 0.8
    g[:, 1, 1, 1:36] = False
    for n in range(1, MANY_SHAPE[0], 2):
        a, b = rng.randint(3, 13), rng.randint(20, 33)
        g[n, :, :, a:b + 1] = True
        g[n, 1, 1, a:b + 1] = False
        g[n, 1, 1, a - 1] = g[n, 1, 1, b + 1] = True
    return g


@functools.lru_cache(maxsize=None)
def case(name):
    """bool (N, X, Y, Z), True = wall; read-only"""
    if name in RANDOM_SHAPES:
        g = random_grid(RANDOM_SHAPES[name])
    elif name in CARRIES:
        g = _row(*CARRIES[name])
    elif name in CORRIDOR_NAMES:
        g = corridor(name)
    elif name == 'many_bricks':
        g = many_bricks()
    else:
        raise KeyError(name)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def expected(name):
    """fill_oracle(case(name)); read-only"""
    out = fill_oracle(case(name))
    out.setflags(write=False)
    return out
