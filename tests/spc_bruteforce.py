"""Brute-force SPC decoder in numpy: the oracle of tests/test_spc_cpu.py and tests/test_spc_gpu.py.

From a boolean 2^L cube it derives, level by level and without any of the package's code: the occupied cells (OR-pooling), their
order (Morton code: bit 3i = z_i, 3i + 1 = y_i, 3i + 2 = x_i, so the child index of a cell in its parent is x << 2 | y << 1 | z,
and that is also its bit in the parent's byte), the octree bytes, the pyramid, the inclusive sum of the bit counts, the point
hierarchy, and a (level, x, y, z) -> index dictionary for queries.  tests/golden/spc_examples.json pins it to the reference's
recorded answers.  It must not import kaolin_amd.ops.spc."""
import numpy as np


def morton_code(x, y, z, bits=15):
    code = 0
    for i in range(bits):
        code |= ((int(z) >> i) & 1) << (3 * i)
        code |= ((int(y) >> i) & 1) << (3 * i + 1)
        code |= ((int(x) >> i) & 1) << (3 * i + 2)
    return code


class Decoded:
    """level, octree (uint8), pyramid (2, level + 2) int32, exsum int32, points (n, 3) int16, level_points (list), index (dict)"""


def decode(cube):
    cube = np.asarray(cube, dtype=bool)
    D = cube.shape[0]
    L = int(round(np.log2(D)))
    assert cube.shape == (D, D, D) and 2 ** L == D and cube.any()
    occ = [None] * (L + 1)
    occ[L] = cube
    for l in range(L - 1, -1, -1):
        n = 2 ** l
        occ[l] = occ[l + 1].reshape(n, 2, n, 2, n, 2).any(axis=(1, 3, 5))
    level_points = []
    for l in range(L + 1):
        cells = np.argwhere(occ[l])
        order = np.argsort([morton_code(*c) for c in cells], kind='stable')
        level_points.append(cells[order].astype(np.int16).reshape(-1, 3))
    octree = []
    for l in range(L):
        for x, y, z in level_points[l].astype(np.int64):
            byte = 0
            for child in range(8):
                if occ[l + 1][2 * x + (child >> 2), 2 * y + ((child >> 1) & 1), 2 * z + (child & 1)]:
                    byte |= 1 << child
            octree.append(byte)
    d = Decoded()
    d.level = L
    d.octree = np.array(octree, dtype=np.uint8)
    counts = [len(p) for p in level_points]
    d.pyramid = np.zeros((2, L + 2), dtype=np.int32)
    d.pyramid[0, :L + 1] = counts
    d.pyramid[1, 1:] = np.cumsum(counts)
    d.exsum = np.cumsum([bin(b).count('1') for b in octree]).astype(np.int32).reshape(-1)
    d.level_points = level_points
    d.points = np.concatenate(level_points)
    d.index = {}
    for l in range(L + 1):
        for i, (x, y, z) in enumerate(level_points[l]):
            d.index[(l, int(x), int(y), int(z))] = int(d.pyramid[1, l]) + i
    return d


def decode_batch(cubes):
    """-> (list of Decoded, octrees, lengths int32, pyramids (B, 2, L + 2), exsum, point hierarchies): the packed batch"""
    ds = [decode(c) for c in cubes]
    return (ds, np.concatenate([d.octree for d in ds]), np.array([len(d.octree) for d in ds], dtype=np.int32),
            np.stack([d.pyramid for d in ds]), np.concatenate([d.exsum for d in ds]), np.concatenate([d.points for d in ds]))


def cube_of_points(points, level):
    cube = np.zeros((2 ** level,) * 3, dtype=bool)
    p = np.asarray(points, dtype=np.int64).reshape(-1, 3)
    cube[p[:, 0], p[:, 1], p[:, 2]] = True
    return cube


def random_cube(level, seed, density=None):
    """A random non-empty cube; the default density keeps about 40 cells, whatever the level"""
    rng = np.random.RandomState(seed)
    D = 2 ** level
    if density is None:
        density = min(0.5, 40.0 / D ** 3)
    cube = rng.rand(D, D, D) < density
    cube[tuple(rng.randint(0, D, 3))] = True
    return cube


def query(d, level, cell):
    """index of the point of `level` at integer `cell`, -1 when absent or outside the grid"""
    return d.index.get((level, int(cell[0]), int(cell[1]), int(cell[2])), -1)


def ancestors(d, level, cell):
    """[index at level 0, ..., index at `level`] of the chain that holds integer `cell` of `level`; -1 from the first miss on; all -1
    outside the grid"""
    x, y, z = (int(v) for v in cell)
    if min(x, y, z) < 0 or max(x, y, z) >= 2 ** level:
        return [-1] * (level + 1)
    return [d.index.get((l, x >> (level - l), y >> (level - l), z >> (level - l)), -1) for l in range(level + 1)]
