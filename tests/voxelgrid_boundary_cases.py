"""Meshes on the boundaries of the voxelizer's HIP pass (csrc/voxelgrid.hip) and a restatement of its thread split (helper, not
collected).  test_voxelgrid_boundary_cases_cpu.py proves from the oracle (oracle/voxelgrid.py) that every case has the property it
is named for and runs the package's torch path over the small ones; test_voxelgrid_boundaries_gpu.py runs the HIP pass.

  A  every L0 of the thread split (0 .. 9) against faces whose subdivision tree is empty, shallower than, exactly as deep as and
     deeper than L0.  Marking is idempotent, so a face list cycled to any length F gives the grid of its unique faces; F moves L0
  B  L0 = 0 the ordinary way: 8 spheres of 20 480 faces, and 2 000 spheres of 80 faces (more than two meshes per workgroup)
  C  tiny meshes in a batch, an empty face list, strided inputs
  D  the extent reduction: the vertex that alone holds a mesh's minimum / maximum at chosen indices
  E  NaN vertices (tests/golden/voxelgrid_edges.npz, made by the reference itself)
  F  shapes of the grid-tail cases
"""
import functools
import os

import numpy as np
import torch

from oracle import voxelgrid as vox_oracle
from kaolin_amd.utils.testing import geodesic_sphere

DTYPES = (torch.float32, torch.float64)
NP = {torch.float32: np.float32, torch.float64: np.float64}

# ---------------------------------------------------------------------------------------------------- the thread split
VOX_THREADS, VOX_MAXL0 = 160000, 10        # csrc/voxelgrid.hip: vox_launch's target (the compiled-in default) and VOX_MAXL0
VOX_NP, VOX_SLICE = 32, 256                # partial extents per mesh, vertices per slice and step
BF_THRESHOLDS = ((2, 3), (9, 10), (39, 40), (156, 157), (624, 625), (2499, 2500), (9999, 10000), (39999, 40000),
                 (159999, 160000))


def l0_of(batch, faces):
    """Levels of a face's tree that vox_launch spreads over threads: the smallest L0 with B F 4^L0 >= 160 000 (0 without faces)"""
    l0 = 0
    while faces > 0 and l0 < VOX_MAXL0 and batch * faces * 4 ** l0 < VOX_THREADS:
        l0 += 1
    return l0


def kept_per_round(normed, faces, resolution):
    """Triangles the oracle keeps (subdivides) round by round, for normalised vertices (V, 3) as a numpy array"""
    return [m[0].shape[0] for m in vox_oracle.subdivision_rounds(normed, faces, resolution)]


def normalised(vertices, origin, scale):
    """(B, V, 3) numpy array in the vertices' dtype: the reference's (v - origin) / scale, defaults included"""
    if origin is None:
        origin = torch.min(vertices, dim=1)[0]
    if scale is None:
        scale = torch.max(torch.max(vertices, dim=1)[0] - origin, dim=1)[0]
    return ((vertices - origin.unsqueeze(1)) / scale.view(-1, 1, 1)).numpy()


# ---------------------------------------------------------------------------------------------------- A
def face_of_depth(depth, resolution, rng):
    """Three normalised vertices of a triangle whose tree has `depth` full levels: its longest edge is 2^(depth - 1/2) times the
    edge length at which subdivision stops, (R - 1) / R^2 (half of that for depth 0), a factor sqrt(2) away from either
    neighbouring depth; the other edges are 0.6 and about 0.87 of it.  The first corner lies in the grid."""
    stop = (resolution - 1) / resolution ** 2
    longest = stop * 2.0 ** (depth - 0.5)
    anchor = rng.uniform(0.05, 0.45, 3)
    u = rng.uniform(0.3, 1.0, 3)
    u /= np.linalg.norm(u)
    p = np.cross(u, rng.uniform(-1.0, 1.0, 3))
    w = 0.5 * u + np.sqrt(0.75) * p / np.linalg.norm(p)            # a unit vector 60 degrees from u
    return np.stack((anchor, anchor + longest * u, anchor + 0.6 * longest * w))


# base meshes: every face on three vertices of its own.  Normalisation is given by the caller so that the depths are the
# builder's: the deep bases sit at R = 256 under a scale of 1/4 (trees of up to 11 levels, deeper than L0 = 9, in a dense grid
# of 256^3), the shallow one at R = 32 serves the long face lists (F 4^depth stays near 10^8 nodes)
A_BASES = {
    'deep_single': dict(resolution=256, depths=(11,), seed=11),
    'deep_pair': dict(resolution=256, depths=(9, 0), seed=12),
    'deep_pair_short': dict(resolution=256, depths=(7, 9), seed=13),
    'deep_trio': dict(resolution=256, depths=(0, 8, 10), seed=14),
    'deep': dict(resolution=256, depths=(0, 3, 5, 6, 7, 8, 10), seed=15),
    'shallow': dict(resolution=32, depths=(0, 1, 2, 3, 4, 5, 6), seed=16),
}
A_ORIGIN, A_SCALE = (0.125, -0.25, 0.5), 0.25
# (base, F): both sides of every threshold of B F, and every L0 from 9 down to 0
A_CASES = (('deep_single', 1), ('deep_single', 2), ('deep_pair', 2), ('deep_pair_short', 2), ('deep_trio', 3),
           ('deep', 9), ('deep', 10), ('deep', 39), ('deep', 40), ('deep', 156), ('deep', 157), ('deep', 624),
           ('shallow', 625), ('shallow', 2499), ('shallow', 2500), ('shallow', 9999), ('shallow', 10000), ('shallow', 39999),
           ('shallow', 40000), ('shallow', 159999), ('shallow', 160000), ('shallow', 200003))
A_BOTH_DTYPES_L0 = (0, 8, 9)


@functools.lru_cache(maxsize=None)
def a_base(name, dtype):
    """-> vertices (1, V, 3) raw, unique faces (U, 3), resolution, origin (1, 3), scale (1)"""
    spec = A_BASES[name]
    rng = np.random.default_rng(spec['seed'])
    normed = np.concatenate([face_of_depth(d, spec['resolution'], rng) for d in spec['depths']])
    origin, scale = torch.tensor([A_ORIGIN], dtype=dtype), torch.tensor([A_SCALE], dtype=dtype)
    vertices = (torch.from_numpy(normed).to(dtype) * scale + origin)[None]
    faces = torch.arange(3 * len(spec['depths'])).reshape(-1, 3)
    return vertices, faces, spec['resolution'], origin, scale


@functools.lru_cache(maxsize=None)
def a_expected(name, dtype):
    """The oracle's grid of the base's UNIQUE faces, computed once"""
    vertices, faces, resolution, origin, scale = a_base(name, dtype)
    return vox_oracle.trianglemeshes_to_voxelgrids(vertices, faces, resolution, origin, scale)


@functools.lru_cache(maxsize=None)
def a_depths(name, dtype):
    """Per unique face of the base: the triangles kept round by round, counted in the oracle"""
    vertices, faces, resolution, origin, scale = a_base(name, dtype)
    normed = normalised(vertices, origin, scale)[0]
    return tuple(tuple(kept_per_round(normed, faces[i:i + 1].numpy(), resolution)) for i in range(faces.shape[0]))


def cycled(faces, count):
    """The face list repeated up to `count` rows (count >= its length: every unique face is there)"""
    assert count >= faces.shape[0]
    return faces.repeat(-(-count // faces.shape[0]), 1)[:count].contiguous()


def a_cases(dtype):
    return [(name, count) for name, count in A_CASES if dtype == torch.float32 or l0_of(1, count) in A_BOTH_DTYPES_L0]


# ---------------------------------------------------------------------------------------------------- B
@functools.lru_cache(maxsize=None)
def sphere_batch(level, batch, dtype, seed):
    """`batch` copies of geodesic_sphere(level), each under an anisotropic scale and a translation of its own"""
    v, f = geodesic_sphere(level)
    g = torch.Generator().manual_seed(seed)
    stretch = 0.4 + 1.2 * torch.rand(batch, 1, 3, generator=g, dtype=torch.float64)
    shift = 4 * torch.rand(batch, 1, 3, generator=g, dtype=torch.float64) - 2
    return (v[None] * stretch + shift).to(dtype), f


def given_norm(vertices, seed):
    """A caller's origin (B, 3) a little below the minimum and scale (B) a little above the extent, per mesh"""
    g = torch.Generator().manual_seed(seed)
    lo, hi = vertices.min(dim=1)[0], vertices.max(dim=1)[0]
    extent = (hi - lo).max(dim=1)[0]
    origin = lo - 0.1 * extent[:, None] * torch.rand(lo.shape, generator=g, dtype=torch.float64).to(vertices.dtype)
    scale = extent * (1.05 + 0.3 * torch.rand(extent.shape, generator=g, dtype=torch.float64).to(vertices.dtype))
    return origin, scale


B8_LEVEL, B8_BATCH, B8_RES, B8_RES_FLAT = 32, 8, 96, 32          # 8 x 20 480 faces = 163 840: L0 = 0
MANY_LEVEL, MANY_BATCH, MANY_RES = 2, 2000, 8                    # 2 000 x 80 faces = 160 000: L0 = 0; V = 42


@functools.lru_cache(maxsize=None)
def b_expected(level, batch, dtype, seed, resolution, given):
    vertices, faces = sphere_batch(level, batch, dtype, seed)
    origin, scale = given_norm(vertices, seed + 1) if given else (None, None)
    return vox_oracle.trianglemeshes_to_voxelgrids(vertices, faces, resolution, origin, scale)


# ---------------------------------------------------------------------------------------------------- C
TET_FACES = torch.tensor([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]])
TET_BATCH, TET_RES = 7, 16


def tet_batch(dtype, seed=70):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(TET_BATCH, 4, 3, generator=g, dtype=torch.float64) * 3 - 1).to(dtype), TET_FACES


def points_only(dtype, seed=71):
    """V = 5 and a face list of shape (0, 3): the reference marks the vertices alone"""
    g = torch.Generator().manual_seed(seed)
    return torch.rand(2, 5, 3, generator=g, dtype=torch.float64).to(dtype), torch.zeros((0, 3), dtype=torch.long)


def strided_inputs(dtype, seed=72):
    """-> a (3, 18, 3) tensor whose every other row is a vertex (``[:, ::2]``: vertices (3, 9, 3)) and a (12, 6) tensor whose every
    other column is a corner (``[:, ::2]``: faces (12, 3)); the rows and columns in between hold values that must not be read"""
    g = torch.Generator().manual_seed(seed)
    wide = torch.rand(3, 18, 3, generator=g, dtype=torch.float64).to(dtype)
    wide[:, 1::2] += 5
    cols = torch.randint(0, 9, (12, 6), generator=g)
    return wide, cols


# ---------------------------------------------------------------------------------------------------- D
EXTENT_V = (255, 256, 257, 8191, 8192, 8193, 16385)
EXTENT_AT = (0, 255, 256, 8191, 8192)            # and V - 1
EXTENT_RES = 16
_TET_LO, _TET_HI = (-1.0, 2.0, 0.5), (3.0, 5.0, 3.5)             # the corner that alone holds every minimum / every maximum
_TET_MID = ((0.5, 4.0, 1.5), (2.0, 3.0, 2.5))


def extent_places(V):
    """(index of the minimum-holding vertex, index of the maximum-holding one): every index of EXTENT_AT below V, and V - 1,
    holds the minimum once and the maximum once"""
    at = sorted({i for i in EXTENT_AT if i < V} | {V - 1})
    return [(at[i], at[(i + 1) % len(at)]) for i in range(len(at))]


def extent_mesh(V, lo_at, hi_at, dtype, seed=0):
    """One tetrahedron among V vertices: corner `lo_at` alone holds the minimum of every axis, corner `hi_at` alone the maximum;
    the other two corners and the V - 4 vertices no face uses lie strictly inside their box -> vertices (V, 3), faces (4, 3)"""
    assert lo_at != hi_at and V >= 4
    g = torch.Generator().manual_seed(1000 * V + seed)
    lo, hi = torch.tensor(_TET_LO, dtype=torch.float64), torch.tensor(_TET_HI, dtype=torch.float64)
    vertices = lo + (hi - lo) * (0.2 + 0.6 * torch.rand(V, 3, generator=g, dtype=torch.float64))
    rest = [i for i in (1, 2, V - 2, V - 3) if i not in (lo_at, hi_at)][:2]
    vertices[lo_at], vertices[hi_at] = lo, hi
    vertices[rest[0]], vertices[rest[1]] = (torch.tensor(m, dtype=torch.float64) for m in _TET_MID)
    corners = torch.tensor([lo_at, rest[0], rest[1], hi_at])
    return vertices.to(dtype), corners[TET_FACES]


def without_vertex(vertices, index):
    """The same vertices with vertex `index` moved to the middle of the box: what a reduction that drops it would see"""
    out = vertices.clone()
    out[index] = (torch.tensor(_TET_LO, dtype=torch.float64) + torch.tensor(_TET_HI, dtype=torch.float64)).to(vertices.dtype) / 2
    return out


# ---------------------------------------------------------------------------------------------------- E
EDGES_NPZ = 'voxelgrid_edges.npz'
NAN_LONE = ('nan_first', 'nan_second', 'nan_third')
EDGE_CASES = NAN_LONE + ('nan_closed', 'nan_batch3', 'coincide')


def edge_case_inputs():
    """name -> (vertices (B, V, 3) float32, faces, resolution, origin or None, scale or None): the inputs of
    tests/golden/voxelgrid_edges.npz (make_golden_voxelgrid_edges.py stores them with the reference's outputs)"""
    nan = float('nan')
    quad = torch.tensor([[[0.1, 0.1, 0.1], [0.9, 0.2, 0.3], [0.2, 0.8, 0.5], [nan, 0.5, 0.5]]])
    zero, one = torch.zeros(1, 3), torch.ones(1)
    cases = {}
    # a lone face with the NaN vertex as its first, second and third corner: its finite edge belongs to no other face
    for name, face in zip(NAN_LONE, ([3, 0, 1], [0, 3, 1], [0, 1, 3])):
        cases[name] = (quad, torch.tensor([face]), 16, zero, one)
    # an octahedron whose apex (id 5) is NaN: every finite edge of a face at the apex is also an edge of a finite face
    octa = torch.tensor([[[0.5, 0.1, 0.5], [0.9, 0.5, 0.45], [0.5, 0.9, 0.55], [0.1, 0.5, 0.5], [0.45, 0.5, 0.1], [0.5, nan, 0.9]]])
    octa_faces = torch.tensor([[0, 1, 4], [1, 2, 4], [2, 3, 4], [3, 0, 4], [1, 0, 5], [2, 1, 5], [3, 2, 5], [0, 3, 5]])
    cases['nan_closed'] = (octa, octa_faces, 24, zero, one)
    # default origin and scale: the NaN of mesh 1 reaches its origin, the meshes on either side are untouched
    tets = tet_batch(torch.float32, seed=73)[0][:3].clone()
    tets[1, 2, 1] = nan
    cases['nan_batch3'] = (tets, TET_FACES, 16, None, None)
    # every vertex the same point: the default scale is 0 and every normalised coordinate 0 / 0
    cases['coincide'] = (torch.tensor([[[0.25, -1.5, 3.0]] * 4]), TET_FACES, 8, None, None)
    return cases


def load_edge_case(gold, name, dtype):
    """-> vertices, faces, resolution, origin, scale, the reference's dense grid, all in `dtype`"""
    v = torch.from_numpy(gold[name + '_vertices']).to(dtype)
    f, res = torch.from_numpy(gold[name + '_faces']).long(), int(gold[name + '_res'])
    org = torch.from_numpy(gold[name + '_origin']).to(dtype) if name + '_origin' in gold else None
    sc = torch.from_numpy(gold[name + '_scale']).to(dtype) if name + '_scale' in gold else None
    tag = 'f32' if dtype == torch.float32 else 'f64'
    dense = np.unpackbits(gold[f'{name}_packed_{tag}'])[:v.shape[0] * res ** 3].reshape(v.shape[0], res, res, res)
    return v, f, res, org, sc, torch.from_numpy(dense).to(dtype)


def edges_path(golden_dir):
    return os.path.join(golden_dir, EDGES_NPZ)


# ---------------------------------------------------------------------------------------------------- F
DENSE_TAILS = tuple((res, batch) for res in (65, 127) for batch in (1, 3))      # B R^3 4 bytes is no multiple of 16
SPARSE_TAILS = ((5, 2), (33, 3), (65, 2))                                       # R^3 is no multiple of 32


def tail_mesh(batch, dtype=torch.float32, seed=90):
    """A small sphere per mesh, stretched its own way, reaching the last voxels of the grid along every axis"""
    return sphere_batch(3, batch, dtype, seed)
