"""Inputs that put the backward of ops.conversions.FlexiCubes (csrc/flexicubes.hip, fc_backward_kernel: one thread per surface
cube in workgroups of 256) on its boundaries: exact numbers S of surface cubes and Q of quads around 256 and 1024, no quads at
all, cubes of several dual vertices in different count classes, an inverted (ambiguous) cube.  Pure torch on the CPU, seeded by
torch.Generator; every seed is pinned here.  ``make_grid`` returns

    vertices (V, 3) float32, sdf (V,) float32, cube_idx (C, 8) int64, resolution (3 ints), beta (C, 12), alpha (C, 8), gamma_f (C,)

test_flexicubes_boundaries_cpu.py checks that every case is what it claims to be; test_flexicubes_boundaries_gpu.py runs them
through the kernels.  The grids keep A / h small (jitter of a tenth of a cell, |sdf| in [0.25, 1]): the gradient bound of
flexicubes_gradient_oracle.py keeps its teeth there."""
import torch

from kaolin_amd.ops.conversions import FlexiCubes
from kaolin_amd.ops.conversions.flexicubes import flexicubes as fcm
from kaolin_amd.ops.conversions.flexicubes._tables import CHECK_TABLE

BLOCK = 256                                                    # csrc: FC_THREADS


def make_grid(res, seed, kind='sphere', weights=True):
    """CPU inputs: a jittered grid and an sdf -- 'sphere' (plus noise: cubes of several dual vertices), 'signs' (random signs:
    every cube is a surface cube, all four count classes) or 'plane' (exactly the middle layer of cubes along z is crossed)."""
    g = torch.Generator().manual_seed(seed)
    v, c = FlexiCubes('cpu').construct_voxel_grid(res)
    res = fcm._resolution3(res)
    cell = 1.0 / torch.tensor(res, dtype=torch.float32)
    v = v + (torch.rand(v.shape, generator=g) - 0.5) * 0.2 * cell
    if kind == 'sphere':
        s = (v - torch.tensor([0.04, -0.03, 0.02])).norm(dim=-1) - 0.33 + 0.3 * float(cell.max()) * torch.randn(v.shape[0], generator=g)
    elif kind == 'signs':
        s = torch.where(torch.rand(v.shape[0], generator=g) < 0.5, -1.0, 1.0) * (0.25 + 0.75 * torch.rand(v.shape[0], generator=g))
    else:
        layer = torch.round((v[:, 2] + 0.5) * res[2])
        s = torch.where(layer <= res[2] // 2, -1.0, 1.0) * (0.25 + 0.75 * torch.rand(v.shape[0], generator=g))
    n = c.shape[0]
    if not weights:
        return v, s, c, res, None, None, None
    return v, s, c, res, 0.5 * torch.randn(n, 12, generator=g), 0.5 * torch.randn(n, 8, generator=g), 0.5 * torch.randn(n, generator=g)


# name -> (resolution, kind, seed, S, Q); None = whatever the seed gives (asserted by range in the CPU test).
# A 'plane' grid (rx, ry, 3) has S = rx ry surface cubes and Q = (rx - 1)(ry - 1) quads whatever the seed.
CASES = {
    'S255': ((17, 15, 3), 'plane', 335, 255, 224),
    'S256': ((16, 16, 3), 'plane', 335, 256, 225),
    'S257_Q0': ((257, 1, 3), 'plane', 561, 257, 0),            # no quads at all
    'S258': ((43, 6, 3), 'plane', 352, 258, 210),
    'Q255': ((16, 18, 3), 'plane', 337, 288, 255),
    'Q256': ((17, 17, 3), 'plane', 337, 289, 256),
    'S516_Q257': ((258, 2, 3), 'plane', 563, 516, 257),
    'S1023': ((33, 31, 3), 'plane', 367, 1023, 960),
    'S1024': ((32, 32, 3), 'plane', 367, 1024, 961),           # four full workgroups
    'signs_8x8x5': ((8, 8, 5), 'signs', 321, 317, 350),        # more than one workgroup, all four count classes
    'signs_10x10x8': ((10, 10, 8), 'signs', 328, 793, 944),
    'signs_1x1x1': ((1, 1, 1), 'signs', 308, 1, 0),            # one cube of three dual vertices
    'signs_1x1x4': ((1, 1, 4), 'signs', 324, 4, 0),            # cubes of 2, 1, 3 and 2 dual vertices
}
OPTION_CASES = ('Q256', 'signs_8x8x5')


def case_inputs(name):
    res, kind, seed = CASES[name][:3]
    return make_grid(res, seed, kind)


def case_codes(sdf, cube_idx):
    """The case byte of every cube, before the ambiguity rule: bit k set iff sdf(corner k) < 0."""
    return ((sdf[cube_idx] < 0).long() << torch.arange(8)).sum(-1)


def inverted_cubes(sdf, cube_idx, res):
    """The cubes the ambiguity rule inverts, from CHECK_TABLE alone: marked, and the cube across the ambiguous face exists and is
    marked too."""
    codes = case_codes(sdf, cube_idx).tolist()
    found = []
    for c, code in enumerate(codes):
        marked, dx, dy, dz, _ = CHECK_TABLE[code]
        if marked != 1:
            continue
        p = (c // (res[1] * res[2]) + dx, (c // res[2]) % res[1] + dy, c % res[2] + dz)
        if all(0 <= p[d] < res[d] for d in range(3)) and CHECK_TABLE[codes[(p[0] * res[1] + p[1]) * res[2] + p[2]]][0] == 1:
            found.append(c)
    return found


def relabel_for_id_width(inputs, V):
    """-> (dense inputs, sparse inputs, ids) for the pair sort's id width: the grid's vertices renumbered so that the ends 0 and
    n - 1 lie on crossed edges shared by four cubes, then mapped MONOTONELY into [0, V) with 0 -> 0 and n - 1 -> V - 1.  Edge
    pairs compare alike under a monotone map, so the sparse call has the dense call's orders."""
    v, s, c, res, beta, alpha, gamma = inputs
    n = v.shape[0]
    topo = fcm.topology_torch(s, c, res)
    key = (topo['a'] * n + topo['b'])[topo['mask']]
    uniq, counts = torch.unique(key, return_counts=True)
    shared = uniq[counts == 4]                                  # (masked incidences are crossed edges)
    assert shared.numel() >= 2
    p, q = int(shared[0] // n), int(shared[-1] % n)
    assert len({0, n - 1, p, q}) == 4
    label = torch.arange(n)
    label[p], label[0], label[q], label[n - 1] = 0, p, n - 1, q
    dense_v, dense_s = torch.empty_like(v), torch.empty_like(s)
    dense_v[label], dense_s[label] = v, s
    dense = (dense_v, dense_s, label[c], res, beta, alpha, gamma)
    g = torch.Generator().manual_seed(V % 1000003)
    if V == n:
        ids = torch.arange(n)
    else:
        ids = torch.cat([torch.zeros(1, dtype=torch.long), 1 + torch.randperm(V - 2, generator=g)[:n - 2].sort().values,
                         torch.full((1,), V - 1)])
    big_v, big_s = torch.zeros(V, 3), torch.full((V,), -1.0)
    big_v[ids], big_s[ids] = dense_v, dense_s
    return dense, (big_v, big_s, ids[dense[2]], res, beta, alpha, gamma), ids
