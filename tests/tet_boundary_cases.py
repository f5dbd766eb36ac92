"""Inputs that put the tetrahedral pipelines (csrc/sort_scan.h under csrc/marching_tetrahedra.hip and csrc/subdivide_tetmesh.hip)
on the boundaries of their sort, scans and compaction: exact numbers of crossing-edge instances and of tets around the block
sizes 64 / 256 / 1024 / 2048, vertex counts on either side of every radix pass count, long runs of equal keys, high valence, and
the DMTet loop.  Pure torch on the CPU, seeded by torch.Generator.  Every builder returns

    vertices (B, V, 3) float32, tets (T, 4) int64, sdf (B, V) float32, name

test_tet_boundary_cases_cpu.py checks that every case is what it claims to be; test_tet_pipelines_boundaries_gpu.py runs them
through the kernels."""
import torch

from kaolin_amd.utils.testing import kuhn_grid

ONE_TRIANGLE_CASES = (1, 2, 4, 8, 7, 11, 13, 14)      # one or three corners occupied
TWO_TRIANGLE_CASES = (3, 5, 6, 9, 10, 12)             # two corners occupied

INSTANCE_COUNTS = (255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097)      # n = nu of `disjoint`
TET_COUNTS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 4097)              # T of `disjoint`, mixed cases
SOUP_V = (2, 5, 255, 256, 257, 65535, 65536, 65537)                                    # V of `random_soup`
BIG_V = 2 ** 24 + 1000                                                                 # ... and the four-pass case
ST_TET_COUNTS = (1, 2, 42, 43, 170, 171, 255, 256, 257, 341, 342, 683)                 # 6 T around 256, 1024, 2048, 4096


def cdiv(a, b):
    return (a + b - 1) // b


def id_bits(V):
    """csrc: mt_id_bits / st_id_bits, restated"""
    nb = 1
    while nb < 32 and (1 << nb) < V:
        nb += 1
    return nb


def passes_per_half(V):
    """csrc: the 8-bit radix passes over one half of the keys (st_passes_per_half; the `shift < mt_id_bits` loop)"""
    return (id_bits(V) + 7) // 8


def counts_for_instances(n):
    """16 counts per sign case whose tets have exactly n crossing-edge instances, 3 n_one + 4 n_two = n, both kinds present,
    with some tets of the cases 0 and 15 between them."""
    n_two = n // 8
    while n_two % 3 != n % 3:
        n_two -= 1
    n_one = (n - 4 * n_two) // 3
    assert n_one > 0 and n_two > 0 and 3 * n_one + 4 * n_two == n
    counts = [0] * 16
    for k in range(n_one):
        counts[ONE_TRIANGLE_CASES[k % 8]] += 1
    for k in range(n_two):
        counts[TWO_TRIANGLE_CASES[k % 6]] += 1
    counts[0], counts[15] = n_one // 5 + 1, n_one // 7 + 1
    return counts


def counts_for_tets(T):
    """16 counts per sign case that sum to T, dealt round-robin (the valid cases first: T = 1 is one two-triangle tet)."""
    order = (6,) + ONE_TRIANGLE_CASES + tuple(c for c in TWO_TRIANGLE_CASES if c != 6) + (0, 15)
    counts = [0] * 16
    for k in range(T):
        counts[order[k % 16]] += 1
    return counts


def disjoint(case_counts, V_pad=0, seed=0):
    """T = sum(case_counts) tets on 4 T fresh vertices (no two tets share one), ids shuffled over [0, 4 T + V_pad), corners in
    random order, the tets of the 16 sign cases interleaved evenly.  n = 3 n_one + 4 n_two and nu = n exactly."""
    g = torch.Generator().manual_seed(seed)
    case = torch.cat([torch.full((c,), k, dtype=torch.long) for k, c in enumerate(case_counts)])
    T = case.shape[0]
    # stratified shuffle: the k-th of a case's c tets lands at a random place in the k-th of c equal stretches of the list, so
    # every case is spread over the whole list in proportion to its count and no stretch of tets is short of one
    place = torch.cat([(torch.arange(c) + torch.rand(c, generator=g)) / c for c in case_counts if c > 0])
    case = case[place.argsort()]
    V = 4 * T + V_pad
    tets = torch.randperm(V, generator=g)[:4 * T].view(T, 4)
    sdf = (torch.rand(V, generator=g) + 0.2) * (torch.randint(2, (V,), generator=g) * 2 - 1).float()
    occupied = ((case.unsqueeze(1) >> torch.arange(4)) & 1).bool()
    sdf[tets] = sdf[tets].abs() * torch.where(occupied, 1.0, -1.0)
    vertices = torch.rand(1, V, 3, generator=g)
    return vertices, tets, sdf[None], f'disjoint_T{T}_V{V}'


def random_soup(T, V, seed=0, used=None, B=1):
    """T tets whose corners are drawn uniformly from `used` (all of [0, V) by default): any corner order, ~2 % exact
    duplicates, ~1 % with a repeated corner; sdf ~ N(0, 1) with |sdf| >= 0.05 (about 7/8 of the tets are cut).  Tet 0 holds the
    largest id V - 1 and is cut through one of that vertex's edges."""
    g = torch.Generator().manual_seed(seed)
    if used is None:
        used = torch.arange(V)
    tets = used[torch.randint(used.shape[0], (T, 4), generator=g)]
    dup = torch.randperm(T, generator=g)[:max(1, T // 50)]
    tets[dup] = tets[torch.randint(T, dup.shape, generator=g)]
    rep = torch.randperm(T, generator=g)[:max(1, T // 100)]
    tets[rep, 3] = tets[rep, 1]
    sdf = torch.randn(B, V, generator=g)
    sdf = torch.where(sdf.abs() < 0.05, torch.where(sdf < 0, -0.05, 0.05), sdf)
    other = int(used[used != V - 1][0])
    tets[0, 0], tets[0, 1] = V - 1, other
    sdf[:, V - 1], sdf[:, other] = sdf[:, V - 1].abs(), -sdf[:, other].abs()
    vertices = torch.rand(B, V, 3, generator=g)
    return vertices, tets, sdf, f'soup_T{T}_V{V}'


def big_soup(seed=0):
    """The four-pass case: V = 2^24 + 1000, 20 000 tets on 3 000 random ids and every id in [2^24 - 8, 2^24 + 1000)."""
    g = torch.Generator().manual_seed(seed + 1)
    used = torch.cat([torch.randint(2 ** 24 - 8, (3000,), generator=g), torch.arange(2 ** 24 - 8, BIG_V)])
    return random_soup(20000, BIG_V, seed, used)


def repeated(T, alternate=False):
    """One two-triangle tet T times over (nu = 4, n = 4 T, E = 6); with `alternate`, in turns with a one-triangle tet that
    shares its edge (1, 3)."""
    sdf = torch.tensor([[-0.5, 0.7, 0.9, -0.3, -1.1, -0.6]])
    rows = torch.tensor([[2, 0, 3, 1], [4, 1, 5, 3]])
    tets = rows[torch.arange(T) % 2] if alternate else rows[:1].expand(T, 4).contiguous()
    g = torch.Generator().manual_seed(T)
    vertices = torch.rand(1, 6, 3, generator=g)
    return vertices, tets, sdf, f'repeated_T{T}' + ('_alternating' if alternate else '')


def fan(K, V=70000, seed=0):
    """K tets around the edge (0, 1); vertex 0 is the only occupied one; the 2 K other corners are distinct ids scattered over
    [2, V).  n = 3 K, nu = 2 K + 1, and the key (0, 1) comes K times."""
    g = torch.Generator().manual_seed(seed)
    rim = torch.randperm(V - 2, generator=g)[:2 * K].view(K, 2) + 2
    tets = torch.cat([torch.tensor([[0, 1]]).expand(K, 2), rim], dim=1)
    tets = torch.gather(tets, 1, torch.rand(K, 4, generator=g).argsort(dim=1))
    sdf = -(torch.rand(1, V, generator=g) + 0.2)
    sdf[0, 0] = 0.7
    vertices = torch.rand(1, V, 3, generator=g)
    return vertices, tets, sdf, f'fan_K{K}'


def star(K, hub_last=False, seed=0):
    """tets[i] = (0, 3 i + 1, 3 i + 2, 3 i + 3), vertex 0 the only occupied one: it has 3 K crossing edges, and is the min end
    of 3 K of the 6 K edges.  With `hub_last` the hub and the last vertex swap ids: the max end of 3 K edges."""
    g = torch.Generator().manual_seed(seed + K)
    V = 3 * K + 1
    rim = torch.arange(1, V).view(K, 3)
    tets = torch.cat([torch.zeros(K, 1, dtype=torch.long), rim], dim=1)
    sdf = -(torch.rand(1, V, generator=g) + 0.2)
    sdf[0, 0] = 0.7
    vertices = torch.rand(1, V, 3, generator=g)
    if hub_last:
        swap = torch.arange(V)
        swap[0], swap[V - 1] = V - 1, 0
        tets, sdf, vertices = swap[tets], sdf[:, swap], vertices[:, swap]
    return vertices, tets, sdf, f'star_K{K}' + ('_hub_last' if hub_last else '')


def permuted_kuhn_grid(n, seed=0):
    """kuhn_grid(n) with its ids relabelled by a random permutation, the tets shuffled and the corners of each in random
    order -> vertices (V, 3), tets (T, 4)"""
    g = torch.Generator().manual_seed(seed + n)
    vertices, tets = kuhn_grid(n)
    V = vertices.shape[0]
    new_id = torch.randperm(V, generator=g)
    moved = torch.empty_like(vertices)
    moved[new_id] = vertices
    tets = new_id[tets][torch.randperm(tets.shape[0], generator=g)]
    return moved, torch.gather(tets, 1, torch.rand(tets.shape, generator=g).argsort(dim=1))


def dense_signs(n=12, seed=0):
    """permuted_kuhn_grid(n) under three sdfs of random sign: all 16 cases inside every wavefront; an item that is positive
    everywhere; an item with +-0.0, NaN and +-inf entries."""
    vertices, tets = permuted_kuhn_grid(n, seed)
    g = torch.Generator().manual_seed(seed + 100)
    V = vertices.shape[0]
    sdf = torch.randn(3, V, generator=g)
    sdf[1] = sdf[1].abs() + 0.1
    special = torch.tensor([0.0, -0.0, float('nan'), float('inf'), -float('inf')])
    where = torch.randperm(V, generator=g)[:V // 8]
    sdf[2, where] = special[torch.arange(where.shape[0]) % 5]
    return vertices[None].expand(3, -1, -1).contiguous(), tets, sdf, f'dense_signs_{n}'


def dmtet_start(n=6, seed=0):
    """kuhn_grid(n), jittered, with a sphere sdf as a one-channel feature -> vertices (1, V, 3), tets, feature (1, V, 1)"""
    g = torch.Generator().manual_seed(seed + n)
    vertices, tets = kuhn_grid(n)
    vertices = vertices + (torch.rand(vertices.shape, generator=g) - 0.5) * (0.3 / n)
    sdf = 0.37 - (vertices - torch.tensor([0.48, 0.53, 0.5])).norm(dim=-1)
    return vertices[None], tets, sdf[None, :, None]


def dmtet_rounds(subdivide, n=6, rounds=2, device='cpu', seed=0):
    """The DMTet loop: round r + 1's input is round r's `subdivide(vertices, tets, feature)` output.  -> the rounds + 1 states
    (vertices, tets, feature), the start included."""
    vertices, tets, feature = (x.to(device) for x in dmtet_start(n, seed))
    states = [(vertices, tets, feature)]
    for _ in range(rounds):
        vertices, tets, feature = subdivide(vertices, tets, feature)
        states.append((vertices, tets, feature))
    return states


def sign_cases(tets, sdf):
    """sdf (V) -> the sign case 0..15 of every tet"""
    return ((sdf > 0)[tets].long() << torch.arange(4)).sum(-1)


def fewest_cases_in_a_window(case, width=64):
    """the smallest number of distinct sign cases among `width` consecutive tets (any start, the last stretch included)"""
    running = torch.cat([torch.zeros(1, 16, dtype=torch.long), torch.nn.functional.one_hot(case, 16).cumsum(0)])
    return int(((running[width:] - running[:-width]) > 0).sum(dim=1).min())


def mt_counts(formulation, vertices, tets, sdf):
    """n_one, n_two, n, nu of one item, read off the marching-tetrahedra formulation's results"""
    verts, faces, tet_idx = formulation(vertices, tets, sdf, True)
    surface_tets = int(torch.unique(tet_idx).numel())
    n_two = faces.shape[0] - surface_tets
    n_one = surface_tets - n_two
    return n_one, n_two, 3 * n_one + 4 * n_two, verts.shape[0]


def crossing_edges(tets, sdf):
    """(a, b), a < b: the unique edges of the tets with exactly one end occupied, ascending"""
    occ = sdf > 0
    pairs = torch.cat([tets[:, [i, j]] for i in range(4) for j in range(i + 1, 4)])
    pairs = pairs[occ[pairs[:, 0]] != occ[pairs[:, 1]]]
    pairs = torch.unique(torch.sort(pairs, dim=1).values, dim=0)
    return pairs[:, 0], pairs[:, 1]


def mt_term_abs_sums(vertices, tets, sdf, cot):
    """vertices (V, 3), sdf (V), cot (nu, 3) -> per element of grad vertices and of grad sdf, the sum of the magnitudes of the
    terms the backward adds up, in float64 (the formula of tests/golden/make_golden_marching_tetrahedra.py::term_abs_sums)."""
    p, s, g = vertices.double(), sdf.double(), cot.double()
    a, b = crossing_edges(tets, sdf)
    d = s[a] - s[b]
    v = (p[a] * (-s[b]).unsqueeze(1) + p[b] * s[a].unsqueeze(1)) / d.unsqueeze(1)
    tv = torch.zeros_like(p)
    ts = torch.zeros_like(s)
    tv.index_add_(0, a, ((-s[b] / d).unsqueeze(1) * g).abs())
    tv.index_add_(0, b, ((s[a] / d).unsqueeze(1) * g).abs())
    ts.index_add_(0, a, ((g * (p[b] - v)).abs().sum(1) / d.abs()))
    ts.index_add_(0, b, ((g * (v - p[a])).abs().sum(1) / d.abs()))
    return tv, ts


def st_term_abs_sums(V, edges, cot):
    """cot (B, V + E, C), edges (E, 2) -> (B, V, C) float64: |g[v]| + 1/2 sum of |g[V + e]| over the edges holding v (a
    self-edge holds v twice)."""
    g = cot.double().abs()
    tas = g[:, :V].clone()
    tas.index_add_(1, edges[:, 0], 0.5 * g[:, V:])
    tas.index_add_(1, edges[:, 1], 0.5 * g[:, V:])
    return tas


def cotangent(shape, seed=0):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed + 77))


def mt_gradients(run, vertices, tets, sdf, cot, dtype, device='cpu'):
    """run(vertices (1, V, 3), tets, sdf (1, V)) -> verts (nu, 3).  -> the gradients of sum(verts * cot) with respect to
    vertices[0] and sdf[0], on the CPU"""
    p, s = (x.detach().to(device, dtype, copy=True).requires_grad_() for x in (vertices, sdf))
    verts = run(p, tets.to(device), s)
    (verts * cot.to(device, dtype)).sum().backward()
    return p.grad[0].cpu(), s.grad[0].cpu()


def st_gradients(run, vertices, tets, features, cot_v, cot_f, dtype, device='cpu'):
    """run(vertices, tets, features) -> (new_vertices, new_tets, new_features).  -> the gradients of the two cotangent sums with
    respect to vertices and features, on the CPU"""
    p, f = (x.detach().to(device, dtype, copy=True).requires_grad_() for x in (vertices, features))
    new_vertices, _, new_features = run(p, tets.to(device), f)
    ((new_vertices * cot_v.to(device, dtype)).sum() + (new_features * cot_f.to(device, dtype)).sum()).backward()
    return p.grad.cpu(), f.grad.cpu()


def unique_edges(tets):
    """(E, 2): the unique (min, max) edges of the tets, ascending"""
    pairs = torch.cat([tets[:, [i, j]] for i in range(4) for j in range(i + 1, 4)])
    return torch.unique(torch.sort(pairs, dim=1).values, dim=0)
