"""The inputs of the unbatched_pointcloud_to_spc boundary suite (helper, not collected; shared by
tests/test_pointcloud_boundaries_cpu.py and tests/test_pointcloud_boundaries_gpu.py).  The segmented mean of csrc/pointcloud.hip cuts
the sorted points into chunks of 128, so a case is a LAYOUT: the run lengths in Morton order, run r at the sorted positions
[sum(len[:r]), sum(len[:r + 1])).  ``layout_cloud`` builds a cloud with exactly these runs, ``describe`` is a pure-Python model of
the kernels' bookkeeping (which chunk writes ``first`` / ``last``, which boundary finishes a run, how many pieces every partial sum
takes -- not of the sums), and every test asserts through it that a layout reaches the branch its docstring names.  The oracle of
a case (tests/pointcloud_bruteforce.py: exact Fractions) is computed once, shared by the tests and never modified."""
import collections
import functools

import numpy as np
import torch

import pointcloud_bruteforce as bf
from test_pointcloud_cpu import features

C = 128                 # sorted positions per chunk of the mean (csrc/pointcloud.hip PC_CHUNK)
WAVE = 64
BLOCK = 256             # threads per block of both kernels of the mean
LEVEL = 8               # the level of every layout: cells of 2^-7, members at multiples of 2^-14 above the centre


# ---- a cloud with given runs ---------------------------------------------------------------------------------------------------------
def cell_of(code, level):
    """the inverse of bf.morton: (x, y, z)"""
    x = y = z = 0
    for i in range(level):
        z |= ((code >> (3 * i)) & 1) << i
        y |= ((code >> (3 * i + 1)) & 1) << i
        x |= ((code >> (3 * i + 2)) & 1) << i
    return x, y, z


def layout_cloud(lengths, level=LEVEL, seed=0):
    """(sum(lengths), 3) float64, exact in float32: len(lengths) distinct cells of `level` with ascending Morton codes, lengths[r]
    distinct points inside cell r (the centre plus (i, j, k) 2^-(level + 6), i, j, k < 32: within a quarter of the cell), the rows under
    one seeded permutation, so that the members of a cell are scattered over the input"""
    assert 1 <= level <= 12 and all(1 <= n <= 32 ** 3 for n in lengths)
    rs = np.random.RandomState(seed)
    codes = set()
    while len(codes) < len(lengths):
        codes.update(rs.randint(0, 8 ** level, len(lengths) - len(codes), dtype=np.int64).tolist())
    size, fine = 2.0 / (1 << level), 2.0 ** -(level + 6)
    rows = []
    for code, n in zip(sorted(codes), lengths):
        centre = -1.0 + (np.array(cell_of(code, level), dtype=np.float64) + 0.5) * size
        t = np.arange(n)
        rows.append(centre + np.stack([t & 31, (t >> 5) & 31, t >> 10], 1) * fine)
    pts = np.concatenate(rows)[rs.permutation(sum(lengths))]
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts) and len(np.unique(pts, axis=0)) == len(pts)
    return torch.from_numpy(pts)


# ---- the bookkeeping of pc_mean_chunks_kernel / pc_mean_runs_kernel ------------------------------------------------------------------
Run = collections.namedtuple('Run', 's e k0 k1 on_start on_end owner pieces')
Description = collections.namedtuple('Description', 'n nchunks DL G runs kinds runs_kernel chunks_per_block')


def lanes(D):
    DL = 1
    while DL < WAVE and DL < D:
        DL *= 2
    return DL


def describe(lengths, D):
    """Per run: its positions [s, e), its first and last chunk k0, k1, whether s / e is a multiple of 128, the boundary (= the chunk
    behind it) whose wavefront finishes it (None: the run lies in one chunk and pc_mean_chunks_kernel stores it) and how many
    ``first`` pieces each of the G partial sums adds (partial 0 also starts from ``last[k0]``).  Per chunk: what it writes of
    'first' (its position 0 is no head) and 'last' (it holds a head and the run of its last position goes on): 'first', 'last',
    'both' or 'none'."""
    n = sum(lengths)
    nchunks = (n + C - 1) // C
    DL = lanes(D)
    G = WAVE // DL
    starts = np.concatenate([[0], np.cumsum(lengths)]).tolist()
    heads = set(starts[:-1])
    runs = []
    for s, e in zip(starts[:-1], starts[1:]):
        k0, k1 = s // C, (e - 1) // C
        pieces = [len(range(k0 + 1 + g, k1 + 1, G)) for g in range(G)] if k1 > k0 else None
        runs.append(Run(s, e, k0, k1, s % C == 0, e % C == 0, k0 + 1 if k1 > k0 else None, pieces))
    kinds = []
    for k in range(nchunks):
        j0, j1 = k * C, min(k * C + C, n)
        first = j0 not in heads
        last = j1 < n and j1 not in heads and any(j in heads for j in range(j0, j1))
        kinds.append('both' if first and last else 'first' if first else 'last' if last else 'none')
    return Description(n, nchunks, DL, G, runs, kinds, nchunks > 1, BLOCK // DL)


def runs_kernel_slot(boundary):
    """(block, wavefront) of pc_mean_runs_kernel that takes the boundary (boundaries count from 1, four wavefronts per block)"""
    return (boundary - 1) // (BLOCK // WAVE), (boundary - 1) % (BLOCK // WAVE)


# ---- the layouts ---------------------------------------------------------------------------------------------------------------------
class Layout:
    """run lengths, the feature width the layout runs at by default, the `describe` facts it must show: `kinds` per chunk (a
    string of n / f / l / b) or None, `crossing` {run: (k0, k1)} of the runs that pc_mean_runs_kernel finishes; the docstring of an
    instance names the branch of csrc/pointcloud.hip it is for"""

    def __init__(self, lengths, doc, kinds=None, crossing=(), D=3):
        self.lengths, self.__doc__, self.kinds, self.D = list(lengths), doc, kinds, D
        self.crossing = None if crossing is None else dict(crossing)


LAYOUTS = {
    # a single chunk: pc_mean_runs_kernel is not launched
    'chunk_one_run': Layout([128], 'one full chunk, one run: stored at the end of the chunk loop with j1 == n, no second kernel', 'n'),
    'chunk_127_1': Layout([127, 1], 'a head at the last position of the only chunk: a run of one stored behind the loop', 'n'),
    'chunk_singles': Layout([1] * 128, '128 runs of one: every position of the chunk is a head, every store inside the loop', 'n'),
    # one boundary
    'tail_129': Layout([129], 'the tail chunk is one headless element: chunk 1 writes `first` only, boundary 1 adds one piece', 'lf',
                       {0: (0, 1)}),
    'ends_on_boundary': Layout([128, 1], 'the run ends on the boundary (flag[j] leaves the wavefront), the last chunk is one complete '
                               'run with j1 == n', 'nn'),
    'one_each_side': Layout([127, 2], 'a run of two with one element on each side of the boundary', 'lf', {1: (0, 1)}),
    'single_127_single': Layout([1, 127, 1], 'a run from position 1 to the boundary: stored by the chunk although it touches the '
                                'boundary, whose wavefront leaves at flag[j]; the last chunk is a run of one', 'nn'),
    'every_run_a_chunk': Layout([128, 128, 128], 'every run is exactly one chunk: neither `first` nor `last` is used, every boundary '
                                'wavefront leaves at flag[j]', 'nnn'),
    # aligned long runs: the head sits at j0, s == k0 * 128 in the ownership test
    'aligned_256': Layout([256], 'the head at j0 of chunk 0 (the j > j0 test skips the store), one headless chunk', 'lf', {0: (0, 1)}),
    'aligned_384': Layout([384], 'as aligned_256 with a headless interior chunk that goes on', 'lff', {0: (0, 2)}),
    'aligned_middle': Layout([128, 256, 128], 'an aligned crossing run between two one-chunk runs: s == k0 * 128 with k0 = 1', 'nlfn',
                             {1: (1, 2)}),
    'mid_start_mid_end': Layout([100, 28 + 256 + 50, 78], 'a run from the middle of chunk 0 over two whole chunks into the middle of '
                                'chunk 3, whose last chunk holds a `first` piece and then a complete run', 'lfff', {1: (0, 3)}),
    'first_runs_last': Layout([200, 10, 10, 300], 'chunk 1 holds a `first` piece, two complete runs and a `last` piece', 'lbfff',
                              {0: (0, 1), 3: (1, 4)}),
    'ownership': Layout([50, 600, 30], 'a run over five boundaries: only the first may finish it (s < k0 * 128 for the other four)',
                        'lfffff', {1: (0, 5)}),
    'short_crossing': Layout([120, 16, 120], 'a run of 16 over the boundary, a complete run behind its `first` piece up to j1 == n',
                             'lf', {1: (0, 1)}),
    'two_crossing': Layout([120, 130, 120], 'two crossing runs back to back: chunk 1 writes `first` for one and `last` for the next',
                           'lbf', {1: (0, 1), 2: (1, 2)}),
    # block edges of pc_mean_runs_kernel: four boundary wavefronts per block
    'runs_block_edge': Layout([639, 5], 'the second run crosses boundary 5 = wavefront 0 of the second block; the first run is owned by '
                              'boundary 1 and refused by 2, 3, 4', 'lfffbf', {0: (0, 4), 1: (4, 5)}),
    'runs_block_last_wave': Layout([511, 2, 131], 'boundary 4 = wavefront 3 of the first block finishes a run of two (one element on each '
                                   'side), boundary 5 = wavefront 0 of the second block the run behind it', 'lffbbf',
                                   {0: (0, 3), 1: (3, 4), 2: (4, 5)}),
    'open_last_run': Layout([100, 156], 'n is a multiple of 128 and the last run is open into the last chunk: j1 == n is no open '
                            'end, the headless last chunk writes `first`', 'lf', {1: (0, 1)}),
    # block edges of pc_mean_chunks_kernel: 256 / DL chunks per block
    'chunks_block_edge_d64': Layout([50, 600, 30], 'D = 64: four chunks per block, the run of `ownership` has pieces in both blocks',
                                    'lfffff', {1: (0, 5)}, D=64),
    'chunks_block_edge_d1': Layout([100] * 327 + [200], 'D = 1: 256 chunks per block; the last run crosses position 32768, the first '
                                   'chunk of the second block', None, None, D=1),
}

# lane groups: G = 64 / DL partial sums take the chunks behind the first in turn; m + 1 pieces over G partials give partials with
# zero, one, two and three pieces, and the butterfly runs from six steps (DL = 1) to none (DL = 64)
LANE_WIDTHS = [(1, 64), (2, 32), (3, 16), (8, 8), (32, 2), (64, 1)]
LANE_CASES = []            # (name, D, G, m)


def lane_layout(m):
    return [37, 91 + 128 * m + 5, 60]


for _D, _G in LANE_WIDTHS:
    for _m in sorted({0, 1, _G - 1, _G, _G + 1, 2 * _G, 2 * _G + 1}):
        _name = f'lanes_d{_D}_m{_m}'
        LAYOUTS[_name] = Layout(lane_layout(_m), f'D = {_D}: {_G} partial sums share the {_m + 1} `first` pieces of the middle run',
                                'l' + 'f' * (_m + 1), {1: (0, _m + 1)}, D=_D)
        LANE_CASES.append((_name, _D, _G, _m))

# several d0 iterations of the runs kernel (D > 64): the lane mask `on` is partially live in the last one
WIDE = [65, 128, 129, 130]
for _D in WIDE:
    LAYOUTS[f'wide_lanes_d{_D}'] = Layout(lane_layout(2), f'D = {_D}: {(_D + 63) // 64} d0 iterations, {_D % 64 or 64} live lanes in '
                                          'the last one', 'lfff', {1: (0, 3)}, D=_D)
    LAYOUTS[f'wide_first_runs_last_d{_D}'] = Layout([200, 10, 10, 300], f'first_runs_last at D = {_D}', 'lbfff', {0: (0, 1), 3: (1, 4)},
                                                    D=_D)

NAMES = list(LAYOUTS)
LARGEST = ['lanes_d1_m129', 'chunks_block_edge_d1']        # the two that the CPU suite leaves to the oracle and the GPU
KIND = {'n': 'none', 'f': 'first', 'l': 'last', 'b': 'both'}


def seed_of(name):
    return sum(map(ord, name))


@functools.lru_cache(maxsize=None)
def points_of(name):
    return layout_cloud(LAYOUTS[name].lengths, LEVEL, seed_of(name))


@functools.lru_cache(maxsize=None)
def case(name, feature_dtype=torch.float32, D=None, scale=1):
    """(points float32, features (n, D), oracle) of a layout, computed once, never modified; D: the layout's own unless given;
    `scale` multiplies the features (int64: k 2^40)"""
    pts = points_of(name).float()
    feats = features(pts.shape[0], D or LAYOUTS[name].D, feature_dtype, name)
    feats = feats if scale == 1 else feats * scale
    assert feats.dtype == feature_dtype
    return pts, feats, bf.Oracle(pts.numpy(), LEVEL, feats.numpy())


def check_layout(name, oracle=None):
    """the layout is what it claims -> its Description"""
    lay = LAYOUTS[name]
    d = describe(lay.lengths, lay.D)
    assert d.n == sum(lay.lengths) and d.G * d.DL == WAVE and d.DL >= min(lay.D, WAVE) and (d.DL == 1 or d.DL < 2 * lay.D)
    if lay.kinds is not None:
        assert d.kinds == [KIND[c] for c in lay.kinds], (name, d.kinds)
    if lay.crossing is not None:
        assert {r: (run.k0, run.k1) for r, run in enumerate(d.runs) if run.owner is not None} == lay.crossing
    for run in d.runs:
        if run.owner is not None:                  # the owner is the only boundary inside the run with s >= (b - 1) * 128
            inside = [b for b in range(1, d.nchunks) if run.s < b * C < run.e]
            assert [b for b in inside if run.s >= (b - 1) * C] == [run.owner] and len(inside) == run.k1 - run.k0
            assert sum(run.pieces) == run.k1 - run.k0 and max(run.pieces) - min(run.pieces) <= 1
            assert d.kinds[run.k0] in ('last', 'both') and all(d.kinds[k] in ('first', 'both') for k in range(run.k0 + 1, run.k1 + 1))
    assert d.runs_kernel == (d.nchunks > 1)
    if oracle is not None:
        assert [len(m) for m in oracle.members] == lay.lengths
    return d


# ---- designed ties of the integer means ------------------------------------------------------------------------------------------------
TIES = [2] * 7 + [4, 3, 3, 110, 40]        # short runs, one run of 110 over the boundary at 128, one run of random values behind it
TIE_CROSSING = 10
_SIGNED = {0: ((1, 2), 2), 1: ((2, 3), 2), 2: ((-1, -2), -2), 3: ((0, 1), 0), 4: ((3, 4), 4), 5: ((-3, -2), -2), 6: ((-128, -127), -128),
           7: ((5, -3, 1, -1), 0), 8: ((1, 1, 2), 1), 9: ((0, 0, 1), 0), 10: ((1, 2) * 55, 2)}
_UINT8 = {0: ((1, 2), 2), 1: ((2, 3), 2), 2: ((255, 254), 254), 3: ((0, 1), 0), 4: ((255, 255), 255), 5: ((253, 254), 254),
          6: ((3, 4), 4), 7: ((1, 1, 0, 0), 0), 8: ((1, 1, 2), 1), 9: ((0, 0, 1), 0), 10: ((255, 254) * 55, 254)}
_BOOL = {0: ((1, 0), 0), 1: ((1, 1), 1), 2: ((0, 0), 0), 3: ((0, 1), 0), 4: ((1, 0), 0), 5: ((0, 1), 0), 6: ((1, 0), 0),
         7: ((1, 1, 0, 0), 0), 8: ((1, 1, 0), 1), 9: ((1, 0, 0), 0), 10: ((1, 0) * 55, 0)}
TIE_VALUES = {torch.bool: _BOOL, torch.uint8: _UINT8, torch.int8: _SIGNED, torch.int16: _SIGNED, torch.int32: _SIGNED,
              torch.int64: _SIGNED}
NOT_A_TIE = {torch.bool: (1, 2, 8, 9), torch.uint8: (4, 8, 9)}       # the designed rows whose exact mean is not x.5 (other dtypes: 8, 9)


@functools.lru_cache(maxsize=None)
def tie_case(dtype):
    """(points, features (n, 2), oracle, {run: hand-written mean of column 0}): column 0 of run r holds TIE_VALUES[dtype][r] in
    the order of the members, the last run and column 1 hold seeded values"""
    pts = layout_cloud(TIES, LEVEL, 77).float()
    members = bf.Oracle(pts.numpy(), LEVEL).members
    assert [len(m) for m in members] == TIES
    feats = features(pts.shape[0], 2, dtype, 'ties').clone()
    want = {}
    for r, (values, mean) in TIE_VALUES[dtype].items():
        assert len(values) == TIES[r]
        feats[torch.tensor(members[r]), 0] = torch.tensor(values).to(dtype)
        want[r] = mean
    return pts, feats, bf.Oracle(pts.numpy(), LEVEL, feats.numpy()), want


# ---- keys and sort ---------------------------------------------------------------------------------------------------------------------
TOP_BIT_PAIR = [[-0.75, 0.3125, -0.4375], [0.25, 0.3125, -0.4375]]      # x + 1 = 0.25 and 1.25: the x cells differ by 2^(level - 1)


@functools.lru_cache(maxsize=None)
def sweep_case(level, point_dtype):
    """300 seeded points and TOP_BIT_PAIR with one feature column -> (points, features, oracle)"""
    g = torch.Generator().manual_seed(4242)
    pts = torch.cat([(torch.rand((300, 3), generator=g) * 2 - 1).float().double(), torch.tensor(TOP_BIT_PAIR, dtype=torch.float64)])
    pts = pts[torch.randperm(302, generator=g)].to(point_dtype)
    feats = features(302, 1, torch.float32, 'sweep')
    return pts, feats, bf.Oracle(pts.numpy(), level, feats.numpy())


def border_values(level, dtype):
    """the coordinates on the cell borders -1 + 2 k / 2^level for k in {0, 1, 2^(level - 1), 2^level - 1, 2^level}, each with its
    neighbours below and above in `dtype` (numpy), and the values at which x + 1 itself rounds"""
    res = 1 << level
    dt = np.dtype(dtype).type
    vals = []
    for k in sorted({0, 1, res // 2, res - 1, res}):
        x = dt(-1.0 + 2.0 * k / res)
        assert float(x) == -1.0 + 2.0 * k / res                    # a border is exact in every dtype at the levels it is used at
        vals += [np.nextafter(x, dt(-np.inf)), x, np.nextafter(x, dt(np.inf))]
    vals += [np.nextafter(dt(1), dt(0)), dt(-2.0 ** -25), dt(-2.0 ** -26), np.nextafter(dt(-1), dt(0))]
    return np.array(vals, dtype=dtype)


@functools.lru_cache(maxsize=None)
def border_case(level, point_dtype):
    """every border value on every axis (the other two axes at seeded border values too) -> (points, None, oracle)"""
    vals = border_values(level, torch.empty(0, dtype=point_dtype).numpy().dtype)
    rs = np.random.RandomState(level)
    pts = np.concatenate([np.stack([np.roll([v, vals[rs.randint(len(vals))], vals[rs.randint(len(vals))]], axis) for v in vals])
                          for axis in range(3)]).astype(vals.dtype)
    pts = torch.from_numpy(pts)
    return pts, None, bf.Oracle(pts.numpy(), level)


# ---- the worst share of the oracle's bound per dtype over the layouts ---------------------------------------------------------------
WORST = {}


def record(device, dtype, name, share):
    if share is not None and share > WORST.get((device, dtype), (-1.0, ''))[0]:
        WORST[(device, dtype)] = (share, name)


def report(device):
    for (dev, dtype), (share, name) in sorted(WORST.items(), key=str):
        if dev == device:
            print(f'pointcloud_to_spc boundaries {dev} {dtype}: worst share of the bound {share:.4f} at {name}')
