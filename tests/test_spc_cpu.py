"""ops.spc on CPU tensors (the torch formulations) against the brute-force decoder of tests/spc_bruteforce.py, and the decoder against
the reference's recorded answers (tests/golden/spc_examples.json).  Every comparison is torch.equal: integers and exact copies.
`check_pipeline` and the helpers are shared with tests/test_spc_gpu.py, which runs them through the HIP path."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

import spc_bruteforce as bf
from conftest import GOLDEN_DIR


def spc():
    import kaolin_amd as kal
    return kal.ops.spc


def fixture():
    with open(os.path.join(GOLDEN_DIR, 'spc_examples.json')) as f:
        return json.load(f)


def t(array, device, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(array), dtype=dtype).to(device)


# ---------------------------------------------------------------------------------------------------------- the decoder is pinned
def test_decoder_matches_reference_batch():
    ex = fixture()['batch']
    pyr = np.array(ex['pyramids'])
    hier = np.array(ex['point_hierarchies'])
    L, first, cubes = ex['max_level'], 0, []
    for b in range(2):                                           # the cube of an item = its recorded points of the last level
        leaves = hier[first + pyr[b, 1, L]:first + pyr[b, 1, L + 1]]
        cubes.append(bf.cube_of_points(leaves, L))
        first += pyr[b, 1, L + 1]
    _, octrees, lengths, pyramids, exsum, points = bf.decode_batch(cubes)
    assert octrees.tolist() == ex['octrees'] and lengths.tolist() == ex['lengths']
    assert pyramids.tolist() == ex['pyramids'] and exsum.tolist() == ex['exsum']
    assert points.tolist() == ex['point_hierarchies'] and len(points) == 27


def test_decoder_matches_reference_docstrings():
    doc = fixture()
    q = doc['query_example']
    d = bf.decode(bf.cube_of_points(q['points'], q['level']))
    assert [bf.query(d, q['level'], c) for c in q['query']] == q['pidx']
    assert [bf.ancestors(d, q['level'], c) for c in q['query']] == q['pidx_with_parents']
    m = doc['morton_example']
    assert [bf.morton_code(*p) for p in m['points']] == m['codes']


# ------------------------------------------------------------------------------------------------------- the package on the fixture
def check_fixture(device):
    S, doc = spc(), fixture()
    ex = doc['batch']
    octrees = torch.tensor(ex['octrees'], dtype=torch.uint8, device=device)
    lengths = torch.tensor(ex['lengths'], dtype=torch.int32)
    max_level, pyramids, exsum = S.scan_octrees(octrees, lengths)
    assert max_level == ex['max_level'] and pyramids.dtype == torch.int32 and pyramids.device.type == 'cpu'
    assert torch.equal(pyramids, torch.tensor(ex['pyramids'], dtype=torch.int32))
    assert exsum.dtype == torch.int32 and exsum.device.type == device
    assert torch.equal(exsum.cpu(), torch.tensor(ex['exsum'], dtype=torch.int32))
    points = S.generate_points(octrees, pyramids, exsum)
    assert points.dtype == torch.int16 and torch.equal(points.cpu(), torch.tensor(ex['point_hierarchies'], dtype=torch.int16))
    q = doc['query_example']
    octree = S.unbatched_points_to_octree(torch.tensor(q['points'], dtype=torch.int16, device=device), q['level'])
    _, _, prefix = S.scan_octrees(octree, torch.tensor([len(octree)], dtype=torch.int32))
    coords = torch.tensor(q['query'], dtype=torch.int16, device=device)
    assert S.unbatched_query(octree, prefix, coords, q['level']).tolist() == q['pidx']
    assert S.unbatched_query(octree, prefix, coords, q['level'], with_parents=True).tolist() == q['pidx_with_parents']
    m = doc['morton_example']
    codes = S.points_to_morton(torch.tensor(m['points'], dtype=torch.int16, device=device))
    assert codes.dtype == torch.long and codes.tolist() == m['codes']
    assert S.morton_to_points(codes).tolist() == m['points']


def test_fixture_cpu():
    check_fixture('cpu')


# ------------------------------------------------------------------------------------------------- every function against the decoder
def check_queries(S, d, octree, exsum, level, device, dtypes=(torch.float32,)):
    """every occupied point of `level` finds itself (arange + the level's offset), its empty neighbours find nothing, and the rows
    with parents are the decoder's ancestor chains"""
    pts = d.level_points[level].astype(np.int64)
    n, res = len(pts), 2 ** level
    want = torch.arange(n) + int(d.pyramid[1, level])
    got = S.unbatched_query(octree, exsum, t(pts, device, torch.int16), level)
    assert got.dtype == torch.long and torch.equal(got.cpu(), want)
    nb = np.concatenate([pts + o for o in ([1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, 1, 0])])     # inside or outside the grid
    cells = np.concatenate([pts, nb])
    centres = (cells + 0.5) / res * 2.0 - 1.0                    # exact in every dtype used (level <= 7: 9 bits)
    want = torch.tensor([bf.query(d, level, c) if (c >= 0).all() and (c < res).all() else -1 for c in cells])
    # with parents the reference truncates 2^level (q / 2 + 1 / 2) toward zero instead of flooring it: cell -1 lands in cell 0
    chains = torch.tensor([bf.ancestors(d, level, c) for c in np.trunc(cells + 0.5).astype(np.int64)]).reshape(-1, level + 1)
    for dtype in dtypes:
        q = t(centres, device, dtype)
        assert torch.equal(S.unbatched_query(octree, exsum, q, level).cpu(), want), dtype
        got = S.unbatched_query(octree, exsum, q, level, with_parents=True)
        assert got.shape == (len(cells), level + 1) and got.dtype == torch.long
        assert torch.equal(got.cpu(), chains), dtype


def check_pipeline(cubes, device, query_dtypes=(torch.float32,)):
    S = spc()
    ds, octrees_np, lengths_np, pyramids_np, exsum_np, points_np = bf.decode_batch(cubes)
    L, B = ds[0].level, len(ds)
    rng = np.random.RandomState(L * 10 + B)
    for d in ds:                                                 # octree build: shuffled, with duplicates; and sorted
        leaves = d.level_points[L]
        pick = np.concatenate([rng.permutation(len(leaves)), rng.randint(0, len(leaves), 5)])
        octree = S.unbatched_points_to_octree(t(leaves[pick], device), L)
        assert octree.dtype == torch.uint8 and torch.equal(octree.cpu(), t(d.octree, 'cpu'))
        octree = S.unbatched_points_to_octree(t(leaves, device), L, sorted=True)
        assert torch.equal(octree.cpu(), t(d.octree, 'cpu'))
    octrees, lengths = t(octrees_np, device), t(lengths_np, 'cpu')
    max_level, pyramids, exsum = S.scan_octrees(octrees, lengths)
    assert max_level == L and pyramids.shape == (B, 2, L + 2) and pyramids.dtype == torch.int32
    assert torch.equal(pyramids, t(pyramids_np, 'cpu')) and torch.equal(exsum.cpu(), t(exsum_np, 'cpu'))
    assert exsum.dtype == torch.int32 and exsum.device.type == device
    points = S.generate_points(octrees, pyramids, exsum)
    assert points.dtype == torch.int16 and torch.equal(points.cpu(), t(points_np, 'cpu'))
    # Morton codes, points, corners
    codes = S.points_to_morton(points.reshape(1, -1, 3))
    assert codes.shape == (1, len(points_np)) and codes.tolist()[0] == [bf.morton_code(*p) for p in points_np]
    assert torch.equal(S.morton_to_points(codes), points.reshape(1, -1, 3))
    corners = S.points_to_corners(points)
    offs = np.array([[j >> 2, (j >> 1) & 1, j & 1] for j in range(8)], dtype=np.int16)
    assert corners.shape == (len(points_np), 8, 3) and torch.equal(corners.cpu(), t(points_np[:, None, :] + offs[None], 'cpu'))
    # per item: level points, queries at the deepest level and one above
    first_byte = first_point = 0
    for b, d in enumerate(ds):
        octree = octrees[first_byte:first_byte + len(d.octree)]
        prefix = exsum[first_byte:first_byte + len(d.octree)]
        hier = points[first_point:first_point + len(d.points)]
        for l in range(L + 1):
            assert torch.equal(S.unbatched_get_level_points(hier, pyramids[b], l).cpu(), t(d.level_points[l], 'cpu'))
        for l in sorted({L, max(L - 1, 0)}):
            check_queries(S, d, octree, prefix, l, device, query_dtypes)
        first_byte += len(d.octree)
        first_point += len(d.points)
    # to_dense at the deepest level (level = -1) and an inner one
    for level in sorted({-1, L // 2} if L <= 6 else {L // 2}):       # (a dense 128^3 grid per channel is not a quick test)
        l = L if level < 0 else level
        for C in (1, 4):
            rows = int(pyramids[:, 0, l].sum())
            x = torch.arange(1, rows * C + 1, dtype=torch.float32).reshape(rows, C)
            want = np.zeros((B, C, 2 ** l, 2 ** l, 2 ** l), dtype=np.float32)
            r = 0
            for b, d in enumerate(ds):
                for px, py, pz in d.level_points[l]:
                    want[b, :, px, py, pz] = x[r].numpy()
                    r += 1
            got = S.to_dense(points, pyramids, x.to(device), level)
            assert got.dtype == torch.float32 and torch.equal(got.cpu(), t(want, 'cpu'))
    return ds, octrees, lengths, pyramids, exsum, points


def cubes_for(level, B):
    return [bf.random_cube(level, 100 * level + b, density=(0.3, 0.05, 0.6)[b] if level <= 2 else None) for b in range(B)]


@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('level', [1, 2, 4, 6])
def test_pipeline_cpu(level, B):
    check_pipeline(cubes_for(level, B), 'cpu', query_dtypes=(torch.float16, torch.float32, torch.float64))


def test_create_dense_spc_and_random_octrees_cpu():
    S = spc()
    from kaolin_amd.utils.testing import random_spc_octrees
    octree, lengths = S.create_dense_spc(2, 'cpu')
    assert octree.tolist() == [255] * 9 and lengths.tolist() == [9] and lengths.dtype == torch.int32
    d = bf.decode(np.ones((4, 4, 4), dtype=bool))
    max_level, pyramids, exsum = S.scan_octrees(octree, lengths)
    assert max_level == 2 and torch.equal(S.generate_points(octree, pyramids, exsum), t(d.points, 'cpu'))
    torch.manual_seed(3)
    octrees, lengths = random_spc_octrees(3, 4, 'cpu')
    max_level, pyramids, _ = S.scan_octrees(octrees, lengths)
    assert max_level == 4 and lengths.dtype == torch.int32 and len(set(lengths.tolist())) > 1
    assert bool((pyramids[:, 0, 4] > 0).all())


def test_uint8_helpers():
    S = spc()
    b = torch.arange(256, dtype=torch.uint8).reshape(16, 16)
    bits = S.uint8_to_bits(b)
    assert bits.shape == (16, 16, 8) and bits.dtype == torch.bool
    assert bits[0, 3].tolist() == [True, True, False, False, False, False, False, False]
    assert torch.equal(S.bits_to_uint8(bits), b) and torch.equal(S.bits_to_uint8(bits.float()), b)
    assert S.uint8_bits_sum(b).reshape(-1).tolist() == [bin(i).count('1') for i in range(256)]
    assert S.quantize_points(torch.tensor([[-1.0, 0.0, 1.0], [-3.0, 0.49, 7.0]]), 2).tolist() == [[0, 2, 3], [0, 2, 3]]


def test_legacy_exsum():
    S = spc()
    _, octrees, lengths, _, exsum_np, _ = bf.decode_batch(cubes_for(2, 3))
    octrees, lengths = t(octrees, 'cpu'), t(lengths, 'cpu')
    with pytest.warns(DeprecationWarning):
        max_level, pyramids, legacy = S.scan_octrees(octrees, lengths, legacy_exsum=True)
    want, first = [], 0
    for n in lengths.tolist():
        want += [0] + exsum_np[first:first + n].tolist()
        first += n
    assert legacy.tolist() == want and legacy.dtype == torch.int32 and legacy.numel() == octrees.numel() + 3
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        S.scan_octrees(octrees, lengths)
    with pytest.raises(ValueError, match='legacy'):
        S.generate_points(octrees, pyramids, legacy)
    with pytest.raises(ValueError, match='legacy'):
        S.unbatched_query(octrees[:lengths[0]], legacy[:lengths[0] + 1], torch.zeros(1, 3), 2)


def test_value_errors():
    S = spc()
    shallow, deep = bf.decode(bf.random_cube(1, 1, 0.5)), bf.decode(bf.random_cube(2, 2, 0.3))
    with pytest.raises(ValueError, match='same depth'):
        S.scan_octrees(t(np.concatenate([shallow.octree, deep.octree]), 'cpu'),
                       torch.tensor([len(shallow.octree), len(deep.octree)], dtype=torch.int32))
    assert len(deep.octree) > 2
    with pytest.raises(ValueError, match='account for'):                          # the last byte is missing
        S.scan_octrees(t(deep.octree[:-1], 'cpu'), torch.tensor([len(deep.octree) - 1], dtype=torch.int32))
    with pytest.raises(ValueError, match='account for'):                          # a byte too many
        S.scan_octrees(t(np.concatenate([deep.octree, [1]]).astype(np.uint8), 'cpu'),
                       torch.tensor([len(deep.octree) + 1], dtype=torch.int32))
    with pytest.raises(ValueError, match='no points'):
        S.unbatched_points_to_octree(torch.zeros((0, 3), dtype=torch.int16), 3)
    assert S.unbatched_points_to_octree(torch.zeros((2, 3), dtype=torch.int16), 0).shape == (0,)


def test_to_dense_rejects_other_keywords():
    S = spc()
    d = bf.decode(bf.random_cube(2, 5, 0.3))
    x = torch.ones(len(d.level_points[2]), 1)
    with pytest.raises(TypeError, match='unexpected keyword'):
        S.to_dense(t(d.points, 'cpu'), t(d.pyramid[None], 'cpu'), x, features=x)


# --------------------------------------------------------------------------------------------------------------- feature grids
def check_feature_grid_round_trip(C, with_masks, device):
    S = spc()
    g = torch.Generator().manual_seed(7 + C)
    B, X, Y, Z = 2, 5, 3, 6
    grids = torch.rand((B, C, X, Y, Z), generator=g) + 0.5
    masks = torch.rand((B, X, Y, Z), generator=g) < 0.4
    masks[0, 4, 2, 5] = True
    grids = grids * masks[:, None]
    if with_masks:
        grids[1, :, 0, 0, 0] = 0.0                                # a masked-in cell whose features are all zero
        masks[1, 0, 0, 0] = True
    octrees, lengths, feats = S.feature_grids_to_spc(grids.to(device), masks.to(device) if with_masks else None)
    cubes = np.zeros((B, 8, 8, 8), dtype=bool)
    cubes[:, :X, :Y, :Z] = masks.numpy()
    ds, octrees_np, lengths_np, _, _, _ = bf.decode_batch(list(cubes))
    assert octrees.dtype == torch.uint8 and torch.equal(octrees.cpu(), t(octrees_np, 'cpu'))
    assert lengths.dtype == torch.int32 and lengths.device.type == 'cpu' and torch.equal(lengths, t(lengths_np, 'cpu'))
    leaves = np.concatenate([np.concatenate([np.full((len(d.level_points[3]), 1), b), d.level_points[3]], 1) for b, d in enumerate(ds)])
    assert torch.equal(feats.cpu(), grids[leaves[:, 0], :, leaves[:, 1], leaves[:, 2], leaves[:, 3]])
    max_level, pyramids, exsum = S.scan_octrees(octrees, lengths)
    points = S.generate_points(octrees, pyramids, exsum)
    dense = S.to_dense(points, pyramids, feats)
    assert max_level == 3 and dense.shape == (B, C, 8, 8, 8)
    want = torch.zeros(B, C, 8, 8, 8)
    want[:, :, :X, :Y, :Z] = grids
    assert torch.equal(dense.cpu(), want)


@pytest.mark.parametrize('with_masks', [False, True])
@pytest.mark.parametrize('C', [1, 3])
def test_feature_grid_round_trip_cpu(C, with_masks):
    check_feature_grid_round_trip(C, with_masks, 'cpu')


# ------------------------------------------------------------------------------------------------------------ to_dense backward
def index_put_to_dense(points, pyramids, x, level):
    """to_dense spelled with index_put on a channels-last grid: what autograd differentiates as the reference of the backward"""
    B, L = pyramids.shape[0], pyramids.shape[2] - 2
    out = torch.zeros((B, 2 ** level, 2 ** level, 2 ** level, x.shape[1]), dtype=x.dtype, device=x.device)
    first_point = row = 0
    for b in range(B):
        n = int(pyramids[b, 0, level])
        p = points[first_point + int(pyramids[b, 1, level]):first_point + int(pyramids[b, 1, level]) + n].long()
        out = out.index_put((torch.full((n,), b, device=x.device), p[:, 0], p[:, 1], p[:, 2]), x[row:row + n])
        first_point += int(pyramids[b, 1, L + 1])
        row += n
    return out.permute(0, 4, 1, 2, 3)


def check_to_dense_backward(cubes, device, level, C, dtype=torch.float64):
    S = spc()
    _, _, _, pyramids_np, _, points_np = bf.decode_batch(cubes)
    pyramids, points = t(pyramids_np, 'cpu'), t(points_np, device)
    l = pyramids.shape[2] - 2 if level < 0 else level
    rows = int(pyramids[:, 0, l].sum())
    g = torch.Generator().manual_seed(rows)
    wide = torch.rand((rows, 2 * C), generator=g, dtype=dtype).to(device)
    w = torch.rand((len(cubes), C, 2 ** l, 2 ** l, 2 ** l), generator=g, dtype=dtype).to(device)
    a = wide.clone().requires_grad_()
    b = wide[:, ::2].clone().requires_grad_()
    assert not a[:, ::2].is_contiguous()
    out = S.to_dense(points, pyramids, a[:, ::2], level)                                      # a non-contiguous input
    ref = index_put_to_dense(points, pyramids, b, l)
    assert out.dtype == dtype and torch.equal(out, ref)
    (out * w).sum().backward()
    (ref * w).sum().backward()
    assert torch.equal(a.grad[:, ::2], b.grad) and not bool(a.grad[:, 1::2].any())
    return out.detach(), a.grad


@pytest.mark.parametrize('level', [-1, 1])
def test_to_dense_backward_cpu(level):
    check_to_dense_backward(cubes_for(3, 3), 'cpu', level, C=2)
