"""The scenes of deftet_boundary_cases.py without a GPU: the restated dispatch rules give the grid resolutions and scan sizes
the pixel-count edges are named for, every scene feeds the kernels it claims to feed (by the restated rules) and produces the
hits it claims to produce (by the CPU oracle), and on the backward sweep's scene the float oracle's own error stays small
enough that the floor of the GPU tests' bound cannot hide a failure."""
import functools

import numpy as np
import pytest
import torch

import deftet_boundary_cases as dbc
import oracle
from render_helper_cases import CONDITIONED_E32

F32, F64 = torch.float32, torch.float64
BACKWARD_D = (1, 2, 3, 4, 5, 8)
BACKWARD_K = 48

mixed = functools.lru_cache(maxsize=None)(dbc.mixed)


def forward(case, K, dtype=F32, bb=None):
    pix, ranges, z, img = (t.to(dtype) for t in case[:4])
    bb = dbc.boxes_of(img) if bb is None else bb.to(dtype)
    return oracle.deftet_sparse_render_forward(z, img, bb, pix, ranges, K, 1e-8, omp=True)


def kinds_of(case, b):
    pix, _, _, img = case[:4]
    return dbc.handover(pix[b], dbc.boxes_of(img)[b], pix.shape[1])


def test_grid_resolutions_and_scan_blocks():
    assert [dbc.gshift(P) for P in dbc.P_EDGES] == [4, 5, 5, 6, 6, 7, 7, 8]
    assert [dbc.scan_blocks(P) for P in dbc.P_EDGES] == [1, 1, 1, 4, 4, 16, 16, 64]
    assert dbc.gshift(1) == 4 and dbc.gshift(1 << 20) == 8 and dbc.gshift(1 << 30) == 8


def test_sort_path_edge():
    B, P, (k_lo, k_hi) = dbc.KH_EDGE['B'], dbc.KH_EDGE['P'], dbc.KH_EDGE['K']
    assert B * P * k_lo == 4178430 < 2 ** 22 <= 4194816 == B * P * k_hi
    assert dbc.sort_path(B, P, k_lo) == 'one_pass' and dbc.sort_path(B, P, k_hi) == 'fill_then_rank'
    assert dbc.sort_path(1, 1 << 20, 8) == 'fill_then_rank' and dbc.sort_path(3, 3000, 48) == 'one_pass'


def test_axis_cell_is_the_float_expression():
    lo, hi = np.float32([-1., -1.]), np.float32([1., 1.])
    inv = dbc.cell_inverse(lo, hi, 64)
    assert inv.dtype == np.float32 and float(inv[0]) == 32.
    v = np.array([-2., -1., -0.97, 0., 0.999, 1., 7., np.nan, np.inf, -np.inf])
    assert dbc.axis_cell(v, lo[0], inv[0], 64).tolist() == [0, 0, 0, 32, 63, 63, 63, 0, 63, 0]
    third = dbc.cell_inverse(np.float32([0.]), np.float32([3.]), 16)            # 1 / (3 / 16) is rounded once, in float
    assert third.dtype == np.float32 and float(third[0]) == float(np.float32(1) / (np.float32(3) / np.float32(16)))
    for degenerate in ((0.25, 0.25), (np.inf, -np.inf), (-3e38, 3e38), (-1., np.inf)):
        assert float(dbc.cell_inverse(np.float32([degenerate[0]]), np.float32([degenerate[1]]), 16)[0]) == 1.


def test_extent_rounds_outwards_and_skips_non_finite_pixels():
    pix = np.array([[0.1, 0.2], [np.nan, -5.], [7., np.inf], [-0.3, 0.25], [1e39, -1e39]])
    lo, hi = dbc.extent(pix[:4])
    down = float(np.nextafter(np.float32(0.2), np.float32(0)))              # float32(0.2) > 0.2, float32(-0.3) < -0.3
    assert lo.dtype == np.float32 and lo.tolist() == [float(np.float32(-0.3)), down] and down < 0.2 < float(np.float32(0.2))
    assert hi.tolist() == [float(np.float32(0.1)), 0.25] and float(hi[0]) > 0.1
    lo, hi = dbc.extent(-pix[:4])
    assert hi.tolist() == [float(np.float32(0.3)), -down] and lo.tolist() == [-float(np.float32(0.1)), -0.25]
    lo, hi = dbc.extent(pix)
    assert float(hi[0]) == np.inf and float(lo[1]) == -np.inf and np.isfinite(lo[0]) and np.isfinite(hi[1])
    lo, hi = dbc.extent(pix[1:3])
    assert lo.tolist() == [np.inf, np.inf] and hi.tolist() == [-np.inf, -np.inf]


@pytest.mark.parametrize('P', dbc.P_EDGES)
def test_mixed_feeds_every_face_kernel(P):
    case = mixed(2, P, 1)
    assert case[0].shape == (2, P, 2) and case[3].shape == (2, sum(dbc.MIXED_FACES), 3, 2)
    for t in case[:4]:
        assert torch.equal(t, dbc.r32(t)) and t.dtype == F64
    for b in range(2):
        kinds, ncell = kinds_of(case, b)
        n = {k: int((kinds == k).sum()) for k in ('none', 'thread', 'wave', 'group')}
        print(P, b, n, 'largest box', int(ncell.max()), 'cells')
        if P >= 8193:
            assert n['group'] >= 4 and n['wave'] >= 20 and n['thread'] >= 100, (P, b, n)
            assert int(ncell[kinds == 'group'].min()) > dbc.WAVE_CELLS
        else:
            assert n['group'] == 0 and n['wave'] >= 20 and n['thread'] >= 100, (P, b, n)
        assert int(ncell.max()) <= 4 ** dbc.gshift(P)
    # the four full-extent faces are not the first of the mesh
    big = (dbc.boxes_of(case[3])[..., 2:] - dbc.boxes_of(case[3])[..., :2]).min(dim=-1)[0] > 1.5
    assert big.sum(dim=1).tolist() == [4, 4] and not bool(big[:, :4].all())


def test_cluster_hands_a_small_box_to_a_wavefront():
    case = dbc.mixed(2, 3000, 2, cluster=True)
    small_wave = 0
    for b in range(2):
        kinds, ncell = kinds_of(case, b)
        small_wave += int(((kinds == 'wave') & (ncell <= dbc.SMALL_CELLS)).sum())
    assert small_wave >= 1
    face_idx = forward(case, 64)[0]
    sizes = (dbc.boxes_of(case[3])[..., 2:] - dbc.boxes_of(case[3])[..., :2]).max(dim=-1)[0]
    hit_small = torch.zeros(2, dtype=torch.bool)
    for b in range(2):
        faces = face_idx[b][face_idx[b] >= 0]
        hit_small[b] = bool((sizes[b][faces] < 0.05).any())
    assert bool(hit_small.all())                             # the crowded cell's pixels lie inside small faces


def test_outlier_flattens_one_axis():
    case = dbc.mixed(2, 3000, 2, outlier=True)
    lo, hi = dbc.extent(case[0][0])
    assert float(hi[0]) == 1e6 and float(hi[1]) <= 1.
    inv = dbc.cell_inverse(lo, hi, 32)
    cells = dbc.axis_cell(case[0][0][:, 0].numpy(), lo[0], inv[0], 32)
    assert sorted(set(cells.tolist())) == [0, 31]
    kinds, _ = kinds_of(case, 0)
    assert int((kinds == 'wave').sum()) >= 20
    assert int(dbc.hit_counts(forward(case, 64)[0])[0].max()) > 1


def test_identical_pixels_make_one_crowded_cell():
    case = dbc.degenerate('identical')
    total = 0
    for b in range(2):
        kinds, ncell = kinds_of(case, b)
        alive = kinds != 'none'
        assert bool((kinds[alive] == 'wave').all()) and bool((ncell[alive] == 1).all())
        total += int(alive.sum())
    assert total >= 1
    assert int(dbc.hit_counts(forward(case, 64)[0]).max()) >= 1


def test_line_has_one_flat_axis():
    case = dbc.degenerate('line')
    lo, hi = dbc.extent(case[0][0])
    assert float(lo[0]) == float(hi[0]) == 0.25 and float(hi[1]) - float(lo[1]) > 1.9
    assert float(dbc.cell_inverse(lo, hi, 16)[0]) == 1.
    kinds, _ = kinds_of(case, 0)
    assert int((kinds != 'none').sum()) >= 4 and int(dbc.hit_counts(forward(case, 64)[0]).max()) > 1


def test_hit_counts_of_the_overflow_scene():
    """mixed(2, 8193): pixels with more than 1 and more than 4 hits (knum = 1 and 4 redo them), pixels with none, and a pixel
    whose hits come from a workgroup face, a wavefront face and a thread face together."""
    case = mixed(2, 8193, 1)
    face_idx = forward(case, 64)[0]
    hits = dbc.hit_counts(face_idx)
    print('pixels with > 4 hits', int((hits > 4).sum()), 'with > 1', int((hits > 1).sum()), 'most', int(hits.max()))
    assert int(hits.max()) < 64
    assert int((hits > 4).sum()) > 1000 and int((hits > 1).sum()) > 5000 and int((hits == 0).sum()) > 0
    together = 0
    for b in range(2):
        kinds, _ = kinds_of(case, b)
        code = torch.tensor([{'none': 0, 'thread': 1, 'wave': 2, 'group': 4}[k] for k in kinds.tolist()] + [0])
        seen = code[face_idx[b]]                                            # (-1 reads the appended 0)
        assert not bool(((seen == 0) & (face_idx[b] >= 0)).any())           # a face that is hit is never rejected
        together += int(((seen == 1).any(-1) & (seen == 2).any(-1) & (seen == 4).any(-1)).sum())
    assert together > 0


def test_non_finite_pixels_hit_nothing():
    case = dbc.degenerate('no_finite')
    assert not bool(torch.isfinite(case[0]).all(dim=-1).any())
    assert bool(torch.isfinite(case[0]).any()) and bool(torch.isnan(case[0]).any()) and bool(torch.isinf(case[0]).any())
    for dtype in (F32, F64):
        assert int(dbc.hit_counts(forward(case, 16, dtype)[0]).sum()) == 0
    kinds, _ = kinds_of(case, 0)
    assert bool((kinds == 'none').all())
    case = dbc.degenerate('one_finite')
    assert int(torch.isfinite(case[0]).all(dim=-1).sum()) == 1
    for dtype in (F32, F64):
        hits = dbc.hit_counts(forward(case, 16, dtype)[0])
        assert int((hits > 0).sum()) == 1 and int(hits[1, 500 // 3]) > 0


def test_wide_extent_stays_finite_in_float():
    case = dbc.degenerate('wide_f32')
    lo, hi = dbc.extent(case[0][0])
    assert np.isfinite(hi - lo).all() and float((hi - lo).min()) > 1.9e36
    inv = dbc.cell_inverse(lo, hi, 32)
    assert float(inv.max()) < 1e-34 and float(inv.min()) > float(np.finfo(np.float32).tiny)      # a normal float
    kinds, _ = kinds_of(case, 0)
    assert int((kinds == 'wave').sum()) >= 20 and int((kinds == 'thread').sum()) >= 100
    forward(case, 16, F32)                                                  # (products overflow: any result, but a result)


def test_coordinates_beyond_float_are_hit_in_double():
    case = dbc.degenerate('beyond_f32')
    pix, ranges, z, img, _ = case
    far = pix[..., 0] > 1e38
    assert far.sum(dim=1).tolist() == [dbc.BEYOND_PIXELS] * 2
    assert not bool(torch.isfinite(pix[far].to(F32)).any())                 # no float holds them
    face_idx = forward(case, 64, F64)[0]
    assert bool((face_idx[far][:, 0] == dbc.BEYOND_FACE).all()) and bool((face_idx[far][:, 1:] == -1).all())
    assert int((dbc.hit_counts(face_idx)[~far] > 0).sum()) > 1000           # and the ordinary scene is rendered around them
    lo, hi = dbc.extent(pix[0])
    assert float(hi[0]) == np.inf and float(lo[1]) == -np.inf
    kinds, _ = kinds_of(case, 0)
    assert kinds[dbc.BEYOND_FACE] != 'none'


def test_given_boxes_cut_hits():
    pix, ranges, z, img, bb, _ = dbc.boxes_given()
    own = dbc.boxes_of(img)
    assert bool(torch.isnan(bb[:, 0::5]).any(dim=-1).all()) and all(bool(torch.isnan(bb[:, 0::5, k]).any()) for k in range(4))
    assert bool((bb[:, 1::5, 0] > bb[:, 1::5, 2]).all())
    assert bool((bb[:, 2::5, 2:] < own[:, 2::5, 2:]).all()) and bool((bb[:, 2::5, 2:] > own[:, 2::5, :2]).all())
    assert bool((bb[:, 3, 0] == bb[:, 3, 2]).all())
    assert torch.equal(bb[:, 4::5], own[:, 4::5])
    for dtype in (F32, F64):
        with_own = int(dbc.hit_counts(forward((pix, ranges, z, img), 64, dtype)[0]).sum())
        with_given = int(dbc.hit_counts(forward((pix, ranges, z, img), 64, dtype, bb)[0]).sum())
        print(dtype, 'hits with the faces\' boxes', with_own, 'with the given boxes', with_given)
        assert 0 < with_given < with_own
    kinds, _ = dbc.handover(pix[0], bb[0], pix.shape[1])
    assert bool((kinds[0::5] == 'none').all()) and bool((kinds[1::5] == 'none').all()) and kinds[3] == 'none'
    assert int((kinds[2::5] != 'none').sum()) > 50


def test_clean_scene_is_clean():
    pix, ranges, z, img, _ = dbc.clean()
    assert img.shape == (2, 300, 3, 2) and pix.shape == (2, 700, 2)
    assert float(dbc.smallest_altitude(img).min()) >= 0.05
    assert torch.unique(img.reshape(-1, 6), dim=0).shape[0] == 600
    assert bool((ranges == torch.tensor([-10., 0.], dtype=F64)).all())
    hits = dbc.hit_counts(forward((pix, ranges, z, img), 300)[0])
    assert BACKWARD_K > int(hits.max()) > 10 and float(hits.float().mean()) > 4       # K = 48 keeps every hit


def backward_triple(case, D, K, seed=0):
    """-> (ref64, ref32, E32) of (grad_face_vertices_image, grad_face_features) with the float oracle's forward"""
    pix, ranges, z, img = case[:4]
    feat = dbc.features(img.shape[0], img.shape[1], D, seed)
    r = oracle.deftet_sparse_render(pix.float(), ranges.float(), z.float(), img.float(), feat.float(), K, omp=True)
    grad = dbc.upstream(r['features'].shape, seed)
    ref32 = oracle.deftet_sparse_render_backward(grad.float(), r['face_idx'], r['weights'], img.float(), feat.float(), 1e-8)
    ref64 = oracle.deftet_sparse_render_backward(grad, r['face_idx'], r['weights'].double(), img, feat, 1e-8)
    return ref64, ref32, [float((a.double() - b).abs().max()) for a, b in zip(ref32, ref64)]


@pytest.mark.parametrize('D', BACKWARD_D)
def test_clean_scene_is_conditioned(D):
    """E32 <= CONDITIONED_E32 * max |ref64| for both gradients: the floor 4 E32 of the GPU tests' bound then stays below
    4e-5 of the largest entry."""
    ref64, _, e32 = backward_triple(dbc.clean(), D, BACKWARD_K, seed=D)
    for what, ref, e in zip(('grad_face_vertices_image', 'grad_face_features'), ref64, e32):
        scale = float(ref.abs().max())
        print(f'D={D} {what}: E32 = {e:.3e} = {e / scale:.3e} of the largest entry {scale:.3e}')
        assert scale > 0 and e <= CONDITIONED_E32 * scale, (D, what, e, scale)
