"""Every case of tests/weighted_sum_dibr_cases.py has the property it aims at (oracle only: runs without a GPU).

The GPU comparison (tests/test_weighted_sum_dibr_oracle_gpu.py) passes on a case whether or not the case still reaches its edge; a
change to a scene helper that moves the sphere out of the partial tiles, or the big faces off the hot-face table, must fail HERE."""
import numpy as np
import pytest
import torch

import oracle
import weighted_sum_dibr_cases as C

DTYPES = [torch.float, torch.double]


def _reference(case):
    fz, fimg, feat, nz, H, W, knum, boxlen = case
    return oracle.dibr_rasterization(H, W, fz, fimg, feat, nz, boxlen=boxlen, knum=knum, omp=True)


def _check_partial_tiles(case):
    H, W = case[4], case[5]
    ref = _reference(case)
    edge = C.partial_raster_tile_mask(H, W)
    assert bool(edge.any()), 'the image has no partial raster tile'
    covered = ref['face_idx'] >= 0                                  # (B, H, W)
    soft_hit = (ref['close_face_idx'] >= 0).any(dim=-1)             # (B, H, W): the pixel is in some K-buffer
    assert int((covered & edge).sum()) >= 1, 'no covered pixel in a partial raster tile'
    assert int((soft_hit & edge).sum()) >= 1, 'no soft hit in a partial raster tile'
    return covered


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('D', C.RAGGED_D)
def test_ragged_reaches_partial_tiles(D, dtype):
    case = C.ragged(D, dtype)
    assert case[2].shape == (3, 720, 3, D) and case[2].dtype == dtype and (case[4], case[5]) == (35, 31)
    _check_partial_tiles(case)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('D', C.TINY_D)
def test_tiny_is_one_partial_tile_of_one_view(D, dtype):
    case = C.tiny(D, dtype)
    H, W = case[4], case[5]
    assert case[1].shape[0] == 1 and case[2].shape[-1] == D
    assert H < C.R_TILE and W < C.R_TILE and bool(C.partial_raster_tile_mask(H, W).all())
    _check_partial_tiles(case)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B', C.VIEWS_B)
def test_views_every_view_is_covered(B, dtype):
    case = C.views(B, dtype)
    assert case[1].shape[0] == B and case[2].shape[-1] == 3
    covered = _check_partial_tiles(case)
    per_view = covered.reshape(B, -1).sum(dim=1)
    assert bool((per_view > 0).all()), f'views without a covered pixel: {per_view.tolist()}'
    assert B >= 8 and {b % 8 for b in C.VIEWS_B} == {0, 1}          # 8: no remainder; 9 and 17: one view beyond whole groups of 8


def soft_big_faces(fimg, H, W, boxlen, multiplier=1000.):
    """(B, F) bool: the faces the binning launch enters into the hot-face table.  The rule, csrc/tile_lists.h (bin kernel, soft pass):

        bx0 = xmin - in.margin;  by0 = ymin - in.margin;  bx1 = xmax + in.margin;  by1 = ymax + in.margin;
        if (pixel_range<T>(bx0, by0, bx1, by1, in.H, in.W, in.multiplier, &pr_s)) {
          sx0 = pr_s.c_lo / S_TILE;  sx1 = pr_s.c_hi / S_TILE;  sy0 = pr_s.r_lo / S_TILE;  sy1 = pr_s.r_hi / S_TILE;
          big_s = pr_s.everywhere || sx1 - sx0 >= 8 || sy1 - sy0 >= 8;

    with x / y the vertices times the multiplier, margin = boxlen * multiplier, and pixel_range (float32 whatever T is):

        sx = (float)W / multiplier, sy = (float)H / multiplier;  dx = 1e-3f + 1e-6f * W, dy = 1e-3f + 1e-6f * H;
        cl = ceilf((fxmin * sx + (float)(W - 1)) * 0.5f - dx), ch = ceilf((fxmax * sx + (float)(W - 1)) * 0.5f + dx) - 1.0f;
        rl = ceilf(((float)(H - 1) - fymax * sy) * 0.5f - dy), rh = ceilf(((float)(H - 1) - fymin * sy) * 0.5f + dy) - 1.0f;
        if (ch < 0 || cl > W - 1 || rh < 0 || rl > H - 1) return false;        // the box misses the image
        c_lo = max(cl, 0), c_hi = min(ch, W - 1), r_lo = max(rl, 0), r_hi = min(rh, H - 1);

    -- "more than 8 x 8 soft tiles": a span of 9 or more tile columns, or tile rows.  (No NaN here: nothing is `everywhere`.)"""
    f32 = np.float32
    scaled = fimg * multiplier                                      # in the case's dtype, as the kernel forms it
    margin = torch.tensor(boxlen * multiplier, dtype=fimg.dtype)
    lo = (scaled.min(dim=-2)[0] - margin).numpy().astype(f32)       # (B, F, 2)
    hi = (scaled.max(dim=-2)[0] + margin).numpy().astype(f32)
    sx, sy = f32(W) / f32(multiplier), f32(H) / f32(multiplier)
    dx, dy = f32(1e-3) + f32(1e-6) * f32(W), f32(1e-3) + f32(1e-6) * f32(H)
    half = f32(0.5)
    cl = np.ceil((lo[..., 0] * sx + f32(W - 1)) * half - dx)
    ch = np.ceil((hi[..., 0] * sx + f32(W - 1)) * half + dx) - f32(1)
    rl = np.ceil((f32(H - 1) - hi[..., 1] * sy) * half - dy)
    rh = np.ceil((f32(H - 1) - lo[..., 1] * sy) * half + dy) - f32(1)
    on_image = ~((ch < 0) | (cl > W - 1) | (rh < 0) | (rl > H - 1))
    c_lo, c_hi = np.maximum(cl, 0).astype(np.int64), np.minimum(ch, W - 1).astype(np.int64)
    r_lo, r_hi = np.maximum(rl, 0).astype(np.int64), np.minimum(rh, H - 1).astype(np.int64)
    on_image &= (c_lo <= c_hi) & (r_lo <= r_hi)
    big = (c_hi // C.S_TILE - c_lo // C.S_TILE >= 8) | (r_hi // C.S_TILE - r_lo // C.S_TILE >= 8)
    return torch.from_numpy(on_image & big)


BIG_HASH_MAX = 2048      # csrc/tile_lists.h: "at most BIG_HASH_MAX keys: beyond that the table is not used"


def _hot_stats(case):
    """-> (faces on the table, soft hits whose face is one of them, pixels with a soft hit)"""
    fz, fimg, feat, nz, H, W, knum, boxlen = case
    hot = soft_big_faces(fimg, H, W, boxlen)
    assert (W + C.S_TILE - 1) // C.S_TILE >= 9, 'fewer than 9 soft tile columns: no face can span more than 8'
    idx = _reference(case)['close_face_idx']                          # (1, H, W, knum), -1: empty
    on_hot = hot[0][idx.clamp(min=0)] & (idx >= 0)
    return int(hot.sum()), int(on_hot.sum()), int((idx >= 0).any(dim=-1).sum())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n_big', C.HOT_N_BIG)
def test_hot_recipe_puts_faces_on_the_table(n_big, dtype):
    """The recipe of test_fused_backward_with_image_sized_faces_equals_the_composition.  A random face of size 2.2 spans 9 soft tile
    columns or rows in ~6 % of the draws: 2 of the 40, and 158 of the 2 500 -- BOTH counts are within BIG_HASH_MAX, the table is
    in use either way (2 500 such faces do not take it over its limit, whatever that test's docstring said; and they cover every
    pixel, so no soft hit is left: what 2 500 adds is the rasterizer's fold over 158 records of zeros).  The case over the limit is
    hot_slivers, below."""
    case = C.hot(n_big, dtype)
    assert (case[4], case[5], case[6]) == (288, 288, 5) and case[2].shape == (1, n_big + 300, 3, 2)
    n_hot, hits_on_hot, soft_px = _hot_stats(case)
    assert 1 <= n_hot <= BIG_HASH_MAX, n_hot
    if n_big == 40:
        assert hits_on_hot >= 1000, hits_on_hot      # the soft backward really adds to the per-XCD copies


@pytest.mark.parametrize('dtype', DTYPES)
def test_hot_slivers_overflow_the_table(dtype):
    case = C.hot_slivers(dtype)
    assert (case[4], case[5], case[6]) == (288, 288, 5) and case[2].shape == (1, 2800, 3, 2)
    n_hot, hits_on_hot, soft_px = _hot_stats(case)
    assert n_hot > BIG_HASH_MAX, n_hot
    assert hits_on_hot >= 100000 and soft_px >= 288 * 288 // 2, (hits_on_hot, soft_px)
    covered = _reference(case)['face_idx'] >= 0
    assert int(covered.sum()) >= 5000                # ... and the rasterizer's backward has tiles to walk
