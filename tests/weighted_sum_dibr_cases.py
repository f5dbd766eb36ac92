"""Case builders for the oracle comparison of the fused weighted_sum backward (test infrastructure; plain CPU torch, used by
tests/test_weighted_sum_dibr_cases_cpu.py and tests/test_weighted_sum_dibr_oracle_gpu.py).

Every builder returns (fz, fimg, feat, nz, H, W, knum, boxlen) with `feat` ONE (B, F, 3, D) tensor: a list of features comes back
from dibr_rasterization as views of one buffer, and weighted_sum of a view takes the unfused path.  The features are drawn per view
from a seeded generator, so any D is possible (the scene helpers only make D = 3) and a wrong batch stride shows.

What each family is for (tests/test_weighted_sum_dibr_cases_cpu.py asserts that it still is):
  ragged  35 x 31, 3 views: partial 16 x 16 raster tiles and partial 32 x 32 soft tiles, every D the launchers switch on
          (1 - 4: staged rows with DT = D; 5, 7: the generic branch, DT = 0)
  tiny    7 x 5, one view: ONE partial raster tile, a batch of 1
  views   8, 9, 17 views: the list kernel deals its entries to the XCDs by b % 8 "with 8 or more views"; 9 and 17 leave a remainder
  hot     image-sized faces: the soft backward's hot-face table (tile_lists.h, BIG_HASH_MAX) in use (n_big = 40) or over its
          limit and ignored (2 500)"""
import torch

RAGGED_D = (1, 2, 3, 4, 5, 7)
TINY_D = (3, 5)
VIEWS_B = (8, 9, 17)
HOT_N_BIG = (40, 2500)

R_TILE = 16          # csrc/tile_lists.h: rasterizer tile
S_TILE = 32          # ... soft-mask tile


def _features(B, F, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((B, F, 3, D), generator=g, dtype=torch.float64).to(dtype)


def _sphere(level, views, D, dtype, seed):
    from kaolin_amd.utils import testing as T
    fz, fimg, _, nz = T.sphere_scene(level=level, num_views=views, dtype=dtype)
    return fz, fimg, _features(fimg.shape[0], fimg.shape[1], D, dtype, seed), nz


def ragged(D, dtype):
    """The ragged scene of test_dibr_rasterization_vs_oracle (720 faces, 3 views, 35 x 31, boxlen 0.2) with D features."""
    fz, fimg, feat, nz = _sphere(6, 3, D, dtype, 100 + D)
    return fz, fimg, feat, nz, 35, 31, 30, 0.2


def tiny(D, dtype):
    fz, fimg, feat, nz = _sphere(4, 1, D, dtype, 200 + D)
    return fz, fimg, feat, nz, 7, 5, 30, 0.2


def views(B, dtype):
    fz, fimg, feat, nz = _sphere(4, B, 3, dtype, 300 + B)
    return fz, fimg, feat, nz, 35, 31, 5, 0.1


def hot(n_big, dtype):
    """The recipe of test_dibr_gpu.py::test_fused_backward_with_image_sized_faces_equals_the_composition: 300 small faces and `n_big`
    of size 2.2 on 288 x 288, 30 % back faces, D = 2, knum = 5.  Drawn in float32 and converted, so both dtypes see the same scene."""
    g = torch.Generator().manual_seed(n_big)
    H = W = 288
    n_small = 300
    F = n_big + n_small
    size = torch.cat([torch.full((n_big,), 2.2), torch.full((n_small,), 0.06)])[torch.randperm(F, generator=g)]
    centre = (torch.rand(1, F, 1, 2, generator=g) - 0.5) * 1.6
    img = centre + (torch.rand(1, F, 3, 2, generator=g) - 0.5) * size.view(1, F, 1, 1)
    z = -(torch.rand(1, F, 3, generator=g) * 2 + 0.5)
    feat = torch.rand(1, F, 3, 2, generator=g)
    nz = torch.rand(1, F, generator=g) - 0.3          # 30 % back faces
    return z.to(dtype), img.to(dtype), feat.to(dtype), nz.to(dtype), H, W, 5, 0.02


def hot_slivers(dtype, n_big=2500):
    """`n_big` slivers across the whole image -- one vertex in the left margin, one in the right, the third within a pixel of the line
    between them -- plus the 300 small faces of :func:`hot`; 95 % back faces.  EVERY sliver's enlarged box spans the 9 soft tile
    columns of 288 pixels, so the table is over BIG_HASH_MAX = 2 048 with 2 500 of them (the random faces of size 2.2 of
    :func:`hot` span 9 columns or rows in ~6 % of the draws: 158 of 2 500).  Thin and mostly back facing, they leave most pixels
    uncovered, each within the enlarged boxes of dozens of slivers: the soft backward sends its terms to faces that WOULD be on
    the table."""
    g = torch.Generator().manual_seed(7000 + n_big)
    H = W = 288
    n_small = 300
    F = n_big + n_small
    r = lambda *s: torch.rand(*s, generator=g)    # noqa: E731
    y = (r(n_big) - 0.5) * 1.8
    tilt = (r(n_big) - 0.5) * 0.2
    x2 = r(n_big) - 0.5
    big = torch.stack([torch.stack([-(0.85 + 0.2 * r(n_big)), y - tilt], -1),
                       torch.stack([0.85 + 0.2 * r(n_big), y + tilt], -1),
                       torch.stack([x2, y + tilt * x2 / 0.95 + (r(n_big) - 0.5) * 0.02], -1)], 1)       # (n_big, 3, 2)
    small = (r(n_small, 1, 2) - 0.5) * 1.6 + (r(n_small, 3, 2) - 0.5) * 0.06
    order = torch.randperm(F, generator=g)
    img = torch.cat([big, small])[order].unsqueeze(0).contiguous()
    z = -(r(1, F, 3) * 2 + 0.5)
    feat = r(1, F, 3, 2)
    nz = torch.cat([r(n_big) - 0.95, r(n_small) - 0.3])[order].unsqueeze(0).contiguous()
    return z.to(dtype), img.to(dtype), feat.to(dtype), nz.to(dtype), H, W, 5, 0.02


def loss_weights(B, H, W, D, dtype, seed):
    """G1 (B, H, W, D) and G2 (B, H, W), uniform in [0, 1)."""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((B, H, W, D), generator=g, dtype=torch.float64).to(dtype),
            torch.rand((B, H, W), generator=g, dtype=torch.float64).to(dtype))


def partial_raster_tile_mask(H, W):
    """(H, W) bool: the pixels of the last column / row of 16 x 16 raster tiles where that column / row is cut by the image's edge."""
    m = torch.zeros((H, W), dtype=torch.bool)
    if W % R_TILE:
        m[:, (W // R_TILE) * R_TILE:] = True
    if H % R_TILE:
        m[(H // R_TILE) * R_TILE:, :] = True
    return m
