"""Generates tests/golden/pointcloud_voxelgrids.npz FROM THE REFERENCE ITSELF (kaolin.ops.conversions.pointclouds_to_voxelgrids).

Run in the build container (where the reference tree is mounted):
    python tests/golden/make_golden_pointcloud.py
The reference file is loaded by path on top of _refload's stub ``kaolin`` package and run on the CPU, in float32, float64 and half.
Every input is built here (seeded where random).  A case is ``<name>_<dtype>`` (dtype f32 / f64 / f16); the file holds
``<case>_in`` (B, P, 3), ``<case>_R``, optionally ``<case>_origin`` (B, 3) and ``<case>_scale`` (B) -- absent: the defaults --,
``<case>_bits`` (np.packbits of the flattened dense (B, R, R, R) result) and ``<case>_idx`` (4, nnz) int16, the indices of the
reference's sparse result after coalesce().  ``cases`` lists the case names.

The float64 inputs are the float32 inputs converted (and the half inputs the float32 inputs rounded) unless stated: the SAME
points then land in different voxels because every operation is rounded in the dtype -- the generator asserts that the seeded
2 x 50 case differs between the dtypes.

Cases:
  ref_default, ref_origin, ref_scale   the three recorded cases of the reference's tests (R = 3; origin = 1; scale = 4)
  r<R>_b<B>_p<P>   R in {1, 2, 3, 32}, B in {1, 3}, P in {1, 255, 257}: seeded uniform points in [-1, 1], default origin and scale
                   (P = 1: scale 0, 0 / 0 = NaN, empty grid; R = 1: every finite point lands in the one voxel)
  outside          points in [-1, 2]^3 with origin 0, scale 1, R = 8: most lie outside the box
  coincide         B = 2, the points of item 0 all coincide (scale 0 -> empty grid), item 1 random
  ties_r3, ties_r5 origin 0, scale 1: coordinates (k + 1/2) / (R - 1), exact in every dtype, so x (R - 1) = k + 1/2 exactly
  ties_r7          per dtype the coordinate nearest to (k + 1/2) / 6 and its two neighbours in that dtype: whether the product is
                   a tie depends on the dtype's rounding (the generator asserts that each dtype meets at least one exact tie)
  seeded_2x50      2 x 50 seeded uniform points in [0, 1), R = 8
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload  # noqa: E402

OUT = os.path.join(HERE, 'pointcloud_voxelgrids.npz')
DTYPES = {'f32': torch.float32, 'f64': torch.float64, 'f16': torch.float16}


def typed(x32, dtype):
    return x32.to(dtype)


def build_cases():
    """{name: {dtype tag: (points, R, origin or None, scale or None)}}"""
    g = torch.Generator().manual_seed(20261019)
    cases = {}

    def same(name, pts32, R, origin=None, scale=None):
        cases[name] = {tag: (typed(pts32, dt), R, None if origin is None else typed(origin, dt),
                             None if scale is None else typed(scale, dt)) for tag, dt in DTYPES.items()}

    ref = torch.tensor([[[0, 0, 0], [1, 1, 1], [2, 2, 2], [0, 2, 2]], [[0, 1, 2], [2, 0, 0], [1, 2, 0], [1, 1, 2]]], dtype=torch.float32)
    same('ref_default', ref, 3)
    same('ref_origin', ref, 3, origin=torch.ones((2, 3)))
    same('ref_scale', ref, 3, scale=torch.ones(2) * 4)
    for R in (1, 2, 3, 32):
        for B in (1, 3):
            for P in (1, 255, 257):
                same(f'r{R}_b{B}_p{P}', torch.rand((B, P, 3), generator=g) * 2 - 1, R)
    same('outside', torch.rand((2, 200, 3), generator=g) * 3 - 1, 8, origin=torch.zeros((2, 3)), scale=torch.ones(2))
    co = torch.rand((2, 40, 3), generator=g)
    co[0] = co[0, 0]
    same('coincide', co, 8)
    for R in (3, 5):
        k = torch.arange(R - 1, dtype=torch.float32)
        x = (k + 0.5) / (R - 1)
        pts = torch.stack(torch.meshgrid(x, x, x, indexing='ij'), dim=-1).reshape(1, -1, 3)
        same(f'ties_r{R}', pts, R, origin=torch.zeros((1, 3)), scale=torch.ones(1))
    cases['ties_r7'] = {}
    for tag, dt in DTYPES.items():
        centre = ((torch.arange(6, dtype=torch.float64) + 0.5) / 6).to(dt)
        lo = torch.nextafter(centre, torch.zeros_like(centre)) if dt != torch.float16 else \
            (centre.view(torch.int16) - 1).view(torch.float16)
        hi = torch.nextafter(centre, torch.ones_like(centre)) if dt != torch.float16 else \
            (centre.view(torch.int16) + 1).view(torch.float16)
        x = torch.cat([lo, centre, hi])                                                         # 18 coordinates
        prod = x * (torch.ones(1, dtype=dt) * 6)
        assert ((prod - torch.floor(prod)) == 0.5).any(), f'{tag}: no exact tie at R = 7'
        pts = torch.stack([x, x.flip(0), x.roll(5)], dim=-1).reshape(1, -1, 3)
        cases['ties_r7'][tag] = (pts, 7, torch.zeros((1, 3), dtype=dt), torch.ones(1, dtype=dt))
    same('seeded_2x50', torch.rand((2, 50, 3), generator=g), 8)
    return cases


def main():
    ref = _refload.load_reference()['conv_pointcloud']
    out, names, counts = {}, [], {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for name, per_dtype in build_cases().items():
            for tag, (pts, R, origin, scale) in per_dtype.items():
                case = f'{name}_{tag}'
                dense = ref.pointclouds_to_voxelgrids(pts, R, origin=origin, scale=scale)
                sparse = ref.pointclouds_to_voxelgrids(pts, R, origin=origin, scale=scale, return_sparse=True).coalesce()
                assert dense.dtype == pts.dtype and dense.shape == (pts.shape[0], R, R, R)
                assert ((dense == 0) | (dense == 1)).all()
                idx = sparse.indices()
                assert torch.equal(sparse.to_dense().to(pts.dtype), dense) and (sparse.values() == 1).all()
                assert idx.dtype == torch.int64 and idx.shape[0] == 4 and idx.shape[1] == int(dense.sum())
                out[f'{case}_in'] = pts.numpy()
                out[f'{case}_R'] = np.array(R, dtype=np.int64)
                if origin is not None:
                    out[f'{case}_origin'] = origin.numpy()
                if scale is not None:
                    out[f'{case}_scale'] = scale.numpy()
                out[f'{case}_bits'] = np.packbits(dense.numpy().astype(bool).reshape(-1))
                out[f'{case}_idx'] = idx.numpy().astype(np.int16)
                names.append(case)
                counts[case] = int(dense.sum())

    # the stated properties
    assert counts['ref_default_f32'] == 8 and counts['ref_origin_f32'] == 3 and counts['ref_scale_f32'] == 6
    for tag in DTYPES:
        assert counts[f'coincide_{tag}'] > 0 and not np.unpackbits(out[f'coincide_{tag}_bits'])[:512].any()
        assert counts[f'r32_b1_p1_{tag}'] == 0 and counts[f'r1_b3_p257_{tag}'] == 3
        assert 0 < counts[f'outside_{tag}'] < 200
    seeded = [counts[f'seeded_2x50_{tag}'] for tag in DTYPES]
    assert len(set(seeded)) > 1, seeded
    print('seeded 2 x 50 at R = 8 fills', dict(zip(DTYPES, seeded)), 'voxels')
    out['cases'] = np.array(names)

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 1000000, size
    print('wrote pointcloud_voxelgrids.npz', len(names), 'cases', size, 'bytes')


if __name__ == '__main__':
    main()
