"""Makes tests/golden/gs_to_voxelgrid.npz from the reference's own recorded result and test expectations.

    python tests/golden/make_golden_gs_to_voxelgrid.py /path/to/kaolin

Reads <kaolin>/tests/samples/ops/conversions/gs_to_voxelgrid_large.pt (level 7 of the 8 Gaussians of
tests/python/kaolin/ops/conversions/test_gaussians.py: 197 824 voxels int16, merged opacities float32) and records the level-0 and
level-1 expectations that test file spells out.  The full record does not fit the size of a committed fixture, so ALL voxel
coordinates are kept and every OPACITY_STRIDE-th opacity (``opacity_stride`` in the file: opacities_7[i] belongs to voxel
i * opacity_stride).  Data only; the reference is read when the golden is made and never by a test."""
import math
import os
import sys

import numpy as np
import torch

OPACITY_STRIDE = 2


def inputs():
    """the 8 Gaussians of the reference's test (test_gaussians.py:24-76)"""
    xyz = np.array([[0.5, 0.5, 0.5], [0.5, 0.5, -0.5], [0.5, -0.5, 0.5], [0.5, -0.5, -0.5],
                    [-0.5, 0.5, 0.5], [-0.5, 0.5, -0.5], [-0.5, -0.5, 0.5], [-0.5, -0.5, -0.5]], np.float32)
    scales = np.tile(np.array([[0.2, 0.05, 0.05]], np.float32), (8, 1))
    t0, t1 = math.acos(1 / math.sqrt(3)) / 2, math.acos(-1 / math.sqrt(3)) / 2
    c = 1 / math.sqrt(2)
    rows = [(t0, -1), (t1, 1), (t0, 1), (t1, -1), (t1, -1), (t0, 1), (t1, 1), (t0, -1)]
    rots = torch.tensor([[math.cos(t), 0, c * math.sin(t), s * c * math.sin(t)] for t, s in rows], dtype=torch.float).numpy()
    opacities = np.array([[1.0], [0.8], [0.6], [0.4], [0.2], [0.1], [0.05], [0.01]], np.float32)
    return xyz, scales, rots, opacities


def main(reference_root):
    rec = torch.load(os.path.join(reference_root, 'tests', 'samples', 'ops', 'conversions', 'gs_to_voxelgrid_large.pt'),
                     map_location='cpu')
    voxels, opac = rec['voxels'].numpy(), rec['merged_opacities'].numpy()
    assert voxels.dtype == np.int16 and opac.dtype == np.float32 and len(voxels) == len(opac)
    xyz, scales, rots, opacities = inputs()
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'gs_to_voxelgrid.npz')
    np.savez_compressed(
        out, xyz=xyz, scales=scales, rots=rots, opacities=opacities,
        voxels_7=voxels, opacities_7=opac[::OPACITY_STRIDE], opacity_stride=np.int64(OPACITY_STRIDE),
        voxels_0=np.array([[0, 0, 0]], np.int16), opacities_0=np.array([0.0678], np.float32),
        voxels_1=np.array([[i >> 2, (i >> 1) & 1, i & 1] for i in range(8)], np.int16),
        opacities_1=np.array([0.0004, 0.0018, 0.0036, 0.0072, 0.0144, 0.0216, 0.0288, 0.0359], np.float32))
    print(out, os.path.getsize(out), 'bytes;', len(voxels), 'voxels,', len(opac[::OPACITY_STRIDE]), 'opacities')


if __name__ == '__main__':
    main(sys.argv[1])
