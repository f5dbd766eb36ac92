"""Generates tests/golden/voxelgrid_edges.npz FROM THE REFERENCE ITSELF (kaolin.ops.conversions.trianglemeshes_to_voxelgrids).

Run in the build container (where the reference tree is mounted):
    python tests/golden/make_golden_voxelgrid_edges.py
The reference's files are loaded by path on top of _refload's stub ``kaolin`` package; the operator is pure PyTorch and runs on
the CPU.  The inputs are tests/voxelgrid_boundary_cases.py's ``edge_case_inputs`` (NaN vertices and a mesh of coinciding
vertices), in float32; the reference is run on them as they are and cast to float64.  Per case: ``<case>_vertices``, ``_faces``,
``_res``, ``_origin`` / ``_scale`` where the case gives them, and ``<case>_packed_f32`` / ``_packed_f64`` (np.packbits of the dense
result) with ``<case>_count_f32`` / ``_count_f64`` (its sum)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _refload  # noqa: E402
import voxelgrid_boundary_cases as cases  # noqa: E402


def main():
    conv = _refload.load_reference()['conv_trianglemesh'].trianglemeshes_to_voxelgrids
    out = {}
    for name, (v, f, res, org, sc) in cases.edge_case_inputs().items():
        assert v.dtype == torch.float32
        out[name + '_vertices'], out[name + '_faces'], out[name + '_res'] = v.numpy(), f.numpy().astype(np.int16), res
        if org is not None:
            out[name + '_origin'], out[name + '_scale'] = org.numpy(), sc.numpy()
        for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
            dense = conv(v.to(dt), f, res, None if org is None else org.to(dt), None if sc is None else sc.to(dt), False)
            assert dense.dtype == dt and dense.shape == (v.shape[0], res, res, res)
            assert bool(((dense == 0) | (dense == 1)).all())
            out[f'{name}_packed_{tag}'] = np.packbits(dense.numpy().astype(np.uint8).reshape(-1))
            out[f'{name}_count_{tag}'] = int(dense.sum())
    path = os.path.join(HERE, cases.EDGES_NPZ)
    np.savez_compressed(path, **out)
    print('wrote', cases.EDGES_NPZ, len(out), 'arrays', os.path.getsize(path), 'bytes')
    for k in sorted(out):
        if '_count_' in k:
            print(k, int(out[k]))


if __name__ == '__main__':
    main()
