"""Generates tests/golden/cubic_meshes.npz FROM THE REFERENCE ITSELF (kaolin.ops.conversions.voxelgrids_to_cubic_meshes).

Run in the build container (where the reference tree is mounted):
    python tests/golden/make_golden_cubic_meshes.py
The reference file is loaded by path on top of _refload's stub ``kaolin`` package and run on the CPU.  Every input is built
here (seeded where random).  Per case the file holds the input -- ``<case>_in_bits`` (np.packbits of the flattened grid) and
``<case>_in_shape``, or ``<case>_in`` (float32) for the valued case -- and per item b the reference's outputs:
``<case>_verts_<b>`` (lattice coordinates, uint8), ``<case>_tri_<b>`` and ``<case>_quad_<b>`` (int32; is_trimesh True / False).

Cases, and what each is for (the generator asserts the stated property of the reference's answer):
  doc          (1,1,1,1) of ones: the docstring example, which pins the corner order of the three quad templates
  single_in_2  (1,2,2,2) with one voxel
  full         (1,4,3,5) of ones: only boundary faces, every face touches the zero padding
  checker      (1,4,5,6) 3D checkerboard: every pair of adjacent voxels has a face (and every occupied voxel of the boundary one
               towards the padding), every lattice point is used but the four corners whose voxel is empty, inverted and
               non-inverted faces alternate
  hollow       a 5^3 cube with its centre removed: the inner faces wind the other way
  batch        (3,2,3,2): item 0 empty; item 1 two voxels sharing a face (no internal face, 12 vertices); item 2 two voxels
               touching only at an edge (the shared edge's vertices are merged: 14 vertices)
  thin_x       (1,1,6,7) and
  thin_z       (1,6,7,1), random: one voxel thick along the slowest and the fastest axis
  wave_tail    (1,3,7,70) random p = 0.5: Z + 1 = 71 crosses a 64-lane wavefront inside a row, the lattice (4 * 8 * 71 = 2272
               points) spans several 256-point workgroups with a partial last one
  rand12       (2,12,12,12) random p = 0.5
  values       (1,2,2,2) of [[0.5,1.5],[2,-1]], [[0.25,0],[1,3]] (exact in half): faces follow rint(hi - lo) != 0, inverted
               when it is -1; 22 vertices, 25 quads, 50 triangles
Every non-empty item of every case has a face on each of the three axes: where an axis has none the reference's per-axis
counts misalign (it is not a definition there), so such a case must not be recorded.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload  # noqa: E402

OUT = os.path.join(HERE, 'cubic_meshes.npz')


def load_reference():
    _refload.load_reference()
    return _refload._load('kaolin.ops.conversions.voxelgrid', 'kaolin/ops/conversions/voxelgrid.py')


def binary_cases():
    g = torch.Generator().manual_seed(20260)
    cases = {}
    cases['doc'] = np.ones((1, 1, 1, 1), dtype=bool)
    single = np.zeros((1, 2, 2, 2), dtype=bool)
    single[0, 1, 0, 1] = True
    cases['single_in_2'] = single
    cases['full'] = np.ones((1, 4, 3, 5), dtype=bool)
    x, y, z = np.meshgrid(np.arange(4), np.arange(5), np.arange(6), indexing='ij')
    cases['checker'] = (((x + y + z) % 2) == 0)[None]
    hollow = np.ones((1, 5, 5, 5), dtype=bool)
    hollow[0, 2, 2, 2] = False
    cases['hollow'] = hollow
    batch = np.zeros((3, 2, 3, 2), dtype=bool)
    batch[1, 0, 1, 0] = batch[1, 1, 1, 0] = True
    batch[2, 0, 0, 1] = batch[2, 1, 1, 1] = True
    cases['batch'] = batch
    for name, shape in (('thin_x', (1, 1, 6, 7)), ('thin_z', (1, 6, 7, 1)), ('wave_tail', (1, 3, 7, 70)), ('rand12', (2, 12, 12, 12))):
        cases[name] = (torch.rand(shape, generator=g) < 0.5).numpy()
    return cases


def axis_face_counts(grid):
    """(3,) exposed faces per axis of one float item, by shifted comparisons of the zero-padded grid."""
    p = np.pad(grid.astype(np.float32), 1)
    return [int((np.rint(np.diff(p, axis=d)) != 0).sum()) for d in range(3)]


def main():
    ref = load_reference()
    out = {}
    inputs = {k: torch.from_numpy(v).float() for k, v in binary_cases().items()}
    for name, t in inputs.items():
        out[f'{name}_in_bits'] = np.packbits(t.numpy().astype(bool).reshape(-1))
        out[f'{name}_in_shape'] = np.array(t.shape, dtype=np.int64)
    values = torch.tensor([[[0.5, 1.5], [2., -1.]], [[0.25, 0.], [1., 3.]]]).unsqueeze(0)
    assert torch.equal(values.half().float(), values)
    inputs['values'] = values
    out['values_in'] = values.numpy()

    got = {}
    for name, t in inputs.items():
        verts, tris = ref.voxelgrids_to_cubic_meshes(t)
        verts_q, quads = ref.voxelgrids_to_cubic_meshes(t, is_trimesh=False)
        assert len(verts) == len(tris) == len(quads) == t.shape[0]
        for b in range(t.shape[0]):
            v, tri, quad = verts[b], tris[b], quads[b]
            assert torch.equal(v, verts_q[b])
            assert v.dtype == torch.float32 and tri.dtype == torch.int64 and quad.dtype == torch.int64
            assert v.shape[1:] == (3,) and tri.shape == (2 * quad.shape[0], 3) and quad.shape[1:] == (4,)
            counts = axis_face_counts(t[b].numpy())
            assert sum(counts) == quad.shape[0], (name, b, counts)
            if quad.shape[0] > 0:
                assert min(counts) > 0, f'{name}[{b}]: an axis without a face -- the reference misaligns, not a golden'
                assert v.min() >= 0 and v.max() <= 255 and torch.equal(v, v.round())
            out[f'{name}_verts_{b}'] = v.numpy().astype(np.uint8)
            out[f'{name}_tri_{b}'] = tri.numpy().astype(np.int32)
            out[f'{name}_quad_{b}'] = quad.numpy().astype(np.int32)
            got[name, b] = (v, tri, quad)

    # the stated properties
    v, tri, quad = got['doc', 0]
    assert tri.tolist() == [[0, 1, 2], [5, 4, 7], [0, 4, 1], [6, 2, 7], [0, 2, 4], [3, 1, 7], [3, 2, 1], [6, 7, 4], [5, 1, 4], [3, 7, 2],
                            [6, 4, 2], [5, 7, 1]]
    assert quad.tolist() == [[0, 2, 3, 1], [5, 7, 6, 4], [0, 1, 5, 4], [6, 7, 3, 2], [0, 4, 6, 2], [3, 7, 5, 1]]
    assert got['single_in_2', 0][0].shape[0] == 8 and got['single_in_2', 0][2].shape[0] == 6
    assert got['full', 0][2].shape[0] == 2 * (4 * 3 + 3 * 5 + 5 * 4)
    v, _, quad = got['checker', 0]
    c = inputs['checker'][0].bool()
    towards_padding = sum(int(c.select(d, 0).sum() + c.select(d, -1).sum()) for d in range(3))
    assert v.shape[0] == 5 * 6 * 7 - 4 and quad.shape[0] == 3 * 5 * 6 + 4 * 4 * 6 + 4 * 5 * 5 + towards_padding
    assert got['hollow', 0][2].shape[0] == 6 * 25 + 6 and got['hollow', 0][0].shape[0] == 6 ** 3 - 4 ** 3 + 8
    assert got['batch', 0][0].shape[0] == 0 and got['batch', 0][1].shape == (0, 3) and got['batch', 0][2].shape == (0, 4)
    assert got['batch', 1][0].shape[0] == 12 and got['batch', 1][2].shape[0] == 10
    assert got['batch', 2][0].shape[0] == 14 and got['batch', 2][2].shape[0] == 12
    assert got['values', 0][0].shape[0] == 22 and got['values', 0][2].shape[0] == 25 and got['values', 0][1].shape[0] == 50
    out['cases'] = np.array(sorted(inputs))

    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < 1000000, size
    print('wrote cubic_meshes.npz', len(out), 'arrays', size, 'bytes')


if __name__ == '__main__':
    main()
