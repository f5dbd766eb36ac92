"""Generates tests/golden/voxelgrid_ops.npz FROM THE REFERENCE ITSELF (kaolin.ops.voxelgrid, kaolin.metrics.voxelgrid).

Run in the build container (where the reference tree is mounted and SciPy is installed: the reference's ``fill`` is SciPy's
``binary_fill_holes``):
    python tests/golden/make_golden_voxelgrid_ops.py
The two reference files are loaded by path on top of _refload's stub ``kaolin`` package.  Every input is built here
(seeded where random); the file records inputs, the reference's outputs and the type and text of the errors it raises.
Boolean grids are stored as np.packbits of the flattened grid plus ``<name>_shape``.

``fill`` cases, and what each is for (the generator asserts the stated property of the reference's answer):
  doc            the reference's docstring grid (1, 3, 4, 5)
  shell_thin     lattice shell 14^2 <= |p - c|^2 <= 15^2 on (70, 45, 37), c = (33, 22, 18): Z = 37 is one word and a partial
  shell_thick    one; the cavity crosses the word boundary and the brick boundaries.  Filled: |p - c|^2 <= 15^2, 14147 voxels
  shell_puncture shell_thick without (33, 22, 31..33): a one-voxel channel; the answer is the input
  cube_corner    5^3, cube 1:4 without its centre and its corner (1, 1, 1): the centre fills, the corner (reached only
                 across edges and corners of the outside) does not -- connectivity is 6
  values         3^3 of 0.4, -1, nan, one -0.0 and an enclosed 0: != 0 is the wall test (valued: float dtypes only)
  serp_open      a one-voxel-wide serpentine corridor in the middle layer of a (41, 41, 3) slab of walls, entered from the
  serp_sealed    face x = 0: open -> the input; entrance sealed -> everything.  Its geodesic length is >= 500
  serpz_open     the same corridor in the (y, z) plane of a (3, 21, 72) slab: the long runs lie along Z, across the word
  serpz_sealed   boundaries at 32 and 64
  batch          3 items of (9, 9, 37): a closed box, nothing, and walls on the array's own faces (everything fills); voxels
                 enclosed in one item are outside in the next, rows adjacent in memory belong to different items
  z1, x1         Z = 1 and X = 1: every voxel is on a boundary face
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload  # noqa: E402


def load_modules():
    _refload.load_reference()
    ops = _refload._load('kaolin.ops.voxelgrid', 'kaolin/ops/voxelgrid.py')
    metrics = _refload._load('kaolin.metrics.voxelgrid', 'kaolin/metrics/voxelgrid.py')
    return ops, metrics


def lattice_shell(shape, c, r1, r2):
    x, y, z = np.meshgrid(*[np.arange(s) for s in shape], indexing='ij')
    d2 = (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2
    return (d2 >= r1 * r1) & (d2 <= r2 * r2), d2


def serpentine(rows, cols):
    """(rows, cols) plane, True = wall: corridor rows 1, 3, ... spanning columns 1..cols-2, joined at alternating ends,
    entered at (0, 1).  Returns (walls, the entrance)."""
    wall = np.ones((rows, cols), dtype=bool)
    odd = list(range(1, rows - 1, 2))
    for i, r in enumerate(odd):
        wall[r, 1:cols - 1] = False
        if i + 1 < len(odd):
            wall[r + 1, cols - 2 if i % 2 == 0 else 1] = False
    wall[0, 1] = False
    return wall, (0, 1)


def geodesic_length(wall, start):
    """Steps of 6-connected growth from `start` through the empty voxels until nothing is added."""
    reached = np.zeros_like(wall)
    reached[start] = True
    steps = 0
    while True:
        grown = reached.copy()
        for ax in range(wall.ndim):
            a = [slice(None)] * wall.ndim
            b = [slice(None)] * wall.ndim
            a[ax], b[ax] = slice(1, None), slice(None, -1)
            grown[tuple(a)] |= reached[tuple(b)]
            grown[tuple(b)] |= reached[tuple(a)]
        grown &= ~wall
        if (grown == reached).all():
            return steps, reached
        reached, steps = grown, steps + 1


def fill_cases():
    cases = {}
    doc = np.zeros((1, 3, 4, 5), dtype=bool)
    doc[0, :, 1:, 1:] = True
    doc[0, 1, 2, 2:4] = False
    cases['doc'] = doc

    shape, c = (70, 45, 37), (33, 22, 18)
    thin, d2 = lattice_shell(shape, c, 14, 15)
    thick, _ = lattice_shell(shape, c, 13, 15)
    punct = thick.copy()
    punct[33, 22, 31:34] = False
    cases['shell_thin'], cases['shell_thick'], cases['shell_puncture'] = thin[None], thick[None], punct[None]

    cube = np.zeros((5, 5, 5), dtype=bool)
    cube[1:4, 1:4, 1:4] = True
    cube[2, 2, 2] = False
    cube[1, 1, 1] = False
    cases['cube_corner'] = cube[None]

    for name, plane_shape, embed in (('serp', (41, 41), lambda p: np.stack([np.ones_like(p), p, np.ones_like(p)], axis=2)),
                                     ('serpz', (21, 72), lambda p: np.stack([np.ones_like(p), p, np.ones_like(p)], axis=0))):
        plane, entrance = serpentine(*plane_shape)
        grid = embed(plane)
        start = (entrance[0], entrance[1], 1) if name == 'serp' else (1, entrance[0], entrance[1])
        assert not grid[start]
        length, reached = geodesic_length(grid, start)
        assert length >= 500, (name, length)
        assert (reached == ~grid).all()          # one corridor: the entrance reaches every empty voxel
        sealed = grid.copy()
        sealed[start] = True
        cases[f'{name}_open'], cases[f'{name}_sealed'] = grid[None], sealed[None]

    batch = np.zeros((3, 9, 9, 37), dtype=bool)
    batch[0, 1:8, 1:8, 1:36] = True
    batch[0, 2:7, 2:7, 2:35] = False             # a closed box: its inside is enclosed, the array's last rows stay empty
    batch[2] = True
    batch[2, 1:8, 1:8, 1:36] = False             # walls on the array's faces: the whole interior is enclosed
    cases['batch'] = batch

    ring = np.zeros((2, 7, 7, 1), dtype=bool)
    ring[0, 1:6, 1:6, 0] = True
    ring[0, 2:5, 2:5, 0] = False
    ring[1, 3, :, 0] = True
    cases['z1'] = ring
    flat = np.zeros((1, 1, 9, 40), dtype=bool)
    flat[0, 0, 2:7, 10:36] = True
    flat[0, 0, 3:6, 12:34] = False
    cases['x1'] = flat
    return cases, d2


def record_error(out, name, fn):
    try:
        fn()
    except Exception as err:  # noqa: BLE001  (the reference's own error, whatever its type)
        out[f'err_{name}'] = np.array([type(err).__name__, str(err)])
        return
    raise AssertionError(f'{name}: the reference raised nothing')


def main():
    ops, metrics = load_modules()
    g = torch.Generator().manual_seed(0)
    out = {}

    def store_bool(name, arr):
        arr = np.asarray(arr, dtype=bool)
        out[f'{name}_bits'] = np.packbits(arr.reshape(-1))
        out[f'{name}_shape'] = np.array(arr.shape, dtype=np.int64)

    # ---- fill ----------------------------------------------------------------------------------------------------------
    cases, d2 = fill_cases()
    for name, grid in cases.items():
        res = ops.fill(torch.from_numpy(grid).float())
        assert res.dtype == torch.bool and tuple(res.shape) == grid.shape
        store_bool(f'fill_{name}_in', grid)
        store_bool(f'fill_{name}_out', res.numpy())
    got = {k: np.unpackbits(out[f'fill_{k}_out_bits'])[:cases[k].size].reshape(cases[k].shape).astype(bool) for k in cases}
    ball = d2 <= 15 * 15
    assert ball.sum() == 14147
    assert (got['shell_thin'][0] == ball).all() and (got['shell_thick'][0] == ball).all()
    assert (got['shell_puncture'] == cases['shell_puncture']).all()
    assert got['cube_corner'][0, 2, 2, 2] and not got['cube_corner'][0, 1, 1, 1]
    for name in ('serp', 'serpz'):
        assert (got[f'{name}_open'] == cases[f'{name}_open']).all() and got[f'{name}_sealed'].all()
    assert (got['batch'][1] == 0).all() and got['batch'][2].all() and got['batch'][0, 1:8, 1:8, 1:36].all()
    assert got['batch'][0].sum() == 7 * 7 * 35
    assert (got['z1'] == cases['z1']).all() and (got['x1'] == cases['x1']).all()
    out['fill_cases'] = np.array(sorted(cases))

    nan = float('nan')
    values = torch.tensor([[[0.4, -1., nan], [nan, 0.4, -1.], [-1., nan, 0.4]],
                           [[-1., 0.4, nan], [0.4, 0., -1.], [nan, -1., 0.4]],
                           [[-0., nan, -1.], [-1., 0.4, nan], [0.4, -1., nan]]]).unsqueeze(0)
    res = ops.fill(values)
    assert res[0, 1, 1, 1] and not res[0, 2, 0, 0] and res.sum() == 26
    out['fill_values_in'] = values.numpy()
    store_bool('fill_values_out', res.numpy())

    # ---- extract_surface ---------------------------------------------------------------------------------------------
    solid = torch.zeros(2, 6, 7, 8)
    solid[0, 1:6, 0:5, 2:8] = 1.
    solid[1] = (torch.rand(6, 7, 8, generator=g) < 0.7).float()
    out['surface_in'] = solid.numpy()
    for mode in ('wide', 'thin'):
        res = ops.extract_surface(solid, mode)
        assert res.dtype == torch.bool
        store_bool(f'surface_{mode}', res.numpy())
    record_error(out, 'surface_mode', lambda: ops.extract_surface(solid, 'narrow'))
    record_error(out, 'surface_ndim', lambda: ops.extract_surface(solid[0]))

    # ---- downsample: values are multiples of 1/16, so every summation order gives the same float --------------------------
    dense = torch.randint(0, 17, (2, 8, 12, 6), generator=g).float() / 16
    out['down_in'] = dense.numpy()
    for tag, scale in (('int2', 2), ('list232', [2, 3, 2]), ('list461', [4, 6, 1]), ('tuple223', (2, 2, 3)), ('int1', 1)):
        out[f'down_{tag}'] = ops.downsample(dense, scale).numpy()
    out['down_bool_in'] = (dense > 0.5).numpy()
    out['down_bool_int2'] = ops.downsample(dense > 0.5, 2).numpy()
    record_error(out, 'down_list_len', lambda: ops.downsample(dense, [2, 2]))
    record_error(out, 'down_ndim', lambda: ops.downsample(dense.unsqueeze(0), [2, 2, 2]))
    record_error(out, 'down_small', lambda: ops.downsample(dense, [2, 0, 2]))
    record_error(out, 'down_large', lambda: ops.downsample(dense, [2, 2, 7]))
    record_error(out, 'down_type', lambda: ops.downsample(dense, 2.5))
    record_error(out, 'down_int_large', lambda: ops.downsample(dense, 7))

    # ---- odms -----------------------------------------------------------------------------------------------------------
    vox = (torch.rand(2, 5, 5, 5, generator=g) < 0.35)
    vox[1, 1:4, 1:4, 1:4] = True
    out['odm_vox'] = vox.numpy()
    odms = ops.extract_odms(vox)
    assert odms.dtype == torch.long
    out['odm_odms'] = odms.numpy()
    out['odm_odms_float'] = ops.extract_odms(vox.float()).numpy()
    noisy = (odms + torch.randint(-1, 3, odms.shape, generator=g)).clamp(0, 5)
    out['odm_noisy'] = noisy.numpy()
    for votes in (1, 2, 7):
        for tag, src in (('exact', odms), ('noisy', noisy)):
            store_bool(f'proj_{tag}_v{votes}', ops.project_odms(src, votes=votes).numpy())
            store_bool(f'proj_{tag}_v{votes}_vox', ops.project_odms(src, voxelgrids=vox, votes=votes).numpy())
    record_error(out, 'proj_six', lambda: ops.project_odms(odms[:, :5]))
    record_error(out, 'proj_batch', lambda: ops.project_odms(odms, voxelgrids=vox[:1]))
    record_error(out, 'proj_dim', lambda: ops.project_odms(odms, voxelgrids=torch.ones(2, 5, 4, 5)))

    # ---- iou ------------------------------------------------------------------------------------------------------------
    pred = (torch.rand(3, 4, 5, 6, generator=g) < 0.5).float()
    gt = (torch.rand(3, 4, 5, 6, generator=g) < 0.5).float()
    pred[2] = 0.
    gt[2] = 0.                                    # an empty union: nan is the reference's answer
    res = metrics.iou(pred, gt)
    assert res.dtype == torch.float32 and torch.isnan(res[2]) and not torch.isnan(res[:2]).any()
    out.update(iou_pred=pred.numpy(), iou_gt=gt.numpy(), iou_out=res.numpy())
    record_error(out, 'iou_shape', lambda: metrics.iou(pred, gt[:, :3]))

    np.savez_compressed(os.path.join(HERE, 'voxelgrid_ops.npz'), **out)
    print('wrote voxelgrid_ops.npz', len(out), 'arrays', os.path.getsize(os.path.join(HERE, 'voxelgrid_ops.npz')), 'bytes')
    for k in sorted(out):
        if k.startswith('err_'):
            print(k, list(out[k]))


if __name__ == '__main__':
    main()
