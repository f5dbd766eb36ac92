"""Generates tests/golden/render_helpers.npz FROM THE REFERENCE ITSELF: ``prepare_vertices`` and ``texture_mapping`` of
kaolin/render/mesh/utils.py and ``mask_iou`` of kaolin/metrics/render.py, in float64 on the CPU.

Run in the build container (where the reference tree is mounted):
    python tests/golden/make_golden_render_helpers.py
The reference's files are loaded by path on top of _refload's stub ``kaolin`` package: render/mesh/utils.py, metrics/render.py,
render/camera/legacy.py and, for ``index_vertices_by_faces`` and ``face_normals``, ops/mesh/mesh.py and ops/mesh/trianglemesh.py.
The inputs come from tests/render_helper_cases.py (its head describes every case); the file records them as float32, and for
every entry of the pinning sets (``PV_PINNED``, ``TM_PINNED``, ``MI_PINNED``) the reference's float64 outputs and the autograd
gradients of sum(output * upstream gradient).

The generator asserts what the cases claim to be, on the reference's own answers:
  * the faces of ``PV_ZERO_NORMALS`` (a repeated vertex, three collinear vertices) have a normal of exactly 0, in float64 and
    in float32, and a finite vertex gradient;
  * the tie cases put at least 5 coordinates on x.5 source indices, the same ones in float32 and float64 arithmetic, and
    `nearest` picks the even neighbour there;
  * in every `nearest` case of the kernel set the float32 and the float64 run choose the same texel everywhere;
  * a source index exactly on the first or last texel centre has a uv gradient of exactly 0, and such samples exist;
  * the ``kinds`` batch of mask_iou holds an empty pair, an identical hard pair and an empty-against-full pair.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import _refload  # noqa: E402
import render_helper_cases as rc  # noqa: E402


def load_modules():
    mods = _refload.load_reference()
    mesh = _refload._load('kaolin.ops.mesh.mesh', 'kaolin/ops/mesh/mesh.py')
    k = sys.modules['kaolin']
    k.ops, k.render = sys.modules['kaolin.ops'], sys.modules['kaolin.render']
    k.ops.mesh = sys.modules['kaolin.ops.mesh']
    k.ops.mesh.index_vertices_by_faces = mesh.index_vertices_by_faces
    k.ops.mesh.face_normals = mods['ops_trianglemesh'].face_normals
    cam = sys.modules['kaolin.render.camera']
    k.render.camera = cam
    cam.rotate_translate_points = mods['legacy_camera'].rotate_translate_points
    cam.perspective_camera = mods['legacy_camera'].perspective_camera
    utils = _refload._load('kaolin.render.mesh.utils', 'kaolin/render/mesh/utils.py')
    metrics = _refload._load('kaolin.metrics.render', 'kaolin/metrics/render.py')
    return utils.prepare_vertices, utils.texture_mapping, metrics.mask_iou


def main():
    prepare_vertices, texture_mapping, mask_iou = load_modules()
    f64, f32 = torch.float64, torch.float32
    out = {}

    def store(tag, res, names):
        for k in names:
            if res[k] is not None:
                assert res[k].dtype == f64 and bool(torch.isfinite(res[k]).all()), (tag, k)
                out[f'{tag}__{k}'] = res[k].numpy()

    def store_inputs(prefix, case, names):
        for k in names:
            t = case[k]
            out[f'{prefix}__{case["name"]}__in_{k}'] = t.numpy() if t.dtype == torch.long else t.to(f32).numpy()
            assert t.dtype == torch.long or bool((t.to(f32).double() == t).all())

    # ---- prepare_vertices ------------------------------------------------------------------------------------------------
    pv = rc.pv_cases()
    for name in sorted({e[0] for e in rc.PV_PINNED}):
        store_inputs('pv', pv[name], rc.PV_INPUTS)
    for name, camera, layout, which in rc.PV_PINNED:
        res = rc.pv_run(prepare_vertices, pv[name], camera, layout, f64, which=which)
        store(rc.pv_tag(name, camera, layout, which), res, rc.PV_TENSORS)
        if name in rc.PV_ZERO_NORMALS:
            res32 = rc.pv_run(prepare_vertices, pv[name], camera, layout, f32, which=which)
            for r in (res, res32):
                faces = list(rc.PV_ZERO_NORMALS[name])
                assert bool((r['nrm'][:, faces] == 0).all()), (name, camera, layout)
                assert bool((r['nrm'].norm(dim=-1)[:, [f for f in range(r['nrm'].shape[1]) if f not in faces]] > 0.99).all())
                assert bool(torch.isfinite(r['gv']).all())
        if name == 'f0':
            assert res['cam'].shape == (2, 0, 3, 3) and res['img'].shape == (2, 0, 3, 2) and res['nrm'].shape == (2, 0, 3)
            assert bool((res['gv'] == 0).all())
        idle = rc.unreferenced_vertices(pv[name])
        if layout != 'strided':
            assert bool((res['gv'][:, idle] == 0).all())
    assert bool(rc.unreferenced_vertices(pv['b3_f21']).any())

    # ---- texture_mapping -------------------------------------------------------------------------------------------------
    tm = rc.tm_cases()
    for name in sorted({e[0] for e in rc.TM_PINNED}):
        store_inputs('tm', tm[name], rc.TM_INPUTS)
    for name, mode, need in rc.TM_PINNED:
        store(rc.tm_tag(name, mode, need), rc.tm_run(texture_mapping, tm[name], mode, f64, need=need), rc.TM_TENSORS)
    clipped = 0
    for name in rc.TM_KERNEL_SET:
        case = tm[name]
        n64, n32 = (rc.tm_run(texture_mapping, case, 'nearest', dt) for dt in (f64, f32))
        assert torch.equal(n32['out'].double(), n64['out']), name                  # the same texel in both precisions
        assert bool((n64['g_uv'] == 0).all()) and bool((n32['g_uv'] == 0).all())
        th, tw = case['tex'].shape[2:]
        s64, s32 = rc.tm_source_index(case, f64), rc.tm_source_index(case, f32)
        lim = torch.tensor([tw - 1., th - 1.], dtype=f64)
        if name in rc.TM_TIE_CASES:
            inside = (s64 > 0) & (s64 < lim)
            tie64, tie32 = (s64 - torch.floor(s64) == 0.5) & inside, (s32 - torch.floor(s32) == 0.5) & inside
            assert torch.equal(tie64, tie32) and int(tie64.sum()) >= 5, (name, int(tie64.sum()))
            # round half to even: among the ties there are indices k + 0.5 with k odd, where floor(x + 0.5) would differ
            assert bool((torch.floor(s64[tie64]) % 2 == 0).any())
            B, C = case['tex'].shape[:2]
            picked = n64['out'].reshape(B, -1, C)
            both = tie64.any(dim=-1)
            ix, iy = torch.round(s64[..., 0].clamp(0, tw - 1)).long(), torch.round(s64[..., 1].clamp(0, th - 1)).long()   # torch.round: half to even
            for b, i in both.nonzero().tolist():
                assert torch.equal(picked[b, i], case['tex'][b, :, iy[b, i], ix[b, i]]), (name, b, i)
        if case['conditioned']:
            b64 = rc.tm_run(texture_mapping, case, 'bilinear', f64)
            on_border = (s64 == 0) | (s64 == lim)                                   # exactly on the first / last centre
            g = b64['g_uv'].reshape(s64.shape)
            assert bool((g[on_border] == 0).all()), name
            clipped += int(on_border.sum())
    assert clipped >= 20, clipped

    # ---- mask_iou --------------------------------------------------------------------------------------------------------
    mi = rc.mi_cases()
    for name in sorted({e[0] for e in rc.MI_PINNED}):
        store_inputs('mi', mi[name], rc.MI_INPUTS)
    for name, need in rc.MI_PINNED:
        store(rc.mi_tag(name, need), rc.mi_run(mask_iou, mi[name], f64, need=need), rc.MI_TENSORS)
    kinds = mi['kinds']
    assert not kinds['lhs'][0].any() and not kinds['rhs'][0].any()
    assert torch.equal(kinds['lhs'][1], kinds['rhs'][1]) and set(kinds['lhs'][1].unique().tolist()) == {0., 1.}
    assert not kinds['lhs'][2].any() and bool((kinds['rhs'][2] == 1).all())

    path = os.path.join(HERE, 'render_helpers.npz')
    np.savez_compressed(path, **out)
    print('wrote render_helpers.npz', len(out), 'arrays', os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
