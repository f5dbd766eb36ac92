"""Generates tests/golden/sg_lighting.npz FROM THE REFERENCE ITSELF (kaolin.render.lighting).

Run in the build container (where the reference tree is mounted):
    python tests/golden/make_golden_sg.py
The reference's render/lighting/sg.py and sh.py are loaded by path on top of _refload's stub ``kaolin`` package.  The fused
reduced op is replaced by the reference's own ground truth, ``unbatched_sg_inner_product(...).sum(1)`` (the comparison its
test_sg.py makes).  Inputs are seeded; every output is computed in float64 and its gradients by autograd.
"""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _refload  # noqa: E402

REDUCED_CASES = ((1, 1), (17, 7), (33, 8), (64, 17), (65, 64), (100, 65), (23, 511), (7, 1))


def load_lighting():
    _refload.load_reference()
    sys.modules['kaolin._C'].render.sg = types.ModuleType('kaolin._C.render.sg')
    sys.modules['kaolin._C.render.sg'] = sys.modules['kaolin._C'].render.sg
    sys.modules['kaolin.render.lighting'] = types.ModuleType('kaolin.render.lighting')
    sys.modules['kaolin.render.lighting'].__path__ = []
    sg = _refload._load('kaolin.render.lighting.sg', 'kaolin/render/lighting/sg.py')
    sh = _refload._load('kaolin.render.lighting.sh', 'kaolin/render/lighting/sh.py')
    sg.unbatched_reduced_sg_inner_product = lambda *a: sg.unbatched_sg_inner_product(*a).sum(1)
    return sg, sh


def unit(n, g):
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return v / v.norm(dim=1, keepdim=True)


def main():
    sg, sh = load_lighting()
    g = torch.Generator().manual_seed(0)
    out = {}

    def rand(*shape):
        return torch.rand(*shape, generator=g, dtype=torch.float64)

    # broadcast inner product
    args = [rand(5, 3), rand(5, 3), rand(5), rand(7, 3), rand(7, 3), rand(7)]
    for k, t in zip(('a', 'd', 's', 'oa', 'od', 'os'), args):
        out[f'inner_{k}'] = t
    out['inner_out'] = sg.unbatched_sg_inner_product(*args)

    # reduced op: forward, |terms| summed, and the six gradients of sum(out * grad_out)
    for n, m in REDUCED_CASES:
        tag = f'red_{n}_{m}'
        args = [rand(n, 3), rand(n, 3), rand(n), rand(m, 3), rand(m, 3), rand(m)]
        go = rand(n, 3)
        args = [t.requires_grad_() for t in args]
        pairs = sg.unbatched_sg_inner_product(*args)
        res = sg.unbatched_reduced_sg_inner_product(*args)
        grads = torch.autograd.grad((res * go).sum(), args)
        for k, t in zip(('a', 'd', 's', 'oa', 'od', 'os'), args):
            out[f'{tag}_{k}'] = t.detach()
        out[f'{tag}_go'] = go
        out[f'{tag}_out'] = res.detach()
        out[f'{tag}_out_abs'] = pairs.detach().abs().sum(1)
        for k, t in zip(('ga', 'gd', 'gs', 'goa', 'god', 'gos'), grads):
            out[f'{tag}_{k}'] = t

    # shading: lights, surface points
    L, P = 9, 50
    la, ld, ls = rand(L, 3) * 2., unit(L, g), rand(L) * 8. + 0.5
    normal, albedo = unit(P, g), rand(P, 3)
    view = normal + 0.5 * unit(P, g)
    view = view / view.norm(dim=1, keepdim=True)
    rough, spec = rand(P) * 0.6 + 0.3, rand(P, 3)
    for k, t in dict(la=la, ld=ld, ls=ls, normal=normal, albedo=albedo, view=view, rough=rough, spec=spec).items():
        out[f'shade_{k}'] = t
    out['irr_ip'] = sg.sg_irradiance_inner_product(la, ld, ls, normal)
    out['diff_ip'] = sg.sg_diffuse_inner_product(la, ld, ls, normal, albedo)
    out['irr_fit'] = sg.sg_irradiance_fitted(la, ld, ls, normal)
    out['diff_fit'] = sg.sg_diffuse_fitted(la, ld, ls, normal, albedo)
    out['spec'] = sg.sg_warp_specular_term(la, ld, ls, normal, rough, view, spec)
    da, dd, ds = sg.sg_distribution_term(normal, rough)
    out['ndf_a'], out['ndf_s'] = da, ds
    wa, wd, ws = sg.sg_warp_distribution(da, dd, ds, view)
    out['warp_d'], out['warp_s'] = wd, ws
    ldh = rand(P, 1)
    out['fresnel_ldh'], out['fresnel'] = ldh, sg.fresnel(ldh, spec)
    out['integral'] = sg.approximate_sg_integral(la, ls)

    # suns and parameters
    sun_dir, strength = unit(4, g), rand(4) * 3. + 1.
    angle = torch.tensor([math.pi / 4, 0.1, 1.0, 2 * math.pi], dtype=torch.float64)
    color = rand(4, 3)
    amp, _, sharp = sg.sg_from_sun(sun_dir, strength, angle, color)
    out.update(sun_dir=sun_dir, sun_strength=strength, sun_angle=angle, sun_color=color, sun_amp=amp, sun_sharp=sharp)
    az, el = rand(6) * 2 * math.pi, rand(6) * math.pi - math.pi / 2
    out.update(azel_az=az, azel_el=el, azel_dir=sg.sg_direction_from_azimuth_elevation(az, el))
    p = sg.SgLightingParameters.from_sun(sun_dir.float(), 2.5, 0.5)
    out.update(params_sun_amp=p.amplitude, params_sun_dir=p.direction, params_sun_sharp=p.sharpness)
    raw_dir = rand(3, 3) + 0.1
    p = sg.SgLightingParameters(amplitude=2., direction=raw_dir.float(), sharpness=4.)
    out.update(params_raw_dir=raw_dir, params_amp=p.amplitude, params_dir=p.direction, params_sharp=p.sharpness)

    # spherical harmonics
    sh_dir = unit(1, g)[0]
    out.update(sh_dir=sh_dir, sh_coeffs=sh.project_onto_sh9(sh_dir), sh_normals=normal,
               sh_proj=sh.project_onto_sh9(normal), sh_irr=sh.sh9_irradiance(sh.project_onto_sh9(sh_dir), normal),
               sh_diffuse=sh.sh9_diffuse(sh_dir, normal, albedo))

    arrays = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, 'sg_lighting.npz'), **arrays)
    print('wrote sg_lighting.npz', len(arrays), 'arrays')


if __name__ == '__main__':
    main()
