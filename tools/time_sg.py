"""Times kaolin.render.lighting's SG shading on one GPU: one JSON line per case, forward and forward + backward.

    python tools/time_sg.py [--reps 10] [--no-torch]

Cases: sg_diffuse_inner_product (the constant cosine lobe: 12-byte rows) and sg_warp_specular_term (general rows: 28 bytes),
on N = the covered pixels of the bench's sphere scene over 8 views at 1024^2 (`sphere_scene` / `fibonacci_cameras`, normals
interpolated by the rasterizer) and on all 8 x 1024^2 pixels, with L = 8, 32 and 128 lights.  Beside the HIP path: the torch
broadcast composition (unbatched_sg_inner_product(...).sum(1), what the reference runs below 8 lights and what its test uses
as ground truth) where it fits in memory, else null.

Bounds of the reduced-product kernels (the rest of each public call is a few elementwise torch ops):
  * bytes / HBM peak (8.0 TB/s): rows read and written once per launch, lights negligible;
  * vector issue / the chip's vector rate: per (row, light) pair the arithmetic of csrc/sg_lighting.hip in wave64 issue
    cycles -- 4 per v_fma / v_mul / v_add, 8 per transcendental (v_exp_f32 x2, v_rsq_f32 x1) (MI355X_MICROARCH constants:
    'vector-instruction ISSUE cost') -- over 256 CUs x 4 SIMDs x 2.4 GHz.  Forward: 17 plain + 3 transcendental = 92
    cycles per 64 pairs; backward: 31 plain (34 with general rows) + 3 transcendental = 148 (160).  These are the source's
    minimum counts; the compiled loop adds moves of the wave-uniform light values.
`frac_of_bound` = the tighter (larger) bound over the measured time of the whole public call.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

HBM_BPS = 8.0e12
SIMD_CYCLES_PER_S = 256 * 4 * 2.4e9
CYC = {('fwd', 'diffuse'): 17 * 4 + 3 * 8, ('fwd', 'specular'): 17 * 4 + 3 * 8,
       ('bwd', 'diffuse'): 31 * 4 + 3 * 8, ('bwd', 'specular'): 34 * 4 + 3 * 8}
ROW_BYTES = {('fwd', 'diffuse'): 12 + 12, ('fwd', 'specular'): 28 + 12,
             ('bwd', 'diffuse'): 12 + 12 + 12, ('bwd', 'specular'): 12 + 28 + 28}


def bounds_ms(case, n, m, with_bwd):
    parts = ('fwd', 'bwd') if with_bwd else ('fwd',)
    byt = sum(ROW_BYTES[(p, case)] for p in parts) * n
    cyc = sum(CYC[(p, case)] for p in parts) * n * m / 64
    return byt / HBM_BPS * 1e3, cyc / SIMD_CYCLES_PER_S * 1e3


def covered_normals(views=8, res=1024):
    """Unit normals of the covered pixels of the sphere scene (per-vertex normals interpolated by the rasterizer)."""
    import kaolin_amd as kal
    from kaolin_amd.utils import testing as T
    verts, faces = T.geodesic_sphere(16)
    verts = verts.float().cuda()
    faces = faces.cuda()
    fz, fimg, nz = T.project_mesh(verts, faces, T.fibonacci_cameras(views).cuda())
    feat = torch.nn.functional.normalize(verts, dim=1)[faces].unsqueeze(0).expand(views, -1, -1, -1).contiguous()
    with torch.no_grad():
        (img,), _, face_idx = kal.render.mesh.dibr_rasterization(res, res, fz, fimg, [feat], nz)
    return torch.nn.functional.normalize(img[face_idx >= 0], dim=1).contiguous()


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--no-torch', action='store_true')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_sg.py measures on the GPU'
    from kaolin_amd.render import lighting
    from kaolin_amd.render.lighting import sg as sgm

    g = torch.Generator(device='cuda').manual_seed(0)
    cov = covered_normals()
    full_n = 8 * 1024 * 1024
    full = torch.nn.functional.normalize(torch.randn(full_n, 3, generator=g, device='cuda'), dim=1)

    def composition(case, lights, x):
        la, ld, ls = lights
        if case == 'diffuse':
            irr = sgm.unbatched_sg_inner_product(*sgm.cosine_lobe_sg(x['normal']), la, ld, ls).sum(1)
            return torch.clamp(irr, min=0.) * (x['albedo'] / math.pi)
        # the specular term with the reduced product as the broadcast sum
        saved = sgm.unbatched_reduced_sg_inner_product
        sgm.unbatched_reduced_sg_inner_product = lambda *a: sgm.unbatched_sg_inner_product(*a).sum(1)
        try:
            return lighting.sg_warp_specular_term(la, ld, ls, x['normal'], x['rough'], x['view'], x['spec'])
        finally:
            sgm.unbatched_reduced_sg_inner_product = saved

    def hip(case, lights, x):
        if case == 'diffuse':
            return lighting.sg_diffuse_inner_product(*lights, x['normal'], x['albedo'])
        return lighting.sg_warp_specular_term(*lights, x['normal'], x['rough'], x['view'], x['spec'])

    for case in ('diffuse', 'specular'):
        for rows_name, normal in (('covered_8x1024^2', cov), ('all_8x1024^2', full)):
            n = normal.shape[0]
            x = {'normal': normal, 'albedo': torch.rand(n, 3, generator=g, device='cuda')}
            if case == 'specular':
                jitter = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, device='cuda'), dim=1)
                x['view'] = torch.nn.functional.normalize(normal + 0.5 * jitter, dim=1)
                x['rough'] = torch.rand(n, generator=g, device='cuda') * 0.6 + 0.3
                x['spec'] = torch.rand(n, 3, generator=g, device='cuda')
            gout = torch.rand(n, 3, generator=g, device='cuda')
            for m in (8, 32, 128):
                lights = [torch.rand(m, 3, generator=g, device='cuda') * 2,
                          torch.nn.functional.normalize(torch.randn(m, 3, generator=g, device='cuda'), dim=1),
                          torch.rand(m, generator=g, device='cuda') * 8 + 0.5]
                lights = [t.requires_grad_() for t in lights]
                xg = dict(x, normal=x['normal'].clone().requires_grad_())
                diff = lights + [xg['normal']]

                def fwd(f):
                    def run():
                        with torch.no_grad():
                            f(case, lights, xg)
                    return run

                def fwd_bwd(f):
                    def run():
                        torch.autograd.grad(f(case, lights, xg), diff, gout)
                    return run

                rec = {'case': case, 'rows': rows_name, 'N': n, 'L': m}
                rec['hip_fwd_ms'] = round(timed(fwd(hip), args.reps), 4)
                rec['hip_fwd_bwd_ms'] = round(timed(fwd_bwd(hip), args.reps), 4)
                for key, with_bwd in (('fwd', False), ('fwd_bwd', True)):
                    b_bytes, b_valu = bounds_ms(case, n, m, with_bwd)
                    rec[f'bound_{key}_bytes_ms'] = round(b_bytes, 4)
                    rec[f'bound_{key}_valu_ms'] = round(b_valu, 4)
                    rec[f'{key}_bound'] = 'valu' if b_valu >= b_bytes else 'bytes'
                    rec[f'{key}_frac_of_bound'] = round(max(b_bytes, b_valu) / rec[f'hip_{key}_ms'], 3)
                rec['torch_fwd_ms'] = rec['torch_fwd_bwd_ms'] = None
                # broadcast intermediates: ~12 (N, L, 3) fp32 tensors alive with autograd
                if not args.no_torch and n * m * 3 * 4 * 12 < 150e9:
                    try:
                        reps = max(1, args.reps // 5)
                        rec['torch_fwd_ms'] = round(timed(fwd(composition), reps, warmup=1), 4)
                        rec['torch_fwd_bwd_ms'] = round(timed(fwd_bwd(composition), reps, warmup=1), 4)
                    except torch.cuda.OutOfMemoryError:
                        rec['torch_note'] = 'out of memory'
                    torch.cuda.empty_cache()
                print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
