"""Times ops.mesh.sample_points and face_areas (the HIP pipeline of csrc/sample_points.hip) on one GPU: one JSON line per case.

    python tools/time_sample_points.py [--reps 7] [--out profiles/sample_points_time.jsonl]

Shapes (seeded, float32): the bench sphere (geodesic, 50 000 faces) with B = 8 and N = 100 000 samples per item, without features and
with D = 3 features; a 709 x 709 grid mesh (1 005 362 faces) with B = 1 and N = 2^20; D = 4 / 8 / 16 / 32 features on the sphere at
N = 20 000, the shapes either side of the kernel's switch from a loop in the sample's thread to lanes along the feature dimension
(``SP_FEATURE_LANES_FROM``).  With an experiment build of the library (``make -C kaolin_amd/csrc variant``, ``KAMD_LIB_PATH``) the
switch follows ``KAMD_SP_LANES_FROM``; the value is recorded as `lanes_from_env`, so both forms can be timed at one D.  Every case
runs in a child process of its own under a time limit; the first failure ends the run.

Per case, the median over the repetitions of the whole public call between two device events, after a warm-up: `fwd_ms`,
`fwd_bwd_ms` (forward + backward to vertices and face_features), `areas_ms` (face_areas alone), and `user_*` = the same for WHAT THE
REFERENCE RUNS: its expression written in torch on the same GPU tensors (index_select x 3, Categorical(...).sample, gather, rand,
blend).  Before timing the areas of both sides are compared (the samples are not comparable: other random streams).  `launches_*`
are device activities counted by torch's profiler over one call (the two rand of the HIP side included), `host_reads_*` the
synchronising reads torch reports.  `bound_share_*` = the time the compulsory traffic takes at 6.3 TB/s (inputs read once, outputs
written once) over the measured time."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ['sphere', 'sphere_d3', 'grid_1m', 'sphere_d4', 'sphere_d8', 'sphere_d16', 'sphere_d32']
CASE_TIME_LIMIT_S = 150
HBM_BYTES_PER_S = 6.3e12


def median_ms(fn, reps):
    import torch
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return round(statistics.median(times), 4)


def count_launches(fn):
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return n if n > 0 else 'not measured'
    except Exception:  # noqa: BLE001  (no profiler on this build: the count is optional)
        return 'not measured'


def count_host_reads(fn):
    import torch
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            fn()
        return sum(1 for w in seen if 'synchroniz' in str(w.message))
    finally:
        torch.cuda.set_sync_debug_mode('default')


def grid_mesh(cells):
    import numpy as np
    import torch
    i, j = np.meshgrid(np.arange(cells), np.arange(cells), indexing='ij')
    a = i * (cells + 1) + j
    b, c, d = a + cells + 1, a + cells + 2, a + 1
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    x, y = np.meshgrid(np.linspace(-1, 1, cells + 1), np.linspace(-1, 1, cells + 1), indexing='ij')
    vertices = np.stack([x, y, 0.1 * np.sin(3 * x) * np.cos(2 * y)], -1).reshape(-1, 3)
    return torch.from_numpy(vertices).float(), torch.from_numpy(faces)


def reference_sample_points(vertices, faces, num_samples, face_features=None):
    """kaolin/ops/mesh/trianglemesh.py:159-240, its expression in torch"""
    import torch
    f0, f1, f2 = torch.split(faces, 1, dim=1)
    fv = [torch.index_select(vertices, 1, f.reshape(-1)) for f in (f0, f1, f2)]
    x1, x2, x3 = torch.split(fv[0] - fv[1], 1, dim=-1)
    y1, y2, y3 = torch.split(fv[1] - fv[2], 1, dim=-1)
    areas = (torch.sqrt((x2 * y3 - x3 * y2) ** 2 + (x3 * y1 - x1 * y3) ** 2 + (x1 * y2 - x2 * y1) ** 2) * 0.5).squeeze(-1)
    choices = torch.distributions.Categorical(areas).sample([num_samples]).transpose(0, 1)
    index = choices.unsqueeze(-1).repeat(1, 1, 3)
    v0, v1, v2 = (torch.gather(c, 1, index) for c in fv)
    shape = tuple(v0.shape[:-1]) + (1,)
    u = torch.sqrt(torch.rand(shape, device=v0.device, dtype=v0.dtype))
    v = torch.rand(shape, device=v0.device, dtype=v0.dtype)
    w0, w1, w2 = 1 - u, u * (1 - v), u * v
    points = w0 * v0 + w1 * v1 + w2 * v2
    if face_features is None:
        return points, choices, areas
    chosen = torch.gather(face_features, 1, choices[..., None, None].repeat(1, 1, 3, face_features.shape[-1]))
    c0, c1, c2 = (t.squeeze(2) for t in torch.split(chosen, 1, dim=2))
    return points, choices, areas, w0 * c0 + w1 * c1 + w2 * c2


def run_case(name, reps):
    import torch
    from kaolin_amd.ops import mesh
    from kaolin_amd.utils import testing as T
    assert torch.cuda.is_available(), 'time_sample_points.py measures on the GPU'
    g = torch.Generator().manual_seed(0)
    if name.startswith('sphere'):
        verts, faces = T.geodesic_sphere(50)
        verts, faces = torch.as_tensor(verts).float(), torch.as_tensor(faces).long()
        B, N = 8, (100000 if name in ('sphere', 'sphere_d3') else 20000)
        D = int(name.split('_d')[1]) if '_d' in name else 0
        verts = verts[None] * (1 + 0.1 * torch.rand(B, 1, 1, generator=g))
    else:
        verts, faces = grid_mesh(709)
        verts, B, N, D = verts[None], 1, 1 << 20, 0
    V, F = verts.shape[1], faces.shape[0]
    faces = faces.cuda()
    leaf = verts.cuda().requires_grad_()
    feats = torch.randn((B, F, 3, D), generator=g).cuda().requires_grad_() if D else None
    cot_p = torch.randn((B, N, 3), generator=g).cuda()
    cot_f = torch.randn((B, N, D), generator=g).cuda() if D else None

    def hip():
        return mesh.sample_points(leaf, faces, N, face_features=feats)

    def user():
        return reference_sample_points(leaf, faces, N, feats)

    def with_backward(fn):
        def step():
            leaf.grad = None
            out = fn()
            loss = (out[0] * cot_p).sum()
            if D:
                feats.grad = None
                loss = loss + (out[-1] * cot_f).sum()
            loss.backward()
        return step

    def hip_areas():
        return mesh.face_areas(leaf.detach(), faces)

    def user_areas():
        with torch.no_grad():
            f0, f1, f2 = torch.split(faces, 1, dim=1)
            fv = [torch.index_select(leaf, 1, f.reshape(-1)) for f in (f0, f1, f2)]
            x1, x2, x3 = torch.split(fv[0] - fv[1], 1, dim=-1)
            y1, y2, y3 = torch.split(fv[1] - fv[2], 1, dim=-1)
            return (torch.sqrt((x2 * y3 - x3 * y2) ** 2 + (x3 * y1 - x1 * y3) ** 2 + (x1 * y2 - x2 * y1) ** 2) * 0.5).squeeze(-1)

    hip()                                                        # (the one host read of a new `faces`)
    a, b = hip_areas(), user_areas()
    assert torch.allclose(a, b, rtol=1e-6, atol=0), f'{name}: the areas of the two sides differ'
    equal_areas = bool(torch.equal(a, b))
    del a, b
    read_bytes = (B * V * 3 + B * N * 2) * 4 + B * N * 8 + F * 3 * 8 + B * F * 3 * D * 4
    written_bytes = B * N * 3 * 4 + B * N * 8 + B * N * D * 4
    areas_bytes = B * V * 3 * 4 + F * 3 * 8 + B * F * 4
    res = {'op': 'sample_points', 'input': name, 'reps': reps, 'B': B, 'F': F, 'V': V, 'N': N, 'D': D, 'areas_equal_bits': equal_areas,
           'lanes_from_env': os.environ.get('KAMD_SP_LANES_FROM') if os.environ.get('KAMD_LIB_PATH') else None}
    for key, fn in (('fwd', hip), ('user_fwd', user), ('fwd_bwd', with_backward(hip)), ('user_fwd_bwd', with_backward(user)),
                    ('areas', hip_areas), ('user_areas', user_areas)):
        fn()
        torch.cuda.synchronize()
        res[f'{key}_ms'] = median_ms(fn, reps)
        res[f'launches_{key}'] = count_launches(fn)
        res[f'host_reads_{key}'] = count_host_reads(fn)
    res.update(user_over_hip_fwd=round(res['user_fwd_ms'] / res['fwd_ms'], 2),
               user_over_hip_fwd_bwd=round(res['user_fwd_bwd_ms'] / res['fwd_bwd_ms'], 2),
               user_over_hip_areas=round(res['user_areas_ms'] / res['areas_ms'], 2),
               compulsory_bytes_fwd=read_bytes + written_bytes,
               bound_share_fwd=float(f'{(read_bytes + written_bytes) / HBM_BYTES_PER_S / (res["fwd_ms"] * 1e-3):.3g}'),
               bound_share_areas=float(f'{areas_bytes / HBM_BYTES_PER_S / (res["areas_ms"] * 1e-3):.3g}'))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--case', type=int, default=None, help='(internal) run one case in this process')
    ap.add_argument('--only', default=None, help='comma-separated case names (default: all)')
    args = ap.parse_args()
    if args.case is not None:
        print(json.dumps(run_case(CASES[args.case], max(args.reps, 5))), flush=True)
        return 0
    lines, status = [], 0
    for k in range(len(CASES)):
        if args.only and CASES[k] not in args.only.split(','):
            continue
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', str(k), '--reps', str(args.reps)],
                                 stdout=subprocess.PIPE, text=True, timeout=CASE_TIME_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f'case {CASES[k]} exceeded its {CASE_TIME_LIMIT_S} s limit: stopping', file=sys.stderr)
            status = 1
            break
        if res.returncode != 0 or not res.stdout.strip():
            print(f'case {CASES[k]} ended with status {res.returncode}: stopping', file=sys.stderr)
            status = 1
            break
        line = res.stdout.strip().splitlines()[-1]
        print(line, flush=True)
        lines.append(line)
    if args.out and lines:          # what was measured before a failure is kept
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return status


if __name__ == '__main__':
    sys.exit(main())
