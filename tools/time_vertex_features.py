"""Times ops.mesh.average_face_vertex_features (the HIP gather of csrc/vertex_features.hip) on one GPU: one JSON line per case.

    python tools/time_vertex_features.py [--reps 7] [--out profiles/vertex_features_time.jsonl]

Shapes (seeded, float32): the bench sphere (geodesic, 50 000 faces) with B = 8, N = 3 and one feature row per face expanded over the
corners with stride 0 (how compute_vertex_normals is called); the same sphere with N = 32, materialised; a 709 x 709 grid mesh
(1 005 362 faces) with B = 1, N = 3, materialised; the long run: F = 2^18 faces whose every corner is vertex 0 of V = 2, B = 1,
N = 3.  Every case runs in a child process of its own under a time limit; the first failure ends the run.

Per case, the median over the repetitions of the whole public call between two device events, after a warm-up:
`cold_ms` (the topology cache cleared before every call: the build of the corner lists and its host read included), `warm_ms` (the
forward with the cache warm), `warm_fwd_bwd_ms` (forward + backward with the cache warm); `user_ms` / `user_fwd_bwd_ms` = the same
for WHAT A USER WRITES WITHOUT THIS FUNCTION: the reference's expression, scatter_add_ per corner slot and one division, in torch on
the same GPU tensors.  Before timing the results are compared (the yardstick's atomics fix no order: rtol 1e-4; the HIP result twice:
equal bits).  `launches` and `host_reads` are counted from the launch sequence of csrc/vertex_features.hip and its shim.
`bound_share` = the time the compulsory traffic (every feature read once, the result written once) takes at 6.3 TB/s, over
warm_ms."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ['sphere_n3_expanded', 'sphere_n32', 'grid_1m', 'long_run']
CASE_TIME_LIMIT_S = 150
HBM_BYTES_PER_S = 6.3e12


def median_ms(fn, reps, before=None):
    import torch
    times = []
    for _ in range(reps):
        if before is not None:
            before()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return round(statistics.median(times), 4), round(min(times), 4)


def grid_faces(cells):
    import numpy as np
    import torch
    i, j = np.meshgrid(np.arange(cells), np.arange(cells), indexing='ij')
    a = i * (cells + 1) + j
    b, c, d = a + cells + 1, a + cells + 2, a + 1
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    return torch.from_numpy(faces), (cells + 1) ** 2


def run_case(name, reps):
    import torch
    from kaolin_amd.ops import mesh
    from kaolin_amd.ops.mesh import vertex_features as vf
    from kaolin_amd.utils import testing as T
    assert torch.cuda.is_available(), 'time_vertex_features.py measures on the GPU'
    g = torch.Generator().manual_seed(0)
    if name.startswith('sphere'):
        verts, faces = T.geodesic_sphere(50)
        V, B, N = verts.shape[0], 8, (3 if name == 'sphere_n3_expanded' else 32)
    elif name == 'grid_1m':
        (faces, V), B, N = grid_faces(709), 1, 3
    else:
        faces, V, B, N = torch.zeros((1 << 18, 3), dtype=torch.long), 2, 1, 3
    F, K = faces.shape
    faces = faces.cuda()
    expanded = name == 'sphere_n3_expanded'
    leaf = torch.randn((B, F, N) if expanded else (B, F, K, N), generator=g).cuda().requires_grad_()
    cotangent = torch.randn((B, V, N), generator=g).cuda()

    def features():
        return leaf[:, :, None, :].expand(B, F, K, N) if expanded else leaf

    def hip():
        return mesh.average_face_vertex_features(faces, features(), V)

    def user():
        return vf._torch_vertex_gather(faces, features(), V, True)

    def with_backward(fn):
        def step():
            leaf.grad = None
            fn().backward(cotangent)
            return leaf.grad
        return step

    a, b = hip().detach(), user().detach()
    assert torch.equal(a, hip().detach()), f'{name}: two HIP calls differ'
    assert torch.allclose(a, b, rtol=1e-4, atol=1e-4 * float(b.abs().max())), f'{name}: the yardstick differs from the HIP path'
    ga, gb = with_backward(hip)().clone(), with_backward(user)().clone()
    assert torch.allclose(ga, gb, rtol=1e-4, atol=1e-9), f'{name}: the yardstick\'s gradient differs from the HIP path\'s'
    del a, b, ga, gb
    torch.cuda.synchronize()
    passes = (max(V - 1, 0).bit_length() + 7) // 8
    traffic = (leaf.numel() + B * V * N) * 4
    res = {'op': 'average_face_vertex_features', 'input': name, 'reps': reps, 'B': B, 'F': F, 'K': K, 'V': V, 'N': N,
           'expanded_over_corners': expanded, 'launches_cold': 2 + (4 * passes if passes else 1) + 1 + 1, 'host_reads_cold': 1,
           'launches_warm': 1, 'host_reads_warm': 0, 'launches_warm_backward': 1}
    res['cold_ms'], res['cold_min_ms'] = median_ms(hip, reps, before=vf._clear_vertex_corners_cache)
    hip()
    for key, fn in (('warm', hip), ('user', user), ('warm_fwd_bwd', with_backward(hip)), ('user_fwd_bwd', with_backward(user))):
        fn()
        torch.cuda.synchronize()
        res[f'{key}_ms'], res[f'{key}_min_ms'] = median_ms(fn, reps)
    res.update(user_over_warm=round(res['user_ms'] / res['warm_ms'], 2),
               user_over_warm_fwd_bwd=round(res['user_fwd_bwd_ms'] / res['warm_fwd_bwd_ms'], 2), compulsory_bytes=traffic,
               bound_share=float(f'{traffic / HBM_BYTES_PER_S / (res["warm_ms"] * 1e-3):.3g}'))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--case', type=int, default=None, help='(internal) run one case in this process')
    args = ap.parse_args()
    if args.case is not None:
        print(json.dumps(run_case(CASES[args.case], max(args.reps, 5))), flush=True)
        return 0
    lines, status = [], 0
    for k in range(len(CASES)):
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
