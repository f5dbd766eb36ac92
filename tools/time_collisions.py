"""Times kaolin_amd.physics.Collision (csrc/collisions.hip) on one GPU against the package's torch formulation on the same GPU
tensors, one JSON line per scene.

    python tools/time_collisions.py [--out profiles/collisions_time.jsonl]

Scenes: two balls of N / 2 uniformly sampled points each, of radius 1 with centres 1 apart (they interpenetrate), two objects,
collision radius 0.4 of the mean point spacing (R = 1.2 spacings), N in {10^4, 10^5}, H in {8, 32} handles with softmax weights,
max_contacting_pairs = 64 N so that nothing is truncated; dx for the terms = a small random displacement after detection.
Timed, each as the whole call between two device events after a warm-up, the median, smallest and largest of REPS repetitions, HIP
and torch alternating: detect_collisions (with its host reads), energy, gradient, hessian, reduced_terms with and without K.  The
torch side is _detect_definition (all pairs in chunks: ONE repetition at N = 10^5), the vectorised terms and the dense J.
Before timing the results are compared: detection by torch.equal on the four tensors, the rest by max difference over the largest
entry.  `reduced_mfma_share` = 18 (4 H)^2 C useful flop (the nine full blocks, as the definition forms them; the kernel computes
the lower half) over the median over 157 Tflop/s, the float32 matrix peak.  `detect_launches` is counted from the pipeline: keys 1,
the cell sort 7 passes of 4 launches, count 1, scan 2, totals 1, emit 1, the key sort 2 ceil(bits(N) / 8) passes of 4, finish 1;
`detect_host_reads` 2 (the counts, and the unique object pairs)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = [(N, H) for N in (10 ** 4, 10 ** 5) for H in (8, 32)]
REPS = 7


def ball(torch, n, centre):
    p = torch.randn(n, 3, device='cuda')
    return p / p.norm(dim=1, keepdim=True) * torch.rand(n, 1, device='cuda') ** (1 / 3) + torch.tensor(centre, device='cuda')


def timed(torch, fns, reps):
    times = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1))
    return {f'{name}{k}': round(f(ts), 4) for name, ts in times.items() for k, f in (('_ms', statistics.median), ('_min_ms', min), ('_max_ms', max))}


def main():
    import torch
    from kaolin_amd.physics import Collision, collisions
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_collisions.py measures on the GPU'
    lines = []
    for N, H in SCENES:
        torch.manual_seed(N + H)
        x0 = torch.cat([ball(torch, N // 2, (0.0, 0.0, 0.0)), ball(torch, N // 2, (1.0, 0.0, 0.0))])
        dx0 = torch.zeros_like(x0)
        obj = (torch.arange(N, device='cuda') >= N // 2).int()
        static = torch.zeros_like(obj)
        radius = 0.4 * (4.18879 / (N // 2)) ** (1 / 3)
        col = Collision(dt=0.01, collision_particle_radius=radius, max_contacting_pairs=64 * N)
        R, immune = 2.0 * radius * 1.5, radius * col.ignore_self_collision_ratio
        hip_detect = lambda: col.detect_collisions(dx0, x0, obj, static)
        torch_detect = lambda: collisions._detect_definition(dx0, x0, obj, static, R, immune, 64 * N)
        hip_detect()
        found = torch_detect()
        got = (col.collision_indices_a, col.collision_indices_b, col.collision_normals, col.collision_kinematic_gaps)
        C, bits = col.num_contacts, max(1, (N - 1).bit_length())
        res = {'op': 'collisions', 'N': N, 'H': H, 'C': C, 'truncated': found[0] > 64 * N,
               'detect_equal': all(torch.equal(a, b) for a, b in zip(got, found[1:5])),
               'detect_launches': 1 + 28 + 1 + 2 + 1 + 1 + 8 * ((bits + 7) // 8) + 1, 'detect_host_reads': 2}
        res.update(timed(torch, {'detect_hip': hip_detect}, REPS))
        res.update(timed(torch, {'detect_torch': torch_detect}, REPS if N <= 10 ** 4 else 1))
        dx = 0.05 * radius * torch.randn_like(x0)
        w = torch.softmax(2 * torch.rand(N, H, device='cuda'), dim=1)
        tensors = col._contact_tensors(dx)
        offsets = lambda: collisions._contact_offsets(*tensors[:3], *tensors[4:])
        terms = lambda **kw: collisions._contact_terms(offsets(), tensors[3], tensors[5] < 0, 1.0, *col._params(), **kw)
        pairs = {
            'energy': (lambda: col.energy(dx, x0, 1.0), lambda: terms()[0].sum().reshape(1)),
            'gradient': (lambda: col.gradient(dx, x0, 1.0), lambda: terms(gradient=True)[1]),
            'hessian': (lambda: col.hessian(dx, x0, 1.0), lambda: terms(hessian=True)[2]),
            'reduced': (lambda: col.reduced_terms(dx, w, x0, 1.0), lambda: col._reduced_dense(tensors, w, x0, 1.0, True)),
            'reduced_noK': (lambda: col.reduced_terms(dx, w, x0, 1.0, hessian=False),
                            lambda: col._reduced_dense(tensors, w, x0, 1.0, False)),
        }
        for name, (hip, definition) in pairs.items():
            a, b = hip(), definition()                              # (the warm-up)
            a, b = (a, b) if torch.is_tensor(a) else (a[-1] if a[-1] is not None else a[1], b[-1] if b[-1] is not None else b[1])
            res[f'{name}_diff'] = ((a - b).abs().max() / b.abs().max()).item()
            del a, b
            res.update(timed(torch, {f'{name}_hip': hip, f'{name}_torch': definition}, REPS))
        res['active_contacts'] = int((col.gradient(dx, x0, 1.0) != 0).any(dim=1).sum())
        res['reduced_mfma_share'] = round(18 * (4 * H) ** 2 * C / (res['reduced_hip_ms'] * 1e-3) / 157e12, 4)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
