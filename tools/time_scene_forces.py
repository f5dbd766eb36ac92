"""Times kaolin_amd.physics.reduced_scene_terms (csrc/scene_forces.hip) on one GPU against the package's torch definition on the same
GPU tensors, one JSON line per scene.

    python tools/time_scene_forces.py [--out profiles/scene_forces_time.jsonl]

Scenes: N uniformly sampled points of the unit cube, H handles with softmax weights, small random transforms, all four terms:
gravity, a floor at y = 0.5 under half of the points, N / 100 pins on random points, inertia; (N, H) in {10^4, 10^5} x {8, 32}.
Timed, each as the whole call between two device events after a warm-up, the median, smallest and largest of REPS repetitions, HIP
and torch alternating: reduced_scene_terms with and without K.  The torch side is _reduced_scene_definition (the dense B of 3 N x
12 H floats, B^T diag(d) B).  Before timing the results are compared: max difference over the largest entry, of K with it and of
g without.  `mfma_share` = 6 (4 H)^2 (N + P) useful flop (the three full blocks, as the definition forms them; the kernel computes
the lower half) over the median over 157 Tflop/s, the float32 matrix peak."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCENES = [(N, H) for N in (10 ** 4, 10 ** 5) for H in (8, 32)]
REPS = 7


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
    from kaolin_amd.physics import Boundary, Floor, Gravity, reduced_scene_terms, scene_forces
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_scene_forces.py measures on the GPU'
    lines = []
    for N, H in SCENES:
        torch.manual_seed(N + H)
        rand = lambda *shape: torch.rand(*shape, device='cuda')
        pts, w, z = rand(N, 3), torch.softmax(2 * rand(N, H), dim=1), 0.1 * (rand(H, 3, 4) - 0.5)
        rho, vol, P, dt = 900 + 200 * rand(N), (0.5 + rand(N)) / N, N // 100, 0.01
        pins = Boundary(vol)
        idx = torch.randint(0, N, (P,), device='cuda')
        pins.set_pinned(idx, pts[idx] + 0.1 * (rand(P, 3) - 0.5))
        forces = [(Gravity((1.0, 9.81, 0.5), rho, vol), 0.7), (Floor(0.5, 1, False, vol), 300.0), (pins, 50.0)]
        inertia = (rho * vol, z - 0.02 * rand(H, 3, 4), 0.1 * (rand(H, 3, 4) - 0.5), dt)
        parsed = scene_forces._scene_arguments(z, pts, w, forces, inertia)
        res = {'op': 'scene_forces', 'N': N, 'H': H, 'P': P}
        for name, hess in (('reduced', True), ('reduced_noK', False)):
            hip = lambda: reduced_scene_terms(z, pts, w, forces, inertia=inertia, pe_scale=dt * dt, hessian=hess)
            definition = lambda: scene_forces._reduced_scene_definition(*parsed, dt * dt, hess)
            a, b = hip(), definition()                              # (the warm-up)
            a, b = (a[2], b[2]) if hess else (a[1], b[1])
            res[f'{name}_diff'] = ((a - b).abs().max() / b.abs().max()).item()
            del a, b
            res.update(timed(torch, {f'{name}_hip': hip, f'{name}_torch': definition}, REPS))
        res['mfma_share'] = round(6 * (4 * H) ** 2 * (N + P) / (res['reduced_hip_ms'] * 1e-3) / 157e12, 4)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
