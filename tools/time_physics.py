"""Times physics.simplicits.reduced_neohookean_terms (csrc/physics.hip) against its torch definition on one GPU: one JSON line per size.

    python tools/time_physics.py [--reps 20] [--out profiles/physics_time.jsonl]

Sizes (N, H): (10^4, 8), (10^5, 8), (10^4, 32), (10^5, 32); seeded inputs as in tests/test_physics_cpu.py, float32.  Paths: `hip` =
the fused kernel and its finishing launch, `hip_no_hessian` = the same without K, `definition` = dense dFdz_matrix, the (N, 9, 9)
blocks, bmm and matmul on the same GPU tensors (what the reference's hess_reduction does after its Warp kernels).  Before timing,
K and g of both paths are compared (max difference over the largest entry) and the figure goes into the line.

Per path: the median, smallest and largest repetition of the whole call between two device events after a warm-up; the
repetitions of the paths alternate.  `hip_mac_per_s` = the 6 W^2 3 N multiply-adds of the six computed K blocks (W = 4 H) over the
median: a whole-call rate, not a kernel's share of peak."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(10 ** 4, 8), (10 ** 5, 8), (10 ** 4, 32), (10 ** 5, 32)]
ARGS = ('z', 'pts', 'weights', 'weights_jac', 'mu', 'lam', 'vol')


def main():
    import torch
    from kaolin_amd.physics import simplicits
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_physics.py measures on the GPU'
    lines = []
    for N, H in SIZES:
        gen = torch.Generator().manual_seed(N + H)
        r = lambda *shape: torch.randn(*shape, generator=gen)
        d = dict(z=0.1 * r(H, 3, 4), pts=2 * torch.rand(N, 3, generator=gen) - 1, weights=torch.softmax(r(N, H), dim=1),
                 weights_jac=0.5 * r(N, H, 3), mu=1 + r(N).abs(), lam=2 + 3 * r(N).abs(), vol=0.1 + 0.05 * r(N).abs())
        d = {k: v.cuda() for k, v in d.items()}
        paths = {'hip': lambda: simplicits.reduced_neohookean_terms(coeff=0.7, **d),
                 'hip_no_hessian': lambda: simplicits.reduced_neohookean_terms(coeff=0.7, hessian=False, **d),
                 'definition': lambda: simplicits._reduced_definition(*(d[k] for k in ARGS), 0.7, True)}
        results = {name: fn() for name, fn in paths.items()}       # (the warm-up)
        torch.cuda.synchronize()
        diff = [((a - b).abs().max() / b.abs().max()).item() for a, b in zip(results['hip'][1:], results['definition'][1:])]
        times = {name: [] for name in paths}
        for _ in range(args.reps):
            for name, fn in paths.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                torch.cuda.synchronize()
                times[name].append(t0.elapsed_time(t1))
        res = {'op': 'reduced_neohookean_terms', 'N': N, 'H': H, 'g_diff': diff[0], 'K_diff': diff[1]}
        for name, ts in times.items():
            res.update({f'{name}_ms': round(statistics.median(ts), 4), f'{name}_min_ms': round(min(ts), 4),
                        f'{name}_max_ms': round(max(ts), 4)})
        res['hip_mac_per_s'] = round(6 * (4 * H) ** 2 * 3 * N / (res['hip_ms'] * 1e-3))
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
