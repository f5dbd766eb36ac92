"""Times kaolin_amd.physics.solve_spd (csrc/spd_solve.hip) on one GPU against torch on the same GPU tensors, one JSON line per size.

    python tools/time_spd_solve.py [--out profiles/spd_solve_time.jsonl]

Systems: A = M M^T / (2 n) + 0.1 I with M ~ N(0, 1) of (n, 2 n), b ~ N(0, 1), float32; n = 96, 384, 1536, the reduced Hessians of
H = 8, 32, 128 handles.  Timed, each as the whole call between two device events after a warm-up, the median, smallest and largest
of REPS repetitions, the three alternating: solve_spd; torch.linalg.solve (a pivoted LU, what the reference calls); and
torch.linalg.cholesky_ex + torch.cholesky_solve.  Before timing the results are compared: max difference over the largest entry,
each against the float64 solve.  `factor_hip` and `substitute_hip` time the two C calls apart (the second is one workgroup)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [96, 384, 1536]
REPS = 15


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
    from kaolin_amd import _C
    from kaolin_amd.physics import solve_spd
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_spd_solve.py measures on the GPU'
    lines = []
    for n in SIZES:
        torch.manual_seed(n)
        M = torch.randn(n, 2 * n, device='cuda', dtype=torch.float64)
        A = (M @ M.T / (2 * n) + 0.1 * torch.eye(n, device='cuda', dtype=torch.float64)).float()
        A = A.tril() + A.tril(-1).T
        b = torch.randn(n, device='cuda')
        ref = torch.linalg.solve(A.double(), b.double())

        def cholesky():
            L, _ = torch.linalg.cholesky_ex(A)
            return torch.cholesky_solve(b[:, None], L)[:, 0]
        fns = {'hip': lambda: solve_spd(A, b)[0], 'torch_solve': lambda: torch.linalg.solve(A, b), 'torch_cholesky': cholesky}
        res = {'op': 'spd_solve', 'n': n}
        for name, fn in fns.items():                                   # (the warm-up)
            res[f'{name}_diff'] = ((fn().double() - ref).abs().max() / ref.abs().max()).item()
        res.update(timed(torch, fns, REPS))
        L, info, ws = _C.physics.spd_factor_cuda(A)
        res.update(timed(torch, {'factor_hip': lambda: _C.physics.spd_factor_cuda(A),
                                 'substitute_hip': lambda: _C.physics.spd_solve_cuda(L, b, info, ws)}, REPS))
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
