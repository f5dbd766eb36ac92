"""Times kaolin.metrics.tetmesh on one GPU: one JSON line per (operator, path, mode).

    python tools/time_tetmesh_metrics.py [--grid 128] [--reps 20] [--out profiles/tetmesh_metrics_time.jsonl]

Workload: the Kuhn grid of 128^3 cells (12.6 M tets) with jittered vertices, float32, B = 1; ``tet_vertices = vertices[:, tets]`` is
built once, outside the timed region.  Operators: `volume`, `equivolume` (pow = 4, mean computed), `amips` (inverse offset matrices
of the unjittered grid; for `forward_backward` only ``tet_vertices`` requires grad).  Paths: `hip` = the public call
(csrc/tetmesh_metrics.hip) and `torch` = the package's torch formulation (metrics/tetmesh.py::_torch_*) on the same device -- the
stand-in for what the reference's chain of torch kernels costs on a GPU (the reference itself is not available where this runs).
Modes: `forward` (no autograd graph) and `forward_backward` (the sum of the result is back-propagated).
Every case runs in a child process of its own under a time limit; the first failure ends the run.

Per case: `median_ms` / `min_ms` of `reps` calls after 3 warm-up calls (device events around the call).  `bound_ms` = the bytes the
call cannot avoid over the achievable HBM bandwidth of 6.3 TB/s (8 TB/s peak), per tet: volume forward 52 (48 read, 4 written),
backward 100 (48 + 4 read, 48 written); equivolume reads the tets once per pass (48, and 96 backward: two passes plus the write,
its mean adds a volume forward and backward: 52 + 100); amips forward 84 (48 + 36), backward 132 (84 read, 48 written).  A
forward_backward line is measured against forward + backward bytes.  `bound_over_time` = bound_ms / median_ms.  Each line carries
the commit it was measured at and its parent.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_BPS = 6.3e12
# bytes per tet, float32: (forward, backward)
BYTES = {'volume': (52, 100), 'equivolume': (48 + 52, 96 + 100), 'amips': (84, 132)}
CASES = [(op, path, mode) for op in ('volume', 'equivolume', 'amips') for path in ('hip', 'torch')
         for mode in ('forward', 'forward_backward')]
CASE_TIME_LIMIT_S = 150


def timed(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    return times


def run_case(op, path, mode, grid, reps):
    import torch
    from kaolin_amd.metrics import tetmesh
    from kaolin_amd.ops.mesh import inverse_vertices_offset
    from kaolin_amd.utils.testing import kuhn_grid
    assert torch.cuda.is_available(), 'time_tetmesh_metrics.py measures on the GPU'
    rest, tets = kuhn_grid(grid)
    g = torch.Generator().manual_seed(1)
    vertices = (rest + (torch.rand(rest.shape, generator=g) - 0.5) * (0.2 / grid))[None].cuda()
    tets = tets.cuda()
    tv = vertices[:, tets].contiguous()
    inv = inverse_vertices_offset(rest[None].cuda()[:, tets]).contiguous() if op == 'amips' else None
    del vertices
    grad = mode == 'forward_backward'
    tv.requires_grad_(grad)
    fn = {('volume', 'hip'): lambda: tetmesh.tetrahedron_volume(tv), ('volume', 'torch'): lambda: tetmesh._torch_volume(tv),
          ('equivolume', 'hip'): lambda: tetmesh.equivolume(tv, pow=4),
          ('equivolume', 'torch'): lambda: tetmesh._torch_equivolume(tv, None, 4),
          ('amips', 'hip'): lambda: tetmesh.amips(tv, inv), ('amips', 'torch'): lambda: tetmesh._torch_amips(tv, inv)}[(op, path)]

    def call():
        out = fn()
        if grad:
            tv.grad = None
            out.sum().backward()
        return out

    times = timed(call, reps)
    T = tets.shape[0]
    per_tet = BYTES[op][0] + (BYTES[op][1] if grad else 0)
    bound = T * per_tet / ACHIEVABLE_BPS * 1e3
    med = statistics.median(times)
    return {'operator': op, 'grid': grid, 'tets': T, 'dtype': 'float32', 'path': path, 'mode': mode, 'reps': reps,
            'median_ms': round(med, 4), 'min_ms': round(min(times), 4), 'bytes_per_tet': per_tet, 'bound_ms': round(bound, 4),
            'bound_over_time': round(bound / med, 4)}


def git(*args):
    try:
        return subprocess.run(('git',) + args, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    except OSError:
        return ''


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, default=128)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--commit', default=None, help='recorded with every line (default: git rev-parse HEAD)')
    ap.add_argument('--parent', default=None)
    ap.add_argument('--case', type=int, default=None, help='(internal) run one case in this process')
    args = ap.parse_args()
    if args.case is not None:
        print(json.dumps(run_case(*CASES[args.case], args.grid, args.reps)), flush=True)
        return 0
    stamp = {'commit': args.commit or git('rev-parse', 'HEAD') or None, 'parent': args.parent or git('rev-parse', 'HEAD^') or None}
    lines, status = [], 0
    for k in range(len(CASES)):
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', str(k), '--grid', str(args.grid), '--reps',
                                  str(args.reps)], stdout=subprocess.PIPE, text=True, timeout=CASE_TIME_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f'case {CASES[k]} exceeded its {CASE_TIME_LIMIT_S} s limit: stopping', file=sys.stderr)
            status = 1
            break
        if res.returncode != 0 or not res.stdout.strip():
            print(f'case {CASES[k]} ended with status {res.returncode}: stopping', file=sys.stderr)
            status = 1
            break
        line = json.dumps({**json.loads(res.stdout.strip().splitlines()[-1]), **stamp})
        print(line, flush=True)
        lines.append(line)
    if args.out and lines:          # what was measured before a failure is kept
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return status


if __name__ == '__main__':
    sys.exit(main())
