"""Times kaolin.ops.mesh.subdivide_tetmesh on one GPU: one JSON line per (grid, features, path, mode).

    python tools/time_subdivide_tetmesh.py [--reps 20] [--out profiles/subdivide_tetmesh_time.jsonl]

Grids: the Kuhn grids of 64^3 and 128^3 cells (1.6 M / 12.6 M tets, 0.27 M / 2.1 M vertices), float32, B = 1, without features
and with D = 1 (an sdf).  Paths: `hip` = the public call (csrc/subdivide_tetmesh.hip) and `torch` = the package's torch
formulation (ops/mesh/tetmesh.py::_torch_subdivide) on the same device -- the stand-in for what the reference's chain of torch
kernels costs on a GPU (the reference itself is not available where this runs).  Modes: `forward` (no autograd graph) and
`forward_backward` (inputs require grad; the sum of the float outputs is back-propagated).
Every case runs in a child process of its own under a time limit; the first failure ends the run.

Per case: `median_ms` / `min_ms` of `reps` calls after 3 warm-up calls (device events around the call; both paths synchronise
inside it to read the number of edges).  `bound_ms` = the bytes the forward cannot avoid -- one read of `tets` (32 per tet), one
write of new_tets (256 per tet), and (V + E)(3 + D) elements read and written -- over the achievable HBM bandwidth of 6.3 TB/s
(8 TB/s peak); `bound_over_time` = bound_ms / median_ms, the fraction of that byte bound the whole call reaches (a
forward_backward line is measured against the same forward bound).  The `hip` / `forward` lines also carry `range_check_ms`: the
median of the shim's index-range check alone (a torch min / max pass over `tets` and a host read), which is part of every call.
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
CASES = [(n, d, path, mode) for n in (64, 128) for d in (0, 1) for path in ('hip', 'torch')
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


def run_case(n, d, path, mode, reps):
    import torch
    from kaolin_amd import _C
    from kaolin_amd.ops.mesh import subdivide_tetmesh, tetmesh
    from kaolin_amd.utils.testing import kuhn_grid
    assert torch.cuda.is_available(), 'time_subdivide_tetmesh.py measures on the GPU'
    vertices, tets = kuhn_grid(n)
    sdf = 0.37 - (vertices - torch.tensor([0.48, 0.53, 0.5])).norm(dim=-1)
    vertices, tets = vertices[None].cuda(), tets.cuda()
    features = sdf[None, :, None].cuda() if d else None
    grad = mode == 'forward_backward'
    if grad:
        vertices.requires_grad_()
        if d:
            features.requires_grad_()

    def call():
        out = subdivide_tetmesh(vertices, tets, features) if path == 'hip' else tetmesh._torch_subdivide(vertices, tets, features)
        if grad:
            vertices.grad = None
            if d:
                features.grad = None
            (out[0].sum() + out[2].sum() if d else out[0].sum()).backward()
        return out

    times = timed(call, reps)
    out = call()
    T, V, rows = tets.shape[0], vertices.shape[1], out[0].shape[1]
    bound = (T * (32 + 256) + 2 * rows * (3 + d) * vertices.element_size()) / ACHIEVABLE_BPS * 1e3
    med = statistics.median(times)
    line = {'grid': n, 'tets': T, 'vertices': V, 'edges': rows - V, 'features': d, 'path': path, 'mode': mode, 'reps': reps,
            'median_ms': round(med, 4), 'min_ms': round(min(times), 4), 'bound_ms': round(bound, 4),
            'bound_over_time': round(bound / med, 4)}
    if path == 'hip' and not grad:
        check = timed(lambda: _C.ops.check_tets_in_range(tets, V), reps)
        line['range_check_ms'] = round(statistics.median(check), 4)
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--case', type=int, default=None, help='(internal) run one case in this process')
    args = ap.parse_args()
    if args.case is not None:
        print(json.dumps(run_case(*CASES[args.case], args.reps)), flush=True)
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
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return status


if __name__ == '__main__':
    sys.exit(main())
