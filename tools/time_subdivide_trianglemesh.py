"""Times kaolin.ops.mesh.subdivide_trianglemesh on one GPU: one JSON line per (run, batch, path, mode).

    python tools/time_subdivide_trianglemesh.py [--reps 20] [--out profiles/subdivide_trianglemesh_time.jsonl]

Mesh: an icosphere, the icosahedron subdivided (topology from the package's torch formulation on the CPU; positions pushed to the
unit sphere).  Runs: `large` = 1 iteration from F = 327 680 (the icosahedron subdivided 7 times), `chain` = 3 iterations from
F = 20 480 (5 times).  float32, B = 1 and 8, alpha given.  Paths: `hip` = the public call (csrc/subdivide_trianglemesh.hip) and
`torch` = the package's torch formulation (ops/mesh/trianglemesh.py::_torch_iteration) on the same device -- the stand-in for what
the reference's chain of torch kernels costs on a GPU (the reference itself is not available where this runs, and takes B = 1
only).  Modes: `forward` (no autograd graph) and `forward_backward` (vertices and alpha require grad; the sum of the new vertices
is back-propagated).
Every case runs in a child process of its own under a time limit; the first failure ends the run.

Per case: `median_ms` / `min_ms` of `reps` calls after 3 warm-up calls (device events around the call; both paths synchronise
inside it, once per iteration, to read the number of edges).  `bound_ms` = the bytes the forward cannot avoid, summed over the
iterations -- one read of `faces` (24 per face), one write of the new faces (96 per face), and B (V + E) 4 elements read and
written -- over the achievable HBM bandwidth of 6.3 TB/s (8 TB/s peak); `bound_over_time` = bound_ms / median_ms (a
forward_backward line is measured against the same forward bound).
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
RUNS = {'large': (7, 1), 'chain': (5, 3)}      # name -> (subdivisions of the icosahedron before the call, iterations timed)
CASES = [(run, b, path, mode) for run in ('large', 'chain') for b in (1, 8) for path in ('hip', 'torch')
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


def icosphere(level):
    import torch
    from kaolin_amd.ops.mesh import trianglemesh
    from kaolin_amd.utils.testing import geodesic_sphere
    vertices, faces = geodesic_sphere(1)
    vertices = vertices.float()[None]
    for _ in range(level):
        vertices, faces, _ = trianglemesh._torch_iteration(vertices, faces, None)
    return vertices / vertices.norm(dim=-1, keepdim=True), faces


def run_case(run, batch, path, mode, reps):
    import torch
    from kaolin_amd.ops.mesh import subdivide_trianglemesh, trianglemesh
    assert torch.cuda.is_available(), 'time_subdivide_trianglemesh.py measures on the GPU'
    level, iterations = RUNS[run]
    vertices, faces = icosphere(level)
    g = torch.Generator().manual_seed(0)
    vertices = (vertices + (torch.rand((batch,) + vertices.shape[1:], generator=g) - 0.5) * 1e-3).cuda()
    alpha = torch.rand(vertices.shape[:2], generator=g).cuda()
    faces = faces.cuda()
    grad = mode == 'forward_backward'
    if grad:
        vertices.requires_grad_(), alpha.requires_grad_()

    def call():
        if path == 'hip':
            out = subdivide_trianglemesh(vertices, faces, iterations, alpha)
        else:
            x, f, a = vertices, faces, alpha
            for _ in range(iterations):
                x, f, a = trianglemesh._torch_iteration(x, f, a)
            out = (x, f)
        if grad:
            vertices.grad = alpha.grad = None
            out[0].sum().backward()
        return out

    times = timed(call, reps)
    F, V, nbytes = faces.shape[0], vertices.shape[1], 0
    for _ in range(iterations):                       # a closed manifold: E = 3 F / 2
        E = 3 * F // 2
        nbytes += F * (24 + 96) + 2 * batch * (V + E) * 4 * vertices.element_size()
        F, V = 4 * F, V + E
    out = call()
    assert out[0].shape[1] == V and out[1].shape[0] == F
    bound = nbytes / ACHIEVABLE_BPS * 1e3
    med = statistics.median(times)
    return {'run': run, 'faces': faces.shape[0], 'vertices': vertices.shape[1], 'iterations': iterations, 'batch': batch, 'path': path,
            'mode': mode, 'reps': reps, 'median_ms': round(med, 4), 'min_ms': round(min(times), 4), 'bound_ms': round(bound, 4),
            'bound_over_time': round(bound / med, 4)}


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
