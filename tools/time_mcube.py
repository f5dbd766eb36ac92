"""Times kaolin.ops.conversions.voxelgrids_to_trianglemeshes on one GPU: one JSON line per (grid, B).

    python tools/time_mcube.py [--reps 7] [--commit TEXT] [--out profiles/mcube_time.jsonl]

Grids, float32: `sphere256` = the bench's geodesic sphere (50 000 faces) through trianglemeshes_to_voxelgrids at 256^3 and
ops.voxelgrid.fill; `rand128` = a seeded random binary 128^3 grid with p = 0.5 (about half of all lattice edges are crossed: the
worst case for the output size).  B = 1 and 8 (the same grid repeated).  Every case runs in a child process of its own under a
time limit; the first failure ends the run.

Per case, on the same GPU tensor, results compared with torch.equal before anything is timed:
  `hip_ms`    the public call on the HIP pipeline (csrc/mcube.hip),
  `torch_ms`  the package's torch formulation of the same pipeline (case bytes, cumsum, gathers: the CPU path, run on the GPU
              tensor, its zero-padded copy included).
Each is the median over the repetitions of the whole call between two device events (both synchronise to read their sizes back).
`bound_ms` = the compulsory bytes -- the grid read once, the vertices and faces written once -- over the achievable HBM bandwidth
of 6.3 TB/s (8 TB/s peak); `bound_over_hip` = bound_ms / hip_ms, the share of the byte bound the call reaches.  `commit` names
what the numbers were taken on.
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
CASES = [(g, n) for g in ('sphere256', 'rand128') for n in (1, 8)]
CASE_TIME_LIMIT_S = 240


def make_grid(name, n):
    import torch
    import kaolin_amd as kal
    if name == 'rand128':
        g = torch.Generator().manual_seed(128)
        grid = (torch.rand((1, 128, 128, 128), generator=g) < 0.5).cuda()
    else:
        from kaolin_amd.utils.testing import geodesic_sphere
        v, f = geodesic_sphere(50)
        grid = kal.ops.voxelgrid.fill(kal.ops.conversions.trianglemeshes_to_voxelgrids(v.float()[None].cuda(), f.cuda(), 256))
    return grid.float().expand(n, -1, -1, -1).contiguous()


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
    return statistics.median(times), min(times)


def run_case(name, n, reps, commit):
    import torch
    import torch.nn.functional as F
    from kaolin_amd.ops.conversions.voxelgrid import _trianglemeshes_torch, voxelgrids_to_trianglemeshes
    assert torch.cuda.is_available(), 'time_mcube.py measures on the GPU'
    x = make_grid(name, n)

    def hip():
        return voxelgrids_to_trianglemeshes(x)

    def formulation():
        verts, faces, nv, nf = _trianglemeshes_torch(F.pad(x, (1,) * 6), 0.5)
        return list(torch.split(verts, nv)), list(torch.split(faces, nf))

    out, got = hip(), formulation()
    assert len(got[0]) == n and all(torch.equal(a, b) for a, b in zip(out[0] + out[1], got[0] + got[1])), \
        'the torch formulation differs from the HIP path'
    del got
    hip()
    formulation()
    torch.cuda.synchronize()
    res = {'grid': name, 'dtype': 'float32', 'B': n, 'reps': reps, 'commit': commit}
    for key, fn in (('hip', hip), ('torch', formulation)):
        med, low = median_ms(fn, reps)
        res[f'{key}_ms'], res[f'{key}_min_ms'] = round(med, 4), round(low, 4)
    nbytes = x.numel() * x.element_size() + sum(t.numel() * t.element_size() for t in out[0] + out[1])
    bound = nbytes / ACHIEVABLE_BPS * 1e3
    res.update(bound_ms=round(bound, 4), bound_over_hip=round(bound / res['hip_ms'], 4),
               torch_over_hip=round(res['torch_ms'] / res['hip_ms'], 2), vertices=out[0][0].shape[0], faces=out[1][0].shape[0])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--commit', default='unnamed')
    ap.add_argument('--out', default=None)
    ap.add_argument('--case', type=int, default=None, help='(internal) run one case in this process')
    args = ap.parse_args()
    if args.case is not None:
        print(json.dumps(run_case(*CASES[args.case], args.reps, args.commit)), flush=True)
        return 0
    lines, status = [], 0
    for k in range(len(CASES)):
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', str(k), '--reps', str(args.reps),
                                  '--commit', args.commit], stdout=subprocess.PIPE, text=True, timeout=CASE_TIME_LIMIT_S)
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
