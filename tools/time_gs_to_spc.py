"""Times ops.conversions.gs_to_voxelgrid and its two operators on one GPU: one JSON line per case.

    python tools/time_gs_to_spc.py [--reps 7] [--out profiles/gs_to_spc_time.jsonl]

Inputs: the reference's 8 Gaussians (tests/golden/gs_to_voxelgrid.npz) at level 7, and 100 000 random small Gaussians at levels 7
and 8: means uniform in [-0.9, 0.9]^3, scales uniform in [0.5, 1.5] voxel sizes of the level, random unit quaternions, opacities
uniform in [0, 1] (seed 0).  For each input three operators: `gs_to_spc_cuda`, `integrate_gs_cuda` (on the pairs of the first) and
the whole `gs_to_voxelgrid`.  Every case runs in a child process of its own under a time limit; the first failure ends the run.

Per case: `hip_ms` = the median over the repetitions of the call between two device events, `torch_ms` = the same for the package's
torch formulation (kaolin_amd/ops/conversions/gaussians.py: what CPU tensors run) on the same GPU tensors, after checking that the
integer results are equal and the float ones within a float32 ulp of each other's neighbourhood (2 ulp).  The torch formulation is
the yardstick: the parent commit has nothing to time and the reference does not run on this hardware.  `launches` and `host_reads`
are counted from the launch sequence of csrc/gs_to_spc.hip and its shim for the case's level.  `exp_per_s` (integrate_gs only) =
pairs * step^3 / hip time."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ISO, TOL, STEP = 11.345, 1. / 8., 10
INPUTS = [('reference8', 7), ('random100k', 7), ('random100k', 8)]
OPS = ['gs_to_spc_cuda', 'integrate_gs_cuda', 'gs_to_voxelgrid']
CASES = [(name, level, op) for name, level in INPUTS for op in OPS]
CASE_TIME_LIMIT_S = 150


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


def make_inputs(name, level):
    import numpy as np
    import torch
    if name == 'reference8':
        g = np.load(os.path.join(ROOT, 'tests', 'golden', 'gs_to_voxelgrid.npz'))
        arrays = [g['xyz'], g['scales'], g['rots'], g['opacities'].reshape(-1)]
    else:
        rng, G = np.random.RandomState(0), 100000
        q = rng.normal(size=(G, 4))
        arrays = [rng.uniform(-0.9, 0.9, (G, 3)), rng.uniform(0.5, 1.5, (G, 3)) * 2.0 / (1 << level),
                  q / np.linalg.norm(q, axis=1, keepdims=True), rng.uniform(0.0, 1.0, G)]
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in arrays]


def close(a, b):
    """within 2 float32 ulp (each path is within one ulp of the exact value)"""
    import torch
    return bool(((a.double() - b.double()).abs() <= 2.0 ** -22 * b.double().abs() + 2.0 ** -148).all())


def run_case(name, level, op, reps):
    import torch
    import kaolin_amd as kal
    from kaolin_amd.ops.conversions import gaussians as G
    from kaolin_amd.render.spc import raytrace as R
    assert torch.cuda.is_available(), 'time_gs_to_spc.py measures on the GPU'
    C = kal._C.ops.conversions
    xyz, scales, rots, opacities = make_inputs(name, level)
    points, gid, boundary, cov = C.gs_to_spc_cuda(xyz, scales, rots, ISO, TOL, level)
    pairs, voxels = points.size(0), int(boundary.sum())
    stages, passes = max(1, -(-level // 3)), (3 * level + 7) // 8
    res = {'op': op, 'input': name, 'gaussians': xyz.size(0), 'level': level, 'pairs': pairs, 'voxels': voxels, 'reps': reps}
    if op == 'gs_to_spc_cuda':
        def hip():
            return C.gs_to_spc_cuda(xyz, scales, rots, ISO, TOL, level)

        def torch_():
            return G.gs_to_spc_torch(xyz, scales, rots, ISO, TOL, level)

        def same(a, b):
            return all(torch.equal(x, y) for x, y in zip(a, b))
        # prepare; per stage count + the scan's two + emit; per sort pass histogram + the scan's two + scatter; heads, points
        launches, reads = 1 + 4 * stages + 4 * max(passes, 1) + 2, stages
    elif op == 'integrate_gs_cuda':
        def hip():
            return C.integrate_gs_cuda(points, gid, xyz, cov, opacities, level, STEP)

        def torch_():
            return G.integrate_gs_torch(points, gid, xyz, cov, opacities, level, STEP)
        same, launches, reads = close, 1, 0
    else:
        def hip():
            return kal.ops.conversions.gs_to_voxelgrid(xyz, scales, rots, opacities, level, ISO, TOL, STEP)

        def torch_():
            p, i, b, c = G.gs_to_spc_torch(xyz, scales, rots, ISO, TOL, level)
            integral = G.integrate_gs_torch(p, i, xyz, c, opacities, level, STEP)
            merged = 1. - R._torch_pack_reduce((1. - integral).unsqueeze(-1), b, True).squeeze(-1)
            return p[b], merged

        def same(a, b):
            return torch.equal(a[0], b[0]) and bool(((a[1] - b[1]).abs() <= 1e-5).all())
        # the two operators, the elementwise 1 - x twice, prod_reduce (boundaries to int, inclusive sum, fill, reduce), the mask
        launches, reads = None, stages + 2
    a, b = hip(), torch_()
    assert same(a, b), f'{op}: the torch formulation differs from the HIP path'
    del a, b
    hip()
    torch.cuda.synchronize()
    torch_reps = reps if name == 'reference8' else min(reps, 3)
    for key, fn, n in (('hip', hip, reps), ('torch', torch_, torch_reps)):
        med, low = median_ms(fn, n)
        res[f'{key}_ms'], res[f'{key}_min_ms'] = round(med, 4), round(low, 4)
    res.update(torch_reps=torch_reps, torch_over_hip=round(res['torch_ms'] / res['hip_ms'], 2), launches=launches, host_reads=reads)
    if op == 'integrate_gs_cuda':
        res['exp_per_s'] = float(f'{pairs * STEP ** 3 / (res["hip_ms"] * 1e-3):.4g}')
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
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
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return status


if __name__ == '__main__':
    sys.exit(main())
