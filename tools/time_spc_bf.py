"""Times ops.gaussians.sample_points_in_volume, ops.spc.bf_recon and the densifier's final step on one GPU: one JSON line per case.

    python tools/time_spc_bf.py [--reps 5] [--out profiles/spc_bf_time.jsonl]

Inputs: `sphere20k`, the end-to-end model of tests/test_spc_bf_cpu.py (20 000 isotropic Gaussians of scale 0.01 and opacity 0.9 on
a Fibonacci sphere of radius 0.5), and `random100k`, 100 000 random small Gaussians (means uniform in [-0.9, 0.9]^3, scales uniform
in [0.5, 1.5] voxel sizes of the level, random unit quaternions, opacities uniform in [0, 1], seed 0), each at levels 6 and 8 with
the densifier's default viewpoints (seed 0) and 256 x 256 depth maps.  Every (input, level) runs in a child process of its own
under a time limit; the first failure ends the run.

Per case, the whole call between two device events, median over the repetitions:
  * `sample_points_in_volume` (jitter off): `hip_ms`, and `torch_ms` with the Bayesian-fusion operators and bf_cells replaced by
    the package's torch formulations (kaolin_amd/ops/spc/bf_torch.py: what CPU tensors run) on the same GPU tensors -- the
    voxeliser and the ray tracer stay on their HIP paths in both, so the difference is this change's kernels alone;
  * `bf_recon` alone on the frames of the dataset, ray traced beforehand (the depth maps are cloned per repetition, because
    a frame converts its map in place): `hip_ms` / `torch_ms` likewise; `*_torch_equals_hip` records whether both paths gave the
    same samples, respectively the same octree and empty (recorded, not asserted: the shape is timed either way);
  * the final step: `bf_cells_cuda` against the reference's form, the empty-aware query of all 8^level cells of a dense grid
    (`dense_ms`, HIP kernels too), with the peak memory each form allocates (`*_peak_mb`, torch's allocator).
The torch formulation is the yardstick: the parent commit has nothing to time and the reference does not run on this hardware.
`launches` and `host_reads` per frame and per fusion are DERIVED figures, not counted from the runtime: the operator calls are
counted by wrapping `_C.ops.spc` and multiplied by the LAUNCHES / READS tables below (kernel launches per operator, read off
csrc/spc_bf.hip and its shim and kept in step with them by hand, fills included; a host read is every `.item()` of bf_recon.py, every operator that
reads its output size back, and scan_octrees).  The level-10 figure of the dense form is arithmetic, not a measurement: 2^30 int16
points (6.4 GB) plus an int64 arange of 8.6 GB."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = [('sphere20k', 6), ('sphere20k', 8), ('random100k', 6), ('random100k', 8)]
CASE_TIME_LIMIT_S = 240
MIP_LEVELS = 6
# kernel launches per operator call (fills of the outputs included), and whether the call reads a size back
LAUNCHES = {'build_mip2d': MIP_LEVELS, 'oracleB': 1, 'oracleB_final': 1, 'colorsB_final': 1, 'inclusive_sum': 2, 'subdivide': 3,
            'compactify': 3, 'process_final_voxels': 1, 'compactify_nodes': 3, 'merge_empty': 1, 'bq_merge': 2}
READS = {'subdivide': 1, 'compactify': 1, 'compactify_nodes': 1}


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
    return round(statistics.median(times), 3), round(min(times), 3)


def make_inputs(name, level):
    import math
    import numpy as np
    import torch
    if name == 'sphere20k':
        n = 20000
        i = np.arange(n) + 0.5
        phi, theta = np.arccos(1 - 2 * i / n), math.pi * (1 + 5 ** 0.5) * i
        xyz = 0.5 * np.stack([np.cos(theta) * np.sin(phi), np.sin(theta) * np.sin(phi), np.cos(phi)], axis=1)
        arrays = [xyz, np.full((n, 3), 0.01), np.tile([1.0, 0.0, 0.0, 0.0], (n, 1)), np.full(n, 0.9)]
    else:
        rng, G = np.random.RandomState(0), 100000
        q = rng.normal(size=(G, 4))
        arrays = [rng.uniform(-0.9, 0.9, (G, 3)), rng.uniform(0.5, 1.5, (G, 3)) * 2.0 / (1 << level),
                  q / np.linalg.norm(q, axis=1, keepdims=True), rng.uniform(0.0, 1.0, G)]
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda() for a in arrays]


def counted(real, counts):
    def wrap(name):
        def call(*a, **kw):
            counts[name] = counts.get(name, 0) + 1
            return getattr(real, name)(*a, **kw)
        return call
    return types.SimpleNamespace(**{**vars(real), **{n: wrap(n) for n in LAUNCHES}})


def launches_and_reads(counts, items, scans):
    return (sum(LAUNCHES[k] * v for k, v in counts.items()) + 4 * scans,
            sum(READS.get(k, 0) * v for k, v in counts.items()) + items + scans)


def run_case(name, level, reps):
    import torch
    import kaolin_amd as kal
    from kaolin_amd.ops.gaussians import densifier
    from kaolin_amd.ops.spc import bf_recon as bfr
    from kaolin_amd.ops.spc import bf_torch
    from kaolin_amd.ops.spc.raytraced_spc_dataset import RayTracedSPCDataset
    assert torch.cuda.is_available(), 'time_spc_bf.py measures on the GPU'
    xyz, scales, rots, opacities = make_inputs(name, level)
    torch.manual_seed(0)
    viewpoints = densifier._generate_default_viewpoints()
    hip_ops, torch_ops = bfr._ops, (lambda t: bf_torch.ops)
    res = {'input': name, 'gaussians': xyz.size(0), 'level': level, 'views': len(viewpoints), 'reps': reps}

    def sample():
        return kal.ops.gaussians.sample_points_in_volume(xyz, scales, rots, opacities, octree_level=level, jitter=False,
                                                         viewpoints=viewpoints)
    a = sample()
    bfr._ops = torch_ops
    b = sample()
    bfr._ops = hip_ops
    res['sample_torch_equals_hip'] = bool(a.shape == b.shape and torch.equal(a, b))
    res['samples'] = a.size(0)
    res['sample_hip_ms'], res['sample_hip_min_ms'] = median_ms(sample, reps)
    bfr._ops = torch_ops
    res['sample_torch_ms'], res['sample_torch_min_ms'] = median_ms(sample, min(reps, 3))
    bfr._ops = hip_ops

    # bf_recon alone: the frames of the densifier's dataset, ray traced once
    cen = 0.5 * (xyz.min(0).values + xyz.max(0).values)
    dmax = 0.5 * (xyz.max(0).values - xyz.min(0).values).max() + 0.05
    voxels, merged = kal.ops.conversions.gs_to_voxelgrid((xyz - cen) / dmax, scales / dmax, rots, opacities, level, iso=11.345,
                                                         tol=0.125, step=10)
    gs_octree = kal.ops.spc.unbatched_points_to_octree(voxels[merged >= 0.35].contiguous(), level)
    ds = RayTracedSPCDataset(viewpoints, gs_octree)
    frames = [ds[i] for i in range(len(ds))]
    res['frames_hit'] = sum(bool(f[9]) for f in frames)

    def recon():
        fresh = [(f[0], f[1].clone()) + tuple(f[2:]) if f[9] else f for f in frames]
        return bfr.bf_recon(fresh, level, 0.0005)
    a = recon()
    bfr._ops = torch_ops
    b = recon()
    bfr._ops = hip_ops
    res['recon_torch_equals_hip'] = bool((a[0] is None and b[0] is None) or (
        a[0] is not None and b[0] is not None and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])))
    res['octree_bytes'] = 0 if a[0] is None else a[0].numel()
    res['recon_hip_ms'], res['recon_hip_min_ms'] = median_ms(recon, reps)
    bfr._ops = torch_ops
    res['recon_torch_ms'], res['recon_torch_min_ms'] = median_ms(recon, min(reps, 3))
    bfr._ops = hip_ops
    res['recon_torch_over_hip'] = round(res['recon_torch_ms'] / res['recon_hip_ms'], 2)
    res['sample_torch_over_hip'] = round(res['sample_torch_ms'] / res['sample_hip_ms'], 2)

    # launches and host reads of one frame and one fusion
    hit = [f for f in frames if f[9]]
    if len(hit) >= 2 and a[0] is not None:
        counts = {}
        bfr._ops = lambda t: counted(kal._C.ops.spc, counts)
        f0 = bfr.processFrame((hit[0][0], hit[0][1].clone()) + tuple(hit[0][2:]), level, 0.0005)
        # .item() per level, after oracleB_final and before compactify_nodes; scan_octrees: 4 launches and a read
        res['frame_launches'], res['frame_host_reads'] = launches_and_reads(counts, (level - 4) + 2, 1)
        f1 = bfr.processFrame((hit[1][0], hit[1][1].clone()) + tuple(hit[1][2:]), level, 0.0005)
        counts.clear()
        bfr.fuseBF(f0, f1)
        # .item() per level, after bq_merge, after every process_final_voxels and before compactify_nodes; morton_to_points
        res['fusion_launches'], res['fusion_host_reads'] = launches_and_reads(counts, (level - 4) + 1 + level + 1, 1)
        res['fusion_launches'] += 2 + (level - 4) + 1        # arange + morton_to_points, and the max() before each .item()
        bfr._ops = hip_ops

    # the final step: bf_cells against the dense query of all 8^level cells
    if a[0] is not None:
        octree, empty = a[0], a[1]

        def cells():
            return kal._C.ops.spc.bf_cells_cuda(octree, empty, level)

        def dense():
            _, _, exsum = kal.ops.spc.scan_octrees(octree, torch.tensor([len(octree)], dtype=torch.int))
            q = kal.ops.spc.morton_to_points(torch.arange(8 ** level, dtype=torch.long, device='cuda'))
            return q[bfr.unbatched_query(octree, empty, exsum, q, level) != -1]
        assert torch.equal(cells(), dense()), 'bf_cells_cuda differs from the dense query form'
        for key, fn in (('cells', cells), ('dense', dense)):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            res[f'{key}_peak_mb'] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 2)
            res['cells'] = out.size(0)
            del out
            res[f'{key}_ms'], res[f'{key}_min_ms'] = median_ms(fn, reps)
        res['dense_over_cells'] = round(res['dense_ms'] / res['cells_ms'], 2)
        res['cells_launches'], res['cells_host_reads'] = level + 4, 1
    res['dense_level10_gb_arithmetic'] = round((2 ** 30 * 6 + 2 ** 30 * 8) / 1e9, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
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
