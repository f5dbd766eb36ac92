"""Times the operators of kaolin.ops.spc on one GPU: one JSON line per case.

    python tools/time_spc.py [--reps 20] [--out profiles/spc_time.jsonl]

The workload is the project's own: the octree of unbatched_mesh_to_spc for the bench's geodesic sphere (50 000 faces) at level 9,
alone (B = 1) and repeated (B = 8), for scan_octrees and generate_points; its last-level points, shuffled, into
unbatched_points_to_octree; 1 M float32 queries, half at occupied voxel centres and half uniform in the cube, without and with
parents; to_dense at level 7 with 4 channels.  Every case runs in a child process of its own under a time limit; the first failure
ends the run.

Per case: `hip_ms` = the median over the repetitions of the public call between two device events, `torch_ms` = the same for the
package's torch formulation of the pipeline (the CPU path, run on the same GPU tensors), after checking with torch.equal that the
two agree.  The torch formulation is the yardstick: the parent commit has nothing to time and the reference does not run on this
hardware.  `bound_ms` = the compulsory bytes (inputs read once, results written once) over the achievable HBM bandwidth of
6.3 TB/s.  `launches` and `host_reads` are counted from the launch sequence of csrc/spc.hip and its shim for the case's level and
size (allocations and the small host-to-device copies of the CPU pyramid are not launches)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_BPS = 6.3e12
LEVEL, DENSE_LEVEL, DENSE_CHANNELS, QUERIES = 9, 7, 4, 1 << 20
CASES = [('scan_octrees', 1), ('scan_octrees', 8), ('generate_points', 1), ('generate_points', 8), ('points_to_octree', 1),
         ('query', 1), ('query_with_parents', 1), ('to_dense', 1), ('to_dense', 8)]
CASE_TIME_LIMIT_S = 240


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


def same(a, b):
    import torch
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return torch.equal(a, b) if torch.is_tensor(a) else a == b


def run_case(op, B, reps):
    import torch
    import kaolin_amd as kal
    from kaolin_amd._C.ops import finish_scan
    from kaolin_amd.ops.spc import points as P, spc as S
    from kaolin_amd.utils.testing import geodesic_sphere
    assert torch.cuda.is_available(), 'time_spc.py measures on the GPU'
    v, f = geodesic_sphere(50)
    one = kal.ops.conversions.unbatched_mesh_to_spc((v.float() * 1.2)[f].contiguous().cuda(), LEVEL)[0]
    octrees = one.repeat(B)
    lens = [one.numel()] * B
    lengths = torch.tensor(lens, dtype=torch.int32)
    max_level, pyramids, exsum = S.scan_octrees(octrees, lengths)
    points = S.generate_points(octrees, pyramids, exsum)
    N, npoints, leaves = octrees.numel(), points.shape[0], int(pyramids[0, 0, LEVEL])
    res = {'op': op, 'B': B, 'level': LEVEL, 'octree_bytes': N, 'points': npoints, 'reps': reps}
    if op == 'scan_octrees':
        def hip():
            return S.scan_octrees(octrees, lengths)

        def torch_():
            full, depths, ex = S._torch_scan_octrees(octrees, lens)
            return finish_scan(op, full, depths, lens) + (ex,)
        nbytes, launches, reads = N + 4 * N, 4, 1
    elif op == 'generate_points':
        def hip():
            return S.generate_points(octrees, pyramids, exsum)

        def torch_():
            return S._torch_generate_points(octrees, pyramids)
        nbytes, launches, reads = N + 4 * N + 6 * npoints, LEVEL, 0
    elif op == 'points_to_octree':
        last = S.unbatched_get_level_points(points, pyramids[0], LEVEL)
        shuffled = last[torch.randperm(leaves, generator=torch.Generator().manual_seed(0)).cuda()].contiguous()
        res['n'] = leaves

        def hip():
            return P.unbatched_points_to_octree(shuffled, LEVEL)

        def torch_():
            return P._torch_morton_to_octree(P._torch_points_to_morton(shuffled), LEVEL)
        passes = (3 * LEVEL + 7) // 8
        # codes, mask, per sort pass a histogram, a 2-launch scan and a scatter, heads + scan + unique, per level heads + scan +
        # parents, gather
        nbytes, launches, reads = 6 * leaves + one.numel(), 2 + 4 * passes + 4 + 4 * LEVEL + 1, 1
    elif op in ('query', 'query_with_parents'):
        parents = op == 'query_with_parents'
        last = S.unbatched_get_level_points(points, pyramids[0], LEVEL)
        g = torch.Generator().manual_seed(1)
        pick = torch.randint(0, leaves, (QUERIES // 2,), generator=g).cuda()
        centres = (last[pick].float() + 0.5) / 2 ** LEVEL * 2.0 - 1.0
        coords = torch.cat([centres, (torch.rand((QUERIES // 2, 3), generator=g) * 2.0 - 1.0).cuda()]).contiguous()
        res['Q'] = QUERIES

        def hip():
            return S.unbatched_query(one, exsum[:one.numel()], coords, LEVEL, with_parents=parents)

        def torch_():
            out = S._torch_query(one, exsum[:one.numel()], coords, LEVEL, parents)
            return out if parents else out[:, LEVEL].contiguous()
        nbytes, launches, reads = 12 * QUERIES + 8 * QUERIES * (LEVEL + 1 if parents else 1) + 5 * one.numel(), 1, 0
    else:
        rows = int(pyramids[:, 0, DENSE_LEVEL].sum())
        x = torch.rand((rows, DENSE_CHANNELS), generator=torch.Generator().manual_seed(2)).cuda()
        res.update(dense_level=DENSE_LEVEL, channels=DENSE_CHANNELS, rows=rows)

        def hip():
            return S.to_dense(points, pyramids, x, DENSE_LEVEL)

        def torch_():
            return S._torch_to_dense(points, pyramids, x, DENSE_LEVEL)
        nbytes = B * DENSE_CHANNELS * (2 ** DENSE_LEVEL) ** 3 * 4 + rows * (DENSE_CHANNELS * 4 + 6)
        launches, reads = 2, 0                                  # the zero fill and the scatter
    a, b = hip(), torch_()
    assert same(a, b), f'{op}: the torch formulation differs from the HIP path'
    if op.startswith('query'):
        res['hits'] = int((a.reshape(QUERIES, -1)[:, -1] >= 0).sum())
    del a, b
    for _ in range(2):
        hip()
        torch_()
    torch.cuda.synchronize()
    for key, fn in (('hip', hip), ('torch', torch_)):
        med, low = median_ms(fn, reps)
        res[f'{key}_ms'], res[f'{key}_min_ms'] = round(med, 4), round(low, 4)
    bound = nbytes / ACHIEVABLE_BPS * 1e3
    res.update(torch_over_hip=round(res['torch_ms'] / res['hip_ms'], 2), compulsory_bytes=nbytes, bound_ms=round(bound, 5),
               bound_over_hip=round(bound / res['hip_ms'], 4), launches=launches, host_reads=reads)
    return res


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
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return status


if __name__ == '__main__':
    sys.exit(main())
