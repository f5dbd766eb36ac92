"""Times the SPC feature-grid operators of kaolin.ops.spc on one GPU: one JSON line per case.

    python tools/time_spc_trilinear.py [--reps 20] [--out profiles/spc_trilinear_time.jsonl]

The workload is the project's own: the octree of unbatched_mesh_to_spc for the bench's geodesic sphere (50 000 faces) at level 9;
its dual and its trinkets; and 2^20 coordinates inside occupied leaves (S = 1) interpolated from D = 16 features per corner of the
last level: forward in float32 and half, the gradient by the features and the gradient by the coordinates in float32.  Every case
runs in a child process of its own under a time limit; the first failure ends the run.

Per case: `hip_ms` = the median over the repetitions of the call between two device events, `torch_ms` = the same for the package's
torch formulation (the CPU path, run on the same GPU tensors), after checking that the two agree: torch.equal for the integer
results and the float32 forward; for half and the gradients the bounds of tests/test_spc_dual_cpu.py against the formulation in
float64 (forward 64 * 2^-24 max_k |f_k| + the half rounding; grad_feats (K + 8) 2^-24 sum |g|; grad_coords (D + 48) 2^-24 sum_d
|g_d| max_k |f_kd|).  The torch formulation is the yardstick: the parent commit has nothing to time and the reference does not run
on this hardware.  `bound_ms` = the compulsory bytes (inputs read once, results written once) over the achievable HBM bandwidth
of 6.3 TB/s; for the gradient by the features plus the added bytes over 1.3 TB/s, the APPROXIMATE chip-wide float-atomic rate measured elsewhere for 256-byte
and 128-byte segments (this kernel adds 64-byte segments): an estimate, not a floor, so `bound_over_hip` may exceed 1 there.
`launches_by_construction` and `host_reads_by_construction` are NOT measured: they are worked out here from the launch sequence of
csrc/spc_trilinear.hip and its shim for the case's depth, and have to follow that code when it changes."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_BPS = 6.3e12
ATOMIC_BPS = 1.3e12
LEVEL, SAMPLES, D = 9, 1 << 20, 16
CASES = ['make_dual', 'make_trinkets', 'interpolate_forward_f32', 'interpolate_forward_f16', 'interpolate_backward_feats',
         'interpolate_backward_coords']
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
    return torch.equal(a, b)


def run_case(op, reps):
    import torch
    import kaolin_amd as kal
    from kaolin_amd import _C
    from kaolin_amd.ops.spc import points as P, spc as S
    from kaolin_amd.utils.testing import geodesic_sphere
    assert torch.cuda.is_available(), 'time_spc_trilinear.py measures on the GPU'
    v, f = geodesic_sphere(50)
    octree = kal.ops.conversions.unbatched_mesh_to_spc((v.float() * 1.2)[f].contiguous().cuda(), LEVEL)[0]
    _, pyramids, exsum = S.scan_octrees(octree, torch.tensor([octree.numel()], dtype=torch.int32))
    pyramid = pyramids[0].contiguous()
    points = S.generate_points(octree, pyramids, exsum)
    dual, pyramid_dual = S.unbatched_make_dual(points, pyramid)
    trinkets, parents = S.unbatched_make_trinkets(points, pyramid, dual, pyramid_dual)
    n, nd, leaves, nf = points.shape[0], dual.shape[0], int(pyramid[0, LEVEL]), int(pyramid_dual[0, LEVEL])
    res = {'op': op, 'level': LEVEL, 'points': n, 'dual_points': nd, 'reps': reps}
    agree = same
    if op == 'make_dual':
        def hip():
            return S.unbatched_make_dual(points, pyramid)

        def torch_():
            return S._torch_make_dual(points, pyramid)
        passes = (3 * (LEVEL + 1) + 7) // 8 + 1
        # keys, per sort pass a histogram, a 2-launch scan and a scatter, heads + scan, the level starts, decode
        nbytes, launches, reads = 6 * n + 6 * nd, 1 + 4 * passes + 3 + 1 + 1, 1
    elif op == 'make_trinkets':
        def hip():
            return S.unbatched_make_trinkets(points, pyramid, dual, pyramid_dual)

        def torch_():
            return S._torch_make_trinkets(points, pyramid, dual, pyramid_dual)
        nbytes, launches, reads = 6 * n + 6 * nd + 36 * n, 1, 0
    else:
        half = op.endswith('f16')
        g = torch.Generator().manual_seed(1)
        first = int(pyramid[1, LEVEL])
        pick = torch.randint(0, leaves, (SAMPLES,), generator=g).cuda()
        pidx = (first + pick).int()
        inside = (points[first + pick].float() + torch.rand((SAMPLES, 3), generator=g).cuda()) / 2 ** LEVEL * 2.0 - 1.0
        coords = inside[:, None, :].contiguous()
        feats = (torch.rand((nf, D), generator=g) * 2.0 - 1.0).cuda()
        grad_out = (torch.rand((SAMPLES, 1, D), generator=g) * 2.0 - 1.0).cuda()
        if half:
            feats = feats.half()
        size = 2 if half else 4
        args = (coords, pidx, points, trinkets, feats, LEVEL)
        args64 = (coords.double(), pidx, points, trinkets, feats.double(), LEVEL)
        res.update(samples=SAMPLES, S=1, D=D, num_feats=nf, dtype='float16' if half else 'float32')
        cells = min(leaves, SAMPLES) * 38                      # the points and trinkets of the cells that are hit
        if op.startswith('interpolate_forward'):
            def hip():
                return P.unbatched_interpolate_trilinear(*args)

            def torch_():
                return P._torch_interpolate_forward(*args)
            if half:
                def agree(a, b):
                    want = P._torch_interpolate_forward(*args64)
                    fmax = feats.double()[trinkets[pidx.long()].long()].abs().amax(dim=1)[:, None, :]
                    bound = 64 * 2.0 ** -24 * fmax + torch.clamp(2.0 ** -11 * want.abs(), min=2.0 ** -25)
                    return bool(((a.double() - want).abs() <= bound).all()) and torch.equal(a, b)
            nbytes, launches, reads = 16 * SAMPLES + SAMPLES * D * size + nf * D * size + cells, 1, 0
        elif op == 'interpolate_backward_feats':
            def hip():
                return _C.ops.spc.interpolate_trilinear_backward_feats_cuda(*args, grad_out)

            def torch_():
                return P._torch_interpolate_backward_feats(*args, grad_out)

            def agree(a, b):
                want = P._torch_interpolate_backward_feats(*args64, grad_out.double())
                rows = trinkets[pidx.long()].long().reshape(-1)
                abs_sum = torch.zeros_like(want).index_add_(0, rows, grad_out.double().abs().expand(-1, 8, -1).reshape(-1, D))
                count = torch.zeros(nf, dtype=torch.float64, device='cuda').index_add_(0, rows, torch.ones_like(rows, dtype=torch.float64))
                bound = (count[:, None] + 8) * 2.0 ** -24 * abs_sum
                res['max_adds_per_row'] = int(count.max())
                return bool(((a.double() - want).abs() <= bound).all()) and bool(((b.double() - want).abs() <= bound).all())
            added = 8 * SAMPLES * D * 4
            res.update(atomic_bytes=added, atomic_ms=round(added / ATOMIC_BPS * 1e3, 5))
            nbytes, launches, reads = 16 * SAMPLES + SAMPLES * D * 4 + nf * D * 4 + cells, 2, 0       # the zero fill and the kernel
        else:
            def hip():
                return _C.ops.spc.interpolate_trilinear_backward_coords_cuda(*args, grad_out)

            def torch_():
                return P._torch_interpolate_backward_coords(*args, grad_out)

            def agree(a, b):
                want = P._torch_interpolate_backward_coords(*args64, grad_out.double())
                fmax = feats.double()[trinkets[pidx.long()].long()].abs().amax(dim=1)[:, None, :]
                bound = ((D + 48) * 2.0 ** -24 * (grad_out.double().abs() * fmax).sum(dim=-1))[..., None]
                return bool(((a.double() - want).abs() <= bound).all()) and bool(((b.double() - want).abs() <= bound).all())
            nbytes, launches, reads = 16 * SAMPLES + SAMPLES * D * 4 + nf * D * 4 + cells + 12 * SAMPLES, 1, 0
    a, b = hip(), torch_()
    assert agree(a, b), f'{op}: the torch formulation differs from the HIP path'
    del a, b
    for _ in range(2):
        hip()
        torch_()
    torch.cuda.synchronize()
    for key, fn in (('hip', hip), ('torch', torch_)):
        med, low = median_ms(fn, reps)
        res[f'{key}_ms'], res[f'{key}_min_ms'] = round(med, 4), round(low, 4)
    bound = nbytes / ACHIEVABLE_BPS * 1e3 + res.get('atomic_ms', 0.0)
    res.update(torch_over_hip=round(res['torch_ms'] / res['hip_ms'], 2), compulsory_bytes=nbytes, bound_ms=round(bound, 5),
               bound_over_hip=round(bound / res['hip_ms'], 4), launches_by_construction=launches, host_reads_by_construction=reads)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--case', type=int, default=None, help='(internal) run one case in this process')
    args = ap.parse_args()
    if args.case is not None:
        print(json.dumps(run_case(CASES[args.case], args.reps)), flush=True)
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
