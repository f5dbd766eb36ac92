"""Times the SPC convolutions of kaolin.ops.spc on one GPU: one JSON line per case.

    python tools/time_spc_conv.py [--reps 20] [--out profiles/spc_conv_time.jsonl]

The workload is the project's own: the octree of unbatched_mesh_to_spc for the bench's geodesic sphere (50 000 faces) with features
at level 8; a 3^3 kernel; 32 -> 32 and 64 -> 64 channels; jump 0 and jump 1; conv3d (input at level 8) and conv_transpose3d (output
at level 8); the forward alone and the forward with both gradients; float32.  Every (operator, jump) runs in a child process of its
own under a time limit; the first failure ends the run.

Per case: `hip_ms` = the median over the repetitions of the call between two device events, `torch_ms` = the same for the package's
torch formulation (the CPU path, run on the same GPU tensors), after checking that both agree with that formulation in float64
within the bound of tests/spc_conv_bruteforce.py ((T + 1) u / (1 - (T + 1) u) sum |a b| + u |want|, T the products of the element).
The torch formulation is the yardstick: the parent commit has nothing to time and the reference does not run on this hardware.
`hits` = the (offset, output row) pairs with a neighbour; `useful_tflops` = 2 hits in out (three times that with the gradients)
over hip_ms, `share_of_f32_matrix_peak` = that over 157 TF; `map_ms` = the neighbour-map kernel alone.  `launches_by_construction`
and `host_reads_by_construction` are NOT measured: they follow the launch sequence of csrc/spc_conv.hip and its shim."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32_MATRIX_PEAK = 157e12
LEVEL = 8
GROUPS = [(False, 0), (False, 1), (True, 0), (True, 1)]        # (transposed, jump)
CHANNELS = [32, 64]
GROUP_TIME_LIMIT_S = 280


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


def run_group(transposed, jump, reps):
    import itertools
    import torch
    import kaolin_amd as kal
    from kaolin_amd import _C, _lib
    from kaolin_amd.ops.spc import convolution as V
    from kaolin_amd.utils.testing import geodesic_sphere
    assert torch.cuda.is_available(), 'time_spc_conv.py measures on the GPU'
    v, f = geodesic_sphere(50)
    octree = kal.ops.conversions.unbatched_mesh_to_spc((v.float() * 1.2)[f].contiguous().cuda(), LEVEL)[0]
    s = kal.rep.Spc(octree, torch.tensor([octree.numel()], dtype=torch.int32))
    pyramids, points, exsum = s.pyramids, s.point_hierarchies, s.exsum
    in_level = LEVEL - jump if transposed else LEVEL
    out_level = LEVEL if transposed else LEVEL - jump
    kv = torch.tensor(list(itertools.product((-1, 0, 1), repeat=3)), dtype=torch.int16).cuda()
    K, n_in, n_out = kv.size(0), int(pyramids[0, 0, in_level]), int(pyramids[0, 0, out_level])
    op = kal.ops.spc.conv_transpose3d if transposed else kal.ops.spc.conv3d
    table = V._torch_neighbour_map(points, pyramids, kv, out_level, in_level, transposed)
    hits = int((table >= 0).sum())
    per_row = (table >= 0).sum(dim=0).double()[:, None]

    def map_alone():
        lib = _lib.load()
        meta = _C.ops.spc_conv_meta(pyramids, out_level, in_level).cuda()
        out = torch.empty((K, n_out), dtype=torch.int32, device='cuda')

        def call():
            _lib.check(lib.kamd_spc_conv_map(_lib.stream_ptr(out.device), int(transposed), 1, K, n_out, out_level, jump,
                                             octree.numel(), points.size(0), n_in, _lib.ptr(octree), _lib.ptr(exsum),
                                             _lib.ptr(points), _lib.ptr(kv), _lib.ptr(meta), _lib.ptr(out)), 'conv_map')
        call()
        assert torch.equal(out.long(), table), 'the map kernel differs from the torch formulation'
        return median_ms(call, reps)[0]
    map_ms = map_alone()
    lines = []
    for C in CHANNELS:
        g = torch.Generator().manual_seed(C)
        x = (torch.rand((n_in, C), generator=g) * 2 - 1).cuda()
        w = ((torch.rand((K, C, C), generator=g) * 2 - 1) / (K * C) ** 0.5).cuda()
        grad = (torch.rand((n_out, C), generator=g) * 2 - 1).cuda()
        structure = (octree, points, in_level, pyramids, exsum)

        def torch_forward(x, w):
            return V._torch_conv(transposed, points, in_level, out_level, pyramids, x, w, kv)

        def hip_forward(x, w):
            return op(*structure, x, w, kv, jump)[0]
        # agreement: both against the formulation in float64, within the bound
        want = torch_forward(x.double(), w.double())
        abs_sum = torch_forward(x.double().abs(), w.double().abs())
        t = (per_row * C + 1) * 2.0 ** -24
        bound = t / (1 - t) * abs_sum + 2.0 ** -24 * want.abs()
        worst = 0.0
        for fn in (hip_forward, torch_forward):
            share = float((((fn(x, w).double() - want).abs() / bound.clamp(min=1e-300))[bound > 0]).max())
            assert share <= 1.0, f'{fn.__name__} misses the bound: {share}'
            worst = max(worst, share) if fn is hip_forward else worst
        for mode in ('forward', 'forward_backward'):
            def make(fn):
                if mode == 'forward':
                    return lambda: fn(x, w)
                xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()

                def step():
                    xg.grad = wg.grad = None
                    fn(xg, wg).backward(grad)
                return step
            hip, torch_ = make(hip_forward), make(torch_forward)
            for _ in range(2):
                hip()
                torch_()
            torch.cuda.synchronize()
            res = {'op': 'conv_transpose3d' if transposed else 'conv3d', 'mode': mode, 'jump': jump, 'channels': C, 'level': LEVEL,
                   'rows_in': n_in, 'rows_out': n_out, 'kernel_vectors': K, 'hits': hits, 'dtype': 'float32', 'reps': reps}
            for key, fn in (('hip', hip), ('torch', torch_)):
                med, low = median_ms(fn, reps)
                res[f'{key}_ms'], res[f'{key}_min_ms'] = round(med, 4), round(low, 4)
            flops = 2.0 * hits * C * C * (3 if mode == 'forward_backward' else 1)
            rate = flops / (res['hip_ms'] * 1e-3)
            res.update(torch_over_hip=round(res['torch_ms'] / res['hip_ms'], 2), useful_tflops=round(rate / 1e12, 3),
                       share_of_f32_matrix_peak=round(rate / F32_MATRIX_PEAK, 4), map_ms=round(map_ms, 4),
                       forward_share_of_bound=round(worst, 3), launches_by_construction=2 if mode == 'forward' else 6,
                       host_reads_by_construction=0)
            lines.append(json.dumps(res))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=None)
    ap.add_argument('--group', type=int, default=None, help='(internal) run one (operator, jump) in this process')
    args = ap.parse_args()
    if args.group is not None:
        print('\n'.join(run_group(*GROUPS[args.group], args.reps)), flush=True)
        return 0
    lines, status = [], 0
    for k in range(len(GROUPS)):
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), '--group', str(k), '--reps', str(args.reps)],
                                 stdout=subprocess.PIPE, text=True, timeout=GROUP_TIME_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f'group {GROUPS[k]} exceeded its {GROUP_TIME_LIMIT_S} s limit: stopping', file=sys.stderr)
            status = 1
            break
        if res.returncode != 0 or not res.stdout.strip():
            print(f'group {GROUPS[k]} ended with status {res.returncode}: stopping', file=sys.stderr)
            status = 1
            break
        got = [line for line in res.stdout.strip().splitlines() if line.startswith('{')]
        print('\n'.join(got), flush=True)
        lines.extend(got)
    if args.out and lines:          # what was measured before a failure is kept
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return status


if __name__ == '__main__':
    sys.exit(main())
