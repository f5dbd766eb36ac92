"""Times kaolin.ops.voxelgrid.fill on one GPU at 256^3: one JSON line per (grid, dtype, N).

    python tools/time_voxelgrid_fill.py [--reps 20] [--out profiles/voxelgrid_fill_time.jsonl]

Grids: `shell` = the lattice shell 118^2 <= |p - c|^2 <= 120^2 around (127, 130, 125); `sphere` = the bench's geodesic
sphere (50 000 faces) through trianglemeshes_to_voxelgrids.  Input float32 and bool, N = 1 and 8 (the same grid repeated).
Every case runs in a child process of its own under a time limit; the first failure ends the run.

Per case: `median_ms` of the whole public call (device events around it; the call itself synchronises its stream to poll),
`passes` that changed something plus the one that found the fixed point, passes `launched`, host `polls`, and -- from a
second, separately profiled set of calls (the library's per-kernel events, kamd_profile_enable) -- the mean time of the pack,
pass and unpack kernels.  `bound_ms` = the bytes of the two compulsory passes (the dense input read once, the bool output
written once) over the achievable HBM bandwidth of 6.3 TB/s (8 TB/s peak); `bound_over_time` = bound_ms / median_ms, and
`pack_unpack_bound_frac` = bound_ms over the pack + unpack kernel time alone.  `filled` = voxels set in one item.
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
R = 256
CASES = [(g, d, n) for g in ('shell', 'sphere') for d in ('float32', 'bool') for n in (1, 8)]
CASE_TIME_LIMIT_S = 120


def make_grid(name, dtype, n):
    import torch
    import kaolin_amd as kal
    if name == 'shell':
        r = torch.arange(R, device='cuda', dtype=torch.int32)
        d2 = ((r - 127) ** 2).view(-1, 1, 1) + ((r - 130) ** 2).view(1, -1, 1) + ((r - 125) ** 2).view(1, 1, -1)
        grid = ((d2 >= 118 * 118) & (d2 <= 120 * 120)).unsqueeze(0)
    else:
        from kaolin_amd.utils.testing import geodesic_sphere
        v, f = geodesic_sphere(50)
        grid = kal.ops.conversions.trianglemeshes_to_voxelgrids(v.float()[None].cuda(), f.cuda(), R)
    return grid.to(getattr(torch, dtype)).expand(n, -1, -1, -1).contiguous()


def run_case(name, dtype, n, reps):
    import torch
    from kaolin_amd import _C, _lib
    assert torch.cuda.is_available(), 'time_voxelgrid_fill.py measures on the GPU'
    lib = _lib.load()
    x = make_grid(name, dtype, n)
    stats = {}
    for _ in range(3):
        out = _C.ops.voxelgrid_fill_cuda(x, stats=stats)
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        _C.ops.voxelgrid_fill_cuda(x)
        t1.record()
        torch.cuda.synchronize()
        times.append(t0.elapsed_time(t1))
    lib.kamd_profile_reset()
    lib.kamd_profile_select(-1)
    lib.kamd_profile_enable(1)
    for _ in range(5):
        _C.ops.voxelgrid_fill_cuda(x)
    torch.cuda.synchronize()
    lib.kamd_profile_enable(0)
    prof = _lib.kernel_profile(reset=True)
    kern = {k: prof[k][0] / 5 for k in ('vf_pack_kernel', 'vf_pass_kernel', 'vf_unpack_kernel')}   # ms per call
    bound = n * R ** 3 * (x.element_size() + 1) / ACHIEVABLE_BPS * 1e3
    med = statistics.median(times)
    return {'grid': name, 'dtype': dtype, 'N': n, 'reps': reps, 'median_ms': round(med, 4), 'min_ms': round(min(times), 4),
            'passes': stats['passes'], 'launched': stats['launched'], 'polls': stats['polls'],
            'pack_ms': round(kern['vf_pack_kernel'], 4), 'passes_ms': round(kern['vf_pass_kernel'], 4),
            'unpack_ms': round(kern['vf_unpack_kernel'], 4), 'bound_ms': round(bound, 4),
            'bound_over_time': round(bound / med, 4),
            'pack_unpack_bound_frac': round(bound / (kern['vf_pack_kernel'] + kern['vf_unpack_kernel']), 4),
            'filled': int(out[0].sum())}


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
