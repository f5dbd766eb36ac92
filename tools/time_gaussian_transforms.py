"""Times kaolin.ops.gaussians.transform_gaussians on one GPU: one JSON line per (N, degree, transform, path, mode).

    python tools/time_gaussian_transforms.py [--reps 7] [--label direct_rows] [--out profiles/gaussian_transforms_time.jsonl]

Workload: N = 2^20 and 2^22 Gaussians, float32, SH degree 3 and degree 0, ONE transform (`shared`) and one per Gaussian (`per`): a
rotation, a uniform scale and a translation.  Paths: `hip` = the public call (csrc/gaussian_transform.hip) and `torch` = the
package's torch formulation (ops/gaussians/transforms.py::_torch_transform_gaussians) on the same GPU tensors -- the stand-in for
what the reference's chain of torch kernels costs on a GPU (the reference itself is not available where this runs).  The two
results are compared before anything is timed.  Modes: `forward` (no autograd graph) and `forward_backward` (the four outputs are
back-propagated with cotangents of ones into positions, orientations, scales and sh_coeff).
Every (N, degree, transform) runs in a child process of its own under a time limit; the first failure ends the run.

Per line: `median_ms` / `min_ms` of `reps` whole calls after 3 warm-up calls (device events around the call); `launches` = the
device kernels of one call and `host_reads` = its device-to-host copies, both counted with torch's profiler; `bound_ms` = the bytes
the call cannot avoid (every input read once, every output written once; the backward reads the four cotangents, the orientations
and the transform and writes four gradients) over the achievable HBM bandwidth of 6.3 TB/s; `bound_over_time` = bound_ms /
median_ms.  `--label` names the build that was measured (KAMD_LIB_PATH selects a development build: that is how the rejected lane
mapping was measured before it was deleted).  Each line carries the commit it was measured at and its parent.
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
CASES = [(n, degree, tf) for n in (1 << 20, 1 << 22) for degree in (3, 0) for tf in ('shared', 'per')]
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


def counted(fn):
    """-> (device kernels, device-to-host copies) of one call"""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name.lower() for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    kernels = [s for s in names if 'memcpy' not in s and 'memset' not in s]
    host_reads = [s for s in names if 'memcpy' in s and ('dtoh' in s or 'device -> host' in s or 'devicetohost' in s)]
    return len(kernels), len(host_reads)


def bytes_per_gaussian(degree, tf, grad):
    sh = 12 * (degree + 1) ** 2
    matrix = 64 if tf == 'per' else 0
    forward = (12 + 16 + 12 + sh + matrix) + (12 + 16 + 12 + sh)
    backward = (12 + 16 + 12 + sh + 16 + matrix) + (12 + 16 + 12 + sh)
    return forward + (backward if grad else 0)


def run_case(n, degree, tf, reps, label, only=None):
    import torch
    from kaolin_amd.ops.gaussians import transforms
    assert torch.cuda.is_available(), 'time_gaussian_transforms.py measures on the GPU'
    g = torch.Generator().manual_seed(1)
    m = n if tf == 'per' else 1
    quat = torch.nn.functional.normalize(torch.randn(m, 4, generator=g), dim=-1)
    x, y, z, w = quat.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                     2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                     2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], dim=-1).reshape(m, 3, 3)
    transform = torch.zeros(m, 4, 4)
    transform[:, :3, :3] = R * (0.5 + 1.5 * torch.rand(m, 1, 1, generator=g))
    transform[:, :3, 3] = torch.randn(m, 3, generator=g)
    transform[:, 3, 3] = 1
    transform = transform.cuda()
    inputs = [torch.randn(n, 3, generator=g).cuda(), torch.randn(n, 4, generator=g).cuda(),
              (0.2 + torch.rand(n, 3, generator=g)).cuda(), torch.randn(n, (degree + 1) ** 2, 3, generator=g).cuda()]

    def hip():
        return transforms.transform_gaussians(inputs[0], inputs[1], inputs[2], transform, inputs[3])

    def formulation():
        return transforms._torch_transform_gaussians(inputs[0], inputs[1], inputs[2], transform, inputs[3], degree, False, False)

    with torch.no_grad():
        for a, b in zip(hip(), formulation()):
            assert torch.allclose(a, b, rtol=1e-4, atol=1e-4), 'the two paths disagree'
    lines = []
    for mode in ('forward', 'forward_backward'):
        grad = mode == 'forward_backward'
        for t in inputs:
            t.requires_grad_(grad)
        ones = [torch.ones_like(t) for t in inputs]
        for path, fn in (('hip', hip), ('torch', formulation)):
            if only not in (None, path):
                continue
            def call():
                with torch.set_grad_enabled(grad):
                    out = fn()
                    if grad:
                        torch.autograd.grad(out, inputs, ones)
            times = timed(call, reps)
            launches, host_reads = counted(call)
            per = bytes_per_gaussian(degree, tf, grad)
            bound = n * per / ACHIEVABLE_BPS * 1e3
            med = statistics.median(times)
            lines.append({'operator': 'transform_gaussians', 'label': label, 'n': n, 'degree': degree, 'transform': tf,
                          'dtype': 'float32', 'path': path, 'mode': mode, 'reps': reps, 'median_ms': round(med, 4),
                          'min_ms': round(min(times), 4), 'launches': launches, 'host_reads': host_reads, 'bytes_per_gaussian': per,
                          'bound_ms': round(bound, 4), 'bound_over_time': round(bound / med, 4)})
    return lines


def git(*args):
    try:
        return subprocess.run(('git',) + args, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True).stdout.strip()
    except OSError:
        return ''


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    ap.add_argument('--label', default='direct_rows', help='names the build that is measured')
    ap.add_argument('--only', default=None, choices=('hip', 'torch'), help='time this path alone (the other one is not run)')
    ap.add_argument('--commit', default=None, help='recorded with every line (default: git rev-parse HEAD)')
    ap.add_argument('--parent', default=None)
    ap.add_argument('--case', type=int, default=None, help='(internal) run one case in this process')
    args = ap.parse_args()
    if args.case is not None:
        for line in run_case(*CASES[args.case], args.reps, args.label, args.only):
            print(json.dumps(line), flush=True)
        return 0
    stamp = {'commit': args.commit or git('rev-parse', 'HEAD') or None, 'parent': args.parent or git('rev-parse', 'HEAD^') or None}
    lines, status = [], 0
    for k in range(len(CASES)):
        try:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), '--case', str(k), '--reps', str(args.reps), '--label',
                                  args.label] + (['--only', args.only] if args.only else []), stdout=subprocess.PIPE, text=True, timeout=CASE_TIME_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(f'case {CASES[k]} exceeded its {CASE_TIME_LIMIT_S} s limit: stopping', file=sys.stderr)
            status = 1
            break
        if res.returncode != 0 or not res.stdout.strip():
            print(f'case {CASES[k]} ended with status {res.returncode}: stopping', file=sys.stderr)
            status = 1
            break
        for text in res.stdout.strip().splitlines():
            if not text.startswith('{'):
                continue
            record = {**json.loads(text), **stamp}
            line = json.dumps(record)
            print(line, flush=True)
            lines.append(line)
    if args.out and lines:          # what was measured before a failure is kept
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a' if args.append else 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return status


if __name__ == '__main__':
    sys.exit(main())
