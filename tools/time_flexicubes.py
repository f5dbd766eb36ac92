"""Times kaolin.ops.conversions.FlexiCubes on one GPU: one JSON line per (resolution, mode).

    python tools/time_flexicubes.py [--reps 7] [--commit TEXT] [--out profiles/flexicubes_time.jsonl]

Workload, float32: ``construct_voxel_grid(res)`` for res = 64 and 128, an off-centre sphere as the scalar field, seeded random
beta / alpha / gamma_f (0.5 randn).  Modes: ``train_fwd`` (training=True, the call), ``train_fwd_bwd`` (the call and the backward of
``vertices.sum() + L_dev.sum()`` into all five inputs), ``eval_fwd`` (training=False, the call).  Every case runs in a child
process of its own under a time limit; the first failure ends the run.

Per case, on the same GPU tensors, results are compared before anything is timed (faces equal, floats within 1e-5):
  `hip_ms`    the public call on the HIP pipeline (csrc/flexicubes.hip),
  `torch_ms`  the package's torch formulation of the same contract.  It stands for the reference, which is torch code of the same
              kind (a few hundred small launches, about ten host reads) and does not exist on the GPU machine.
Each is the median over the repetitions of the whole step between two device events, ended by a device synchronise.
`hip_launches` / `torch_launches`: the kernels (memsets and copies included) of one step, counted by torch's profiler in a run
of its own, or "not measured" when the profiler gives nothing.  `hip_host_reads` is 2 by construction (the sizes with the index
flag; the number of quads); `torch_host_reads`: the synchronising calls torch reports in its sync debug mode during one step.
`bound_ms` = sdf and cube_idx read once and the outputs written once, over the achievable HBM bandwidth of 6.3 TB/s;
`bound_over_hip` = the share of that byte bound the step reaches.  `commit` names what the numbers were taken on.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_BPS = 6.3e12
CASES = [(r, m) for r in (64, 128) for m in ('train_fwd', 'train_fwd_bwd', 'eval_fwd')]
CASE_TIME_LIMIT_S = 200


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


def count_launches(fn):
    import torch
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
        return n if n > 0 else 'not measured'
    except Exception:  # noqa: BLE001  (no profiler on this build: the count is optional)
        return 'not measured'


def count_host_reads(fn):
    import torch
    torch.cuda.set_sync_debug_mode('warn')
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            fn()
        return sum(1 for w in seen if 'synchroniz' in str(w.message))
    finally:
        torch.cuda.set_sync_debug_mode('default')


def run_case(res, mode, reps, commit):
    import torch
    from kaolin_amd.ops.conversions import FlexiCubes
    from kaolin_amd.ops.conversions.flexicubes import flexicubes as fcm
    assert torch.cuda.is_available(), 'time_flexicubes.py measures on the GPU'
    dev = 'cuda:0'
    training, backward = mode != 'eval_fwd', mode == 'train_fwd_bwd'
    fc = FlexiCubes(dev)
    v, c = fc.construct_voxel_grid(res)
    g = torch.Generator().manual_seed(res)
    s = (v - torch.tensor([0.04, -0.03, 0.02], device=dev)).norm(dim=-1) - 0.33
    weights = [(0.5 * torch.randn(shape, generator=g)).to(dev) for shape in ((c.shape[0], 12), (c.shape[0], 8), (c.shape[0],))]
    leaves = [t.clone().requires_grad_(backward) for t in (v, s, *weights)]

    def step(fn):
        out = fn(*leaves)
        if backward:
            for t in leaves:
                t.grad = None
            (out[0].sum() + out[2].sum()).backward()
        return out

    def hip():
        return step(lambda x, sdf, b, a, gm: fc(x, sdf, c, res, beta=b, alpha=a, gamma_f=gm, training=training))

    def formulation():
        return step(lambda x, sdf, b, a, gm: fcm.flexicubes_torch(x, sdf, c, (res,) * 3, 0.99, b, a, gm, training)[:3])

    out = hip()
    grads = [t.grad.clone() for t in leaves] if backward else []
    want = formulation()
    assert torch.equal(out[1], want[1]), 'the faces of the torch formulation differ from the HIP path'
    assert torch.allclose(out[0], want[0], rtol=0, atol=1e-5) and torch.allclose(out[2], want[2], rtol=0, atol=1e-5)
    for got, leaf in zip(grads, leaves):
        scale = float(leaf.grad.abs().max())
        assert float((got - leaf.grad).abs().max()) <= 1e-3 * scale + 1e-6, 'the gradients differ'
    torch.cuda.synchronize()
    result = {'res': res, 'mode': mode, 'dtype': 'float32', 'reps': reps, 'commit': commit, 'cubes': c.shape[0],
              'vertices': out[0].shape[0], 'faces': out[1].shape[0], 'incidences': out[2].shape[0]}
    for key, fn in (('hip', hip), ('torch', formulation)):
        fn()
        med, low = median_ms(fn, reps)
        result[f'{key}_ms'], result[f'{key}_min_ms'] = round(med, 4), round(low, 4)
    nbytes = s.numel() * 4 + c.numel() * 8 + sum(t.numel() * t.element_size() for t in out)
    bound = nbytes / ACHIEVABLE_BPS * 1e3
    result.update(bound_ms=round(bound, 4), bound_over_hip=round(bound / result['hip_ms'], 4),
                  torch_over_hip=round(result['torch_ms'] / result['hip_ms'], 2), hip_launches='not measured',
                  torch_launches='not measured', hip_host_reads=2, torch_host_reads='not measured')
    print(json.dumps(result), flush=True)                       # (the times stand even if the counting below does not end)
    result['torch_host_reads'] = count_host_reads(formulation)
    result['hip_launches'], result['torch_launches'] = count_launches(hip), count_launches(formulation)
    return result


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
        except subprocess.TimeoutExpired as late:
            print(f'case {CASES[k]} exceeded its {CASE_TIME_LIMIT_S} s limit: stopping', file=sys.stderr)
            partial = late.stdout.decode() if isinstance(late.stdout, bytes) else (late.stdout or '')
            lines += [ln for ln in partial.strip().splitlines() if ln.startswith('{')][-1:]
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
