"""Times one Simplicits training step, forward plus backward, on one GPU: kaolin_amd.physics.simplicits.compute_losses and
(le + lo).backward() at the training size, one JSON line.

    python tools/time_simplicits_training.py [--out profiles/simplicits_training_time.jsonl]

float32, N = 1000 sample points of 10000, B = 10 transforms, H = 10 handles, (W, L) = (64, 6); default init.  Paths: `hip` = the step
as the package runs it (csrc/skinning_mlp_backward.hip and csrc/simplicits_loss.hip, with the draws, the packing of the parameters
and the split of their gradient: the whole step), `torch` = the same step with the network in this package's torch forward mode under
autograd and the losses in their torch definition, on the same GPU tensors: what a step cost before the kernels existed.  Before
timing, the two paths' losses and parameter gradients under one seed are compared (normwise, hip against torch) and the figures go
into the line.  Per path: the median, smallest and largest of 7 repetitions of 50 steps between two device events after a warm-up,
the paths alternating; milliseconds per step."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

M, N, B, H, W, L = 10000, 1000, 10, 10, 64, 6
REPS, STEPS = 7, 50


def main():
    import torch
    from kaolin_amd.physics import simplicits
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_simplicits_training.py measures on the GPU'
    torch.manual_seed(0)
    mod = simplicits.SimplicitsMLP(3, W, H, L).cuda()
    pts = torch.rand(M, 3, device='cuda')
    yms, prs, rhos = (torch.full((M,), v, device='cuda') for v in (1e5, 0.45, 1000.0))

    def hip():
        mod.zero_grad()
        le, lo = simplicits.compute_losses(mod, pts, yms, prs, rhos, 0.5, B, 1.0, N, 0.1, 1e6)
        (le + lo).backward()
        return [le, lo] + [p.grad for p in mod.parameters()]

    def torch_path():
        mod.zero_grad()
        idx = torch.randint(low=0, high=M, size=(N,), device='cuda')
        x = pts[idx]
        mus, lams = simplicits._materials(yms[idx], prs[idx], 0.5, False)
        w, jac = mod._forward_mode(x, box=(0.0, 1.0))
        tfms = 0.1 * torch.randn(B, H - 1, 3, 4).cuda()
        le, lo = simplicits._losses_definition(w[:, :-1], jac[:, :-1], x, tfms, mus, lams, 0.5, 1.0 / N, 1.0)
        le, lo = 0.1 * le, 1e6 * lo
        (le + lo).backward()
        return [le, lo] + [p.grad for p in mod.parameters()]

    paths = {'hip': hip, 'torch': torch_path}
    results = {}
    for name, fn in paths.items():       # (the warm-up)
        torch.manual_seed(1)
        results[name] = [t.detach().clone() for t in fn()]
    torch.cuda.synchronize()
    res = {'op': 'simplicits_training_step', 'N': N, 'B': B, 'H': H, 'W': W, 'L': L}
    diffs = [((a - b).norm() / b.norm()).item() for a, b in zip(results['hip'], results['torch'])]
    res.update({'le_diff': diffs[0], 'lo_diff': diffs[1], 'grad_diff_max': max(diffs[2:])})
    times = {name: [] for name in paths}
    for _ in range(REPS):
        for name, fn in paths.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(STEPS):
                fn()
            t1.record()
            torch.cuda.synchronize()
            times[name].append(t0.elapsed_time(t1) / STEPS)
    for name, ts in times.items():
        res.update({f'{name}_ms': round(statistics.median(ts), 4), f'{name}_min_ms': round(min(ts), 4), f'{name}_max_ms': round(max(ts), 4)})
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
