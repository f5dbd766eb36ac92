"""Times SimplicitsMLP.compute_weights_and_dwdx (csrc/skinning_mlp.hip) on one GPU, one JSON line per size, and measures the
device's expm1f / expf as that kernel calls them.

    python tools/time_skinning.py [--out profiles/skinning_time.jsonl]

float32, (W, L) = (64, 6), H in {8, 32, 128}, N in {2^12, 2^17, 2^20}; default init.  Paths: `hip` = the one launch (with the packing
of the parameters: the whole call), `torch` = this package's forward-mode path on the same GPU tensors under no_grad, `jacrev` = the
reference's expression, the weights call plus vmap(jacrev(...)), where its (N, H - 1, W) activations fit (N (H - 1) <= 2^22).
Before timing, the paths are compared (max difference over the largest entry of the Jacobian) and the figure goes into the line.
Per path: the median, smallest and largest of 7 repetitions of the whole call between two device events after a warm-up, the
paths alternating.  `hip_mfma_share` = 8 N (3 W + L W^2 + W (H - 1)) useful flop over the median over 157 Tflop/s (the float32
matrix peak); `hip_byte_share` = the bytes of pts, weights and weights_jac over the median over 6.3 TB/s.  Whole-call figures.

The first line is `elu_ulp`: elu and elu' of 2^22 + 1 evenly spaced float32 y in [-30, 0] against float64 (expm1, exp), the largest
error in units of the float64 result's float32 ulp.  Twice the larger is C_ULP of tests/test_skinning_gpu.py."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, L = 64, 6
SIZES = [(N, H) for H in (8, 32, 128) for N in (2 ** 12, 2 ** 17, 2 ** 20)]
REPS = 7


def elu_ulp(torch, _C):
    y = torch.linspace(-30.0, 0.0, 2 ** 22 + 1, dtype=torch.float64).float().cuda()
    worst = {}
    for name, got, want in zip(('expm1f', 'expf'), _C.physics.skinning_elu_cuda(y), (torch.expm1(y.double()), torch.exp(y.double()))):
        ulp = torch.exp2(torch.floor(torch.log2(want.abs().clamp(min=2.0 ** -126))) - 23)
        worst[name] = ((got.double() - want).abs() / ulp).max().item()
    return {'op': 'elu_ulp', 'points': y.numel(), 'expm1f_ulp': round(worst['expm1f'], 4), 'expf_ulp': round(worst['expf'], 4)}


def main():
    import torch
    from kaolin_amd import _C
    from kaolin_amd.physics import simplicits
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_skinning.py measures on the GPU'
    lines = [json.dumps(elu_ulp(torch, _C))]
    print(lines[0], flush=True)
    for N, H in SIZES:
        torch.manual_seed(N + H)
        mod = simplicits.SimplicitsMLP(3, W, H, L).requires_grad_(False).cuda()
        pts = torch.rand(N, 3, device='cuda')
        paths = {'hip': lambda: mod.compute_weights_and_dwdx(pts), 'torch': lambda: mod._forward_mode(pts)}
        if N * (H - 1) <= 2 ** 22:
            paths['jacrev'] = lambda: (simplicits.SkinningModule.compute_skinning_weights(mod, pts),
                                       simplicits.SkinningModule.compute_dwdx(mod, pts))
        results = {name: fn() for name, fn in paths.items()}       # (the warm-up)
        torch.cuda.synchronize()
        res = {'op': 'skinning_mlp', 'N': N, 'W': W, 'L': L, 'H': H}
        for name in list(paths)[1:]:
            res[f'{name}_jac_diff'] = ((results['hip'][1] - results[name][1]).abs().max() / results[name][1].abs().max()).item()
        del results
        times = {name: [] for name in paths}
        for _ in range(REPS):
            for name, fn in paths.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                torch.cuda.synchronize()
                times[name].append(t0.elapsed_time(t1))
        for name, ts in times.items():
            res.update({f'{name}_ms': round(statistics.median(ts), 4), f'{name}_min_ms': round(min(ts), 4),
                        f'{name}_max_ms': round(max(ts), 4)})
        seconds = res['hip_ms'] * 1e-3
        res['hip_mfma_share'] = round(8 * N * (3 * W + L * W * W + W * (H - 1)) / seconds / 157e12, 4)
        res['hip_byte_share'] = round(4 * N * (3 + 4 * H) / seconds / 6.3e12, 4)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
