"""Times ops.pointcloud.farthest_point_sampling (csrc/fps.hip) on one GPU: one JSON line per size.

    python tools/time_fps.py [--reps 20] [--baseline-reps 5] [--out profiles/fps_time.jsonl]

Sizes (B, N, k): (32, 4096, 1024), (8, 16384, 2048), (1, 16384, 2048), (1, 100000, 4096); seeded lattice clouds (coordinates j / 1024:
the centre is exact in any summation order, so every path has the same right answer).  Paths: `block` = one workgroup per cloud with
the points in registers (N up to the block limit), `rounds` = one launch per selected point (forced), `torch` = the same rule as a
plain torch loop on the GPU, a round = a dozen torch launches and no host read -- it stands in for what a user without the operator
runs.  Before timing the indices of all paths are compared (torch.equal) and the run fails if they differ.

Per path: the median over the repetitions of the whole call between two device events after a warm-up, `*_ms`, the smallest and
largest repetition, and `*_us_per_round` = median / k.  The repetitions of the paths ALTERNATE (block, rounds, block, ...), so that a
difference between the two can be held against the spread of each."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(32, 4096, 1024), (8, 16384, 2048), (1, 16384, 2048), (1, 100000, 4096)]


def torch_loop(points, k):
    """the rule of ops.pointcloud.farthest_point_sampling, batched, nothing read back"""
    import torch
    B, N, _ = points.shape
    index = torch.arange(N, device=points.device).expand(B, N)
    rows = torch.arange(B, device=points.device)
    out = torch.empty((B, k), dtype=torch.int64, device=points.device)

    def sq_dist(q):
        sq = (points - q[:, None]) * (points - q[:, None])
        return (sq[..., 0] + sq[..., 1]) + sq[..., 2]

    finite = torch.isfinite(points).all(dim=2, keepdim=True)
    centre = (torch.where(finite, points, 0.0).double().sum(dim=1) / finite.sum(dim=1)).float()
    centre = torch.where(torch.isfinite(centre).all(dim=1, keepdim=True), centre, 0.0)
    d = sq_dist(centre)
    D = torch.where(torch.isfinite(d), d, -1.0)
    for r in range(k):
        s = torch.where(D == D.max(dim=1, keepdim=True)[0], index, N).min(dim=1)[0]
        out[:, r] = s
        d = sq_dist(points[rows, s])
        D = torch.where(torch.isfinite(d), torch.minimum(D, d), D) if r else torch.where(torch.isfinite(d), d, -1.0)
        D[rows, s] = -2.0
    return out


def main():
    import torch
    from kaolin_amd import _C, _lib
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--baseline-reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_fps.py measures on the GPU'
    limit = _lib.load().kamd_fps_block_limit()
    lines = []
    for B, N, k in SIZES:
        points = (torch.randint(0, 1024, (B, N, 3), generator=torch.Generator().manual_seed(N)) / 1024).cuda()
        paths = {'rounds': lambda: _C.ops.farthest_point_sampling_cuda(points, k, path='rounds'),
                 'torch': lambda: torch_loop(points, k)}
        if N <= limit:
            paths = {'block': lambda: _C.ops.farthest_point_sampling_cuda(points, k, path='block'), **paths}
        results = {name: fn() for name, fn in paths.items()}       # (the warm-up)
        torch.cuda.synchronize()
        for name, got in results.items():
            assert torch.equal(got, results['rounds']), f'{(B, N, k)}: {name} and rounds select different points'
        times = {name: [] for name in paths}
        for rep in range(args.reps):
            for name, fn in paths.items():
                if name == 'torch' and rep >= args.baseline_reps:
                    continue
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                torch.cuda.synchronize()
                times[name].append(t0.elapsed_time(t1))
        res = {'op': 'farthest_point_sampling', 'B': B, 'N': N, 'k': k, 'block_limit': limit, 'indices_equal': True}
        for name, ts in times.items():
            med = statistics.median(ts)
            res.update({f'{name}_ms': round(med, 4), f'{name}_min_ms': round(min(ts), 4), f'{name}_max_ms': round(max(ts), 4),
                        f'{name}_reps': len(ts), f'{name}_us_per_round': round(med * 1e3 / k, 3)})
        line = json.dumps(res)
        print(line, flush=True)
        lines.append(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
