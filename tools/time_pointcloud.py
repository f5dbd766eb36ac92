"""Times ops.conversions.unbatched_pointcloud_to_spc and pointclouds_to_voxelgrids on one GPU: one JSON line per case.

    python tools/time_pointcloud.py [--reps 7] [--out profiles/pointcloud_time.jsonl]

Inputs (seeded): 2^20 points on the sphere of radius 0.9 at levels 8 and 10 with no features, 3 and 32 float32 features; the same
number of points uniform in the octant [0, 0.9]^3 at level 1 (ONE cell: the long-run case of the mean) with 3 and 32 features;
8 clouds of 2^17 uniform points into 128^3 grids, float32, dense and sparse.  Every case runs in a child process of its own under
a time limit; the first failure ends the run.

Per case: `hip_ms` = the median over the repetitions of the whole public call between two device events, after a warm-up;
`user_ms` = the same for WHAT A USER WRITES WITHOUT THESE FUNCTIONS, from the package's other public operators and torch, on the
same GPU tensors: quantize_points, torch.unique(dim=0, return_inverse, return_counts), points_to_morton, torch.sort,
morton_to_points, unbatched_points_to_octree(sorted=True), index_add_ of doubles, divide, gather (the call sequence of the
reference's function); for the grids torch.cat / torch.unique(dim=0) over (B P, 4) int64 rows and a sparse -> dense conversion.
Before timing the results are compared: octrees and grids equal, features within 1e-6 relative (the yardstick's atomics fix no
order).  `launches` and `host_reads` are counted from the launch sequence of csrc/pointcloud.hip and its shim.  `bound_share` =
the time the compulsory traffic (points and features read once, results written once) takes at 6.3 TB/s, over hip_ms."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 1 << 20
CASES = [('spc', 'sphere', level, D) for level in (8, 10) for D in (0, 3, 32)] + \
        [('spc', 'octant', 1, D) for D in (3, 32)] + [('voxelgrids', 'dense', 128, 0), ('voxelgrids', 'sparse', 128, 0)]
CASE_TIME_LIMIT_S = 150
HBM_BYTES_PER_S = 6.3e12


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


def user_spc(pointcloud, level, features):
    """the octree and the mean features from the operators the package had before this function"""
    import torch
    from kaolin_amd.ops import spc as S
    cells, inverse, counts = torch.unique(S.quantize_points(pointcloud.contiguous(), level), dim=0, return_inverse=True,
                                          return_counts=True)
    morton, order = torch.sort(S.points_to_morton(cells.contiguous()).contiguous())
    octree = S.unbatched_points_to_octree(S.morton_to_points(morton.contiguous()), level, sorted=True)
    if features is None:
        return octree, None
    total = torch.zeros((cells.shape[0], features.shape[1]), dtype=torch.float64, device=features.device)
    mean = total.index_add_(0, inverse, features.double()) / counts[:, None].double()
    return octree, mean.to(features.dtype)[order]


def user_voxelgrids(pointclouds, resolution, return_sparse):
    import torch
    B, P, R = pointclouds.shape[0], pointclouds.shape[1], resolution
    origin = pointclouds.min(dim=1)[0]
    scale = (pointclouds.max(dim=1)[0] - origin).max(dim=1)[0]
    index = torch.round(((pointclouds - origin[:, None]) / scale[:, None, None]) * (torch.ones(1, device=pointclouds.device) * (R - 1))).long()
    item = torch.arange(B, device=pointclouds.device).repeat_interleave(P)[:, None]
    rows = torch.unique(torch.cat([item, index.reshape(-1, 3)], dim=1), dim=0)
    rows = rows[((rows[:, 1:] >= 0) & (rows[:, 1:] <= R - 1)).all(dim=1)]
    grid = torch.sparse_coo_tensor(rows.T, torch.ones(rows.shape[0], device=rows.device), (B, R, R, R))
    return grid if return_sparse else grid.to_dense()


def run_case(kind, name, level, D, reps):
    import torch
    import kaolin_amd as kal
    assert torch.cuda.is_available(), 'time_pointcloud.py measures on the GPU'
    g = torch.Generator().manual_seed(0)
    res = {'op': kind, 'input': name, 'reps': reps}
    if kind == 'spc':
        if name == 'sphere':
            pts = torch.randn((N, 3), generator=g)
            pts = 0.9 * pts / pts.norm(dim=1, keepdim=True)
        else:
            pts = torch.rand((N, 3), generator=g) * 0.9
        pts = pts.cuda()
        feats = torch.randn((N, D), generator=g).cuda() if D else None

        def hip():
            s = kal.ops.conversions.unbatched_pointcloud_to_spc(pts, level, feats)
            return s.octrees, s.features

        def user():
            return user_spc(pts, level, feats)

        def same(a, b):
            return torch.equal(a[0], b[0]) and (D == 0 or torch.allclose(a[1], b[1], rtol=1e-6, atol=1e-6))
        octree, out = hip()
        cells = out.shape[0] if D else None
        passes = (3 * level + 7) // 8
        traffic = N * 12 + N * D * 4 + octree.numel() + (cells * D * 4 if D else 0)
        res.update(points=N, level=level, D=D, cells=cells, octree_bytes=octree.numel(),
                   launches=11 + 4 * passes + 4 * level + (2 if D else 0), host_reads=1)
    else:
        B, P, R = 8, 1 << 17, level
        pts = torch.rand((B, P, 3), generator=g).cuda()
        sparse = name == 'sparse'

        def hip():
            return kal.ops.conversions.pointclouds_to_voxelgrids(pts, R, return_sparse=sparse)

        def user():
            return user_voxelgrids(pts, R, sparse)

        def same(a, b):
            if not sparse:
                return torch.equal(a, b)
            a, b = a.coalesce(), b.coalesce()
            return torch.equal(a.indices(), b.indices()) and torch.equal(a.values(), b.values())
        got = hip()
        nnz = int(got.sum()) if not sparse else got.coalesce().indices().shape[1]
        traffic = B * P * 12 + (B * R ** 3 * 4 if not sparse else nnz * 36)
        # the default origin and scale are torch reductions (4 launches) in front of the fill and the one kernel
        res.update(batch=B, points=P, resolution=R, voxels=nnz, launches=None if sparse else 2, host_reads=2 if sparse else 0)
    a, b = hip(), user()
    assert same(a, b), f'{kind} {name}: the yardstick differs from the HIP path'
    del a, b
    hip()
    user()
    torch.cuda.synchronize()
    for key, fn in (('hip', hip), ('user', user)):
        med, low = median_ms(fn, reps)
        res[f'{key}_ms'], res[f'{key}_min_ms'] = round(med, 4), round(low, 4)
    res.update(user_over_hip=round(res['user_ms'] / res['hip_ms'], 2), compulsory_bytes=traffic,
               bound_share=float(f'{traffic / HBM_BYTES_PER_S / (res["hip_ms"] * 1e-3):.3g}'))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    ap.add_argument('--case', type=int, default=None, help='(internal) run one case in this process')
    args = ap.parse_args()
    if args.case is not None:
        print(json.dumps(run_case(*CASES[args.case], max(args.reps, 5))), flush=True)
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
