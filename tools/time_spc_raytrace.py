"""Times kaolin.render.spc on one GPU: one JSON line per case.

    python tools/time_spc_raytrace.py [--reps 10] [--out profiles/spc_raytrace_time.jsonl]

The scene is the one of tools/time_spc.py: the level-9 octree of unbatched_mesh_to_spc for the bench's geodesic sphere (50 000
faces).  Rays: 1024 x 1024 perspective rays from a camera outside the volume that frames the sphere, in pixel order (and once
shuffled: what losing the coherence between neighbouring lanes costs), and 512 x 512 rays from a point inside the sphere.  Traced
without depths, with the entry depth and with entry and exit; then exponential_integration with 3 channels over the packs of the
outside trace.  Every case runs in a child process of its own under a time limit; the first failure ends the run.

Per case: `hip_ms` = the median over the repetitions of the public call between two device events, `torch_ms` = the same for the
package's torch formulation (the CPU path, run on the same GPU tensors), after checking with torch.equal that the two agree.  The
torch formulation is the yardstick: the parent commit has nothing to time and the reference does not run on this hardware.
`bound_ms` = the compulsory bytes (rays read once, results written once; for the integration its inputs and results) over the
achievable HBM bandwidth of 6.3 TB/s.  `launches` and `host_reads` are counted from the launch sequence of csrc/spc_raytrace.hip
and its shim."""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ACHIEVABLE_BPS = 6.3e12
LEVEL, CHANNELS = 9, 3
# (rays, return_depth, with_exit)
CASES = [('outside', False, False), ('outside', True, False), ('outside', True, True), ('outside_shuffled', True, False),
         ('inside', True, False), ('integration', True, False)]
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
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def camera_rays(side, eye, fov):
    """side x side perspective rays from `eye` towards the centre of the volume, pixel order (row-major)"""
    import torch
    eye = torch.tensor(eye, dtype=torch.float64)
    z = -eye / eye.norm() if float(eye.norm()) > 0 else torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    x = torch.linalg.cross(torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64), z)
    x = x / x.norm()
    y = torch.linalg.cross(z, x)
    s = (torch.arange(side, dtype=torch.float64) + 0.5) / side * 2.0 - 1.0
    v, u = torch.meshgrid(s, s, indexing='ij')
    d = z[None, None] + math.tan(0.5 * fov) * (u[..., None] * x + v[..., None] * y)
    d = (d / d.norm(dim=-1, keepdim=True)).reshape(-1, 3)
    return eye.float().expand(side * side, 3).contiguous().cuda(), d.float().contiguous().cuda()


def run_case(rays, return_depth, with_exit, reps):
    import torch
    import kaolin_amd as kal
    from kaolin_amd.ops.spc import spc as S
    from kaolin_amd.render.spc import raytrace as R
    from kaolin_amd.utils.testing import geodesic_sphere
    assert torch.cuda.is_available(), 'time_spc_raytrace.py measures on the GPU'
    v, f = geodesic_sphere(50)
    octree = kal.ops.conversions.unbatched_mesh_to_spc((v.float() * 1.2)[f].contiguous().cuda(), LEVEL)[0]
    lengths = torch.tensor([octree.numel()], dtype=torch.int32)
    _, pyramids, exsum = S.scan_octrees(octree, lengths)
    points = S.generate_points(octree, pyramids, exsum)
    pyramid = pyramids[0]
    if rays == 'inside':
        origin, direction = camera_rays(512, [0.1, 0.0, 0.2], math.radians(150))
        direction = -direction                                   # the camera looks away from the centre, through the near wall
    else:
        origin, direction = camera_rays(1024, [0.0, 0.0, -2.5], 2 * math.atan(0.65 / 2.5))
        if rays == 'outside_shuffled':
            perm = torch.randperm(origin.size(0), generator=torch.Generator().manual_seed(0)).cuda()
            origin, direction = origin[perm].contiguous(), direction[perm].contiguous()
    N = origin.size(0)
    res = {'op': 'exponential_integration' if rays == 'integration' else 'unbatched_raytrace', 'rays': rays, 'N': N, 'level': LEVEL,
           'octree_bytes': octree.numel(), 'points': points.size(0), 'reps': reps}
    if rays == 'integration':
        ridx, pidx, depth = R.unbatched_raytrace(octree, points, pyramid, exsum, origin, direction, LEVEL)
        n = ridx.numel()
        b = R.mark_pack_boundaries(ridx)
        g = torch.Generator().manual_seed(3)
        feats = torch.rand((n, CHANNELS), generator=g).cuda()
        tau = (torch.rand((n, 1), generator=g) * 0.5).cuda()
        packs = int(b.sum())
        res.update(hits=n, packs=packs, channels=CHANNELS)

        def hip():
            return R.exponential_integration(feats, tau, b)

        def torch_():
            alpha = 1.0 - torch.exp(-tau)
            tr = torch.exp(-1.0 * R._torch_pack_scan(tau, b, False, True, False)) * alpha
            return R._torch_pack_reduce(tr * feats, b, False), tr
        nbytes = n * (4 * CHANNELS + 4 + 1) + n * 4 + packs * 4 * CHANNELS
        launches, reads = 2, 1                                   # the scan and the reduction (+ torch's elementwise kernels)
    else:
        res.update(return_depth=return_depth, with_exit=with_exit)

        def hip():
            return R.unbatched_raytrace(octree, points, pyramid, exsum, origin, direction, LEVEL, return_depth, with_exit)

        def torch_():
            nuggets, depths = R._torch_raytrace(octree, points, exsum, origin, direction, LEVEL, return_depth, with_exit)
            return (nuggets[:, 0], nuggets[:, 1]) + ((depths,) if return_depth else ())
        launches, reads = 4, 1                                   # count, the 2-launch scan, emit; the hit total
    a, c = hip(), torch_()
    assert same(a, c), f'{rays}: the torch formulation differs from the HIP path'
    if rays != 'integration':
        hits = a[0].numel()
        res.update(hits=hits, rays_with_hits=int(torch.unique(a[0]).numel()))
        nbytes = 24 * N + 8 * hits + (4 * hits * (2 if with_exit else 1) if return_depth else 0)
    del a, c
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
    ap.add_argument('--reps', type=int, default=10)
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
