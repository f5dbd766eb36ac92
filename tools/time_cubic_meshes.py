"""Times kaolin.ops.conversions.voxelgrids_to_cubic_meshes on one GPU: one JSON line per (grid, dtype, is_trimesh, B).

    python tools/time_cubic_meshes.py [--reps 20] [--out profiles/cubic_meshes_time.jsonl]

Grids: `sphere256` = the bench's geodesic sphere (50 000 faces) through trianglemeshes_to_voxelgrids at 256^3 and
ops.voxelgrid.fill; `rand128` = a seeded random 128^3 grid with p = 0.5, the worst case for the face count (half of all voxel
faces are exposed).  Input float32 and bool, both is_trimesh values, B = 1 and 8 (the same grid repeated).  Every case runs in
a child process of its own under a time limit; the first failure ends the run.

Per case, three implementations on the same GPU and the same input, results compared with torch.equal before anything is
timed:
  `hip_ms`        the public call on the HIP pipeline (csrc/cubic_meshes.hip),
  `torch_ms`      the package's torch formulation of the same prefix-count pipeline (flags, cumsum, gathers: the CPU path, run
                  on the GPU tensor),
  `reference_ms`  the reference's algorithm restated here (conv3d, nonzero, four corners per face, one torch.unique(dim=0) per
                  item), at most 3 repetitions.
Each is the median over the repetitions of the whole call between two device events (every one of the three synchronises to
read its sizes back).  From a second, separately profiled set of calls (the library's per-kernel events, kamd_profile_enable)
come the mean times of the four stages.  `bound_ms` = the compulsory bytes -- the grid read once, the vertices and faces
written once -- over the achievable HBM bandwidth of 6.3 TB/s (8 TB/s peak); `bound_over_hip` = bound_ms / hip_ms, and
`bound_over_kernels` = bound_ms over the summed kernel time alone.
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
CASES = [(g, d, t, n) for g in ('sphere256', 'rand128') for d in ('float32', 'bool') for t in (True, False) for n in (1, 8)]
CASE_TIME_LIMIT_S = 240
KERNELS = ('cm_classify_kernel', 'cm_scan(scan + bases)', 'cm_vertices_kernel', 'cm_faces_kernel')


def make_grid(name, dtype, n):
    import torch
    import kaolin_amd as kal
    if name == 'rand128':
        g = torch.Generator().manual_seed(128)
        grid = (torch.rand((1, 128, 128, 128), generator=g) < 0.5).cuda()
    else:
        from kaolin_amd.utils.testing import geodesic_sphere
        v, f = geodesic_sphere(50)
        grid = kal.ops.voxelgrid.fill(kal.ops.conversions.trianglemeshes_to_voxelgrids(v.float()[None].cuda(), f.cuda(), 256))
    return grid.to(getattr(torch, dtype)).expand(n, -1, -1, -1).contiguous()


def reference_algorithm(voxelgrids, is_trimesh):
    """The reference's way to the same answer, written out from its description: signed face indicators from a 2-tap difference
    per axis over the zero-padded grid (as a conv3d), their non-zero positions, four float corners per face, and per item a
    torch.unique over the corner rows whose inverse mapping numbers the vertices."""
    import torch
    dev = voxelgrids.device
    taps = torch.zeros((3, 1, 2, 2, 2), device=dev)
    taps[:, 0, 0, 0, 0] = -1
    taps[0, 0, 1, 0, 0] = taps[1, 0, 0, 1, 0] = taps[2, 0, 0, 0, 1] = 1
    signed = torch.nn.functional.conv3d(voxelgrids.float().unsqueeze(1), taps, padding=1).round().transpose(0, 1)
    axis, item, x, y, z = torch.nonzero(signed, as_tuple=True)
    reverse = signed[axis, item, x, y, z] == -1
    corner = torch.tensor([[[0, -1, -1], [0, 0, -1], [0, -1, 0], [0, 0, 0]],
                           [[-1, 0, -1], [-1, 0, 0], [0, 0, -1], [0, 0, 0]],
                           [[-1, -1, 0], [0, -1, 0], [-1, 0, 0], [0, 0, 0]]], dtype=torch.float, device=dev)
    corners = corner[axis] + torch.stack([x, y, z], -1).unsqueeze(1).float()          # (faces, 4, 3)
    verts_out, faces_out = [], []
    for b in range(voxelgrids.shape[0]):
        mine = item == b
        rows = corners[mine].reshape(-1, 3)
        n = rows.shape[0] // 4
        quads = torch.arange(4 * n, device=dev).view(n, 4)[:, [0, 1, 3, 2]]
        quads = torch.where(reverse[mine].unsqueeze(1), quads.flip(1), quads)
        faces = torch.cat([quads[:, [0, 3, 1]], quads[:, [2, 1, 3]]]) if is_trimesh else quads
        if n == 0:
            verts_out.append(rows)
            faces_out.append(faces)
            continue
        verts, inverse = torch.unique(rows, return_inverse=True, dim=0)
        verts_out.append(verts)
        faces_out.append(inverse[faces])
    return verts_out, faces_out


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


def run_case(name, dtype, is_trimesh, n, reps):
    import torch
    from kaolin_amd import _lib
    from kaolin_amd.ops.conversions.voxelgrid import _cubic_meshes_torch, voxelgrids_to_cubic_meshes
    assert torch.cuda.is_available(), 'time_cubic_meshes.py measures on the GPU'
    lib = _lib.load()
    x = make_grid(name, dtype, n)
    impls = {'hip': lambda: voxelgrids_to_cubic_meshes(x, is_trimesh), 'torch': lambda: _cubic_meshes_torch(x, is_trimesh),
             'reference': lambda: reference_algorithm(x, is_trimesh)}
    out = impls['hip']()
    for other in ('torch', 'reference'):
        got = impls[other]()
        same = all(torch.equal(a, b) for a, b in zip(out[0] + out[1], got[0] + got[1]))
        assert same and len(got[0]) == n, f'{other} differs from the HIP path'
        del got
    for _ in range(2):
        impls['hip']()
        impls['torch']()
    torch.cuda.synchronize()
    res = {'grid': name, 'dtype': dtype, 'is_trimesh': is_trimesh, 'B': n, 'reps': reps}
    for key, fn in impls.items():
        med, low = median_ms(fn, reps if key != 'reference' else min(reps, 3))
        res[f'{key}_ms'], res[f'{key}_min_ms'] = round(med, 4), round(low, 4)
    lib.kamd_profile_reset()
    lib.kamd_profile_select(-1)
    lib.kamd_profile_enable(1)
    for _ in range(5):
        impls['hip']()
    torch.cuda.synchronize()
    lib.kamd_profile_enable(0)
    prof = _lib.kernel_profile(reset=True)
    kern = {k: prof[k][0] / 5 for k in KERNELS}                                         # ms per call
    nbytes = x.numel() * x.element_size() + sum(t.numel() * t.element_size() for t in out[0] + out[1])
    bound = nbytes / ACHIEVABLE_BPS * 1e3
    res.update(classify_ms=round(kern[KERNELS[0]], 4), scan_ms=round(kern[KERNELS[1]], 4), vertices_ms=round(kern[KERNELS[2]], 4),
               faces_ms=round(kern[KERNELS[3]], 4), bound_ms=round(bound, 4), bound_over_hip=round(bound / res['hip_ms'], 4),
               bound_over_kernels=round(bound / sum(kern.values()), 4), torch_over_hip=round(res['torch_ms'] / res['hip_ms'], 2),
               reference_over_hip=round(res['reference_ms'] / res['hip_ms'], 2),
               vertices=out[0][0].shape[0], faces=out[1][0].shape[0])
    return res


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
