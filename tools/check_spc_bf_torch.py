"""Compares the torch formulations of the Bayesian-fusion operators (kaolin_amd/ops/spc/bf_torch.py) with the HIP path on a large
frame, call by call.

    python tools/check_spc_bf_torch.py [--frames 2] [--level 8]

Input: the 100 000 random Gaussians of tools/time_spc_bf.py, voxelised at `--level` and ray traced from the densifier's default
viewpoints (seed 0); a frame of level 8 has about 8.5 M final-level points.  For every frame, `processFrame` runs three times with
every operator's outputs recorded: through the HIP operators, through the torch formulations on the same GPU tensors with their
chunks of 2^20 points, and through the torch formulations on GPU tensors IN ONE PIECE (`bf_torch._CHUNK` lifted).  The first
operator call whose outputs differ from the HIP path's is reported, with the verdict of the formulations on CPU tensors for that
call.  Exit status 0 when the chunked formulation equals the HIP path on every call of every frame.

Why it exists: in one piece, on GPU tensors of this size, `oracleB_final`'s formulation has been seen to return zeros in some
probabilities, where the HIP path, the chunked formulation and the formulation on CPU tensors agree on every point.  The kernels
are not involved; the formulations are therefore chunked, and this tool is the reproducer for whoever looks into the operation on
the large intermediates that goes wrong."""
import argparse
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    import torch
    import time_spc_bf as T
    import kaolin_amd as kal
    from kaolin_amd.ops.gaussians import densifier
    from kaolin_amd.ops.spc import bf_recon as bfr
    from kaolin_amd.ops.spc import bf_torch
    from kaolin_amd.ops.spc.raytraced_spc_dataset import RayTracedSPCDataset
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2)
    ap.add_argument('--level', type=int, default=8)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'check_spc_bf_torch.py compares on the GPU'
    level = args.level
    xyz, scales, rots, opacities = T.make_inputs('random100k', level)
    torch.manual_seed(0)
    viewpoints = densifier._generate_default_viewpoints()
    cen = 0.5 * (xyz.min(0).values + xyz.max(0).values)
    dmax = 0.5 * (xyz.max(0).values - xyz.min(0).values).max() + 0.05
    voxels, merged = kal.ops.conversions.gs_to_voxelgrid((xyz - cen) / dmax, scales / dmax, rots, opacities, level, iso=11.345,
                                                         tol=0.125, step=10)
    ds = RayTracedSPCDataset(viewpoints, kal.ops.spc.unbatched_points_to_octree(voxels[merged >= 0.35].contiguous(), level))
    names = list(T.LAUNCHES)
    real_ops, chunk = bfr._ops, bf_torch._CHUNK

    def run(batch, ops, device, one_piece=False):
        log = []

        def wrap(name):
            def call(*a, **kw):
                out = getattr(ops, name)(*a, **kw)
                log.append((name, [o.detach().cpu() for o in (out if isinstance(out, (tuple, list)) else (out,))]))
                return out
            return call
        table = types.SimpleNamespace(**{**vars(ops), **{n: wrap(n) for n in names}})
        bfr._ops = lambda t: table
        bf_torch._CHUNK = 1 << 62 if one_piece else chunk
        fresh = tuple(x.clone().to(device) if k in (0, 1, 8) else x for k, x in enumerate(batch))
        try:
            bfr.processFrame(fresh, level, 0.0005)
        except bfr.BFReconstructionTerminatedException:
            pass
        finally:
            bfr._ops, bf_torch._CHUNK = real_ops, chunk
        return log

    def first_difference(a, b):
        for k, ((name, x), (_, y)) in enumerate(zip(a, b)):
            if any(p.shape != q.shape or not torch.equal(p, q) for p, q in zip(x, y)):
                return k, name
        return None

    status, done = 0, 0
    for i in range(len(ds)):
        batch = ds[i]
        if not batch[9]:
            continue
        hip = run(batch, kal._C.ops.spc, 'cuda')
        for label, one_piece in (('in chunks', False), ('in one piece', True)):
            diff = first_difference(hip, run(batch, bf_torch.ops, 'cuda', one_piece))
            line = f'frame {i}, torch formulation on GPU tensors {label}: '
            if diff is None:
                print(line + f'equals the HIP path on all {len(hip)} calls', flush=True)
                continue
            k, name = diff
            cpu = run(batch, bf_torch.ops, 'cpu')
            agrees = all(p.shape == q.shape and torch.equal(p, q) for p, q in zip(hip[k][1], cpu[k][1]))
            print(line + f'call {k} ({name}) differs from the HIP path; the formulation on CPU tensors '
                  f'{"agrees" if agrees else "DISAGREES"} with the HIP path there', flush=True)
            if not one_piece:
                status = 1
        done += 1
        if done >= args.frames:
            break
    return status


if __name__ == '__main__':
    sys.exit(main())
