"""Generates tests/golden/flexicubes.npz FROM THE REFERENCE ITSELF (kaolin.ops.conversions.FlexiCubes).

Run in the build container (where the reference tree is mounted):
    python tests/golden/make_golden_flexicubes.py
The reference's files are loaded by path on top of _refload's stub ``kaolin`` package; FlexiCubes is pure PyTorch and runs on the
CPU with ``FlexiCubes(device='cpu')``.  Every input is built here (seeded) and holds values a float32 represents exactly, so it is
stored once, as float32.  Each case runs in float32 and again in float64 under ``torch.set_default_dtype(torch.float64)`` (the
reference allocates with the default dtype); integer results are asserted equal between the two runs and stored once.  Per case
``<case>_{vertices,sdf,cubes,res}`` and, where given, ``<case>_{beta,alpha,gamma}``; results ``<case>[_train]_verts_{f32,f64}``,
``<case>[_train]_ldev_{f32,f64}``, ``<case>[_train]_faces``.

  cases256    resolution 1, the 256 sign patterns as 256 calls (bit k set iff sdf(corner k) < 0): jittered corners, eight distinct
              |sdf|, random beta / alpha.  No faces (no edge has four cubes): vertices and L_dev of all calls one after the other,
              ``cases256_nv`` / ``cases256_nl`` the counts per call.  Pins group order and slot order.
  invert<i>   small grids with random signs, found by a seeded search that stops once the set covers: marked cubes that invert
              across an x, a y and a z face; a marked cube next to an unmarked one; a marked cube whose neighbour is outside the
              grid; a marked cube whose neighbour is marked in another direction (and inverts it all the same: only possible
              when the cubes do not share their vertices, so that grid has 8 private vertices per cube).
              ``invert_count`` grids
  grid        resolution (5, 3, 4), jittered vertices, an off-centre sphere plus noise (cubes of 1, 2 and 3 dual vertices), random beta / alpha / gamma_f, training both ways;
              every quad has |g0 g2 - g1 g3| >= 1e-3 (normalised gammas, float64)
  defaults    the same with beta = alpha = gamma_f = None (float64 run: beta = alpha = 0, which normalise to exactly 1 -- the
              reference's own defaults do not run in float64)
  zeros       resolution 3: exact 0.0 on a third of the vertices, one -0.0, a NaN on the outer end of a crossed edge
  empty_pos / empty_neg   resolution 2, one sign everywhere
  features    grid with 5 channels: ``features_feats_{f32,f64}`` (training=False only: with training=True the reference fails
              in its own ``torch.cat`` of the centre features)
  grads       the reference's autograd gradients for grid, training=True: ``grads_{vertices,sdf,beta,alpha,gamma}_{f32,f64}``
              under the seeded cotangents ``grads_cot_verts`` / ``grads_cot_ldev``; the latter is zero where L_dev is below
              1e-2 of its median: there the derivative sign(dist - mean) hangs on rounding.  Raw weights are 0.5 randn
  err_*       type and text of what the reference raises for wrong argument shapes
  construct_* ``construct_voxel_grid`` at 1, 4 and (5, 3, 4): ``construct_<i>_{verts,cubes}``
Asserted: every crossed edge without a NaN has |s0| + |s1| >= 1e-2 median |sdf| (the zero-crossing's denominator).
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import _refload  # noqa: E402
from kaolin_amd.ops.conversions.flexicubes import flexicubes as ours  # noqa: E402

EDGES = torch.tensor(ours.CUBE_EDGES)


def load_reference():
    _refload.load_reference()
    # two imports of the reference's utils/testing.py that check_tensor never touches
    for name in ('kaolin.ops.spc.uint8', 'kaolin.ops.random'):
        parent, _, leaf = name.rpartition('.')
        sys.modules[name] = types.ModuleType(name)
        setattr(sys.modules[parent], leaf, sys.modules[name])
    testing = _refload._load('kaolin.utils.testing', 'kaolin/utils/testing.py')
    sys.modules['kaolin.utils'].testing = testing
    _refload._pkg('kaolin.ops.conversions.flexicubes')
    _refload._load('kaolin.ops.conversions.flexicubes.tables', 'kaolin/ops/conversions/flexicubes/tables.py')
    return _refload._load('kaolin.ops.conversions.flexicubes.flexicubes', 'kaolin/ops/conversions/flexicubes/flexicubes.py')


def exact(t, step=1.0 / 4096):
    """Rounds to multiples of a power of two: values a float32 holds exactly."""
    return (torch.round(t.double() / step) * step).float()


def record_error(out, name, fn):
    try:
        fn()
    except Exception as err:  # noqa: BLE001  (the reference's own error, whatever its type)
        out[f'err_{name}'] = np.array([type(err).__name__, str(err)])
        return
    raise AssertionError(f'{name}: the reference raised nothing')


def check_conditioning(sdf, cubes):
    a, b = cubes[:, EDGES[:, 0]].reshape(-1), cubes[:, EDGES[:, 1]].reshape(-1)
    s0, s1 = sdf[a].double(), sdf[b].double()
    crossed = ((s0 < 0) != (s1 < 0)) & ~torch.isnan(s0) & ~torch.isnan(s1)
    if bool(crossed.any()):
        floor = 1e-2 * float(sdf[~torch.isnan(sdf)].abs().median())
        assert float((s0.abs() + s1.abs())[crossed].min()) >= floor, 'ill-conditioned crossed edge: change the seed'


def main():
    mod = load_reference()
    g = torch.Generator().manual_seed(20261)
    out = {}

    def call(dt, verts, sdf, cubes, res, beta=None, alpha=None, gamma=None, training=False, feats=None, grad=False):
        torch.set_default_dtype(dt)
        try:
            fc = mod.FlexiCubes(device='cpu')
            cast = [None if t is None else t.to(dt).clone().requires_grad_(grad) for t in (verts, sdf, beta, alpha, gamma, feats)]
            res_arg = list(res) if isinstance(res, (tuple, list)) else res
            result = fc(cast[0], cast[1], cubes, res_arg, beta=cast[2], alpha=cast[3], gamma_f=cast[4], training=training,
                        voxelgrid_features=cast[5])
            return result, cast
        finally:
            torch.set_default_dtype(torch.float32)

    def run(case, verts, sdf, cubes, res, beta=None, alpha=None, gamma=None, trainings=(False,), feats=None, store=True,
            conditioned=True):
        assert verts.dtype == torch.float32 and sdf.dtype == torch.float32 and cubes.dtype == torch.long
        if conditioned:
            check_conditioning(sdf, cubes)
        if store:
            out[f'{case}_vertices'], out[f'{case}_sdf'], out[f'{case}_cubes'] = verts.numpy(), sdf.numpy(), cubes.numpy()
            out[f'{case}_res'] = np.array(res if isinstance(res, (tuple, list)) else [res] * 3)
            for name, t in (('beta', beta), ('alpha', alpha), ('gamma', gamma), ('feats', feats)):
                if t is not None:
                    out[f'{case}_{name}'] = t.numpy()
        results = {}
        for training in trainings:
            tag = f'{case}_train' if training else case
            r32, _ = call(torch.float32, verts, sdf, cubes, res, beta, alpha, gamma, training, feats)
            # the reference's default beta / alpha are float32 whatever the default dtype and its float64 index_add_ refuses them:
            # the float64 run of a case without weights passes zeros, which normalise to exactly 1
            zeros = [torch.zeros(cubes.shape[0], n) if t is None else t for t, n in ((beta, 12), (alpha, 8))]
            r64, _ = call(torch.float64, verts, sdf, cubes, res, zeros[0], zeros[1], gamma, training, feats)
            assert r32[0].dtype == torch.float32 and r64[0].dtype == torch.float64 and r32[1].dtype == torch.long
            assert torch.equal(r32[1], r64[1]) and r32[0].shape == r64[0].shape and r32[2].shape == r64[2].shape
            out[f'{tag}_faces'] = r32[1].numpy()
            for d, r in (('f32', r32), ('f64', r64)):
                out[f'{tag}_verts_{d}'], out[f'{tag}_ldev_{d}'] = r[0].detach().numpy(), r[2].detach().numpy()
                if feats is not None:
                    out[f'{tag}_feats_{d}'] = r[3].detach().numpy()
            results[training] = r32
        return results

    fc = mod.FlexiCubes(device='cpu')

    # ---- construct_voxel_grid ----------------------------------------------------------------------------------------------
    for i, res in enumerate((1, 4, (5, 3, 4))):
        v, c = fc.construct_voxel_grid(res)
        assert v.dtype == torch.float32 and c.dtype == torch.long
        out[f'construct_{i}_verts'], out[f'construct_{i}_cubes'] = v.numpy(), c.numpy()

    # ---- cases256 ----------------------------------------------------------------------------------------------------------
    v1, c1 = fc.construct_voxel_grid(1)
    v1 = exact(v1 + (torch.rand(v1.shape, generator=g) - 0.5) * 0.2)
    mag = torch.tensor([0.75, 1.25, 0.5, 2.0, 1.0, 1.5, 0.625, 1.75])
    beta1, alpha1 = exact(0.5 * torch.randn(1, 12, generator=g)), exact(0.5 * torch.randn(1, 8, generator=g))
    out['cases256_vertices'], out['cases256_mag'], out['cases256_cubes'] = v1.numpy(), mag.numpy(), c1.numpy()
    out['cases256_beta'], out['cases256_alpha'] = beta1.numpy(), alpha1.numpy()
    parts = {k: [] for k in ('verts_f32', 'verts_f64', 'ldev_f32', 'ldev_f64')}
    nv, nl = [], []
    for case in range(256):
        bits = (case >> torch.arange(8)) & 1
        sdf = torch.where(bits.bool(), -mag, mag)
        sdf = torch.zeros(8).scatter(0, c1[0], sdf)                     # corner k -> its vertex id
        r32, _ = call(torch.float32, v1, sdf, c1, 1, beta1, alpha1)
        r64, _ = call(torch.float64, v1, sdf, c1, 1, beta1, alpha1)
        assert r32[1].shape == (0, 3) and r64[1].shape == (0, 3) and r32[0].shape == r64[0].shape
        assert r32[0].shape[0] == int(fc.num_vd_table[case]) and (r32[0].shape[0] == 0) == (case in (0, 255))
        assert torch.unique(r32[0], dim=0).shape[0] == r32[0].shape[0]
        nv.append(r32[0].shape[0])
        nl.append(r32[2].shape[0])
        for d, r in (('f32', r32), ('f64', r64)):
            parts[f'verts_{d}'].append(r[0].numpy())
            parts[f'ldev_{d}'].append(r[2].numpy())
    out['cases256_nv'], out['cases256_nl'] = np.array(nv), np.array(nl)
    for k, v in parts.items():
        out[f'cases256_{k}'] = np.concatenate(v)

    # ---- invert: a seeded search for sign patterns that cover the situations of the ambiguity rule ----------------------------
    check = fc.check_table
    wanted = {'invert_x', 'invert_y', 'invert_z', 'beside_unmarked', 'beside_outside', 'other_direction'}
    count = 0
    for attempt in range(20000):
        if not wanted:
            break
        res = ((3, 2, 2), (2, 3, 2), (2, 2, 3))[attempt % 3]
        v, c = fc.construct_voxel_grid(res)
        if wanted == {'other_direction'}:
            # cubes that share a face agree on its four corners, so the neighbour of a marked cube can only be marked back at
            # it; with private corners per cube (no shared vertices) the rule's quirk shows
            v, c = v[c.reshape(-1)], torch.arange(c.numel()).reshape(-1, 8)
        sign = torch.where(torch.rand(v.shape[0], generator=g) < 0.65, -1.0, 1.0)
        mags = exact(0.25 + 0.75 * torch.rand(v.shape[0], generator=g), 1.0 / 64)
        case = ((sign[c] < 0).long() << torch.arange(8)).sum(1)
        row = check[case]
        lin = torch.arange(c.shape[0])
        pos = torch.stack([lin // (res[1] * res[2]), (lin // res[2]) % res[1], lin % res[2]], 1)
        found = set()
        for n in torch.nonzero(row[:, 0] == 1).reshape(-1).tolist():
            q = pos[n] + row[n, 1:4]
            if bool((q < 0).any()) or bool((q >= torch.tensor(res)).any()):
                found.add('beside_outside')
                continue
            m = int((q[0] * res[1] + q[1]) * res[2] + q[2])
            if int(row[m, 0]) != 1:
                found.add('beside_unmarked')
            elif bool((row[m, 1:4] == -row[n, 1:4]).all()):
                found.add('invert_' + 'xyz'[int(torch.nonzero(row[n, 1:4]).reshape(-1)[0])])
            else:
                found.add('other_direction')
        if found & wanted:
            wanted -= found
            vj = exact(v + (torch.rand(v.shape, generator=g) - 0.5) * 0.08)
            run(f'invert{count}', vj, sign * mags, c, res, exact(0.5 * torch.randn(c.shape[0], 12, generator=g)),
                exact(0.5 * torch.randn(c.shape[0], 8, generator=g)), exact(0.5 * torch.randn(c.shape[0], generator=g)))
            count += 1
    assert not wanted, wanted
    out['invert_count'] = np.array(count)

    # ---- grid, defaults, features, grads --------------------------------------------------------------------------------------
    res = (5, 3, 4)
    v, c = fc.construct_voxel_grid(res)
    for attempt in range(100):
        vj = exact(v + (torch.rand(v.shape, generator=g) - 0.5) * torch.tensor([0.06, 0.1, 0.07]))
        sdf = exact((vj - torch.tensor([0.05, -0.04, 0.03])).norm(dim=-1) - 0.37 + 0.06 * torch.randn(v.shape[0], generator=g))
        beta, alpha = exact(0.5 * torch.randn(c.shape[0], 12, generator=g)), exact(0.5 * torch.randn(c.shape[0], 8, generator=g))
        gamma = exact(0.5 * torch.randn(c.shape[0], generator=g))
        topo = ours.topology_torch(sdf, c, res)
        gn = (torch.sigmoid(gamma.double()) * 0.99 + 0.005)[topo['cubes'][topo['vd_cube']]][topo['quads']]
        classes = set(fc.num_vd_table[((sdf[c] < 0).long() << torch.arange(8)).sum(1)].tolist())
        try:
            check_conditioning(sdf, c)
        except AssertionError:
            continue
        if float((gn[:, 0] * gn[:, 2] - gn[:, 1] * gn[:, 3]).abs().min()) >= 1e-3 and classes >= {1, 2, 3}:
            break
    else:
        raise AssertionError('no seed with a clear quad split')
    r = run('grid', vj, sdf, c, res, beta, alpha, gamma, trainings=(False, True))
    nvd = topo['vd_cube'].shape[0]
    assert torch.equal(r[True][1].reshape(-1, 4, 3)[:, :, 0], topo['quads']) and r[False][0].shape[0] == nvd
    run('defaults', vj, sdf, c, res, trainings=(False, True), store=False)
    feats = exact(torch.randn(v.shape[0], 5, generator=g))
    run('features', vj, sdf, c, res, beta, alpha, gamma, feats=feats, store=False)
    out['features_feats'] = feats.numpy()

    cot_v = exact(torch.rand(r[True][0].shape, generator=g) * 2 - 1)
    cot_l = exact(torch.rand(r[True][2].shape, generator=g) * 2 - 1)
    l64 = torch.from_numpy(out['grid_train_ldev_f64'])
    cot_l[l64 < 1e-2 * float(l64.median())] = 0.0               # (there sign(dist - mean), L_dev's derivative, hangs on rounding)
    assert 0 < int((cot_l == 0).sum()) < 10
    out['grads_cot_verts'], out['grads_cot_ldev'] = cot_v.numpy(), cot_l.numpy()
    for d, dt in (('f32', torch.float32), ('f64', torch.float64)):
        res_d, leaves = call(dt, vj, sdf, c, res, beta, alpha, gamma, True, grad=True)
        ((res_d[0] * cot_v.to(dt)).sum() + (res_d[2] * cot_l.to(dt)).sum()).backward()
        for name, leaf in zip(('vertices', 'sdf', 'beta', 'alpha', 'gamma'), leaves):
            out[f'grads_{name}_{d}'] = leaf.grad.numpy()

    # ---- zeros ---------------------------------------------------------------------------------------------------------------
    vz, cz = fc.construct_voxel_grid(3)
    vz = exact(vz + (torch.rand(vz.shape, generator=g) - 0.5) * 0.05)
    sz = exact((vz - torch.tensor([0.1, 0.05, -0.08])).norm(dim=-1) - 0.4)
    sz[torch.randperm(sz.shape[0], generator=g)[:sz.shape[0] // 3]] = 0.0
    zero_ids = torch.nonzero(sz == 0).reshape(-1)
    sz[zero_ids[0]] = -0.0
    a, b = cz[:, EDGES[:, 0]].reshape(-1), cz[:, EDGES[:, 1]].reshape(-1)
    crossed = torch.nonzero(((sz[a] < 0) != (sz[b] < 0)) & (sz[a] != 0) & (sz[b] != 0)).reshape(-1)
    pick = int(crossed[int(torch.randint(0, crossed.shape[0], (1,), generator=g))])
    nan_vertex = int(a[pick] if sz[a[pick]] > 0 else b[pick])           # the outer end: it stays outside as NaN
    sz[nan_vertex] = float('nan')
    assert bool(torch.signbit(sz[zero_ids[0]])) and int((sz == 0).sum()) >= sz.shape[0] // 3 - 1
    rz = run('zeros', vz, sz, cz, 3, exact(0.5 * torch.randn(27, 12, generator=g)), exact(0.5 * torch.randn(27, 8, generator=g)),
             exact(0.5 * torch.randn(27, generator=g)), trainings=(False, True))
    assert bool(torch.isnan(rz[False][0]).any())

    # ---- empty ---------------------------------------------------------------------------------------------------------------
    ve, ce = fc.construct_voxel_grid(2)
    for name, value in (('empty_pos', 0.5), ('empty_neg', -0.5)):
        re_ = run(name, ve, torch.full((27,), value), ce, 2)
        assert re_[False][0].shape == (0, 3) and re_[False][1].shape == (0, 3) and re_[False][2].shape == (0,)

    # ---- errors --------------------------------------------------------------------------------------------------------------
    nc = c.shape[0]
    record_error(out, 'vertices', lambda: fc(vj[:, :2], sdf, c, res))
    record_error(out, 'sdf', lambda: fc(vj, sdf[:-1], c, res))
    record_error(out, 'cubes', lambda: fc(vj, sdf, c[:, :7], res))
    record_error(out, 'beta', lambda: fc(vj, sdf, c, res, beta=torch.zeros(nc, 11)))
    record_error(out, 'alpha', lambda: fc(vj, sdf, c, res, alpha=torch.zeros(nc - 1, 8)))
    record_error(out, 'gamma', lambda: fc(vj, sdf, c, res, gamma_f=torch.zeros(nc, 1)))
    record_error(out, 'features', lambda: fc(vj, sdf, c, res, voxelgrid_features=feats[:-1]))
    record_error(out, 'features_tetmesh', lambda: fc(vj, sdf, c, res, voxelgrid_features=feats, output_tetmesh=True))

    path = os.path.join(HERE, 'flexicubes.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != 'flexicubes.npz')
    assert size <= largest, (size, largest)
    print('wrote flexicubes.npz', len(out), 'arrays', size, 'bytes;', 'grid:', nvd, 'dual vertices', topo['quads'].shape[0],
          'quads;', count, 'invert grids')
    for k in sorted(out):
        if k.startswith('err_'):
            print(k, list(out[k]))


if __name__ == '__main__':
    main()
