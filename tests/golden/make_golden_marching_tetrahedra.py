"""Generates tests/golden/marching_tetrahedra.npz FROM THE REFERENCE ITSELF (kaolin.ops.conversions.marching_tetrahedra).

Run in the build container (where the reference tree is mounted):
    python tests/golden/make_golden_marching_tetrahedra.py
The reference's file is loaded by path on top of _refload's stub ``kaolin`` package; it is pure PyTorch and runs on the CPU.
Every input is built here (seeded where random) and holds values a float32 represents exactly, so it is stored once, as
float32, and the float64 runs use its widening.  Per case ``<case>_vertices`` (B, V, 3), ``<case>_tets`` (T, 4),
``<case>_sdf`` (B, V) and, per item b and dtype d in {f32, f64}, the reference's ``<case>_verts_<b>_<d>``,
``<case>_faces_<b>`` and ``<case>_tet_idx_<b>`` (the two integer results are asserted equal between the dtypes).

  cases16     one tet, the 16 sign patterns as 16 batch items (item c has corner k occupied iff bit k of c); positions
              without symmetry and four distinct |sdf|, so that no two output vertices coincide.  Items 0 and 15 are empty
  doc         the example of the reference's docstring
  kat         inputs and expected tensors of the reference's own tests/python/kaolin/ops/conversions/test_tetmesh.py, read
              from its fixtures (``kat_expected_*``), next to what the reference returns for them
  zeros_nan   4^3 Kuhn grid: exact zeros on a third of the vertices, one -0.0, one NaN on a vertex of a crossing edge (the
              expected vertices hold that NaN)
  grid9       9^3 Kuhn grid (4 374 tets, 1 000 vertices), jittered; sdf = an off-centre sphere.  Tets randomly permuted, the
              corners of each tet randomly permuted, 50 tets duplicated, 20 degenerate tets with a repeated corner.  B = 2:
              item 1 is positive everywhere (empty result)
  sparse_ids  grid9's topology, vertex ids mapped through a seeded injection ``sparse_ids_map`` into [0, 70 001) (id 70 000
              is used): V = 70 001, the vertices nobody uses are zeros with sdf -1.  Stored: the map, the tets and the results
  grads       for grid9 item 0 and sparse_ids: the reference's autograd gradients ``grads_<case>_vertices_<d>`` /
              ``grads_<case>_sdf_<d>`` under the seeded cotangent ``grads_<case>_cotangent`` (given in the order of that
              case's output vertices), and ``grads_<case>_{vertices,sdf}_tas``: per element the sum of the magnitudes of the
              terms it accumulates, in float64, from
                  d = s_a - s_b, v = (p_a (-s_b) + p_b s_a) / d:
                  grad p_a += (-s_b / d) g, grad p_b += (s_a / d) g, grad s_a += g.(p_b - v) / d, grad s_b += g.(v - p_a) / d
              (for sparse_ids the rows of the 1 000 used ids, in grid9's vertex order; every other row is zero).
              Asserted: every crossing edge has |s_a - s_b| >= 1e-2 median |sdf|.
  err_*       type and text of what the reference raises for wrong argument shapes / types
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import _refload  # noqa: E402
from kaolin_amd.utils.testing import kuhn_grid  # noqa: E402

SPARSE_V = 70001


def load_modules():
    _refload.load_reference()
    tm = _refload._load('kaolin.ops.conversions.tetmesh', 'kaolin/ops/conversions/tetmesh.py')
    sys.modules['kaolin.ops.conversions'].tetmesh = tm
    kat = _refload._load('ref_test_tetmesh', 'tests/python/kaolin/ops/conversions/test_tetmesh.py')
    return tm, kat


def record_error(out, name, fn):
    try:
        fn()
    except Exception as err:  # noqa: BLE001  (the reference's own error, whatever its type)
        out[f'err_{name}'] = np.array([type(err).__name__, str(err)])
        return
    raise AssertionError(f'{name}: the reference raised nothing')


def sphere_sdf(vertices, centre, radius):
    return (radius - (vertices - torch.tensor(centre, dtype=vertices.dtype)).norm(dim=-1)).float()


def grid9_case(g):
    vertices, tets = kuhn_grid(9)
    vertices = (vertices + (torch.rand(vertices.shape, generator=g) - 0.5) * 0.03).float()
    tets = tets[torch.randperm(tets.shape[0], generator=g)]
    tets = torch.cat([tets, tets[torch.randperm(tets.shape[0], generator=g)[:50]]])
    degenerate = tets[torch.randperm(tets.shape[0], generator=g)[:20]].clone()
    degenerate[:, 3] = degenerate[:, 1]
    tets = torch.cat([tets, degenerate])
    tets = tets[torch.randperm(tets.shape[0], generator=g)]
    corner_order = torch.rand(tets.shape, generator=g).argsort(dim=1)
    tets = torch.gather(tets, 1, corner_order)
    sdf0 = sphere_sdf(vertices, (0.47, 0.55, 0.42), 0.337)
    sdf1 = sdf0.abs() + 0.05
    return vertices[None].expand(2, -1, -1).contiguous(), tets, torch.stack([sdf0, sdf1])


def crossing_edges(tets, sdf):
    """(a, b), a < b: the unique edges of the tets with exactly one end occupied, ascending (for the generator's checks)."""
    occ = sdf > 0
    pairs = torch.cat([tets[:, [i, j]] for i in range(4) for j in range(i + 1, 4)])
    pairs = pairs[occ[pairs[:, 0]] != occ[pairs[:, 1]]]
    pairs = torch.unique(torch.sort(pairs, dim=1).values, dim=0)
    return pairs[:, 0], pairs[:, 1]


def term_abs_sums(vertices, tets, sdf, cot):
    p, s, g = vertices.double(), sdf.double(), cot.double()
    a, b = crossing_edges(tets, sdf)
    d = s[a] - s[b]
    v = (p[a] * (-s[b]).unsqueeze(1) + p[b] * s[a].unsqueeze(1)) / d.unsqueeze(1)
    tv = torch.zeros_like(p)
    ts = torch.zeros_like(s)
    tv.index_add_(0, a, ((-s[b] / d).unsqueeze(1) * g).abs())
    tv.index_add_(0, b, ((s[a] / d).unsqueeze(1) * g).abs())
    ts.index_add_(0, a, ((g * (p[b] - v)).abs().sum(1) / d.abs()))
    ts.index_add_(0, b, ((g * (v - p[a])).abs().sum(1) / d.abs()))
    return tv, ts


def main():
    tm, kat = load_modules()
    g = torch.Generator().manual_seed(20260)
    out = {}

    def run(case, vertices, tets, sdf, store_inputs=True):
        if store_inputs:
            out[f'{case}_vertices'], out[f'{case}_tets'], out[f'{case}_sdf'] = vertices.numpy(), tets.numpy(), sdf.numpy()
        assert vertices.dtype == torch.float32 and sdf.dtype == torch.float32 and tets.dtype == torch.long
        res = {}
        for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
            verts, faces, tet_idx = tm.marching_tetrahedra(vertices.to(dt), tets, sdf.to(dt), True)
            res[tag] = (verts, faces, tet_idx)
            for b in range(vertices.shape[0]):
                assert verts[b].dtype == dt and faces[b].dtype == torch.long and tet_idx[b].dtype == torch.long
                out[f'{case}_verts_{b}_{tag}'] = verts[b].numpy()
        for b in range(vertices.shape[0]):
            assert torch.equal(res['f32'][1][b], res['f64'][1][b]) and torch.equal(res['f32'][2][b], res['f64'][2][b])
            out[f'{case}_faces_{b}'] = res['f32'][1][b].numpy()
            out[f'{case}_tet_idx_{b}'] = res['f32'][2][b].numpy()
        return res['f32']

    # ---- cases16 ---------------------------------------------------------------------------------------------------------
    v1 = torch.tensor([[0.0625, 0.125, 0.03125], [1.25, 0.1875, -0.0625], [0.3125, 1.5, 0.21875], [0.15625, 0.4375, 1.75]])
    mag = torch.tensor([0.75, 1.25, 0.5, 2.0])
    bits = (torch.arange(16).unsqueeze(1) >> torch.arange(4)) & 1
    sdf16 = torch.where(bits.bool(), mag, -mag)
    verts, faces, _ = run('cases16', v1[None].expand(16, -1, -1).contiguous(), torch.tensor([[0, 1, 2, 3]]), sdf16)
    for c in range(16):
        n = {0: 0, 4: 0, 1: 3, 3: 3, 2: 4}[int(bits[c].sum())]
        assert verts[c].shape == (n, 3) and torch.unique(verts[c], dim=0).shape[0] == n
        assert faces[c].shape == ({0: 0, 3: 1, 4: 2}[n], 3)

    # ---- doc ---------------------------------------------------------------------------------------------------------------
    run('doc', torch.tensor([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]], dtype=torch.float),
        torch.tensor([[0, 1, 2, 3]]), torch.tensor([[-1., -1., 0.5, 0.5]]))

    # ---- kat: the reference's own test, its fixtures read as data ----------------------------------------------------------
    t = kat.TestMarchingTetrahedra()
    fx = {n: getattr(kat.TestMarchingTetrahedra, n).__wrapped__ for n in
          ('vertices', 'tets', 'sdf', 'expected_verts', 'expected_faces', 'expected_tet_idx')}
    kv, kt, ks = fx['vertices'](t, 'cpu').contiguous(), fx['tets'](t, 'cpu'), fx['sdf'](t, 'cpu')
    run('kat', kv, kt, ks)
    t.test_output_value(kv, kt, ks, fx['expected_verts'](t, 'cpu'), fx['expected_faces'](t, 'cpu'), fx['expected_tet_idx'](t, 'cpu'))
    for b in range(4):
        out[f'kat_expected_verts_{b}'] = fx['expected_verts'](t, 'cpu')[b].numpy()
        out[f'kat_expected_faces_{b}'] = fx['expected_faces'](t, 'cpu')[b].numpy()
        out[f'kat_expected_tet_idx_{b}'] = fx['expected_tet_idx'](t, 'cpu')[b].numpy()

    # ---- zeros_nan -------------------------------------------------------------------------------------------------------
    zv, zt = kuhn_grid(4)
    zs = sphere_sdf(zv, (0.4, 0.55, 0.45), 0.36)
    zs[torch.randperm(zs.shape[0], generator=g)[:zs.shape[0] // 3]] = 0.0
    a, b = crossing_edges(zt, zs)
    pick = int(torch.randint(0, a.shape[0], (1,), generator=g))
    nan_vertex = int(a[pick] if zs[a[pick]] <= 0 else b[pick])        # the unoccupied end: it stays unoccupied as NaN
    zs[nan_vertex] = float('nan')
    zero_ids = torch.nonzero(zs == 0).reshape(-1)
    zs[zero_ids[0]] = -0.0
    assert int((zs == 0).sum()) >= zs.shape[0] // 3 - 2 and bool(torch.signbit(zs[zero_ids[0]]))
    verts, _, _ = run('zeros_nan', zv[None].contiguous(), zt, zs[None].contiguous())
    assert bool(torch.isnan(verts[0]).any())
    a, b = crossing_edges(zt, zs)
    assert bool(((a == nan_vertex) | (b == nan_vertex)).any()) and verts[0].shape[0] == a.shape[0]

    # ---- grid9 -----------------------------------------------------------------------------------------------------------
    gv, gt, gs = grid9_case(g)
    assert gt.shape == (4374 + 70, 4) and gv.shape == (2, 1000, 3)
    verts, faces, tet_idx = run('grid9', gv, gt, gs)
    assert verts[1].shape == (0, 3) and faces[1].shape == (0, 3) and tet_idx[1].shape == (0,)
    occ = gs[0] > 0
    cases = ((occ[gt]).long() << torch.arange(4)).sum(1)
    assert sorted(torch.unique(cases).tolist()) == list(range(16))
    a, b = crossing_edges(gt, gs[0])
    assert verts[0].shape[0] == a.shape[0]
    threshold = 1e-2 * float(gs[0].abs().median())
    assert float((gs[0][a] - gs[0][b]).abs().min()) >= threshold, 'ill-conditioned crossing edge: change the seed / the offset'

    # ---- sparse_ids ------------------------------------------------------------------------------------------------------
    id_map = torch.randperm(SPARSE_V - 1, generator=g)[:1000]
    id_map[int(a[int(torch.randint(0, a.shape[0], (1,), generator=g))])] = SPARSE_V - 1     # an end of a crossing edge
    assert torch.unique(id_map).shape[0] == 1000 and int(id_map.max()) == SPARSE_V - 1
    sv = torch.zeros(SPARSE_V, 3)
    sv[id_map] = gv[0]
    ss = torch.full((SPARSE_V,), -1.0)
    ss[id_map] = gs[0]
    st = id_map[gt]
    out['sparse_ids_map'], out['sparse_ids_tets'] = id_map.numpy(), st.numpy()
    sverts, sfaces, _ = run('sparse_ids', sv[None], st, ss[None], store_inputs=False)
    assert sverts[0].shape == verts[0].shape and sfaces[0].shape == faces[0].shape
    a, b = crossing_edges(st, ss)
    assert int(a.max()) >= 2 ** 16 and int(b.max()) == SPARSE_V - 1      # keys need more than 16 bits per half

    # ---- grads -----------------------------------------------------------------------------------------------------------
    for case, (vertices, tets, sdf, rows) in {'grid9': (gv[0], gt, gs[0], None), 'sparse_ids': (sv, st, ss, id_map)}.items():
        nv = out[f'{case}_verts_0_f32'].shape[0]
        cot = (torch.rand(nv, 3, generator=g) * 2 - 1).float()
        out[f'grads_{case}_cotangent'] = cot.numpy()
        for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
            p, s = vertices.clone().to(dt).requires_grad_(), sdf.clone().to(dt).requires_grad_()
            verts, _ = tm.marching_tetrahedra(p[None], tets, s[None])
            (verts[0] * cot.to(dt)).sum().backward()
            gp, gsd = p.grad, s.grad
            if rows is not None:
                rest = torch.ones(vertices.shape[0], dtype=torch.bool)
                rest[rows] = False
                assert not bool(gp[rest].any()) and not bool(gsd[rest].any())
                gp, gsd = gp[rows], gsd[rows]
            out[f'grads_{case}_vertices_{tag}'], out[f'grads_{case}_sdf_{tag}'] = gp.numpy(), gsd.numpy()
        tv, ts = term_abs_sums(vertices, tets, sdf, cot)
        if rows is not None:
            tv, ts = tv[rows], ts[rows]
        assert bool((tv + 1e-300 >= torch.from_numpy(out[f'grads_{case}_vertices_f64']).abs() * (1 - 1e-9)).all())
        assert bool((ts + 1e-300 >= torch.from_numpy(out[f'grads_{case}_sdf_f64']).abs() * (1 - 1e-9)).all())
        out[f'grads_{case}_vertices_tas'], out[f'grads_{case}_sdf_tas'] = tv.numpy(), ts.numpy()

    # ---- errors ----------------------------------------------------------------------------------------------------------
    ev, et, es = gv[:, :8], torch.tensor([[0, 1, 2, 3], [4, 5, 6, 7]]), gs[:, :8]
    record_error(out, 'sdf_unbatched', lambda: tm.marching_tetrahedra(ev, et, es[0]))
    record_error(out, 'sdf_batch', lambda: tm.marching_tetrahedra(ev, et, es[:1]))
    record_error(out, 'tets_width', lambda: tm.marching_tetrahedra(ev, et[:, :3], es))
    record_error(out, 'tets_float', lambda: tm.marching_tetrahedra(ev, et.float(), es))

    path = os.path.join(HERE, 'marching_tetrahedra.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != 'marching_tetrahedra.npz')
    assert size < largest, (size, largest)
    print('wrote marching_tetrahedra.npz', len(out), 'arrays', size, 'bytes;', 'grid9 item 0:',
          out['grid9_verts_0_f32'].shape[0], 'vertices', out['grid9_faces_0'].shape[0], 'faces')
    for k in sorted(out):
        if k.startswith('err_'):
            print(k, list(out[k]))


if __name__ == '__main__':
    main()
