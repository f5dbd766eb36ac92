"""Generates tests/golden/subdivide_tetmesh.npz FROM THE REFERENCE ITSELF (kaolin.ops.mesh.subdivide_tetmesh and
inverse_vertices_offset).

Run in the build container (where the reference tree is mounted):
    python tests/golden/make_golden_subdivide_tetmesh.py
The reference's file is loaded by path on top of _refload's stub ``kaolin`` package (kaolin.ops.conversions.tetmesh first, for
its ``_sort_edges``); it is pure PyTorch and runs on the CPU.  Inputs hold values a float32 represents exactly, so they are
stored once, as float32, and the float64 runs use their widening.  Rows [0, V) of the reference's new_vertices / new_features
are its inputs bit for bit (asserted here), so per case and dtype d in {f32, f64} only the E midpoint rows are stored:
``<case>_mid_vertices_<d>`` (B, E, 3), ``<case>_mid_features_<d>`` (B, E, D), and the topology (asserted equal between the
dtypes and with / without features): ``<case>_new_tets`` (8 T, 4) for the small cases; for grid9 and sparse_ids
``<case>_slot_ids`` (T, 6), the new ids (ab ac ad bc bd cd) of every tet, from which ``child_blocks`` rebuilds the reference's
new_tetrahedrons exactly (asserted here; tests/subdivide_tetmesh_golden.py holds the same function) -- a quarter of the bytes.

  doc         the example of the reference's docstring
  kat1, kat2  inputs and expected tensors of the reference's own tests/python/kaolin/ops/mesh/test_tetmesh.py, read from its
              fixtures (``kat*_expected_*``): one tet, and the same tet twice; next to what the reference returns for them.
              ``ivo_*``: the known answer of inverse_vertices_offset from the same file and what the reference returns
  grid9       the 9^3 Kuhn grid of marching_tetrahedra.npz (``grid9_tets``: T = 4 444 tets in random order with permuted corners,
              50 duplicates, 20 tets with a repeated corner -> self-edges; V = 1 000).  B = 2: item 0 is ``grid9_vertices[0]``
              of that file (jittered), item 1 the plain grid ``kuhn_grid(9)``; neither is stored again.  D = 5 seeded features
              from {-1, -0.5, 0, 0.5, 1}; ``grid9_d1_*``: D = 1 (the first channel); the call without features is asserted to
              return the same vertices and tets
  sparse_ids  grid9's topology with the vertex ids mapped through the seeded injection ``sparse_ids_map`` of
              marching_tetrahedra.npz into [0, 70 001) (id 70 000 is used), its first 1 500 tets (the whole topology makes the
              file too large): the keys need a third byte per half.  B = 1, D = 5; the used ids carry grid9's item 1 and the
              features of item 0, the ids nobody uses are zero
  empty       T = 0 on grid9's vertices (``empty_*`` shapes)
  grads       for grid9 and sparse_ids: the reference's autograd gradients ``grads_<case>_{vertices,features}_<d>`` under the
              seeded cotangents ``grads_<case>_cot_{vertices,features}`` on both outputs, and ``..._tas``: per element the
              float64 sum of the magnitudes of the terms it accumulates, |g[v]| + 1/2 sum |g[V + e]| (asserted to bound the
              gradient).  For sparse_ids the cotangent rows of the unused ids follow ``unused_cotangent`` below and are not
              stored (stored: the rows of the 1 000 used ids in grid9's vertex order, then the E midpoint rows); the gradient
              rows of the unused ids are asserted to be exactly their cotangent
  dtypes_*    the dtypes the reference returns for half inputs, for int32 tetrahedrons and for float32 vertices with float64
              features
  err_*       type and text of what the reference raises for malformed arguments
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
SPARSE_T = 1500


def load_modules():
    _refload.load_reference()
    conv = _refload._load('kaolin.ops.conversions.tetmesh', 'kaolin/ops/conversions/tetmesh.py')
    sys.modules['kaolin.ops.conversions'].tetmesh = conv
    tm = _refload._load('kaolin.ops.mesh.tetmesh', 'kaolin/ops/mesh/tetmesh.py')
    sys.modules['kaolin.ops.mesh'].tetmesh = tm
    kat = _refload._load('ref_test_mesh_tetmesh', 'tests/python/kaolin/ops/mesh/test_tetmesh.py')
    return tm, kat


def record_error(out, name, fn):
    try:
        fn()
    except Exception as err:  # noqa: BLE001  (the reference's own error, whatever its type)
        out[f'err_{name}'] = np.array([type(err).__name__, str(err)])
        return
    print(f'err_{name}: the reference raised nothing; not recorded')


def unused_cotangent(rows, channels):
    """The cotangent of the sparse_ids rows nobody uses: a pattern of exact eighths (tests rebuild it from this rule)."""
    r = torch.arange(rows, dtype=torch.long).unsqueeze(1)
    c = torch.arange(channels, dtype=torch.long).unsqueeze(0)
    return ((r * 7 + c * 3) % 17 - 8).float() / 8


def halves(shape, g):
    """Seeded values from {-1, -0.5, 0, 0.5, 1}: sums of them are exact in float32, and the file stays small."""
    return (torch.randint(-2, 3, shape, generator=g).float() / 2)


def child_blocks(tets, slots):
    """new_tetrahedrons from the corners (a b c d) and the new ids (ab ac ad bc bd cd) of every tet: eight blocks of T rows.
    (tests/subdivide_tetmesh_golden.py holds a copy for decoding ``slot_ids``: keep the two in step.)"""
    a, b, c, d = tets.unbind(1)
    ab, ac, ad, bc, bd, cd = slots.unbind(1)
    rows = ((a, ab, ac, ad), (b, bc, ab, bd), (c, ac, bc, cd), (d, ad, cd, bd),
            (ab, ac, ad, bd), (ab, ac, bd, bc), (cd, ac, bd, ad), (cd, ac, bc, bd))
    return torch.cat([torch.stack(r, dim=1) for r in rows], dim=0)


def unique_edges(tets):
    pairs = torch.cat([tets[:, [i, j]] for i in range(4) for j in range(i + 1, 4)])
    return torch.unique(torch.sort(pairs, dim=1).values, dim=0)


def term_abs_sums(cot, edges, num_vertices):
    g = cot.double().abs()
    tas = g[:, :num_vertices].clone()
    tas.index_add_(1, edges[:, 0], 0.5 * g[:, num_vertices:])
    tas.index_add_(1, edges[:, 1], 0.5 * g[:, num_vertices:])
    return tas


def main():
    tm, kat = load_modules()
    mt = np.load(os.path.join(HERE, 'marching_tetrahedra.npz'))
    g = torch.Generator().manual_seed(20261)
    out = {}

    def run(case, vertices, tets, features, store_inputs=True):
        """Runs the reference in both dtypes, with and without features; stores the midpoint rows and the topology."""
        assert vertices.dtype == torch.float32 and tets.dtype == torch.long
        if store_inputs:
            out[f'{case}_vertices'], out[f'{case}_tets'] = vertices.numpy(), tets.numpy()
            if features is not None:
                out[f'{case}_features'] = features.numpy()
        V = vertices.shape[1]
        topo = None
        for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
            res = tm.subdivide_tetmesh(vertices.to(dt), tets) if features is None else \
                tm.subdivide_tetmesh(vertices.to(dt), tets, features.to(dt))
            assert len(res) == (2 if features is None else 3)
            assert res[0].dtype == dt and res[1].dtype == torch.long and res[1].shape == (8 * tets.shape[0], 4)
            assert torch.equal(res[0][:, :V], vertices.to(dt))                 # rows [0, V): the inputs, bit for bit
            mid = (vertices.to(dt)[:, unique_edges(tets)[:, 0]] + vertices.to(dt)[:, unique_edges(tets)[:, 1]]) * 0.5
            assert torch.equal(res[0][:, V:], mid)                             # one addition and an exact halving
            out[f'{case}_mid_vertices_{tag}'] = res[0][:, V:].numpy()
            if features is not None:
                assert res[2].dtype == dt and torch.equal(res[2][:, :V], features.to(dt))
                out[f'{case}_mid_features_{tag}'] = res[2][:, V:].numpy()
                bare = tm.subdivide_tetmesh(vertices.to(dt), tets)
                assert len(bare) == 2 and torch.equal(bare[0], res[0]) and torch.equal(bare[1], res[1])
            assert topo is None or torch.equal(topo, res[1])
            topo = res[1]
        if tets.shape[0] <= 16:
            out[f'{case}_new_tets'] = topo.numpy()
        else:
            # 8 T x 4 ids name only T x 10 different numbers.  Stored: the six new ids of every tet, read off the blocks
            # (a ab ac ad) (b bc ab bd) (c ac bc cd); asserted: the eight blocks rebuilt from them ARE the reference's result
            T = tets.shape[0]
            slots = torch.stack([topo[:T, 1], topo[:T, 2], topo[:T, 3], topo[T:2 * T, 1], topo[T:2 * T, 3], topo[2 * T:3 * T, 3]], dim=1)
            assert torch.equal(child_blocks(tets, slots), topo)
            out[f'{case}_slot_ids'] = slots.numpy().astype(np.int16 if int(slots.max()) < 2 ** 15 else np.int32)
        return topo

    # ---- doc ---------------------------------------------------------------------------------------------------------------
    run('doc', torch.tensor([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]], dtype=torch.float), torch.tensor([[0, 1, 2, 3]]),
        torch.tensor([[[-1.], [-1.], [0.5], [0.5]]]))

    # ---- kat: the reference's own test, its fixtures read as data ----------------------------------------------------------
    t = kat.TestSubdivideTetmesh()
    fx = {n: getattr(kat.TestSubdivideTetmesh, n).__wrapped__(t, 'cpu') for n in
          ('vertices_single_tet', 'faces_single_tet', 'expected_vertices_single_tet', 'expected_faces_single_tet',
           'faces_two_tets', 'expected_faces_two_tets', 'features_single_tet', 'expected_features_single_tet')}
    run('kat1', fx['vertices_single_tet'], fx['faces_single_tet'], fx['features_single_tet'])
    run('kat2', fx['vertices_single_tet'], fx['faces_two_tets'], fx['features_single_tet'])
    t.test_subdivide_tetmesh_no_features(fx['vertices_single_tet'], fx['faces_single_tet'], fx['expected_vertices_single_tet'],
                                         fx['expected_faces_single_tet'], fx['features_single_tet'],
                                         fx['expected_features_single_tet'])
    t.test_subdivide_tetmesh_shared_verts(fx['vertices_single_tet'], fx['faces_two_tets'], fx['expected_vertices_single_tet'],
                                          fx['expected_faces_two_tets'], fx['features_single_tet'],
                                          fx['expected_features_single_tet'])
    out['kat_expected_vertices'] = fx['expected_vertices_single_tet'].numpy()
    out['kat_expected_features'] = fx['expected_features_single_tet'].numpy()
    out['kat1_expected_tets'] = fx['expected_faces_single_tet'].numpy()
    out['kat2_expected_tets'] = fx['expected_faces_two_tets'].numpy()
    ivo_in = torch.tensor([[[[-0.0500, 0.0000, 0.0500], [-0.0250, -0.0500, 0.0000], [0.0000, 0.0000, 0.0500],
                             [0.5000, 0.5000, 0.4500]]]])
    ivo_known = torch.tensor([[[[0.0000, 20.0000, 0.0000], [79.9999, -149.9999, 10.0000], [-99.9999, 159.9998, -10.0000]]]])
    ivo = tm.inverse_vertices_offset(ivo_in)
    assert torch.allclose(ivo, ivo_known, rtol=1e-4)
    out['ivo_tet_vertices'], out['ivo_known'], out['ivo_reference'] = ivo_in.numpy(), ivo_known.numpy(), ivo.numpy()
    for name, bad in (('ivo_ndim', torch.zeros(2, 2)), ('ivo_dim2', torch.zeros(1, 2, 3, 3)), ('ivo_dim3', torch.zeros(1, 2, 4, 2))):
        record_error(out, name, lambda bad=bad: tm.inverse_vertices_offset(bad))

    # ---- grid9 -----------------------------------------------------------------------------------------------------------
    gv0 = torch.from_numpy(mt['grid9_vertices'])[0]
    gt = torch.from_numpy(mt['grid9_tets'])
    assert gt.shape == (4444, 4) and gv0.shape == (1000, 3)
    gv = torch.stack([gv0, kuhn_grid(9)[0]])
    gf = halves((2, 1000, 5), g)
    topo = run('grid9', gv, gt, gf, store_inputs=False)
    out['grid9_features'] = gf.numpy()
    edges = unique_edges(gt)
    E = edges.shape[0]
    assert int((edges[:, 0] == edges[:, 1]).sum()) > 0                          # self-edges of the degenerate tets
    assert int(topo.max()) == 1000 + E - 1
    d1 = tm.subdivide_tetmesh(gv, gt, gf[..., :1])
    assert torch.equal(d1[1], topo) and d1[2].shape == (2, 1000 + E, 1)
    out['grid9_d1_mid_features_f32'] = d1[2][:, 1000:].numpy()
    out['grid9_d1_mid_features_f64'] = tm.subdivide_tetmesh(gv.double(), gt, gf[..., :1].double())[2][:, 1000:].numpy()

    # ---- sparse_ids ------------------------------------------------------------------------------------------------------
    id_map = torch.from_numpy(mt['sparse_ids_map'])
    st = torch.from_numpy(mt['sparse_ids_tets'])
    assert torch.equal(st, id_map[gt]) and int(id_map.max()) == SPARSE_V - 1
    st = st[:SPARSE_T]                                                           # (the whole topology makes the file too large)
    sv, sf = torch.zeros(1, SPARSE_V, 3), torch.zeros(1, SPARSE_V, 5)
    sv[0, id_map], sf[0, id_map] = gv[1], gf[0]                                  # (the unjittered positions: a small file)
    run('sparse_ids', sv, st, sf, store_inputs=False)
    sedges = unique_edges(st)
    Es = sedges.shape[0]
    assert int(sedges[:, 0].max()) >= 2 ** 16 and int(sedges[:, 1].max()) == SPARSE_V - 1

    # ---- empty -----------------------------------------------------------------------------------------------------------
    for feats in (None, gf):
        res = tm.subdivide_tetmesh(gv, gt[:0]) if feats is None else tm.subdivide_tetmesh(gv, gt[:0], feats)
        assert torch.equal(res[0], gv) and res[1].shape == (0, 4) and res[1].dtype == torch.long
        assert feats is None or torch.equal(res[2], feats)
    out['empty_new_tets'] = res[1].numpy()

    # ---- grads -----------------------------------------------------------------------------------------------------------
    for case, (vertices, tets, feats, rows, ed) in {'grid9': (gv, gt, gf, None, edges), 'sparse_ids': (sv, st, sf, id_map, sedges)}.items():
        B, V = vertices.shape[:2]
        if rows is None:
            cot_v = halves((B, V + E, 3), g)
            cot_f = halves((B, V + E, 5), g)
            out[f'grads_{case}_cot_vertices'], out[f'grads_{case}_cot_features'] = cot_v.numpy(), cot_f.numpy()
        else:
            used_v = halves((B, 1000 + Es, 3), g)
            used_f = halves((B, 1000 + Es, 5), g)
            out[f'grads_{case}_cot_vertices'], out[f'grads_{case}_cot_features'] = used_v.numpy(), used_f.numpy()
            cot_v = torch.cat([unused_cotangent(V, 3)[None], used_v[:, 1000:]], dim=1)            # (V + Es rows)
            cot_f = torch.cat([unused_cotangent(V, 5)[None], used_f[:, 1000:]], dim=1)
            cot_v[0, rows], cot_f[0, rows] = used_v[0, :1000], used_f[0, :1000]
        for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
            p, f = vertices.clone().to(dt).requires_grad_(), feats.clone().to(dt).requires_grad_()
            nv, _, nf = tm.subdivide_tetmesh(p, tets, f)
            ((nv * cot_v.to(dt)).sum() + (nf * cot_f.to(dt)).sum()).backward()
            gp, gfe = p.grad, f.grad
            if rows is not None:
                rest = torch.ones(V, dtype=torch.bool)
                rest[rows] = False
                assert torch.equal(gp[0, rest], cot_v[0, :V][rest].to(dt)) and torch.equal(gfe[0, rest], cot_f[0, :V][rest].to(dt))
                gp, gfe = gp[:, rows], gfe[:, rows]
            out[f'grads_{case}_vertices_{tag}'], out[f'grads_{case}_features_{tag}'] = gp.numpy(), gfe.numpy()
        tv, tf = term_abs_sums(cot_v, ed, V), term_abs_sums(cot_f, ed, V)
        if rows is not None:
            tv, tf = tv[:, rows], tf[:, rows]
        assert bool((tv + 1e-300 >= torch.from_numpy(out[f'grads_{case}_vertices_f64']).abs() * (1 - 1e-9)).all())
        assert bool((tf + 1e-300 >= torch.from_numpy(out[f'grads_{case}_features_f64']).abs() * (1 - 1e-9)).all())
        out[f'grads_{case}_vertices_tas'], out[f'grads_{case}_features_tas'] = tv.numpy(), tf.numpy()

    # ---- dtypes ----------------------------------------------------------------------------------------------------------
    def dtypes(name, *args):
        try:
            res = tm.subdivide_tetmesh(*args)
        except Exception as err:  # noqa: BLE001
            print(f'dtypes_{name}: the reference raised {type(err).__name__}: {err}; not recorded')
            return
        out[f'dtypes_{name}'] = np.array([str(r.dtype) for r in res])

    dtypes('half', gv.half(), gt, gf.half())
    dtypes('int32_tets', gv, gt.int(), gf)
    dtypes('mixed', gv, gt, gf.double())

    # ---- errors ----------------------------------------------------------------------------------------------------------
    ev, et, ef = gv[:, :8], torch.tensor([[0, 1, 2, 3], [4, 5, 6, 7]]), gf[:, :8]
    record_error(out, 'tets_width', lambda: tm.subdivide_tetmesh(ev, et[:, :3], ef))
    record_error(out, 'tets_float', lambda: tm.subdivide_tetmesh(ev, et.float(), ef))
    record_error(out, 'features_rows', lambda: tm.subdivide_tetmesh(ev, et, ef[:, :7]))

    path = os.path.join(HERE, 'subdivide_tetmesh.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != 'subdivide_tetmesh.npz')
    assert size < largest, (size, largest)
    print('wrote subdivide_tetmesh.npz', len(out), 'arrays', size, 'bytes; grid9:', E, 'edges; sparse_ids:', Es, 'edges')
    for k in sorted(out):
        if k.startswith('err_') or k.startswith('dtypes_'):
            print(k, list(out[k]))


if __name__ == '__main__':
    main()
