"""Generates tests/golden/sample_points.npz FROM THE REFERENCE ITSELF (kaolin.ops.mesh.face_areas, packed_face_areas,
_base_sample_points_selected_faces of kaolin/ops/mesh/trianglemesh.py, pure PyTorch, on the CPU).

Run in the build container (where the reference tree is mounted):
    python tests/golden/make_golden_sample_points.py
Inputs hold values a float32 represents exactly: they are stored once, as float32, and the float64 runs use their widening.
``<d>`` is f32 or f64.

  tables      the inputs of the reference's own TestFaceAreas, recorded while its tests run here against the reference (the calls'
              arguments ``tables_{areas,packed}_*``, the reference's results ``*_out_<d>`` and what the tests compare them with,
              ``*_expected_<d>``)
  ico         a jittered icosphere (320 faces) + one degenerate face (a repeated vertex) + one duplicated face, B = 2 (item 1 is
              item 0 scaled and shifted): ``ico_vertices``, ``ico_faces``, the reference's ``ico_areas_<d>``; the same mesh packed
              as two items with their own faces: ``ico_packed_*`` and ``ico_packed_areas_<d>``
  *_ieee_<d>  torch's CPU sqrt is not correctly rounded everywhere (built on MKL's vector maths: one unit in the last place off for
              about 0.6 % of its arguments).  Next to what the reference returns as it stands, ``ico_areas_ieee_<d>``,
              ``ico_packed_areas_ieee_<d>``, ``blend_points_ieee_<d>`` and ``blend_feats_ieee_<d>`` hold what the reference's code
              returns with its ``torch.sqrt`` replaced by the correctly rounded root (numpy's) and nothing else changed: the values
              the contract defines
  blend       _base_sample_points_selected_faces on recorded inputs: ``blend_choices`` (B, N) seeded face choices on ico, the two
              draws of the reference's ``torch.rand`` recorded through a wrapper (``blend_u_<d>``: the argument of its sqrt,
              ``blend_v_<d>``), ``blend_features`` (B, F, 3, 2), the reference's ``blend_points_<d>`` and ``blend_feats_<d>``
  grads       float64 autograd of the reference under seeded cotangents of exact halves: ``grads_areas_cot`` -> ``grads_areas_
              vertices`` (face_areas on ico: NaN at the vertices of the degenerate face) and ``grads_blend_cot_{points,feats}`` ->
              ``grads_blend_{vertices,features}`` (the blend with the recorded draws replayed, through the reference's gathers)
  cases       the reference's TestSamplePoints as data: its fixtures ``cases_*``, and per call of sample_points /
              packed_sample_points made by its tests (run here against the reference) the number of samples and the shapes and
              dtypes of the results: ``cases_calls`` (rows of strings)
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
from kaolin_amd.utils import testing as T  # noqa: E402

DTYPES = (('f32', torch.float32), ('f64', torch.float64))
REAL_SQRT = torch.sqrt


def ieee_sqrt(t):
    """the correctly rounded square root (numpy's: the hardware instruction), as a stand-in for torch.sqrt on detached CPU tensors"""
    with np.errstate(invalid='ignore'):
        return torch.from_numpy(np.sqrt(t.numpy()))


class ieee_root:
    """Runs the reference with its torch.sqrt replaced by the correctly rounded one: torch's CPU sqrt, built on MKL's vector maths,
    is one unit in the last place off for about 0.6 % of its arguments"""

    def __enter__(self):
        torch.sqrt = ieee_sqrt

    def __exit__(self, *exc):
        torch.sqrt = REAL_SQRT


def load_modules():
    mods = _refload.load_reference()
    tm = mods['ops_trianglemesh']
    batch = _refload._load('kaolin.ops.batch', 'kaolin/ops/batch.py')
    for name in ('tile_to_packed', 'packed_to_padded', 'get_first_idx'):
        setattr(tm, name, getattr(batch, name))
    kaolin = sys.modules['kaolin']
    kaolin.ops = sys.modules['kaolin.ops']
    kaolin.ops.mesh = sys.modules['kaolin.ops.mesh']
    kaolin.ops.batch = batch
    sys.modules['kaolin.utils.testing'] = T
    for name in ('face_areas', 'packed_face_areas', 'sample_points', 'packed_sample_points', 'face_normals',
                 'index_vertices_by_faces'):
        setattr(kaolin.ops.mesh, name, getattr(tm, name) if hasattr(tm, name) else None)
    mesh_py = _refload._load('ref_ops_mesh_mesh', 'kaolin/ops/mesh/mesh.py')
    kaolin.ops.mesh.index_vertices_by_faces = mesh_py.index_vertices_by_faces
    tests = _refload._load('ref_test_trianglemesh', 'tests/python/kaolin/ops/mesh/test_trianglemesh.py')
    return tm, tests


class Recorder:
    """Wraps a function of kaolin.ops.mesh: keeps the arguments and the result of every call"""

    def __init__(self, fn):
        self.fn, self.calls = fn, []

    def __call__(self, *args, **kwargs):
        out = self.fn(*args, **kwargs)
        self.calls.append((args, kwargs, out))
        return out


def ico_mesh(g):
    v, f = T.geodesic_sphere(4)
    v, f = torch.as_tensor(v).float(), torch.as_tensor(f).long()
    v = (v + (torch.rand(v.shape, generator=g) - 0.5) * 0.02).float()
    assert f.shape == (320, 3)
    degenerate = f[17].clone()
    degenerate[2] = degenerate[0]
    f = torch.cat([f[:100], degenerate[None], f[100:], f[41:42]])
    v = torch.stack([v, (v * 1.5 + torch.tensor([0.25, -0.5, 1.0])).float()])
    return v, f


def main():
    tm, tests = load_modules()
    kaolin = sys.modules['kaolin']
    g = torch.Generator().manual_seed(20261)
    out = {}

    # ---- tables: the reference's TestFaceAreas, run against the reference with its calls and comparisons recorded ---------------
    for tag, dt in DTYPES:
        rec_a, rec_p = Recorder(tm.face_areas), Recorder(tm.packed_face_areas)
        kaolin.ops.mesh.face_areas, kaolin.ops.mesh.packed_face_areas = rec_a, rec_p
        compared = []
        real_equal, real_close = torch.equal, tests.check_allclose
        torch.equal = lambda a, b: (compared.append(b), real_equal(a, b))[1]
        tests.check_allclose = lambda a, b, **kw: (compared.append(b), real_close(a, b, **kw))[1]
        try:
            t = tests.TestFaceAreas()
            t.test_face_areas('cpu', dt)
            t.test_packed_face_areas('cpu', dt)
        finally:
            torch.equal, tests.check_allclose = real_equal, real_close
        (args_a, _, out_a), = rec_a.calls
        (args_p, _, out_p), = rec_p.calls
        assert len(compared) == 2 and out_a.dtype == dt and out_p.dtype == dt
        if tag == 'f32':
            out['tables_areas_vertices'], out['tables_areas_faces'] = args_a[0].numpy(), args_a[1].numpy()
            out['tables_packed_vertices'], out['tables_packed_first_idx_vertices'] = args_p[0].numpy(), args_p[1].numpy()
            out['tables_packed_faces'], out['tables_packed_num_faces_per_mesh'] = args_p[2].numpy(), args_p[3].numpy()
        out[f'tables_areas_out_{tag}'], out[f'tables_areas_expected_{tag}'] = out_a.numpy(), compared[0].numpy()
        out[f'tables_packed_out_{tag}'], out[f'tables_packed_expected_{tag}'] = out_p.numpy(), compared[1].numpy()
    kaolin.ops.mesh.face_areas, kaolin.ops.mesh.packed_face_areas = tm.face_areas, tm.packed_face_areas

    # ---- ico ---------------------------------------------------------------------------------------------------------------------
    iv, iface = ico_mesh(g)
    B, V, F = iv.shape[0], iv.shape[1], iface.shape[0]
    out['ico_vertices'], out['ico_faces'] = iv.numpy(), iface.numpy()
    for tag, dt in DTYPES:
        areas = tm.face_areas(iv.to(dt), iface)
        assert areas.dtype == dt and float(areas[0, 100]) == 0.0 and torch.equal(areas[:, 41], areas[:, -1])
        out[f'ico_areas_{tag}'] = areas.numpy()
        with ieee_root():
            out[f'ico_areas_ieee_{tag}'] = tm.face_areas(iv.to(dt), iface).numpy()
        off = out[f'ico_areas_{tag}'] != out[f'ico_areas_ieee_{tag}']
        assert int(off.sum()) <= 0.02 * off.size
        assert np.allclose(out[f'ico_areas_{tag}'], out[f'ico_areas_ieee_{tag}'], rtol=2.0 ** (-22 if tag == 'f32' else -51), atol=0)
    # packed: item 0 = the first 150 faces on the vertices of batch item 0, item 1 = the rest on the vertices of batch item 1
    pv = torch.cat([iv[0], iv[1]])
    first_idx_vertices, num_faces_per_mesh = torch.LongTensor([0, V, 2 * V]), torch.LongTensor([150, F - 150])
    out['ico_packed_vertices'], out['ico_packed_first_idx_vertices'] = pv.numpy(), first_idx_vertices.numpy()
    out['ico_packed_num_faces_per_mesh'] = num_faces_per_mesh.numpy()
    for tag, dt in DTYPES:
        areas = tm.packed_face_areas(pv.to(dt), first_idx_vertices, iface, num_faces_per_mesh)
        assert torch.equal(areas[:150], torch.from_numpy(out[f'ico_areas_{tag}'])[0, :150])
        assert torch.equal(areas[150:], torch.from_numpy(out[f'ico_areas_{tag}'])[1, 150:])
        out[f'ico_packed_areas_{tag}'] = areas.numpy()
        with ieee_root():
            out[f'ico_packed_areas_ieee_{tag}'] = tm.packed_face_areas(pv.to(dt), first_idx_vertices, iface, num_faces_per_mesh).numpy()

    # ---- blend: the reference's blend on recorded inputs; its two torch.rand calls recorded ------------------------------------
    N, D = 97, 2
    choices = torch.randint(0, F, (B, N), generator=g)
    feats = (torch.randint(-8, 9, (B, F, 3, D), generator=g).float() / 4)
    out['blend_choices'], out['blend_features'] = choices.numpy(), feats.numpy()

    def gathered(vertices, features):
        corners = tuple(torch.gather(torch.index_select(vertices, 1, iface[:, k]), 1, choices.unsqueeze(-1).repeat(1, 1, 3))
                        for k in range(3))
        chosen = torch.gather(features, 1, choices[..., None, None].repeat(1, 1, 3, D))
        return corners, tuple(chosen[:, :, k] for k in range(3))

    real_rand = torch.rand
    draws = {}
    for tag, dt in DTYPES:
        drawn = []
        torch.rand = lambda *a, **kw: (drawn.append(real_rand(*a, **kw, generator=g)), drawn[-1])[1]
        try:
            points, bfeats = tm._base_sample_points_selected_faces(*gathered(iv.to(dt), feats.to(dt)))
        finally:
            torch.rand = real_rand
        assert len(drawn) == 2 and all(d.shape == (B, N, 1) and d.dtype == dt for d in drawn) and points.dtype == dt
        draws[tag] = drawn
        out[f'blend_u_{tag}'], out[f'blend_v_{tag}'] = drawn[0].squeeze(-1).numpy(), drawn[1].squeeze(-1).numpy()
        out[f'blend_points_{tag}'], out[f'blend_feats_{tag}'] = points.numpy(), bfeats.numpy()
        replay = list(drawn)
        torch.rand = lambda *a, **kw: replay.pop(0)
        try:
            with ieee_root():
                points, bfeats = tm._base_sample_points_selected_faces(*gathered(iv.to(dt), feats.to(dt)))
        finally:
            torch.rand = real_rand
        out[f'blend_points_ieee_{tag}'], out[f'blend_feats_ieee_{tag}'] = points.numpy(), bfeats.numpy()

    # ---- grads (float64) ---------------------------------------------------------------------------------------------------------
    halves = lambda *shape: (torch.randint(-4, 5, shape, generator=g).double() / 2)  # noqa: E731
    cot = halves(B, F)
    p = iv.double().requires_grad_()
    (tm.face_areas(p, iface) * cot).sum().backward()
    degenerate_vertices = torch.unique(iface[100])
    rest = torch.ones(V, dtype=torch.bool)
    rest[degenerate_vertices] = False
    assert bool(torch.isnan(p.grad[:, degenerate_vertices]).all()) and bool(torch.isfinite(p.grad[:, rest]).all())
    out['grads_areas_cot'], out['grads_areas_vertices'] = cot.numpy(), p.grad.numpy()

    cot_p, cot_f = halves(B, N, 3), halves(B, N, D)
    p, q = iv.double().requires_grad_(), feats.double().requires_grad_()
    replay = list(draws['f64'])
    torch.rand = lambda *a, **kw: replay.pop(0)
    try:
        points, bfeats = tm._base_sample_points_selected_faces(*gathered(p, q))
    finally:
        torch.rand = real_rand
    assert torch.equal(points.detach(), torch.from_numpy(out['blend_points_f64']))
    ((points * cot_p).sum() + (bfeats * cot_f).sum()).backward()
    out['grads_blend_cot_points'], out['grads_blend_cot_feats'] = cot_p.numpy(), cot_f.numpy()
    out['grads_blend_vertices'], out['grads_blend_features'] = p.grad.numpy(), q.grad.numpy()

    # ---- cases: the reference's TestSamplePoints, its fixtures as data and its calls recorded ------------------------------------
    cls = tests.TestSamplePoints
    fixture = lambda name: getattr(getattr(cls, name), '__wrapped__', None) or getattr(cls, name).__pytest_wrapped__.obj  # noqa: E731
    t = cls()
    fx = {name: fixture(name)(t, 'cpu', torch.float32) for name in
          ('vertices', 'faces', 'face_features', 'packed_vertices_info', 'packed_faces_info')}
    out['cases_vertices'], out['cases_faces'] = fx['vertices'].numpy(), fx['faces'].numpy()
    out['cases_face_features'] = fx['face_features'].numpy()
    out['cases_packed_vertices'], out['cases_packed_first_idx_vertices'] = (x.numpy() for x in fx['packed_vertices_info'])
    out['cases_packed_faces'], out['cases_packed_num_faces_per_mesh'] = (x.numpy() for x in fx['packed_faces_info'])
    calls = []
    for tag, dt in DTYPES:
        fx = {name: fixture(name)(t, 'cpu', dt) for name in fx}
        rec_s, rec_p = Recorder(tm.sample_points), Recorder(tm.packed_sample_points)
        kaolin.ops.mesh.sample_points, kaolin.ops.mesh.packed_sample_points = rec_s, rec_p
        torch.manual_seed(7)
        t.test_sample_points(fx['vertices'], fx['faces'], fx['face_features'], False, 'cpu', dt)
        t.test_sample_points(fx['vertices'], fx['faces'], fx['face_features'], True, 'cpu', dt)
        t.test_packed_sample_points(fx['packed_vertices_info'], fx['packed_faces_info'], 'cpu', dt)
        for name, rec in (('sample_points', rec_s), ('packed_sample_points', rec_p)):
            for args, kwargs, res in rec.calls:
                num_samples = args[4] if name == 'packed_sample_points' else args[2]
                calls.append([name, tag, str(num_samples), str(int('face_features' in kwargs))] +
                             [f'{tuple(x.shape)}:{str(x.dtype).replace("torch.", "")}' for x in res] + [''] * (3 - len(res)))
    kaolin.ops.mesh.sample_points, kaolin.ops.mesh.packed_sample_points = tm.sample_points, tm.packed_sample_points
    assert len(calls) == 6
    out['cases_calls'] = np.array(calls)

    path = os.path.join(HERE, 'sample_points.npz')
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != 'sample_points.npz')
    assert size < largest, (size, largest)
    print('wrote sample_points.npz', len(out), 'arrays', size, 'bytes')
    for row in calls:
        print(row)


if __name__ == '__main__':
    main()
