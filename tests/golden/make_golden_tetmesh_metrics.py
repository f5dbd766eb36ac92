"""Generates tests/golden/tetmesh_metrics.npz FROM THE REFERENCE ITSELF (kaolin.metrics.tetmesh: tetrahedron_volume, equivolume,
amips).

Run in the build container (where the reference tree is mounted):
    python tests/golden/make_golden_tetmesh_metrics.py
The reference's files are loaded by path on top of _refload's stub ``kaolin`` package; they are pure PyTorch and run on the CPU.
Inputs are rebuilt from rules (tests/tetmesh_metrics_golden.py, shared with the tests) and from marching_tetrahedra.npz.  Per
result the file holds the reference's float64 answer ``<name>_f64``, ``<name>_ref32_dev`` = its float32 answer minus that
(float32 inputs widened for the float64 run), and for per-element results ``<name>_tas``: the float64 sum of the magnitudes of
the terms the element adds (asserted to bound it; stored as a float32 rounded upwards).  Gradients with respect to ``tet_vertices`` are recorded gathered onto the
vertices through ``vertices[:, tets]`` ((B, V, 3); per tet they would make the file several times the size limit asserted below).

  kat_*       the inputs of the reference's own tests/python/kaolin/metrics/test_tetmesh.py (the same as its docstrings'), read
              off its calls: ``kat_<fn>_in<k>``, what the reference returns ``kat_<fn>_ret_{f32,f64}`` and what its test expects
              ``kat_<fn>_expected``.  For equivolume the two DISAGREE (B == T == 2: the mean of item j is subtracted from tet
              j); the tests pin what is returned.
  vol_grid9   tet_vertices = vertices[:, grid9_tets], B = 2 (tests/tetmesh_metrics_golden.py::grid9): ``vol_grid9_f64`` (2, T),
              ``vol_grid9_cot`` the seeded cotangent of exact halves, ``vol_grid9_grad_*`` the gradient on the vertices
  equi_*      ``equi_item<b>_pow<p>_{loss,grad}_*``: B = 1 on either grid9 item, mean computed; ``equi_given_{loss,grad,
              grad_mean}_*``: B = 2, pow = 4, the one-element mean GIVEN_MEAN.  The cotangent of the loss is 1.
  amips_*     rest shape kuhn_grid(6); ``amips_vertices`` (2, 343, 3) = rest + seeded jitter of +-0.02; ``amips_inv_{f32,f64}``
              (1, T, 3, 3) the reference's inverse_vertices_offset of the rest shape; tet_vertices by ``amips_tet_vertices``
              (swapped and zero-row tets).  ``amips_loss_*`` with the zero-row tets, ``amips_grad_{vertices,inv}_*`` without
              them (cotangent 1); ``amips_grad_loss_*``: the loss of that gradient case
  err_*       type and text of what the reference raises; dtypes_*: the dtype it returns, or ('raises', type, text)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import _refload  # noqa: E402
import tetmesh_metrics_golden as H  # noqa: E402
from kaolin_amd.utils.testing import kuhn_grid  # noqa: E402

NAME = 'tetmesh_metrics.npz'


def load_modules():
    _refload.load_reference()
    conv = _refload._load('kaolin.ops.conversions.tetmesh', 'kaolin/ops/conversions/tetmesh.py')
    sys.modules['kaolin.ops.conversions'].tetmesh = conv
    ops = _refload._load('kaolin.ops.mesh.tetmesh', 'kaolin/ops/mesh/tetmesh.py')
    sys.modules['kaolin.ops.mesh'].tetmesh = ops
    ref = _refload._load('kaolin.metrics.tetmesh', 'kaolin/metrics/tetmesh.py')
    sys.modules['kaolin.metrics'].tetmesh = ref
    kat = _refload._load('ref_test_metrics_tetmesh', 'tests/python/kaolin/metrics/test_tetmesh.py')
    return ref, ops, kat


class _Calls:
    """Stands in for the module under test and for ``torch`` inside the reference's test file: records the arguments of every
    call of the metrics and both sides of every ``allclose``."""

    def __init__(self, ref):
        self.ref, self.calls, self.compared = ref, [], []

    def __getattr__(self, name):
        if name == 'allclose':
            return lambda a, b, **k: self.compared.append((a, b)) or True
        if hasattr(self.ref, name) and name in ('tetrahedron_volume', 'equivolume', 'amips'):
            def fn(*args, **kwargs):
                self.calls.append((name, args, kwargs))
                return getattr(self.ref, name)(*args, **kwargs)
            return fn
        return getattr(torch, name)


def leaf(x, dtype):
    return x.detach().clone().to(dtype).requires_grad_()


def record_error(out, name, fn):
    try:
        fn()
    except Exception as err:  # noqa: BLE001  (the reference's own error, whatever its type)
        out[f'err_{name}'] = np.array([type(err).__name__, str(err)])
        return
    raise AssertionError(f'err_{name}: the reference raised nothing')


def main():
    torch.set_num_threads(1)                      # index_put's accumulation (the backward of vertices[:, tets]) in one fixed order
    torch.use_deterministic_algorithms(True)
    ref, ops, kat = load_modules()
    gen = torch.Generator().manual_seed(20262)
    out = {}

    def both(fn):
        """fn(dtype) -> tensor or tuple of tensors; -> the float64 answers and ref32 - ref64"""
        r32, r64 = fn(torch.float32), fn(torch.float64)
        if not isinstance(r32, tuple):
            r32, r64 = (r32,), (r64,)
        assert all(a.dtype == torch.float32 and b.dtype == torch.float64 and bool(torch.isfinite(b).all()) for a, b in zip(r32, r64))
        return [b.detach() for b in r64], [(a.detach().double() - b.detach()).float() for a, b in zip(r32, r64)]

    def store(name, r64, dev, tas=None):
        out[f'{name}_f64'], out[f'{name}_ref32_dev'] = r64.numpy(), dev.numpy()
        if dev.numel() > 16:     # per-element deviations are a record, not a bound: 8 significant bits (they compress to half)
            out[f'{name}_ref32_dev'] = (dev.numpy().view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
        if tas is not None:
            assert bool((tas * (1 + 1e-9) + 1e-300 >= r64.abs()).all()), name
            out[f'{name}_tas'] = (tas * (1 + 2.0 ** -22)).float().numpy()      # float32, rounded up: half the bytes, still a bound
            assert bool((torch.from_numpy(out[f'{name}_tas']).double() >= tas).all()), name

    # ---- kat: the reference's own test, its inputs and expectations read as data ----------------------------------------------
    spy = _Calls(ref)
    kat.tetmesh, kat.torch = spy, spy
    t = kat.TestTetMeshMetrics()
    t.test_tetrahedron_volume(), t.test_amips(), t.test_equivolume()
    assert [c[0] for c in spy.calls] == ['tetrahedron_volume', 'amips', 'equivolume'] and len(spy.compared) == 3
    for (fn, args, kwargs), (returned, expected) in zip(spy.calls, spy.compared):
        assert kwargs == ({'pow': 4} if fn == 'equivolume' else {})
        for k, a in enumerate(args):
            out[f'kat_{fn}_in{k}'] = a.numpy()
        out[f'kat_{fn}_ret_f32'] = returned.numpy()
        out[f'kat_{fn}_ret_f64'] = getattr(ref, fn)(*[a.double() for a in args], **kwargs).numpy()
        out[f'kat_{fn}_expected'] = expected.numpy()
    assert np.allclose(out['kat_equivolume_ret_f32'], [[2.2961e-10], [7.7704e-10]], rtol=1e-4, atol=0)       # (its docstring's numbers)
    assert not np.allclose(out['kat_equivolume_ret_f32'], out['kat_equivolume_expected'], rtol=1e-2, atol=0)  # its test fails

    # ---- vol_grid9 ---------------------------------------------------------------------------------------------------------
    gv, gt = H.grid9()
    V, T = gv.shape[1], gt.shape[0]
    assert (V, T) == (1000, 4444)
    cot = torch.randint(-2, 3, (2, T), generator=gen).float() / 2
    out['vol_grid9_cot'] = cot.numpy()

    def vol(dt):
        p = leaf(gv, dt)
        v = ref.tetrahedron_volume(p[:, gt])
        (v * cot.to(dt)).sum().backward()
        return v, p.grad

    (v64, g64), (vdev, gdev) = both(vol)
    assert int((v64 > 0).sum()) > 100 and int((v64 < 0).sum()) > 100 and int((v64[1] == 0).sum()) >= 20
    store('vol_grid9', v64, vdev, H.volume_terms(gv[:, gt]))
    store('vol_grid9_grad', g64, gdev, H.to_vertices(H.volume_grad_terms(gv[:, gt], cot), gt, V))

    # ---- equi --------------------------------------------------------------------------------------------------------------
    def well_signed(v, m):
        # the sign of v - m is not a float32 question: no |v - m| within 1e-3 of the median of zero -- apart from the tets whose
        # volume is zero up to its own rounding (a repeated corner: |v| <= 1e-12 mean|v|), where v - m = -m: there |m| must be twice the worst
        # case of the rounding error of a float32 mean, T u mean|v| with the unit roundoff u = eps / 2
        d = (v - m).abs()
        safe_mean = abs(float(m)) >= 2 * v.shape[-1] * float(torch.finfo(torch.float32).eps) / 2 * float(v.abs().mean())
        assert bool(((d == 0) | (d >= 1e-3 * d.median()) | ((v.abs() <= 1e-12 * v.abs().mean()) & safe_mean)).all())

    for b in range(2):
        item = gv[b:b + 1]
        well_signed(v64[b], v64[b].mean())
        for p in H.EQUI_POWS:
            def equi(dt, p=p):
                x = leaf(item, dt)
                loss = ref.equivolume(x[:, gt], pow=p)
                loss.sum().backward()
                return loss, x.grad
            (l64, eg64), (ldev, egdev) = both(equi)
            assert l64.shape == (1, 1)
            terms, _ = H.equivolume_grad_terms(item[:, gt], v64[b].mean().reshape(1), p, True)
            store(f'equi_item{b}_pow{p}_loss', l64, ldev)
            store(f'equi_item{b}_pow{p}_grad', eg64, egdev, H.to_vertices(terms, gt, V))
    well_signed(v64, H.GIVEN_MEAN)

    def equi_given(dt):
        x, m = leaf(gv, dt), leaf(torch.tensor([H.GIVEN_MEAN]), dt)
        loss = ref.equivolume(x[:, gt], m, pow=4)
        loss.sum().backward()
        return loss, x.grad, m.grad
    (l64, eg64, em64), (ldev, egdev, emdev) = both(equi_given)
    assert l64.shape == (2, 1) and em64.shape == (1,)
    terms, mean_terms = H.equivolume_grad_terms(gv[:, gt], torch.tensor([H.GIVEN_MEAN]), 4, False)
    store('equi_given_loss', l64, ldev)
    store('equi_given_grad', eg64, egdev, H.to_vertices(terms, gt, V))
    store('equi_given_grad_mean', em64, emdev, mean_terms.reshape(1))

    # ---- amips -------------------------------------------------------------------------------------------------------------
    rest, at = kuhn_grid(6)
    AT = at.shape[0]
    assert AT == 1296
    av = rest[None] + (torch.rand((2,) + rest.shape, generator=gen) - 0.5) * 0.04
    out['amips_vertices'] = av.numpy()
    inv = {dt: ops.inverse_vertices_offset(rest.to(dt)[None][:, at]) for dt in (torch.float32, torch.float64)}
    out['amips_inv_f32'], out['amips_inv_f64'] = inv[torch.float32].numpy(), inv[torch.float64].numpy()
    x64 = H.amips_tet_vertices(av.double(), at)
    jac = (x64[:, :, 1:] - x64[:, :, :1]) @ inv[torch.float64]
    det, zero = torch.det(jac), H.zero_row_tets(AT)
    assert bool((det[:, ~zero].abs() >= 0.1).all()) and bool((jac[:, zero].abs().sum(-1) == 0).any(-1).all())
    rows = jac[:, ~zero]                                                            # no tet with two equal non-zero rows
    assert not any(bool((rows[:, :, i] == rows[:, :, k]).all(-1).any()) for i, k in ((0, 1), (0, 2), (1, 2)))
    assert int((det[:, ~zero] < 0).sum()) >= 2 * (AT // 7 - AT // 77)

    def amips(dt, zero_rows, grads):
        x, m = leaf(av, dt), leaf(inv[dt], dt)
        loss = ref.amips(H.amips_tet_vertices(x, at, zero_rows), m)
        if not grads:
            return loss
        loss.sum().backward()
        return loss, x.grad, m.grad
    (l64,), (ldev,) = both(lambda dt: amips(dt, True, False))
    assert l64.shape == (2, 1)
    store('amips_loss', l64, ldev)
    (l64, ag64, am64), (ldev, agdev, amdev) = both(lambda dt: amips(dt, False, True))
    tv_terms, inv_terms = H.amips_grad_terms(H.amips_tet_vertices(av, at, False), inv[torch.float64])
    store('amips_grad_loss', l64, ldev)
    store('amips_grad_vertices', ag64, agdev, H.to_vertices(tv_terms, at, rest.shape[0]))
    store('amips_grad_inv', am64, amdev, inv_terms.sum(0, keepdim=True))

    # ---- errors and dtypes -------------------------------------------------------------------------------------------------
    for fn in ('tetrahedron_volume', 'equivolume'):
        record_error(out, f'{fn}_ndim', lambda: getattr(ref, fn)(torch.zeros(2, 2)))
        record_error(out, f'{fn}_dim2', lambda: getattr(ref, fn)(torch.zeros(1, 2, 3, 3)))
        record_error(out, f'{fn}_dim3', lambda: getattr(ref, fn)(torch.zeros(1, 2, 4, 2)))
    record_error(out, 'amips_ndim', lambda: ref.amips(torch.zeros(2, 2), torch.zeros(1, 2, 3, 3)))
    record_error(out, 'amips_dim2', lambda: ref.amips(torch.zeros(1, 2, 3, 3), torch.zeros(1, 2, 3, 3)))
    record_error(out, 'amips_dim3', lambda: ref.amips(torch.zeros(1, 2, 4, 2), torch.zeros(1, 2, 3, 3)))
    five = gv[:1, gt[:15]].reshape(3, 5, 4, 3)
    record_error(out, 'equivolume_batch3x5', lambda: ref.equivolume(five))
    record_error(out, 'equivolume_mean3_t5', lambda: ref.equivolume(five, torch.zeros(3)))

    def dtypes(name, fn):
        try:
            out[f'dtypes_{name}'] = np.array([str(fn().dtype)])
        except Exception as err:  # noqa: BLE001
            out[f'dtypes_{name}'] = np.array(['raises', type(err).__name__, str(err)])

    small, small_inv = H.amips_tet_vertices(av, at)[:, :8], inv[torch.float32][:, :8]
    dtypes('volume_half', lambda: ref.tetrahedron_volume(small.half()))
    dtypes('equivolume_half', lambda: ref.equivolume(small[:1].half()))
    dtypes('amips_half', lambda: ref.amips(small.half(), small_inv.half()))
    dtypes('equivolume_mixed', lambda: ref.equivolume(small, torch.tensor([1e-3], dtype=torch.float64)))
    dtypes('amips_mixed', lambda: ref.amips(small, small_inv.double()))
    dtypes('amips_f64', lambda: ref.amips(small.double(), small_inv.double()))

    path = os.path.join(HERE, NAME)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f != NAME)
    assert size < largest, (size, largest)
    print('wrote', NAME, len(out), 'arrays', size, 'bytes')
    for k in sorted(out):
        if k.startswith('err_') or k.startswith('dtypes_') or (k.startswith('kat_') and 'in' not in k):
            print(k, out[k].tolist())


if __name__ == '__main__':
    main()
