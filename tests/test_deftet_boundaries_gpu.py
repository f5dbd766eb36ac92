"""deftet_sparse_render's HIP pipeline (csrc/deftet.hip) at the boundaries of its pixel grid, on the scenes of
deftet_boundary_cases.py (test_deftet_boundary_cases_cpu.py shows that each scene is what it claims to be).

Forward operator: all four outputs equal to the CPU oracle's (torch.equal: the same expressions, contraction off), and the three
counters the call leaves in its workspace -- faces handed to the wavefront kernel, faces handed to the workgroup kernel, pixels
redone because they overflowed their row -- equal to what the restated dispatch rules and the oracle's hit counts say.
Fused forward: face indices equal, features to the tolerances of test_deftet.test_gpu_render_matches_oracle, on either side of
the sort's one-pass / fill-then-rank switch.
Backward: against the oracle in float64 on the widened inputs, with the float oracle's own error E32 as the floor of the bound
(render_helper_cases.mismatch: float |x - ref64| <= 1e-5 |ref64| + 4 E32, double 1e-10 |ref64| + 1e-6 E32).

Which test reaches which path of deftet.hip:
    dt_big_face_kernel<T, 256> (workgroup per face)             test_forward_pixel_count_edges[P >= 8193], test_forward_double
    wave handover by candidate count (<= 16 cells, > 256 px)    test_forward_crowded_cells[cluster], test_forward_degenerate[identical-*]
    gshift 6 and 7 (G = 64, 128)                                test_forward_pixel_count_edges[8193 .. 131072]
    multi-block cell scan (4, 16, 64 blocks) with B = 2         test_forward_pixel_count_edges[P >= 8193], test_forward_double
    dt_sort_interp_kernel<T, 4>, float and double, B = 2        test_fused_on_either_side_of_the_sort_switch
    dt_backward_staged_kernel<float, 1> and <float, 4>          test_backward[float32-1], [float32-4], test_backward_through_big_faces
    dt_backward_kernel<float> (generic)                         test_backward[float32-5], [float32-8]
    overflow redo fed by all three face paths, knum = 1 and 4   test_forward_overflow_redo
    degenerate / empty / overflowing extent, beyond float       test_forward_degenerate, test_forward_crowded_cells[outlier]
    caller-supplied boxes: empty, inverted, NaN, too small      test_forward_given_boxes"""
import functools

import pytest
import torch

import deftet_boundary_cases as dbc
import oracle
from render_helper_cases import mismatch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32, F64 = torch.float32, torch.float64
COUNT_K = 64                                     # more slots than any pixel of these scenes has hits


def ids(value):
    return str(value).replace('torch.', '') if isinstance(value, torch.dtype) else None


mixed = functools.lru_cache(maxsize=None)(dbc.mixed)
clean = functools.lru_cache(maxsize=None)(dbc.clean)


def forward_with_counters(z, img, bb, pix, ranges, K, eps=1e-8):
    """The call of _C.render.mesh.deftet_sparse_render_forward_cuda with the workspace in hand
    -> [face_idx, depths, w0, w1], counters[0..2] (see DtWs in deftet.hip: zeroed when a call starts, never afterwards)"""
    from kaolin_amd import _lib
    lib = _lib.load()
    B, F, P = z.shape[0], z.shape[1], pix.shape[1]
    dtype, device = z.dtype, z.device
    assert all(t.is_contiguous() and t.dtype == dtype and t.device == device for t in (z, img, bb, pix, ranges))
    assert img.shape == (B, F, 3, 2) and bb.shape == (B, F, 4) and pix.shape == ranges.shape == (B, P, 2)
    sfx = _lib.dtype_suffix(dtype, 'forward_with_counters')
    with _lib.on_device(device):
        face_idx = torch.empty((B, P, K), dtype=torch.long, device=device)
        depths, w0, w1 = (torch.empty((B, P, K), dtype=dtype, device=device) for _ in range(3))
        nbytes = lib.kamd_deftet_forward_workspace(B, F, P, dtype.itemsize)
        ws = torch.ones((nbytes + 3) // 4, dtype=torch.int32, device=device)      # (the operator passes torch.empty)
        st = getattr(lib, f'kamd_deftet_sparse_render_forward_{sfx}')(
            _lib.stream_ptr(device), B, F, P, K, _lib.ptr(z), _lib.ptr(img), _lib.ptr(bb), _lib.ptr(pix), _lib.ptr(ranges),
            float(eps), _lib.ptr(face_idx), _lib.ptr(depths), _lib.ptr(w0), _lib.ptr(w1), _lib.ptr(ws), nbytes)
    _lib.check(st, 'forward_with_counters')
    return [face_idx, depths, w0, w1], ws[:3].tolist()


def same(a, b):
    """torch.equal with NaNs in the same places"""
    if a.is_floating_point():
        return torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    return torch.equal(a, b)


def check_forward(case, K, dtype, bb=None, minimums=None):
    """-> the counters.  case = (pix, ranges, z, img, ...) float64 on the CPU"""
    pix, ranges, z, img = (t.to(dtype).contiguous() for t in case[:4])
    name = (case[-1], K, dtype)
    bb = dbc.boxes_of(img) if bb is None else bb.to(dtype).contiguous()
    got, counters = forward_with_counters(z.to(DEV), img.to(DEV), bb.to(DEV), pix.to(DEV), ranges.to(DEV), K)
    ref = oracle.deftet_sparse_render_forward(z, img, bb, pix, ranges, K, 1e-8, omp=True)
    for what, a, b in zip(('face_idx', 'depths', 'w0', 'w1'), got, ref):
        assert same(a.cpu(), b), (name, what, int((a.cpu() != b).sum()))
    hits = dbc.hit_counts(ref[0] if K >= COUNT_K else
                          oracle.deftet_sparse_render_forward(z, img, bb, pix, ranges, COUNT_K, 1e-8, omp=True)[0])
    assert int(hits.max()) < max(K, COUNT_K), name
    want = dbc.handover_counts(pix.double(), bb.double())
    print(name, 'counters', counters, 'restated rules', want, 'pixels with more than K hits', int((hits > K).sum()))
    assert counters == [want['wave'], want['group'], int((hits > K).sum())], (name, counters, want)
    for got_n, least in zip(counters, minimums or ()):
        assert got_n >= least, (name, counters, minimums)
    return counters


# ---- the forward operator ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('P', dbc.P_EDGES)
def test_forward_pixel_count_edges(P):
    """gshift 4 .. 8, 1 .. 64 scan blocks with B = 2, all three face kernels in one call (from 8193 pixels on)"""
    counters = check_forward(mixed(2, P, 1), 8, F32, minimums=(40, 8 if P >= 8193 else 0, 0))
    assert (counters[1] > 0) == (P >= 8193)


@pytest.mark.parametrize('P', [8193, 32769])
def test_forward_double(P):
    check_forward(mixed(2, P, 1), 8, F64, minimums=(40, 8, 0))


@pytest.mark.parametrize('K', [1, 4])
def test_forward_overflow_redo(K):
    """rows of the overflow redo = the oracle's first K hits in mesh order, of faces from all three face kernels
    (test_deftet_boundary_cases_cpu.test_hit_counts_of_the_overflow_scene)"""
    counters = check_forward(mixed(2, 8193, 1), K, F32, minimums=(40, 8, 5001 if K == 1 else 1001))
    assert counters[2] > (5000 if K == 1 else 1000)


@pytest.mark.parametrize('dtype', [F32, F64], ids=ids)
@pytest.mark.parametrize('kind', ['cluster', 'outlier'])
def test_forward_crowded_cells(kind, dtype):
    """cluster: a box over <= 16 cells goes to a wavefront because of the pixels in them; outlier: one axis in a single cell"""
    case = dbc.mixed(2, 3000, 2, cluster=kind == 'cluster', outlier=kind == 'outlier')
    check_forward(case, 8, dtype, minimums=(40, 0, 0))


@pytest.mark.parametrize('kind,dtype', [(kind, dtype) for kind in dbc.DEGENERATE
                                        for dtype in dbc.DEGENERATE_DTYPES.get(kind, (F32, F64))], ids=ids)
def test_forward_degenerate(kind, dtype):
    counters = check_forward(dbc.degenerate(kind), 8, dtype)
    if kind == 'identical':
        assert counters[0] >= 1 and counters[1] == 0
    if kind == 'no_finite':
        assert counters == [0, 0, 0]


@pytest.mark.parametrize('dtype', [F32, F64], ids=ids)
def test_forward_given_boxes(dtype):
    pix, ranges, z, img, bb, name = dbc.boxes_given()
    check_forward((pix, ranges, z, img, name), 8, dtype, bb=bb)


@pytest.mark.parametrize('F', [1, 255, 256, 257])
def test_forward_face_count_edges(F):
    pix, ranges, z, img, name = mixed(2, 3000, 2)
    check_forward((pix, ranges, z[:, :F], img[:, :F], f'{name}_F{F}'), 8, F32)


# ---- the fused forward on either side of the sort's switch ---------------------------------------------------------------
def fused(case, feat, K, dtype):
    import kaolin_amd as kal
    pix, ranges, z, img = (t.to(dtype).to(DEV).contiguous() for t in case[:4])
    args = (pix, ranges, z, img, feat.to(dtype).to(DEV).contiguous())
    return kal.render.mesh.deftet_sparse_render(*args) if K is None else kal.render.mesh.deftet_sparse_render(*args, K)


def check_fused(out, idx, case, feat, K, dtype):
    pix, ranges, z, img = (t.to(dtype) for t in case[:4])
    ref = oracle.deftet_sparse_render(pix, ranges, z, img, feat.to(dtype), K, omp=True)
    assert out.shape == ref['features'].shape and out.dtype == dtype and idx.dtype == torch.long
    assert torch.equal(idx.cpu(), ref['face_idx'])
    tol = dict(rtol=1e-5, atol=1e-6) if dtype == F32 else dict(rtol=1e-12, atol=1e-13)
    assert torch.allclose(out.cpu(), ref['features'], **tol)
    void = idx == -1
    assert bool((out[void] == 0).all()) and bool(void.any()) and int(idx.min()) == -1
    hits = dbc.hit_counts(idx)
    assert bool((idx[..., 1:] == -1)[idx[..., :-1] == -1].all())             # the hits lead the row
    return hits


@pytest.mark.parametrize('dtype,D', [(F32, 3), (F64, 1)], ids=ids)
def test_fused_on_either_side_of_the_sort_switch(dtype, D):
    B, P, (k_lo, k_hi) = dbc.KH_EDGE['B'], dbc.KH_EDGE['P'], dbc.KH_EDGE['K']
    assert dbc.sort_path(B, P, k_lo) == 'one_pass' and dbc.sort_path(B, P, k_hi) == 'fill_then_rank'
    case = mixed(B, P, 1)
    feat = dbc.features(B, sum(dbc.MIXED_FACES), D, seed=D)
    out_lo, idx_lo = fused(case, feat, k_lo, dtype)
    hits = check_fused(out_lo, idx_lo, case, feat, k_lo, dtype)
    assert 4 < int(hits.max()) < k_lo and int(hits.min()) == 0
    out_hi, idx_hi = fused(case, feat, k_hi, dtype)
    check_fused(out_hi, idx_hi, case, feat, k_hi, dtype)
    assert torch.equal(idx_hi[..., :k_lo], idx_lo) and torch.equal(out_hi[..., :k_lo, :], out_lo)
    assert bool((idx_hi[..., k_lo:] == -1).all()) and bool((out_hi[..., k_lo:, :] == 0).all())


def test_fused_default_knum():
    case = clean()
    feat = dbc.features(2, 300, 2, seed=9)
    out, idx = fused(case, feat, None, F32)
    assert idx.shape == (2, 700, 300)
    check_fused(out, idx, case, feat, 300, F32)


# ---- backward ----------------------------------------------------------------------------------------------------------
def check_backward(case, D, K, dtype, seed):
    """Both gradients, through autograd and through the C operator, against the float64 oracle on the GPU forward's face_idx
    and weights; the floor of the bound is the float oracle's own error on the same inputs."""
    import kaolin_amd as kal
    name = (case[-1], D, K, dtype)
    pix, ranges, z, img = (t.to(dtype).to(DEV).contiguous() for t in case[:4])
    B, F = img.shape[:2]
    feat64 = dbc.features(B, F, D, seed)
    feat = feat64.to(dtype).to(DEV)
    _, idx, weights = kal._C.render.mesh.deftet_sparse_render_forward_fused(z, img, dbc.boxes_of(img), pix, ranges, feat, K, 1e-8)
    want_idx = oracle.deftet_sparse_render(pix, ranges, z, img, feat, K, omp=True)['face_idx']
    assert torch.equal(idx.cpu(), want_idx), name
    assert int(dbc.hit_counts(want_idx).max()) > 4
    grad64 = dbc.upstream(idx.shape + (D,), seed)
    w64 = weights.cpu().double()
    ref64 = oracle.deftet_sparse_render_backward(grad64, idx, w64, case[3], feat64, 1e-8)
    ref32 = oracle.deftet_sparse_render_backward(grad64.float(), idx, w64.float(), case[3].float(), feat64.float(), 1e-8)
    e32 = [float((a.double() - b).abs().max()) for a, b in zip(ref32, ref64)]
    grad = grad64.to(dtype).to(DEV)

    a, u = img.clone().requires_grad_(), feat.clone().requires_grad_()
    out, idx_api = kal.render.mesh.deftet_sparse_render(pix, ranges, z, a, u, K)
    assert torch.equal(idx_api, idx), name
    out.backward(grad)
    direct = kal._C.render.mesh.deftet_sparse_render_backward_cuda(grad, idx, weights, img, feat, 1e-8)
    failures = []
    for route, got in (('autograd', (a.grad, u.grad)), ('operator', direct)):
        for what, x, ref, e in zip(('grad_face_vertices_image', 'grad_face_features'), got, ref64, e32):
            worst, msg = mismatch(x, ref, e, dtype)
            print(name, route, what, f'worst ratio {worst:.3g} of the bound, E32 = {e:.3e}, largest entry {float(ref.abs().max()):.3e}')
            if msg is not None:
                failures.append((route, what, f'worst ratio {worst:.3g}', msg))
    assert not failures, (name, failures)


@pytest.mark.parametrize('dtype,D', [(F32, D) for D in (1, 2, 3, 4, 5, 8)] + [(F64, 1), (F64, 5)], ids=ids)
def test_backward(dtype, D):
    """float D = 1 .. 4: dt_backward_staged_kernel<float, D>; float D = 5, 8 and double: dt_backward_kernel"""
    check_backward(clean(), D, 48, dtype, seed=D)


def test_backward_through_big_faces():
    """a full-extent face collects thousands of hits on each of its atomic targets"""
    case = mixed(2, 8193, 1)
    check_backward(case, 4, 16, F32, seed=4)
