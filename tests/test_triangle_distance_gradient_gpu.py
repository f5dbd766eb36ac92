"""The gradient of the point -> triangle distance, GPU part: td_backward_kernel (kaolin_amd/csrc/triangle_distance.hip) driven directly
through `_C.metrics.unbatched_triangle_distance_backward_cuda` with prescribed faces and regions -- per-point terms bit-equal to the
pinned oracle at every wavefront / workgroup edge and region layout, clamped and short edges, shared faces per element under
gamma_(n-1) sum|term|, non-finite inputs, and the calls users make.  Bounds, cases and reference: tests/triangle_distance_gradient_cases.py;
the oracle itself is held to float64 autograd in tests/test_triangle_distance_gradient_cpu.py.  Every index passed is in [0, F)."""
import numpy as np
import pytest
import torch

import oracle
import triangle_distance_gradient_cases as C

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]


gpu_backward = C.gpu_backward


def _tm():
    from kaolin_amd.metrics import trianglemesh
    return trianglemesh


def _bits_equal(a, b):
    """torch.equal on the bit patterns (it tells +0.0 from -0.0)."""
    as_int = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(as_int), b.contiguous().view(as_int))


# ---------------------------------------------------------------------------------------------------------------- terms, bit for bit
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('n', C.SIZES)
@pytest.mark.parametrize('layout', C.LAYOUTS)
def test_private_face_terms_equal_the_pinned_oracle(layout, n, dtype):
    """One contributor per face: g_points and g_faces are the per-point terms and equal the fused oracle's bit for bit (same IEEE
    operations in the same order, incl. the fma pin and 1 / sqrt), with every region in one wavefront (cyclic), one region filling a
    wavefront (its `touched` mask in all 64 rows of the LDS stage) and one filling a workgroup, at N on either side of 64 and 256."""
    case = C.private_case(layout, n, dtype)
    g_p, g_f = gpu_backward(*case)
    o_p, o_f = oracle.triangle_distance_backward(*case)
    assert torch.equal(g_p, o_p), f'g_points: {int((g_p != o_p).any(1).sum())} of {n} points differ'
    assert torch.equal(g_f, o_f), f'g_faces: {int((g_f != o_f).reshape(n, -1).any(1).sum())} of {n} faces differ'
    # values the region does not touch are +0.0 (nothing was added: not even a -0.0)
    untouched = C.touched_bits(case[4]) == 0
    assert bool((g_f.reshape(n, 9)[untouched] == 0).all()) and not bool(torch.signbit(g_f.reshape(n, 9)[untouched]).any())
    # ... and directly against float64 autograd of the stored region
    s_p, s_f = C.term_shares(g_p, g_f.reshape(n, 9), *case, C.U[dtype])
    print(C.fmt_regions(f'{layout} N={n} {dtype}: bit-equal to the oracle; terms / (u M)', s_p, s_f, case[4]))
    assert C.terms_within(s_p, s_f)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_clamped_edges_equal_the_pinned_oracle(dtype):
    """Types 4 - 6 with k < 0, = 0, inside, = 1, > 1 (exact), grad zero / negative / 1e6: bit-equal to the oracle, which the CPU tests hold
    to float64 autograd; here also directly, under K u M."""
    case, ks = C.clamp_case(dtype)
    g_p, g_f = gpu_backward(*case)
    o_p, o_f = oracle.triangle_distance_backward(*case)
    assert torch.equal(g_p, o_p) and torch.equal(g_f, o_f)
    s_p, s_f = C.term_shares(g_p, g_f.reshape(-1, 9), *case, C.U[dtype])
    print(C.fmt_regions(f'clamp {dtype} / (u M)', s_p, s_f, case[4]))
    assert C.terms_within(s_p, s_f)
    zero = case[0] == 0
    assert bool((g_p[zero] == 0).all()) and bool((g_f[zero] == 0).all())


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_short_edges_equal_the_pinned_oracle(dtype):
    case = C.short_edge_case(dtype)
    g_p, g_f = gpu_backward(*case)
    o_p, o_f = oracle.triangle_distance_backward(*case)
    assert torch.equal(g_p, o_p) and torch.equal(g_f, o_f)
    s_p, s_f = C.term_shares(g_p, g_f.reshape(-1, 9), *case, C.U[dtype])
    print(C.fmt_regions(f'short edge {dtype} / (u M)', s_p, s_f, case[4]))
    assert C.terms_within(s_p, s_f)


# ---------------------------------------------------------------------------------------------------------------- accumulation
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('name', ['one_face', 'middle_of_3', 'alternating_2', 'random_300'])
def test_shared_faces_per_element(name, dtype):
    """Every face value against the sum of its contributors' terms (the kernel's own, from a private-face run, themselves bit-equal
    to the oracle's): |got - want| <= gamma_(n-1) sum|term| with the element's own n; twice, since the atomics' order is free."""
    case = C.shared_cases(dtype)[name]
    grad, pts, fv, idx, typ = case
    t_p, t_f = C.operator_terms(gpu_backward, *case)
    o_p, o_f = C.operator_terms(oracle.triangle_distance_backward, *case)
    assert torch.equal(t_p, o_p) and torch.equal(t_f, o_f)
    for run in range(2):
        g_p, g_f = gpu_backward(*case)
        assert torch.equal(g_p, t_p)
        s, count = C.accumulation_share(g_f, t_f, idx, typ, C.U[dtype])
        print(f'{name} {dtype} run {run}: worst share {s.max():.3f} of gamma_(n-1) sum|term|, n up to {count.max()}')
        assert C.accumulation_within(s), f'{int((~(s <= 1)).sum())} values outside the bound'
        nobody = torch.from_numpy(count == 0)
        assert bool((g_f.reshape(-1, 9)[nobody] == 0).all()) and not bool(torch.signbit(g_f.reshape(-1, 9)[nobody]).any())
    if name == 'middle_of_3':
        assert not bool(g_f[0].bool().any()) and not bool(g_f[2].bool().any()) and not bool(torch.signbit(g_f[[0, 2]]).any())


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_private_faces_run_to_run(dtype):
    case = C.private_case('cyclic', 513, dtype)
    a, b = gpu_backward(*case), gpu_backward(*case)
    assert _bits_equal(a[0], b[0]) and _bits_equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------- non-finite inputs
@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_zero_area_face_gives_nan_at_the_oracles_positions(dtype):
    """Face 2 has v1 == v2 (normal exactly 0) and is hit with region 0 by points 64 - 66: 0 / 0 in the unit normal.  NaN in that face's
    nine values and those points' gradients, nowhere else; everything else as the oracle (one contributor per other face)."""
    grad, pts, fv, idx, typ = C.private_case('cyclic', 130, dtype)
    fv[2, 1] = fv[2, 0]
    idx, typ = idx.clone(), typ.clone()
    idx[64:67], typ[64:67] = 2, 0
    # face 2's own point moves to face 3 with region 4 (values 0 - 5; face 3's own point has region 3: values 6 - 8, so no value of any
    # finite face is a sum of two terms and the comparison stays exact)
    idx[2], typ[2] = 3, 4
    case = (grad, pts, fv, idx, typ)
    g_p, g_f = gpu_backward(*case)
    o_p, o_f = oracle.triangle_distance_backward(*case)
    assert torch.equal(g_p.isnan(), o_p.isnan()) and torch.equal(g_f.isnan(), o_f.isnan())
    assert g_p.isnan().nonzero()[:, 0].unique().tolist() == [64, 65, 66] and bool(g_p[64:67].isnan().all())
    assert bool(g_f[2].isnan().all()) and int(g_f.isnan().sum()) == 9
    assert torch.allclose(g_p, o_p, rtol=0, atol=0, equal_nan=True)
    assert torch.allclose(g_f, o_f, rtol=0, atol=0, equal_nan=True)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_infinite_vertex_outside_the_region_is_not_touched(dtype):
    """Face 5's v3 is inf and the face is hit with region 4 (edge v1 -> v2) only: the formula does not involve v3, and its three values
    stay exactly +0.0 (a 0 * inf or an added 0 + NaN would show)."""
    grad, pts, fv, idx, typ = C.private_case('cyclic', 130, dtype)
    fv[5, 2] = float('inf')
    idx, typ = idx.clone(), typ.clone()
    idx[70:73], typ[70:73], typ[5] = 5, 4, 4
    case = (grad, pts, fv, idx, typ)
    g_p, g_f = gpu_backward(*case)
    o_p, o_f = oracle.triangle_distance_backward(*case)
    assert bool((g_f[5, 2] == 0).all()) and not bool(torch.signbit(g_f[5, 2]).any())
    assert bool(torch.isfinite(g_f).all()) and bool(torch.isfinite(g_p).all())
    assert torch.equal(g_p, o_p)
    keep = torch.arange(130) != 5
    assert torch.equal(g_f[keep], o_f[keep])
    t_p, t_f = C.operator_terms(gpu_backward, grad, pts, torch.nan_to_num(fv, posinf=0.0), idx, typ)   # (v3 plays no part in these terms)
    s, _ = C.accumulation_share(g_f, t_f, idx, typ, C.U[dtype])
    assert C.accumulation_within(s)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_zero_length_edge_gives_nan_at_the_oracles_positions(dtype):
    """Face 7 has v1 == v2 and is hit with region 4 (that edge): k = 0 / 0.  The kernel clamps with fmax / fmin, which drop a NaN
    (the reference's max / min), the oracle with comparisons, which keep it; l_bar = 0 * (1 / 0) makes the six values of v1, v2 and
    the point's gradient NaN either way, and v3's three values stay +0.0."""
    grad, pts, fv, idx, typ = C.private_case('cyclic', 130, dtype)
    fv[7, 1] = fv[7, 0]
    typ = typ.clone()
    typ[7] = 4
    case = (grad, pts, fv, idx, typ)
    g_p, g_f = gpu_backward(*case)
    o_p, o_f = oracle.triangle_distance_backward(*case)
    assert bool(g_p[7].isnan().all()) and bool(g_f[7, :2].isnan().all())
    assert bool((g_f[7, 2] == 0).all()) and not bool(torch.signbit(g_f[7, 2]).any())
    assert int(g_p.isnan().sum()) == 3 and int(g_f.isnan().sum()) == 6
    assert torch.allclose(g_p, o_p, rtol=0, atol=0, equal_nan=True) and torch.allclose(g_f, o_f, rtol=0, atol=0, equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------- the way users call it
def _public(pts, fv):
    a, b = pts.cuda().requires_grad_(), fv.cuda().requires_grad_()
    dist, idx, typ = _tm().point_to_mesh_distance(a[None], b[None])
    return a, b, dist[0], idx[0].cpu(), typ[0].cpu()


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('kind', ['soup', 'sphere'])
def test_forward_chosen_regions_and_common_calls(kind, dtype):
    """N = 2000 on the soup and the sphere with the face and region the forward picks: dist.sum().backward() (a stride-0 cotangent),
    (dist * w).sum().backward(), and autograd.grad for the points alone and the faces alone -- terms under K u M against float64
    autograd, g_points equal to the terms, g_faces per element under the accumulation bound."""
    w, pts, fv = C.natural_inputs(kind, 2000, dtype=dtype)
    a, b, dist, idx, typ = _public(pts, fv)
    o = oracle.triangle_distance_forward(pts, fv, omp=True)
    assert torch.equal(idx, o[1]) and torch.equal(typ, o[2]) and torch.equal(dist.detach().cpu(), o[0])
    ones = torch.ones_like(w)
    g_p1, g_f1, worst_t, worst_a = C.check_operator(gpu_backward, ones, pts, fv, idx, typ, dtype, f'{kind} {dtype} grad = 1')
    dist.sum().backward(retain_graph=True)
    t_p, t_f = C.operator_terms(gpu_backward, ones, pts, fv, idx, typ)
    assert torch.equal(a.grad.cpu(), t_p)
    s, _ = C.accumulation_share(b.grad.cpu(), t_f, idx, typ, C.U[dtype])
    assert C.accumulation_within(s)
    a.grad = b.grad = None
    C.check_operator(gpu_backward, w, pts, fv, idx, typ, dtype, f'{kind} {dtype} grad = w')
    (dist * w.cuda()).sum().backward(retain_graph=True)
    t_p, t_f = C.operator_terms(gpu_backward, w, pts, fv, idx, typ)
    assert torch.equal(a.grad.cpu(), t_p)
    s, _ = C.accumulation_share(b.grad.cpu(), t_f, idx, typ, C.U[dtype])
    assert C.accumulation_within(s)
    only_p, = torch.autograd.grad(dist, a, w.cuda(), retain_graph=True)
    only_f, = torch.autograd.grad(dist, b, w.cuda())
    assert torch.equal(only_p.cpu(), t_p)
    s, _ = C.accumulation_share(only_f.cpu(), t_f, idx, typ, C.U[dtype])
    assert C.accumulation_within(s)


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
def test_batched_api_gradients_per_item(dtype):
    """point_to_mesh_distance with B = 3 and different contents per item: every item's gradients against that item's unbatched call
    and against float64 autograd."""
    g = torch.Generator().manual_seed(21)
    pts = (torch.randn(3, 200, 3, generator=g) * torch.tensor([1., .5, 2.]).view(3, 1, 1)).to(dtype)
    fv = torch.randn(3, 50, 3, 3, generator=g).to(dtype)
    w = (torch.rand(3, 200, generator=g) + 0.5).to(dtype)
    a, b = pts.cuda().requires_grad_(), fv.cuda().requires_grad_()
    dist, idx, typ = _tm().point_to_mesh_distance(a, b)
    (dist * w.cuda()).sum().backward()
    for i in range(3):
        o = oracle.triangle_distance_forward(pts[i], fv[i])
        assert torch.equal(idx[i].cpu(), o[1]) and torch.equal(typ[i].cpu(), o[2])
        g_p, g_f, _, _ = C.check_operator(gpu_backward, w[i], pts[i], fv[i], o[1], o[2], dtype, f'item {i} {dtype}')
        assert torch.equal(a.grad[i].cpu(), g_p)
        t_p, t_f = C.operator_terms(gpu_backward, w[i], pts[i], fv[i], o[1], o[2])
        s, _ = C.accumulation_share(b.grad[i].cpu(), t_f, o[1], o[2], C.U[dtype])
        print(f'item {i} {dtype}: batched face gradient, worst share {np.nanmax(s):.3f}')
        assert C.accumulation_within(s)
