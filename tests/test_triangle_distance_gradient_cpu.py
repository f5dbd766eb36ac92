"""The gradient of the point -> triangle distance, CPU part: the oracle's backward (oracle/tridist_oracle.inc, the restated kernel the HIP
path is compared with bit for bit) against an independent formulation -- float64 autograd of the squared distance to the stored region
-- per point, per region, under the conditioned bound K u M of tests/triangle_distance_gradient_cases.py; K re-measured; the
prescribed cases still reach their edges; and four negative controls that the new check rejects, two of which the max-norm assertion
it replaces lets through."""
import numpy as np
import pytest
import torch

import oracle
import triangle_distance_gradient_cases as C

F32, F64 = torch.float32, torch.float64


def _forward(pts, fv):
    return oracle.triangle_distance_forward(pts, fv, omp=True)


@pytest.fixture(scope='module')
def cases():
    """{name: (case, float64 reference terms)}: the two scenes at 20 000 points and all prescribed cases as one.  Read only."""
    out = {'soup': C.natural_case('soup', _forward), 'sphere': C.natural_case('sphere', _forward),
           'prescribed': C.concat_cases(C.prescribed_cases().values())}
    return {k: (c, C.reference_terms(*c)) for k, c in out.items()}


def _oracle(fused):
    return lambda *a: oracle.triangle_distance_backward(*a, fused=fused)


@pytest.mark.parametrize('name', ['soup', 'sphere', 'prescribed'])
def test_every_region_holds_200_points(cases, name):
    typ = cases[name][0][4]
    counts = torch.bincount(typ.long(), minlength=7)
    print(name, dict(zip(C.REGION_NAMES, counts.tolist())))
    assert int(counts.min()) >= 200


def test_k_is_four_times_the_measured_share(cases):
    """K comes from the reference at working precision -- torch float32 autograd of the same formulation against its float64 self --
    not from the kernel or the oracle: K = ceil(4 x worst share)."""
    worst = {}
    for name, (case, ref) in cases.items():
        a32 = C.reference_terms(*case, dtype=F32)
        s_p, s_f = C.term_shares(a32[0], a32[1], *case, C.U[F32], want=ref)
        print(C.fmt_regions(f'{name}: float32 autograd / (u M)', s_p, s_f, case[4]))
        worst[name] = float(torch.maximum(s_p, s_f).max())
    measured = max(worst.values())
    print(f'measured share {worst} -> K = {C.rule_k(measured)} (committed: {C.K})')
    # (the rule, re-applied with this machine's torch: float32 autograd on another instruction set may round a reduction differently
    # and move the share by a few per cent, so the committed K may sit one beside the rule's; a stale K does not)
    assert abs(C.rule_k(measured) - C.K) <= 1


@pytest.mark.parametrize('fused', [True, False], ids=['fused', 'unfused'])
@pytest.mark.parametrize('name', ['soup', 'sphere', 'prescribed'])
def test_float32_oracle_terms_within_bound_of_float64_autograd(cases, name, fused):
    case, ref = cases[name]
    t_p, t_f = C.operator_terms(_oracle(fused), *case)
    s_p, s_f = C.term_shares(t_p, t_f, *case, C.U[F32], want=ref)
    print(C.fmt_regions(f'{name} float32 oracle {"fused" if fused else "unfused"} / (u M)', s_p, s_f, case[4]))
    assert C.terms_within(s_p, s_f)


@pytest.mark.parametrize('name', ['soup', 'sphere', 'prescribed'])
def test_float64_oracle_terms_within_bound_of_float64_autograd(cases, name):
    """Two float64 evaluations, each with its own error: 2 K u64 M."""
    case, ref = cases[name]
    grad, pts, fv, idx, typ = case
    c64 = (grad.double(), pts.double(), fv.double(), idx, typ)
    t_p, t_f = C.operator_terms(oracle.triangle_distance_backward, *c64)
    s_p, s_f = C.term_shares(t_p, t_f, *c64, C.U[F64], want=ref)
    print(C.fmt_regions(f'{name} float64 oracle / (u64 M)', s_p, s_f, typ))
    assert C.terms_within(s_p, s_f, 2 * C.K)


def test_private_faces_return_the_terms_unchanged():
    """The construction everything rests on: the oracle accumulates in double and rounds once, so with one contributor per face its
    face gradient IS that contributor's float term; and summing those terms in any order reproduces a shared-face call within the
    accumulation bound (the oracle's own double sum: well inside)."""
    for dtype in (F32, F64):
        for name, case in C.shared_cases(dtype).items():
            grad, pts, fv, idx, typ = case
            t_p, t_f = C.operator_terms(oracle.triangle_distance_backward, *case)
            g_p, g_f = oracle.triangle_distance_backward(*case)
            assert torch.equal(g_p, t_p)
            # untouched values of a term are +0.0
            assert bool((t_f[C.touched_bits(typ) == 0] == 0).all())
            s, count = C.accumulation_share(g_f, t_f, idx, typ, C.U[dtype])
            print(f'{name} {dtype}: oracle sum, worst share {s.max():.3f}, n up to {count.max()}')
            assert C.accumulation_within(s)
            assert bool((g_f.reshape(-1, 9)[torch.from_numpy(count == 0)] == 0).all())


def test_clamp_case_reaches_its_edges():
    """k = l / m is exact in float32 and takes each of the five prescribed values on each of the three edges, with each grad."""
    (grad, pts, fv, idx, typ), ks = C.clamp_case(F32)
    for t in (4, 5, 6):
        m = typ == t
        a, b = fv[m, C.EDGE[t][0]], fv[m, C.EDGE[t][1]]
        k = ((b - a) * (pts[m] - a)).sum(-1) / ((b - a) ** 2).sum(-1)
        assert torch.equal(k, ks[m])
        for kv in C.CLAMP_K:
            assert set(grad[m][ks[m] == kv].tolist()) == set(torch.tensor(C.CLAMP_GRADS).tolist())
    # clamped points: the gradient is that of the distance to the end vertex, nothing flows along the edge
    ref_p, ref_f = C.reference_terms(grad, pts, fv, idx, typ)
    end = torch.where(ks <= 0, torch.tensor([0, 1, 2])[(typ - 4).long()], torch.tensor([1, 2, 0])[(typ - 4).long()])
    clamped = (ks <= 0) | (ks >= 1)
    want = 2 * grad.double()[:, None] * (pts.double() - fv.double()[idx, end])
    assert torch.equal(ref_p[clamped], want[clamped])


def test_short_edge_case_is_short():
    grad, pts, fv, idx, typ = C.short_edge_case(F32)
    for t in (4, 5, 6):
        m = typ == t
        a, b = fv[m, C.EDGE[t][0]].double(), fv[m, C.EDGE[t][1]].double()
        ratio = (b - a).norm(dim=-1) / (pts[m].double() - a).norm(dim=-1)
        assert float(ratio.max()) < 2.0 ** -9.9 and float(ratio.min()) > 2.0 ** -10.1
        k = ((b - a) * (pts[m].double() - a)).sum(-1) / ((b - a) ** 2).sum(-1)
        assert int((k < 0).sum()) > 5 and int((k > 1).sum()) > 5 and int(((k > 0) & (k < 1)).sum()) > 20


def test_layouts_fill_wavefronts_and_workgroups():
    seen = {layout: set() for layout in C.LAYOUTS}
    for layout in C.LAYOUTS:
        for n in C.SIZES:
            t = C.layout_types(layout, n)
            seen[layout] |= set(t.tolist())
            if layout == 'cyclic' and n >= 7:
                assert set(t[:64].tolist()) == set(range(7))
            if layout != 'cyclic':
                span = 64 if layout == 'wave' else 256
                for s0 in range(0, n, span):
                    assert len(set(t[s0:s0 + span].tolist())) == 1
        assert seen[layout] == set(range(7)), layout


# ---------------------------------------------------------------------------------------------------------------- negative controls
@pytest.fixture(scope='module')
def sphere_terms(cases):
    case, ref = cases['sphere']
    t_p, t_f = C.operator_terms(oracle.triangle_distance_backward, *case)
    return case, ref, t_p, t_f


def _old_passes_terms(got_p, got_f, want_p, want_f):
    return C.old_max_norm_passes(got_p, want_p) and C.old_max_norm_passes(got_f, want_f)


def test_control_twelve_bit_rounding_fails_new_check_passes_old(sphere_terms):
    """One point's terms off by 2^-12 relative -- thousands of float32 roundings.  The max-norm assertion scales its tolerance by the
    LARGEST element of 20 000 points' terms; a point whose own terms are 4 % of that or less may be wrong in its 12th bit."""
    case, ref, t_p, t_f = sphere_terms
    grad, pts, fv, idx, typ = case
    m_p, m_f = C.yardstick(*case)
    small = (t_p.abs().amax(1) < 0.02 * t_p.abs().max()) & (t_f.abs().amax(1) < 0.02 * t_f.abs().max())
    # among those, the point whose term is the largest part of its own yardstick (the check compares with M, not with the term)
    i = int(torch.where(small, ref[0].abs().amax(1) / m_p, torch.zeros_like(m_p)).argmax())
    bad_p, bad_f = C.control_rounded(t_p, t_f, i)
    s_p, s_f = C.term_shares(bad_p, bad_f, *case, C.U[F32], want=ref)
    print(f'12-bit rounding of point {i} (region {int(typ[i])}): shares {float(s_p[i]):.1f} / {float(s_f[i]):.1f} of u M against K = {C.K}; '
          f'old max-norm assertion passes: {_old_passes_terms(bad_p, bad_f, t_p, t_f)}')
    assert not C.terms_within(s_p, s_f)
    assert float(s_p[i]) > C.K and int((torch.maximum(s_p, s_f) > C.K).sum()) == 1
    assert _old_passes_terms(bad_p, bad_f, t_p, t_f)


def test_control_wrong_mask_fails_new_check(sphere_terms):
    case, ref, t_p, t_f = sphere_terms
    typ = case[4]
    i = int((typ == 5).nonzero()[0])
    bad_f = C.control_wrong_mask(t_f, typ, i)
    s_p, s_f = C.term_shares(t_p, bad_f, *case, C.U[F32], want=ref)
    print(f'region-5 point {i} written through 0x1C7: face share {float(s_f[i]):.3g} of u M; '
          f'old max-norm assertion passes: {C.old_max_norm_passes(bad_f, t_f)}')
    assert not C.terms_within(s_p, s_f) and float(s_f[i]) > C.K
    # ... and summed into a shared face, the accumulation check sees it too
    grad, pts, fv, idx, _ = case
    g_f = torch.zeros(fv.shape[0], 9).index_add_(0, idx, bad_f)
    s, _ = C.accumulation_share(g_f, t_f, idx, typ, C.U[F32])
    assert not C.accumulation_within(s)


def test_control_unclamped_edge_fails_new_check():
    (grad, pts, fv, idx, typ), ks = C.clamp_case(F32)
    case = (grad, pts, fv, idx, typ)
    ref = C.reference_terms(*case)
    t_p, t_f = C.operator_terms(oracle.triangle_distance_backward, *case)
    s_p, s_f = C.term_shares(t_p, t_f, *case, C.U[F32], want=ref)
    assert C.terms_within(s_p, s_f)
    bad_p, bad_f = C.control_unclamped(*case, F32)
    s_p, s_f = C.term_shares(bad_p, bad_f, *case, C.U[F32], want=ref)
    outside = ((ks < 0) | (ks > 1)) & (grad != 0)
    print(f'dj_dk = 1 on clamped points: {int((torch.maximum(s_p, s_f) > C.K).sum())} of {int(outside.sum())} clamped points with grad != 0 '
          f'fail; old max-norm assertion passes: {_old_passes_terms(bad_p, bad_f, t_p, t_f)}')
    assert not C.terms_within(s_p, s_f)
    # the face's values differ at every point that is really clamped; nothing else does (k = 0 and k = 1: both formulas agree)
    assert torch.equal(s_f > C.K, outside)


def test_control_dropped_lane_fails_new_check_passes_old():
    """513 contributors on face 0, one of them missing from the sum.  Face 1 is hit once with grad = 1e6 (one of the prescribed grads):
    the max-norm assertion scales by THAT face's values, and face 0 may lose a whole contribution."""
    grad, pts, fv, idx, typ = C.shared_cases(F32)['one_face']
    g = torch.Generator().manual_seed(9)
    fv = torch.cat([fv, torch.randn(1, 3, 3, generator=g)])
    pts = torch.cat([pts, torch.randn(1, 3, generator=g)])
    grad, idx, typ = torch.cat([grad, torch.tensor([1e6])]), torch.cat([idx, torch.tensor([1])]), torch.cat([typ, torch.tensor([0], dtype=torch.int32)])
    case = (grad, pts, fv, idx, typ)
    t_p, t_f = C.operator_terms(oracle.triangle_distance_backward, *case)
    _, g_f = oracle.triangle_distance_backward(*case)
    s, count = C.accumulation_share(g_f, t_f, idx, typ, C.U[F32])
    assert C.accumulation_within(s) and int(count.max()) > 200
    drop = int(t_f[:513].abs().amax(1).argmax())
    bad = C.control_dropped_lane(t_f, idx, typ, 2, drop, F32).reshape(2, 3, 3)
    s, _ = C.accumulation_share(bad, t_f, idx, typ, C.U[F32])
    print(f'lane {drop} dropped from a 513-contributor face: worst share {np.nanmax(s):.1f} of gamma_(n-1) sum|term|; '
          f'old max-norm assertion passes: {C.old_max_norm_passes(bad, g_f)}')
    assert not C.accumulation_within(s)
    assert bool((s[1] == 0).all())                     # (the other face is untouched by the control)
    assert C.old_max_norm_passes(bad, g_f)
