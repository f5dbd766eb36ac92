"""Cases, reference, yardstick and negative controls for the gradient of the point -> triangle distance (test infrastructure; plain
CPU torch / numpy, used by tests/test_triangle_distance_gradient_cpu.py, tests/test_triangle_distance_gradient_gpu.py and
tests/test_triangle_distance.py).

The backward operator takes any in-range (face_idx, dist_type), so every case here PRESCRIBES each point's face and region instead of
waiting for the forward to pick a rare one.  With `face_vertices[face_idx]` as a soup of N faces and `face_idx = arange(N)` ("private
faces") every face has one contributor and the operator returns the per-point terms: 3 values for the point, 9 for the face.

Reference (:func:`sqdist`): the squared distance to the STORED region -- the plane, a vertex, or a clamped edge -- written from the
geometry, not from the kernel; torch autograd of it in float64 with the cotangent `grad` (:func:`reference_terms`).

Yardstick (:func:`yardstick`; float64, from the inputs only).  g = 2|grad|, e_max the face's longest edge, len = |n|, pv = |p - v1|; for
an edge a -> b: pb = |p - a|, L = |b - a|.
    region      M_p (the point's 3 values)     M_f (the face's 9 values from this point)
    plane       g pv e_max^2 / len             M_p (1 + pv e_max / len)
    vertex t    g |p - v_t|                    the same
    edge        g (pb + L)                     M_p (1 + pb / L)
A term passes when max_c |got - want| <= K u M (u = 2^-24 / 2^-53).  The factors are the conditioning of the formulas: dot(pv, un)
cancels against |pv|, and the edge's m_bar carries l / m^2.

K is measured, not chosen: the worst share that torch FLOAT32 autograd of :func:`sqdist` uses against its own float64 self over the
committed cases (:func:`natural_case` soup and sphere, 20 000 points each, and :func:`prescribed_cases`), times four (the kernel
normalises before it projects and pins 1 / sqrt: about twice the rounded steps of the autograd expression), rounded up.
    measured share (float32 autograd, CPU):  soup 3.02, sphere 3.83, prescribed 1.71      ->      K = ceil(4 * 3.83) = 16
    worst shares under K = 16, CPU:  float32 oracle, fused / unfused: soup 3.02 / 2.66, sphere 6.81 / 6.90, prescribed 2.90 / 2.25
                                     (all in the plane region; vertex and edge regions stay below 1.8; the per-region median is
                                     0.07 - 1.5, so the bound bites in every region);
                                     float64 oracle against float64 autograd: 6.14 units of 2^-53 (sphere; the bound there is 2 K = 32)
    worst shares on the MI355X:      the HIP kernel's terms equal the fused oracle's bit for bit in all 48 private-face cases and in
                                     the clamped, short-edge and shared cases, float32 and float64, so its shares are the oracle's;
                                     forward-chosen regions at N = 2000: soup 1.76, sphere 6.62 (float32), 1.53 / 5.47 (float64);
                                     test_gpu_vs_oracle at 30 000 points on the 5 120-face sphere: 8.29 (float32), 6.52 (float64);
                                     accumulation: 0.027 of gamma_(n-1) sum|term| with 513 points on one face (n up to 294 per
                                     value), up to 0.998 where n = 2 (ONE rounding of the sum of two like-signed terms uses
                                     the whole of gamma_1 = u: the bound cannot be tighter)
(tests/test_triangle_distance_gradient_cpu.py re-measures the share and fails when K is not what the rule gives.)

Accumulation (:func:`accumulation_share`): a face's value is the sum of its contributors' terms, added with atomics in no fixed order:
|got - want| <= gamma_(n-1) sum|term| per element, gamma_k = k u / (1 - k u), n = the element's OWN number of contributors (a region
touches 3, 6 or 9 of the face's values), want = the sum of the same per-point terms.  There is no K in it; n = 1 means equality and
n = 0 means +0.0.  `want` is summed in extended precision (numpy longdouble), so that for float64 terms it carries no rounding
of its own that the bound would have to cover."""
import math

import numpy as np
import torch

U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
K = 16
# which of the face's nine values a region's formula writes (bit c: value c of v1.xyz v2.xyz v3.xyz)
MASK = (0x1FF, 0x007, 0x038, 0x1C0, 0x03F, 0x1F8, 0x1C7)
EDGE = {4: (0, 1), 5: (1, 2), 6: (2, 0)}             # type -> (a, b) of the edge a -> b
REGION_NAMES = ('plane', 'v1', 'v2', 'v3', 'e12', 'e23', 'e31')

SIZES = (1, 63, 64, 65, 255, 256, 257, 513)           # either side of a wavefront (64) and of a workgroup (256)
LAYOUTS = ('cyclic', 'wave', 'block')


# ---------------------------------------------------------------------------------------------------------------- the reference
def sqdist(p, tri, typ, clamp=True):
    """Squared distance of p (N, 3) to the stored region `typ` (N) of its own triangle tri (N, 3, 3)."""
    out = p.new_zeros(p.shape[0])
    for t in range(7):
        m = typ == t
        if not bool(m.any()):
            continue
        q, v = p[m], tri[m]
        if t == 0:
            n = torch.linalg.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
            out[m] = (((q - v[:, 0]) * n).sum(-1) / n.norm(dim=-1)) ** 2
        elif t <= 3:
            out[m] = ((q - v[:, t - 1]) ** 2).sum(-1)
        else:
            a, b = v[:, EDGE[t][0]], v[:, EDGE[t][1]]
            k = ((b - a) * (q - a)).sum(-1) / ((b - a) ** 2).sum(-1)
            if clamp:
                k = k.clamp(0, 1)
            out[m] = ((k[:, None] * (b - a) - (q - a)) ** 2).sum(-1)
    return out


def reference_terms(grad, pts, fv, idx, typ, dtype=torch.float64, clamp=True):
    """Autograd of :func:`sqdist` in `dtype` with cotangent grad -> per-point terms (N, 3), (N, 9)."""
    p = pts.to(dtype).clone().requires_grad_()
    tri = fv.to(dtype)[idx].clone().requires_grad_()
    gp, gt = torch.autograd.grad(sqdist(p, tri, typ, clamp), (p, tri), grad.to(dtype))
    return gp, gt.reshape(-1, 9)


def operator_terms(backward, grad, pts, fv, idx, typ):
    """The per-point terms of a backward operator `backward(grad, pts, fv, idx, typ) -> (g_points, g_faces)` through private faces."""
    n = pts.shape[0]
    gp, gf = backward(grad, pts, fv[idx].contiguous(), torch.arange(n), typ)
    return gp, gf.reshape(n, 9)


# ---------------------------------------------------------------------------------------------------------------- the yardstick
def yardstick(grad, pts, fv, idx, typ):
    """-> (M_p, M_f), float64 (N) each: the module docstring's table."""
    p, tri, g = pts.double(), fv.double()[idx], 2 * grad.double().abs()
    rows, t = torch.arange(p.shape[0]), typ.long()
    elen = (tri.roll(-1, 1) - tri).norm(dim=-1)                          # |v2 - v1|, |v3 - v2|, |v1 - v3|
    e_max = elen.max(dim=1).values
    length = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]).norm(dim=-1)
    pv = (p - tri[:, 0]).norm(dim=-1)
    plane_p = g * pv * e_max ** 2 / length
    plane_f = plane_p * (1 + pv * e_max / length)
    vert = g * (p - tri[rows, (t - 1).clamp(0, 2)]).norm(dim=-1)
    e = (t - 4).clamp(0, 2)
    pb, L = (p - tri[rows, e]).norm(dim=-1), elen[rows, e]
    edge_p = g * (pb + L)
    edge_f = edge_p * (1 + pb / L)
    m_p = torch.where(t == 0, plane_p, torch.where(t <= 3, vert, edge_p))
    m_f = torch.where(t == 0, plane_f, torch.where(t <= 3, vert, edge_f))
    return m_p, m_f


def share(got, want, m, u):
    """Per point: max_c |got - want| / (u M), float64; 0 where got == want (M may be 0 there: grad = 0, a point on its vertex);
    inf where they differ and M = 0; NaN (which no bound admits) where either is NaN."""
    d = (got.double() - want.double()).abs().amax(dim=1)
    return torch.where(d == 0, torch.zeros_like(d), d / (u * m))


def term_shares(got_p, got_f, grad, pts, fv, idx, typ, u, want=None):
    """-> (share of the point's values, share of the face's values) against the float64 reference (or `want` = (p, f))."""
    want_p, want_f = reference_terms(grad, pts, fv, idx, typ) if want is None else want
    m_p, m_f = yardstick(grad, pts, fv, idx, typ)
    return share(got_p, want_p, m_p, u), share(got_f, want_f, m_f, u)


def worst_by_region(s, typ):
    """{region name: (worst, median, count)} of a per-point share."""
    out = {}
    for t in range(7):
        v = s[typ == t]
        if v.numel():
            out[REGION_NAMES[t]] = (float(v.max()) if not bool(v.isnan().any()) else float('nan'), float(v.median()), int(v.numel()))
    return out


def fmt_regions(tag, s_p, s_f, typ):
    s = torch.maximum(s_p, s_f)
    return tag + ': ' + '  '.join(f'{k} {w:.2f} (med {m:.2f}, n {n})' for k, (w, m, n) in worst_by_region(s, typ).items())


def terms_within(s_p, s_f, k=K):
    return bool((s_p <= k).all()) and bool((s_f <= k).all())          # (NaN fails)


def old_max_norm_passes(got, want):
    """The assertion this bound replaces: one tolerance scaled by the tensor's largest element."""
    return float((got.double() - want.double()).abs().max()) <= 1e-5 * max(float(want.double().abs().max()), 1e-30)


# ---------------------------------------------------------------------------------------------------------------- accumulation
def touched_bits(typ):
    """(N, 9) 0 / 1: the face values a point's region writes."""
    return (torch.tensor(MASK)[typ.long()][:, None] >> torch.arange(9)[None, :]) & 1


def accumulate(term_f, idx, typ, num_faces):
    """-> want (F, 9) longdouble, sum of magnitudes (F, 9) longdouble, contributor count per element (F, 9) int64."""
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, 'extended precision needed for the sums of float64 terms'
    t = term_f.double().numpy().astype(np.longdouble)
    want, mag = np.zeros((num_faces, 9), np.longdouble), np.zeros((num_faces, 9), np.longdouble)
    count = np.zeros((num_faces, 9), np.int64)
    np.add.at(want, idx.numpy(), t)
    np.add.at(mag, idx.numpy(), np.abs(t))
    np.add.at(count, idx.numpy(), touched_bits(typ).numpy())
    return want, mag, count


def accumulation_share(got_f, term_f, idx, typ, u):
    """|got - want| / (gamma_(n-1) sum|term|) per element, (F, 9) float64: 0 where got == want, inf where they differ and the bound is
    0 (n <= 1: equality is asked), NaN where got is NaN.  -> (share, count)"""
    num_faces = got_f.shape[0]
    want, mag, count = accumulate(term_f, idx, typ, num_faces)
    k = np.maximum(count - 1, 0).astype(np.longdouble)
    bound = k * u / (1 - k * u) * mag
    d = np.abs(got_f.double().numpy().reshape(num_faces, 9).astype(np.longdouble) - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = np.where(d == 0, 0.0, d / bound)
    return s.astype(np.float64), count


def accumulation_within(s):
    return bool((s <= 1.0).all())                                      # (NaN fails)


def gpu_backward(grad, pts, fv, idx, typ):
    """The HIP backward through its shim, CPU tensors in, CPU tensors out (gradients pre-zeroed, as the autograd function does).  The
    shim does not range-check: only indices in [0, F) and types 0 .. 6 leave this function."""
    from kaolin_amd import _C
    assert fv.shape[0] > 0 and idx.dtype == torch.long and typ.dtype == torch.int32 and idx.shape == typ.shape == pts.shape[:1]
    assert int(idx.min()) >= 0 and int(idx.max()) < fv.shape[0] and int(typ.min()) >= 0 and int(typ.max()) <= 6
    g_p, g_f = torch.zeros_like(pts, device='cuda'), torch.zeros_like(fv, device='cuda')
    _C.metrics.unbatched_triangle_distance_backward_cuda(grad.cuda().contiguous(), pts.cuda().contiguous(), fv.cuda().contiguous(),
                                                         idx.cuda(), typ.cuda(), g_p, g_f)
    return g_p.cpu(), g_f.cpu()


def check_operator(backward, grad, pts, fv, idx, typ, dtype, tag=''):
    """What every comparison of a whole backward call asks, for `backward` run at `dtype` on CPU tensors in, CPU tensors out:
    its per-point terms (private faces) within K u M of float64 autograd; its g_points equal to those terms (one term, stored); its
    g_faces within the accumulation bound of the sum of those terms.  -> (g_points, g_faces, worst term share, worst accumulation share)"""
    grad, pts, fv = grad.to(dtype), pts.to(dtype), fv.to(dtype)
    u = U[dtype]
    t_p, t_f = operator_terms(backward, grad, pts, fv, idx, typ)
    s_p, s_f = term_shares(t_p, t_f, grad, pts, fv, idx, typ, u)
    print(fmt_regions(f'{tag} terms / (u M)', s_p, s_f, typ))
    assert terms_within(s_p, s_f), fmt_regions('terms outside K u M', s_p, s_f, typ)
    g_p, g_f = backward(grad, pts, fv, idx, typ)
    assert torch.equal(g_p, t_p), 'g_points differs from the per-point terms'
    s_a, count = accumulation_share(g_f, t_f, idx, typ, u)
    print(f'{tag} accumulation: worst share {np.nanmax(s_a) if s_a.size else 0.0:.3f} of gamma_(n-1) sum|term|, '
          f'n up to {int(count.max()) if count.size else 0}')
    assert accumulation_within(s_a), f'{int((~(s_a <= 1.0)).sum())} face values outside gamma_(n-1) sum|term|'
    worst_t = float(torch.maximum(s_p, s_f).max()) if s_p.numel() else 0.0
    return g_p, g_f, worst_t, float(np.nanmax(s_a)) if s_a.size else 0.0


# ---------------------------------------------------------------------------------------------------------------- the cases
# Every case: (grad (N), points (N, 3), face_vertices (F, 3, 3), face_idx (N) int64, dist_type (N) int32).  Values are drawn in float32
# and converted, so float32 and float64 runs see the same numbers.
def layout_types(layout, n):
    """cyclic: all seven regions in every wavefront; wave / block: one region per 64 / 256 points (its `touched` mask fills the whole
    wavefront / workgroup), starting at region n % 7 so that the sizes of SIZES cover all seven between them."""
    i = torch.arange(n)
    t = {'cyclic': i, 'wave': i // 64 + n, 'block': i // 256 + n}[layout] % 7
    return t.to(torch.int32)


def private_case(layout, n, dtype=torch.float32):
    g = torch.Generator().manual_seed(1000 * LAYOUTS.index(layout) + n)
    fv = torch.randn(n, 3, 3, generator=g)
    pts = torch.randn(n, 3, generator=g)
    grad = torch.rand(n, generator=g) + 0.5
    return grad.to(dtype), pts.to(dtype), fv.to(dtype), torch.arange(n), layout_types(layout, n)


CLAMP_K = (-0.5, 0.0, 0.25, 1.0, 1.5)
CLAMP_GRADS = (0.0, -1.5, 1e6, 0.75)


def clamp_case(dtype=torch.float32):
    """Edge regions with the edge parameter k below 0, at 0, inside, at 1 and above 1 -- points and faces of exact binary fractions,
    so k = l / m is exact in float32 (tests/test_triangle_distance_gradient_cpu.py asserts it) -- with grad zero, negative, 1e6 and
    ordinary.  -> case + the prescribed k (N)."""
    base = torch.tensor([[0., 0., 0.], [1., 0., 0.], [0., 1., 0.]])
    # a vector of binary fractions perpendicular to each edge direction (v2 - v1, v3 - v2, v1 - v3), with a part out of the plane
    perp = {4: torch.tensor([0., -1., 1.]), 5: torch.tensor([1., 1., .5]), 6: torch.tensor([-1., 0., .5])}
    shift = torch.tensor([.5, .25, -1.])
    fv, pts, typ, ks, grads = [], [], [], [], []
    for t in (4, 5, 6):
        for k in CLAMP_K:
            for scale in (1., 2., .5):
                for off in (.25, -.75):
                    for grad in CLAMP_GRADS:
                        tri = base * scale + shift
                        a, b = tri[EDGE[t][0]], tri[EDGE[t][1]]
                        fv.append(tri)
                        pts.append(a + k * (b - a) + off * scale * perp[t])
                        typ.append(t)
                        ks.append(k)
                        grads.append(grad)
    n = len(pts)
    case = (torch.tensor(grads).to(dtype), torch.stack(pts).to(dtype), torch.stack(fv).to(dtype), torch.arange(n),
            torch.tensor(typ, dtype=torch.int32))
    return case, torch.tensor(ks)


def short_edge_case(dtype=torch.float32, per_type=70):
    """Edge regions on an edge 2^-10 times as long as the point is far: L = 2^-10 r, p = a + k (b - a) + r w with w perpendicular to
    the edge and k drawn from (-0.5, 1.5): l / m^2 is 2^20 times 1 / r^2, the conditioning M_f's factor 1 + pb / L stands for."""
    g = torch.Generator().manual_seed(77)
    n = 3 * per_type
    typ = (torch.arange(n) % 3 + 4).to(torch.int32)
    a = torch.randn(n, 3, generator=g, dtype=torch.float64)
    d = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=torch.float64), dim=-1)
    w = torch.nn.functional.normalize(torch.linalg.cross(d, torch.randn(n, 3, generator=g, dtype=torch.float64)), dim=-1)
    r = torch.rand(n, 1, generator=g, dtype=torch.float64) + 0.5
    k = torch.rand(n, 1, generator=g, dtype=torch.float64) * 2 - 0.5
    b = a + d * r * 2.0 ** -10
    pts = a + k * (b - a) + r * w
    third = torch.randn(n, 3, generator=g, dtype=torch.float64)
    fv = torch.empty(n, 3, 3, dtype=torch.float64)
    for t in (4, 5, 6):
        m = typ == t
        ia, ib = EDGE[t]
        fv[m, ia], fv[m, ib], fv[m, 3 - ia - ib] = a[m], b[m], third[m]
    grad = torch.rand(n, generator=g) + 0.5
    f32 = lambda x: x.float().to(dtype)                                # noqa: E731
    return f32(grad), f32(pts), f32(fv), torch.arange(n), typ


def prescribed_cases(dtype=torch.float32):
    """{name: case}: every private-face case of the GPU tests."""
    out = {f'{layout}-{n}': private_case(layout, n, dtype) for layout in LAYOUTS for n in SIZES}
    out['clamp'] = clamp_case(dtype)[0]
    out['short_edge'] = short_edge_case(dtype)
    return out


def concat_cases(cases):
    """Private-face cases side by side as one (face indices shifted)."""
    grad, pts, fv, idx, typ, base = [], [], [], [], [], 0
    for c in cases:
        grad.append(c[0]); pts.append(c[1]); fv.append(c[2]); idx.append(c[3] + base); typ.append(c[4])   # noqa: E702
        base += c[2].shape[0]
    return tuple(torch.cat(x) for x in (grad, pts, fv, idx, typ))


def natural_inputs(kind, n, seed=1, dtype=torch.float32):
    """The inputs of the two scenes: 'soup' = 300 randn faces and n randn points; 'sphere' = the 1280-face geodesic sphere of radius
    0.5 and n points in [-0.6, 0.6]^3; grad = rand + 0.5.  -> (grad, points, face_vertices)"""
    g = torch.Generator().manual_seed(seed)
    if kind == 'soup':
        fv = torch.randn(300, 3, 3, generator=g)
        pts = torch.randn(n, 3, generator=g)
    else:
        from kaolin_amd.utils.testing import geodesic_sphere
        v, f = geodesic_sphere(8)
        fv = v.float()[f].contiguous()
        pts = torch.rand(n, 3, generator=g) * 1.2 - 0.6
    return (torch.rand(n, generator=g) + 0.5).to(dtype), pts.to(dtype), fv.to(dtype)


def natural_case(kind, forward, n=20000, forced=1750, dtype=torch.float32):
    """A scene of :func:`natural_inputs` with the face and region `forward(points, face_vertices) -> (dist, idx, type)` chooses; the
    last `forced` points keep their nearest face and get regions 0 .. 6 in turn (the forward picks a vertex region for ~2 % of a
    soup's points and for 1 in 10 000 on the sphere), so that every region holds at least forced / 7 points."""
    grad, pts, fv = natural_inputs(kind, n, dtype=dtype)
    _, idx, typ = forward(pts, fv)
    typ = typ.clone()
    if forced:
        typ[n - forced:] = (torch.arange(forced) % 7).to(torch.int32)
    return grad, pts, fv, idx, typ


def shared_cases(dtype=torch.float32):
    """{name: case} where faces are shared: 513 points on the one face of F = 1 (every wavefront: 64 lanes on one address); all on the
    middle face of F = 3 (the outer faces nobody hits stay +0.0); the 64 lanes of a wavefront on 2 faces in turn; F = 300 at random."""
    g = torch.Generator().manual_seed(5)
    out = {}
    for name, n, num_faces in (('one_face', 513, 1), ('middle_of_3', 513, 3), ('alternating_2', 64, 2), ('random_300', 513, 300)):
        fv = torch.randn(num_faces, 3, 3, generator=g)
        pts = torch.randn(n, 3, generator=g)
        grad = torch.rand(n, generator=g) + 0.5
        typ = (torch.randperm(n, generator=g) % 7).to(torch.int32)
        idx = {'one_face': torch.zeros(n, dtype=torch.long), 'middle_of_3': torch.ones(n, dtype=torch.long),
               'alternating_2': torch.arange(n) % 2, 'random_300': torch.randint(0, 300, (n,), generator=g)}[name]
        out[name] = (grad.to(dtype), pts.to(dtype), fv.to(dtype), idx, typ)
    return out


# ---------------------------------------------------------------------------------------------------------------- negative controls
# Applied to ARRAYS of terms (never to a kernel): what a subtly wrong kernel would hand back.  Each must fail the new check.
def control_rounded(t_p, t_f, i):
    """One intermediate of point i rounded to 12 bits: its terms off by a factor 1 + 2^-12."""
    t_p, t_f = t_p.clone(), t_f.clone()
    t_p[i] *= 1 + 2.0 ** -12
    t_f[i] *= 1 + 2.0 ** -12
    return t_p, t_f


def control_wrong_mask(t_f, typ, i):
    """Point i of region 5 (edge v2 -> v3, mask 0x1F8) written through region 6's mask 0x1C7: its v2 block lands on v1."""
    assert int(typ[i]) == 5
    t_f = t_f.clone()
    t_f[i, 0:3] = t_f[i, 3:6]
    t_f[i, 3:6] = 0
    return t_f


def control_unclamped(grad, pts, fv, idx, typ, dtype):
    """dj_dk forced to 1: the gradient of the UNCLAMPED edge formula, in `dtype` (it differs where k is outside [0, 1])."""
    return reference_terms(grad, pts, fv, idx, typ, dtype=dtype, clamp=False)


def control_dropped_lane(term_f, idx, typ, num_faces, drop, dtype):
    """The face values summed without contributor `drop` -> (F, 9) in `dtype`."""
    keep = torch.arange(term_f.shape[0]) != drop
    want, _, _ = accumulate(term_f[keep], idx[keep], typ[keep], num_faces)
    return torch.from_numpy(want.astype(np.float64)).to(dtype)


def rule_k(measured):
    return int(math.ceil(4 * measured))
