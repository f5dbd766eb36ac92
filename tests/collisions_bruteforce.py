"""The oracle of kaolin_amd.physics.collisions: the detection contract over all pairs in numpy float32 (one rounding per
operation) and by a sweep along x for many points, the contact energy of the reference's test in float64 with its derivatives
by autograd, a bound per element on the reduction of the terms, and the inputs that tests/test_collisions_cpu.py and
tests/test_collisions_gpu.py share."""
import logging

import numpy as np
import torch

from kaolin_amd.physics import collisions

f32 = np.float32


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def detect(dx, x0, obj, static, radius=0.1, detection_ratio=1.5, ignore_ratio=100000.0, max_pairs=10000):
    """-> (total, indices_a, indices_b, normals, gaps) of the contract in kaolin_amd/physics/collisions.py"""
    x0, dx = np.asarray(x0, f32), np.asarray(dx, f32)
    pos, n = x0 + dx, len(x0)
    R, immune = f32(2.0 * radius * detection_ratio), f32(radius * ignore_ratio)
    with np.errstate(invalid='ignore', over='ignore'):
        e, r = pos[:, None] - pos[None], x0[:, None] - x0[None]
        mask = (np.sqrt(_dot(e, e)) <= R) & (np.arange(n)[None] > np.arange(n)[:, None])
        mask &= ~((static[:, None] == 1) & (static[None] == 1)) & ~((obj[:, None] == obj[None]) & (_dot(r, r) < immune))
    return _stored(pos, static, *np.nonzero(mask), max_pairs)                      # row-major: sorted by (a, b)


def _stored(pos, static, a, b, max_pairs):
    """what the contract stores for the contacts (a, b), sorted: the first max_pairs of them"""
    total, a, b = len(a), a[:max_pairs], b[:max_pairs]
    e = pos[a] - pos[b]
    d = np.sqrt(_dot(e, e))[:, None]
    with np.errstate(invalid='ignore', divide='ignore'):
        normals = np.where(d == 0, f32(0), e / d).astype(f32)
    gaps = _dot(e, normals)[:, None] * normals
    return total, np.where(static[a] == 1, -1, a).astype(np.int32), np.where(static[b] == 1, -1, b).astype(np.int32), normals, gaps


def detect_sweep(dx, x0, obj, static, radius=0.1, detection_ratio=1.5, ignore_ratio=100000.0, max_pairs=10000, block=512):
    """`detect` for many points: sorted by x, each block of points against those up to R (1 + 2^-6) further in x (a pair further
    apart in x has fl(ex ex) > R^2, so d > R), with the same float32 expressions"""
    x0, dx = np.asarray(x0, f32), np.asarray(dx, f32)
    pos, n = x0 + dx, len(x0)
    R, immune = f32(2.0 * radius * detection_ratio), f32(radius * ignore_ratio)
    order = np.argsort(pos[:, 0], kind='stable')                               # NaN last
    xs, found = pos[order, 0], []
    with np.errstate(invalid='ignore', over='ignore'):
        for s in range(0, n, block):
            rows = order[s:s + block]
            stop = np.searchsorted(xs, xs[min(s + block, n) - 1] + R * f32(1.015625), side='right')
            cols = order[s:max(stop, s + len(rows))]
            e, r = pos[rows, None] - pos[None, cols], x0[rows, None] - x0[None, cols]
            mask = (np.sqrt(_dot(e, e)) <= R) & (np.arange(len(cols))[None] > np.arange(len(rows))[:, None])   # each sorted pair once
            mask &= ~((static[rows, None] == 1) & (static[None, cols] == 1))
            mask &= ~((obj[rows, None] == obj[None, cols]) & (_dot(r, r) < immune))
            i, j = np.nonzero(mask)
            found.append(np.stack([np.minimum(rows[i], cols[j]), np.maximum(rows[i], cols[j])], axis=1))
    pairs = np.concatenate(found)
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    return _stored(pos, static, pairs[:, 0], pairs[:, 1], max_pairs)


def radii(radius=0.05, detection_ratio=1.5):
    """(R, S) of csrc/collisions.hip: the detection radius and the cell edge R (1 + 2^-6), float32"""
    R = f32(2.0 * radius * detection_ratio)
    return R, R * f32(1.015625)


def cell(p, S):
    """cl_cell of csrc/collisions.hip in numpy float32: clamp(floor(p / S), -2^15, 2^15 - 1) + 2^15, a NaN quotient on the lower bound"""
    with np.errstate(invalid='ignore', over='ignore'):
        return np.fmin(np.fmax(np.floor(np.asarray(p, f32) / f32(S)), f32(-32768)), f32(32767)).astype(np.int64) + 32768


STRADDLE_FACES = (0, -1, 1, 1000, -1000, 32000, -32000)
HUGE = 8                                                                       # the last points of 'huge'


def _straddle():
    """Pairs (2 i, 2 i + 1), three or more apart from each other in a coordinate.  Per axis and face k S: a one float32 step below
    the face, b = a + R along the axis.  Then pairs one cell apart on two and on three axes, d = 0.999 R"""
    R, S = radii()
    down = lambda k: np.nextafter(f32(k) * S, f32(-np.inf))
    pts = []
    for axis in range(3):
        for k in STRADDLE_FACES:
            a = np.full(3, 3.0 * (len(pts) // 2 + 1) + 0.07, f32)
            a[axis] = down(k)
            b = a.copy()
            b[axis] = a[axis] + R
            pts += [a, b]
    for k in (3, -5):
        for axes, z in (((0, 1), 300.0), ((0, 1, 2), 0.0)):
            a = np.array([0, 0, z], f32)
            a[list(axes)] = down(k)
            b = a.copy()
            b[list(axes)] += f32(0.999) * R / f32(np.sqrt(len(axes)))
            pts += [a, b]
    return np.stack(pts)


def detection_case(name):
    """-> (dx, x0, obj, static, constructor arguments)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    kw = dict(collision_particle_radius=0.05)                                  # R = 0.15, cell edge 0.152
    if name == 'n4097':                                                        # 2.7 contacts a point: three sort blocks, five scan blocks
        n, x0 = 4097, rng.uniform(0.0, 1.7, (4097, 3))
    elif name == 'n65537':                                                     # 1.3 contacts a point: 17-bit indices in the emit keys
        n, x0 = 65537, rng.uniform(0.0, 1.0, (65537, 3)) * [100.0, 1.25, 1.25]
    elif name == 'straddle':
        x0 = _straddle()
        n = len(x0)
    elif name in ('clamp_hi', 'clamp_lo'):                                     # the clamp of cl_cell lies at 32767 S = 4991.85 and at -32768 S = -4992
        n, x0 = 300, rng.uniform(4991.0, 4992.6, (300, 3)) if name == 'clamp_hi' else rng.uniform(-4992.8, -4991.2, (300, 3))
    elif name == 'huge':                                                       # finite, their differences are not
        n, x0 = 70 + HUGE, rng.uniform(-0.2, 0.2, (70 + HUGE, 3))
        x0[70:] = [[1e30, 0, 0], [-1e30, 0.1, 0], [0, 3e38, 0], [0, -3e38, 0], [0.1, 0, 3e38], [0, 0, -3e38], [3e38, 3e38, 3e38], [-3e38, 3e38, -1e30]]
    elif name[1:].isdigit():                                                   # negative coordinates, points on either side of cell faces
        n = int(name[1:])
        x0 = rng.uniform(-0.3, 0.3, (n, 3))
    elif name == 'one_cell':
        n, x0 = 65, rng.uniform(0.0, 0.1, (65, 3))
    elif name == 'exact':                                                      # R = 0.75 exactly: d == R is a contact, one float32 step beyond is not
        kw = dict(collision_particle_radius=0.25)
        n, x0 = 4, np.array([[0, 0, 0], [0.75, 0, 0], [0, 5, 0], [np.nextafter(f32(0.75), f32(1)), 5, 0]])
    elif name == 'duplicates':
        n, x0 = 40, rng.uniform(-0.2, 0.2, (40, 3))
        x0[7] = x0[8] = x0[21]                                                 # objects 1, 0, 1: two contacts at d == 0
    elif name == 'nan':
        n, x0 = 70, rng.uniform(-0.2, 0.2, (70, 3))
        x0[11, 1], x0[30, 0] = np.nan, np.inf
    elif name == 'immune':                                                     # same object: a contact only from 0.1 apart
        kw['ignore_self_collision_ratio'] = 0.2
        n, x0 = 80, rng.uniform(-0.2, 0.2, (80, 3))
    elif name == 'static':                                                     # the reference's two_objects_one_static, and a static pair of two more objects
        n, x0 = 42, np.concatenate([rng.uniform(0, 1, (40, 3)), [[3, 3, 3], [3.05, 3, 3]]])
    elif name == 'none':
        n, x0 = 30, np.arange(90.0).reshape(30, 3)
    dx = rng.uniform(-0.01, 0.01, (n, 3)) * (name not in ('exact', 'straddle'))
    if name == 'duplicates':
        dx[7] = dx[8] = dx[21]
    obj, static = (np.arange(n) % 2).astype(np.int32), np.zeros(n, np.int32)
    if name == 'static':
        obj = np.concatenate([np.repeat([0, 1], 20), [2, 3]]).astype(np.int32)
        dx[20:40, 1] += 0.5
        static[:20], static[40:] = 1, 1
    return dx.astype(f32), x0.astype(f32), obj, static, kw


DETECTION_CASES = ['n1', 'n63', 'n64', 'n65', 'n257', 'one_cell', 'exact', 'duplicates', 'nan', 'immune', 'static', 'none']
# across cell faces, at the clamp of the cell coordinates, with overflowing differences, past one sort and one scan block
EDGE_DETECTION_CASES = ['straddle', 'clamp_hi', 'clamp_lo', 'huge', 'n4097']
ROOM = {'n4097': 1 << 15, 'n65537': 1 << 18}                                   # max_pairs above the case's total
MAX_PAIRS_EDGES = ['1', 'T-1', 'T', 'T+1', 'offs[k]', 'offs[k]+1']


def max_pairs_edge(label, name='n257'):
    """max_pairs around the total T of a case and around offs[k], the number of contacts of the points before a point k that has some"""
    dx, x0, obj, static, kw = detection_case(name)
    T, ia, *_ = detect(dx, x0, obj, static, kw['collision_particle_radius'], max_pairs=1 << 30)
    offs = np.concatenate([[0], np.cumsum(np.bincount(ia, minlength=len(x0)))])
    k = next(k for k in range(len(x0) // 2, len(x0)) if offs[k] < offs[k + 1])
    assert 1 < offs[k] < offs[k] + 1 < T - 1
    return {'1': 1, 'T-1': T - 1, 'T': T, 'T+1': T + 1, 'offs[k]': int(offs[k]), 'offs[k]+1': int(offs[k]) + 1}[label]


def check_detection(name, device, caplog, max_pairs=10000, oracle=detect):
    """detect_collisions on `device` against the oracle: torch.equal on all four tensors, twice"""
    dx, x0, obj, static, kw = detection_case(name)
    total, *expected = oracle(dx, x0, obj, static, kw['collision_particle_radius'], 1.5, kw.get('ignore_self_collision_ratio', 100000.0),
                              max_pairs)
    col = collisions.Collision(dt=0.01, max_contacting_pairs=max_pairs, **kw)
    results = []
    for _ in range(2):
        with caplog.at_level(logging.WARNING):
            caplog.clear()
            col.detect_collisions(*(torch.from_numpy(t).to(device) for t in (dx, x0, obj, static)))
        assert ('contact buffer size exceed' in caplog.text) == (total > max_pairs)
        results.append((col.collision_indices_a, col.collision_indices_b, col.collision_normals, col.collision_kinematic_gaps))
        assert col.num_contacts == min(total, max_pairs) == len(expected[0])
        for got, want in zip(results[-1], expected):
            assert got.device.type == device and torch.equal(got.cpu(), torch.from_numpy(want)), name
        assert torch.equal(col.cp_dx_at_nm_iteration_0.cpu(), torch.from_numpy(dx))
    assert all(torch.equal(p, q) for p, q in zip(*results))
    return col, total


# ---- the contact terms ------------------------------------------------------------------------------------------------------------------
PARAMS = dict(dt=1.0, collision_particle_radius=0.1, impenetrable_barrier_ratio=0.5, friction_regularization=0.1, friction_fluid=0.1,
              friction=0.5)
RADIUS, RP, MU, MU_DT, NU = 0.1, 0.5, 0.5, 0.1, 0.01      # the kernels' constants for PARAMS
COEFF = 0.7
# |vt| of the three friction regimes of contact c % 3.  The float32 and the float64 evaluation must take the same branch, so |vt|
# stays a tenth away from 1 and, in the first regime, two decades below 1e-4 once the float32 rounding of the inputs (an offset
# of 0.2 carries 1e-8, |vt| = |t| / 0.1 carries 2e-7) is in: terms64 asserts |vt| < 1e-6 there.  In that regime the reference's
# Hessian is a limit form that leaves out terms of relative size |vt| / dt <= 1e-5: LIMIT_FORM bounds what the float64
# formulation may differ from autograd by, and the float32 definition and the kernel carry it alike.
LIMIT_FORM = 1e-6 / MU_DT
VT_RANGES = ((1e-9, 1e-8), (1e-2, 0.9), (1.1, 3.0))


def energy64(offset, nor, rc):
    """The reference test's _collision_contact_energy_analytical per contact, float64"""
    d = (offset * nor).sum(-1)
    d_hat = d / rc
    active = (d_hat > RP) & (d_hat <= 1.0)
    dc, dp = d_hat - 1.0, torch.where(active, d_hat - RP, torch.ones_like(d_hat))
    dE = -dc * (2.0 * torch.log(dp) + dc / dp)
    vtn = ((offset - d[:, None] * nor) / MU_DT).norm(dim=-1)
    h_vt = 0.5 * NU * vtn * vtn + torch.where(vtn < 1.0, vtn * vtn * (1.0 - vtn / 3.0), vtn - 1.0 / 3.0)
    return COEFF * torch.where(active, -dc * dc * torch.log(dp) - MU * dE / rc * MU_DT * h_vt, torch.zeros_like(d))


def synthetic(C, N, H, seed, static=False):
    """C contacts among N points with H handles, float64 values that are float32 numbers: d_hat in [0.6, 0.95], |vt| in the regime
    c % 3; every 7th contact inactive (d_hat 1.2 or 0.3); with `static`, side b of every 4th contact and side a of every 9th"""
    g = torch.Generator().manual_seed(seed)
    rand = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64)
    ia, ib = torch.randint(0, N, (C,), generator=g), torch.randint(0, N, (C,), generator=g)
    if static:
        ib[::4], ia[1::9] = -1, -1
    c = torch.arange(C)
    nor = torch.nn.functional.normalize(rand(C, 3) - 0.5, dim=1).float().double()
    tangent = torch.nn.functional.normalize(torch.linalg.cross(nor, rand(C, 3) - 0.5), dim=1)
    d_hat = 0.6 + 0.35 * rand(C)
    d_hat = torch.where(c % 7 == 3, torch.where(c % 2 == 0, 1.2, 0.3).double(), d_hat)
    lo, hi = torch.tensor(VT_RANGES, dtype=torch.float64)[c % 3].T
    rc = torch.where(ib < 0, 1.0, 2.0).double() * RADIUS
    offset = (d_hat * rc)[:, None] * nor + ((lo + (hi - lo) * rand(C)) * MU_DT)[:, None] * tangent
    dx0, dx = (0.02 * (rand(N, 3) - 0.5)).float().double(), (0.02 * (rand(N, 3) - 0.5)).float().double()
    delta = dx - dx0
    zero = torch.zeros(1, 3, dtype=torch.float64)
    gaps = offset - torch.where((ia >= 0)[:, None], delta[ia], zero) + torch.where((ib >= 0)[:, None], delta[ib], zero)
    w = torch.nn.functional.softmax(2 * rand(N, H), dim=1)
    x0 = rand(N, 3) - 0.5
    return {k: (v.float().double() if v.is_floating_point() else v.int())
            for k, v in dict(dx=dx, dx0=dx0, gaps=gaps, normals=nor, ia=ia, ib=ib, w=w, x0=x0).items()}


def collision_of(d, dtype, device):
    """A Collision holding the contacts of `synthetic`, and (dx, w, x0), as `dtype` on `device`"""
    to = lambda t: t.to(device=device, dtype=dtype if t.is_floating_point() else None)
    col = collisions.Collision(**PARAMS)
    col.cp_dx_at_nm_iteration_0, col.collision_kinematic_gaps, col.collision_normals = to(d['dx0']), to(d['gaps']), to(d['normals'])
    col.collision_indices_a, col.collision_indices_b, col.num_contacts = to(d['ia']), to(d['ib']), len(d['ia'])
    return col, to(d['dx']), to(d['w']), to(d['x0'])


def terms64(d):
    """(gradient (C, 3), hessian (C, 3, 3)) of energy64 by autograd, after asserting the regime margins on the float64 side"""
    offset = collisions._contact_offsets(d['dx'], d['dx0'], d['gaps'], d['ia'], d['ib']).requires_grad_()
    rc = torch.where(d['ib'] < 0, 1.0, 2.0).double() * RADIUS
    dn = (offset * d['normals']).sum(-1)
    vtn = ((offset - dn[:, None] * d['normals']) / MU_DT).norm(dim=-1).detach()
    d_hat = (dn / rc).detach()
    assert ((vtn < 1e-6) | ((vtn > 5e-3) & (vtn < 0.9)) | (vtn > 1.1)).all() and ((d_hat - 0.5).abs() > 0.05).all() and ((d_hat - 1).abs() > 0.04).all()
    assert (vtn < 1e-6).any() and ((vtn > 5e-3) & (vtn < 0.9)).any() and (vtn > 1.1).any() and (d_hat > 1).any() and (d_hat < 0.5).any()
    G, = torch.autograd.grad(energy64(offset, d['normals'], rc).sum(), offset, create_graph=True)
    Hs = torch.stack([torch.autograd.grad(G[:, i].sum(), offset, retain_graph=True)[0] for i in range(3)], dim=1)
    return G.detach(), Hs


def check(name, got, definition, ref, factor=4):
    """tests/test_physics_gpu.py's measure and yardstick: e = max|X - X64| / max|X64|, e_got <= 4 max(e_def, 2^-24), e_def < 1e-4"""
    e_got, e_def = ((x.double().cpu() - ref.cpu()).abs().max().item() / ref.abs().max().item() for x in (got, definition))
    print(f'{name}: e_hip {e_got:.3e} e_def {e_def:.3e}')
    assert torch.isfinite(got).all() and e_def < 1e-4 and e_got <= factor * max(e_def, 2.0 ** -24), (name, e_got, e_def)


# ---- the reduction alone: a bound per element of g and K ----------------------------------------------------------------------------------
EPS32 = float(np.finfo(f32).eps)


def reduced_sums(G, Hs, w, x0, ia, ib):
    """In float64, from the contacts' terms as given (G (C, 3), Hs (C, 3, 3)) and m_c[4 h + n] = w[a][h] xt_a[n] - w[b][h] xt_b[n]:
    g_ref = sum_c G_c[b] m_c and K_ref = sum_c Hs_c[b][b'] m_c[i] m_c[j] in the layout of reduced_terms, and T_g, T_K, the same sums
    on absolute values with |m| replaced by |w_a xt_a| + |w_b xt_b|"""
    G, Hs, w, x0 = (t.detach().double().cpu() for t in (G, Hs, w, x0))
    C, H = G.shape[0], w.shape[1]
    xt = torch.cat([x0, torch.ones_like(x0[:, :1])], dim=1)

    def side(i):
        i = i.cpu().long()
        return (w[i.clamp(min=0)][:, :, None] * xt[i.clamp(min=0)][:, None, :] * (i >= 0)[:, None, None]).reshape(C, 4 * H)
    ma, mb = side(ia), side(ib)
    out = []
    for m, G_, H_ in ((ma - mb, G, Hs), (ma.abs() + mb.abs(), G.abs(), Hs.abs())):
        g = (G_.T @ m).reshape(3, H, 4).permute(1, 0, 2).reshape(12 * H)
        K = (H_.reshape(C, 9, 1) * m[:, None, :]).permute(1, 2, 0) @ m                                   # (9, W, W)
        out += [g, K.reshape(3, 3, H, 4, H, 4).permute(2, 0, 3, 4, 1, 5).reshape(12 * H, 12 * H)]
    return out[0], out[1], out[2], out[3]


def bound_share(got, ref, T, per, slices):
    """max over the elements of |got - ref| / ((per + slices + 8) eps32 T): at most 1 within the bound.  One slice is a sum of `per`
    products, each with at most 7 roundings (two products and a subtraction per m, the scaling by H_c), and the finishing kernel
    adds `slices` partials in order.  Where T == 0 the element must be 0"""
    err, bound = (got.detach().double().cpu() - ref).abs(), (per + slices + 8) * EPS32 * T
    share = torch.where(bound > 0, err / bound, torch.where(err > 0, float('inf'), 0.0).double())
    return share.max().item()


def check_reduced_elementwise(name, g, K, G, Hs, w, x0, ia, ib, per, slices):
    """g (12 H) and K (12 H, 12 H) or None against reduced_sums of the HIP terms G, Hs, per element"""
    g_ref, K_ref, T_g, T_K = reduced_sums(G, Hs, w, x0, ia, ib)
    shares = {'g': bound_share(g, g_ref, T_g, per, slices)}
    if K is not None:
        shares['K'] = bound_share(K, K_ref, T_K, per, slices)
    print(f'{name}: per {per} slices {slices}, largest share of the element-wise bound ' + ' '.join(f'{k} {v:.3f}' for k, v in shares.items()))
    assert all(v <= 1 for v in shares.values()), (name, shares)


# ---- the ends of the active interval and of the stick regime ------------------------------------------------------------------------------
# exact in float32 and float64 alike: rc = 0.25 or 0.125, rp = 0.5, dt = nu = 1 / 8 for the kernels
EDGE_PARAMS = dict(dt=1.0, collision_particle_radius=0.125, impenetrable_barrier_ratio=0.5, friction_regularization=0.125,
                   friction_fluid=0.125, friction=0.5)
EDGE_CONSTANTS = (0.125, 0.5, 0.5, 0.125, 0.015625)        # Collision(**EDGE_PARAMS)._params()


def regime_edges():
    """60 contacts between two points at rest, offset = d n + t e: (n, e, side b static) = (x, y, no), (-z, x, no), (y, z, yes);
    d / rc in {1, 1 + ulp, 1 - ulp, 0.5, 0.5 + ulp}; t / 0.125 in {0, 1 - ulp, 1, 1 + ulp}.  -> (the tensors of `synthetic`, float64
    values that are float32 numbers; d_hat (C); vtn (C)), after asserting that float32 and float64 take the same side of every
    comparison of the terms for every contact, and that every comparison goes both ways"""
    up, down = (lambda v: np.nextafter(f32(v), f32(4))), (lambda v: np.nextafter(f32(v), f32(0)))
    rows = [(n, e, static, d_hat, vtn)
            for n, e, static in (((1, 0, 0), (0, 1, 0), False), ((0, 0, -1), (1, 0, 0), False), ((0, 1, 0), (0, 0, 1), True))
            for d_hat in (f32(1), up(1), down(1), f32(0.5), up(0.5)) for vtn in (f32(0), down(1), f32(1), up(1))]
    nor = np.array([r[0] for r in rows], f32)
    tan = np.array([r[1] for r in rows], f32)
    static = np.array([r[2] for r in rows])
    rc = np.where(static, f32(0.125), f32(0.25)).astype(f32)
    offset = (np.array([r[3] for r in rows], f32) * rc)[:, None] * nor + (np.array([r[4] for r in rows], f32) * f32(0.125))[:, None] * tan
    sides = []
    for t in (np.float32, np.float64):
        off, n = offset.astype(t), nor.astype(t)
        d = _dot(off, n)
        d_hat = d / rc.astype(t)
        vt = (off - d[:, None] * n) / t(0.125)
        vtn = np.sqrt(_dot(vt, vt))
        sides.append(np.stack([t(0.5) < d_hat, d_hat <= t(1), vtn < t(1), vtn < t(1.0e-4), vtn > t(1.0e-4), vtn > t(0)]))
        assert np.array_equal(d_hat, np.array([r[3] for r in rows], t)) and np.array_equal(vtn, np.array([r[4] for r in rows], t))
    assert np.array_equal(*sides) and sides[0].any(axis=1).all() and not sides[0].all(axis=1).any()
    C = len(rows)
    d = dict(dx=torch.zeros(2, 3), dx0=torch.zeros(2, 3), gaps=torch.from_numpy(offset), normals=torch.from_numpy(nor),
             ia=torch.zeros(C, dtype=torch.int32), ib=torch.from_numpy(np.where(static, -1, 1).astype(np.int32)))
    return {k: v.double() if v.is_floating_point() else v for k, v in d.items()}, torch.from_numpy(d_hat), torch.from_numpy(vtn)


def edge_collision(d, dtype, device, rows=slice(None)):
    """A Collision(**EDGE_PARAMS) holding the contacts `rows` of regime_edges, and dx"""
    to = lambda t: t.to(device=device, dtype=dtype if t.is_floating_point() else None)
    col = collisions.Collision(**EDGE_PARAMS)
    col.cp_dx_at_nm_iteration_0, col.collision_kinematic_gaps, col.collision_normals = to(d['dx0']), to(d['gaps'][rows]), to(d['normals'][rows])
    col.collision_indices_a, col.collision_indices_b = to(d['ia'][rows]), to(d['ib'][rows])
    col.num_contacts = len(col.collision_indices_a)
    return col, to(d['dx'])


def edge_terms(d, dtype):
    """(E (C), G (C, 3), Hs (C, 3, 3)) of the torch formulation on the CPU, per contact"""
    return collisions._contact_terms(d['gaps'].to(dtype), d['normals'].to(dtype), d['ib'] < 0, COEFF, *EDGE_CONSTANTS, gradient=True, hessian=True)


def check_regime_edges(name, got, d, d_hat, vtn):
    """`got` = (E (C), G (C, 3), Hs (C, 3, 3)) in float32 against edge_terms in float64, per contact: e_c = max|X_c - X64_c| /
    max|X64_c| with e_got <= 4 max(e_def, 2^-24) and e_def < 1e-4, e_def from the CPU float32 formulation; where X64_c is all zero,
    exact zeros.  And what the ends themselves require"""
    got = [t.detach().cpu() for t in got]
    E, G, Hs = got
    assert all(torch.isfinite(t).all() for t in got)                              # no NaN or inf at either end, active or not
    worst = {}
    for label, x, x32, x64 in zip('EGH', got, edge_terms(d, torch.float32), edge_terms(d, torch.float64)):
        C = len(x)
        top = x64.reshape(C, -1).abs().amax(dim=1)
        zero = top == 0
        assert (x[zero] == 0).all() and (x32[zero] == 0).all(), (name, label)
        e_got, e_def = (((y.double() - x64).reshape(C, -1).abs().amax(dim=1) / top)[~zero] for y in (x, x32))
        worst[label] = (e_got.max().item(), e_def.max().item(), (e_got / e_def.clamp(min=2.0 ** -24)).max().item())
        print(f'{name} {label}: over {int((~zero).sum())} contacts, largest e_got {worst[label][0]:.3e} e_def {worst[label][1]:.3e} '
              f'e_got / max(e_def, 2^-24) {worst[label][2]:.3f}')
    outside = (d_hat > 1) | (d_hat == 0.5)
    assert outside.sum() == 24 and (E[outside] == 0).all() and (G[outside] == 0).all() and (Hs[outside] == 0).all()
    at_one = d_hat == 1                                                           # active: E is 0, the Hessian is not
    assert at_one.sum() == 12 and (E[at_one] == 0).all() and (Hs[at_one] != 0).any(dim=2).any(dim=1).all()
    assert (Hs[~outside] != 0).any(dim=2).any(dim=1).all()
    rest = (vtn == 0) & ~outside                                                  # no tangential part: G along n, Hs diagonal in these frames
    along = d['normals'].abs() == 1
    assert rest.sum() == 9 and (G[rest][~along[rest]] == 0).all() and (Hs[rest][~torch.eye(3, dtype=torch.bool).expand(9, 3, 3)] == 0).all()
    assert all(e_def < 1e-4 and ratio <= 4 for _, e_def, ratio in worst.values()), (name, worst)
