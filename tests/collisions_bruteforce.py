"""The oracle of kaolin_amd.physics.collisions: the detection contract over all pairs in numpy float32 (one rounding per
operation), the contact energy of the reference's test in float64 with its derivatives by autograd, and the inputs that
tests/test_collisions_cpu.py and tests/test_collisions_gpu.py share."""
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
    e, r = pos[:, None] - pos[None], x0[:, None] - x0[None]
    with np.errstate(invalid='ignore', over='ignore'):
        mask = (np.sqrt(_dot(e, e)) <= R) & (np.arange(n)[None] > np.arange(n)[:, None])
        mask &= ~((static[:, None] == 1) & (static[None] == 1)) & ~((obj[:, None] == obj[None]) & (_dot(r, r) < immune))
    a, b = np.nonzero(mask)                      # row-major: sorted by (a, b)
    total, a, b = len(a), a[:max_pairs], b[:max_pairs]
    e = pos[a] - pos[b]
    d = np.sqrt(_dot(e, e))[:, None]
    with np.errstate(invalid='ignore', divide='ignore'):
        normals = np.where(d == 0, f32(0), e / d).astype(f32)
    gaps = _dot(e, normals)[:, None] * normals
    return total, np.where(static[a] == 1, -1, a).astype(np.int32), np.where(static[b] == 1, -1, b).astype(np.int32), normals, gaps


def detection_case(name):
    """-> (dx, x0, obj, static, constructor arguments)"""
    rng = np.random.default_rng(sum(map(ord, name)))
    kw = dict(collision_particle_radius=0.05)                                  # R = 0.15, cell edge 0.152
    if name[1:].isdigit():                                                     # negative coordinates, points on either side of cell faces
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
    dx = rng.uniform(-0.01, 0.01, (n, 3)) * (name != 'exact')
    if name == 'duplicates':
        dx[7] = dx[8] = dx[21]
    obj, static = (np.arange(n) % 2).astype(np.int32), np.zeros(n, np.int32)
    if name == 'static':
        obj = np.concatenate([np.repeat([0, 1], 20), [2, 3]]).astype(np.int32)
        dx[20:40, 1] += 0.5
        static[:20], static[40:] = 1, 1
    return dx.astype(f32), x0.astype(f32), obj, static, kw


DETECTION_CASES = ['n1', 'n63', 'n64', 'n65', 'n257', 'one_cell', 'exact', 'duplicates', 'nan', 'immune', 'static', 'none']


def check_detection(name, device, caplog, max_pairs=10000):
    """detect_collisions on `device` against the oracle: torch.equal on all four tensors, twice"""
    dx, x0, obj, static, kw = detection_case(name)
    total, *expected = detect(dx, x0, obj, static, kw['collision_particle_radius'], 1.5, kw.get('ignore_self_collision_ratio', 100000.0),
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
