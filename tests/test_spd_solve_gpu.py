"""kaolin_amd.physics.optimization on the GPU (csrc/spd_solve.hip, float32) against float64 torch on the same float32 values.

The yardstick is that of test_scene_forces_gpu.py: e = max|X - X64| / max|X64|, e_hip <= 4 max(e_def, u), u = 2^-24, and
e_def < 1e-4, with e_def the same measure for float32 LAPACK on the CPU (torch.linalg.cholesky, torch.cholesky_solve: not the code
under test).  Inputs: A = M M^T / (2 n) + 0.1 I, M ~ N(0, 1) of (n, 2 n) drawn in float64 from a generator seeded with n, rounded
to float32 and mirrored from its lower triangle (condition number 10 to 17), b ~ N(0, 1).  Every figure is printed before it is
asserted (pytest -s)."""
import functools

import pytest
import torch

from kaolin_amd import _C
from kaolin_amd.physics import Floor, Gravity, cholesky_spd, lbs_matrix, newtons_method, optimization, reduced_scene_terms, solve_spd
from kaolin_amd.physics.simplicits import reduced_neohookean_terms
from test_physics_cpu import make_inputs

pytestmark = pytest.mark.gpu

NB = _C.physics.spd_panel()
U = 2.0 ** -24


@functools.lru_cache(maxsize=None)
def system(n):
    """(A, b in float64 of float32 values, x in float64, LAPACK's float32 L and x, the HIP L, x and the two infos)"""
    gen = torch.Generator().manual_seed(n)
    M = torch.randn(n, 2 * n, generator=gen, dtype=torch.float64)
    A = (M @ M.T / (2 * n) + 0.1 * torch.eye(n, dtype=torch.float64)).float().double().tril()
    A = A + A.tril(-1).T
    b = torch.randn(n, generator=gen, dtype=torch.float64).float().double()
    L_def = torch.linalg.cholesky(A.float())
    x_def = torch.cholesky_solve(b.float()[:, None], L_def)[:, 0]
    L, info_L = cholesky_spd(A.float().cuda())
    x, info_x = solve_spd(A.float().cuda(), b.float().cuda())
    return A, b, torch.linalg.solve(A, b), L_def, x_def, L, x, info_L, info_x


def check(name, hip, definition, ref):
    e_hip, e_def = ((x.double().cpu() - ref).abs().max().item() / ref.abs().max().item() for x in (hip, definition))
    print(f'{name}: e_hip {e_hip:.3e} e_def {e_def:.3e} ratio {e_hip / max(e_def, U):.2f}')
    assert torch.isfinite(hip).all() and e_def < 1e-4 and e_hip <= 4 * max(e_def, U), (name, e_hip, e_def)


@pytest.mark.parametrize('n', [1, 12, NB - 1, NB, NB + 1, 2 * NB + 1, 384, 1536])
def test_factor_and_solve(n):
    A, b, x64, L_def, x_def, L, x, info_L, info_x = system(n)
    assert L.shape == (n, n) and x.shape == (n,) and info_L.shape == info_x.shape == (1,) and info_L.dtype == torch.int32
    assert info_L.item() == 0 and info_x.item() == 0 and not L.triu(1).any()
    check(f'x n={n}', x, x_def, x64)
    check(f'L L^T n={n}', L.double() @ L.double().T, L_def.double() @ L_def.double().T, A)


def test_upper_triangle_is_not_read_and_repeats():
    n = 2 * NB + 1
    A, b, _, _, _, L, x, _, _ = system(n)
    lower = A.float().masked_fill(torch.ones(n, n).triu(1).bool(), float('nan')).cuda()
    for matrix in (lower, A.float().cuda()):   # NaN above the diagonal; the same call again
        x2, info = solve_spd(matrix, b.float().cuda())
        assert info.item() == 0 and torch.equal(x2, x) and torch.equal(cholesky_spd(matrix)[0], L)


@pytest.mark.parametrize('j', [0, NB - 1, NB, 2 * NB + 1])
def test_failure_index(j):
    A = torch.eye(2 * NB + 2)
    A[j, j] = -1
    expected = torch.linalg.cholesky_ex(A)[1].item()
    x, info = solve_spd(A.cuda(), torch.ones(2 * NB + 2).cuda())
    torch.cuda.synchronize()
    assert expected == j + 1 and info.item() == cholesky_spd(A.cuda())[1].item() == j + 1


def newton_objective(dtype, device):
    """N = 200 points, H = 4 handles: Neo-Hookean + gravity + floor + inertia, dt = 0.05 -> (z, energy, gradient, Hessian, the
    points' distance from the floor at z)"""
    N, H, dt = 200, 4, 0.05
    gen = torch.Generator().manual_seed(1)
    rand = lambda *shape: torch.rand(*shape, generator=gen, dtype=torch.float64)
    d = make_inputs(N, H, seed=5)
    d.update(rho=900 + 200 * rand(N), z_prev=d['z'] - 0.02 * rand(H, 3, 4), z_dot=0.1 * (rand(H, 3, 4) - 0.5), mu=1e4 * d['mu'], lam=1e4 * d['lam'])
    d = {k: v.float().to(dtype=dtype, device=device) for k, v in d.items()}
    forces = [(Gravity((0.0, 9.8, 0.0), d['rho'], d['vol']), 1.0), (Floor(-0.5, 1, False, d['vol']), 1e5)]
    inertia = ((d['rho'].double() * d['vol'].double()).float().to(dtype), d['z_prev'], d['z_dot'], dt)

    def terms(z, hessian):
        a = reduced_neohookean_terms(z, d['pts'], d['weights'], d['weights_jac'], d['mu'], d['lam'], d['vol'], coeff=dt * dt, hessian=hessian)
        b = reduced_scene_terms(z, d['pts'], d['weights'], forces, inertia=inertia, pe_scale=dt * dt, hessian=hessian)
        return [p + q for p, q in zip(a[:3 if hessian else 2], b)]
    z = d['z'].reshape(-1)
    margin = ((d['pts'].reshape(-1) + lbs_matrix(d['weights'], d['pts']) @ z).reshape(N, 3)[:, 1] + 0.5).abs().min().item()
    return z, (lambda z: terms(z, False)[0]), (lambda z: terms(z, False)[1]), (lambda z: terms(z, True)[2]), margin


def test_newton_step(monkeypatch):
    """One step of newtons_method, float32 on the GPU, against the same driver in float64 on the dense CPU definitions; e_def: the
    float32 GPU run with torch.linalg.solve in place of the HIP solve.  Asserted on the float64 run: no point within 1e-3 of the
    floor (the Hessian jumps there), and the Armijo test, which the driver evaluates twice on the full step (the enlarged step is
    clamped by the bounds of 1), accepts with a slack of at least |g . dx| / 2, so no rounding decides the line search."""
    z, E, g, K, margin = newton_objective(torch.float64, 'cpu')
    dx = -torch.linalg.solve(K(z), g(z))
    descent = -(g(z) @ dx).item()
    slack = (E(z) + 1e-3 * (g(z) @ dx) - E(z + dx)).item()
    ref = newtons_method(z, E, g, K, nm_max_iters=1)
    print(f'floor margin {margin:.3e} |g.dx| {descent:.3e} slack {slack:.3e} = {slack / descent:.4f} |g.dx|')
    assert margin >= 1e-3 and descent > 0 and slack >= 0.5 * descent and (ref - (z + dx)).abs().max() <= 1e-9
    args = newton_objective(torch.float32, 'cuda')[:4]
    hip = newtons_method(*args, nm_max_iters=1)
    monkeypatch.setattr(optimization, 'solve_spd', lambda A, b: (torch.linalg.solve(A, b), torch.zeros(1, dtype=torch.int32, device=A.device)))
    check('newton z', hip, newtons_method(*args, nm_max_iters=1), ref)
