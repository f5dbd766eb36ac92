"""kaolin_amd.physics.optimization, the driver's logic in float64 on the CPU (no kernel): newtons_method against a plain Newton loop
written here, on E(x) = 1/2 x^T A x - b^T x + 1/4 sum x^4 with A symmetric positive definite, n = 12; and solve_spd's torch path."""
import pytest
import torch

from kaolin_amd.physics import cholesky_spd, newtons_method, solve_spd

N = 12
GEN = torch.Generator().manual_seed(N)
M = torch.randn(N, 2 * N, generator=GEN, dtype=torch.float64)
A = M @ M.T / (2 * N) + 0.1 * torch.eye(N, dtype=torch.float64)
B = 0.1 * torch.randn(N, generator=GEN, dtype=torch.float64)   # small: the quartic bends every step, none overshoots
X0 = 0.1 * torch.randn(N, generator=GEN, dtype=torch.float64)
FCNS = (lambda x: 0.5 * x @ A @ x - B @ x + 0.25 * (x ** 4).sum(), lambda x: A @ x - B + x ** 3, lambda x: A + torch.diag(3 * x ** 2))


def test_newtons_method_against_a_plain_loop():
    E, g, K = FCNS
    x, steps = X0.clone(), 0
    while (torch.linalg.solve(K(x), g(x)) @ g(x)).abs() >= 1e-4:
        dx = -torch.linalg.solve(K(x), g(x))
        assert E(x + dx) <= E(x) + 1e-3 * (g(x) @ dx)   # the line search accepts every full step of this start
        x, steps = x + dx, steps + 1
    assert 1 <= steps < 10
    out = newtons_method(X0, E, g, K, nm_max_iters=10, conv_tol=1e-4)
    dx = -torch.linalg.solve(K(out), g(out))
    print(f'steps {steps} |dx.g| {(dx @ g(out)).abs().item():.3e} difference {(out - x).abs().max().item():.3e}')
    assert (dx @ g(out)).abs() < 1e-4 and (out - x).abs().max() <= 1e-9
    assert torch.equal(newtons_method(X0, E, g, K, nm_max_iters=steps - 1), newtons_method(X0, E, g, K, nm_max_iters=steps - 1,
                                                                                            bounds_fcn=lambda dx, x: None))


def test_bounds_and_unbuilt_arguments():
    E, g, K = FCNS
    full = newtons_method(X0, E, g, K, nm_max_iters=1) - X0
    half = newtons_method(X0, E, g, K, nm_max_iters=1, bounds_fcn=lambda dx, x: torch.full_like(x, 0.5)) - X0
    assert full.abs().max() > 0 and (half - 0.5 * full).abs().max() <= 1e-12 * full.abs().max()
    with pytest.raises(NotImplementedError):
        newtons_method(X0, E, g, K, direct_solve=False)


def test_solve_spd_on_cpu_is_the_torch_definition():
    L, info = torch.linalg.cholesky_ex(A)
    x, info_x = solve_spd(A, B)
    assert torch.equal(x, torch.cholesky_solve(B[:, None], L)[:, 0]) and torch.equal(cholesky_spd(A)[0], L)
    assert info_x.shape == (1,) and info_x.dtype == torch.int32 and info_x.item() == info.item() == 0
    nb = 64
    for j in (0, nb - 1, nb, 2 * nb + 1):
        bad = torch.eye(2 * nb + 2, dtype=torch.float64)
        bad[j, j] = -1
        assert solve_spd(bad, bad[0])[1].item() == cholesky_spd(bad)[1].item() == j + 1
