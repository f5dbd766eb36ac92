"""Newton's method on the reduced (Simplicits) objective, behind the name of kaolin/physics/common/optimization.py, and its linear
solve: a Cholesky factorisation and two substitutions in HIP on a GPU (kaolin_amd/csrc/spd_solve.hip).

The reference's ``newtons_method`` takes NVIDIA Warp arrays and sparse matrices and, with ``direct_solve=True`` (what
``SimplicitsScene.run_sim_step`` asks for), makes the Hessian dense and calls ``torch.linalg.solve``, a pivoted LU.  Here the
callables take and return torch tensors, as :func:`~kaolin_amd.physics.simplicits.reduced_neohookean_terms`,
:func:`~kaolin_amd.physics.scene_forces.reduced_scene_terms` and :meth:`~kaolin_amd.physics.collisions.Collision.reduced_terms`
return them, and the solve uses that the Hessian is symmetric positive definite."""
import torch

from .. import _C

__all__ = ['cholesky_spd', 'solve_spd', 'newtons_method']


def _check_system(A, b=None):
    if not isinstance(A, torch.Tensor) or A.dtype not in (torch.float32, torch.float64) or A.dim() != 2 or \
            A.shape[0] != A.shape[1] or A.shape[0] < 1:
        raise ValueError('A must be a float32 or float64 tensor of shape (n, n), n >= 1')
    if b is not None and (not isinstance(b, torch.Tensor) or tuple(b.shape) != (A.shape[0],) or b.dtype != A.dtype or
                          b.device != A.device):
        raise ValueError(f'b must be of shape ({A.shape[0]},), of the dtype and on the device of A')
    return A.detach(), None if b is None else b.detach()


def _on_hip(A):
    return A.is_cuda and A.dtype == torch.float32 and A.shape[0] <= _C.physics.spd_max_n()


def cholesky_spd(A):
    r"""The Cholesky factor of a symmetric positive definite matrix, :math:`A = L L^T`.  Only the lower triangle of ``A`` is read.

    float32 tensors on a GPU with :math:`n \le` ``kaolin_amd._C.physics.spd_max_n()`` (1536, the reduced Hessian of 128 handles) run
    the blocked HIP factorisation: the same inputs give the same bits on every call, and nothing is read back.  Everything else
    (CPU, float64, larger :math:`n`) runs ``torch.linalg.cholesky_ex``.  No autograd.

    Args:
        A (torch.Tensor): of shape :math:`(n, n)`.

    Returns:
        (torch.Tensor, torch.Tensor): :math:`L` of shape :math:`(n, n)`, lower triangular, and ``info`` of shape :math:`(1,)`,
        int32: 0, or the 1-based index of the first column whose pivot is not positive (LAPACK's convention, that of
        ``torch.linalg.cholesky_ex``; the HIP path also counts a pivot that is not finite).  :math:`L` is then unspecified.
    """
    A, _ = _check_system(A)
    if _on_hip(A):
        L, info, _ = _C.physics.spd_factor_cuda(A.contiguous())
        return L, info
    L, info = torch.linalg.cholesky_ex(A)
    return L, info.reshape(1)


def solve_spd(A, b):
    r"""Solves :math:`A x = b` for a symmetric positive definite :math:`A` and one right-hand side by a Cholesky factorisation
    and two substitutions.  Paths and ``info`` as in :func:`cholesky_spd`; the torch path is ``torch.linalg.cholesky_ex`` and
    ``torch.cholesky_solve``.

    Args:
        A (torch.Tensor): of shape :math:`(n, n)`; only its lower triangle is read.
        b (torch.Tensor): of shape :math:`(n,)`.

    Returns:
        (torch.Tensor, torch.Tensor): :math:`x` of shape :math:`(n,)` and ``info`` of shape :math:`(1,)`; where ``info`` is not
        0, :math:`x` is unspecified.
    """
    A, b = _check_system(A, b)
    if _on_hip(A):
        L, info, workspace = _C.physics.spd_factor_cuda(A.contiguous())
        return _C.physics.spd_solve_cuda(L, b.contiguous(), info, workspace), info
    L, info = torch.linalg.cholesky_ex(A)
    return torch.cholesky_solve(b[:, None], L)[:, 0], info.reshape(1)


def _apply_bounds(direction, bounds, t):
    return direction * torch.min(bounds, torch.as_tensor(t, dtype=bounds.dtype, device=bounds.device))


def _line_search(func, x, direction, gradient, initial_step_size, bounds, alpha=1e-3, beta=0.6, max_steps=10):
    """The reference's backtracking line search, step for step: the Armijo test on the bounded direction; the first accepted step
    is enlarged once by 1 / beta and returned when the test accepts again, a rejected step shrinks by beta."""
    t = initial_step_size
    f = func(x)
    can_break = False
    bounded_direction = _apply_bounds(direction, bounds, t)
    for _ in range(max_steps):
        f_new = func(x + bounded_direction)
        if f_new <= f + alpha * (gradient @ bounded_direction):
            if can_break:
                return bounded_direction
            can_break = True
            t = t / beta
        else:
            t *= beta
        bounded_direction = _apply_bounds(direction, bounds, t)
    return bounded_direction


@torch.no_grad()
def newtons_method(x, energy_fcn, gradient_fcn, hessian_fcn, bounds_fcn=None, nm_max_iters=5, conv_tol=1e-4, direct_solve=True):
    r"""Newton's method with the reference's loop and line search: at each iteration the direction :math:`dx = -K^{-1} g`, a stop
    when :math:`|dx \cdot g| <` ``conv_tol``, the collision bounds of ``bounds_fcn`` clamped with :math:`\min(bounds, t)`, and a
    backtracking Armijo search (:math:`\alpha = 10^{-3}`, :math:`\beta = 0.6`, at most 10 steps) that enlarges its first accepted
    step once.

    Each iteration solves with :func:`solve_spd`; ``info`` and the convergence scalar come back in one host read.  An iteration
    whose factorisation fails (``info != 0``: :math:`K` is not positive definite) solves again with ``torch.linalg.solve``, which
    is what the reference calls in every iteration.

    Of the reference's arguments these are not built: ``direct_solve=False`` (conjugate gradients, with ``cg_tol``, ``cg_iters``
    and ``preconditioner_fcn``) raises ``NotImplementedError``; the projections ``P`` / ``Pt`` of kinematic degrees of freedom and
    the QR transforms of the bounds (``bounds_qr_tfm``, ``bounds_qr_tfm_inv``) are absent.

    Args:
        x (torch.Tensor): the initial guess, of shape :math:`(n,)`.
        energy_fcn (function): ``x`` -> the energy, a scalar tensor or of shape :math:`(1,)`.
        gradient_fcn (function): ``x`` -> the gradient, of shape :math:`(n,)`.
        hessian_fcn (function): ``x`` -> the Hessian, dense, of shape :math:`(n, n)`.
        bounds_fcn (function, optional): ``(dx, x)`` -> the largest step per degree of freedom, of shape :math:`(n,)`, or None
            for no bound.  Default: no bound.
        nm_max_iters (int): the most iterations. Default: 5.
        conv_tol (float): the stop on :math:`|dx \cdot g|`. Default: 1e-4.
        direct_solve (bool): only True is built. Default: True.

    Returns:
        (torch.Tensor): the optimised ``x``, of shape :math:`(n,)`.
    """
    if not direct_solve:
        raise NotImplementedError('newtons_method: only the direct solve is built (direct_solve=True), not conjugate gradients')
    for _ in range(nm_max_iters):
        g = gradient_fcn(x).reshape(-1)
        K = hessian_fcn(x)
        sol, info = solve_spd(K, g)
        dx = -sol
        failed, conv = torch.cat([info.to(g.dtype), (dx @ g).abs().reshape(1)]).tolist()
        if failed != 0:
            dx = -torch.linalg.solve(K, g)
            conv = (dx @ g).abs().item()
        if conv < conv_tol:
            break
        bounds = bounds_fcn(dx, x) if bounds_fcn is not None else None
        if bounds is None:
            bounds = torch.ones_like(x)
        x = x + _line_search(energy_fcn, x, dx, g, 1.0, bounds)
    return x
