"""Quaternions in the **xyzw** layout (API mirror of the three functions of ``kaolin.math.quat`` that
``ops.gaussians.transforms`` uses).  Plain torch: any device, any floating dtype, differentiable."""
import torch

__all__ = ['quat_unit', 'quat_mul', 'quat_from_rot33']


def quat_unit(quat):
    """Normalize quaternions to norm 1.

    Args:
        quat (torch.Tensor): quaternions, of shape :math:`(\\ldots, 4)`.

    Returns:
        (torch.Tensor): ``quat / max(|quat|, 1e-12)``, of the same shape.
    """
    return quat / torch.linalg.norm(quat, dim=-1, keepdim=True).clamp_min(1e-12)


def quat_mul(a, b):
    """The Hamilton product :math:`a \\otimes b` of quaternions in xyzw layout (the rotation ``b`` followed by ``a``).

    Args:
        a (torch.Tensor): of shape :math:`(\\ldots, 4)`.
        b (torch.Tensor): of a shape that broadcasts against ``a``.

    Returns:
        (torch.Tensor): the products, of the broadcast shape.
    """
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    x = aw * bx + ax * bw + ay * bz - az * by
    y = aw * by + ay * bw + az * bx - ax * bz
    z = aw * bz + az * bw + ax * by - ay * bx
    w = aw * bw - ax * bx - ay * by - az * bz
    return torch.stack([x, y, z, w], dim=-1)


def quat_from_rot33(mat):
    """Rotation matrices to quaternions in xyzw layout, by the branch on the largest of the trace and the diagonal: the trace
    when it is > 0; else ``m00`` when it is > ``m11`` and > ``m22``; else ``m11`` when it is > ``m22``; else ``m22``.  The
    component the branch names is the positive one (the other three take their signs from the off-diagonal differences and
    sums), so the result is continuous inside a branch and may flip its overall sign across two of them.

    Args:
        mat (torch.Tensor): rotation matrices, of shape :math:`(\\ldots, 3, 3)`.

    Returns:
        (torch.Tensor): quaternions, of shape :math:`(\\ldots, 4)`.
    """
    assert mat.shape[-1] == 3
    assert mat.shape[-2] == 3
    m00, m01, m02 = mat[..., 0, 0], mat[..., 0, 1], mat[..., 0, 2]
    m10, m11, m12 = mat[..., 1, 0], mat[..., 1, 1], mat[..., 1, 2]
    m20, m21, m22 = mat[..., 2, 0], mat[..., 2, 1], mat[..., 2, 2]
    trace = m00 + m11 + m22

    use_trace = trace > 0
    use_x = ~use_trace & (m00 > m11) & (m00 > m22)
    use_y = ~use_trace & ~use_x & (m11 > m22)
    use_z = ~use_trace & ~use_x & ~use_y

    def root(selected, arg):
        # the square root of a branch that is not selected sees 1, so that no NaN of it reaches a gradient
        return torch.sqrt(torch.where(selected, arg, torch.ones_like(arg)))

    def branch(selected, lead, plus, minus1, minus2, sums, diff):
        # s = 4 |component `lead`|; the other two vector components from the symmetric sums, w from the difference
        s = 2.0 * root(selected, 1.0 + plus - minus1 - minus2)
        parts = [None, None, None, diff / s]
        parts[lead] = 0.25 * s
        for k, v in sums.items():
            parts[k] = v / s
        return torch.stack(parts, dim=-1)

    s0 = 0.5 / root(use_trace, trace + 1.0)
    by_trace = torch.stack([(m21 - m12) * s0, (m02 - m20) * s0, (m10 - m01) * s0, 0.25 / s0], dim=-1)
    by_x = branch(use_x, 0, m00, m11, m22, {1: m01 + m10, 2: m02 + m20}, m21 - m12)
    by_y = branch(use_y, 1, m11, m00, m22, {0: m01 + m10, 2: m12 + m21}, m02 - m20)
    by_z = branch(use_z, 2, m22, m00, m11, {0: m02 + m20, 1: m12 + m21}, m10 - m01)
    out = torch.where(use_y.unsqueeze(-1), by_y, by_z)
    out = torch.where(use_x.unsqueeze(-1), by_x, out)
    return torch.where(use_trace.unsqueeze(-1), by_trace, out)
