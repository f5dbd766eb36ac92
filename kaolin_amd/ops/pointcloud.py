"""Point-cloud operators behind the API of kaolin/ops/pointcloud.py.

``farthest_point_sampling`` is the one with kernels (kaolin_amd/csrc/fps.hip): the reference runs NVIDIA Warp kernels, which
have no route on an AMD GPU, and its result depends on the outcome of a race.  Here the result is fixed by one rule, stated in
the function's docstring; a GPU tensor runs it in HIP, a CPU tensor as a short torch loop.  ``center_points`` is the
reference's torch expression and runs on either device.
"""
import torch

from .. import _C

__all__ = ['center_points', 'farthest_point_sampling']


def center_points(points, normalize=False, eps=1e-6):
    r"""Moves every point cloud so that the middle of its bounding box is at the origin; each cloud of the batch on its own.

    Args:
        points (torch.Tensor): of shape :math:`(\text{batch_size}, \text{num_points}, C)`, usually :math:`C = 3`.
        normalize (bool): also divide each cloud by the longest side of its bounding box, so that it fits :math:`[-0.5, 0.5]`.
        eps (float): lower clip of that side (a cloud of identical points is divided by ``eps``, not by zero).

    Returns:
        (torch.Tensor): of the shape, dtype and device of ``points``.
    """
    assert len(points.shape) == 3, f'Points have unexpected shape {points.shape}'
    vmin = points.min(dim=1, keepdim=True)[0]
    vmax = points.max(dim=1, keepdim=True)[0]
    res = points - (vmin + vmax) / 2
    if normalize:
        res = res / (vmax - vmin).max(dim=-1, keepdim=True)[0].clip(min=eps)
    return res


def _torch_farthest_point_sampling(points, k):
    """The definition, cloud by cloud: every operation of the distance is a float32 tensor operation of its own (nothing fused)."""
    out = torch.empty((points.shape[0], k), dtype=torch.int64, device=points.device)

    def sq_dist(p, q):
        sq = (p - q) * (p - q)
        return (sq[:, 0] + sq[:, 1]) + sq[:, 2]

    for b, p in enumerate(points):
        finite = torch.isfinite(p).all(dim=1)
        centre = (p[finite].double().sum(dim=0) / finite.sum()).float()
        if not torch.isfinite(centre).all():
            centre = torch.zeros_like(centre)
        d = sq_dist(p, centre)
        D = torch.where(torch.isfinite(d), d, -1.0)
        for r in range(k):
            s = int(torch.nonzero(D == D.max())[0])     # the lowest index among the largest
            out[b, r] = s
            d = sq_dist(p, p[s])
            if r == 0:
                D = torch.where(torch.isfinite(d), d, -1.0)
            else:
                D = torch.where(torch.isfinite(d), torch.minimum(D, d), D)
            D[s] = -2.0
    return out


def farthest_point_sampling(points, k):
    r"""Picks :math:`k` well-spread points out of each cloud: first the point farthest from the center, then, again and again,
    the point farthest from everything picked so far.

    The result is fixed by this rule, with :math:`d(a, b) = (dx \cdot dx + dy \cdot dy) + dz \cdot dz` and every operation
    rounded to float32:

    1. the center is the mean of the points whose three coordinates are finite, summed in float64 and rounded to float32
       (the origin when there is no such point);
    2. the first point has the largest :math:`D_i = d(p_i, center)`, where a :math:`d` that is not finite counts as -1;
    3. then :math:`D_i = d(p_i, p_{first})` (-1 where not finite), and each further point is the arg-max of :math:`D`, after
       which :math:`D_i = \min(D_i, d(p_i, p_s))` wherever that :math:`d` is finite.  A taken point has :math:`D = -2`.

    Ties go to the lowest index.  So the function always returns :math:`k` distinct indices, takes a point with an `inf` or
    `NaN` coordinate only after every finite point (such points in ascending index order) and duplicates of taken points
    after everything at a positive distance; the same input gives the same indices on every call, on the CPU and on the GPU.

    On a GPU tensor the rule runs in HIP kernels and the call neither reads back nor synchronises (it can be captured in a
    graph); the reference needs NVIDIA Warp, returns its result on the host, and accepts no CPU tensor.

    Args:
        points (torch.FloatTensor): of shape :math:`(\text{batch_size}, \text{num_points}, 3)`, float32.
        k (int): how many points to pick per cloud, :math:`0 \le k \le \text{num_points}`.

    Returns:
        (torch.LongTensor): of shape :math:`(\text{batch_size}, k)`, the picked indices in picking order, on the device of
        ``points``.
    """
    assert len(points.shape) == 3, f'Points have unexpected shape {points.shape}'
    assert points.dtype == torch.float32, f'Points should have dtype float32. dtype is {points.dtype}'
    assert 0 <= k <= points.shape[1], f'k must satisfy 0 <= k <= num_points, but got k={k} and num_points={points.shape[1]}'
    points = points.detach()
    if points.is_cuda:
        return _C.ops.farthest_point_sampling_cuda(points, k)
    return _torch_farthest_point_sampling(points, k)
