"""kaolin.ops.conversions.gaussians (reference: kaolin/ops/conversions/gaussians.py): 3D Gaussian splats -> the voxels of an SPC level
with their accumulated opacity.  GPU tensors run csrc/gs_to_spc.hip; the torch formulation below is what CPU tensors run (the
reference has none) and the yardstick of tools/time_gs_to_spc.py on GPU tensors."""
import torch

from ... import _C
from ...render import spc as spc_render

__all__ = ['gs_to_voxelgrid']


def gs_to_voxelgrid(xyz, scales, rots, opacities, level, iso=11.345, tol=1. / 8., step=10):
    r"""Define a voxelgrid overlapping with a 3D Gaussians Splat. Opacity is integrated over multiple samples.

    .. note::
        This op is not differentiable

    Args:
        xyz (torch.FloatTensor): means of the Gaussians, of shape :math:`(\text{num_gaussians, 3})`.
        scales (torch.FloatTensor): scales, of shape :math:`(\text{num_gaussians, 3})`.
        rots (torch.FloatTensor): rotations as quaternions (r, x, y, z), used as given, of shape :math:`(\text{num_gaussians, 4})`.
        opacities (torch.FloatTensor): opacities, of shape :math:`(\text{num_gaussians})` or :math:`(\text{num_gaussians, 1})`.
        level (int): level at which to process, the resolution is :math:`2^{level}`.
        iso (float): the isocontour value that bounds a Gaussian.  Default: the 99th percentile, 11.345.
        tol (float): smallest allowed scale, relative to the size of a voxel at ``level``.  Default: 0.125.
        step (int): samples per axis of the opacity integral.

    Returns:
        (torch.ShortTensor, torch.FloatTensor):

            - the voxel coordinates, of shape :math:`(\text{num_voxels}, 3)`, in Morton order
            - the accumulated opacities, of shape :math:`(\text{num_voxels})`
    """
    xyz = xyz.detach().contiguous()
    scales = scales.detach().contiguous()
    rots = rots.detach().contiguous()
    opacities = opacities.detach().contiguous()
    points, gaus_id, pack_boundary, cov3d_invs = _C.ops.conversions.gs_to_spc_cuda(xyz, scales, rots, iso, tol, level)
    integral = _C.ops.conversions.integrate_gs_cuda(points, gaus_id, xyz, cov3d_invs, opacities, level, step)
    if points.size(0) == 0:
        return points, integral
    merged = 1. - spc_render.prod_reduce((1. - integral).unsqueeze(-1), pack_boundary).squeeze(-1)
    return points[pack_boundary], merged


# ---- the torch formulation: the reference's expressions in its operand order, one op per operation (nothing is fused), one octree
# level per round, a stable sort, the integral in float64.  The integer results and cov3d_invs carry the same bits as the HIP path.
def _voxel_size(level):
    return 2.0 / float(1 << int(level))             # a power of two: exact in float32


def _f32(value):
    return float(torch.tensor(float(value), dtype=torch.float32))


def _prepare(means, scales, rots, iso, tol, level):
    min_scale = _f32(tol) * _voxel_size(level)
    s = torch.fmax(scales, scales.new_tensor(min_scale))
    det_s = s[:, 0].double() * s[:, 1].double() * s[:, 2].double()
    r, x, y, z = rots.unbind(1)
    zero = torch.zeros_like(r)
    R = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y + r * z), 2.0 * (x * z - r * y)],
         [2.0 * (x * y - r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z + r * x)],
         [2.0 * (x * z + r * y), 2.0 * (y * z - r * x), 1.0 - 2.0 * (x * x + y * y)]]
    S = [[(1.0 / s[:, i]) if i == k else zero for k in range(3)] for i in range(3)]
    M = [[S[i][0] * R[0][j] + S[i][1] * R[1][j] + S[i][2] * R[2][j] for j in range(3)] for i in range(3)]
    Sg = [[M[0][i] * M[0][j] + M[1][i] * M[1][j] + M[2][i] * M[2][j] for j in range(3)] for i in range(3)]
    cov = torch.stack([Sg[0][0], Sg[0][1], Sg[0][2], Sg[1][1], Sg[1][2], Sg[2][2]], 1).contiguous()
    c0, c1, c2, c3, c4, c5 = cov.double().unbind(1)
    h0 = c3 * c5 - c4 * c4
    h1 = c2 * c4 - c1 * c5
    h2 = c1 * c4 - c2 * c3
    h3 = c0 * c5 - c2 * c2
    h4 = c1 * c2 - c0 * c4
    h5 = c0 * c3 - c1 * c1
    iso64 = _f32(iso)
    w = [det_s * torch.sqrt(iso64 / h0), det_s * torch.sqrt(iso64 / h3), det_s * torch.sqrt(iso64 / h5)]
    Q = [[h0, h1, h2], [h1, h3, h4], [h2, h4, h5]]
    cp = torch.stack([torch.stack([(w[i] * Q[i][k]).float() for k in range(3)], 1) for i in range(3)], 1)     # (G, 3, 3)
    big = torch.finfo(torch.float32).max
    pmin, pmax = torch.full_like(means, big), torch.full_like(means, -big)
    for i in range(3):
        for p in (cp[:, i], -1.0 * cp[:, i]):
            pmin, pmax = torch.fmin(pmin, p), torch.fmax(pmax, p)
    return cov, pmin + means, pmax + means, cp


def _edge_test(c0, c1, c2, c3, c4, c5, iso32, s, t, lo, hi):
    a = c0.double()
    b = (2.0 * (c1 * s + c2 * t)).double()
    c = (((c3 * s * s + 2.0 * c4 * s * t) + c5 * t * t) - iso32).double()
    d = b * b - 4.0 * a * c
    d = torch.fmax(d, torch.zeros_like(d))
    b2a = -0.5 * b / a
    rd = 0.5 * torch.sqrt(d) / a
    return (d > 0) & ~((hi.double() <= b2a - rd) | (b2a + rd <= lo.double()))


def _face_test(p, q, vs, i, j, k, o):
    t = ((q[:, i] - (p[:, i] + o)).double() / (2.0 * q[:, i].double())).float()
    f = 1.0 - 2.0 * t.double()
    hj, hk = (f * q[:, j].double()).float(), (f * q[:, k].double()).float()
    return (0.0 <= t) & (t <= 1.0) & (p[:, j] <= hj) & (hj <= p[:, j] + vs) & (p[:, k] <= hk) & (hk <= p[:, k] + vs)


def _decide(g, gid, level, means, cov, ab0, ab1, cp, iso32):
    vs = _voxel_size(level)
    v = g.float() * vs + (-1.0)                     # == fmaf(g, vs, -1): g * vs is exact
    a0, a1 = ab0[gid], ab1[gid]
    inside = (v <= a0).all(1) & (v + vs >= a1).all(1)
    overlap = ~((a1 < v).any(1) | (a0 > v + vs).any(1))
    p = v - means[gid]
    hit = torch.zeros_like(inside)
    for i, j, k in ((0, 1, 2), (1, 0, 2), (2, 0, 1)):
        q = cp[gid, i]
        for o in (0.0, vs):
            hit |= _face_test(p, q, vs, i, j, k, o)
    C = cov[gid].unbind(1)
    for i in range(4):
        o1, o2 = (vs if i // 2 else 0.0), (vs if i % 2 else 0.0)
        hit |= _edge_test(C[0], C[1], C[2], C[3], C[4], C[5], iso32, p[:, 1] + o1, p[:, 2] + o2, p[:, 0], p[:, 0] + vs)
        hit |= _edge_test(C[3], C[1], C[4], C[0], C[2], C[5], iso32, p[:, 0] + o1, p[:, 2] + o2, p[:, 1], p[:, 1] + vs)
        hit |= _edge_test(C[5], C[2], C[4], C[0], C[1], C[3], iso32, p[:, 0] + o1, p[:, 1] + o2, p[:, 2], p[:, 2] + vs)
    return inside | (overlap & hit)


def _morton(g):
    m = torch.zeros(g.size(0), dtype=torch.long, device=g.device)
    for b in range(15):
        m |= (((g[:, 0] >> b) & 1) << (3 * b + 2)) | (((g[:, 1] >> b) & 1) << (3 * b + 1)) | (((g[:, 2] >> b) & 1) << (3 * b))
    return m


def gs_to_spc_torch(means, scales, rots, iso, tol, level):
    """-> [points int16 (N, 3), gaus_id int64 (N,), pack_boundary bool (N,), cov3d_invs float32 (G, 6)], on the inputs' device"""
    dev, level = means.device, int(level)
    cov, ab0, ab1, cp = _prepare(means, scales, rots, iso, tol, level)
    iso32 = _f32(iso)
    G = means.size(0)
    g = torch.zeros((G, 3), dtype=torch.long, device=dev)
    gid = torch.arange(G, dtype=torch.long, device=dev)
    child = torch.tensor([[i >> 2, (i >> 1) & 1, i & 1] for i in range(8)], dtype=torch.long, device=dev)
    for l in range(level + 1):
        keep = _decide(g, gid, l, means, cov, ab0, ab1, cp, iso32)
        g, gid = g[keep], gid[keep]
        if l < level:
            g = (2 * g[:, None, :] + child[None]).reshape(-1, 3)
            gid = gid.repeat_interleave(8)
    m, order = torch.sort(_morton(g), stable=True)
    g, gid = g[order], gid[order]
    boundary = torch.ones(m.size(0), dtype=torch.bool, device=dev)
    boundary[1:] = m[1:] != m[:-1]
    return [g.to(torch.int16).contiguous(), gid.contiguous(), boundary, cov]


def integrate_gs_torch(points, gaus_id, means, cov3d_invs, opacities, level, step, chunk=None):
    """-> float32 (N,): opacity * (the mean of exp(-q / 2) over step^3 samples of the voxel), accumulated in float64"""
    dev, step = points.device, int(step)
    vs = _voxel_size(level)
    step_size = float(torch.tensor(vs, dtype=torch.float32) / torch.tensor(float(step - 1 if step > 1 else 1), dtype=torch.float32))
    opac = opacities.reshape(-1)
    idx = torch.arange(step, dtype=torch.float32, device=dev)
    out = torch.empty(points.size(0), dtype=torch.float32, device=dev)
    chunk = chunk or (4096 if dev.type == 'cpu' else 65536)
    for s in range(0, points.size(0), chunk):
        gid = gaus_id[s:s + chunk]
        fp = ((vs * points[s:s + chunk].float()).double() - 1.0).float()
        mean = means[gid]
        c0, c1, c2, c3, c4, c5 = (c[:, None, None, None] for c in cov3d_invs[gid].double().unbind(1))
        off = [((fp[:, a, None] + idx[None, :] * step_size) - mean[:, a, None]).double() for a in range(3)]
        vx, vy, vz = off[0][:, :, None, None], off[1][:, None, :, None], off[2][:, None, None, :]
        inter = c0 * vx * vx + 2.0 * c1 * vx * vy + c3 * vy * vy
        total = torch.exp(-0.5 * (inter + 2.0 * c2 * vx * vz + 2.0 * c4 * vy * vz + c5 * vz * vz)).sum(dim=(1, 2, 3))
        out[s:s + chunk] = (opac[gid].double() * total / float(step * step * step)).float()
    return out
