"""kaolin.ops.conversions.FlexiCubes (*Shen et al.*, `Flexible Isosurface Extraction for Gradient-Based Mesh Optimization`_):
differentiable dual marching cubes over a voxel grid of (possibly deformed) vertices and a scalar field.

Two implementations of one contract and the same orders:
  * float32 GPU tensors without ``voxelgrid_features`` run the HIP pipeline of csrc/flexicubes.hip (``_C.ops.conversions``);
  * everything else (CPU, float64, half, features) runs the torch formulation below: one pass over all dual vertices, padded to
    7 edges each, no loop over the four count classes and no host read but the empty-surface test.
The case tables are generated from rules (tools/gen_flexicubes_table.py).

.. _Flexible Isosurface Extraction for Gradient-Based Mesh Optimization:
    https://research.nvidia.com/labs/toronto-ai/flexicubes/
"""
import torch
from torch.autograd.function import once_differentiable

from .... import _C
from ....utils import testing
from ._tables import CHECK_TABLE, DMC_TABLE, NUM_VD_TABLE

__all__ = ['FlexiCubes']

# the cube's 12 edges as corner pairs, corners k = x + 2 y + 4 z
CUBE_EDGES = ((0, 1), (1, 5), (4, 5), (0, 4), (2, 3), (3, 7), (6, 7), (2, 6), (2, 0), (3, 1), (7, 5), (6, 4))
_TABLES = {}


def _tables(device):
    device = torch.device(device)
    if device not in _TABLES:
        _TABLES[device] = (torch.tensor(DMC_TABLE, dtype=torch.long, device=device),
                           torch.tensor(NUM_VD_TABLE, dtype=torch.long, device=device),
                           torch.tensor(CHECK_TABLE, dtype=torch.long, device=device),
                           torch.tensor([e[0] for e in CUBE_EDGES], dtype=torch.long, device=device),
                           torch.tensor([e[1] for e in CUBE_EDGES], dtype=torch.long, device=device))
    return _TABLES[device]


def _resolution3(resolution):
    if isinstance(resolution, (list, tuple)):
        res = tuple(int(r) for r in resolution)
    else:
        res = (int(resolution),) * 3
    if len(res) != 3 or min(res) < 1:
        raise ValueError(f"'resolution' should be a positive int or 3 positive ints, but got {resolution}")
    return res


def _check_grid(cube_idx, res):
    """The ambiguity rule reads a cube's neighbour by position: the cubes are laid out x ry rz + y rz + z (the reference indexes
    a (rx, ry, rz) volume with them and fails otherwise)."""
    if cube_idx.shape[0] != res[0] * res[1] * res[2]:
        raise ValueError(f"'cube_idx' holds {cube_idx.shape[0]} cubes, but 'resolution' {tuple(res)} means "
                         f"{res[0] * res[1] * res[2]}")


def normalize_weights(beta, alpha, gamma_f, weight_scale):
    """tanh / sigmoid normalisation of the raw weights (None stays None = all ones)."""
    if beta is not None:
        beta = torch.tanh(beta) * weight_scale + 1
    if alpha is not None:
        alpha = torch.tanh(alpha) * weight_scale + 1
    if gamma_f is not None:
        gamma_f = torch.sigmoid(gamma_f) * weight_scale + (1 - weight_scale) / 2
    return beta, alpha, gamma_f


@torch.no_grad()
def topology_torch(scalar_field, cube_idx, res):
    """Everything integer about one call, or None when no cube is crossed:
        cubes (S,)           the surface cubes, ascending
        vd_cube (N,)         per dual vertex its surface cube (an index into ``cubes``); dual vertices go by count class
                             ascending, then surface cube, then group
        slots, mask (N, 7)   per dual vertex its cube edges, ascending; where mask is False the first edge is repeated
        a, b (N, 7)          the grid vertices at the ends of those edges, as written in CUBE_EDGES
        quads (Q, 4)         dual-vertex ids: by surface-edge rank, the quads whose first endpoint has sdf > 0 first
    """
    dev = scalar_field.device
    dmc, num_vd, check, e0, e1 = _tables(dev)
    cube_idx = cube_idx.long()
    occ = scalar_field < 0
    case = (occ[cube_idx.reshape(-1)].reshape(-1, 8).long() << torch.arange(8, device=dev)).sum(-1)
    surf = (case > 0) & (case < 255)
    cubes = torch.nonzero(surf).squeeze(1)
    if cubes.shape[0] == 0:
        return None
    # ambiguity: a marked cube is inverted iff the cube across its ambiguous face exists and is marked too (in any direction)
    row = check[case]
    marked = row[:, 0] == 1
    lin = torch.arange(case.shape[0], device=dev)
    pos = torch.stack([lin // (res[1] * res[2]), (lin // res[2]) % res[1], lin % res[2]], 1) + row[:, 1:4]
    inside = ((pos >= 0) & (pos < torch.tensor(res, device=dev))).all(1)
    other = (pos[:, 0] * res[1] + pos[:, 1]) * res[2] + pos[:, 2]
    invert = marked & inside & marked[other.clamp(0, case.shape[0] - 1)]
    case = torch.where(invert, row[:, 4], case)[cubes]

    corners = cube_idx[cubes]                                   # (S, 8)
    ea, eb = corners[:, e0], corners[:, e1]                     # (S, 12)
    # surface edges: unique (first id, second id) pairs, as written; one key per pair keeps their lexicographic order
    key = (ea * scalar_field.shape[0] + eb).reshape(-1)
    _, inverse, counts = torch.unique(key, return_inverse=True, return_counts=True)
    crossed = (occ[ea] != occ[eb]).reshape(-1)

    n = num_vd[case]
    cube_of, group_of = torch.nonzero(torch.arange(4, device=dev).unsqueeze(0) < n.unsqueeze(1), as_tuple=True)
    order = torch.argsort(n[cube_of], stable=True)              # count class ascending; cube, then group inside a class
    vd_cube, vd_group = cube_of[order], group_of[order]
    slots = dmc[case[vd_cube], vd_group]                        # (N, 7)
    mask = slots >= 0
    slots = torch.where(mask, slots, slots[:, :1])
    rows = vd_cube.unsqueeze(1).expand(-1, 7)
    a, b = ea[rows, slots], eb[rows, slots]

    vd_of = torch.zeros(cubes.shape[0] * 12, dtype=torch.long, device=dev)
    vd_of[(rows * 12 + slots)[mask]] = torch.arange(vd_cube.shape[0], device=dev).unsqueeze(1).expand(-1, 7)[mask]
    in_quad = (counts[inverse] == 4) & crossed                  # crossed edges shared by four cubes
    edge, at = torch.sort(inverse[in_quad], stable=True)        # by surface-edge rank; the four cubes ascending
    quads = vd_of[in_quad][at].reshape(-1, 4)
    first = ea.reshape(-1)[in_quad][at].reshape(-1, 4)[:, 0]
    flip = scalar_field[first] > 0
    quads = torch.cat([quads[flip][:, [0, 1, 3, 2]], quads[~flip][:, [2, 3, 1, 0]]])
    return dict(cubes=cubes, vd_cube=vd_cube, slots=slots, mask=mask, a=a, b=b, quads=quads)


def _interp(w0, w1, p0, p1):
    """(p0 w0 + p1 w1) / (w0 + w1): the point of an edge with the weights (s1, -s0) of its ends."""
    return (p0 * w0.unsqueeze(-1) + p1 * w1.unsqueeze(-1)) / (w0 + w1).unsqueeze(-1)


def _slot_sum(values, mask):
    """Sum over the 7 slots of a dual vertex, sequential in slot order (what the HIP kernel and a CPU index_add_ do)."""
    m = mask.to(values.dtype)
    if values.dim() == 3:
        m = m.unsqueeze(-1)
    total = values[:, 0] * m[:, 0]
    for j in range(1, 7):
        total = total + values[:, j] * m[:, j]
    return total


def numerics_gathered(x0, x1, s0, s1, al0, al1, be, gamma_vd, mask, quads, training, f0=None, f1=None):
    """The differentiable part on per-incidence operands, all (N, 7, ...): the ends' positions, sdf values and alpha weights, the
    edge's beta weight; gamma_vd (N,).  -> (vertices, L_dev, features or None)."""
    w0, w1 = s1 * al1, -(s0 * al0)
    beta_sum = _slot_sum(be, mask)
    vd = _slot_sum(_interp(w0, w1, x0, x1) * be.unsqueeze(-1), mask) / beta_sum.unsqueeze(-1)
    zero_crossing = _interp(s1, -s0, x0, x1)
    dist = torch.linalg.norm(zero_crossing - vd.unsqueeze(1), dim=-1)
    mean = _slot_sum(dist, mask) / mask.sum(1).to(dist.dtype)
    l_dev = (dist - mean.unsqueeze(1)).abs()[mask]
    feats = None
    if f0 is not None:
        feats = _slot_sum(_interp(w0, w1, f0, f1) * be.unsqueeze(-1), mask) / beta_sum.unsqueeze(-1)
    if training:
        g = gamma_vd[quads]                                     # (Q, 4)
        g02, g13 = (g[:, 0] * g[:, 2]).unsqueeze(-1), (g[:, 1] * g[:, 3]).unsqueeze(-1)
        weight_sum = (g02 + g13) + 1e-8

        def centre(t):
            q = t[quads]
            return ((q[:, 0] + q[:, 2]) / 2 * g02 + (q[:, 1] + q[:, 3]) / 2 * g13) / weight_sum
        if feats is not None:
            feats = torch.cat([feats, centre(feats)])
        vd = torch.cat([vd, centre(vd)])
    return vd, l_dev, feats


def gather_operands(topo, vertices, scalar_field, beta, alpha, gamma_f, features=None):
    """The operands of ``numerics_gathered`` from the grid's tensors and the NORMALISED weights (None = ones)."""
    dev, dt = vertices.device, vertices.dtype
    _, _, _, e0, e1 = _tables(dev)
    a, b, slots, cube = topo['a'], topo['b'], topo['slots'], topo['cubes'][topo['vd_cube']]
    rows = cube.unsqueeze(1).expand(-1, 7)
    ones = torch.ones(a.shape, dtype=dt, device=dev)
    al0 = alpha[rows, e0[slots]] if alpha is not None else ones
    al1 = alpha[rows, e1[slots]] if alpha is not None else ones
    be = beta[rows, slots] if beta is not None else ones
    gamma_vd = gamma_f[cube] if gamma_f is not None else ones[:, 0]
    ops = dict(x0=vertices[a], x1=vertices[b], s0=scalar_field[a], s1=scalar_field[b], al0=al0, al1=al1, be=be,
               gamma_vd=gamma_vd)
    if features is not None:
        ops['f0'], ops['f1'] = features[a], features[b]
    return ops


def triangulate(topo, gamma_vd, num_vd, training):
    """faces (F, 3) int64 from the quads: two triangles per quad, split by gamma0 gamma2 > gamma1 gamma3; in training four, around
    a centre vertex appended after the ``num_vd`` dual vertices."""
    quads = topo['quads']
    dev = quads.device
    if training:
        centre = torch.arange(quads.shape[0], device=dev).reshape(-1, 1, 1).expand(-1, 4, 1) + num_vd
        sides = quads[:, [0, 1, 1, 2, 2, 3, 3, 0]].reshape(-1, 4, 2)
        return torch.cat([sides, centre], -1).reshape(-1, 3)
    g = gamma_vd.detach()[quads]
    first = (g[:, 0] * g[:, 2] > g[:, 1] * g[:, 3]).unsqueeze(1)
    return torch.where(first, quads[:, [0, 1, 2, 0, 2, 3]], quads[:, [0, 1, 3, 3, 1, 2]]).reshape(-1, 3)


def flexicubes_torch(vertices, scalar_field, cube_idx, res, weight_scale=0.99, beta=None, alpha=None, gamma_f=None,
                     training=False, features=None):
    """The definition, on any device and in any floating-point dtype.  -> (vertices, faces, L_dev, features or None)."""
    dev, dt = vertices.device, vertices.dtype
    _check_grid(cube_idx, res)
    topo = topology_torch(scalar_field, cube_idx, res)
    if topo is None:
        return (torch.zeros((0, 3), dtype=dt, device=dev), torch.zeros((0, 3), dtype=torch.long, device=dev),
                torch.zeros((0,), dtype=dt, device=dev),
                None if features is None else torch.zeros((0, features.shape[-1]), dtype=features.dtype, device=dev))
    beta, alpha, gamma_f = normalize_weights(beta, alpha, gamma_f, weight_scale)
    ops = gather_operands(topo, vertices, scalar_field, beta, alpha, gamma_f, features)
    verts, l_dev, feats = numerics_gathered(mask=topo['mask'], quads=topo['quads'], training=training, **ops)
    faces = triangulate(topo, ops['gamma_vd'], topo['vd_cube'].shape[0], training)
    return verts, faces, l_dev, feats


class _FlexiCubesHip(torch.autograd.Function):
    """float32 GPU tensors -> (vertices, L_dev, faces) on the HIP pipeline; the backward is HIP too and recomputes from the
    inputs and the integer state of the forward."""

    @staticmethod
    def forward(ctx, vertices, scalar_field, beta, alpha, gamma_f, cube_idx, res, weight_scale, training):
        verts, faces, l_dev, state = _C.ops.conversions.flexicubes_forward_cuda(
            vertices, scalar_field, cube_idx, res, weight_scale, beta, alpha, gamma_f, training)
        ctx.save_for_backward(vertices, scalar_field, beta, alpha, gamma_f, cube_idx, verts, *state)
        ctx.args = (weight_scale, training)
        ctx.mark_non_differentiable(faces)
        return verts, l_dev, faces

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_verts, grad_l_dev, _):
        vertices, scalar_field, beta, alpha, gamma_f, cube_idx, verts, *state = ctx.saved_tensors
        weight_scale, training = ctx.args
        grads = _C.ops.conversions.flexicubes_backward_cuda(grad_verts, grad_l_dev, vertices, scalar_field, cube_idx, weight_scale,
                                                            beta, alpha, gamma_f, training, verts, state)
        return (*grads, None, None, None, None)


class FlexiCubes:
    r"""FlexiCubes: differentiable dual marching cubes, the reference's class (``kaolin.ops.conversions.FlexiCubes``).

    Extracts a triangle mesh from a scalar field on a voxel grid whose vertices may be deformed; per-cube weights ``beta`` (edges),
    ``alpha`` (corners) and ``gamma_f`` (quad split) move the dual vertices.  The output is differentiable in the vertex positions,
    the scalar field and the weights.  Vertex, face and ``L_dev`` orders are the reference's: dual vertices go by the number of
    dual vertices of their cube (1 to 4), then by cube, then by group as the generated case table lists them; quads by the rank of
    their grid edge among the crossed edges ``(first id, second id)``, those whose first endpoint has ``sdf > 0`` first.

    float32 GPU tensors without ``voxelgrid_features`` run a HIP pipeline (csrc/flexicubes.hip) with two host reads per call
    (the sizes of the surface and the index-error flag; the number of quads): the call synchronises the current stream and
    **cannot be captured in a HIP graph**.  Its forward uses no atomics (two calls give the same bits); its backward adds the
    gradients of the shared grid vertices and sdf values with float atomics (run-to-run variation of rounding size) and writes
    ``beta``, ``alpha`` and ``gamma_f`` rows by their owner.  Every other input runs the same contract in plain torch.

    ``output_tetmesh=True`` and ``grad_func`` are not implemented (they need the tetrahedralisation table and a batched
    least-squares solve) and raise ``NotImplementedError``.

    Args:
        device (torch.device or str): where ``construct_voxel_grid`` builds its tensors. Default: ``'cuda'``.
    """

    def __init__(self, device="cuda"):
        self.device = device

    def construct_voxel_grid(self, resolution):
        r"""The vertices of a regular voxel grid in :math:`[-0.5, 0.5]^3` and the 8 vertex ids of every voxel.

        Args:
            resolution (int or list[int]): the number of voxels, for all three or per dimension (x, y, z).

        Return:
            (torch.Tensor, torch.LongTensor): the vertices, of shape :math:`((r_x+1)(r_y+1)(r_z+1), 3)`, ordered by (x, y, z),
            and the cubes, of shape :math:`(r_x r_y r_z, 8)`, cube :math:`x r_y r_z + y r_z + z`, corner :math:`k = dx + 2 dy + 4 dz`.
        """
        res = _resolution3(resolution)
        dev = self.device
        # a coordinate is i / r, rounded to 5 decimals (float32), minus 0.5
        axes = [torch.round(torch.arange(r + 1, device=dev).float() / float(r) * 10 ** 5) / (10 ** 5) - 0.5 for r in res]
        verts = torch.stack(torch.meshgrid(*axes, indexing='ij'), -1).reshape(-1, 3)
        ix, iy, iz = torch.meshgrid(*[torch.arange(r, device=dev) for r in res], indexing='ij')
        k = torch.arange(8, device=dev)
        cubes = (((ix.reshape(-1, 1) + (k & 1)) * (res[1] + 1) + iy.reshape(-1, 1) + ((k >> 1) & 1)) * (res[2] + 1)
                 + iz.reshape(-1, 1) + ((k >> 2) & 1))
        return verts, cubes

    def __call__(self, voxelgrid_vertices, scalar_field, cube_idx, resolution, qef_reg_scale=1e-3,
                 weight_scale=0.99, beta=None, alpha=None, gamma_f=None, training=False,
                 output_tetmesh=False, grad_func=None, voxelgrid_features=None):
        r"""Extracts the mesh.

        Args:
            voxelgrid_vertices (torch.Tensor): vertex positions, of shape :math:`(\text{num_vertices}, 3)`.
            scalar_field (torch.Tensor): the field at the vertices, negative inside, of shape :math:`(\text{num_vertices},)`.
            cube_idx (torch.LongTensor): the 8 vertex ids of every cube, of shape :math:`(\text{num_cubes}, 8)`, cubes laid out
                as ``construct_voxel_grid`` does.
            resolution (int or list[int]): the resolution of the grid.
            qef_reg_scale (float, optional): only used with ``grad_func``. Default: 1e-3.
            weight_scale (float, optional): the scale of the weights, in (0, 1). Default: 0.99.
            beta (torch.Tensor, optional): of shape :math:`(\text{num_cubes}, 12)`. Default: uniform.
            alpha (torch.Tensor, optional): of shape :math:`(\text{num_cubes}, 8)`. Default: uniform.
            gamma_f (torch.Tensor, optional): of shape :math:`(\text{num_cubes},)`. Default: uniform.
            training (bool, optional): four triangles per quad around a weighted centre vertex. Default: False.
            output_tetmesh (bool, optional): not implemented.
            grad_func (callable, optional): not implemented.
            voxelgrid_features (torch.Tensor, optional): of shape :math:`(\text{num_vertices}, \text{num_channels})`.

        Return:
            (torch.Tensor, torch.LongTensor, torch.Tensor[, torch.Tensor]): vertices :math:`(\text{V}, 3)`, faces
            :math:`(\text{F}, 3)`, ``L_dev`` with one entry per (dual vertex, edge) incidence and, with ``voxelgrid_features``,
            the features of the vertices.
        """
        def require(ok, text):                                  # (the reference asserts: same type, same text)
            if not ok:
                raise AssertionError(text)

        def shaped(t, shape):
            return torch.is_tensor(t) and testing.check_tensor(t, shape, throw=False)
        require(shaped(voxelgrid_vertices, (None, 3)), "'voxelgrid_vertices' should be a tensor of shape (num_vertices, 3)")
        num_vertices = voxelgrid_vertices.shape[0]
        require(shaped(scalar_field, (num_vertices,)), "'scalar_field' should be a tensor of shape (num_vertices,)")
        require(shaped(cube_idx, (None, 8)), "'cube_idx' should be a tensor of shape (num_cubes, 8)")
        num_cubes = cube_idx.shape[0]
        require(beta is None or shaped(beta, (num_cubes, 12)), "'beta' should be a tensor of shape (num_cubes, 12)")
        require(alpha is None or shaped(alpha, (num_cubes, 8)), "'alpha' should be a tensor of shape (num_cubes, 8)")
        require(gamma_f is None or shaped(gamma_f, (num_cubes,)), "'gamma_f' should be a tensor of shape (num_cubes,)")
        require(voxelgrid_features is None or shaped(voxelgrid_features, (num_vertices, None)),
                "'voxelgrid_features' should be a tensor of shape (num_cubes, num_features)")
        require(voxelgrid_features is None or not (output_tetmesh or grad_func is not None),
                "'voxelgrid_features' is not supported with 'output_tetmesh' or 'grad_func'")
        if output_tetmesh:
            raise NotImplementedError("FlexiCubes: 'output_tetmesh=True' is not implemented (out of scope: it needs the "
                                      "tetrahedralisation table)")
        if grad_func is not None:
            raise NotImplementedError("FlexiCubes: 'grad_func' is not implemented (out of scope: it needs a batched "
                                      "least-squares solve)")
        res = _resolution3(resolution)
        weights = [w for w in (beta, alpha, gamma_f) if w is not None]
        hip = (voxelgrid_vertices.is_cuda and voxelgrid_features is None and cube_idx.dtype == torch.long
               and all(t.dtype == torch.float32 and t.device == voxelgrid_vertices.device
                       for t in (voxelgrid_vertices, scalar_field, *weights))
               and cube_idx.device == voxelgrid_vertices.device)
        if hip:
            _check_grid(cube_idx, res)
            vertices, l_dev, faces = _FlexiCubesHip.apply(voxelgrid_vertices, scalar_field, beta, alpha, gamma_f, cube_idx, res,
                                                          float(weight_scale), bool(training))
            return vertices, faces, l_dev
        vertices, faces, l_dev, feats = flexicubes_torch(voxelgrid_vertices, scalar_field, cube_idx, res, weight_scale, beta,
                                                         alpha, gamma_f, training, voxelgrid_features)
        if voxelgrid_features is None:
            return vertices, faces, l_dev
        return vertices, faces, l_dev, feats
