"""Voxelgrid conversions behind the API of kaolin/ops/conversions/voxelgrid.py: ``voxelgrids_to_cubic_meshes`` (Mesh R-CNN's
"Cubify"), same signature, default, result dtypes and orders.

The reference finds the faces with a ``conv3d`` and a ``nonzero`` and merges the corners with one ``torch.unique(dim=0)`` per
item -- a lexicographic sort of 4 F float rows.  No sort is needed: every vertex is a point of the (X+1)(Y+1)(Z+1) integer
lattice, so lattice order is "unique, sorted", a vertex's id is a prefix count of a flag over the lattice, and the reference's
face order (axis, then raster order of the face's location) is a prefix count too.  On a GPU tensor that pipeline runs as HIP
kernels (kaolin_amd/csrc/cubic_meshes.hip); on the CPU it is the same pipeline in plain torch (flags, ``cumsum``, gathers),
which is also the readable definition.

``voxelgrids_to_trianglemeshes`` (marching cubes) is the sibling pipeline: a case byte per cell of the (X+1)(Y+1)(Z+1) lattice of
the zero-bordered grid, one vertex per crossed lattice edge (owned by the cell at the edge's lower end), vertex ids and face rows
as prefix counts (kaolin_amd/csrc/mcube.hip); ``_trianglemeshes_torch`` is the same pipeline in plain torch.  Its 256-case
triangle table is generated from rules (tools/gen_mcube_table.py -> kaolin_amd/csrc/mcube_table.h).
"""
import math
import os
import re

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from ... import _C
from ..voxelgrid import _require_4d

__all__ = ['voxelgrids_to_cubic_meshes', 'voxelgrids_to_trianglemeshes']


def _corner_offsets(sx, sy):
    """Per axis, the four corners of the quad of a face located at lattice point p, as offsets from p in lattice points (the
    lattice is raveled with strides sx, sy, 1), in the reference's corner order.  The corners are p and three earlier points:
        axis 0: (0,-1,-1) (0,0,-1) (0,0,0) (0,-1,0)    axis 1: (-1,0,-1) (-1,0,0) (0,0,0) (0,0,-1)
        axis 2: (-1,-1,0) (0,-1,0) (0,0,0) (-1,0,0)"""
    return [[-sy - 1, -1, 0, -sy], [-sx - 1, -sx, 0, -1], [-sx - sy, -sy, 0, -sx]]


def _cubic_meshes_torch(voxelgrids, is_trimesh):
    """The definition, on any device: flags over the lattice, prefix counts, gathers.  No sort, no loop over the batch."""
    B, X, Y, Z = voxelgrids.shape
    dev = voxelgrids.device
    width = 3 if is_trimesh else 4
    padded = F.pad(voxelgrids.float(), (1, 1, 1, 1, 1, 1))
    # lattice point (i, j, k) is the low corner of voxel (i, j, k) = padded[i + 1, j + 1, k + 1]; the face of axis d located
    # there lies between the voxels lo = (i, j, k) - (1, 1, 1) and hi = lo + e_d
    lo = padded[:, :-1, :-1, :-1]
    r = torch.stack([padded[:, 1:, :-1, :-1] - lo, padded[:, :-1, 1:, :-1] - lo, padded[:, :-1, :-1, 1:] - lo]).round()
    face = r != 0                                                    # (3, B, X+1, Y+1, Z+1)
    inverted = r == -1
    # a lattice point is a vertex when it is a corner of some face: the face's own location and three earlier points
    used = torch.zeros(face.shape[1:], dtype=torch.bool, device=dev)
    for d, (u, w) in enumerate(((2, 3), (1, 3), (1, 2))):           # the two lattice axes (as tensor dims) the quad spans
        f = face[d].narrow(u, 1, face.shape[u + 1] - 1).narrow(w, 1, face.shape[w + 1] - 1)   # (a face never sits at index 0 there)
        for du in (0, 1):
            for dw in (0, 1):
                used.narrow(u, du, f.shape[u]).narrow(w, dw, f.shape[w]).logical_or_(f)
    L = (X + 1) * (Y + 1) * (Z + 1)
    used = used.view(B, L)
    rank = used.cumsum(1) - 1                                        # int64: the vertex id of a used lattice point in its item
    num_verts = used.sum(1)
    verts = torch.nonzero(used.view(B, X + 1, Y + 1, Z + 1))[:, 1:].float()

    face = face.view(3, B, L)
    num_faces = face.sum(2)                                          # (3, B)
    num_quads = num_faces.sum(0)                                     # (B)
    item_first = num_quads.cumsum(0) - num_quads                     # the first quad of every item in the batch's buffer
    axis_first = num_faces.cumsum(0) - num_faces                     # ... and of every axis within its item
    quads = torch.empty((int(num_quads.sum()), 4), dtype=torch.long, device=dev)
    item_of_quad = torch.empty(quads.shape[0], dtype=torch.long, device=dev)
    offsets = torch.tensor(_corner_offsets((Y + 1) * (Z + 1), Z + 1), dtype=torch.long, device=dev)
    for d in range(3):
        b, p = torch.nonzero(face[d], as_tuple=True)                 # ordered by item, then raster order of the location
        q = rank[b.unsqueeze(1), p.unsqueeze(1) + offsets[d]]
        q = torch.where(inverted.view(3, B, L)[d, b, p].unsqueeze(1), q.flip(1), q)
        group_first = num_faces[d].cumsum(0) - num_faces[d]          # the first face of every item among this axis' faces
        row = item_first[b] + axis_first[d, b] + torch.arange(b.shape[0], device=dev) - group_first[b]
        quads[row] = q
        item_of_quad[row] = b
    if is_trimesh:
        faces = torch.empty((2 * quads.shape[0], 3), dtype=torch.long, device=dev)
        row = torch.arange(quads.shape[0], device=dev) + item_first[item_of_quad]     # item b starts at row 2 item_first[b]
        faces[row] = quads[:, [0, 3, 1]]
        faces[row + num_quads[item_of_quad]] = quads[:, [2, 1, 3]]
    else:
        faces = quads
    nv, nq = num_verts.tolist(), num_quads.tolist()                  # the one host read
    return list(torch.split(verts, nv)), list(torch.split(faces, [(2 if is_trimesh else 1) * n for n in nq]))


def voxelgrids_to_cubic_meshes(voxelgrids, is_trimesh=True):
    r"""Convert voxelgrids to meshes by replacing each occupied voxel with a unit cube and dropping the internal faces: one
    quad (or two triangles) per exposed voxel face, the lattice corners merged into shared vertices.  With
    ``is_trimesh=True`` this is "Cubify" of the ICCV 2019 paper "Mesh R-CNN": https://arxiv.org/abs/1906.02739.

    Values are taken as float32.  With the grid padded by one voxel of zeros on every side, two adjacent voxels ``lo`` and
    ``hi = lo + e_d`` have a face between them when ``r = rint(hi - lo)`` (half to even) is not 0, wound the opposite way when
    ``r == -1``.  A binary grid is the intended use; the rule makes other finite values well defined (0.5 next to 0: no face).
    NaN and infinities are unspecified.

    ``verts[b]`` holds the lattice points touched by a face of item ``b`` in lexicographic :math:`(x, y, z)` order, in voxel
    units: :math:`(i, j, k)` is the low corner of voxel :math:`(i, j, k)`.  Quads are ordered by axis (0, 1, 2) and, within
    an axis, in raster order of the face's location; triangle ``n`` and ``N_b + n`` are corners ``[0, 3, 1]`` and
    ``[2, 1, 3]`` of quad ``n``.

    On a GPU tensor this is a HIP pipeline without a sort; bool, uint8, half and float grids of any strides are read in place,
    other dtypes are cast once with ``.float()``.  Result sizes depend on the data, so the host reads the per-item counts once:
    the call synchronises the current stream and **cannot be captured in a HIP graph**.  The lattice
    :math:`(X+1)(Y+1)(Z+1)` of one item must stay below :math:`2^{31}` there.  On the CPU it is the same pipeline in plain torch.

    Where the reference fails incidentally this function does not: an empty batch gives two empty lists (the reference dies
    in ``repeat_interleave``), a tensor that is not 4-dimensional raises ``ValueError`` (the reference dies in ``conv3d``),
    and a non-binary grid in which some axis has no face while another has one follows the rule above (the reference's
    per-axis counts misalign).

    .. Note::
        This function is not differentiable: the input is detached and the outputs never require grad.

    Args:
        voxelgrids (torch.Tensor): binary voxel array, of shape
                                   :math:`(\text{batch_size}, \text{X}, \text{Y}, \text{Z})`.
        is_trimesh (optional, bool): if True, the outputs are triangular meshes.
                                     Otherwise quadmeshes are returned. Default: True.

    Returns:
        (list[torch.Tensor], list[torch.LongTensor]):

            - The list of vertices for each mesh, each of shape :math:`(\text{V}_b, 3)`, float32.
            - The list of faces for each mesh, each of shape :math:`(2 \text{N}_b, 3)` or :math:`(\text{N}_b, 4)`.

    Example:
        >>> voxelgrids = torch.ones((1, 1, 1, 1))
        >>> verts, faces = voxelgrids_to_cubic_meshes(voxelgrids)
        >>> verts[0]
        tensor([[0., 0., 0.],
                [0., 0., 1.],
                [0., 1., 0.],
                [0., 1., 1.],
                [1., 0., 0.],
                [1., 0., 1.],
                [1., 1., 0.],
                [1., 1., 1.]])
        >>> faces[0]
        tensor([[0, 1, 2],
                [5, 4, 7],
                [0, 4, 1],
                [6, 2, 7],
                [0, 2, 4],
                [3, 1, 7],
                [3, 2, 1],
                [6, 7, 4],
                [5, 1, 4],
                [3, 7, 2],
                [6, 4, 2],
                [5, 7, 1]])
        >>> voxelgrids_to_cubic_meshes(voxelgrids, is_trimesh=False)[1][0]
        tensor([[0, 2, 3, 1],
                [5, 7, 6, 4],
                [0, 1, 5, 4],
                [6, 7, 3, 2],
                [0, 4, 6, 2],
                [3, 7, 5, 1]])
    """
    _require_4d(voxelgrids)
    voxelgrids = voxelgrids.detach()
    if voxelgrids.shape[0] == 0:
        return [], []
    if voxelgrids.is_cuda:
        return _C.ops.conversions.voxelgrids_to_cubic_meshes_cuda(voxelgrids, is_trimesh)
    return _cubic_meshes_torch(voxelgrids, is_trimesh)


# ---- marching cubes -----------------------------------------------------------------------------------------------------------
# Cell geometry, in tensor-index terms (dim0, dim1, dim2); tools/gen_mcube_table.py has the rules the table follows.
_MC_CORNERS = ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0))
_MC_EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
_MC_TABLE = None


def _mcube_table():
    """The generated table as Python lists, read once from the header the HIP kernels compile: (256 rows of 16 edge ids ended by
    255, 256 triangle counts)."""
    global _MC_TABLE
    if _MC_TABLE is None:
        path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', 'csrc', 'mcube_table.h')
        with open(path) as f:
            text = re.sub(r'//[^\n]*', '', f.read())
        rows, counts = (list(map(int, re.findall(r'\d+', body))) for body in re.findall(r'=\s*\{([^}]*)\}', text))
        if len(rows) != 256 * 16 or len(counts) != 256:
            raise RuntimeError(f'{path}: not the generated marching-cubes table')
        _MC_TABLE = ([rows[16 * c:16 * c + 16] for c in range(256)], counts)
    return _MC_TABLE


def _trianglemeshes_torch(field, iso_value):
    """The definition, on any device, of marching cubes over ``field`` (B, NX, NY, NZ) AS GIVEN (the public function pads the
    grid with its border of zeros first; the HIP path never builds that copy): case bytes, ``cumsum``, gathers through the
    generated table; no loop over cells or items.  Arithmetic in ``field.dtype`` (float32 is the operator; float64 serves as
    the yardstick of the gradient tests).  Differentiable in ``field`` through the vertices.
    Returns (vertices (sum V_b, 3), faces (sum F_b, 3) int64 with ids local to the item, [V_b], [F_b])."""
    B, NX, NY, NZ = field.shape
    dev, dtype = field.device, field.dtype
    if B == 0 or min(NX, NY, NZ) < 2:
        return (torch.zeros((0, 3), dtype=dtype, device=dev), torch.zeros((0, 3), dtype=torch.long, device=dev), [0] * B, [0] * B)
    rows, counts = _mcube_table()
    table = torch.tensor(rows, dtype=torch.long, device=dev)
    num_tri = torch.tensor(counts, dtype=torch.long, device=dev)
    L, sx, sy = NX * NY * NZ, NY * NZ, NZ
    stride = torch.tensor([sx, sy, 1], dtype=torch.long, device=dev)
    # per cell edge: the lattice point at its lower end, as an offset from the cell, and its axis
    lower = [min(_MC_CORNERS[a], _MC_CORNERS[b]) for a, b in _MC_EDGES]
    edge_offset = torch.tensor([o[0] * sx + o[1] * sy + o[2] for o in lower] + [0] * 244, dtype=torch.long, device=dev)
    edge_axis = torch.tensor([[x != y for x, y in zip(_MC_CORNERS[a], _MC_CORNERS[b])].index(True) for a, b in _MC_EDGES]
                             + [0] * 244, dtype=torch.long, device=dev)
    iso = torch.tensor(iso_value, dtype=torch.float32, device=dev).to(dtype)     # (rounded to float32 once)

    # every lattice point is the corner 0 of a cell; past the last point of an axis the field repeats, so that an edge leaving
    # the lattice is never crossed, and such a cell (not a real one) gets no triangles
    below = field.detach() < iso                                                 # (NaN: not below)
    for d in (1, 2, 3):
        below = torch.cat([below, below.narrow(d, below.shape[d] - 1, 1)], d)
    bit = [below[:, a:a + NX, b:b + NY, c:c + NZ] for a, b, c in _MC_CORNERS]
    case = sum(bit[k].long() << k for k in range(8)).reshape(B, L)
    real = torch.ones((NX, NY, NZ), dtype=torch.bool, device=dev)
    real[-1], real[:, -1], real[:, :, -1] = False, False, False
    # a cell owns the three edges that leave its corner 0 (along dim0, dim1, dim2): one vertex per crossed one
    own = torch.stack([bit[0] ^ bit[4], bit[0] ^ bit[3], bit[0] ^ bit[1]], -1).reshape(B, L, 3)
    own_count = own.sum(2)
    first = own_count.cumsum(1) - own_count                                      # the first vertex id of every cell
    before = own.cumsum(2) - own.long()                                          # own vertices of the cell below an axis
    b, p, axis = torch.nonzero(own, as_tuple=True)                               # item, lattice point, axis: the vertex order
    flat = field.reshape(B, L)
    f_lo, f_hi = flat[b, p], flat[b, p + stride[axis]]
    coords = torch.stack([p // sx, (p // sy) % NY, p % NZ], 1).to(dtype)
    at = coords.gather(1, axis.unsqueeze(1)).squeeze(1)
    moved = torch.where(axis == 0, at + (iso - f_lo) / (f_hi - f_lo), (at + 1) - (iso - f_hi) / (f_lo - f_hi))
    verts = coords.scatter(1, axis.unsqueeze(1), moved.unsqueeze(1))

    tri_count = num_tri[case] * real.reshape(1, L)
    cb, cp = torch.nonzero(tri_count, as_tuple=True)                             # cells in raster order
    n = tri_count[cb, cp]
    cell = torch.repeat_interleave(torch.arange(cb.shape[0], device=dev), n)     # the cell of every triangle
    slot = torch.arange(cell.shape[0], device=dev) - (n.cumsum(0) - n)[cell]     # its number within the cell
    e = table[case[cb, cp][cell].unsqueeze(1), slot.unsqueeze(1) * 3 + torch.arange(3, device=dev)]
    item = cb[cell].unsqueeze(1).expand(-1, 3)
    owner = cp[cell].unsqueeze(1) + edge_offset[e]
    faces = first[item, owner] + before[item, owner, edge_axis[e]]
    return verts, faces, own_count.sum(1).tolist(), tri_count.sum(1).tolist()


class _MarchingCubes(torch.autograd.Function):
    """voxelgrids (half or float, CUDA) -> the vertex buffer of the batch; the faces and the state of the pipeline ride along."""

    @staticmethod
    def forward(ctx, voxelgrids, iso_value):
        verts, faces, nv, nf, state = _C.ops.conversions.mcube_forward_cuda(voxelgrids, iso_value)
        ctx.save_for_backward(voxelgrids, state)
        ctx.iso_value = iso_value
        ctx.mark_non_differentiable(faces)
        return verts, faces, nv, nf

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_verts, *_):
        voxelgrids, state = ctx.saved_tensors
        return _C.ops.conversions.mcube_backward_cuda(grad_verts, voxelgrids, ctx.iso_value, state), None


def _check_iso(iso_value):
    if isinstance(iso_value, torch.Tensor) and iso_value.numel() == 1:
        iso_value = iso_value.item()
    if isinstance(iso_value, bool) or not isinstance(iso_value, (int, float)):
        raise ValueError(f'iso_value must be a real number, but got {type(iso_value).__name__}')
    if not math.isfinite(iso_value):
        raise ValueError(f'iso_value must be finite, but got {iso_value}')
    return float(iso_value)


def voxelgrids_to_trianglemeshes(voxelgrids, iso_value=0.5):
    r"""Converts voxelgrids to triangle meshes with the marching cubes algorithm (*Lorensen, Cline*: `Marching cubes, A high
    resolution 3D surface construction algorithm`_), batched, on the GPU or the CPU.

    The field is the grid, taken as float32, with an implicit border of zeros: voxel :math:`n` sits at coordinate :math:`n + 1`
    and the surface of a grid that is full up to its boundary is closed.  A corner is *below* when its value is
    :math:`< \text{iso_value}` (``iso_value`` rounded to float32; NaN is not below), and every lattice edge with one end below
    carries one vertex, shared by the up to four cells around it: on an edge along dim 1 or dim 2 at
    :math:`p_{hi} - (iso - f_{hi}) / (f_{lo} - f_{hi})`, on an edge along dim 0 at :math:`p_{lo} + (iso - f_{lo}) / (f_{hi} - f_{lo})`
    (float32, one division and one addition: the bits of the reference's kernel).  A crossed edge with a NaN end gives a NaN
    vertex.

    ``vertices[b]`` is ordered by the raster index (dim 0 slowest) of the lower end of the vertex' edge, then by the edge's axis;
    ``faces[b]`` by cell in raster order, then as the case table lists the cell's triangles.  Normals point from the values
    :math:`\geq` ``iso_value`` to those below.  Two calls give the same bits.

    Compared with the reference: the same surface -- the same vertices as a set and, on every cell face, the same segments --
    but another vertex order inside a cell, another split of a cell's loops into triangles and another triangle order inside a
    cell (its table is not reproduced: ours is generated from rules, tools/gen_mcube_table.py); grids that are not cubes are
    handled correctly; there is no cap on the number of vertices; CPU tensors work (the same pipeline in plain torch, same
    bits); the batch is one pipeline, not a loop; and ``vertices[b]`` is differentiable in a floating-point ``voxelgrids``
    that requires grad (through the position along the edge; the reference returns no gradient).

    On a GPU tensor this is a HIP pipeline; bool, uint8, half and float grids of any strides are read in place, other dtypes
    are cast once with ``.float()``.  Result sizes depend on the data, so the host reads the per-item counts once: the call
    synchronises the current stream and **cannot be captured in a HIP graph**.

    Args:
        voxelgrids (torch.Tensor): voxel array of shape :math:`(\text{batch_size}, \text{X}, \text{Y}, \text{Z})`,
                                   any :math:`\text{X}, \text{Y}, \text{Z} \geq 1` with
                                   :math:`3 (X+1)(Y+1)(Z+1) < 2^{31}` (the most vertices an item can have).
        iso_value (optional, float): the level of the surface. Default: 0.5.

    Returns:
        (list[torch.FloatTensor], list[torch.LongTensor]):

            - The list of vertices of each mesh, each of shape :math:`(\text{V}_b, 3)`, float32.
            - The list of faces of each mesh, each of shape :math:`(\text{F}_b, 3)`, int64.

    Example:
        >>> voxelgrid = torch.tensor([[[[1, 0],
        ...                             [0, 0]],
        ...                            [[0, 0],
        ...                             [0, 0]]]], dtype=torch.uint8)
        >>> vertices, faces = voxelgrids_to_trianglemeshes(voxelgrid)
        >>> vertices[0]
        tensor([[0.5000, 1.0000, 1.0000],
                [1.0000, 0.5000, 1.0000],
                [1.0000, 1.0000, 0.5000],
                [1.5000, 1.0000, 1.0000],
                [1.0000, 1.5000, 1.0000],
                [1.0000, 1.0000, 1.5000]])
        >>> faces[0].shape
        torch.Size([8, 3])

    .. _Marching cubes, A high resolution 3D surface construction algorithm:
        https://www.researchgate.net/publication/202232897_Marching_Cubes_A_High_Resolution_3D_Surface_Construction_Algorithm
    """
    _require_4d(voxelgrids)
    iso_value = _check_iso(iso_value)
    B, X, Y, Z = voxelgrids.shape
    lattice = (X + 1) * (Y + 1) * (Z + 1)
    if min(X, Y, Z) < 1 and B > 0:
        raise ValueError(f'Expected X, Y, Z >= 1, but got a grid of {X} x {Y} x {Z}')
    if 3 * lattice >= 2 ** 31:
        raise ValueError(f'the lattice (X + 1)(Y + 1)(Z + 1) = {lattice} holds up to {3 * lattice} vertices: '
                         'more than 32-bit indices cover')
    if B == 0:
        return [], []
    needs_grad = voxelgrids.is_floating_point() and voxelgrids.requires_grad and torch.is_grad_enabled()
    if not needs_grad:
        voxelgrids = voxelgrids.detach()
    if voxelgrids.is_cuda:
        if not needs_grad:
            return _C.ops.conversions.voxelgrids_to_trianglemeshes_cuda(voxelgrids, iso_value)
        if voxelgrids.dtype not in (torch.float16, torch.float32):
            voxelgrids = voxelgrids.float()
        verts, faces, nv, nf = _MarchingCubes.apply(voxelgrids, iso_value)
    else:
        verts, faces, nv, nf = _trianglemeshes_torch(F.pad(voxelgrids.float(), (1, 1, 1, 1, 1, 1)), iso_value)
    return list(torch.split(verts, nv)), list(torch.split(faces, nf))
