"""Voxelgrid conversions behind the API of kaolin/ops/conversions/voxelgrid.py: ``voxelgrids_to_cubic_meshes`` (Mesh R-CNN's
"Cubify"), same signature, default, result dtypes and orders.

The reference finds the faces with a ``conv3d`` and a ``nonzero`` and merges the corners with one ``torch.unique(dim=0)`` per
item -- a lexicographic sort of 4 F float rows.  No sort is needed: every vertex is a point of the (X+1)(Y+1)(Z+1) integer
lattice, so lattice order is "unique, sorted", a vertex's id is a prefix count of a flag over the lattice, and the reference's
face order (axis, then raster order of the face's location) is a prefix count too.  On a GPU tensor that pipeline runs as HIP
kernels (kaolin_amd/csrc/cubic_meshes.hip); on the CPU it is the same pipeline in plain torch (flags, ``cumsum``, gathers),
which is also the readable definition.

``voxelgrids_to_trianglemeshes`` (marching cubes) is not provided.
"""
import torch
import torch.nn.functional as F

from ... import _C
from ..voxelgrid import _require_4d

__all__ = ['voxelgrids_to_cubic_meshes']


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
