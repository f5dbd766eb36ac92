"""``subdivide_tetmesh`` and ``inverse_vertices_offset`` (API mirror of kaolin/ops/mesh/tetmesh.py).

``subdivide_tetmesh`` splits every tetrahedron into eight through the midpoints of its six edges -- the other half of the DMTet
loop next to ``ops.conversions.marching_tetrahedra``.  The six edge slots of a tet ``(a, b, c, d)`` are ab, ac, ad, bc, bd, cd; an
edge is the pair (min, max) of its ends (a repeated corner gives a self-edge, an edge like any other); the E unique edges are
numbered in ascending (min, max) order and edge e becomes the new vertex ``V + e``, at ``(x[min] + x[max]) * 0.5``.  The new
topology is eight blocks of T rows in tet order, ``CHILD_TETS`` below.

float32 / float64 CUDA tensors with int64 tetrahedrons run the HIP pipeline of csrc/subdivide_tetmesh.hip; everything else (CPU
tensors, half, mixed dtypes, int32 tetrahedrons) runs the torch formulation below, which mirrors that pipeline: one 64-bit key
``min << 32 | max`` per edge slot, ``torch.unique`` on the keys alone, ``torch.searchsorted`` for each slot's rank.
"""
import torch
from torch.autograd.function import once_differentiable

from ... import _C

__all__ = ['subdivide_tetmesh', 'inverse_vertices_offset']

# The six edge slots of a tet: the pairs of its corners.
EDGE_CORNERS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# The eight children of a tet, block by block; `xy` is the new vertex of the edge slot xy.  csrc/subdivide_tetmesh.hip spells out
# the same rows.  CHILD_TETS holds them as columns of (a, b, c, d, ab, ac, ad, bc, bd, cd).
_COLUMNS = ('a', 'b', 'c', 'd', 'ab', 'ac', 'ad', 'bc', 'bd', 'cd')
CHILD_TETS = tuple(tuple(_COLUMNS.index(name) for name in row.split()) for row in (
    'a ab ac ad', 'b bc ab bd', 'c ac bc cd', 'd ad cd bd', 'ab ac ad bd', 'ab ac bd bc', 'cd ac bd ad', 'cd ac bc bd'))


def _validate_tet_vertices(tet_vertices):
    assert tet_vertices.ndim == 4, \
        f"tetrahedrons has {tet_vertices.ndim} but must have 4 dimensions."
    assert tet_vertices.shape[2] == 4, \
        f"The third dimension of the tetrahedrons must be 4 " \
        f"but the input has {tet_vertices.shape[2]}. Each tetrahedron has 4 vertices."
    assert tet_vertices.shape[3] == 3, \
        f"The fourth dimension of the tetrahedrons must be 3 " \
        f"but the input has {tet_vertices.shape[3]}. Each vertex must have 3 dimensions."


def inverse_vertices_offset(tet_vertices):
    r"""Given tetrahedrons with 4 vertices A, B, C, D, compute the inverse of the offset matrix w.r.t. vertex A of each
    tetrahedron: the rows :math:`B - A`, :math:`C - A` and :math:`D - A`, inverted (reference: kaolin/ops/mesh/tetmesh.py).
    Plain torch on every device.

    Args:
        tet_vertices (torch.Tensor): batched tetrahedrons, of shape :math:`(\text{batch_size}, \text{num_tetrahedrons}, 4, 3)`.

    Returns:
        (torch.Tensor): batched inverse offset matrix, of shape :math:`(\text{batch_size}, \text{num_tetrahedrons}, 3, 3)`.

    Example:
        >>> tet_vertices = torch.tensor([[[[-0.0500,  0.0000,  0.0500],
        ...                                [-0.0250, -0.0500,  0.0000],
        ...                                [ 0.0000,  0.0000,  0.0500],
        ...                                [0.5000, 0.5000, 0.4500]]]])
        >>> inverse_vertices_offset(tet_vertices)
        tensor([[[[   0.0000,   20.0000,    0.0000],
                  [  79.9999, -149.9999,   10.0000],
                  [ -99.9999,  159.9998,  -10.0000]]]])
    """
    _validate_tet_vertices(tet_vertices)
    return torch.inverse(tet_vertices[:, :, 1:] - tet_vertices[:, :, :1])


def _torch_subdivide(vertices, tetrahedrons, features):
    device = vertices.device
    num_vertices = vertices.shape[1]
    if features is not None:                       # the reference concatenates the two: both results take the promoted type
        dtype = torch.promote_types(vertices.dtype, features.dtype)
        vertices, features = vertices.to(dtype), features.to(dtype)
    with torch.no_grad():
        tets = tetrahedrons.long()
        slot_a = torch.tensor([e[0] for e in EDGE_CORNERS], device=device)
        slot_b = torch.tensor([e[1] for e in EDGE_CORNERS], device=device)
        ea, eb = tets[:, slot_a], tets[:, slot_b]                                     # (T, 6): the ends of every edge slot
        keys = (torch.minimum(ea, eb) << 32) | torch.maximum(ea, eb)
        unique_keys = torch.unique(keys)                                              # ascending (min, max): the edge list
        lo, hi = unique_keys >> 32, unique_keys & 0xffffffff
        rank = torch.searchsorted(unique_keys, keys) + num_vertices
        columns = torch.cat((tets, rank), dim=1)                                      # (T, 10)
        children = torch.tensor(CHILD_TETS, device=device)
        new_tets = columns[:, children].permute(1, 0, 2).reshape(-1, 4)

    def midpoints(x):
        return torch.cat((x, (x.index_select(1, lo) + x.index_select(1, hi)) * 0.5), dim=1)

    if features is None:
        return midpoints(vertices), new_tets
    return midpoints(vertices), new_tets, midpoints(features)


class _SubdivideTetmesh(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, tetrahedrons, features):
        edges, new_tets = _C.ops.mesh.subdivide_tetmesh_cuda(tetrahedrons, vertices.shape[1])
        new_vertices, new_features = _C.ops.mesh.tetmesh_midpoints_forward_cuda(vertices, features, edges, check_edges=False)
        ctx.save_for_backward(edges)
        ctx.num_vertices = vertices.shape[1]
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(new_tets)
        return (new_vertices, new_tets) if features is None else (new_vertices, new_tets, new_features)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_new_vertices, _, grad_new_features=None):
        edges, = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            grad_new_vertices = None
        if not ctx.needs_input_grad[2]:
            grad_new_features = None
        if grad_new_vertices is None and grad_new_features is None:
            return None, None, None
        grad_vertices, grad_features = _C.ops.mesh.tetmesh_midpoints_backward_cuda(grad_new_vertices, grad_new_features, edges,
                                                                                   ctx.num_vertices, check_edges=False)
        return grad_vertices, None, grad_features


def _check_arguments(vertices, tetrahedrons, features):
    """The reference checks nothing; what it raises for ill-shaped arguments comes out of its indexing and its ``cat``.  The
    same types and texts, raised up front."""
    if tetrahedrons.dim() == 2 and tetrahedrons.shape[1] < 4:
        raise IndexError(f'index 3 is out of bounds for dimension 0 with size {tetrahedrons.shape[1]}')
    if features is not None and features.dim() == vertices.dim() == 3 and features.shape[1] != vertices.shape[1]:
        raise RuntimeError(f'Sizes of tensors must match except in dimension 2. Expected size {vertices.shape[1]} but got size '
                           f'{features.shape[1]} for tensor number 1 in the list.')
    if tetrahedrons.dtype.is_floating_point or tetrahedrons.dtype.is_complex:
        raise IndexError('tensors used as indices must be long, int, byte or bool tensors')
    if vertices.dim() != 3 or vertices.shape[2] != 3:
        raise RuntimeError(f'vertices must of size {{batch_size, num_vertices, 3}}, but got {list(vertices.shape)}')
    if tetrahedrons.dim() != 2 or tetrahedrons.shape[1] != 4:
        raise RuntimeError(f'tetrahedrons must of size {{num_tetrahedrons, 4}}, but got {list(tetrahedrons.shape)}')
    if features is not None and (features.dim() != 3 or features.shape[0] != vertices.shape[0]):
        raise RuntimeError(f'features must of size {{batch_size, num_vertices, feature_dim}}, but got {list(features.shape)}')


def subdivide_tetmesh(vertices, tetrahedrons, features=None):
    r"""Subdivide each tetrahedron in tetmesh into 8 smaller tetrahedrons by adding midpoints.  If per-vertex features (e.g. SDF
    value) are given, the features of the new vertices are computed by averaging the features of vertices on the edge
    (reference: kaolin/ops/mesh/tetmesh.py; `Deep Marching Tetrahedra`_, NeurIPS 2021).  Differentiable in ``vertices`` and
    ``features``.

    float32 / float64 CUDA tensors (int64 ``tetrahedrons``) run hand-written HIP kernels.  The number of new vertices depends on
    the data, so the call reads one count back: it synchronises the current stream once and cannot be captured in a graph -- as
    the reference, whose ``torch.unique`` synchronises too.  Every other input runs in torch.  An entry of ``tetrahedrons``
    outside ``[0, num_vertices)`` raises IndexError.

    Args:
        vertices (torch.Tensor): batched vertices of tetrahedral meshes, of shape
                                 :math:`(\text{batch_size}, \text{num_vertices}, 3)`.
        tetrahedrons (torch.LongTensor): unbatched tetrahedral mesh topology, of shape :math:`(\text{num_tetrahedrons}, 4)`.
        features (optional, torch.Tensor): batched per-vertex feature vectors, of shape
                                 :math:`(\text{batch_size}, \text{num_vertices}, \text{feature_dim})`.

    Returns:
        (torch.Tensor, torch.LongTensor, (optional) torch.Tensor):

        - batched vertices of subdivided tetrahedral meshes, of shape :math:`(\text{batch_size}, \text{new_num_vertices}, 3)`
        - unbatched tetrahedral mesh topology, of shape :math:`(\text{num_tetrahedrons} * 8, 4)`.
        - batched per-vertex feature vectors of subdivided tetrahedral meshes, of shape
          :math:`(\text{batch_size}, \text{new_num_vertices}, \text{feature_dim})`.

    Example:
        >>> vertices = torch.tensor([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]], dtype=torch.float)
        >>> tetrahedrons = torch.tensor([[0, 1, 2, 3]], dtype=torch.long)
        >>> sdf = torch.tensor([[[-1.], [-1.], [0.5], [0.5]]], dtype=torch.float)
        >>> new_vertices, new_tetrahedrons, new_sdf = subdivide_tetmesh(vertices, tetrahedrons, sdf)
        >>> new_vertices
        tensor([[[0.0000, 0.0000, 0.0000],
                 [1.0000, 0.0000, 0.0000],
                 [0.0000, 1.0000, 0.0000],
                 [0.0000, 0.0000, 1.0000],
                 [0.5000, 0.0000, 0.0000],
                 [0.0000, 0.5000, 0.0000],
                 [0.0000, 0.0000, 0.5000],
                 [0.5000, 0.5000, 0.0000],
                 [0.5000, 0.0000, 0.5000],
                 [0.0000, 0.5000, 0.5000]]])
        >>> new_tetrahedrons
        tensor([[0, 4, 5, 6],
                [1, 7, 4, 8],
                [2, 5, 7, 9],
                [3, 6, 9, 8],
                [4, 5, 6, 8],
                [4, 5, 8, 7],
                [9, 5, 8, 6],
                [9, 5, 7, 8]])
        >>> new_sdf[0, 4:, 0]
        tensor([-1.0000, -0.2500, -0.2500, -0.2500, -0.2500,  0.5000])

    .. _Deep Marching Tetrahedra: https://arxiv.org/abs/2111.04276
    """
    _check_arguments(vertices, tetrahedrons, features)
    hip = (vertices.is_cuda and tetrahedrons.is_cuda and tetrahedrons.device == vertices.device and
           tetrahedrons.dtype == torch.long and vertices.dtype in (torch.float32, torch.float64) and
           (features is None or (features.dtype == vertices.dtype and features.device == vertices.device)))
    if hip:
        return _SubdivideTetmesh.apply(vertices, tetrahedrons, features)
    _C.ops.check_tets_in_range(tetrahedrons, vertices.shape[1], 'subdivide_tetmesh')  # (the HIP shim makes the same check)
    return _torch_subdivide(vertices, tetrahedrons, features)
