"""``marching_tetrahedra`` (API mirror of kaolin/ops/conversions/tetmesh.py): the zero level set of a signed-distance field
given on the vertices of a tetrahedral grid, as a triangle mesh, differentiable in the grid's vertex positions and sdf values.

A vertex is occupied when ``sdf > 0``.  A tet with 1 to 3 occupied corners is cut by the surface: it emits one triangle (1 or 3
corners) or two (2 corners), whose corners lie on its crossing edges (exactly one end occupied).  Output vertices are the
unique crossing edges {a < b} in ascending (a, b) order; faces are the one-triangle tets' in tet order, then the two-triangle
tets' in tet order.

float32 / float64 CUDA tensors with int64 tets run the HIP pipeline of csrc/marching_tetrahedra.hip; everything else (CPU
tensors, half, mixed dtypes, int32 tets) runs the torch formulation below, which mirrors that pipeline: one 64-bit key
``a << 32 | b`` per crossing edge, ``torch.unique`` on the keys alone, ``torch.searchsorted`` for each edge's rank.
"""
import torch
from torch.autograd.function import once_differentiable

from ... import _C

__all__ = ['marching_tetrahedra']

# The six edge slots of a tet: the pairs of its corners.
EDGE_CORNERS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
# sign case (sum of occupied(corner k) << k) -> the edge slots of its triangles' corners (3 per triangle; cases with one
# triangle are padded with slot 0).  Which slots, in which order, is the reference's behaviour: this table was built from its
# answers for the 16 sign patterns of a single tet (tests/golden/marching_tetrahedra.npz, `cases16`), and
# tests/test_marching_tetrahedra_cpu.py rebuilds it from that record.  csrc/marching_tetrahedra.hip holds the same table.
TRIANGLE_SLOTS = (
    (0, 0, 0, 0, 0, 0), (1, 0, 2, 0, 0, 0), (4, 0, 3, 0, 0, 0), (1, 4, 2, 1, 3, 4), (3, 1, 5, 0, 0, 0), (2, 3, 0, 2, 5, 3),
    (1, 4, 0, 1, 5, 4), (4, 2, 5, 0, 0, 0), (4, 5, 2, 0, 0, 0), (4, 1, 0, 4, 5, 1), (3, 2, 0, 3, 5, 2), (1, 3, 5, 0, 0, 0),
    (4, 1, 2, 4, 3, 1), (3, 0, 4, 0, 0, 0), (2, 0, 1, 0, 0, 0), (0, 0, 0, 0, 0, 0))
NUM_TRIANGLES = tuple((0, 1, 2, 1, 0)[bin(case).count('1')] for case in range(16))


def _torch_unbatched(vertices, tets, sdf, return_tet_idx):
    device = vertices.device
    with torch.no_grad():
        tets = tets.long()
        slot_a = torch.tensor([e[0] for e in EDGE_CORNERS], device=device)
        slot_b = torch.tensor([e[1] for e in EDGE_CORNERS], device=device)
        occupied = (sdf > 0)[tets]                                                    # (T, 4)
        case = (occupied.long() << torch.arange(4, device=device)).sum(-1)
        num_tri = torch.tensor(NUM_TRIANGLES, device=device)[case]
        valid = torch.nonzero(num_tri > 0).reshape(-1)                                # the surface tets, ascending
        case, num_tri, corners = case[valid], num_tri[valid], tets[valid]
        ea, eb = corners[:, slot_a], corners[:, slot_b]                               # (Nt, 6): the ends of every edge slot
        keys = (torch.minimum(ea, eb) << 32) | torch.maximum(ea, eb)
        crossing = (((case.unsqueeze(1) >> slot_a) ^ (case.unsqueeze(1) >> slot_b)) & 1).bool()
        unique_keys = torch.unique(keys[crossing])                                    # ascending (a, b): the vertex list
        a, b = unique_keys >> 32, unique_keys & 0xffffffff
        rank = torch.searchsorted(unique_keys, keys)                                  # (meaningful on the crossing slots)
        table = torch.tensor(TRIANGLE_SLOTS, device=device)
        one, two = num_tri == 1, num_tri == 2
        faces = torch.cat((torch.gather(rank[one], 1, table[case[one]][:, :3]),
                           torch.gather(rank[two], 1, table[case[two]]).reshape(-1, 3)), dim=0)
    sa, nsb = sdf.index_select(0, a).unsqueeze(1), -sdf.index_select(0, b).unsqueeze(1)
    verts = (vertices.index_select(0, a) * nsb + vertices.index_select(0, b) * sa) / (sa + nsb)
    if return_tet_idx:
        return verts, faces, torch.cat((valid[one], valid[two].repeat_interleave(2)), dim=0)
    return verts, faces


class _MarchingTetrahedra(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, sdf, tets, return_tet_idx):
        out = _C.ops.conversions.marching_tetrahedra_cuda(vertices, tets, sdf, return_tet_idx)
        verts, faces, edges = out[:3]
        ctx.save_for_backward(vertices, sdf, edges)
        ctx.mark_non_differentiable(faces, *out[3:])
        return (verts, faces) + tuple(out[3:])

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_verts, *_):
        vertices, sdf, edges = ctx.saved_tensors
        grad_vertices, grad_sdf = _C.ops.conversions.marching_tetrahedra_backward_cuda(grad_verts, vertices, sdf, edges)
        return grad_vertices, grad_sdf, None, None


def _check_arguments(vertices, tets, sdf):
    """The reference checks nothing; what it raises for ill-shaped arguments comes out of its indexing.  The same types and
    texts, raised up front."""
    batch_size = vertices.shape[0]
    if sdf.dim() >= 1 and sdf.shape[0] < batch_size:
        raise IndexError(f'index {sdf.shape[0]} is out of bounds for dimension 0 with size {sdf.shape[0]}')
    if tets.dtype.is_floating_point or tets.dtype.is_complex:
        raise IndexError('tensors used as indices must be long, int, byte or bool tensors')
    if sdf.dim() == 1:
        raise IndexError('too many indices for tensor of dimension 0')
    if tets.dim() != 2 or tets.shape[1] != 4:
        raise RuntimeError(f"shape '[-1, 4]' is invalid for input of size {tets.numel()}")
    if vertices.dim() != 3 or vertices.shape[2] != 3:
        raise RuntimeError(f'vertices must of size {{batch_size, num_vertices, 3}}, but got {list(vertices.shape)}')
    if sdf.dim() != 2 or sdf.shape[1] != vertices.shape[1]:
        raise RuntimeError(f'sdf must of size {{batch_size, num_vertices}}, but got {list(sdf.shape)}')


def marching_tetrahedra(vertices, tets, sdf, return_tet_idx=False):
    r"""Convert discrete signed distance fields encoded on tetrahedral grids to triangle meshes with the marching tetrahedra
    algorithm.  The output surface is differentiable with respect to the input vertex positions and the SDF values
    (reference: kaolin/ops/conversions/tetmesh.py).

    float32 / float64 CUDA tensors (int64 ``tets``) run hand-written HIP kernels.  The sizes of the results depend on the
    data, so the call reads two counts back per batch item: it synchronises the current stream and cannot be captured in a
    graph -- as the reference, whose ``torch.unique`` and mask indexing synchronise too.  Every other input runs in torch.
    An entry of ``tets`` outside ``[0, num_vertices)`` raises IndexError.

    Args:
        vertices (torch.Tensor): batched vertices of tetrahedral meshes, of shape
                                 :math:`(\text{batch_size}, \text{num_vertices}, 3)`.
        tets (torch.Tensor): unbatched tetrahedral mesh topology, of shape :math:`(\text{num_tetrahedrons}, 4)`.
        sdf (torch.Tensor): batched SDFs which specify the SDF value of each vertex, of shape
                            :math:`(\text{batch_size}, \text{num_vertices})`.
        return_tet_idx (optional, bool): if True, return index of tetrahedron where each face is extracted. Default: False.

    Returns:
        (list[torch.Tensor], list[torch.LongTensor], (optional) list[torch.LongTensor]):

            - the vertices of the mesh extracted from each tetrahedral grid, each of shape (num_verts, 3).
            - the faces of the mesh extracted from each tetrahedral grid, each of shape (num_faces, 3).
            - the indices of the tetrahedra the faces are extracted from, each of shape (num_faces).

    Example:
        >>> vertices = torch.tensor([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]], dtype=torch.float)
        >>> tets = torch.tensor([[0, 1, 2, 3]], dtype=torch.long)
        >>> sdf = torch.tensor([[-1., -1., 0.5, 0.5]], dtype=torch.float)
        >>> verts_list, faces_list, tet_idx_list = marching_tetrahedra(vertices, tets, sdf, True)
        >>> verts_list[0]
        tensor([[0.0000, 0.6667, 0.0000],
                [0.0000, 0.0000, 0.6667],
                [0.3333, 0.6667, 0.0000],
                [0.3333, 0.0000, 0.6667]])
        >>> faces_list[0]
        tensor([[3, 0, 1],
                [3, 2, 0]])
        >>> tet_idx_list[0]
        tensor([0, 0])
    """
    if vertices.shape[0] == 0:
        return []
    _check_arguments(vertices, tets, sdf)
    hip = (vertices.is_cuda and sdf.is_cuda and tets.is_cuda and tets.dtype == torch.long and
           vertices.dtype == sdf.dtype and vertices.dtype in (torch.float32, torch.float64))
    if hip:
        outputs = [_MarchingTetrahedra.apply(vertices[b], sdf[b], tets, return_tet_idx) for b in range(vertices.shape[0])]
    else:
        _C.ops.check_tets_in_range(tets, vertices.shape[1])      # (the HIP shim makes the same check, per item)
        outputs = [_torch_unbatched(vertices[b], tets, sdf[b], return_tet_idx) for b in range(vertices.shape[0])]
    return list(zip(*outputs))
