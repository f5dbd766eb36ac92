"""``subdivide_trianglemesh``: Loop subdivision with a learnable per-vertex smoothing factor (API mirror of
kaolin/ops/mesh/trianglemesh.py) -- the third stage of the DMTet loop, after ``ops.conversions.marching_tetrahedra`` and next to
``ops.mesh.subdivide_tetmesh``.

One iteration, for V vertices and the faces ``(a, b, c)``.  The edge slots of a face are ab, bc, ca, with the opposite corners
c, a, b; an edge is the pair (min, max) of its ends (a repeated corner gives a self-edge, an edge like any other); the E unique
edges are numbered in ascending (min, max) order and edge e becomes the new vertex ``V + e``.  ``count[e]`` is the number of face
slots holding edge e, ``n[v]`` the number of unique edges holding v (a self-edge counts once; the neighbour sum then includes
``x[v]``).

    old vertex v      (1 - alpha[v]) x[v] + alpha[v] / n[v] * sum of x[u] over the neighbours u; alpha[v] given and carried over
                      the iterations, or in every iteration 5/8 - (3/8 + cos(2 pi / n) / 4)^2 (9/16 at n = 3); a vertex no face
                      uses (n = 0) keeps its position and its alpha
    edge e, for the   count[e] == 2: (3 (x[lo] + x[hi]) + (x[opp0] + x[opp1])) / 8, the two opposite corners added to each other
    channels x y z    first; any other count (boundary, non-manifold): (x[lo] + x[hi]) / 2
    and alpha
    new faces         four consecutive rows per face, CHILD_FACES below

float32 / float64 CUDA tensors with int64 faces run the HIP pipeline of csrc/subdivide_trianglemesh.hip; everything else (CPU
tensors, half, mixed dtypes or devices, int32 faces) runs the torch formulation below, which mirrors that pipeline: one 64-bit key
``min << 32 | max`` per edge slot, ``torch.unique`` on the keys alone, ``index_add_`` of the opposite corners, ``where`` on
``count == 2``, and the neighbour sums as the run of edges with min = v followed by the run with max = v.
"""
import math

import torch
from torch.autograd.function import once_differentiable

from ... import _C
from .vertex_features import vertex_tangents  # noqa: F401  (the reference keeps it in trianglemesh.py)

__all__ = ['subdivide_trianglemesh', 'vertex_tangents']

# The four children of a face, in order; `xy` is the new vertex of the edge slot xy.  csrc/subdivide_trianglemesh.hip spells out
# the same rows.  CHILD_FACES holds them as columns of (a, b, c, ab, bc, ca).
_COLUMNS = ('a', 'b', 'c', 'ab', 'bc', 'ca')
CHILD_FACES = tuple(tuple(_COLUMNS.index(name) for name in row.split()) for row in ('b bc ab', 'a ab ca', 'c ca bc', 'ca ab bc'))


def _torch_topology(faces, num_vertices):
    """-> new_faces (4 F, 3) and what the values need: lo, hi (E) the ends of the unique edges in ascending order; proper (E) bool,
    lo != hi; slot_edge, slot_opp (3 F) the edge and the opposite corner of every face slot; two (E) bool, count == 2; valence (V)"""
    f = faces.long()
    a, b, c = f.unbind(1)
    p, q, opp = torch.stack((a, b, c), dim=1), torch.stack((b, c, a), dim=1), torch.stack((c, a, b), dim=1)
    keys = (torch.minimum(p, q) << 32) | torch.maximum(p, q)
    unique_keys, inverse, counts = torch.unique(keys, return_inverse=True, return_counts=True)   # ascending (min, max)
    lo, hi = unique_keys >> 32, unique_keys & 0xffffffff
    columns = torch.cat((f, inverse + num_vertices), dim=1)                                     # (F, 6)
    new_faces = columns[:, torch.tensor(CHILD_FACES, device=f.device)].reshape(-1, 3)
    proper = lo != hi
    valence = torch.bincount(lo, minlength=num_vertices) + torch.bincount(hi[proper], minlength=num_vertices)
    return new_faces, (lo, hi, proper, inverse.reshape(-1), opp.reshape(-1), counts == 2, valence)


def _default_alpha(n):
    """The Loop weights of the valences n (a float tensor, n >= 1)"""
    alpha = 0.625 - (0.375 + 0.25 * torch.cos(2 * math.pi / n)) ** 2
    return torch.where(n == 3, torch.full_like(alpha, 0.5625), alpha)


def _torch_iteration(vertices, faces, alpha):
    """One iteration in torch: vertices (B, V, 3), faces (F, 3), alpha (B, V) or None -> new_vertices, new_faces, new_alpha"""
    num_vertices = vertices.shape[1]
    with torch.no_grad():
        new_faces, (lo, hi, proper, slot_edge, slot_opp, two, valence) = _torch_topology(faces, num_vertices)
        used = (valence > 0)[None, :, None]
        n = valence.clamp(min=1).to(vertices.dtype)
        lo_proper, hi_proper = lo[proper], hi[proper]
    a = _default_alpha(n)[None, :, None] if alpha is None else alpha.unsqueeze(-1)
    # the neighbours of v: the max ends of the edges with min = v (one run of the edge list), then the min ends of the edges with
    # max = v (one run of the transposed list; the self-edge is in the first run already)
    neighbours = torch.zeros_like(vertices)
    neighbours.index_add_(1, lo, vertices.index_select(1, hi))
    neighbours.index_add_(1, hi_proper, vertices.index_select(1, lo_proper))
    moved = (1 - a) * vertices + a / n[None, :, None] * neighbours
    old_rows = torch.where(used, moved, vertices)
    x = vertices if alpha is None else torch.cat((vertices, alpha.unsqueeze(-1)), dim=2)
    ends = x.index_select(1, lo) + x.index_select(1, hi)
    far = torch.zeros_like(ends).index_add_(1, slot_edge, x.index_select(1, slot_opp))
    edge_rows = torch.where(two[None, :, None], (ends * 3 + far) * 0.125, ends * 0.5)
    new_vertices = torch.cat((old_rows, edge_rows[..., :3]), dim=1)
    new_alpha = None if alpha is None else torch.cat((alpha, edge_rows[..., 3]), dim=1)
    return new_vertices, new_faces, new_alpha


class _LoopIteration(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, faces, alpha):
        new_faces, topo = _C.ops.mesh.subdivide_trianglemesh_cuda(faces, vertices.shape[1], check_faces=False)
        new_vertices, new_alpha = _C.ops.mesh.trianglemesh_loop_forward_cuda(vertices, alpha, topo)
        ctx.save_for_backward(vertices, alpha, *topo)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(new_faces)
        return new_vertices, new_faces, new_alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_new_vertices, _, grad_new_alpha=None):
        vertices, alpha, *topo = ctx.saved_tensors
        alpha_needs_grad = alpha is not None and ctx.needs_input_grad[2]
        if (grad_new_vertices is None and grad_new_alpha is None) or not (ctx.needs_input_grad[0] or alpha_needs_grad):
            return None, None, None
        if grad_new_vertices is None:
            grad_new_vertices = grad_new_alpha.new_zeros(grad_new_alpha.shape + (3,))
        grad_vertices, grad_alpha = _C.ops.mesh.trianglemesh_loop_backward_cuda(grad_new_vertices, grad_new_alpha, vertices, alpha,
                                                                                tuple(topo), alpha_needs_grad)
        return grad_vertices, None, grad_alpha


def _check_arguments(vertices, faces, iterations, alpha):
    """The reference checks nothing; what it raises for ill-shaped arguments comes out of its indexing.  The meaningful ones keep
    their type and text, raised up front; the rest are this module's own."""
    if vertices.dim() != 3 or vertices.shape[2] != 3:
        raise RuntimeError(f'vertices must of size {{batch_size, num_vertices, 3}}, but got {list(vertices.shape)}')
    if faces.dim() == 1:
        raise IndexError('too many indices for tensor of dimension 1')
    if faces.dtype.is_floating_point or faces.dtype.is_complex or faces.dtype == torch.bool:
        raise RuntimeError('indices must be an int64 tensor')
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise RuntimeError(f'faces must of size {{num_faces, 3}}, but got {list(faces.shape)}')
    if alpha is not None:
        batch_size, num_vertices = vertices.shape[:2]
        if not (alpha.dim() in (2, 3) and tuple(alpha.shape[:2]) == (batch_size, num_vertices) and (alpha.dim() == 2 or alpha.shape[2] == 1)):
            raise RuntimeError(f'alpha must of size {{batch_size, num_vertices}} or {{batch_size, num_vertices, 1}} = '
                               f'{{{batch_size}, {num_vertices}}}, but got {list(alpha.shape)}')
        if not alpha.dtype.is_floating_point:
            raise RuntimeError(f'alpha must be of a floating-point type, but got {alpha.dtype}')
    if not isinstance(iterations, int) or isinstance(iterations, bool):
        raise TypeError(f"'{type(iterations).__name__}' object cannot be interpreted as an integer")


def subdivide_trianglemesh(vertices, faces, iterations, alpha=None):
    r"""Subdivide triangular meshes following the scheme of Loop subdivision (`Smooth Subdivision Surfaces Based on Triangles`_).
    If the smoothing factor alpha is not given, this function performs exactly as Loop subdivision.  Elsewise the vertex position
    is updated using the given per-vertex alpha value, which is differentiable and carries over to subsequent subdivision
    iterations.  Higher alpha leads to smoother surfaces, and a vertex with alpha = 0 will not change from its initial position
    during the subdivision: alpha can be learnt to preserve sharp geometric features (`Deep Marching Tetrahedra`_, NeurIPS 2021;
    reference: kaolin/ops/mesh/trianglemesh.py).  Differentiable in ``vertices`` and ``alpha``.

    Where this differs from the reference:

    - The reference computes in float32 only (double and half raise ``expected scalar type Float``) and only for
      ``batch_size == 1`` (its sparse ``bmm`` fails on a larger batch).  This function takes every floating-point dtype and every
      batch size and returns the dtype it was given (mixed ``vertices`` / ``alpha`` dtypes promote).
    - A vertex that no face uses keeps its position and its alpha; the reference returns NaN for it.
    - ``faces`` that are not triangles, and an ``alpha`` whose size does not match ``vertices``, raise RuntimeError (the reference
      silently mis-handles quads).

    float32 / float64 CUDA tensors (int64 ``faces``, ``alpha`` of the dtype of ``vertices``) run hand-written HIP kernels.  The
    number of new vertices depends on the data, so every iteration reads one count back: it synchronises the current stream once
    per iteration and cannot be captured in a graph -- as the reference, whose ``torch.unique`` synchronises too.  The forward
    uses no floating-point atomics: two calls on the same input return the same bits.  Every other input runs in torch.  An
    entry of ``faces`` outside ``[0, num_vertices)`` raises IndexError.

    Args:
        vertices (torch.Tensor): batched vertices of triangle meshes, of shape
                                 :math:`(\text{batch_size}, \text{num_vertices}, 3)`.
        faces (torch.LongTensor): unbatched triangle mesh faces, of shape :math:`(\text{num_faces}, 3)`.
        iterations (int): number of subdivision iterations.
        alpha (optional, torch.Tensor): batched per-vertex smoothing factor, alpha, of shape
                            :math:`(\text{batch_size}, \text{num_vertices})` or :math:`(\text{batch_size}, \text{num_vertices}, 1)`.

    Returns:
        (torch.Tensor, torch.LongTensor):

        - batched vertices of triangle meshes, of shape :math:`(\text{batch_size}, \text{new_num_vertices}, 3)`.
        - unbatched triangle mesh faces, of shape :math:`(\text{num_faces} \cdot 4^\text{iterations}, 3)`.

    Example:
        >>> vertices = torch.tensor([[[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]], dtype=torch.float)
        >>> faces = torch.tensor([[0, 1, 2], [0, 1, 3], [0, 2, 3], [1, 2, 3]], dtype=torch.long)
        >>> alpha = torch.tensor([[0, 0, 0, 0]], dtype=torch.float)
        >>> new_vertices, new_faces = subdivide_trianglemesh(vertices, faces, 1, alpha)
        >>> new_vertices
        tensor([[[0.0000, 0.0000, 0.0000],
                 [1.0000, 0.0000, 0.0000],
                 [0.0000, 1.0000, 0.0000],
                 [0.0000, 0.0000, 1.0000],
                 [0.3750, 0.1250, 0.1250],
                 [0.1250, 0.3750, 0.1250],
                 [0.1250, 0.1250, 0.3750],
                 [0.3750, 0.3750, 0.1250],
                 [0.3750, 0.1250, 0.3750],
                 [0.1250, 0.3750, 0.3750]]])
        >>> new_faces[:4]
        tensor([[1, 7, 4],
                [0, 4, 5],
                [2, 5, 7],
                [5, 4, 7]])

    .. _Smooth Subdivision Surfaces Based on Triangles:
            https://www.microsoft.com/en-us/research/wp-content/uploads/2016/02/thesis-10.pdf

    .. _Deep Marching Tetrahedra: https://arxiv.org/abs/2111.04276
    """
    _check_arguments(vertices, faces, iterations, alpha)
    if iterations <= 0:
        return vertices, faces
    if faces.shape[0] == 0:
        return vertices, torch.empty((0, 3), dtype=torch.long, device=faces.device)
    _C.ops.check_faces_in_range(faces, vertices.shape[1], 'subdivide_trianglemesh')   # once: the later faces are made here
    if alpha is not None:
        alpha = alpha.reshape(alpha.shape[:2])
    hip = (vertices.is_cuda and faces.is_cuda and faces.device == vertices.device and faces.dtype == torch.long and
           vertices.dtype in (torch.float32, torch.float64) and
           (alpha is None or (alpha.dtype == vertices.dtype and alpha.device == vertices.device)))
    if not hip:
        faces = faces.to(vertices.device)
        if alpha is not None:
            alpha = alpha.to(vertices.device, torch.promote_types(vertices.dtype, alpha.dtype))
            vertices = vertices.to(alpha.dtype)
    for _ in range(iterations):
        if hip:
            vertices, faces, alpha = _LoopIteration.apply(vertices, faces, alpha)
        else:
            vertices, faces, alpha = _torch_iteration(vertices, faces, alpha)
    return vertices, faces
