"""Face areas and uniform surface sampling of triangle meshes: ``face_areas``, ``packed_face_areas``, ``sample_points``,
``packed_sample_points`` (API mirror of kaolin/ops/mesh/trianglemesh.py:98-311) -- the step between an extracted mesh and the point
cloud a chamfer loss compares.

The contract of both paths (DESIGN.md "ops.mesh.sample_points" has the reasons):

* areas: the reference's expression in its order, one rounding per operation and a correctly rounded square root: the HIP result
  carries the bits of the torch expression on the CPU wherever torch's CPU ``sqrt`` is correctly rounded (built on MKL's vector
  maths it is one unit in the last place off for about 0.6 % of its arguments, float and double; the same holds for the
  ``sqrt(uv0)`` of the blend);
* random numbers: ``sample_points`` draws ``r = torch.rand((B, N), dtype=float64)`` and then ``uv = torch.rand((B, N, 2),
  dtype=vertices.dtype)`` from torch's default generator on the device of ``vertices``, whether ``areas`` is given or not.
  Everything after the draws is a deterministic function of (vertices, faces, areas, face_features, r, uv):
  ``_C.ops.mesh.sample_points_forward_cuda`` on the GPU, :func:`sample_points_torch` elsewhere.  THE SAMPLES OF A SEED ARE NOT THE
  REFERENCE'S: its ``Categorical.sample`` / ``multinomial`` stream is no contract;
* face choice: ``cdf`` = the inclusive float64 sums of an item's areas, ``total = cdf[-1]``, ``t = min(r total,
  nextbelow(total))``, the first face with ``cdf[f] > t``: a face without area is never chosen and the index always lies inside
  the item.  An item whose total is not a positive finite number gets NaN points and features and its first face as the choice --
  no host read and no exception (the reference's ``Categorical`` raises there, through a validation that synchronises);
* points and features: ``u = sqrt(uv0)``, weights ``(1 - u, u (1 - uv1), u uv1)``, ``(w0 v0 + w1 v1) + w2 v2``;
* gradients: points in ``vertices``, features in ``face_features``, areas in ``vertices``; nothing flows through the face choice
  (so nothing through ``areas``).  The HIP backward of ``face_areas`` has no atomics and gives the same bits every run (NaN at a
  zero-area face, as the reference's autograd); the HIP backward of ``sample_points`` adds with float atomics, so those two
  gradients vary from run to run in their last bits, like the backward of ``marching_tetrahedra``.

float32 / float64 CUDA ``vertices`` of any strides with int64 CUDA ``faces`` run csrc/sample_points.hip (at most 5 launches besides
the two ``rand``, no host read once ``faces`` has been seen); CPU tensors, half / bfloat16 and other id dtypes run the torch
formulation of the same contract.  Face ids are checked once per ``faces`` tensor (the cached ``faces_in_range``: one host read for
a new tensor, none afterwards; ``IndexError``); the packed functions check their local ids against every item's vertex count with
ONE host read per call.
"""
import torch
from torch.autograd.function import once_differentiable

from ... import _C
from ..._C.render.mesh import faces_in_range
from . import vertex_features as _vf

__all__ = ['face_areas', 'packed_face_areas', 'sample_points', 'packed_sample_points']

_HIP_DTYPES = (torch.float32, torch.float64)
_INDEX_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)


# ---- the torch formulation of the contract ------------------------------------------------------------------------------------------
def _base_face_areas(v0, v1, v2, sqrt=torch.sqrt):
    """kaolin/ops/mesh/trianglemesh.py:30-40.  ``sqrt``: the tests pass a correctly rounded root; torch's CPU ``sqrt`` is off by one
    unit in the last place for about 0.6 % of its arguments where torch is built on MKL's vector maths, the HIP kernels' is not."""
    x1, x2, x3 = torch.split(v0 - v1, 1, dim=-1)
    y1, y2, y3 = torch.split(v1 - v2, 1, dim=-1)
    a = (x2 * y3 - x3 * y2) ** 2
    b = (x3 * y1 - x1 * y3) ** 2
    c = (x1 * y2 - x2 * y1) ** 2
    return sqrt(a + b + c) * 0.5


def _face_corners(vertices, faces):
    """(B, V, 3), (F, 3) -> three (B, F, 3)"""
    faces = faces.long()
    return tuple(torch.index_select(vertices, 1, faces[:, k]) for k in range(3))


def face_areas_torch(vertices, faces, sqrt=torch.sqrt):
    """(B, V, 3), (F, 3) -> (B, F): the reference's expression"""
    return _base_face_areas(*_face_corners(vertices, faces), sqrt=sqrt).squeeze(-1)


def blend_torch(w_uv, c0, c1, c2, sqrt=torch.sqrt):
    """uv (..., 2) and three corner values (..., C) -> (w0 c0 + w1 c1) + w2 c2 with the contract's weights"""
    u = sqrt(w_uv[..., 0:1])
    v = w_uv[..., 1:2]
    w0 = 1 - u
    w1 = u * (1 - v)
    w2 = u * v
    return w0 * c0 + w1 * c1 + w2 * c2


def choose_faces_torch(areas, r):
    """areas (B, F), r (B, N) float64 -> (face choices (B, N) long, live (B, 1) bool): the contract's face choice with a sequential
    float64 cumsum"""
    cdf = torch.cumsum(areas.detach().double(), dim=1)
    total = cdf[:, -1:]
    live = (total > 0) & torch.isfinite(total)
    t = torch.minimum(r.double() * total, torch.nextafter(total, torch.zeros_like(total)))
    t = torch.where(live, t, torch.zeros_like(t))
    choices = torch.searchsorted(cdf, t.contiguous(), right=True).clamp(max=areas.shape[1] - 1)
    return torch.where(live, choices, torch.zeros_like(choices)), live


def sample_points_torch(vertices, faces, areas, r, uv, face_features=None, sqrt=torch.sqrt):
    """The operator of the contract in torch, any device and float dtype: vertices (B, V, 3), faces (F, 3), areas (B, F) or None,
    r (B, N) float64, uv (B, N, 2), face_features (B, F, 3, D) or None -> (points, face_choices, features or None)"""
    corners = _face_corners(vertices, faces)
    if areas is None:
        areas = _base_face_areas(*corners, sqrt=sqrt).squeeze(-1)
    choices, live = choose_faces_torch(areas, r)
    index = choices.unsqueeze(-1).expand(-1, -1, 3)
    nan = torch.full((), float('nan'), dtype=vertices.dtype, device=vertices.device)
    points = blend_torch(uv, *(torch.gather(c, 1, index) for c in corners), sqrt=sqrt)
    points = torch.where(live.unsqueeze(-1), points, nan)
    features = None
    if face_features is not None:
        D = face_features.shape[-1]
        chosen = torch.gather(face_features, 1, choices[..., None, None].expand(-1, -1, 3, D))
        features = blend_torch(uv, chosen[:, :, 0], chosen[:, :, 1], chosen[:, :, 2], sqrt=sqrt)
        features = torch.where(live.unsqueeze(-1), features, nan)
    return points, choices, features


# ---- the HIP path -----------------------------------------------------------------------------------------------------------------
def _sum_corner_grads(corner_grads, faces, num_vertices):
    """(B, F, 3, 3) per-corner gradients -> (B, V, 3) with the deterministic sum-mode gather of vertex_features.py"""
    kernel_faces, offsets, corners = _vf._vertex_corners(faces, num_vertices)
    return _C.ops.mesh.vertex_gather_forward_cuda(corner_grads, offsets, corners, num_vertices, False)


class _FaceAreas(torch.autograd.Function):
    """items None: (B, V, 3) -> (B, F); else packed (V, 3) -> (F,), merged_faces for the backward's gather"""

    @staticmethod
    def forward(ctx, vertices, faces, items, merged_faces):
        ctx.save_for_backward(vertices, faces, merged_faces)
        ctx.items = items
        return _C.ops.mesh.face_areas_forward_cuda(vertices, faces, items)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_areas):
        vertices, faces, merged_faces = ctx.saved_tensors
        corner_grads = _C.ops.mesh.face_areas_backward_cuda(grad_areas, vertices, faces, ctx.items)
        if ctx.items is None:
            return _sum_corner_grads(corner_grads, faces, vertices.shape[1]), None, None, None
        return _sum_corner_grads(corner_grads.unsqueeze(0), merged_faces, vertices.shape[0])[0], None, None, None


class _SamplePoints(torch.autograd.Function):
    @staticmethod
    def forward(ctx, vertices, face_features, faces, items, areas, r, uv):
        points, choices, features, _, cdf = _C.ops.mesh.sample_points_forward_cuda(vertices, faces, items, areas, r, uv, face_features)
        ctx.save_for_backward(faces, cdf, uv, choices)
        ctx.items = items
        ctx.num_vertices = vertices.shape[-2]
        ctx.feature_dim = 0 if face_features is None else face_features.shape[-1]
        ctx.mark_non_differentiable(choices)
        return points, choices, features

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_points, _grad_choices, grad_features):
        faces, cdf, uv, choices = ctx.saved_tensors
        want_v, want_f = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and grad_features is not None
        grad_vertices, grad_ff = _C.ops.mesh.sample_points_backward_cuda(
            grad_points if want_v else None, grad_features if want_f else None, faces, ctx.items, cdf, uv, choices, ctx.num_vertices,
            ctx.feature_dim if want_f else 0)
        return grad_vertices, grad_ff, None, None, None, None, None


# ---- argument checks --------------------------------------------------------------------------------------------------------------
def _describe(t):
    return f'{tuple(t.shape)} {t.dtype}' if isinstance(t, torch.Tensor) else type(t).__name__


def _check_mesh(fn, vertices, faces, packed):
    if not isinstance(faces, torch.Tensor) or faces.dim() < 1:
        raise ValueError(f'{fn}: faces must be an integer tensor of shape (num_faces, 3), got {_describe(faces)}')
    if faces.shape[-1] != 3:
        raise NotImplementedError(f'{fn} is only implemented for triangle meshes')
    if faces.dim() != 2 or faces.dtype not in _INDEX_DTYPES:
        raise ValueError(f'{fn}: faces must be an integer tensor of shape (num_faces, 3), got {_describe(faces)}')
    want = '(num_vertices, 3)' if packed else '(batch_size, num_vertices, 3)'
    if not isinstance(vertices, torch.Tensor) or vertices.dim() != (2 if packed else 3) or vertices.shape[-1] != 3 or \
            not vertices.is_floating_point():
        raise ValueError(f'{fn}: vertices must be a floating point tensor of shape {want}, got {_describe(vertices)}')
    if faces.device != vertices.device:
        raise ValueError(f'{fn}: vertices are on {vertices.device} and faces on {faces.device}')
    if faces.shape[0] < 1:
        raise ValueError(f'{fn}: no faces')


def _check_ids(fn, faces, num_vertices):
    if not faces_in_range(faces, num_vertices):
        raise IndexError(f'{fn}: faces hold an index outside [0, num_vertices = {num_vertices})')


def _check_num_samples(fn, num_samples):
    if isinstance(num_samples, bool) or not isinstance(num_samples, int) or num_samples < 0:
        raise ValueError(f'{fn}: num_samples must be a non-negative int, got {num_samples!r}')


def _check_per_face(fn, name, t, shape, vertices):
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or not t.is_floating_point():
        raise ValueError(f'{fn}: {name} must be a floating point tensor of shape {shape}, got {_describe(t)}')
    if t.device != vertices.device:
        raise ValueError(f'{fn}: vertices are on {vertices.device} and {name} on {t.device}')


def _on_hip(vertices, faces, areas=None, face_features=None):
    return vertices.is_cuda and vertices.dtype in _HIP_DTYPES and faces.dtype == torch.int64 and \
        (areas is None or areas.dtype in _HIP_DTYPES) and (face_features is None or face_features.dtype == vertices.dtype)


def _packed_items(fn, vertices, first_idx_vertices, faces, num_faces_per_mesh):
    """The per-item table of the packed form, built on the host (both index tensors are CPU tensors by the reference's contract)
    -> (rows [(face_begin, face_end, vertex_base)], vertex counts)"""
    for name, t in (('first_idx_vertices', first_idx_vertices), ('num_faces_per_mesh', num_faces_per_mesh)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.is_floating_point():
            raise ValueError(f'{fn}: {name} must be a 1-D integer tensor, got {_describe(t)}')
    counts = [int(c) for c in num_faces_per_mesh.tolist()]
    first = [int(c) for c in first_idx_vertices.tolist()]
    if len(counts) < 1 or len(first) != len(counts) + 1:
        raise ValueError(f'{fn}: first_idx_vertices must hold batch_size + 1 = {len(counts) + 1} entries, got {len(first)}')
    if min(counts) < 1 or sum(counts) != faces.shape[0]:
        raise ValueError(f'{fn}: num_faces_per_mesh must hold positive counts that add up to the {faces.shape[0]} faces, got {counts}')
    if first[0] < 0 or any(b < a for a, b in zip(first, first[1:])) or first[-1] > vertices.shape[0]:
        raise ValueError(f'{fn}: first_idx_vertices must ascend inside the {vertices.shape[0]} vertices, got {first}')
    rows, begin = [], 0
    for b, count in enumerate(counts):
        rows.append((begin, begin + count, first[b]))
        begin += count
    return rows, [first[b + 1] - first[b] for b in range(len(counts))]


def _packed_tensors(fn, vertices, faces, rows, vertex_counts):
    """-> (items for the shims, merged faces); raises IndexError for a local id outside its item's vertices: ONE host read"""
    dev = vertices.device
    table = torch.tensor(rows, dtype=torch.long)
    per_item = table[:, 1] - table[:, 0]
    base = torch.repeat_interleave(table[:, 2], per_item).to(dev)
    limit = torch.repeat_interleave(torch.tensor(vertex_counts, dtype=torch.long), per_item).to(dev)
    local = faces.long()
    if bool(((local < 0) | (local >= limit.unsqueeze(1))).any()):                      # the one host read
        raise IndexError(f'{fn}: faces hold an index outside the vertices of their mesh')
    return (table.to(dev), int(per_item.max())), local + base.unsqueeze(1)


# ---- the public functions ---------------------------------------------------------------------------------------------------------
def face_areas(vertices, faces):
    r"""Compute the areas of each face of triangle meshes (reference: kaolin/ops/mesh/trianglemesh.py:98-122).

    ``sqrt((a + b) + c) * 0.5`` of the reference's cross-product terms, one rounding per operation: on float / double CUDA tensors
    one HIP launch whose result carries the bits of the reference's CPU result.  Differentiable in ``vertices`` (HIP: a per-corner
    kernel and the deterministic per-vertex sum of ``average_face_vertex_features``; NaN at a zero-area face, as the reference).

    Args:
        vertices (torch.Tensor): The vertices of the meshes, of shape :math:`(\text{batch_size}, \text{num_vertices}, 3)`,
            any strides.
        faces (torch.LongTensor): the faces of the meshes, of shape :math:`(\text{num_faces}, 3)`.

    Returns:
        (torch.Tensor): the face areas of same type as vertices and of shape :math:`(\text{batch_size}, \text{num_faces})`.
    """
    fn = 'face_areas'
    _check_mesh(fn, vertices, faces, False)
    _check_ids(fn, faces, vertices.shape[1])
    if _on_hip(vertices, faces) and vertices.shape[0] >= 1:
        return _FaceAreas.apply(vertices, faces, None, None)
    return face_areas_torch(vertices, faces)


def packed_face_areas(vertices, first_idx_vertices, faces, num_faces_per_mesh):
    r"""Compute the areas of each face of packed triangle meshes (reference: kaolin/ops/mesh/trianglemesh.py:125-156).

    Args:
        vertices (torch.Tensor): The packed vertices of the meshes, of shape :math:`(\text{num_vertices}, 3)`.
        first_idx_vertices (torch.Tensor): The first_idx associated to vertices, of shape :math:`(\text{batch_size} + 1)`, on the CPU.
        faces (torch.LongTensor): The packed faces of the meshes (ids local to each mesh), of shape :math:`(\text{num_faces}, 3)`.
        num_faces_per_mesh: The number of faces per mesh, of shape :math:`(\text{batch_size})`, on the CPU.

    Returns:
        (torch.Tensor): The face areas of same type as vertices and of shape :math:`(\text{num_faces})`.
    """
    fn = 'packed_face_areas'
    _check_mesh(fn, vertices, faces, True)
    rows, vertex_counts = _packed_items(fn, vertices, first_idx_vertices, faces, num_faces_per_mesh)
    items, merged = _packed_tensors(fn, vertices, faces, rows, vertex_counts)
    if _on_hip(vertices, faces):
        return _FaceAreas.apply(vertices, faces, items, merged)
    return face_areas_torch(vertices.unsqueeze(0), merged)[0]


def sample_points(vertices, faces, num_samples, areas=None, face_features=None):
    r"""Uniformly sample points over the surface of triangle meshes (reference: kaolin/ops/mesh/trianglemesh.py:159-240).

    The face of every point is chosen with a probability proportional to its area, the point uniformly on the face.  Draws
    ``torch.rand((B, N), dtype=float64)`` and ``torch.rand((B, N, 2), dtype=vertices.dtype)`` on the device of ``vertices``, in
    this order, with or without ``areas``; the rest is the deterministic operator of the module's docstring (the samples of a seed
    are NOT the reference's).  Differentiable in ``vertices`` and ``face_features``, not in ``areas``.  An item without a positive
    finite total area returns NaN points (the reference raises).

    Args:
        vertices (torch.Tensor): The vertices of the meshes, of shape :math:`(\text{batch_size}, \text{num_vertices}, 3)`.
        faces (torch.LongTensor): The faces of the mesh, of shape :math:`(\text{num_faces}, 3)`.
        num_samples (int): The number of point sampled per mesh.
        areas (torch.Tensor, optional): The areas of each face, of shape :math:`(\text{batch_size}, \text{num_faces})`, can be
            preprocessed, for fast on-the-fly sampling, will be computed if None (default).
        face_features (torch.Tensor, optional): Per-vertex-per-face features, matching ``faces`` order, of shape
            :math:`(\text{batch_size}, \text{num_faces}, 3, \text{feature_dim})`, any strides.

    Returns:
        (torch.Tensor, torch.LongTensor, (optional) torch.Tensor): the pointclouds of shape
        :math:`(\text{batch_size}, \text{num_samples}, 3)`, the indexes of the faces selected, of shape
        :math:`(\text{batch_size}, \text{num_samples})`, and, if ``face_features`` is specified, the interpolated features of
        shape :math:`(\text{batch_size}, \text{num_samples}, \text{feature_dim})`.
    """
    fn = 'sample_points'
    _check_mesh(fn, vertices, faces, False)
    _check_num_samples(fn, num_samples)
    B, V, F, N, dev = vertices.shape[0], vertices.shape[1], faces.shape[0], num_samples, vertices.device
    if areas is not None:
        _check_per_face(fn, 'areas', areas, (B, F), vertices)
    if face_features is not None:
        if not isinstance(face_features, torch.Tensor) or face_features.dim() != 4 or tuple(face_features.shape[:3]) != (B, F, 3) or \
                not face_features.is_floating_point():
            raise ValueError(f'{fn}: face_features must be a floating point tensor of shape ({B}, {F}, 3, feature_dim), '
                             f'got {_describe(face_features)}')
        if face_features.device != dev:
            raise ValueError(f'{fn}: vertices are on {dev} and face_features on {face_features.device}')
    _check_ids(fn, faces, V)
    r = torch.rand((B, N), dtype=torch.float64, device=dev)
    uv = torch.rand((B, N, 2), dtype=vertices.dtype, device=dev)
    D = 0 if face_features is None else face_features.shape[-1]
    if N == 0 or B == 0:
        points, choices = vertices.new_empty((B, N, 3)), torch.empty((B, N), dtype=torch.long, device=dev)
        features = None if face_features is None else face_features.new_empty((B, N, D))
    elif _on_hip(vertices, faces, areas, face_features) and (face_features is None or D >= 1):
        points, choices, features = _SamplePoints.apply(vertices, face_features, faces, None, areas, r, uv)
    else:
        points, choices, features = sample_points_torch(vertices, faces, areas, r, uv, face_features)
    if face_features is not None:
        return points, choices, features
    return points, choices


def packed_sample_points(vertices, first_idx_vertices, faces, num_faces_per_mesh, num_samples, areas=None):
    r"""Uniformly sample points over the surface of packed triangle meshes (reference: kaolin/ops/mesh/trianglemesh.py:246-311);
    the returned pointclouds are with fixed batching.  The draws and the operator are those of :func:`sample_points`.

    Args:
        vertices (torch.Tensor): The packed vertices of the meshes, of shape :math:`(\text{num_vertices}, 3)`.
        first_idx_vertices (torch.Tensor): The first_idx associated to vertices, of shape :math:`(\text{batch_size} + 1)`, on the CPU.
        faces (torch.LongTensor): The packed faces of the meshes (ids local to each mesh), of shape :math:`(\text{num_faces}, 3)`.
        num_faces_per_mesh: The number of faces per mesh, of shape :math:`(\text{batch_size})`, on the CPU.
        num_samples (int): The number of point sampled per mesh.
        areas (torch.Tensor, optional): The areas of each face, of shape :math:`(\text{num_faces})`, computed if None (default).

    Returns:
        (torch.Tensor, torch.LongTensor): The pointclouds, of shape :math:`(\text{batch_size}, \text{num_points}, 3)`, and the
        indexes of the faces selected (as merged faces), of shape :math:`(\text{batch_size}, \text{num_points})`.
    """
    fn = 'packed_sample_points'
    _check_mesh(fn, vertices, faces, True)
    _check_num_samples(fn, num_samples)
    if areas is not None:
        _check_per_face(fn, 'areas', areas, (faces.shape[0],), vertices)
    rows, vertex_counts = _packed_items(fn, vertices, first_idx_vertices, faces, num_faces_per_mesh)
    items, merged = _packed_tensors(fn, vertices, faces, rows, vertex_counts)
    B, N, dev = len(rows), num_samples, vertices.device
    r = torch.rand((B, N), dtype=torch.float64, device=dev)
    uv = torch.rand((B, N, 2), dtype=vertices.dtype, device=dev)
    if N == 0:
        return vertices.new_empty((B, N, 3)), torch.empty((B, N), dtype=torch.long, device=dev)
    if _on_hip(vertices, faces, areas):
        points, choices, _ = _SamplePoints.apply(vertices, None, faces, items, areas, r, uv)
        return points, choices
    points, choices = [], []
    for b, (begin, end, _) in enumerate(rows):          # the torch formulation, item by item on the merged faces
        p, c, _ = sample_points_torch(vertices.unsqueeze(0), merged[begin:end], None if areas is None else areas[None, begin:end],
                                      r[b:b + 1], uv[b:b + 1])
        points.append(p)
        choices.append(c + begin)
    return torch.cat(points), torch.cat(choices)
