"""Per-vertex features from per-face-corner features: ``average_face_vertex_features``, ``compute_vertex_normals``,
``unindex_vertices_by_faces`` (API mirror of kaolin/ops/mesh/mesh.py) and ``vertex_tangents`` (kaolin/ops/mesh/trianglemesh.py) --
the step between a deforming mesh and smooth shading.

The reference adds with ``scatter_add_``, once per corner slot: float atomics on a GPU, an undefined order and results that change
from run to run.  On the CPU the same expression is, per vertex, a sequential sum over the corners that hold it in the order (corner
slot k ascending, then face f ascending), one rounded addition per corner, then ONE division by ``max(count, 1)``.  That order is the
contract of both paths here:

* float32 / float64 CUDA features with integer CUDA ``faces`` run csrc/vertex_features.hip through one autograd function: the lists
  vertex -> incident corners are built once per ``faces`` (``_C.ops.mesh.vertex_corners_cuda``: a stable keys-only sort, one host
  read) and every step is then ONE gather launch without atomics and without a host read; its result equals the reference's CPU
  result bit for bit, and two calls give the same bits;
* everything else (CPU tensors, half, bfloat16, mixed devices, no faces or no vertices) runs the torch formulation below, the
  reference's expression restated.

The topology cache.  The lists of the last ``faces`` are kept, ONE entry per device: the entry holds the ``faces`` tensor itself (a
strong reference: its storage cannot be handed to another tensor while the entry lives), its ``_version``, shape, strides, dtype, the
number of vertices and the two lists.  A call hits the entry when it passes a tensor with the same ``data_ptr()``, ``_version``,
shape, strides, dtype and number of vertices; any other call rebuilds the lists and replaces the entry.  In-place writes through
torch bump ``_version`` and are seen.  A WRITE THAT BYPASSES THE VERSION COUNTER (through ``.data``, ``detach()``-ed aliases written
by a raw kernel, another library) IS NOT SEEN: the lists of the old contents are used.  Pass a new tensor in that case.
"""
import torch
from torch.autograd.function import once_differentiable

from ... import _C

__all__ = ['average_face_vertex_features', 'compute_vertex_normals', 'unindex_vertices_by_faces', 'vertex_tangents']

_HIP_DTYPES = (torch.float32, torch.float64)
_INDEX_DTYPES = (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64)

# device index -> (signature, faces as passed, faces as the kernels read them, offsets, corners)
_vertex_corners_cache = {}


def _clear_vertex_corners_cache():
    _vertex_corners_cache.clear()


def _vertex_corners(faces, num_vertices):
    """The corner lists of ``faces`` from the cache, or built and cached -> (faces for the kernels, offsets, corners)"""
    slot = faces.device.index
    signature = (faces.data_ptr(), faces._version, tuple(faces.shape), faces.stride(), faces.dtype, num_vertices)
    entry = _vertex_corners_cache.get(slot)
    if entry is not None and entry[0] == signature:
        return entry[2:]
    _vertex_corners_cache.pop(slot, None)                 # a failed build leaves no entry behind
    kernel_faces = faces if faces.dtype in (torch.int32, torch.int64) else faces.long()
    offsets, corners = _C.ops.mesh.vertex_corners_cuda(kernel_faces, num_vertices)
    _vertex_corners_cache[slot] = (signature, faces, kernel_faces, offsets, corners)
    return kernel_faces, offsets, corners


class _VertexGather(torch.autograd.Function):
    """(B, F, K, N) -> (B, V, N): the per-vertex sum (or mean) of the corners' features in the order of the lists"""

    @staticmethod
    def forward(ctx, face_features, faces, offsets, corners, num_vertices, mean):
        ctx.save_for_backward(faces, offsets)
        ctx.mean = mean
        return _C.ops.mesh.vertex_gather_forward_cuda(face_features, offsets, corners, num_vertices, mean)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        faces, offsets = ctx.saved_tensors
        return _C.ops.mesh.vertex_gather_backward_cuda(grad_out, faces, offsets, ctx.mean), None, None, None, None, None


def _torch_vertex_gather(faces, face_features, num_vertices, mean):
    """The reference's expression (kaolin/ops/mesh/mesh.py:186-208): scatter_add_ per corner slot, one division"""
    B, F, K, N = face_features.shape
    out = torch.zeros((B, num_vertices, N), dtype=face_features.dtype, device=face_features.device)
    counts = torch.zeros((B, num_vertices), dtype=face_features.dtype, device=face_features.device)
    index = faces.long().unsqueeze(0).repeat(B, 1, 1)
    ones = torch.ones((B, F), dtype=face_features.dtype, device=face_features.device)
    for k in range(K):
        out.scatter_add_(1, index[..., k:k + 1].repeat(1, 1, N), face_features[..., k, :])
        counts.scatter_add_(1, index[..., k], ones)
    if mean:
        out = out / counts.clip(min=1).unsqueeze(-1)
    return out


def _vertex_gather(faces, face_features, num_vertices, mean):
    B, F, K, N = face_features.shape
    if face_features.is_cuda and face_features.dtype in _HIP_DTYPES and faces.device == face_features.device and \
            min(B, F, K, N, num_vertices) >= 1:
        kernel_faces, offsets, corners = _vertex_corners(faces, num_vertices)
        return _VertexGather.apply(face_features, kernel_faces, offsets, corners, num_vertices, mean)
    return _torch_vertex_gather(faces, face_features, num_vertices, mean)


def _check_faces(fn, faces, face_size=None):
    if not isinstance(faces, torch.Tensor) or faces.dim() != 2 or faces.dtype not in _INDEX_DTYPES or \
            (face_size is not None and faces.shape[1] != face_size):
        shape = tuple(faces.shape) if isinstance(faces, torch.Tensor) else type(faces).__name__
        dtype = faces.dtype if isinstance(faces, torch.Tensor) else None
        want = '(num_faces, face_size)' if face_size is None else f'(num_faces, {face_size})'
        raise ValueError(f'{fn}: faces must be an integer tensor of shape {want}, got {shape} {dtype}')


def average_face_vertex_features(faces, face_features, num_vertices=None):
    r"""Given features assigned for every vertex of every face, computes per-vertex features by averaging values across all faces
    incident each vertex (reference: kaolin/ops/mesh/mesh.py:172-208).

    A vertex that no face uses gets zeros; a face that repeats a vertex counts once per corner.  Per vertex the corners are added in
    the order (corner slot, then face), one rounded addition each, and the sum is divided once by the count: on float / double CUDA
    tensors by one HIP launch without atomics, whose result carries the bits of the reference's CPU result and does not change from
    run to run (the module's docstring has the paths and THE RULE OF THE TOPOLOGY CACHE: writes to ``faces`` that bypass its version
    counter are not seen).  Differentiable in ``face_features``.

    Args:
        faces (torch.LongTensor): vertex indices of faces of a fixed-topology mesh batch, of shape
            :math:`(\text{num_faces}, \text{face_size})`, any integer dtype, any strides.
        face_features (torch.Tensor): any features assigned for every vertex of every face, of shape
            :math:`(\text{batch_size}, \text{num_faces}, \text{face_size}, N)`, any strides (expanded dimensions included).
        num_vertices (int, optional): number of vertices V.  Default: ``int(faces.max()) + 1``, which is one host read per call.

    Returns:
        (torch.Tensor): of shape :math:`(\text{batch_size}, V, N)`, in the dtype of ``face_features``.
    """
    fn = 'average_face_vertex_features'
    _check_faces(fn, faces)
    if not isinstance(face_features, torch.Tensor) or face_features.dim() != 4 or not face_features.is_floating_point():
        shape = tuple(face_features.shape) if isinstance(face_features, torch.Tensor) else type(face_features).__name__
        dtype = face_features.dtype if isinstance(face_features, torch.Tensor) else None
        raise ValueError(f'{fn}: face_features must be a floating point tensor of shape (batch_size, num_faces, face_size, N), '
                         f'got {shape} {dtype}')
    if tuple(face_features.shape[1:3]) != tuple(faces.shape):
        raise ValueError(f'{fn}: face_features of shape {tuple(face_features.shape)} do not match faces of shape {tuple(faces.shape)}')
    if num_vertices is None:
        num_vertices = int(faces.max()) + 1
    num_vertices = int(num_vertices)
    if num_vertices < 0:
        raise ValueError(f'{fn}: num_vertices is {num_vertices}')
    return _vertex_gather(faces, face_features, num_vertices, True)


def compute_vertex_normals(faces, face_normals, num_vertices=None):
    r"""Computes normals for every vertex by averaging face normals assigned to that vertex for every face that has this vertex
    (reference: kaolin/ops/mesh/mesh.py:154-169; see :func:`average_face_vertex_features`, which it calls).

    Args:
        faces (torch.LongTensor): vertex indices of faces, of shape :math:`(\text{num_faces}, \text{face_size})`.
        face_normals (torch.Tensor): pre-normalized xyz normal values for every vertex of every face, of shape
            :math:`(\text{batch_size}, \text{num_faces}, \text{face_size}, 3)` (one normal per face expanded over the corners with
            stride 0 is read as it stands).
        num_vertices (int, optional): number of vertices V (set to max index in faces, if not set).

    Returns:
        (torch.Tensor): of shape :math:`(\text{batch_size}, V, 3)`.
    """
    return average_face_vertex_features(faces, face_normals, num_vertices=num_vertices)


def unindex_vertices_by_faces(face_vertex_features):
    r"""Given per-face per-vertex features, reshapes into flat indexed values and an index buffer
    (reference: kaolin/ops/mesh/mesh.py:28-51).

    Args:
        face_vertex_features (torch.Tensor): of shape :math:`(..., \text{num_faces}, \text{face_size}, \text{num_channels})`, with
            any number of preceding batch dimensions.

    Returns:
        (torch.Tensor, torch.LongTensor): of shapes :math:`(..., \text{num_faces} * \text{face_size}, \text{num_channels})` and
        :math:`(\text{num_faces}, \text{face_size})`.
    """
    old_shape = list(face_vertex_features.shape)
    nfaces, fsize, nchannels = old_shape[-3:]
    vertex_features = face_vertex_features.reshape(old_shape[:-3] + [nfaces * fsize, nchannels])
    face_indices = torch.arange(0, nfaces * fsize, device=face_vertex_features.device, dtype=torch.long).reshape((-1, fsize))
    return vertex_features, face_indices


def vertex_tangents(faces, face_vertices, face_uvs, vertex_normals):
    r"""Compute vertex tangents, useful to apply normal maps during rendering (reference: kaolin/ops/mesh/trianglemesh.py:614-670,
    its expressions in its order; see https://en.wikipedia.org/wiki/Normal_mapping#Calculating_tangent_space).

    The per-face tangent is computed in torch (autograd in ``face_vertices``, ``face_uvs`` and ``vertex_normals`` as in the
    reference); the reference's three ``scatter_add_`` calls are one per-vertex sum in the order of
    :func:`average_face_vertex_features`, on float / double CUDA tensors one HIP launch over the per-face tangent expanded over the
    three corners with stride 0.

    Args:
        faces (torch.LongTensor): unbatched triangle mesh faces, of shape :math:`(\text{num_faces}, 3)`.
        face_vertices (torch.Tensor): unbatched triangle face vertices, of shape :math:`(\text{num_faces}, 3, 3)`.
        face_uvs (torch.Tensor): unbatched triangle UVs, of shape :math:`(\text{num_faces}, 3, 2)`.
        vertex_normals (torch.Tensor): unbatched vertex normals, of shape :math:`(\text{num_vertices}, 3)`.

    Returns:
        (torch.Tensor): The vertex tangents, of shape :math:`(\text{num_vertices}, 3)`.
    """
    fn = 'vertex_tangents'
    _check_faces(fn, faces, 3)
    F = faces.shape[0]
    for name, t, shape in (('face_vertices', face_vertices, (F, 3, 3)), ('face_uvs', face_uvs, (F, 3, 2))):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or not t.is_floating_point():
            got = (tuple(t.shape), t.dtype) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f'{fn}: {name} must be a floating point tensor of shape {shape}, got {got}')
    if not isinstance(vertex_normals, torch.Tensor) or vertex_normals.dim() != 2 or vertex_normals.shape[1] != 3 or \
            not vertex_normals.is_floating_point():
        got = (tuple(vertex_normals.shape), vertex_normals.dtype) if isinstance(vertex_normals, torch.Tensor) else \
            type(vertex_normals).__name__
        raise ValueError(f'{fn}: vertex_normals must be a floating point tensor of shape (num_vertices, 3), got {got}')

    face_uvs0, face_uvs1, face_uvs2 = torch.split(face_uvs, 1, dim=-2)
    fv0, fv1, fv2 = torch.split(face_vertices, 1, dim=-2)
    uve1 = face_uvs1 - face_uvs0
    uve2 = face_uvs2 - face_uvs0
    pe1 = (fv1 - fv0).squeeze(-2)
    pe2 = (fv2 - fv0).squeeze(-2)

    nom = pe1 * uve2[..., 1] - pe2 * uve1[..., 1]
    denom = uve1[..., 0] * uve2[..., 1] - uve1[..., 1] * uve2[..., 0]
    # Avoid division by zero for degenerated texture coordinates
    tang = nom / torch.where(denom > 0.0, torch.clamp(denom, min=1e-6), torch.clamp(denom, max=-1e-6))

    if tang.dtype == vertex_normals.dtype and tang.device == vertex_normals.device:
        # (1, F, 3, 3): the tangent of a face at each of its corners, never materialised
        tangents = _vertex_gather(faces, tang[None, :, None, :].expand(1, F, 3, 3), vertex_normals.shape[0], False)[0]
    else:                                                  # mixed dtypes or devices: torch's own error, as in the reference
        tangents = torch.zeros_like(vertex_normals)
        for i in range(3):
            tangents.scatter_add_(0, faces[:, i:i + 1].repeat(1, 3), tang)
    # Normalize and make sure tangent is perpendicular to normal
    tangents = torch.nn.functional.normalize(tangents, dim=1)
    tangents = torch.nn.functional.normalize(
        tangents - torch.sum(tangents * vertex_normals, dim=-1, keepdim=True) * vertex_normals)

    if torch.is_anomaly_enabled():
        assert torch.all(torch.isfinite(tangents))

    return tangents
