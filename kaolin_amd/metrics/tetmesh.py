"""``tetrahedron_volume``, ``equivolume`` and ``amips`` (API mirror of kaolin/metrics/tetmesh.py): the regularisers of the DMTet /
DefTet loop, next to ``ops.conversions.marching_tetrahedra`` and ``ops.mesh.subdivide_tetmesh``.

float32 / float64 CUDA tensors (one device, one dtype, at least one tetrahedron) run the fused kernels of
csrc/tetmesh_metrics.hip: one launch per direction reads every tet once, the backward recomputes from the inputs (nothing of
the size of the mesh is kept for it), the two losses are reduced without atomics -- two runs of a call are bit-identical -- and
nothing synchronises, so the calls capture into a graph.  ``equivolume`` takes that path when the row it subtracts has ONE
element (see its docstring) and ``pow`` is an int in [1, 16].  Everything else (CPU tensors, half, mixed dtypes, no tetrahedrons,
other ``pow``) runs the torch formulations below, which follow the reference's order of operations.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _C
from ..ops.mesh.tetmesh import _validate_tet_vertices

__all__ = ['tetrahedron_volume', 'equivolume', 'amips']

_AMIPS_EPS = 1e-10


# ---- the torch formulations ---------------------------------------------------------------------------------------------------------
def _torch_volume(tet_vertices):
    a, b, c, d = tet_vertices.unbind(dim=2)
    return ((a - d) * torch.cross(b - d, c - d, dim=2)).sum(dim=2) / 6


def _torch_equivolume(tet_vertices, tetrahedrons_mean, pow):
    volumes = _torch_volume(tet_vertices)
    if tetrahedrons_mean is None:
        tetrahedrons_mean = volumes.mean(dim=-1)
    # a (1, M) row against the (B, T) volumes: it broadcasts along the TET axis (see equivolume's docstring)
    return (volumes - tetrahedrons_mean.reshape(1, -1)).abs().pow(pow).mean(dim=-1, keepdim=True)


def _torch_amips(tet_vertices, inverse_offset_matrix):
    offsets = tet_vertices[:, :, 1:] - tet_vertices[:, :, :1]               # the rows B - A, C - A, D - A
    jacobian = torch.matmul(offsets, inverse_offset_matrix)
    det = torch.det(jacobian)
    trace = torch.matmul(jacobian, jacobian.transpose(-2, -1)).diagonal(dim1=-2, dim2=-1).sum(-1)
    denominator = (det.pow(2) + _AMIPS_EPS).pow(1 / 3)
    return (trace / denominator * (det >= 0).float()).mean(dim=1, keepdim=True)   # a mask PRODUCT, as the reference's


# ---- the HIP path -------------------------------------------------------------------------------------------------------------------
class _TetrahedronVolume(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tet_vertices):
        ctx.save_for_backward(tet_vertices)
        return _C.metrics.tetmesh_volume_forward_cuda(tet_vertices)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_volumes):
        tet_vertices, = ctx.saved_tensors
        return _C.metrics.tetmesh_volume_backward_cuda(grad_volumes, tet_vertices)


class _Equivolume(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tet_vertices, mean, power):
        ctx.save_for_backward(tet_vertices, mean)
        ctx.power = power
        return _C.metrics.tetmesh_equivolume_forward_cuda(tet_vertices, mean, power)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        tet_vertices, mean = ctx.saved_tensors
        grad_tet_vertices, grad_mean = _C.metrics.tetmesh_equivolume_backward_cuda(
            grad_loss, tet_vertices, mean, ctx.power, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return grad_tet_vertices, grad_mean, None


class _Amips(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tet_vertices, inverse_offset_matrix):
        ctx.save_for_backward(tet_vertices, inverse_offset_matrix)
        return _C.metrics.tetmesh_amips_forward_cuda(tet_vertices, inverse_offset_matrix)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_loss):
        tet_vertices, inverse_offset_matrix = ctx.saved_tensors
        return _C.metrics.tetmesh_amips_backward_cuda(grad_loss, tet_vertices, inverse_offset_matrix,
                                                      ctx.needs_input_grad[0], ctx.needs_input_grad[1])


def _on_hip(tet_vertices, *others):
    """float32 / float64 on a GPU, at least one tet of at least one item, and every other tensor of that device and dtype"""
    return (tet_vertices.is_cuda and tet_vertices.dtype in (torch.float32, torch.float64) and tet_vertices.shape[0] >= 1 and
            tet_vertices.shape[1] >= 1 and
            all(torch.is_tensor(t) and t.device == tet_vertices.device and t.dtype == tet_vertices.dtype for t in others))


def tetrahedron_volume(tet_vertices):
    r"""Compute the signed volume of tetrahedrons: :math:`((A - D) \cdot ((B - D) \times (C - D))) / 6`
    (reference: kaolin/metrics/tetmesh.py).  Differentiable.

    Args:
        tet_vertices (torch.Tensor):
            Batched tetrahedrons, of shape :math:`(\text{batch_size}, \text{num_tetrahedrons}, 4, 3)`.

    Returns:
        (torch.Tensor):
            volume of each tetrahedron in each mesh, of shape :math:`(\text{batch_size}, \text{num_tetrahedrons})`.

    Example:
        >>> tet_vertices = torch.tensor([[[[0.5000, 0.5000, 0.4500],
        ...                                [0.4500, 0.5000, 0.5000],
        ...                                [0.4750, 0.4500, 0.4500],
        ...                                [0.5000, 0.5000, 0.5000]]]])
        >>> tetrahedron_volume(tet_vertices)
        tensor([[-2.0833e-05]])
    """
    _validate_tet_vertices(tet_vertices)
    if _on_hip(tet_vertices):
        return _TetrahedronVolume.apply(tet_vertices)
    return _torch_volume(tet_vertices)


def equivolume(tet_vertices, tetrahedrons_mean=None, pow=4):
    r"""Compute the EquiVolume loss of `Learning Deformable Tetrahedral Meshes for 3D Reconstruction`_ (NeurIPS 2020): the mean
    over the tetrahedrons of :math:`|volume - mean|^{pow}` (reference: kaolin/metrics/tetmesh.py).  Differentiable in
    ``tet_vertices`` and ``tetrahedrons_mean``.

    As in the reference, ``tetrahedrons_mean`` (by default the mean volume of every mesh, :math:`\text{batch_size}` numbers) is
    reshaped to a :math:`(1, M)` row and subtracted from the :math:`(\text{batch_size}, \text{num_tetrahedrons})` volumes, so it
    broadcasts along the **tetrahedron** axis: the call is well-formed for :math:`M = 1` -- one mesh, or one given number --
    and for :math:`M = \text{num_tetrahedrons}` (entry :math:`j` is then subtracted from tetrahedron :math:`j` of every mesh);
    anything else raises the RuntimeError of the failed broadcast.  :math:`M = 1` with an int ``pow`` in [1, 16] runs the HIP
    kernels on a GPU.

    Args:
        tet_vertices (torch.Tensor):
            Batched tetrahedrons, of shape :math:`(\text{batch_size}, \text{num_tetrahedrons}, 4, 3)`.
        tetrahedrons_mean (torch.Tensor):
            Mean volume of all tetrahedrons in a grid (see above).  Default: the mean volume of every mesh.
        pow (int):
            Power for the equivolume loss.  Increasing power puts more emphasis on the larger tetrahedron deformation.
            Default: 4.

    Returns:
        (torch.Tensor):
            EquiVolume loss for each mesh, of shape :math:`(\text{batch_size}, 1)`.

    Example:
        >>> tet_vertices = torch.tensor([[[[0.5000, 0.5000, 0.7500],
        ...                                [0.4500, 0.8000, 0.6000],
        ...                                [0.4750, 0.4500, 0.2500],
        ...                                [0.5000, 0.3000, 0.3000]],
        ...                               [[0.4750, 0.4500, 0.2500],
        ...                                [0.5000, 0.9000, 0.3000],
        ...                                [0.4500, 0.4000, 0.9000],
        ...                                [0.4500, 0.4500, 0.7000]]]])
        >>> equivolume(tet_vertices, torch.tensor([0.01]), pow=2)
        tensor([[9.4907e-05]])

    .. _Learning Deformable Tetrahedral Meshes for 3D Reconstruction: https://nv-tlabs.github.io/DefTet/
    """
    _validate_tet_vertices(tet_vertices)
    power_ok = isinstance(pow, int) and not isinstance(pow, bool) and 1 <= pow <= 16
    if power_ok and tetrahedrons_mean is None and tet_vertices.shape[0] == 1 and _on_hip(tet_vertices):
        mean = tetrahedron_volume(tet_vertices).mean(dim=-1)             # autograd adds this branch's gradient to the kernel's
        return _Equivolume.apply(tet_vertices, mean, pow)
    if power_ok and tetrahedrons_mean is not None and _on_hip(tet_vertices, tetrahedrons_mean) and tetrahedrons_mean.numel() == 1:
        return _Equivolume.apply(tet_vertices, tetrahedrons_mean, pow)
    return _torch_equivolume(tet_vertices, tetrahedrons_mean, pow)


def amips(tet_vertices, inverse_offset_matrix):
    r"""Compute the AMIPS (Advanced MIPS) loss of `Computing Locally Injective Mappings by Advanced MIPS`_ (SIGGRAPH 2015): with
    the Jacobian :math:`J` = (rows :math:`B - A`, :math:`C - A`, :math:`D - A`) times ``inverse_offset_matrix``, the mean over
    the tetrahedrons of :math:`tr(J J^T) / (\det(J)^2 + 10^{-10})^{1/3}`, counting only tetrahedrons with :math:`\det(J) \ge 0`
    (reference: kaolin/metrics/tetmesh.py).  Differentiable in both arguments.

    Args:
        tet_vertices (torch.Tensor):
            Batched tetrahedrons, of shape :math:`(\text{batch_size}, \text{num_tetrahedrons}, 4, 3)`.
        inverse_offset_matrix (torch.Tensor):
            The inverse of the offset matrix of the rest shape, of shape
            :math:`(\text{batch_size}, \text{num_tetrahedrons}, 3, 3)` (a batch of one broadcasts).
            Refer to :func:`kaolin_amd.ops.mesh.tetmesh.inverse_vertices_offset`.

    Returns:
        (torch.Tensor):
            AMIPS loss for each mesh, of shape :math:`(\text{batch_size}, 1)`.

    Example:
        >>> tet_vertices = torch.tensor([[[[0., 0., 0.], [1., 0., 0.], [0., 1., 0.], [0., 0., 2.]]]])
        >>> amips(tet_vertices, torch.eye(3).reshape(1, 1, 3, 3))
        tensor([[3.7798]])

    .. _Computing Locally Injective Mappings by Advanced MIPS:
        https://www.microsoft.com/en-us/research/publication/computing-locally-injective-mappings-advanced-mips/
    """
    _validate_tet_vertices(tet_vertices)
    if (_on_hip(tet_vertices, inverse_offset_matrix) and inverse_offset_matrix.dim() == 4 and
            inverse_offset_matrix.shape[0] in (1, tet_vertices.shape[0]) and
            inverse_offset_matrix.shape[1:] == (tet_vertices.shape[1], 3, 3)):
        return _Amips.apply(tet_vertices, inverse_offset_matrix)
    return _torch_amips(tet_vertices, inverse_offset_matrix)
