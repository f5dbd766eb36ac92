"""kaolin.ops.conversions.pointcloud (reference: kaolin/ops/conversions/pointcloud.py): point clouds -> occupancy grids, and a point
cloud with per-point features -> a Structured Point Cloud.  GPU tensors run csrc/pointcloud.hip through ``_C.ops.conversions``; CPU
tensors run the torch formulations of the same contracts below (the reference rejects CPU tensors in
``unbatched_pointcloud_to_spc``: its Morton operators are CUDA only)."""
import torch

from ... import _C
from ...rep import Spc
from ..spc.points import quantize_points, unbatched_points_to_octree, _torch_points_to_morton

__all__ = ['pointclouds_to_voxelgrids', 'unbatched_pointcloud_to_spc']

_FLOATS = (torch.float16, torch.float32, torch.float64)
_FEATURE_DTYPES = (torch.bool, torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64) + _FLOATS
_MAX_LEVEL = 15             # KAOLIN_SPC_MAX_LEVELS
_MAX_HALF_LEVEL = 11        # 2^level - 1 is a half up to here


# ---- voxel grids -----------------------------------------------------------------------------------------------------------------------
def _torch_pointclouds_to_voxelgrids(pointclouds, resolution, origin, scale, return_sparse):
    """The contract on any device, every operation rounded in the points' dtype: a point marks the voxel
    round_half_even(((p - origin) / scale) * (R - 1)) when all three indices lie in [0, R - 1]; NaN and +-inf fail that test."""
    B, P, R, dtype, dev = pointclouds.size(0), pointclouds.size(1), resolution, pointclouds.dtype, pointclouds.device
    mult = torch.ones(1, dtype=dtype, device=dev) * (R - 1)
    v = torch.round(((pointclouds - origin.unsqueeze(1)) / scale.view(-1, 1, 1)) * mult)
    keep = ((v >= 0) & (v <= R - 1)).all(dim=-1)                                        # (B, P)
    item = torch.arange(B, device=dev).unsqueeze(1).expand(B, P)[keep]
    cell = v[keep].long()
    lin = ((item * R + cell[:, 0]) * R + cell[:, 1]) * R + cell[:, 2]
    if not return_sparse:
        grid = torch.zeros(B * R ** 3, dtype=dtype, device=dev)
        grid[lin] = 1
        return grid.reshape(B, R, R, R)
    lin = torch.unique(lin)                                                             # ascending = lexicographic (b, x, y, z)
    idx = torch.stack([lin // R ** 3, (lin // (R * R)) % R, (lin // R) % R, lin % R])
    return torch.sparse_coo_tensor(idx, torch.ones(lin.numel(), dtype=dtype, device=dev), (B, R, R, R), is_coalesced=True)


def pointclouds_to_voxelgrids(pointclouds, resolution, origin=None, scale=None, return_sparse=False):
    r"""Converts pointclouds to voxelgrids: a voxel is occupied when a point falls on it.

    Only the points in the range `[0, 1]` after ``(pointclouds - origin) / scale`` are converted: point ``p`` marks the voxel
    ``round(((p - origin) / scale) * (resolution - 1))`` (ties to even).  Every operation is rounded in the dtype of
    ``pointclouds`` (half: computed in float and rounded to half after each operation), so the result carries the reference's bits
    for each dtype.  A point with a NaN or infinite coordinate (also after the division: ``scale = 0``) marks nothing.

    On the GPU the dense grid is a zero fill and ONE HIP launch (one thread per point, plain stores, no atomics, no host read:
    capturable when ``origin`` and ``scale`` are given).  ``return_sparse=True`` sets the voxels' bits in a bit grid
    (``resolution^3 / 8`` bytes per item) with atomic OR and compacts the occupied words in torch (two host reads);
    ``resolution^3`` scalars are never allocated.  Not differentiable (the reference's result carries no gradient either).

    Args:
        pointclouds (torch.Tensor): half, float or double, of shape :math:`(\text{batch_size}, \text{num_points}, 3)`.
        resolution (int): resolution of the voxelgrids.
        origin (optional, torch.Tensor): origin of the voxelgrid in the pointcloud coordinates, of shape
            :math:`(\text{batch_size}, 3)`.  Default: ``torch.min(pointcloud, dim=1)[0]``.
        scale (optional, torch.Tensor): scale by which the coordinates are divided, of shape :math:`(\text{batch_size})`.
            Default: ``torch.max(torch.max(pointclouds, dim=1)[0] - origin, dim=1)[0]``.
        return_sparse (optional, bool): return a sparse COO tensor (int64 indices ``(4, nnz)``, sorted and unique; values ones;
            marked as coalesced).  Default: False.

    Returns:
        (torch.Tensor): the voxelgrids of 0 / 1 in the dtype of ``pointclouds``, of shape
        :math:`(\text{batch_size}, \text{resolution}, \text{resolution}, \text{resolution})`.

    Example:
        >>> pointclouds = torch.tensor([[[0, 0, 0],
        ...                              [1, 1, 1],
        ...                              [2, 2, 2]]], dtype=torch.float)
        >>> pointclouds_to_voxelgrids(pointclouds, 3)
        tensor([[[[1., 0., 0.],
                  [0., 0., 0.],
                  [0., 0., 0.]],
        <BLANKLINE>
                 [[0., 0., 0.],
                  [0., 1., 0.],
                  [0., 0., 0.]],
        <BLANKLINE>
                 [[0., 0., 0.],
                  [0., 0., 0.],
                  [0., 0., 1.]]]])
    """
    if not isinstance(resolution, int):
        raise TypeError(f"Expected resolution to be int "
                        f"but got {type(resolution)}.")
    fn = 'pointclouds_to_voxelgrids'
    if not isinstance(pointclouds, torch.Tensor) or pointclouds.dim() != 3 or pointclouds.size(2) != 3 or \
            pointclouds.dtype not in _FLOATS:
        raise ValueError(f'{fn}: pointclouds must be half, float or double, of size (batch_size, num_points, 3)')
    if resolution < 1:
        raise ValueError(f'{fn}: resolution must be at least 1, got {resolution}')
    B, P = pointclouds.size(0), pointclouds.size(1)
    for name, t, shape in (('origin', origin, (B, 3)), ('scale', scale, (B,))):
        if t is not None and not (isinstance(t, torch.Tensor) and tuple(t.shape) == shape and t.dtype == pointclouds.dtype and
                                  t.device == pointclouds.device):
            raise ValueError(f'{fn}: {name} must be a {pointclouds.dtype} tensor of size {shape} on {pointclouds.device}')
    if P == 0 and (origin is None or scale is None):
        raise ValueError(f'{fn}: a pointcloud without points has no default origin and scale')
    pointclouds = pointclouds.detach()
    if origin is None:
        origin = torch.min(pointclouds, dim=1)[0]
    if scale is None:
        scale = torch.max(torch.max(pointclouds, dim=1)[0] - origin, dim=1)[0]
    if pointclouds.is_cuda:
        return _C.ops.conversions.pointclouds_to_voxelgrids_cuda(pointclouds, resolution, origin, scale, bool(return_sparse))
    return _torch_pointclouds_to_voxelgrids(pointclouds, resolution, origin.detach(), scale.detach(), bool(return_sparse))


# ---- SPC -------------------------------------------------------------------------------------------------------------------------------
def _torch_pointcloud_to_spc(pointcloud, level, features):
    """(octree, features): the octree of the quantised points; per cell, in Morton order, the double sum of its members' features in
    ascending input index, divided by the count in double, rounded (half to even) for integer and bool dtypes, cast."""
    points = quantize_points(pointcloud, level)
    octree = unbatched_points_to_octree(points, level)
    if features is None:
        return octree, None
    morton, order = torch.sort(_torch_points_to_morton(points), stable=True)
    _, run, counts = torch.unique_consecutive(morton, return_inverse=True, return_counts=True)
    total = torch.zeros((counts.numel(), features.size(1)), dtype=torch.float64, device=features.device)
    total.index_add_(0, run, features[order].double())
    mean = total / counts.unsqueeze(1).double()
    if not features.is_floating_point():
        mean = torch.round(mean)
    return octree, mean.to(features.dtype)


def unbatched_pointcloud_to_spc(pointcloud, level, features=None):
    r"""Converts a single point cloud -- continuous coordinates in 3D -- into a Structured Point Cloud: the octree of the cells of
    ``level`` that hold a point and, with ``features``, the mean feature of every cell.

    Coordinates are expected in :math:`[-1, 1]`; a point outside is clipped to the border cells.  The octree is that of
    ``unbatched_points_to_octree(quantize_points(pointcloud, level), level)``, byte for byte.  A NaN COORDINATE QUANTISES TO 0 (the
    cast of NaN to int16).  Half points are taken up to ``level`` 11: beyond, ``2^level - 1`` is not a half and the clamp of
    ``quantize_points`` lets a coordinate wrap negative, so ``ValueError`` is raised.

    Row ``r`` of ``features`` of the result belongs to the ``r``-th point of the last level in Morton order (the rows of
    ``generate_points`` at ``pyramids[0, 1, level]``).  It is the mean over all input points of that cell, accumulated in double in
    a fixed order that depends on the input order only, divided by the count in double, rounded half to even for integer and bool
    dtypes, then cast to the dtype of ``features``: TWO CALLS GIVE THE SAME BITS (the reference adds with float atomics).  The
    result is detached from ``features``: no gradient flows through the mean.

    On the GPU: one thread per point writes (Morton key, index), a stable radix sort of the pairs over ``3 * level`` bits, run
    heads, a scan and the run starts, the octree build from the sorted keys, and a segmented mean with lanes along the feature
    dimension and no atomics -- ``13 + 4 ceil(3 level / 8) + 4 level`` launches (2 fewer without features; the count per stage is in
    ``_C.ops.conversions.pointcloud_to_spc_cuda``) and ONE host read (the number of cells and the level sizes together).  The call
    synchronises the current stream and cannot be captured in a graph.  CPU tensors run the torch formulation of the same
    contract.

    Args:
        pointcloud (torch.Tensor): half, float or double, of shape :math:`(\text{num_points}, 3)`, any strides.
        level (int): depth of the octree, in :math:`[1, 15]`.
        features (optional, torch.Tensor): per-point features of shape :math:`(\text{num_points}, \text{feat_dim})`, any strides, on
            the same device; bool, uint8, int8, int16, int32, int64, half, float or double.

    Returns:
        (kaolin.rep.Spc): a single-item batch: ``octrees`` on the device of ``pointcloud``, ``lengths`` (1) int32 on the CPU,
        ``features`` (or None).
    """
    fn = 'unbatched_pointcloud_to_spc'
    if not isinstance(pointcloud, torch.Tensor) or pointcloud.dim() != 2 or pointcloud.size(1) != 3 or pointcloud.dtype not in _FLOATS:
        raise ValueError(f'{fn}: pointcloud must be half, float or double, of size (num_points, 3)')
    if isinstance(level, bool) or not isinstance(level, int) or not 1 <= level <= _MAX_LEVEL:
        raise ValueError(f'{fn}: level must be an int in [1, {_MAX_LEVEL}], got {level!r}')
    if pointcloud.size(0) == 0:
        raise ValueError(f'{fn}: no points (an octree has at least its root)')
    if pointcloud.dtype == torch.float16 and level > _MAX_HALF_LEVEL:
        raise ValueError(f'{fn}: half points are taken up to level {_MAX_HALF_LEVEL} (2^level - 1 must be a half), got {level}')
    if features is not None:
        if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.size(1) < 1:
            raise ValueError(f'{fn}: features must be of size (num_points, feat_dim) with feat_dim >= 1')
        if features.size(0) != pointcloud.size(0):
            raise ValueError(f'{fn}: {features.size(0)} feature rows for {pointcloud.size(0)} points')
        if features.device != pointcloud.device:
            raise ValueError(f'{fn}: features are on {features.device}, pointcloud on {pointcloud.device}')
        if features.dtype not in _FEATURE_DTYPES:
            raise ValueError(f'{fn}: features of {features.dtype} are not supported')
        features = features.detach()
    pointcloud = pointcloud.detach()
    if pointcloud.is_cuda:
        if pointcloud.dtype == torch.float16:
            pointcloud = quantize_points(pointcloud, level).contiguous()
        octree, feats = _C.ops.conversions.pointcloud_to_spc_cuda(pointcloud, level, features)
    else:
        octree, feats = _torch_pointcloud_to_spc(pointcloud, level, features)
    return Spc(octrees=octree, lengths=torch.tensor([octree.numel()], dtype=torch.int32), features=feats)
