"""``kaolin.ops.spc`` points: quantisation, Morton codes, corners and the octree of a point set (reference:
kaolin/ops/spc/points.py).  CUDA tensors run the HIP kernels of csrc/spc.hip through ``_C.ops.spc``; CPU tensors (which the
reference rejects) run the ``_torch_*`` formulations of the same pipelines below -- also the yardstick of tools/time_spc.py."""
import torch

from ... import _C

__all__ = ['points_to_morton', 'morton_to_points', 'points_to_corners', 'unbatched_points_to_octree', 'quantize_points',
           'create_dense_spc']

_COORD_BITS = 15        # KAOLIN_SPC_MAX_LEVELS: bits of a coordinate in a Morton code


def quantize_points(x, level):
    """Float coordinates in [-1, 1] (last dimension 3) -> int16 coordinates in [0, 2^level - 1]; points outside are clipped."""
    res = 2 ** level
    return torch.floor(torch.clamp(res * (x + 1.0) / 2.0, 0, res - 1.)).short()


def _torch_points_to_morton(points):
    p = points.long()
    x, y, z = p[..., 0], p[..., 1], p[..., 2]
    code = torch.zeros_like(x)
    for i in range(_COORD_BITS):
        code |= ((z >> i) & 1) << (3 * i)
        code |= ((y >> i) & 1) << (3 * i + 1)
        code |= ((x >> i) & 1) << (3 * i + 2)
    return code


def _torch_morton_to_points(morton):
    x, y, z = torch.zeros_like(morton), torch.zeros_like(morton), torch.zeros_like(morton)
    for i in range(_COORD_BITS):
        z |= ((morton >> (3 * i)) & 1) << i
        y |= ((morton >> (3 * i + 1)) & 1) << i
        x |= ((morton >> (3 * i + 2)) & 1) << i
    return torch.stack([x, y, z], dim=-1).short()


def _torch_morton_to_octree(morton, level):
    """Morton codes (N), any order, duplicates allowed -> octree bytes, levels root first: unique codes, then per level the
    unique parents and the OR of their children's bits."""
    cur = torch.unique(morton & ((1 << (3 * level)) - 1))
    levels = []
    for _ in range(level):
        parents, inverse = torch.unique(cur >> 3, return_inverse=True)
        byte = torch.zeros(parents.numel(), dtype=torch.long, device=morton.device)
        byte.scatter_add_(0, inverse, torch.bitwise_left_shift(torch.ones_like(cur), cur & 7))     # children are distinct: + is |
        levels.append(byte.byte())
        cur = parents
    return torch.cat(levels[::-1]) if levels else torch.empty(0, dtype=torch.uint8, device=morton.device)


def points_to_morton(points):
    """Quantised points (..., 3) int16 -> Morton codes (...) int64: bit 3i = z_i, 3i + 1 = y_i, 3i + 2 = x_i."""
    shape = list(points.shape)[:-1]
    points = points.reshape(-1, 3)
    if points.is_cuda:
        return _C.ops.spc.points_to_morton_cuda(points.contiguous()).reshape(*shape)
    return _torch_points_to_morton(points).reshape(*shape)


def morton_to_points(morton):
    """Morton codes (...) int64 -> quantised points (..., 3) int16."""
    shape = list(morton.shape) + [3]
    morton = morton.reshape(-1)
    if morton.is_cuda:
        return _C.ops.spc.morton_to_points_cuda(morton.contiguous()).reshape(*shape)
    return _torch_morton_to_points(morton).reshape(*shape)


_CORNERS = ((0, 0, 0), (0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1))


def _torch_points_to_corners(points):
    return points.unsqueeze(-2) + torch.tensor(_CORNERS, dtype=points.dtype, device=points.device)


def points_to_corners(points):
    """Quantised points (..., 3) int16 -> the 8 corners of their cells (..., 8, 3), corner j = point + (j >> 2, (j >> 1) & 1, j & 1)."""
    shape = list(points.shape)
    shape.insert(-1, 8)
    if points.is_cuda:
        return _C.ops.spc.points_to_corners_cuda(points.reshape(-1, 3).contiguous()).reshape(*shape)
    return _torch_points_to_corners(points)


def unbatched_points_to_octree(points, level, sorted=False):
    """Quantised points (N, 3) int16 of ``level`` -> octree (num_bytes) uint8, levels root first.

    ``sorted=False``: any order, duplicates allowed (on the GPU: Morton codes, a radix sort over their 3 * level bits, unique, then
    every level bottom-up on the device; one host read of the level sizes).  ``sorted=True`` promises unique points in Morton
    order and skips the sort; the result for any other input is unspecified.  ``N = 0`` raises ValueError (the reference reads
    out of bounds); ``level = 0`` returns an empty tensor."""
    if points.dim() != 2 or points.size(1) != 3 or points.dtype != torch.int16:
        raise ValueError(f'unbatched_points_to_octree: points must be short, of size (num_points, 3), got {points.dtype} '
                         f'{tuple(points.shape)}')
    if points.size(0) == 0:
        raise ValueError('unbatched_points_to_octree: no points (an octree has at least its root)')
    level = int(level)
    if not 0 <= level <= _COORD_BITS:
        raise ValueError(f'unbatched_points_to_octree: level must be in [0, {_COORD_BITS}], got {level}')
    if level == 0:
        return torch.empty(0, dtype=torch.uint8, device=points.device)
    if points.is_cuda:
        return _C.ops.spc.points_to_octree(points.contiguous(), level, sorted=bool(sorted))
    return _torch_morton_to_octree(_torch_points_to_morton(points), level)


def create_dense_spc(level, device):
    """-> (octree, lengths) of the full octree of ``level``: every byte 255, sum of 8^l for l < level bytes; lengths (1) int32 CPU."""
    lengths = torch.tensor([sum(8 ** l for l in range(level))], dtype=torch.int32)
    octree = torch.full((int(lengths[0]),), 255, device=device, dtype=torch.uint8)
    return octree, lengths
