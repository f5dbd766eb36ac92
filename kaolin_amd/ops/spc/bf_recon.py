"""``kaolin.ops.spc.bf_recon``: reconstruction of an object from calibrated RGB-D frames by Bayesian fusion of occupancy
probabilities (reference: kaolin/ops/spc/bf_recon.py; the method: "A Closed-Form Bayesian Fusion Equation Using Occupancy
Probabilities", 3DV 2016).  The result is an SPC that knows about empty space: an octree and an ``empty`` tensor in bit-to-bit
correspondence; a cell whose octree bit is clear is unseen (inside the object) when its empty bit is set and empty space when not.

CUDA tensors run the operators of csrc/spc_bf.hip through ``_C.ops.spc``, in the reference's sequence; CPU tensors (which the
reference rejects) run the torch formulations of ``bf_torch``.  ``extractBQ`` and its three operators are not built: the
reference's ``bf_recon`` has the call commented out."""
import numpy as np
import torch

from ... import _C
from . import bf_torch
from .spc import _check_exsum, scan_octrees
from .points import morton_to_points

__all__ = ['BFReconstructionTerminatedException', 'processFrame', 'fuseBF', 'bf_recon', 'unbatched_query']


class BFReconstructionTerminatedException(Exception):
    """Raised inside bf_recon when a frame or a fusion leaves nothing occupied (bad inputs)."""
    pass


def _ops(t):
    """the operator table of the tensor's device (looked up per call, so that a wrapper put around ``_C.ops.spc`` sees every call)"""
    return _C.ops.spc if t.is_cuda else bf_torch.ops


def _assemble(ops, level, vcnt, Sta, Nvs, device, check_levels):
    """Bottom-up: the states of the voxels of every level -> octree and empty bytes, root first, compacted to the occupied nodes."""
    init_size = int(vcnt[1:].sum()) >> 3
    octree = torch.zeros(init_size, dtype=torch.uint8, device=device)
    empty = torch.zeros(init_size, dtype=torch.uint8, device=device)
    occupancies = torch.zeros(init_size, dtype=torch.int32, device=device)
    num_nodes = int(vcnt[level]) >> 3
    total_nodes = num_nodes
    for l in range(level, 0, -1):
        octree, empty, occupancies = ops.process_final_voxels(num_nodes, total_nodes, Sta[l], Nvs[l - 1], occupancies, Sta[l - 1],
                                                              octree, empty)
        if check_levels:
            insum = ops.inclusive_sum(occupancies)
            if insum[-1].item() == 0:
                raise BFReconstructionTerminatedException()
        num_nodes = int(vcnt[l - 1]) >> 3
        total_nodes += num_nodes
    insum = ops.inclusive_sum(occupancies)
    if insum[-1].item() == 0:
        raise BFReconstructionTerminatedException()
    octree, empty = ops.compactify_nodes(total_nodes, insum, octree, empty)
    level, pyramid, exsum = scan_octrees(octree, torch.tensor([len(octree)], dtype=torch.int))
    return octree, empty, level, pyramid, exsum


def _dense_levels(start_level, device, with_occupancy):
    """the levels above start_level: dense, every voxel occupied"""
    Occ, Sta, Nvs = [], [], []
    for l in range(start_level):
        num = 8 ** l
        if with_occupancy:
            Occ.append(torch.ones(num, dtype=torch.int32, device=device))
        Sta.append(torch.full((num,), 2, dtype=torch.int32, device=device))
        Nvs.append(torch.arange(num, dtype=torch.int32, device=device))
    return Occ, Sta, Nvs


def processFrame(batch, level, sigma):
    """One calibrated RGB-D frame (an item of RayTracedSPCDataset) -> the empty-aware SPC of what the frame sees, as a dict with
    'octree', 'empty', 'level', 'pyramid', 'exsum', 'probabilities', 'colors', 'normals'.  ``batch[1]``, the depth map, is converted
    to z depth in place when ``batch[6]`` (true_depth) is set.  Per level below start_level: an oracle, a scan, a host read and a
    subdivision; then the final probabilities, colours and normals and the bottom-up assembly."""
    image = batch[0].contiguous()
    depth_map = batch[1].contiguous()
    camera, intrinsics, max_depth, mip_levels, true_depth, start_level, points = batch[2:9]
    device = points.device
    ops = _ops(points)
    mips = ops.build_mip2d(depth_map, intrinsics, mip_levels, max_depth, true_depth).contiguous()
    Occ, Sta, Nvs = _dense_levels(start_level, device, True)
    vcnt = np.zeros(level + 1, dtype=np.int64)
    for l in range(start_level):
        vcnt[l] = 8 ** l
    for l in range(start_level, level):
        vcnt[l] = points.size(0)
        occupancies, empty_state = ops.oracleB(points, l, sigma, camera, depth_map, mips, mip_levels)
        insum = ops.inclusive_sum(occupancies)
        if insum[-1].item() == 0:
            raise BFReconstructionTerminatedException()
        points, nvsum = ops.subdivide(points, insum)
        Occ.append(occupancies)
        Sta.append(empty_state)
        Nvs.append(nvsum)
    vcnt[level] = points.size(0)
    occupancies, empty_state, probabilities = ops.oracleB_final(points, level, sigma, camera, depth_map)
    insum = ops.inclusive_sum(occupancies)
    if insum[-1].item() == 0:
        raise BFReconstructionTerminatedException()
    points, nvsum = ops.compactify(points, insum)
    probabilities = probabilities[nvsum]
    colors, normals = ops.colorsB_final(points, level, camera, sigma, image, depth_map, probabilities)
    Occ.append(occupancies)
    Sta.append(empty_state)
    octree, empty, level, pyramid, exsum = _assemble(ops, level, vcnt, Sta, Nvs, device, False)
    return {'octree': octree, 'empty': empty, 'level': level, 'pyramid': pyramid, 'exsum': exsum, 'probabilities': probabilities,
            'colors': colors, 'normals': normals}


def fuseBF(spc0, spc1):
    """Two empty-aware SPCs of the same depth (dicts of processFrame / fuseBF) -> their fusion: a cell is empty where either says
    empty, unseen where both say unseen, occupied otherwise, with probability p0 p1 / (p0 p1 + (1 - p0)(1 - p1))."""
    device = spc0['octree'].device
    ops = _ops(spc0['octree'])
    start_level = 4
    points = morton_to_points(torch.arange(8 ** start_level, device=device))
    level = spc0['level']
    _, Sta, Nvs = _dense_levels(start_level, device, False)
    vcnt = np.zeros(level + 1, dtype=np.int64)
    for l in range(start_level):
        vcnt[l] = 8 ** l
    for l in range(start_level, level):
        vcnt[l] = points.size(0)
        occupancies, empty_state = ops.merge_empty(points, l, spc0['octree'], spc1['octree'], spc0['empty'], spc1['empty'],
                                                   spc0['exsum'], spc1['exsum'])
        if occupancies.max().item() == 0:
            raise BFReconstructionTerminatedException()
        insum = ops.inclusive_sum(occupancies)
        points, nvsum = ops.subdivide(points, insum)
        Sta.append(empty_state)
        Nvs.append(nvsum)
    vcnt[level] = points.size(0)
    occupancies, empty_state, probabilities, colors, normals = ops.bq_merge(
        points, level, spc0['octree'], spc1['octree'], spc0['empty'], spc1['empty'], spc0['pyramid'], spc1['pyramid'],
        spc0['probabilities'], spc1['probabilities'], spc0['colors'], spc1['colors'], spc0['normals'], spc1['normals'],
        spc0['exsum'], spc1['exsum'])
    if occupancies.max().item() == 0:
        raise BFReconstructionTerminatedException()
    insum = ops.inclusive_sum(occupancies)
    points, nvsum = ops.compactify(points, insum)
    probabilities, colors, normals = probabilities[nvsum], colors[nvsum], normals[nvsum]
    Sta.append(empty_state)
    octree, empty, level, pyramid, exsum = _assemble(ops, level, vcnt, Sta, Nvs, device, True)
    return {'octree': octree, 'empty': empty, 'level': level, 'pyramid': pyramid, 'exsum': exsum, 'probabilities': probabilities,
            'colors': colors, 'normals': normals}


def bf_recon(input_dataset, final_level, sigma):
    r"""Reconstructs an object from a collection of calibrated RGB-D images (3DV 2016, "A Closed-Form Bayesian Fusion Equation
    Using Occupancy Probabilities").

    input_dataset: an iterable of the ten-tuples of :class:`RayTracedSPCDataset` (an item whose last entry is False -- no ray hit
    anything -- is skipped); final_level: the depth of the result; sigma: roughly the noise level of the depths.

    -> (octree (num_bytes) uint8, empty (num_bytes) uint8 in bit-to-bit correspondence with it, colors (n, 4) uint8 and normals
    (n, 3) float of the points of final_level), or four ``None`` when a frame or a fusion leaves nothing occupied."""
    try:
        spc0 = {'octree': None, 'empty': None, 'colors': None, 'normals': None}
        first_frame_processed = False
        for batch in input_dataset:
            if not batch[9]:
                continue
            if not first_frame_processed:
                spc0 = processFrame(batch, final_level, sigma)
            else:
                spc0 = fuseBF(spc0, processFrame(batch, final_level, sigma))
            first_frame_processed = True
        return spc0['octree'], spc0['empty'], spc0['colors'], spc0['normals']
    except BFReconstructionTerminatedException:
        return None, None, None, None


def unbatched_query(octree, empty, exsum, query_coords, level):
    """The state of every coordinate in an empty-aware SPC -> int64 (Q): >= 0 the index in the point hierarchy of the point of
    ``level`` that holds it, -1 empty space (or outside the cube), ``-2 - depth`` unseen space, where ``depth`` counts the levels
    left below the node at which the walk stopped.

    octree, empty (num_bytes) uint8 and exsum (num_bytes) int32; query_coords (Q, 3): floating point (half / float / double) in
    [-1, 1], or integer in [0, 2^level], converted with ``(q.float() / 2**level) * 2 - 1``.  Quantised as
    ``floor(2^level (q / 2 + 1 / 2))`` in double.  On the GPU: one launch, no host read: graph-capturable."""
    _check_exsum('unbatched_query', exsum, octree.numel())
    level = int(level)
    if not 0 <= level <= 15:
        raise ValueError(f'unbatched_query: level must be in [0, 15], got {level}')
    if empty.numel() != octree.numel():
        raise ValueError(f'unbatched_query: empty has {empty.numel()} bytes, octree {octree.numel()}')
    coords = query_coords if query_coords.is_floating_point() else (query_coords.float() / (2 ** level)) * 2.0 - 1.0
    if coords.dtype not in (torch.float16, torch.float32, torch.float64):
        coords = coords.float()
    return _ops(octree).query_cuda_empty(octree.contiguous(), empty.contiguous(), exsum.contiguous(), coords.contiguous(),
                                         level).long()
