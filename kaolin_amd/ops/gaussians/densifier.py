"""``kaolin.ops.gaussians.sample_points_in_volume``: points inside a shape given as a shell of 3D Gaussian splats (reference:
kaolin/ops/gaussians/densifier.py).

The shell is voxelised (``gs_to_voxelgrid``), ray traced into depth maps from viewpoints around it (``RayTracedSPCDataset``), and
the depth maps are fused into an SPC that tells empty, occupied and unseen space apart (``bf_recon``); the occupied and the unseen
cells are the solid.  The reference ends by querying all 8^level cells of a dense grid -- 2^30 int16 points and an int64 arange
of 8.6 GB at level 10; here ``bf_cells_cuda`` enumerates the same cells, in the same order, with work proportional to their number."""
import logging
import math

import numpy as np
import torch

from ..conversions import gs_to_voxelgrid
from ..random import sample_spherical_coords
from ..spc import bf_recon as bf_recon_module
from ..spc import unbatched_points_to_octree
from ..spc.bf_recon import bf_recon
from ..spc.raytraced_spc_dataset import RayTracedSPCDataset

logger = logging.getLogger(__name__)

__all__ = ['sample_points_in_volume']

_FAILURE = ("3D Gaussian densifier failed to produce a voxelized volume out of the shape.\n"
            "Usually, it means the shape represented by 3D Gaussians has regions of very low "
            "quality which resulted in holes in the shell. \n"
            "To fix this issue, double check your shape, "
            "or try adjusting args passed to the volume sampling function.\n"
            "For example, try reducing the opacity_threshold towards 0.0, or octree_level towards 7 or 6.")


def _generate_default_viewpoints():
    """The default viewpoints that carve the seen space: 14 anchors on the axes and the cube diagonals, an icosahedron, and five
    rotated and scaled copies of it, each perturbed by less than 0.0005 (empirical choices of the reference)."""
    a, b = 4.0, 2.3
    anchors = torch.tensor([[a, 0, 0], [0, a, 0], [0, 0, a], [-a, 0, 0], [0, -a, 0], [0, 0, -a],
                            [b, b, b], [-b, b, b], [b, -b, b], [b, b, -b], [-b, -b, b], [-b, b, -b], [b, -b, -b], [-b, -b, -b]])
    phi = (1 + math.sqrt(5.0)) / 2
    icosahedron = torch.tensor([[+phi, +1, 0], [+phi, -1, 0], [-phi, -1, 0], [-phi, +1, 0], [+1, 0, +phi], [-1, 0, +phi],
                                [-1, 0, -phi], [+1, 0, -phi], [0, +phi, +1], [0, +phi, -1], [0, -phi, -1], [0, -phi, +1]])
    tx, ty, tz = (math.radians(d) for d in (15, 27, 49))
    R_x = torch.tensor([[1.0, 0.0, 0.0], [0.0, np.cos(tx), -np.sin(tx)], [0.0, np.sin(tx), np.cos(tx)]])
    R_y = torch.tensor([[np.cos(ty), 0.0, np.sin(ty)], [0.0, 1.0, 0.0], [-np.sin(ty), 0.0, np.cos(ty)]])
    R_z = torch.tensor([[np.cos(tz), -np.sin(tz), 0.0], [np.sin(tz), np.cos(tz), 0.0], [0.0, 0.0, 1.0]])
    R = (R_z @ R_y @ R_x).float()
    views, rot = [anchors, icosahedron], torch.eye(3)
    for k in range(2, 7):
        rot = rot @ R
        views.append((k * icosahedron) @ rot.T)
    viewpoints = torch.cat(views, dim=0)
    return viewpoints + 0.001 * (0.5 - torch.rand(viewpoints.shape))


def _jitter(pts, octree_level):
    """Every point moved by a random offset: its direction from ``sample_spherical_coords`` over the whole sphere, its length
    ``size * sqrt(u)`` with ``u`` uniform and ``size = 2 / 2^octree_level``, the side of a cell of the [-1, 1] cube."""
    count = pts.shape[0]
    size = 2.0 ** (1 - octree_level)
    length = size * torch.rand(count, device=pts.device).sqrt()
    azimuth, elevation = sample_spherical_coords((count,), 0., 2. * math.pi, -0.5 * math.pi, 0.5 * math.pi,
                                                 device=pts.device, dtype=pts.dtype)
    direction = torch.stack([elevation.sin() * azimuth.cos(), elevation.sin() * azimuth.sin(), elevation.cos()], dim=1)
    return pts + length.unsqueeze(1) * direction


def _solidify(xyz, scales, rots, opacities, opacity_threshold, gs_level, query_level, viewpoints, scaling_activation,
              scaling_inverse_activation):
    """Gaussians -> (K, 3) cell centres of level ``query_level`` inside the shape, in the Gaussians' frame; (0, 3) and a warning
    when the shell leaves nothing to fill."""
    device = xyz.device
    pmin, pmax = torch.min(xyz, dim=0)[0], torch.max(xyz, dim=0)[0]
    cen = 0.5 * (pmin + pmax)
    dmax = 0.5 * torch.max(pmax - pmin) + 0.05              # half the largest extent, and room for the covariances
    # the Gaussians in [-1, 1]^3
    xyz = (xyz - cen) / dmax
    scales = scaling_activation(scaling_inverse_activation(1. / dmax).unsqueeze(0) + scaling_inverse_activation(scales))
    voxels, merged_opacities = gs_to_voxelgrid(xyz, scales, rots, opacities, gs_level, iso=11.345, tol=0.125, step=10)
    voxels = voxels[merged_opacities >= opacity_threshold].contiguous()
    bf_octree = bf_empty = None
    if voxels.size(0) > 0:
        gs_octree = unbatched_points_to_octree(voxels, gs_level)
        dataset = RayTracedSPCDataset(viewpoints.contiguous(), gs_octree.contiguous())
        bf_octree, bf_empty, _, _ = bf_recon(dataset, final_level=query_level, sigma=0.0005)
    if bf_octree is None or bf_empty is None or len(bf_octree) == 0 or len(bf_empty) == 0:
        logging.warning(_FAILURE)
        return xyz.new_empty([0, 3])
    # the occupied and the unseen cells of the level, in Morton order: the solid
    cells = bf_recon_module._ops(bf_octree).bf_cells_cuda(bf_octree, bf_empty, query_level)
    sample_points = 2 ** (1 - query_level) * cells - torch.ones(3, device=device)
    return dmax * sample_points + cen


@torch.no_grad()
def sample_points_in_volume(xyz, scale, rotation, opacity, mask=None, num_samples=None, octree_level=8, opacity_threshold=0.35,
                            post_scale_factor=1.0, jitter=True, clip_samples_to_input_bbox=True, viewpoints=None,
                            scaling_activation=None, scaling_inverse_activation=None):
    r"""Samples points inside a shape represented by 3D Gaussian splats, which only cover its shell.

    xyz (N, 3): the means; scale (N, 3): the post-activation scales; rotation (N, 4): quaternions; opacity (N) or (N, 1).
    mask (N) bool: the Gaussians to use (default all).  num_samples: an upper cap on the points returned, subsampled at random.
    octree_level in [6, 10]: the resolution of the fill, one point per cell.  opacity_threshold: voxels of the shell with less
    accumulated opacity are culled.  post_scale_factor < 1 shrinks the result around its mean.  jitter: perturb every point by
    at most a cell.  clip_samples_to_input_bbox: drop points outside the bounding box of the means.  viewpoints (C, 3): the
    camera positions, looking at the centre, that carve the seen space (default: ``_generate_default_viewpoints``).
    scaling_activation / scaling_inverse_activation: default exp / log.

    -> (K, 3) points.  When the shell has holes, or nothing survives the threshold, a warning is logged and (0, 3) is returned."""
    assert octree_level >= 6 and octree_level <= 10, \
        'octree_level range supported is in [6, 10]. \n' \
        'Higher values, while generating more points within the shape volume, ' \
        'require more memory and may suffer from holes in the shape shell.'
    if opacity.ndim == 2:
        opacity = opacity.squeeze(1)
    if viewpoints is None:
        viewpoints = _generate_default_viewpoints()
    if scaling_activation is None:
        scaling_activation = torch.exp
    if scaling_inverse_activation is None:
        scaling_inverse_activation = torch.log
    device = xyz.device
    mask = mask.to(device=device).clone() if mask is not None else xyz.new_ones((xyz.shape[0],), device=device, dtype=torch.bool)
    xyz, scale, rotation, opacity = xyz[mask].clone(), scale[mask].clone(), rotation[mask].clone(), opacity[mask].clone()
    volume_pts = _solidify(xyz.contiguous(), scale.contiguous(), rotation.contiguous(), opacity.contiguous(),
                           opacity_threshold=opacity_threshold, gs_level=octree_level, query_level=octree_level,
                           viewpoints=viewpoints, scaling_activation=scaling_activation,
                           scaling_inverse_activation=scaling_inverse_activation)
    if volume_pts.shape[0] == 0:        # nothing to fill (the warning is logged): no post-processing
        return volume_pts
    if jitter:
        volume_pts = _jitter(volume_pts, octree_level)
    if post_scale_factor < 1.0:         # shrink around the mean
        centre = volume_pts.mean(dim=0, keepdim=True)
        volume_pts = centre + post_scale_factor * (volume_pts - centre)
    if clip_samples_to_input_bbox:      # keep what lies strictly inside the box of the means
        inside = ((volume_pts > xyz.amin(dim=0)) & (volume_pts < xyz.amax(dim=0))).all(dim=1)
        volume_pts = volume_pts[inside]
    if num_samples is not None and num_samples < volume_pts.shape[0]:
        volume_pts = volume_pts[torch.randperm(volume_pts.shape[0])[:num_samples]]
    return volume_pts
