"""kaolin_amd -- MI355X-native (gfx950) implementation of Kaolin's DIB-R
differentiable-rasterization and 3D-metrics hot path behind Kaolin's own Python API.

    kaolin_amd.render.mesh      rasterize, dibr_soft_mask, dibr_rasterization (+ helpers)
    kaolin_amd.metrics          pointcloud.{sided_distance, chamfer_distance, f_score},
                                trianglemesh.point_to_mesh_distance, render.mask_iou
    kaolin_amd.ops.conversions  trianglemeshes_to_voxelgrids, marching_tetrahedra (HIP extraction pipeline),
                                voxelgrids_to_cubic_meshes (sort-free HIP pipeline), voxelgrids_to_trianglemeshes (marching
                                cubes: batched, differentiable HIP pipeline over a generated case table), pointclouds_to_voxelgrids,
                                FlexiCubes (differentiable dual marching cubes: HIP pipeline, forward and backward),
                                unbatched_pointcloud_to_spc (HIP pair sort + atomic-free segmented mean)
    kaolin_amd.ops.mesh         subdivide_tetmesh (HIP edge-midpoint pipeline), inverse_vertices_offset, check_sign,
                                subdivide_trianglemesh (Loop subdivision with a per-vertex alpha, HIP pipeline),
                                average_face_vertex_features, compute_vertex_normals, vertex_tangents (one deterministic HIP gather
                                over cached vertex -> corner lists, the bits of the reference's CPU result), unindex_vertices_by_faces,
                                face_areas, sample_points and their packed forms (HIP areas, float64 scan, search-and-blend)
    kaolin_amd.ops.spc          the SPC core: scan_octrees, generate_points, unbatched_query, to_dense, unbatched_points_to_octree (HIP),
                                conv3d / conv_transpose3d and their layers (HIP neighbour map + MFMA gather-GEMM)
    kaolin_amd.ops.spc.bf_recon bf_recon, fuseBF, the empty-aware unbatched_query (HIP operators of csrc/spc_bf.hip)
    kaolin_amd.ops.gaussians    sample_points_in_volume: fills a shell of Gaussian splats (also as kaolin_amd.ops.gaussian);
                                transform_gaussians, transform_shs: a rigid / similarity transform of a splat model with its SH
                                rotated (one fused HIP kernel per direction, exact Ivanic-Ruedenberg coefficients)
    kaolin_amd.math.quat        quat_from_rot33, quat_mul, quat_unit (xyzw, plain torch): what the transforms need of kaolin.math
    kaolin_amd.rep              Spc, the structured point cloud data class
    kaolin_amd.ops.voxelgrid    fill (HIP flood fill over bit grids), downsample, extract_surface, extract_odms, project_odms
    kaolin_amd.metrics.voxelgrid  iou
    kaolin_amd.metrics.tetmesh  tetrahedron_volume, equivolume, amips (fused HIP kernels, atomic-free reductions)
    kaolin_amd.render.lighting  spherical-gaussian (HIP reduced inner product) and spherical-harmonic shading
    kaolin_amd.render.spc       unbatched_raytrace (HIP depth-first octree walk), mark_pack_boundaries, diff, cumsum, cumprod,
                                sum_reduce, prod_reduce, exponential_integration (HIP pack scans and reductions)
    kaolin_amd._C               the 8 operator bindings of ``kaolin._C`` on this path
    kaolin_amd.distributed      batch/view sharding over RCCL (new; the reference has none)

``kaolin_amd.install_as_kaolin()`` registers the package under the name ``kaolin`` so that
existing notebooks/tests written against the reference import it unchanged.
"""
import sys

from . import _C  # noqa: F401
from . import io, math, metrics, ops, render, rep, utils  # noqa: F401
from . import distributed  # noqa: F401

__version__ = '0.1.0'


def install_as_kaolin():
    """Alias this package (and the submodules on the hot path) as ``kaolin`` in sys.modules."""
    prefix = __name__ + '.'
    for name, mod in list(sys.modules.items()):
        if name == __name__:
            sys.modules['kaolin'] = mod
        elif name.startswith(prefix):
            sys.modules['kaolin.' + name[len(prefix):]] = mod
    return sys.modules['kaolin']
