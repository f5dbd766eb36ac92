from .trianglemesh import trianglemeshes_to_voxelgrids, unbatched_mesh_to_spc  # noqa: F401
from . import trianglemesh  # noqa: F401
from .tetmesh import marching_tetrahedra  # noqa: F401
from . import tetmesh  # noqa: F401
from .voxelgrid import voxelgrids_to_cubic_meshes, voxelgrids_to_trianglemeshes  # noqa: F401
from . import voxelgrid  # noqa: F401
from .gaussians import gs_to_voxelgrid  # noqa: F401
from . import gaussians  # noqa: F401
from .pointcloud import pointclouds_to_voxelgrids, unbatched_pointcloud_to_spc  # noqa: F401
from . import pointcloud  # noqa: F401
from .flexicubes import FlexiCubes  # noqa: F401
from . import flexicubes  # noqa: F401
