"""``kaolin.ops.spc``: the structured point cloud operators -- octree build, scan, point generation, query, the dense conversion,
and feature grids: the dual octree, trinkets and differentiable trilinear interpolation of corner features (HIP pipelines of
csrc/spc.hip and csrc/spc_trilinear.hip on CUDA tensors, torch formulations on CPU tensors).  Ray tracing lives in
``kaolin.render.spc``.  Convolutions and ``kaolin.rep.Spc`` are not part of this package."""
from .points import *  # noqa: F401,F403
from .spc import *  # noqa: F401,F403
from .uint8 import *  # noqa: F401,F403
from . import points, spc, uint8  # noqa: F401
