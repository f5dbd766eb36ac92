"""``kaolin.ops.spc``: the core of the structured point cloud operators -- octree build, scan, point generation, query and the
dense conversion (HIP pipelines of csrc/spc.hip on CUDA tensors, torch formulations on CPU tensors).  Ray tracing lives in
``kaolin.render.spc``.  Convolutions, dual octrees and trinkets, trilinear interpolation and ``kaolin.rep.Spc`` are not part of
this package."""
from .points import *  # noqa: F401,F403
from .spc import *  # noqa: F401,F403
from .uint8 import *  # noqa: F401,F403
from . import points, spc, uint8  # noqa: F401
