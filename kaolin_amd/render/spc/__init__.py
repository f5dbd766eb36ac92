"""``kaolin.render.spc``: octree ray tracing and the packed ray reductions (HIP walk and pack kernels of csrc/spc_raytrace.hip on
CUDA tensors, torch formulations of the same contract elsewhere).  The reference's ray generation helpers are not provided."""
from .raytrace import *  # noqa: F401,F403
from . import raytrace  # noqa: F401
