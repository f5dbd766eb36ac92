"""``kaolin.ops.spc``: the structured point cloud operators -- octree build, scan, point generation, query, the dense conversion,
feature grids: the dual octree, trinkets and differentiable trilinear interpolation of corner features, and the sparse
convolutions ``conv3d`` / ``conv_transpose3d`` with their layers (HIP pipelines of csrc/spc.hip, csrc/spc_trilinear.hip and
csrc/spc_conv.hip on CUDA tensors, torch formulations on CPU tensors).  Ray tracing lives in ``kaolin.render.spc``, the data
class in ``kaolin.rep.Spc``."""
from .convolution import *  # noqa: F401,F403
from .points import *  # noqa: F401,F403
from .spc import *  # noqa: F401,F403
from .uint8 import *  # noqa: F401,F403
from . import convolution, points, spc, uint8  # noqa: F401
