"""``kaolin.ops.spc``: the structured point cloud operators -- octree build, scan, point generation, query, the dense conversion,
feature grids: the dual octree, trinkets and differentiable trilinear interpolation of corner features, and the sparse
convolutions ``conv3d`` / ``conv_transpose3d`` with their layers (HIP pipelines of csrc/spc.hip, csrc/spc_trilinear.hip and
csrc/spc_conv.hip on CUDA tensors, torch formulations on CPU tensors), and the Bayesian-fusion reconstruction ``bf_recon`` with its
ray-traced depth-map dataset (csrc/spc_bf.hip).  Ray tracing lives in ``kaolin.render.spc``, the data
class in ``kaolin.rep.Spc``."""
from .convolution import *  # noqa: F401,F403
from .points import *  # noqa: F401,F403
from .spc import *  # noqa: F401,F403
from .uint8 import *  # noqa: F401,F403
from . import convolution, points, spc, uint8  # noqa: F401
# as in the reference, the Bayesian-fusion reconstruction and its dataset are sub-modules, not star imports: ``unbatched_query`` of
# this package stays the plain one, ``bf_recon.unbatched_query`` is the empty-aware one
from . import bf_torch, bf_recon, raytraced_spc_dataset  # noqa: F401
