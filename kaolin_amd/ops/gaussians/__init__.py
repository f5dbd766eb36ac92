"""``kaolin.ops.gaussians``: operators on 3D Gaussian splats -- the densifier ``sample_points_in_volume`` and the transforms
``transform_gaussians`` / ``transform_shs``."""
from .densifier import *  # noqa: F401,F403
from .transforms import *  # noqa: F401,F403
from . import densifier  # noqa: F401
from . import transforms  # noqa: F401
