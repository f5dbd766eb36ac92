"""``kaolin.ops.gaussians``: operators on 3D Gaussian splats -- the densifier ``sample_points_in_volume``."""
from .densifier import *  # noqa: F401,F403
from . import densifier  # noqa: F401
