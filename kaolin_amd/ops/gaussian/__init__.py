"""``kaolin.ops.gaussian``: the reference's second spelling of ``kaolin.ops.gaussians`` (the densifier only)."""
from ..gaussians.densifier import *  # noqa: F401,F403
from ..gaussians import densifier  # noqa: F401
