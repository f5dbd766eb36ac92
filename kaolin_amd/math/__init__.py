"""``kaolin.math``: the part of it that ``ops.gaussians.transforms`` needs -- ``quat`` with ``quat_from_rot33``, ``quat_mul`` and
``quat_unit``.  Plain torch, any device and floating dtype, differentiable."""
from . import quat  # noqa: F401
