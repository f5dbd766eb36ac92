"""Lighting of rendered surfaces (``kaolin.render.lighting``): spherical gaussians (DIB-R++ diffuse and specular
shading, with the reduced SG inner product on native HIP kernels) and degree-3 spherical harmonics (pure torch)."""
from .sh import *  # noqa: F401,F403
from .sg import *  # noqa: F401,F403
from . import sg, sh  # noqa: F401

__all__ = [k for k in list(locals().keys()) if not k.startswith('_')]
