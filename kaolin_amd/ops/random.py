"""``kaolin.ops.random``: the sampling helper the Gaussian densifier needs (reference: kaolin/ops/random.py)."""
import math

import torch

__all__ = ['sample_spherical_coords']


def sample_spherical_coords(shape, azimuth_low=0., azimuth_high=math.pi * 2., elevation_low=0., elevation_high=math.pi * 0.5,
                            device='cpu', dtype=torch.float):
    """(azimuth, elevation), both of ``shape``, uniform on the sphere patch between the bounds (radians): the azimuth is uniform,
    the elevation is the arcsine of a uniform sample between the sines of its bounds."""
    rand = torch.rand([2, *shape], dtype=dtype, device=device)
    azimuth = azimuth_low + rand[0] * (azimuth_high - azimuth_low)
    sin_low, sin_high = math.sin(elevation_low), math.sin(elevation_high)
    elevation = torch.asin(sin_low + rand[1] * (sin_high - sin_low))
    return azimuth, elevation
