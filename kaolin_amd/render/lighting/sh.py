"""Degree-3 (nine-coefficient) spherical-harmonic lighting, pure torch: a direction's SH coefficients, the irradiance a
nine-coefficient radiance gives a surface through the clamped-cosine convolution, and its Lambertian radiance."""
import math

import torch

__all__ = ['project_onto_sh9', 'sh9_irradiance', 'sh9_diffuse']

_Y00 = 0.28209479177             # 1 / (2 sqrt(pi))
_Y1 = 0.4886025119               # sqrt(3 / (4 pi))
_Y2 = 1.0925484305920792         # sqrt(15 / (4 pi))
_Y20_A, _Y20_B = 0.94617469575, 0.31539156525   # (3 sqrt(5 / (16 pi)), sqrt(5 / (16 pi)))
_Y22 = 0.5462742152960396        # sqrt(15 / (16 pi))
# the clamped cosine's zonal coefficients per band (pi, 2 pi / 3, pi / 4)
_BAND_SCALE = (math.pi,) + (2. * math.pi / 3.,) * 3 + (math.pi / 4.,) * 5


def _sh9_terms(x, y, z, band0):
    return [band0,
            -_Y1 * y, _Y1 * z, -_Y1 * x,
            _Y2 * (x * y), -_Y2 * (y * z), _Y20_A * (z * z) - _Y20_B, -_Y2 * x * z, _Y22 * (x * x - y * y)]


def project_onto_sh9(directions):
    r"""Real spherical-harmonic coefficients of bands 0 to 2 of cartesian directions.

    Args:
        directions (torch.Tensor or list): the directions, of any shape with last dimension 3, or a list of 3 numbers.

    Returns:
        (torch.Tensor): the 9 coefficients along the last dimension, of shape ``directions.shape[:-1] + (9,)``
        (shape :math:`(9,)` for a list).
    """
    if isinstance(directions, torch.Tensor):
        assert directions.shape[-1] == 3
        x, y, z = directions[..., 0:1], directions[..., 1:2], directions[..., 2:3]
        return torch.cat(_sh9_terms(x, y, z, torch.full_like(x, _Y00)), dim=-1)
    if isinstance(directions, list):
        assert len(directions) == 3
        x, y, z = directions
        return torch.tensor(_sh9_terms(x, y, z, _Y00))
    raise TypeError(f'directions is a {type(directions)}, must be a list or a torch.Tensor')


def sh9_irradiance(lights, normals):
    r"""Irradiance at surface points from a nine-coefficient spherical-harmonic radiance, the clamped cosine lobe being
    expressed in the same basis.

    Args:
        lights (torch.Tensor): the radiance's coefficients (see :func:`project_onto_sh9`), of shape :math:`(9,)`.
        normals (torch.Tensor): the surface normals, of shape :math:`(\text{num_points}, 3)`.

    Returns:
        (torch.Tensor): the irradiance, of shape :math:`(\text{num_points},)`.
    """
    assert lights.shape == (9,)
    assert normals.ndim == 2 and normals.shape[-1] == 3
    bands = project_onto_sh9(normals)
    scale = torch.tensor(_BAND_SCALE, dtype=bands.dtype, device=bands.device)
    return torch.sum(bands * scale * lights.unsqueeze(-2), dim=-1).reshape(*normals.shape[:-1])


def sh9_diffuse(directions, normals, albedo):
    r"""Lambertian radiance at surface points lit by the spherical-harmonic projection of one direction.

    Args:
        directions (torch.Tensor): the light direction, of shape :math:`(3,)`.
        normals (torch.Tensor): the surface normals, of shape :math:`(\text{num_points}, 3)`.
        albedo (torch.Tensor): the surface albedo (RGB), of shape :math:`(\text{num_points}, 3)`.

    Returns:
        (torch.Tensor): the radiance, of the shape of ``albedo``.
    """
    assert directions.shape == (3,)
    assert normals.ndim == 2 and normals.shape[1] == 3
    assert normals.shape == albedo.shape
    irradiance = sh9_irradiance(project_onto_sh9(directions), normals)
    return albedo * irradiance.unsqueeze(-1)
