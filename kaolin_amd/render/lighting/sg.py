r"""Spherical-gaussian (SG) lighting: lights as SG lobes :math:`a\,e^{s(\mu \cdot v - 1)}`, the Lambertian (diffuse) and
Cook-Torrance (specular, DIB-R++) radiance they give a surface, and the SG inner product these rest on.

The reduced inner product -- the SG inner product of every row lobe with every light, summed over the lights -- runs on
the HIP kernels of csrc/sg_lighting.hip for tensors on the GPU, for every number of lights (the reference takes its fused
op only from 8 lights up and the broadcast torch form below that).  On the CPU it is the broadcast torch form.  The
diffuse functions hand the kernels the cosine lobe as two constants and the normals, without materialising the lobe.
"""
from collections.abc import Iterable
import math

import torch

from ... import _C

__all__ = [
    'sg_diffuse_inner_product',
    'sg_diffuse_fitted',
    'sg_warp_specular_term',
    'fresnel',
    'sg_distribution_term',
    'sg_warp_distribution',
    'cosine_lobe_sg',
    'approximate_sg_integral',
    'sg_irradiance_fitted',
    'sg_irradiance_inner_product',
    'SgLightingParameters',
    'sg_from_sun',
    'sg_direction_from_azimuth_elevation',
]

# cosine_lobe_sg: the clamped cosine max(n . v, 0) fitted by one SG lobe
_COSINE_LOBE_AMPLITUDE = 1.17
_COSINE_LOBE_SHARPNESS = 2.133


def _as_tensor(val, shape, device=None, dtype=torch.float):
    """A tensor reshaped to `shape`, an iterable as a tensor, a number broadcast to `shape`."""
    if torch.is_tensor(val):
        return val.reshape(shape)
    kwargs = {'dtype': dtype} if device is None else {'dtype': dtype, 'device': device}
    if isinstance(val, Iterable):
        return torch.tensor(val, **kwargs)
    return torch.full(shape, val, **kwargs)


class SgLightingParameters:
    r"""The lights of a scene as spherical gaussians.

    Args:
        amplitude (float, Iterable or torch.Tensor): RGB amplitude (strength and colour), of shape
            :math:`(\text{num_sg}, 3)`; a number is broadcast.
        direction (Iterable or torch.Tensor): lobe axes, of shape :math:`(\text{num_sg}, 3)`; normalised.
        sharpness (float, Iterable or torch.Tensor): lobe sharpness, of shape :math:`(\text{num_sg},)`; a number is
            broadcast.

    The number of lobes is taken from the first of amplitude, direction, sharpness that is a tensor (1 if none is).
    """
    __slots__ = ['amplitude', 'sharpness', 'direction']

    def __init__(self, amplitude=3., direction=(1., 0., 0.), sharpness=5.):
        num_sg = 1
        if torch.is_tensor(amplitude):
            amplitude = amplitude.reshape(-1, 3)
            num_sg = amplitude.shape[0]
        elif torch.is_tensor(direction):
            direction = direction.reshape(-1, 3)
            num_sg = direction.shape[0]
        elif torch.is_tensor(sharpness):
            sharpness = sharpness.reshape(-1)
            num_sg = sharpness.shape[0]
        self.amplitude = _as_tensor(amplitude, (num_sg, 3))
        self.sharpness = _as_tensor(sharpness, (num_sg,))
        if not torch.is_tensor(direction):
            direction = torch.tensor(direction, dtype=torch.float)
        self.direction = torch.nn.functional.normalize(direction.reshape(-1, 3), dim=1)

    @staticmethod
    def from_sun(direction, strength=3.0, angle=math.pi * 0.25, color=None):
        r"""Lobes that stand for suns.

        Args:
            direction (torch.Tensor): sun directions, of shape :math:`(\text{num_suns}, 3)`.
            strength (float, Iterable or torch.Tensor): strength per sun, of shape :math:`(\text{num_suns},)`.
            angle (float, Iterable or torch.Tensor): angular diameter per sun in radians, of shape
                :math:`(\text{num_suns},)`.
            color (None, Iterable or torch.Tensor): RGB colour per sun in [0, 1], of shape :math:`(\text{num_suns}, 3)`;
                white by default.

        Returns:
            (SgLightingParameters)
        """
        direction = direction.reshape(-1, 3)
        n = direction.shape[0]
        strength = _as_tensor(strength, (n,), device=direction.device)
        angle = _as_tensor(angle, (n,), device=direction.device)
        color = _as_tensor(1.0 if color is None else color, (n, 3), device=direction.device)
        return SgLightingParameters(*sg_from_sun(direction, strength, angle, color))

    @staticmethod
    def from_environment_map(image):
        raise NotImplementedError()

    def to(self, device):
        return SgLightingParameters(amplitude=self.amplitude.to(device), direction=self.direction.to(device),
                                    sharpness=self.sharpness.to(device))

    def cuda(self):
        return SgLightingParameters(amplitude=self.amplitude.cuda(), direction=self.direction.cuda(),
                                    sharpness=self.sharpness.cuda())

    def cpu(self):
        return SgLightingParameters(amplitude=self.amplitude.cpu(), direction=self.direction.cpu(),
                                    sharpness=self.sharpness.cpu())


def sg_from_sun(direction, strength, angle, color):
    r"""SG parameters of suns: amplitude = colour * strength, and the sharpness at which the lobe falls to half its
    strength at half the angular diameter, :math:`\log(0.5 / \text{strength}) / (\cos(\text{angle} / 2) - 1)`.

    Args:
        direction (torch.Tensor): of shape :math:`(\text{num_suns}, 3)`.
        strength (torch.Tensor): of shape :math:`(\text{num_suns},)`.
        angle (torch.Tensor): angular diameters in radians, of shape :math:`(\text{num_suns},)`.
        color (torch.Tensor): of shape :math:`(\text{num_suns}, 3)`.

    Returns:
        (torch.Tensor, torch.Tensor, torch.Tensor): amplitude :math:`(\text{num_suns}, 3)`, the input direction and
        sharpness :math:`(\text{num_suns},)`.
    """
    assert torch.is_tensor(direction) and direction.ndim == 2 and direction.shape[1] == 3
    assert torch.is_tensor(angle) and angle.ndim == 1
    assert torch.is_tensor(strength) and strength.ndim == 1
    assert torch.is_tensor(color) and color.ndim == 2 and color.shape[1] == 3
    amplitude = color * strength.unsqueeze(-1)
    sharpness = torch.log(0.5 / strength) / (torch.cos(angle / 2) - 1)
    return amplitude, direction, sharpness


def sg_direction_from_azimuth_elevation(azimuth, elevation):
    r"""Unit direction of an azimuth and an elevation (radians), y up: :math:`(\sin\phi\cos\theta, \sin\theta,
    \cos\phi\cos\theta)`.

    Args:
        azimuth (float or torch.Tensor)
        elevation (float or torch.Tensor)

    Returns:
        (torch.Tensor): of shape ``azimuth.shape + (3,)`` (numbers: :math:`(1, 3)`).
    """
    if not torch.is_tensor(azimuth):
        azimuth = torch.full((1,), azimuth, dtype=torch.float)
    if not torch.is_tensor(elevation):
        elevation = torch.full((1,), elevation, dtype=torch.float)
    cos_el = torch.cos(elevation)
    return torch.stack([torch.sin(azimuth) * cos_el, torch.sin(elevation), torch.cos(azimuth) * cos_el], dim=-1)


def _dot(a, b):
    return torch.sum(a * b, dim=-1, keepdim=True)


def _smith_ggx_g1(m2, cos_x):
    """One direction's term of the Smith-GGX visibility (the 1 / (4 n.l n.v) of the BRDF folded in)."""
    return 1. / (cos_x + torch.sqrt(m2 + (1. - m2) * cos_x * cos_x))


def sg_distribution_term(direction, roughness):
    r"""The GGX (Trowbridge-Reitz) normal distribution as one SG lobe per point: sharpness :math:`2 / m^2`, amplitude
    :math:`1 / (\pi m^2)`, :math:`m` = roughness.

    Args:
        direction (torch.Tensor): normals, of shape :math:`(\text{num_points}, 3)`.
        roughness (torch.Tensor): of shape :math:`(\text{num_points},)`.

    Returns:
        (torch.Tensor, torch.Tensor, torch.Tensor): amplitude :math:`(\text{num_points}, 3)` (an expanded view), the
        input direction, sharpness :math:`(\text{num_points},)`.
    """
    assert direction.ndim == 2 and direction.shape[-1]
    assert roughness.shape == direction.shape[:1]
    m2 = roughness * roughness
    sharpness = 2. / m2
    amplitude = (1. / (math.pi * m2)).unsqueeze(-1).expand(-1, 3)
    return amplitude, direction, sharpness


def sg_warp_distribution(amplitude, direction, sharpness, view):
    r"""The distribution lobes warped into the BRDF slice of a view (Wang et al. 2009): axis = the view reflected about
    the normal, sharpness divided by :math:`4 \max(n \cdot v, 10^{-4})`.

    Args:
        amplitude, direction (torch.Tensor): of shape :math:`(\text{num_sg}, 3)`.
        sharpness (torch.Tensor): of shape :math:`(\text{num_sg},)`.
        view (torch.Tensor): directions toward the viewer, of shape :math:`(\text{num_sg}, 3)`.

    Returns:
        (torch.Tensor, torch.Tensor, torch.Tensor): the input amplitude, the warped direction and sharpness.
    """
    assert amplitude.ndim == 2 and amplitude.shape[-1] == 3
    assert direction.shape == amplitude.shape
    assert sharpness.shape == amplitude.shape[:1]
    assert view.shape == amplitude.shape
    incoming = -view
    warp_direction = incoming - 2 * _dot(incoming, direction) * direction
    warp_sharpness = sharpness / (4. * torch.clamp(_dot(direction, view).squeeze(-1), min=1e-4))
    return amplitude, warp_direction, warp_sharpness


def fresnel(ldh, spec_albedo):
    r"""Schlick's Fresnel term :math:`F_0 + (1 - F_0)(1 - l \cdot h)^5`."""
    return spec_albedo + (1. - spec_albedo) * torch.pow(1. - ldh, 5)


def sg_warp_specular_term(amplitude, direction, sharpness, normal, roughness, view, spec_albedo):
    r"""Cook-Torrance specular radiance at surface points lit by SG lobes (DIB-R++): the GGX distribution as a warped SG
    lobe, its reduced inner product with the lights, times Smith-GGX visibility, Schlick Fresnel and the cosine, clamped
    at 0.

    Args:
        amplitude, direction (torch.Tensor): the lights, of shape :math:`(\text{num_sg}, 3)`.
        sharpness (torch.Tensor): of shape :math:`(\text{num_sg},)`.
        normal (torch.Tensor): of shape :math:`(\text{num_points}, 3)`.
        roughness (torch.Tensor): of shape :math:`(\text{num_points},)`.
        view (torch.Tensor): directions toward the camera, of shape :math:`(\text{num_points}, 3)`.
        spec_albedo (torch.Tensor): specular albedo (RGB), of shape :math:`(\text{num_points}, 3)`.

    Returns:
        (torch.Tensor): of shape :math:`(\text{num_points}, 3)`.
    """
    assert amplitude.ndim == 2 and amplitude.shape[-1]
    assert direction.shape == amplitude.shape
    assert sharpness.shape == amplitude.shape[:1]
    assert normal.ndim == 2 and normal.shape[-1] == 3
    assert roughness.shape == normal.shape[:1]
    assert view.shape == normal.shape
    assert spec_albedo.shape == normal.shape
    ndf = sg_warp_distribution(*sg_distribution_term(normal, roughness), view)
    warped_dir = ndf[1]
    ndl = torch.clamp(_dot(normal, warped_dir), min=0., max=1.)
    ndv = torch.clamp(_dot(normal, view), min=0., max=1.)
    half = warped_dir + view
    half = half / torch.sqrt(_dot(half, half))
    ldh = torch.clamp(_dot(warped_dir, half), min=0., max=1.)
    out = unbatched_reduced_sg_inner_product(*ndf, amplitude, direction, sharpness)
    m2 = (roughness * roughness).unsqueeze(-1)
    out = out * (_smith_ggx_g1(m2, ndl) * _smith_ggx_g1(m2, ndv))
    out = out * fresnel(ldh, spec_albedo)
    out = out * ndl
    return torch.clamp(out, min=0.)


def cosine_lobe_sg(direction):
    r"""The clamped cosine around `direction` as one SG lobe: amplitude 1.17, sharpness 2.133.

    Args:
        direction (torch.Tensor): of shape :math:`(\text{num}, 3)`.

    Returns:
        (torch.Tensor, torch.Tensor, torch.Tensor): amplitude (the shape of direction), the input direction, sharpness
        :math:`(\text{num},)`.
    """
    amplitude = torch.full_like(direction, _COSINE_LOBE_AMPLITUDE)
    sharpness = torch.full_like(direction[:, 0], _COSINE_LOBE_SHARPNESS)
    return amplitude, direction, sharpness


def approximate_sg_integral(amplitude, sharpness):
    r""":math:`2 \pi a / s`, the integral of an SG lobe over the sphere for large sharpness."""
    return 2. * math.pi * (amplitude / sharpness.unsqueeze(-1))


def sg_irradiance_fitted(amplitude, direction, sharpness, normal):
    r"""Irradiance per point and per SG light through the fitted polynomial of Stephen Hill (no inner product).

    Args:
        amplitude, direction (torch.Tensor): of shape :math:`(\text{num_sg}, 3)`.
        sharpness (torch.Tensor): of shape :math:`(\text{num_sg},)`.
        normal (torch.Tensor): of shape :math:`(\text{num_points}, 3)`.

    Returns:
        (torch.Tensor): of shape :math:`(\text{num_points}, \text{num_sg}, 3)`.
    """
    assert amplitude.ndim == 2 and amplitude.shape[-1] == 3
    assert direction.shape == amplitude.shape
    assert sharpness.shape == amplitude.shape[:1]
    assert normal.ndim == 2 and normal.shape[1] == 3
    mu_n = normal @ direction.t()                 # (num_points, num_sg) cosines
    lam = sharpness.unsqueeze(0)
    c0 = 0.36
    c1 = 1. / (4. * c0)
    e1 = torch.exp(-lam)
    e2 = e1 * e1
    inv = 1. / lam
    scale = 1. + 2. * e2 - inv
    bias = (e1 - e2) * inv - e2
    x = torch.sqrt(1. - scale)
    x0 = c0 * mu_n
    x1 = c1 * x
    n = x0 + x1
    y = torch.where(torch.abs(x0) <= x1, n * n / x, torch.clamp(mu_n, min=0., max=1.))
    return (scale * y + bias).unsqueeze(-1) * approximate_sg_integral(amplitude, sharpness).unsqueeze(0)


def sg_diffuse_fitted(amplitude, direction, sharpness, normal, albedo):
    r"""Lambertian radiance from :func:`sg_irradiance_fitted`: the mean over the lights, clamped at 0, times
    albedo / :math:`\pi`.  Returns shape :math:`(\text{num_points}, 3)`."""
    assert amplitude.ndim == 2 and amplitude.shape[1] == 3
    assert direction.shape == amplitude.shape
    assert sharpness.shape == amplitude.shape[:1]
    assert normal.ndim == 2 and normal.shape[1] == 3
    assert albedo.shape == normal.shape
    irradiance = sg_irradiance_fitted(amplitude, direction, sharpness, normal).mean(1)
    return torch.clamp(irradiance, min=0.) * (albedo / math.pi)


class _ReducedSgCosineLobe(torch.autograd.Function):
    """unbatched_reduced_sg_inner_product(*cosine_lobe_sg(normal), lights) on the constant-lobe kernels: the lobe is two
    constants, the gradient flows into the normals and the lights."""

    @staticmethod
    def forward(ctx, normal, amplitude, direction, sharpness):
        normal, amplitude, direction, sharpness = (t.contiguous() for t in (normal, amplitude, direction, sharpness))
        ctx.save_for_backward(normal, amplitude, direction, sharpness)
        return _C.render.sg.reduced_sg_constant_lobe_forward(_COSINE_LOBE_AMPLITUDE, _COSINE_LOBE_SHARPNESS, normal,
                                                             amplitude, direction, sharpness)

    @staticmethod
    def backward(ctx, grad_out):
        normal, amplitude, direction, sharpness = ctx.saved_tensors
        return tuple(_C.render.sg.reduced_sg_constant_lobe_backward(
            grad_out.contiguous(), _COSINE_LOBE_AMPLITUDE, _COSINE_LOBE_SHARPNESS, normal, amplitude, direction,
            sharpness))


def sg_irradiance_inner_product(amplitude, direction, sharpness, normal):
    r"""Irradiance at surface points: the SG inner product of the cosine lobe around each normal with every light,
    summed over the lights and clamped at 0.

    Args:
        amplitude, direction (torch.Tensor): the lights, of shape :math:`(\text{num_sg}, 3)`.
        sharpness (torch.Tensor): of shape :math:`(\text{num_sg},)`.
        normal (torch.Tensor): of shape :math:`(\text{num_points}, 3)`.

    Returns:
        (torch.Tensor): of shape :math:`(\text{num_points}, 3)`.
    """
    assert amplitude.ndim == 2 and amplitude.shape[1] == 3
    assert direction.shape == amplitude.shape
    assert sharpness.shape == amplitude.shape[:1]
    assert normal.ndim == 2 and normal.shape[1] == 3
    if normal.is_cuda:
        out = _ReducedSgCosineLobe.apply(normal, amplitude, direction, sharpness)
    else:
        out = unbatched_reduced_sg_inner_product(*cosine_lobe_sg(normal), amplitude, direction, sharpness)
    return torch.clamp(out, min=0.)


def sg_diffuse_inner_product(amplitude, direction, sharpness, normal, albedo):
    r"""Lambertian radiance at surface points lit by SG lobes (the diffuse term of DIB-R++, NeurIPS 2021):
    :func:`sg_irradiance_inner_product` times albedo / :math:`\pi`.

    Args:
        amplitude, direction (torch.Tensor): the lights, of shape :math:`(\text{num_sg}, 3)`.
        sharpness (torch.Tensor): of shape :math:`(\text{num_sg},)`.
        normal (torch.Tensor): of shape :math:`(\text{num_points}, 3)`.
        albedo (torch.Tensor): of shape :math:`(\text{num_points}, 3)`.

    Returns:
        (torch.Tensor): of shape :math:`(\text{num_points}, 3)`.
    """
    assert amplitude.ndim == 2 and amplitude.shape[1] == 3
    assert direction.shape == amplitude.shape
    assert sharpness.shape == amplitude.shape[:1]
    assert normal.ndim == 2 and normal.shape[1] == 3
    assert albedo.shape == normal.shape
    return sg_irradiance_inner_product(amplitude, direction, sharpness, normal) * (albedo / math.pi)


def unbatched_sg_inner_product(amplitude, direction, sharpness, other_amplitude, other_direction, other_sharpness):
    r"""SG inner product of every lobe with every other lobe, broadcast in torch:
    :math:`2\pi a_i a_j e^{u - l} (1 - e^{-2u}) / u`, :math:`u = |s_i d_i + s_j d_j|`, :math:`l = s_i + s_j`.

    Args:
        amplitude, direction (torch.Tensor): of shape :math:`(\text{num_sg}, 3)`.
        sharpness (torch.Tensor): of shape :math:`(\text{num_sg},)`.
        other_amplitude, other_direction (torch.Tensor): of shape :math:`(\text{num_other}, 3)`.
        other_sharpness (torch.Tensor): of shape :math:`(\text{num_other},)`.

    Returns:
        (torch.Tensor): of shape :math:`(\text{num_sg}, \text{num_other}, 3)`.
    """
    assert amplitude.ndim == 2 and amplitude.shape[1] == 3
    assert direction.shape == amplitude.shape
    assert sharpness.shape == amplitude.shape[:1]
    assert other_amplitude.ndim == 2 and other_amplitude.shape[1] == 3
    assert other_direction.shape == other_amplitude.shape
    assert other_sharpness.shape == other_amplitude.shape[:1]
    s_i, s_j = sharpness[:, None, None], other_sharpness[None, :, None]
    v = s_i * direction[:, None, :] + s_j * other_direction[None, :, :]
    um = torch.sqrt(_dot(v, v))
    lm = s_i + s_j
    prod = amplitude[:, None, :] * other_amplitude[None, :, :]
    return 2.0 * math.pi * (torch.exp(um - lm) * prod) * (1.0 - torch.exp(-2.0 * um)) / um


class UnbatchedReducedSgInnerProduct(torch.autograd.Function):
    """The reduced product on the HIP kernels (``_C.render.sg``), backward included."""

    @staticmethod
    def forward(ctx, amplitude, direction, sharpness, other_amplitude, other_direction, other_sharpness):
        ts = tuple(t.contiguous() for t in (amplitude, direction, sharpness, other_amplitude, other_direction,
                                            other_sharpness))
        ctx.save_for_backward(*ts)
        return _C.render.sg.unbatched_reduced_sg_inner_product_forward_cuda(*ts)

    @staticmethod
    def backward(ctx, grad_out):
        return tuple(_C.render.sg.unbatched_reduced_sg_inner_product_backward_cuda(grad_out.contiguous(),
                                                                                   *ctx.saved_tensors))


def unbatched_reduced_sg_inner_product(amplitude, direction, sharpness, other_amplitude, other_direction,
                                       other_sharpness):
    r""":func:`unbatched_sg_inner_product` summed over the other lobes, without the :math:`(\text{num_sg},
    \text{num_other}, 3)` intermediate on the GPU (HIP kernels, any num_other; f32 and f64).  On the CPU: the broadcast
    torch form.

    Returns:
        (torch.Tensor): of shape :math:`(\text{num_sg}, 3)`.
    """
    assert amplitude.ndim == 2 and amplitude.shape[1] == 3
    assert direction.shape == amplitude.shape
    assert sharpness.shape == amplitude.shape[:1]
    assert other_amplitude.ndim == 2 and other_amplitude.shape[1] == 3
    assert other_direction.shape == other_amplitude.shape
    assert other_sharpness.shape == other_amplitude.shape[:1]
    if amplitude.is_cuda:
        return UnbatchedReducedSgInnerProduct.apply(amplitude, direction, sharpness, other_amplitude, other_direction,
                                                    other_sharpness)
    return unbatched_sg_inner_product(amplitude, direction, sharpness, other_amplitude, other_direction,
                                      other_sharpness).sum(1)
