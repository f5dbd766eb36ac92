"""kaolin_amd.render.lighting on the CPU (no GPU): every public function against the reference's float64 results in
tests/golden/sg_lighting.npz (tests/golden/make_golden_sg.py), in f32 and f64, plus SgLightingParameters' semantics and the
shape checks."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from kaolin_amd.render import lighting
from kaolin_amd.render.lighting import sg as sgm
from kaolin_amd.utils.testing import elementwise_mismatch

TOL = {torch.float32: 1e-5, torch.float64: 1e-10}
DTYPES = [torch.float32, torch.float64]


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(GOLDEN_DIR, 'sg_lighting.npz'))
    return {k: torch.from_numpy(z[k]) for k in z.files}


def _check(a, b, dtype, term_abs_sum=None):
    msg = elementwise_mismatch(a, b, tol=TOL[dtype], term_abs_sum=term_abs_sum)
    assert msg is None, msg


def test_module_layout():
    import kaolin_amd
    assert kaolin_amd.render.lighting is lighting
    for name in sgm.__all__ + ['project_onto_sh9', 'sh9_irradiance', 'sh9_diffuse']:
        assert hasattr(lighting, name), name
    assert callable(lighting.sg.unbatched_reduced_sg_inner_product)
    assert callable(lighting.sg.unbatched_sg_inner_product)


@pytest.mark.parametrize('dtype', DTYPES)
def test_unbatched_sg_inner_product(gold, dtype):
    args = [gold[f'inner_{k}'].to(dtype) for k in ('a', 'd', 's', 'oa', 'od', 'os')]
    _check(sgm.unbatched_sg_inner_product(*args), gold['inner_out'], dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', ['1_1', '17_7', '33_8', '64_17', '65_64', '100_65', '23_511', '7_1'])
def test_reduced_forward_backward(gold, dtype, case):
    from sg_oracle import reduced_oracle
    tag = f'red_{case}'
    args = [gold[f'{tag}_{k}'].to(dtype).requires_grad_() for k in ('a', 'd', 's', 'oa', 'od', 'os')]
    go = gold[f'{tag}_go'].to(dtype)
    out = sgm.unbatched_reduced_sg_inner_product(*args)
    _check(out, gold[f'{tag}_out'], dtype, gold[f'{tag}_out_abs'])
    grads = torch.autograd.grad((out * go).sum(), args)
    ref = reduced_oracle(*[gold[f'{tag}_{k}'] for k in ('a', 'd', 's', 'oa', 'od', 'os')], grad_out=gold[f'{tag}_go'])
    for name, g in zip(('ga', 'gd', 'gs', 'goa', 'god', 'gos'), grads):
        _check(g, gold[f'{tag}_{name}'], dtype, ref[name + '_abs'])
        # the pairwise oracle agrees with the reference's autograd
        assert torch.allclose(ref[name], gold[f'{tag}_{name}'], rtol=1e-12, atol=1e-12)


def _shade(gold, dtype):
    return {k: gold[f'shade_{k}'].to(dtype) for k in ('la', 'ld', 'ls', 'normal', 'albedo', 'view', 'rough', 'spec')}


@pytest.mark.parametrize('dtype', DTYPES)
def test_shading_functions(gold, dtype):
    from sg_oracle import reduced_oracle
    s = _shade(gold, dtype)
    lights = (s['la'], s['ld'], s['ls'])
    lobe = sgm.cosine_lobe_sg(gold['shade_normal'])
    terms = reduced_oracle(*lobe, gold['shade_la'], gold['shade_ld'], gold['shade_ls'])['out_abs']
    _check(lighting.sg_irradiance_inner_product(*lights, s['normal']), gold['irr_ip'], dtype, terms)
    _check(lighting.sg_diffuse_inner_product(*lights, s['normal'], s['albedo']), gold['diff_ip'], dtype,
           terms * gold['shade_albedo'] / math.pi)
    _check(lighting.sg_irradiance_fitted(*lights, s['normal']), gold['irr_fit'], dtype)
    fit_terms = gold['irr_fit'].abs().mean(1) * gold['shade_albedo'] / math.pi
    _check(lighting.sg_diffuse_fitted(*lights, s['normal'], s['albedo']), gold['diff_fit'], dtype, fit_terms)
    spec = lighting.sg_warp_specular_term(*lights, s['normal'], s['rough'], s['view'], s['spec'])
    # the specular scale factors (visibility, Fresnel, cosine) are at most ~1e2: the reduced sum's slack times that bound
    ndf = sgm.sg_warp_distribution(*sgm.sg_distribution_term(gold['shade_normal'], gold['shade_rough']),
                                   gold['shade_view'])
    spec_terms = reduced_oracle(*ndf, gold['shade_la'], gold['shade_ld'], gold['shade_ls'])['out_abs'] * 1e2
    _check(spec, gold['spec'], dtype, spec_terms)
    a, d, sh = lighting.sg_distribution_term(s['normal'], s['rough'])
    _check(a, gold['ndf_a'], dtype)
    _check(sh, gold['ndf_s'], dtype)
    assert d is s['normal']
    _, wd, ws = lighting.sg_warp_distribution(a, d, sh, s['view'])
    _check(wd, gold['warp_d'], dtype)
    _check(ws, gold['warp_s'], dtype)
    _check(lighting.fresnel(gold['fresnel_ldh'].to(dtype), s['spec']), gold['fresnel'], dtype)
    _check(lighting.approximate_sg_integral(s['la'], s['ls']), gold['integral'], dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_suns_and_directions(gold, dtype):
    amp, d, sharp = lighting.sg_from_sun(gold['sun_dir'].to(dtype), gold['sun_strength'].to(dtype),
                                         gold['sun_angle'].to(dtype), gold['sun_color'].to(dtype))
    _check(amp, gold['sun_amp'], dtype)
    _check(sharp, gold['sun_sharp'], dtype)
    assert torch.isfinite(sharp).all()                     # angle 2 pi among them
    _check(lighting.sg_direction_from_azimuth_elevation(gold['azel_az'].to(dtype), gold['azel_el'].to(dtype)),
           gold['azel_dir'], dtype)


def test_parameters_golden(gold):
    p = lighting.SgLightingParameters.from_sun(gold['sun_dir'].float(), 2.5, 0.5)
    _check(p.amplitude, gold['params_sun_amp'], torch.float32)
    _check(p.direction, gold['params_sun_dir'], torch.float32)
    _check(p.sharpness, gold['params_sun_sharp'], torch.float32)
    p = lighting.SgLightingParameters(amplitude=2., direction=gold['params_raw_dir'].float(), sharpness=4.)
    _check(p.amplitude, gold['params_amp'], torch.float32)
    _check(p.direction, gold['params_dir'], torch.float32)
    _check(p.sharpness, gold['params_sharp'], torch.float32)


@pytest.mark.parametrize('dtype', DTYPES)
def test_spherical_harmonics(gold, dtype):
    _check(lighting.project_onto_sh9(gold['sh_dir'].to(dtype)), gold['sh_coeffs'], dtype)
    _check(lighting.project_onto_sh9(gold['sh_normals'].to(dtype)), gold['sh_proj'], dtype)
    lights = lighting.project_onto_sh9(gold['sh_dir'].to(dtype))
    irr_terms = (gold['sh_proj'].abs() * gold['sh_coeffs'].abs() * math.pi).sum(-1)
    _check(lighting.sh9_irradiance(lights, gold['sh_normals'].to(dtype)), gold['sh_irr'], dtype, irr_terms)
    _check(lighting.sh9_diffuse(gold['sh_dir'].to(dtype), gold['sh_normals'].to(dtype), gold['shade_albedo'].to(dtype)),
           gold['sh_diffuse'], dtype, irr_terms[:, None] * gold['shade_albedo'])
    coeffs = lighting.project_onto_sh9([0.0, 0.6, 0.8])
    assert coeffs.shape == (9,)
    assert torch.allclose(coeffs, lighting.project_onto_sh9(torch.tensor([0.0, 0.6, 0.8])))
    with pytest.raises(TypeError):
        lighting.project_onto_sh9((0.0, 0.6, 0.8))


# ---- SgLightingParameters semantics ---------------------------------------------------------------------------------

def test_parameters_defaults():
    p = lighting.SgLightingParameters()
    assert p.amplitude.shape == (1, 3) and torch.equal(p.amplitude, torch.full((1, 3), 3.))
    assert p.sharpness.shape == (1,) and torch.equal(p.sharpness, torch.tensor([5.]))
    assert torch.equal(p.direction, torch.tensor([[1., 0., 0.]]))
    assert p.amplitude.dtype == p.sharpness.dtype == p.direction.dtype == torch.float32


def test_parameters_broadcast_from_tensor():
    amp = torch.rand(4, 3)
    p = lighting.SgLightingParameters(amplitude=amp, direction=(0., 2., 0.), sharpness=3.)
    assert torch.equal(p.amplitude, amp)
    assert p.sharpness.shape == (4,) and torch.equal(p.sharpness, torch.full((4,), 3.))
    assert torch.allclose(p.direction, torch.tensor([[0., 1., 0.]]))
    d = torch.rand(5, 3) + 0.1
    p = lighting.SgLightingParameters(amplitude=1.5, direction=d, sharpness=2.)
    assert p.amplitude.shape == (5, 3) and p.sharpness.shape == (5,)
    assert torch.allclose(p.direction.norm(dim=1), torch.ones(5))
    assert torch.allclose(p.direction, d / d.norm(dim=1, keepdim=True))
    s = torch.rand(6)
    p = lighting.SgLightingParameters(sharpness=s)
    assert p.amplitude.shape == (6, 3) and torch.equal(p.sharpness, s)
    # flat tensors are reshaped
    p = lighting.SgLightingParameters(amplitude=torch.rand(12), direction=torch.rand(12) + 0.1, sharpness=torch.rand(4))
    assert p.amplitude.shape == (4, 3) and p.direction.shape == (4, 3) and p.sharpness.shape == (4,)


def test_parameters_iterables():
    p = lighting.SgLightingParameters(amplitude=[[1., 2., 3.]], direction=[[0., 0., 3.]], sharpness=[7.])
    assert torch.equal(p.amplitude, torch.tensor([[1., 2., 3.]]))
    assert torch.equal(p.sharpness, torch.tensor([7.]))
    assert torch.equal(p.direction, torch.tensor([[0., 0., 1.]]))


def test_parameters_to_and_from_sun():
    d = torch.tensor([[0., 1., 0.], [1., 0., 0.]])
    p = lighting.SgLightingParameters.from_sun(d, strength=torch.tensor([2., 4.]), angle=0.3,
                                               color=torch.tensor([[1., 0.5, 0.25], [1., 1., 1.]]))
    amp, _, sharp = lighting.sg_from_sun(d, torch.tensor([2., 4.]), torch.full((2,), 0.3),
                                         torch.tensor([[1., 0.5, 0.25], [1., 1., 1.]]))
    assert torch.equal(p.amplitude, amp) and torch.equal(p.sharpness, sharp)
    expected = torch.log(0.5 / torch.tensor([2., 4.])) / (math.cos(0.15) - 1)
    assert torch.allclose(sharp, expected)
    assert torch.equal(amp, torch.tensor([[2., 1., 0.5], [4., 4., 4.]]))
    q = p.to('cpu')
    assert q is not p and torch.equal(q.amplitude, p.amplitude)
    q = p.cpu()
    assert torch.equal(q.direction, p.direction) and torch.equal(q.sharpness, p.sharpness)
    full_circle = lighting.SgLightingParameters.from_sun(d, strength=3., angle=2 * math.pi)
    assert torch.isfinite(full_circle.sharpness).all()
    assert torch.allclose(full_circle.sharpness, torch.full((2,), math.log(0.5 / 3.) / -2.))


def test_cosine_lobe_and_direction_helpers():
    n = torch.rand(5, 3)
    a, d, s = lighting.cosine_lobe_sg(n)
    assert torch.equal(a, torch.full_like(n, 1.17)) and d is n and torch.equal(s, torch.full((5,), 2.133))
    v = lighting.sg_direction_from_azimuth_elevation(0., 0.)
    assert torch.allclose(v, torch.tensor([[0., 0., 1.]]))
    v = lighting.sg_direction_from_azimuth_elevation(math.pi / 2, 0.)
    assert torch.allclose(v, torch.tensor([[1., 0., 0.]]), atol=1e-7)
    v = lighting.sg_direction_from_azimuth_elevation(0., math.pi / 2)
    assert torch.allclose(v, torch.tensor([[0., 1., 0.]]), atol=1e-7)


def test_reduced_cpu_zero_sizes():
    z = sgm.unbatched_reduced_sg_inner_product(torch.rand(4, 3), torch.rand(4, 3), torch.rand(4), torch.rand(0, 3),
                                               torch.rand(0, 3), torch.rand(0))
    assert torch.equal(z, torch.zeros(4, 3))
    z = sgm.unbatched_reduced_sg_inner_product(torch.rand(0, 3), torch.rand(0, 3), torch.rand(0), torch.rand(2, 3),
                                               torch.rand(2, 3), torch.rand(2))
    assert z.shape == (0, 3)


# ---- wrong shapes raise --------------------------------------------------------------------------------------------

def test_wrong_shapes_raise():
    a, d, s = torch.rand(4, 3), torch.rand(4, 3), torch.rand(4)
    n, alb = torch.rand(6, 3), torch.rand(6, 3)
    with pytest.raises(AssertionError):
        sgm.unbatched_reduced_sg_inner_product(a, d, s, torch.rand(2, 3), torch.rand(2, 3), torch.rand(3))
    with pytest.raises(AssertionError):
        sgm.unbatched_reduced_sg_inner_product(torch.rand(4, 2), d, s, a, d, s)
    with pytest.raises(AssertionError):
        sgm.unbatched_sg_inner_product(a, torch.rand(5, 3), s, a, d, s)
    with pytest.raises(AssertionError):
        lighting.sg_diffuse_inner_product(a, d, s, n, torch.rand(5, 3))
    with pytest.raises(AssertionError):
        lighting.sg_irradiance_inner_product(a, d, torch.rand(3), n)
    with pytest.raises(AssertionError):
        lighting.sg_irradiance_fitted(a, d, s, torch.rand(6, 4))
    with pytest.raises(AssertionError):
        lighting.sg_diffuse_fitted(a, d, s, n, torch.rand(6, 2))
    with pytest.raises(AssertionError):
        lighting.sg_warp_specular_term(a, d, s, n, torch.rand(5), n, alb)
    with pytest.raises(AssertionError):
        lighting.sg_warp_distribution(a, d, s, torch.rand(3, 3))
    with pytest.raises(AssertionError):
        lighting.sg_from_sun(torch.rand(2, 3), torch.rand(2, 1), torch.rand(2), torch.rand(2, 3))
    with pytest.raises(AssertionError):
        lighting.sh9_irradiance(torch.rand(8), n)
    with pytest.raises(AssertionError):
        lighting.sh9_diffuse(torch.rand(3), n, torch.rand(5, 3))


def test_backward_workspace_query_is_host_only():
    from kaolin_amd import _lib
    ws = _lib.load().kamd_sg_reduced_inner_product_backward_workspace
    assert ws(0, 32, 4) == 0 and ws(1000, 0, 4) == 0
    assert ws(1000, 32, 4) > 0 and ws(1000, 32, 8) == 2 * ws(1000, 32, 4)
    assert ws(8 << 20, 32, 4) > ws(1000, 32, 4)
    assert ws(8 << 20, 32, 4) == ws(16 << 20, 32, 4)         # the persistent grid: bounded by the CU count, not the rows
    assert ws(8 << 20, 64, 4) == 2 * ws(8 << 20, 32, 4)
