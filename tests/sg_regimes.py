"""Input families of the reduced spherical-gaussian inner product at the values shading runs it with, shared by the
fixture generator (tests/golden/make_golden_sg_regimes.py) and the tests: unit directions over the whole sphere, sharpness
from 0.05 into the hundreds of thousands, lobes that nearly or exactly cancel.  Everything is drawn in float64 from a seeded
CPU generator and then rounded to the requested dtype, so a family at (rows, lights, seed) is the same tensors everywhere.

    wide        both sharpnesses log-uniform 0.05 - 300, signed amplitudes
    sharp       both log-uniform 1 - 5000, signed amplitudes
    cosine      rows = the cosine lobe (1.17, unit normal, 2.133); lights: amplitude >= 0, sharpness log-uniform 0.5 - 5000
    specular    rows = sg_warp_distribution(*sg_distribution_term(normal, roughness), view), roughness 0.05 - 0.9, views from
                head-on to grazing (row sharpness 2.5 .. 1e5); lights as in cosine
    antipodal   lights of sharpness 0.5 - 50; row i is the mirror image of light i % lights up to 1e-4 .. 1e-3 in direction and
                up to 1e-3 relative in sharpness: um of that pair is 5e-5 .. 0.1 at lm up to 100, every other pair is ordinary
    exact_zero  rows and lights of sharpness 0.5 - 50; the rows `zero_rows` are the exact negation of the lights
                `zero_lights` with the bit-equal sharpness, so v == 0 for those pairs in the reference's arithmetic.  The first
                two of these lights have sharpness 2 and 8 (s d is exact), the others a drawn sharpness (s d is rounded, and
                the two roundings cancel exactly only if the two products are rounded apart)

    exact_zero_cosine   the same for the constant-lobe kernels: cosine-lobe rows, and the lights `zero_lights` are the
                negated normals of `zero_rows` with sharpness 2.133 as rounded to the dtype

Every family has a light of amplitude exactly 0 and, where the row amplitude is free, a row of amplitude exactly 0."""
import math
import os

import numpy as np
import torch

from kaolin_amd.render.lighting import sg as sgm

FAMILIES = ('wide', 'sharp', 'cosine', 'specular', 'antipodal', 'exact_zero', 'exact_zero_cosine')
BOUNDED = FAMILIES[:5]                                  # the families with values (the last two: NaN masks)
BOUND_FAMILIES = ('sharp', 'cosine', 'specular')       # K32 is 4 x the reference's own f32 error over these
KEYS = ('a', 'd', 's', 'oa', 'od', 'os')
OUTPUTS = ('out', 'ga', 'gd', 'gs', 'goa', 'god', 'gos')
K_MARGIN = 4.0
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ZERO_ROWS = (5, 70, 131, 200)
ZERO_LIGHTS = (0, 1, 3, 4)

# the cases of tests/golden/sg_regimes.npz: family, rows, lights, seed
FIXTURE_CASES = (('wide', 300, 9, 1), ('wide', 320, 33, 2), ('sharp', 300, 16, 3), ('sharp', 330, 48, 4),
                 ('cosine', 300, 32, 5), ('cosine', 310, 33, 6), ('specular', 300, 9, 7), ('specular', 340, 48, 8),
                 ('antipodal', 300, 16, 9), ('antipodal', 320, 32, 10), ('exact_zero', 300, 33, 11),
                 ('exact_zero_cosine', 300, 33, 12))


def case_tag(family, n, m, seed):
    return f'{family}_{n}_{m}_{seed}'


def _unit(n, g):
    v = torch.randn(n, 3, generator=g, dtype=torch.float64)
    return v / v.norm(dim=1, keepdim=True)


def _loguniform(n, lo, hi, g):
    return torch.exp(torch.rand(n, generator=g, dtype=torch.float64) * (math.log(hi) - math.log(lo)) + math.log(lo))


def _signed(n, g):
    return torch.rand(n, 3, generator=g, dtype=torch.float64) * 4. - 2.


def make(family, n, m, seed, dtype=torch.float32, device='cpu'):
    """-> dict a, d, s, oa, od, os, go (grad_out) in `dtype` on `device`; plus 'normal' (the cosine-lobe families: the
    same tensor as 'd') and 'zero_rows' / 'zero_lights' (the exact_zero families, index tensors)."""
    assert family in FAMILIES
    g = torch.Generator().manual_seed(seed)
    x = {}
    if family in ('wide', 'sharp'):
        lo, hi = (0.05, 300.) if family == 'wide' else (1., 5000.)
        x.update(a=_signed(n, g), d=_unit(n, g), s=_loguniform(n, lo, hi, g),
                 oa=_signed(m, g), od=_unit(m, g), os=_loguniform(m, lo, hi, g))
    elif family in ('cosine', 'specular', 'exact_zero_cosine'):
        normal = _unit(n, g)
        x.update(oa=torch.rand(m, 3, generator=g, dtype=torch.float64) * 2., od=_unit(m, g),
                 os=_loguniform(m, 0.5, 5000., g))
        if family != 'specular':
            x.update(zip(('a', 'd', 's'), sgm.cosine_lobe_sg(normal)))
            x['normal'] = normal
        else:
            roughness = torch.rand(n, generator=g, dtype=torch.float64) * 0.85 + 0.05
            cos_v = torch.clamp(torch.rand(n, generator=g, dtype=torch.float64) ** 2, min=2e-3)    # n . view, to grazing
            t = torch.linalg.cross(normal, _unit(n, g))
            t = t / t.norm(dim=1, keepdim=True)
            view = cos_v[:, None] * normal + torch.sqrt(1. - cos_v * cos_v)[:, None] * t
            a, d, s = sgm.sg_warp_distribution(*sgm.sg_distribution_term(normal, roughness), view)
            x.update(a=a.contiguous(), d=d, s=s)
    else:
        x.update(oa=_signed(m, g), od=_unit(m, g), os=_loguniform(m, 0.5, 50., g))
        if family == 'antipodal':
            j = torch.arange(n) % m
            t = torch.linalg.cross(x['od'][j], _unit(n, g))          # perpendicular: the whole offset turns the direction
            d = -x['od'][j] + _loguniform(n, 1e-4, 1e-3, g)[:, None] * t / t.norm(dim=1, keepdim=True)
            rel = (torch.rand(n, generator=g, dtype=torch.float64) * 2. - 1.) * 1e-3
            x.update(a=_signed(n, g), d=d / d.norm(dim=1, keepdim=True), s=x['os'][j] * (1. + rel))
        else:
            assert n > max(ZERO_ROWS) and m > max(ZERO_LIGHTS)
            x['os'][ZERO_LIGHTS[0]], x['os'][ZERO_LIGHTS[1]] = 2., 8.
            x.update(a=_signed(n, g), d=_unit(n, g), s=_loguniform(n, 0.5, 50., g))
    x['go'] = torch.rand(n, 3, generator=g, dtype=torch.float64) * 2. - 0.5
    if family not in ('cosine', 'specular', 'exact_zero_cosine'):
        x['a'][n // 3] = 0.
    x['oa'][m // 2] = 0.
    x = {k: v.to(dtype) for k, v in x.items()}
    if family == 'exact_zero':
        # after the rounding, so that the negation and the sharpness are bit-equal in `dtype`
        rows, lights = torch.tensor(ZERO_ROWS), torch.tensor(ZERO_LIGHTS)
        x['d'][rows] = -x['od'][lights]
        x['s'][rows] = x['os'][lights]
        x['zero_rows'], x['zero_lights'] = rows, lights
    if family == 'exact_zero_cosine':
        rows, lights = torch.tensor(ZERO_ROWS), torch.tensor(ZERO_LIGHTS)
        x['od'][lights] = -x['d'][rows]
        x['os'][lights] = x['s'][rows]
        x['zero_rows'], x['zero_lights'] = rows, lights
    if family == 'antipodal':
        j = torch.arange(n) % m
        v = x['s'].double()[:, None] * x['d'].double() + x['os'].double()[j][:, None] * x['od'].double()[j]
        assert float(v.norm(dim=1).min()) >= 1e-5        # f64 results are compared at 1e-10: um >= 1e-5 keeps that meaningful
    return {k: v.to(device) for k, v in x.items()}


def mixed_wavefront(m, seed, dtype=torch.float32, device='cpu', blocks=4):
    """Rows for one-lane-per-row kernels with 64-lane wavefronts: per block of 128 rows, 64 rows that alternate between an
    antipodal row (its mirrored pair has um < 1) and a sharp row (sharpness 60 - 5000 against lights of 0.5 - 50: every um is
    above 1), then 64 consecutive sharp rows.  Lights as in `antipodal`."""
    n = blocks * 128
    x = make('antipodal', n, m, seed, torch.float64)
    g = torch.Generator().manual_seed(seed + 1)
    sharp_s = _loguniform(n, 60., 5000., g)
    sharp_d = _unit(n, g)
    r = torch.arange(n) % 128
    is_sharp = (r >= 64) | (r % 2 == 1)
    x['s'] = torch.where(is_sharp, sharp_s, x['s'])
    x['d'] = torch.where(is_sharp[:, None], sharp_d, x['d'])
    x['is_sharp'] = is_sharp
    return {k: (v.to(dtype) if v.is_floating_point() else v).to(device) for k, v in x.items()}


def args_of(x):
    return [x[k] for k in KEYS]


# ---- the fixture tests/golden/sg_regimes.npz ---------------------------------------------------------------------------

def load_fixture():
    z = np.load(os.path.join(GOLDEN_DIR, 'sg_regimes.npz'))
    fx = {k: torch.from_numpy(z[k]) for k in z.files}
    fx['K32'] = K_MARGIN * max(float(fx[f'K_ref_{f}'].max()) for f in BOUND_FAMILIES)
    return fx


def case_inputs(fx, case):
    tag = case_tag(*case)
    x = {k: fx[f'{tag}_{k}'] for k in KEYS + ('go',)}
    if case[0] not in BOUNDED:
        x['zero_rows'], x['zero_lights'] = fx[f'{tag}_zero_rows'], fx[f'{tag}_zero_lights']
    return x


def nan_masks(x, name):
    """exact_zero: the elements that must be NaN -- the collided rows (row-side results) or lights (column gradients)."""
    if 'zero_rows' not in x:
        return None
    rowside = name in ('out', 'ga', 'gd', 'gs')
    like = {'out': x['a'], 'ga': x['a'], 'gd': x['d'], 'gs': x['s'], 'goa': x['oa'], 'god': x['od'], 'gos': x['os']}[name]
    mask = torch.zeros(like.shape, dtype=torch.bool)
    mask[(x['zero_rows'] if rowside else x['zero_lights']).cpu()] = True
    return mask
