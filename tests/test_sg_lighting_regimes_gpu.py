"""The HIP kernels of csrc/sg_lighting.hip at the inputs shading runs them with (tests/sg_regimes.py): unit directions over
the sphere, sharpness into the hundreds of thousands, lobes that nearly or exactly cancel, more than one chunk of lights in
the constant-lobe kernels, and rows beyond the persistent grid together with several chunks.  Forward and all six gradients
against the analytic float64 oracle (tests/sg_oracle.py's stable_oracle) within
    tol |b| + tol median|b| + 64 eps sum|terms| + K32 eps cond,      tol = 1e-5 (f32) / 1e-10 (f64)
where K32 = 4 x the reference's own float32 error in units of eps32 cond, read from tests/golden/sg_regimes.npz.  Every test
prints the largest error in those units and how many elements needed the last term; the module prints the maxima per family
and output when it is done (pytest -s)."""
import collections

import pytest
import torch

import sg_regimes as R
from sg_oracle import conditioned_mismatch, stable_oracle
from kaolin_amd.render.lighting import sg as sgm

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float64]
ROWSIDE = ('out', 'ga', 'gd', 'gs')
CONST_NAMES = ('out', 'gd', 'goa', 'god', 'gos')          # what the constant-lobe kernels return
UNITS = collections.defaultdict(float)                    # (family, dtype, output) -> largest error / (eps cond)
NEEDED = collections.defaultdict(int)                     # (family, dtype) -> elements that needed the cond term


@pytest.fixture(scope='module')
def fx():
    yield R.load_fixture()
    for dtype in DTYPES:
        print(f'\nlargest |error| / (eps cond) on the GPU, {dtype}:')
        print(f'{"family":18s} ' + ' '.join(f'{n:>8s}' for n in R.OUTPUTS) + '   needed the cond term')
        for family in sorted({k[0] for k in UNITS}):
            print(f'{family:18s} ' + ' '.join(f'{UNITS[(family, dtype, n)]:8.3g}' for n in R.OUTPUTS)
                  + f'   {NEEDED[(family, dtype)]}')


def to_gpu(x, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v).cuda() for k, v in x.items()}


def run_general(x):
    args = [x[k].detach().clone().requires_grad_() for k in R.KEYS]
    out = sgm.unbatched_reduced_sg_inner_product(*args)
    return dict(zip(R.OUTPUTS, (out.detach(),) + torch.autograd.grad(out, args, x['go'])))


def run_general_shim(x):
    from kaolin_amd._C.render import sg as shim
    out = shim.unbatched_reduced_sg_inner_product_forward_cuda(*R.args_of(x))
    return dict(zip(R.OUTPUTS, [out] + shim.unbatched_reduced_sg_inner_product_backward_cuda(x['go'], *R.args_of(x))))


def run_const(x):
    """The constant-lobe entry points on a cosine-lobe family: the lobe's two constants as the rows hold them."""
    from kaolin_amd._C.render import sg as shim
    amp, sharp = float(x['a'][0, 0]), float(x['s'][0])
    assert bool((x['a'] == amp).all()) and bool((x['s'] == sharp).all())
    lights = [x[k] for k in ('oa', 'od', 'os')]
    out = shim.reduced_sg_constant_lobe_forward(amp, sharp, x['d'], *lights)
    return dict(zip(CONST_NAMES, [out] + shim.reduced_sg_constant_lobe_backward(x['go'], amp, sharp, x['d'], *lights)))


def check(got, ref, x, k32, family, what, rows=None, control=False):
    """Every result in `got` against the oracle; -> the number of elements that needed the cond term."""
    total = 0
    for name, t in got.items():
        if rows is not None and name in ROWSIDE:
            t = t[rows]
        mask = R.nan_masks(x, name)
        msg, needed, units = conditioned_mismatch(t, ref[name], ref[name + '_abs'], ref[name + '_cond'], k32, allow_nan=mask)
        print(f'{what} {name}: {units:.3g} eps cond, {needed} of {t.numel()} needed the cond term')
        assert msg is None, f'{what} {name}: {msg}'
        if mask is not None:       # exactly the constructed collisions are NaN: the mask's elements, and nothing else
            assert int(torch.isnan(t).sum()) == int(mask.sum()) == len(R.ZERO_ROWS) * (mask[0].numel()), name
        key = (family, t.dtype, name)
        UNITS[key] = max(UNITS[key], units)
        total += needed
    NEEDED[(family, next(iter(got.values())).dtype)] += total
    if control:
        assert total == 0, f'{what}: {total} elements of the rand(0, 1) regime passed only thanks to the cond term'
    return total


def oracle(x, rows=None):
    return stable_oracle(*R.args_of(x), grad_out=x['go'], pairs_per_chunk=1 << 22, rows=rows)


# ---- the fixture's cases: the same inputs the reference ran --------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', R.FIXTURE_CASES, ids=[R.case_tag(*c) for c in R.FIXTURE_CASES])
def test_fixture_cases(fx, case, dtype):
    family, tag = case[0], R.case_tag(*case)
    cpu = R.case_inputs(fx, case)
    x = to_gpu(cpu, dtype)
    ref = oracle(x)
    if family not in R.BOUNDED:
        # the reference's recorded NaN masks are the constructed collisions (pinned on the CPU too): the collided rows are
        # NaN in out and the row gradients, the lights they hit in the three light gradients, everything else is finite
        for name in R.OUTPUTS:
            assert torch.equal(fx[f'{tag}_nan_{name}'], R.nan_masks(cpu, name)), name
    if family != 'exact_zero_cosine':
        got = run_general(x)
        check(got, ref, x, fx['K32'], family, f'{tag} {dtype} general')
    if family in ('cosine', 'exact_zero_cosine'):
        const = run_const(x)
        check(const, ref, x, fx['K32'], family, f'{tag} {dtype} constant lobe')
    if family == 'exact_zero_cosine':
        check(run_general(x), ref, x, fx['K32'], family, f'{tag} {dtype} general')


def test_fixture_cases_through_shim(fx):
    for case in (R.FIXTURE_CASES[3], R.FIXTURE_CASES[9]):
        x = to_gpu(R.case_inputs(fx, case), torch.float32)
        check(run_general_shim(x), oracle(x), x, fx['K32'], case[0], f'{R.case_tag(*case)} shim')


# ---- seeded larger cases ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('num_other', [9, 16, 32, 33, 65, 200])
@pytest.mark.parametrize('num_sg', [63, 4097, 70001])
@pytest.mark.parametrize('family', R.BOUNDED)
def test_families_vs_oracle(fx, family, num_sg, num_other, dtype):
    x = R.make(family, num_sg, num_other, seed=num_sg * 7 + num_other, dtype=dtype, device='cuda')
    check(run_general(x), oracle(x), x, fx['K32'], family, f'{family} {num_sg}x{num_other} {dtype}')


def _same_as_general(const, general, ref, k32, what):
    for name in CONST_NAMES:
        msg, _, _ = conditioned_mismatch(const[name], general[name].double(), ref[name + '_abs'], ref[name + '_cond'], k32)
        assert msg is None, f'{what} {name}, constant lobe vs general kernel: {msg}'


@pytest.mark.parametrize('num_other,dtype', [(33, torch.float32), (65, torch.float32), (200, torch.float32),
                                             (17, torch.float64), (40, torch.float64)])
@pytest.mark.parametrize('num_sg', [63, 4097])
def test_constant_lobe_multi_chunk(fx, num_sg, num_other, dtype):
    """More lights than one chunk (32 in f32, 16 in f64): the constant-lobe backward carries Qr through grad_direction."""
    x = R.make('cosine', num_sg, num_other, seed=100 + num_other, dtype=dtype, device='cuda')
    ref, const = oracle(x), run_const(x)
    what = f'cosine {num_sg}x{num_other} {dtype}'
    check(const, ref, x, fx['K32'], 'cosine', what + ' constant lobe')
    _same_as_general(const, run_general(x), ref, fx['K32'], what)


def test_grid_stride_with_several_chunks(fx):
    """300000 rows (the persistent backward grid covers 2 x CUs x 256 = 131072: every lane owns two or three rows) x 65
    lights (three chunks): a lane re-reads its rows' running sums across the chunks.  Row-side results on a sample of 16384
    rows, the light gradients over all rows.  General and constant-lobe kernels, f32."""
    n, m = 300000, 65
    x = R.make('cosine', n, m, seed=200, dtype=torch.float32, device='cuda')
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(201))[:16384].sort().values.cuda()
    ref = oracle(x, rows=rows)
    general, const = run_general(x), run_const(x)
    check(general, ref, x, fx['K32'], 'cosine', f'cosine {n}x{m} general', rows=rows)
    check(const, ref, x, fx['K32'], 'cosine', f'cosine {n}x{m} constant lobe', rows=rows)
    _same_as_general({k: (v[rows] if k in ROWSIDE else v) for k, v in const.items()},
                     {k: (v[rows] if k in ROWSIDE else v) for k, v in general.items()}, ref, fx['K32'], f'cosine {n}x{m}')
    y = R.make('sharp', n, m, seed=202, dtype=torch.float32, device='cuda')
    check(run_general(y), oracle(y, rows=rows), y, fx['K32'], 'sharp', f'sharp {n}x{m} general', rows=rows)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('num_other', [16, 33])
def test_mixed_wavefront(fx, num_other, dtype):
    """Wavefronts whose lanes alternate between um < 1 (series) and um > 1 (exponential form), next to wavefronts with
    every lane above 1 (the series branch is skipped as a whole)."""
    x = R.mixed_wavefront(num_other, seed=300 + num_other, dtype=dtype, device='cuda')
    a, d, s, oa, od, os_ = (t.double() for t in R.args_of(x))
    um = (s[:, None, None] * d[:, None] + os_[None, :, None] * od[None]).norm(dim=-1).reshape(-1, 2, 64, num_other)
    assert bool((um[:, 1] > 1).all())                                     # the second wavefront of every 128 rows
    first = um[:, 0].reshape(-1, 32, 2, num_other)
    assert bool((first[:, :, 0].min(-1).values < 1).all()) and bool((first[:, :, 1] > 1).all())
    check(run_general(x), oracle(x), x, fx['K32'], 'mixed', f'mixed wavefront x{num_other} {dtype}')


def test_constant_lobe_multi_chunk_is_deterministic():
    x = R.make('cosine', 300000, 65, seed=400, dtype=torch.float32, device='cuda')
    first, second = run_const(x), run_const(x)
    for name in CONST_NAMES:
        assert torch.equal(first[name], second[name]), name


def test_rand01_control_needs_no_cond_term(fx):
    """The regime of tests/test_sg_lighting_gpu.py (every input from rand(0, 1); its shape 10000 x 65) through this file's
    checker: every element passes the existing bound, none thanks to the conditioned term."""
    g = torch.Generator(device='cuda').manual_seed(10000 * 1000 + 65)
    shapes = ((10000, 3), (10000, 3), (10000,), (65, 3), (65, 3), (65,), (10000, 3))
    x = dict(zip(R.KEYS + ('go',), [torch.rand(s, generator=g, dtype=torch.float32, device='cuda') for s in shapes]))
    check(run_general(x), oracle(x), x, fx['K32'], 'rand01', 'rand(0, 1) 10000x65', control=True)
