"""The reduced SG inner product at real shading inputs, the part that needs no GPU: tests/sg_oracle.py's stable_oracle pinned
against the autograd oracle, the reference's float64 results (tests/golden/sg_regimes.npz) and a 50-digit evaluation; the
fixture's own consistency; and the bound K32 eps cond shown reachable in float32 by a torch restatement of the arithmetic of
csrc/sg_lighting.hip, before any GPU time is spent on it."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
import sg_regimes as R
from sg_oracle import conditioned_mismatch, error_units, pair_kernel, reduced_oracle, stable_oracle
from kaolin_amd.render.lighting import sg as sgm

GRADS = R.OUTPUTS[1:]
CASE_IDS = [R.case_tag(*c) for c in R.FIXTURE_CASES]


@pytest.fixture(scope='module')
def fx():
    return R.load_fixture()


# ---- the oracle ------------------------------------------------------------------------------------------------------

def test_fixture_inputs_are_the_generators(fx):
    for case in R.FIXTURE_CASES:
        x, y = R.case_inputs(fx, case), R.make(*case, dtype=torch.float32)
        for k in R.KEYS + ('go',):
            assert x[k].dtype == torch.float32 and torch.allclose(x[k], y[k], rtol=1e-6, atol=0), (case, k)
        if case[0] not in ('cosine', 'specular', 'exact_zero_cosine'):
            assert bool((x['a'] == 0).all(1).any())
        assert bool((x['oa'] == 0).all(1).any())


@pytest.mark.parametrize('case', ['17_7', '64_17', '100_65', '23_511'])
def test_stable_oracle_equals_autograd_oracle_and_golden(case):
    z = np.load(os.path.join(GOLDEN_DIR, 'sg_lighting.npz'))
    args = [torch.from_numpy(z[f'red_{case}_{k}']) for k in R.KEYS]
    go = torch.from_numpy(z[f'red_{case}_go'])
    new, old = stable_oracle(*args, grad_out=go), reduced_oracle(*args, grad_out=go)
    a, d, s, oa, od, os_ = args
    um = (s[:, None, None] * d[:, None] + os_[None, :, None] * od[None]).norm(dim=-1)
    # a row (a light) is compared where every one of its pairs has um > 0.1: below that the autograd form's own
    # cancellation (eps64 / um^2) is what a difference would show
    row_ok, col_ok = (um > 0.1).all(1), (um > 0.1).all(0)
    assert int(row_ok.sum()) >= 3 and int(col_ok.sum()) >= 3
    for name in R.OUTPUTS:
        ok = row_ok if name in ('out', 'ga', 'gd', 'gs') else col_ok
        assert torch.allclose(new[name][ok], old[name][ok], rtol=1e-12, atol=1e-12), name
        assert torch.allclose(new[name][ok], torch.from_numpy(z[f'red_{case}_{name}'])[ok], rtol=1e-12, atol=1e-12), name
        if name not in ('gs', 'gos'):            # (there the new sums take the two pieces apart: larger by design)
            assert torch.allclose(new[name + '_abs'][ok], old[name + '_abs'][ok], rtol=1e-12, atol=1e-12), name
        else:
            assert bool((new[name + '_abs'] >= old[name + '_abs'] * (1 - 1e-12)).all())
        assert bool((new[name + '_cond'] >= new[name + '_abs']).all())


def test_stable_oracle_rows_subset_and_chunks():
    x = R.make('wide', 130, 9, 21, torch.float64)
    full = stable_oracle(*R.args_of(x), grad_out=x['go'])
    rows = torch.tensor([0, 3, 64, 65, 129])
    part = stable_oracle(*R.args_of(x), grad_out=x['go'], pairs_per_chunk=9 * 50, rows=rows)
    for name in R.OUTPUTS:
        for sfx in ('', '_abs', '_cond'):
            want = full[name + sfx][rows] if name in ('out', 'ga', 'gd', 'gs') else full[name + sfx]
            assert torch.allclose(part[name + sfx], want, rtol=1e-13, atol=0), name + sfx
    empty = stable_oracle(*[t[:0] for t in R.args_of(x)[:3]], *R.args_of(x)[3:], grad_out=x['go'][:0])
    assert empty['out'].shape == (0, 3) and empty['gs'].shape == (0,) and float(empty['goa'].abs().max()) == 0.


@pytest.mark.parametrize('case', R.FIXTURE_CASES[:-2], ids=CASE_IDS[:-2])
def test_fixture_float64_reference_vs_oracle(fx, case):
    """The reference's float64 autograd against the analytic oracle.  Where no pair has a small um they agree to a few
    eps64 cond; in `wide` and `antipodal` the autograd form loses eps64 / um^2 (measured: up to 1e-11 of cond), so the
    bound there is 1e-10 cond -- five orders below what a float32 result is asked for."""
    tag, x = R.case_tag(*case), R.case_inputs(fx, case)
    ref = stable_oracle(*R.args_of(x), grad_out=x['go'])
    k = 16. if case[0] in R.BOUND_FAMILIES else 1e-10 / float(torch.finfo(torch.float64).eps)
    for name in R.OUTPUTS:
        u = error_units(fx[f'{tag}_r64_{name}'], ref[name], ref[name + '_cond'])
        print(f'{tag} {name}: reference f64 vs oracle {u:.3g} eps64 cond')
        assert u <= k, name


@pytest.mark.parametrize('case', R.FIXTURE_CASES[-2:], ids=CASE_IDS[-2:])
def test_fixture_exact_zero_masks(fx, case):
    tag, x = R.case_tag(*case), R.case_inputs(fx, case)
    assert x['zero_rows'].tolist() == list(R.ZERO_ROWS) and x['zero_lights'].tolist() == list(R.ZERO_LIGHTS)
    assert torch.equal(x['d'][x['zero_rows']], -x['od'][x['zero_lights']])
    assert torch.equal(x['s'][x['zero_rows']], x['os'][x['zero_lights']])
    for name in R.OUTPUTS:
        mask = fx[f'{tag}_nan_{name}']
        want = torch.zeros_like(mask)
        want[x['zero_rows'] if name in ('out', 'ga', 'gd', 'gs') else x['zero_lights']] = True
        assert torch.equal(mask, want), name


def test_fixture_k32(fx):
    for f in R.BOUNDED:
        assert fx[f'K_ref_{f}'].shape == (7,) and bool(torch.isfinite(fx[f'K_ref_{f}']).all())
    print('K_ref', {f: [round(float(v), 3) for v in fx[f'K_ref_{f}']] for f in R.BOUNDED}, 'K32', fx['K32'])
    assert 1. < fx['K32'] < 8.          # 4 x an error of 0.25 .. 2 eps cond: anything else means the fixture is off


def test_pair_kernel_vs_mpmath():
    """G and G'(um) / um against 50-digit evaluations of 2 e^-lm sinh(um) / um and 2 e^-lm (um cosh um - sinh um) / um^3 on
    360 pairs, um from 1e-6 to 40 across the series threshold."""
    import mpmath
    mpmath.mp.dps = 50
    g = torch.Generator().manual_seed(31)
    um = torch.cat([torch.exp(torch.rand(300, generator=g, dtype=torch.float64) * math.log(4e7) + math.log(1e-6)),
                    torch.tensor([1. - 1e-12, 1., 1. + 1e-12, 0.999, 1.001, 1e-5], dtype=torch.float64),
                    torch.rand(54, generator=g, dtype=torch.float64) * 0.2])
    lm = um + torch.rand(um.shape, generator=g, dtype=torch.float64) * 100.
    G, D = pair_kernel(um, lm)
    worst = [0., 0.]
    for i in range(len(um)):
        u, l = mpmath.mpf(float(um[i])), mpmath.mpf(float(lm[i]))
        g_mp = 2 * mpmath.exp(-l) * mpmath.sinh(u) / u
        d_mp = 2 * mpmath.exp(-l) * (u * mpmath.cosh(u) - mpmath.sinh(u)) / u ** 3
        # in units of eps64 (1 + um + lm): the double nearest to um - lm is off by up to eps64 (um + lm) / 2 from the exact
        # difference, which no float64 evaluation of exp(um - lm) can undo
        unit = 2.220446049250313e-16 * (1. + float(um[i]) + float(lm[i]))
        worst[0] = max(worst[0], float(abs(mpmath.mpf(float(G[i])) - g_mp) / g_mp) / unit)
        worst[1] = max(worst[1], float(abs(mpmath.mpf(float(D[i])) - d_mp) / d_mp) / unit)
    print('pair_kernel vs mpmath, max relative error / (eps64 (1 + um + lm)): G %.3g, D %.3g' % tuple(worst))
    assert worst[0] <= 2. and worst[1] <= 4.
    G0, D0 = pair_kernel(torch.zeros(1, dtype=torch.float64), torch.full((1,), 3., dtype=torch.float64))
    assert float(G0) == pytest.approx(2 * math.exp(-3.), rel=1e-15) and float(D0) == pytest.approx(2 * math.exp(-3.) / 3, rel=1e-15)


def test_stable_oracle_gradients_vs_mpmath_differentiation():
    """All six gradients of a small antipodal case against 50-digit numerical differentiation of sum(out * grad_out), which
    shares nothing with the oracle but the definition of the product."""
    import mpmath
    mpmath.mp.dps = 50
    x = R.make('antipodal', 6, 3, 41, torch.float64)
    ref = stable_oracle(*R.args_of(x), grad_out=x['go'])
    p = {k: [[mpmath.mpf(float(v)) for v in row] for row in x[k].reshape(x[k].shape[0], -1).tolist()]
         for k in R.KEYS + ('go',)}

    def loss(p):
        total = mpmath.mpf(0)
        for i in range(6):
            for j in range(3):
                v = [p['s'][i][0] * p['d'][i][c] + p['os'][j][0] * p['od'][j][c] for c in range(3)]
                um = mpmath.sqrt(sum(t * t for t in v))
                G = (mpmath.exp(um - p['s'][i][0] - p['os'][j][0]) - mpmath.exp(-um - p['s'][i][0] - p['os'][j][0])) / um
                total += 2 * mpmath.pi * G * sum(p['go'][i][c] * p['a'][i][c] * p['oa'][j][c] for c in range(3))
        return total

    for key, name in zip(R.KEYS, GRADS):
        got = ref[name].reshape(ref[name].shape[0], -1)
        cond = ref[name + '_cond'].reshape(got.shape)
        for i in range(got.shape[0]):
            for c in range(got.shape[1]):
                def f(t):
                    q = dict(p)
                    q[key] = [list(r) for r in p[key]]
                    q[key][i][c] = t
                    return loss(q)
                want = mpmath.diff(f, p[key][i][c], h=mpmath.mpf(10) ** -20)
                err = float(abs(mpmath.mpf(float(got[i, c])) - want))
                assert err <= 8 * 2.2e-16 * float(cond[i, c]) + 1e-300, (name, i, c, err, float(cond[i, c]))


# ---- float32: the bound is reachable ----------------------------------------------------------------------------------

def _fma(a, b, c):
    """fma in float32: the product of two floats is exact in double; the sum is rounded to double and then to float (the
    double rounding differs from a true fma in about one case in 2^29)."""
    return (a.double() * b.double() + c.double()).float()


_LOG2E = torch.tensor(1.4426950408889634, dtype=torch.float32)


def _exp32(x):
    return torch.exp2(x * _LOG2E)


def _series(y, coeffs):
    p = torch.full_like(y, coeffs[0])
    for c in coeffs[1:]:
        p = _fma(p, y, torch.full_like(y, c))
    return p


_SINHC = [float(np.float32(1.) / np.float32(d)) for d in (39916800., 362880., 5040., 120., 6., 1.)]
_DSINHC = [float(np.float32(1.) / np.float32(d)) for d in (518918400., 3991680., 45360., 840., 30., 3.)]


def kernel_restatement_f32(a, d, s, oa, od, os_, go):
    """The arithmetic of csrc/sg_lighting.hip in float32 torch, light by light in order: v = s_i d_i + s_j d_j with both
    products rounded, um = um2 rsqrt(um2), exp as exp2(x log2 e), the 6-term series for 0 < um2 < 1, fma accumulation.
    (torch's rsqrt and exp2 stand in for v_rsq_f32 and v_exp_f32; the workgroup tree of the column sums is a plain sum.)"""
    n, m = a.shape[0], oa.shape[0]
    tp = torch.tensor(2 * math.pi, dtype=torch.float32)
    p = s[:, None] * d
    ga = go * a
    r = torch.zeros(n, 3)
    q_row = torch.zeros(n, 3)
    cA, cQ = torch.zeros(m, 3), torch.zeros(m, 3)
    for j in range(m):
        v = p + os_[j] * od[j][None]
        um2 = _fma(v[:, 2], v[:, 2], _fma(v[:, 1], v[:, 1], v[:, 0] * v[:, 0]))
        rs = torch.rsqrt(um2)
        um = um2 * rs
        lm = s + os_[j]
        E, E2 = _exp32(um - lm), _exp32(-um - lm)
        G = (E - E2) * rs
        dG = ((E + E2) - G) * rs * rs
        small = (um2 > 0) & (um2 < 1)
        E0 = 2 * _exp32(-lm)
        G = torch.where(small, E0 * _series(um2, _SINHC), G)
        dG = torch.where(small, E0 * _series(um2, _DSINHC), dG)
        h = _fma(ga[:, 2], oa[j, 2].expand(n), _fma(ga[:, 1], oa[j, 1].expand(n), ga[:, 0] * oa[j, 0]))
        q = h * dG
        r = _fma(oa[j][None].expand(n, 3), G[:, None].expand(n, 3), r)
        qv = q[:, None] * v
        q_row = _fma(q[:, None].expand(n, 3), v, q_row)
        cA[j] = (ga * G[:, None]).sum(0)
        cQ[j] = qv.sum(0)
    qd = _fma(q_row[:, 2], d[:, 2], _fma(q_row[:, 1], d[:, 1], q_row[:, 0] * d[:, 0]))
    gr = _fma(ga[:, 2], r[:, 2], _fma(ga[:, 1], r[:, 1], ga[:, 0] * r[:, 0]))
    cqd = _fma(cQ[:, 2], od[:, 2], _fma(cQ[:, 1], od[:, 1], cQ[:, 0] * od[:, 0]))
    caa = _fma(cA[:, 2], oa[:, 2], _fma(cA[:, 1], oa[:, 1], cA[:, 0] * oa[:, 0]))
    return {'out': tp * a * r, 'ga': tp * go * r, 'gd': (tp * s)[:, None] * q_row, 'gs': tp * (qd - gr),
            'goa': tp * cA, 'god': (tp * os_)[:, None] * cQ, 'gos': tp * (cqd - caa)}


@pytest.mark.parametrize('case', R.FIXTURE_CASES, ids=CASE_IDS)
def test_kernel_formula_in_float32_meets_the_bound(fx, case):
    """Forward and, beyond what fixes K32, all six gradients.  exact_zero: the NaN pattern too."""
    x = R.case_inputs(fx, case)
    got = kernel_restatement_f32(*R.args_of(x), x['go'])
    ref = stable_oracle(*R.args_of(x), grad_out=x['go'])
    for name in R.OUTPUTS:
        msg, needed, units = conditioned_mismatch(got[name], ref[name], ref[name + '_abs'], ref[name + '_cond'], fx['K32'],
                                                  allow_nan=R.nan_masks(x, name))
        print(f'{R.case_tag(*case)} {name}: {units:.3g} eps cond, {needed} of {got[name].numel()} needed the cond term')
        assert msg is None, f'{name}: {msg}'


@pytest.mark.parametrize('case', [c for c in R.FIXTURE_CASES if c[0] in R.BOUND_FAMILIES],
                         ids=[R.case_tag(*c) for c in R.FIXTURE_CASES if c[0] in R.BOUND_FAMILIES])
def test_cpu_fallback_float32_meets_the_bound(fx, case):
    """The CPU path of unbatched_reduced_sg_inner_product is the reference's torch chain and shares its cancellation at
    small um (K_ref of `wide` and `antipodal`): held to K32 in the families without it only."""
    x = R.case_inputs(fx, case)
    args = [t.clone().requires_grad_() for t in R.args_of(x)]
    out = sgm.unbatched_reduced_sg_inner_product(*args)
    grads = torch.autograd.grad((out * x['go']).sum(), args)
    ref = stable_oracle(*R.args_of(x), grad_out=x['go'])
    for name, t in zip(R.OUTPUTS, (out,) + grads):
        msg, needed, units = conditioned_mismatch(t, ref[name], ref[name + '_abs'], ref[name + '_cond'], fx['K32'])
        print(f'{R.case_tag(*case)} {name}: {units:.3g} eps cond, {needed} needed the cond term')
        assert msg is None, f'{name}: {msg}'


def test_rand01_control_needs_no_cond_term(fx):
    """The old regime (every input from rand(0, 1), golden case 100_65) through the new checker: nothing may pass thanks to
    the conditioned term that did not pass the existing bound."""
    z = np.load(os.path.join(GOLDEN_DIR, 'sg_lighting.npz'))
    args = [torch.from_numpy(z[f'red_100_65_{k}']).float() for k in R.KEYS]
    go = torch.from_numpy(z['red_100_65_go']).float()
    got = kernel_restatement_f32(*args, go)
    ref = stable_oracle(*args, grad_out=go)
    for name in R.OUTPUTS:
        msg, needed, _ = conditioned_mismatch(got[name], ref[name], ref[name + '_abs'], ref[name + '_cond'], fx['K32'])
        assert msg is None and needed == 0, (name, msg, needed)
