"""The boundary cases of tests/flexicubes_boundary_cases.py are what their names say, and the per-term gradient bound of
tests/flexicubes_gradient_oracle.py meets its three conditions ("FlexiCubes", "The float bound"):
    (a) float32 evaluations pass it: the reference's recorded float32 gradients, and the float32 torch formulation at every case;
    (b) it is elementwise no larger than the same terms under the grid-wide factor, and for vertices no larger than the bound of
        test_flexicubes_cpu.py (for sdf it cannot be: that bound sums net terms, which fails (a) -- see the oracle's docstring);
    (c) it REJECTS gradients that miss the contribution of one surface cube, at the ranks around the workgroup boundary.
Shares of the bound measured here with the float32 formulation (worst over the cases): see DESIGN.md."""
import itertools

import pytest
import torch

import flexicubes_boundary_cases as cases
import flexicubes_gradient_oracle as oracle
import test_flexicubes_cpu as base
from kaolin_amd.ops.conversions.flexicubes import flexicubes as fcm
from kaolin_amd.ops.conversions.flexicubes._tables import NUM_VD_TABLE

ALL = list(cases.CASES)
_SETUPS = {}


def formulation_fn(v, s, c, r, beta, alpha, gamma, training):
    return fcm.flexicubes_torch(v, s, c, r, base.WS, beta, alpha, gamma, training)[:3]


def cotangents(inputs, training=True, seed=29):
    v, s, c, res, beta, alpha, gamma = inputs
    with torch.no_grad():
        out = formulation_fn(v.double(), s.double(), c, res, *[None if t is None else t.double() for t in (beta, alpha, gamma)], training)
    g = torch.Generator().manual_seed(seed)
    cot_v = (torch.rand(out[0].shape, generator=g) * 2 - 1).float()
    return cot_v, base.settle_cotangent((torch.rand(out[2].shape, generator=g) * 2 - 1).float(), out[2], inputs)


def setup(name):
    """(inputs, cot_v, cot_l, float64 autograd gradients) of a case, computed once and left unchanged."""
    if name not in _SETUPS:
        inputs = cases.case_inputs(name)
        cot_v, cot_l = cotangents(inputs)
        _SETUPS[name] = (inputs, cot_v, cot_l, base.grads_of(formulation_fn, inputs, cot_v, cot_l, torch.float64))
    return _SETUPS[name]


@pytest.mark.parametrize('name', ALL)
def test_case_sits_where_its_name_says(name):
    res, kind, seed, S, Q = cases.CASES[name]
    v, s, c, res3, beta, alpha, gamma = cases.case_inputs(name)
    topo = fcm.topology_torch(s, c, res3)
    codes = cases.case_codes(s, c)
    assert topo['cubes'].shape[0] == S == int(((codes > 0) & (codes < 255)).sum())
    assert topo['quads'].shape[0] == Q
    if kind == 'plane':
        assert S == res[0] * res[1] and Q == (res[0] - 1) * (res[1] - 1) and res[2] == 3
    per_cube = torch.bincount(topo['vd_cube'], minlength=S)
    if name == 'signs_1x1x1':
        assert per_cube.tolist() == [3]
    if name == 'signs_1x1x4':
        assert per_cube.tolist() == [2, 1, 3, 2]
    if name in ('signs_8x8x5', 'signs_10x10x8'):
        assert S > cases.BLOCK and sorted(set(per_cube.tolist())) == [1, 2, 3, 4]
        # dual vertices of one cube in different workgroups' ranges: a cube of 4 after 256 dual vertices of the classes below
        assert int((per_cube < 4).sum()) > cases.BLOCK


def test_block_boundaries_are_covered():
    S = sorted(c[3] for c in cases.CASES.values())
    Q = sorted(c[4] for c in cases.CASES.values())
    for n in (255, 256, 257, 258, 516, 1023, 1024):
        assert n in S
    for n in (0, 255, 256, 257):
        assert n in Q


def test_a_signs_case_holds_an_inverted_cube():
    v, s, c, res, *_ = cases.case_inputs('signs_8x8x5')
    inverted = cases.inverted_cubes(s, c, res)
    assert len(inverted) > 0
    # the formulation's dual-vertex counts are those of the REPLACED case at these cubes
    topo = fcm.topology_torch(s, c, res)
    codes = cases.case_codes(s, c)
    per_cube = dict(zip(topo['cubes'].tolist(), torch.bincount(topo['vd_cube']).tolist()))
    assert all(per_cube[k] == NUM_VD_TABLE[255 - int(codes[k])] for k in inverted)
    assert any(NUM_VD_TABLE[255 - int(codes[k])] != NUM_VD_TABLE[int(codes[k])] for k in inverted)


@pytest.mark.parametrize('training', [False, True])
@pytest.mark.parametrize('name', ['Q256', 'signs_8x8x5', 'signs_1x1x4', 'S257_Q0'])
def test_gathered_grads_are_autograd(name, training):
    """Without drop_cube the scatter of the per-incidence gradients equals plain float64 autograd of flexicubes_torch: both sum the
    same float64 terms, in another order, so they differ by a few units of 2^-53 of the summed magnitudes."""
    inputs = cases.case_inputs(name)
    cot_v, cot_l = cotangents(inputs, training)
    v, s, c, res, beta, alpha, gamma = inputs
    leaves = [t.double().clone().requires_grad_() for t in (v, s, beta, alpha, gamma)]
    out = formulation_fn(leaves[0], leaves[1], c, res, leaves[2], leaves[3], leaves[4], training)
    ((out[0] * cot_v.double()).sum() + (out[2] * cot_l.double()).sum()).backward()
    want = dict(zip(oracle.NAMES, [t.grad for t in leaves]))
    got = oracle.gathered_grads(inputs, cot_v, cot_l, training)
    T, _ = base.term_sums(inputs, cot_v, cot_l, training)
    for k in oracle.NAMES:
        if want[k] is None:
            assert got[k] is None and k == 'gamma' and not training
            continue
        err = float((got[k] - want[k]).abs().max())
        print(f'{name} training={training} {k}: gathered - autograd {err:.2e}')
        assert bool(((got[k] - want[k]).abs() <= 32 * 2.0 ** -53 * (T[k] + want[k].abs())).all()), k
        assert err <= 1e-13
    if cases.CASES[name][4] == 0 and training:
        assert not bool(got['gamma'].any())


def test_reference_float32_passes_the_local_bound():
    """(a) the reference's own float32 gradients."""
    inputs = base.case_inputs('grid')
    oracle.check_grads_local(base.golden_grads('f32'), base.golden_grads('f64'), inputs, base.tensor('grads_cot_verts'),
                             base.tensor('grads_cot_ldev'), True, 'reference f32')


@pytest.mark.parametrize('name', ALL)
def test_float32_formulation_passes_the_local_bound(name):
    """(a) the float32 torch formulation on the CPU against its own float64, at every case."""
    inputs, cot_v, cot_l, want = setup(name)
    got = base.grads_of(formulation_fn, inputs, cot_v, cot_l, torch.float32)
    oracle.check_grads_local(got, want, inputs, cot_v, cot_l, True, f'torch f32 {name}')


SUBSETS = [s for k in range(4) for s in itertools.combinations(('beta', 'alpha', 'gamma'), k)]


@pytest.mark.parametrize('training', [False, True])
@pytest.mark.parametrize('given', SUBSETS, ids=lambda s: '+'.join(s) or 'none')
@pytest.mark.parametrize('name', cases.OPTION_CASES)
def test_float32_formulation_passes_the_local_bound_at_every_option(name, given, training):
    """(a) at the option matrix of the GPU tests: every subset of the weights, with and without training."""
    full = cases.case_inputs(name)
    inputs = (*full[:4], *[w if n in given else None for n, w in zip(('beta', 'alpha', 'gamma'), full[4:7])])
    cot_v, cot_l = cotangents(inputs, training)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        leaves = [None if t is None else t.to(dtype).clone().requires_grad_() for t in (inputs[0], inputs[1], *inputs[4:7])]
        out = formulation_fn(leaves[0], leaves[1], inputs[2], inputs[3], leaves[2], leaves[3], leaves[4], training)
        ((out[0] * cot_v.to(dtype)).sum() + (out[2] * cot_l.to(dtype)).sum()).backward()
        grads[dtype] = dict(zip(oracle.NAMES, [None if t is None else t.grad for t in leaves]))
    oracle.check_grads_local(grads[torch.float32], grads[torch.float64], inputs, cot_v, cot_l, training, f'torch f32 {name} {given}')


@pytest.mark.parametrize('name', ALL + ['golden'])
def test_local_bound_is_no_larger(name):
    """(b) the same terms with amp_vd <= amp, for every tensor; for vertices these are the terms of test_flexicubes_cpu.py, so
    the local bound is elementwise no larger than that one.  The ratio for sdf is printed."""
    if name == 'golden':
        inputs, cot_v, cot_l = base.case_inputs('grid'), base.tensor('grads_cot_verts'), base.tensor('grads_cot_ldev')
    else:
        inputs, cot_v, cot_l, _ = setup(name)
    T, amp = base.term_sums(inputs, cot_v, cot_l)
    local = oracle.term_magnitudes(inputs, cot_v, cot_l)
    wide = oracle.term_magnitudes(inputs, cot_v, cot_l, amp=amp)
    for k in ('vertices', 'sdf', 'beta', 'alpha'):
        assert bool((local[k] <= wide[k] * (1 + 1e-12)).all()), k
    assert bool((local['vertices'] <= amp * T['vertices'] * (1 + 1e-12)).all())
    for k in ('vertices', 'sdf'):
        live = T[k] > 0
        ratio = local[k][live] / (amp * T[k][live])
        print(f'{name} {k}: local / global bound, median {float(ratio.median()):.3g}, largest {float(ratio.max()):.3g}')


@pytest.mark.parametrize('name', ALL)
def test_a_dropped_cube_is_rejected(name):
    """(c) a backward whose thread of surface cube `rank` did nothing: rejected on vertices or sdf and on that cube's own rows
    of beta and alpha, and on no other row of the weights.  gamma: the gradient of a quad that is flat within rounding
    (P = centre to K u 2 A) is below what float32 can resolve, so a missing gamma row is not observable at every cube; the
    bound must still reject a missing gamma row at more than 9 in 10 of the cubes that have a quad."""
    inputs, cot_v, cot_l, want = setup(name)
    topo = fcm.topology_torch(inputs[1], inputs[2], inputs[3])
    S = topo['cubes'].shape[0]
    for rank in sorted({r for r in (0, cases.BLOCK - 1, cases.BLOCK, S - 1) if r < S}):
        got = oracle.gathered_grads(inputs, cot_v, cot_l, True, drop_cube=rank)
        shares = oracle.grad_shares(got, want, inputs, cot_v, cot_l, True)
        cube = int(topo['cubes'][rank])
        over = dict(shared=max(float(shares['vertices'].max()), float(shares['sdf'].max())), beta=float(shares['beta'][cube].max()),
                    alpha=float(shares['alpha'][cube].max()), gamma=float(shares['gamma'][cube]))
        print(f'{name} rank {rank}: the dropped cube exceeds the bound by ' + ', '.join(f'{k} {x:.3g}x' for k, x in over.items()))
        assert over['shared'] > 1 and over['beta'] > 1 and over['alpha'] > 1
        for k in ('beta', 'alpha', 'gamma'):
            rest = shares[k].clone()
            rest[cube] = 0
            assert float(rest.max()) <= 1, k
    if topo['quads'].shape[0] > 0:
        with_quad = torch.unique(topo['cubes'][topo['vd_cube'][topo['quads'].reshape(-1)]])
        missing = oracle.grad_shares(dict(want, gamma=torch.zeros_like(want['gamma'])), want, inputs, cot_v, cot_l, True)['gamma']
        rejected = float((missing[with_quad] > 1).double().mean())
        print(f'{name}: a missing gamma row is rejected at {rejected:.3f} of the cubes with a quad, median '
              f'{float(missing[with_quad].median()):.3g}x the bound')
        assert rejected > 0.9
    else:
        assert not bool(want['gamma'].any())
