"""ops.conversions.FlexiCubes on the CPU: the generated case tables, the torch formulation against the reference's recorded results
(tests/golden/flexicubes.npz, made by tests/golden/make_golden_flexicubes.py), its error texts and ``construct_voxel_grid``.

The float bound ("FlexiCubes", has the derivation; u = 2^-24, A_d = max |x_d| over the grid, everything computed from the
INPUTS of a case in float64, never from a result under test):
    weights     a normalised weight w = tanh(raw) ws + 1 carries r_w = 5 |tanh(raw)| ws / w + 1 units of u (a tanh within
                2 ulp = 4 u, one product, one sum); gamma = sigmoid ws + (1 - ws) / 2 likewise with + 2; r = the largest over the tensor
    vertices    |got - want| <= n_v u A_d + u |want|,     n_v = 2 r_alpha + 2 r_beta + 20
    centres     the same with                             n_c = n_v + 4 r_gamma + 9
    L_dev       |got - want| <= (2 n_v + 44) u ||A||_2    (absolute: a difference of distances)
    gradients   |got - want| <= (2 n_c + 60) u amp T + u |want|, T = the sum of the magnitudes of the terms an element accumulates (one
                term per (dual vertex, edge) incidence and operand, from float64 autograd on the gathered operands), amp = 1 +
                max(A / h k_s, A / d): the cancellations inside a term -- h the shortest crossed edge, k_s = the largest
                (|w0| + |w1|) / min(|w0|, |w1|) of a crossed edge's weights, d the smallest distance of a zero crossing or a weighted edge
                point to its dual vertex.  For gamma_f the term of a (centre, corner) pair counts with 2 A in place of its difference
                P - centre of two points (a flat, regular quad has P = centre, and the error of either is relative to A).
                The raw weights add the cancellation in their derivative: 1 - tanh^2 carries 8 tanh^2 / (1 - tanh^2) units,
                sigmoid (1 - sigmoid) carries 4 sigmoid / (1 - sigmoid); the largest over the tensor is added to 2 n_c + 60.
                Precondition on the inputs (asserted): every L_dev with a cotangent other than 0 exceeds its own bound, so that
                its derivative sign(dist - mean) is settled (settle_cotangent zeroes the others)
The reference's own float32 results must pass the same bounds against its float64 results (test_reference_float32_passes_the_bound).
The gradients are judged a second time by the per-term bound of flexicubes_gradient_oracle.py (local conditioning factors).
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import flexicubes_gradient_oracle as oracle
from kaolin_amd.ops.conversions import FlexiCubes
from kaolin_amd.ops.conversions.flexicubes import flexicubes as fcm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
WS = 0.99


class Golden:
    _data = None

    @classmethod
    def get(cls):
        if cls._data is None:
            with np.load(os.path.join(ROOT, 'tests', 'golden', 'flexicubes.npz')) as z:
                cls._data = {k: z[k] for k in z.files}
        return cls._data


def tensor(name):
    g = Golden.get()
    return torch.from_numpy(g[name]) if name in g else None


def case_inputs(case):
    """(vertices, sdf, cubes, res, beta, alpha, gamma) of a stored case (weights None where the case has none)."""
    src = 'grid' if case in ('defaults', 'features') else case
    res = tuple(int(r) for r in Golden.get()[f'{src}_res'])
    weights = [None] * 3 if case == 'defaults' else [tensor(f'{src}_{n}') for n in ('beta', 'alpha', 'gamma')]
    return (tensor(f'{src}_vertices'), tensor(f'{src}_sdf'), tensor(f'{src}_cubes'), res, *weights)


def weight_units(raw, extra):
    """r_w of the module docstring, the largest over the tensor (1 for weights that are not given: exactly 1)."""
    if raw is None:
        return 1.0
    raw = raw.double().cpu()
    if extra == 1:
        t = torch.tanh(raw) * WS
        w = t + 1
    else:
        t = torch.sigmoid(raw) * WS
        w = t + (1 - WS) / 2
    return float((5 * t.abs() / w + extra).max())


def bounds(vertices, beta, alpha, gamma):
    """(n_v, n_c, A (3,) float64) of a call."""
    n_v = 2 * weight_units(alpha, 1) + 2 * weight_units(beta, 1) + 20
    n_c = n_v + 4 * weight_units(gamma, 2) + 9
    return n_v, n_c, vertices.double().abs().amax(0).cpu()


def assert_close(got, want, bound, what):
    """|got - want| <= bound elementwise; NaN exactly where want has NaN.  Returns the worst share of the bound."""
    got, want = got.detach().double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), f'{what}: NaN positions differ'
    if got.numel() == 0 or bool(nan.all()):
        return 0.0
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(want)
    share = ((got - want).abs() / bound)[~nan].max().item()
    print(f'{what}: worst share of the bound {share:.3f}')
    assert share <= 1.0, f'{what}: {share:.3f} of the bound'
    return share


def check_forward(got, want_verts, want_ldev, want_faces, inputs, num_vd, what):
    """got = (vertices, faces, L_dev) against float64 results; rows >= num_vd of the vertices are centres."""
    vertices, _, _, _, beta, alpha, gamma = inputs
    n_v, n_c, A = bounds(vertices, beta, alpha, gamma)
    assert got[1].dtype == torch.long and torch.equal(got[1].cpu(), want_faces), f'{what}: faces differ'
    n = torch.full((want_verts.shape[0], 1), n_v, dtype=torch.float64)
    n[num_vd:] = n_c
    shares = [assert_close(got[0], want_verts, n * U * A + U * want_verts.double().abs(), f'{what} vertices'),
              assert_close(got[2], want_ldev, (2 * n_v + 44) * U * float(A.norm()), f'{what} L_dev')]
    return max(shares)


def term_sums(inputs, cot_v, cot_l, training=True):
    """float64, from the torch formulation: (T per input tensor, amp) of the module docstring, and the float64 gradients."""
    vertices, sdf, cubes, res, beta, alpha, gamma = [t.double().cpu() if torch.is_tensor(t) and t.is_floating_point() else t
                                                     for t in inputs]
    cubes = cubes.cpu()
    topo = fcm.topology_torch(sdf, cubes, res)
    raw = dict(beta=beta, alpha=alpha, gamma=gamma)
    bn, an, gn = fcm.normalize_weights(beta, alpha, gamma, WS)
    ops = {k: v.detach().requires_grad_() for k, v in fcm.gather_operands(topo, vertices, sdf, bn, an, gn).items()}
    v, l, _ = fcm.numerics_gathered(mask=topo['mask'], quads=topo['quads'], training=training, **ops)
    ((v * cot_v.double().cpu()).sum() + (l * cot_l.double().cpu()).sum()).backward()
    mask, a, b, slots = topo['mask'], topo['a'], topo['b'], topo['slots']
    cube = topo['cubes'][topo['vd_cube']].unsqueeze(1).expand(-1, 7)
    e0 = torch.tensor([e[0] for e in fcm.CUBE_EDGES])
    e1 = torch.tensor([e[1] for e in fcm.CUBE_EDGES])
    g = {k: (t.grad.abs() if t.grad is not None else torch.zeros_like(t)) for k, t in ops.items()}
    T = dict(vertices=torch.zeros_like(vertices), sdf=torch.zeros_like(sdf))
    T['vertices'].index_add_(0, a[mask], g['x0'][mask])
    T['vertices'].index_add_(0, b[mask], g['x1'][mask])
    T['sdf'].index_add_(0, a[mask], g['s0'][mask])
    T['sdf'].index_add_(0, b[mask], g['s1'][mask])
    if alpha is not None:
        d = (WS * (1 - torch.tanh(alpha) ** 2)).reshape(-1)
        T['alpha'] = torch.zeros(alpha.numel(), dtype=torch.float64)
        T['alpha'].index_add_(0, (cube * 8 + e0[slots])[mask], g['al0'][mask])
        T['alpha'].index_add_(0, (cube * 8 + e1[slots])[mask], g['al1'][mask])
        T['alpha'] = (T['alpha'] * d).reshape(alpha.shape)
    if beta is not None:
        d = (WS * (1 - torch.tanh(beta) ** 2)).reshape(-1)
        T['beta'] = torch.zeros(beta.numel(), dtype=torch.float64)
        T['beta'].index_add_(0, (cube * 12 + slots)[mask], g['be'][mask])
        T['beta'] = (T['beta'] * d).reshape(beta.shape)
    if gamma is not None:
        # a centre sends gc . (P - centre) / wsum gamma_opposite to each of its four corners, P the midpoint of the corner's
        # diagonal: a difference of two points of magnitude A, so the term counts with 2 A in its place
        T_vd = torch.zeros_like(ops['gamma_vd'])
        if training and topo['quads'].shape[0] > 0:
            quads, gq = topo['quads'], ops['gamma_vd'].detach()[topo['quads']]
            wsum = gq[:, 0] * gq[:, 2] + gq[:, 1] * gq[:, 3] + 1e-8
            reach = (cot_v.double().cpu()[T_vd.shape[0]:].abs() * 2 * vertices.abs().amax(0)).sum(-1) / wsum
            for m in range(4):
                T_vd.index_add_(0, quads[:, m], reach * gq[:, m ^ 2])
        s = torch.sigmoid(gamma)
        T['gamma'] = torch.zeros_like(gamma).index_add_(0, cube[:, 0], T_vd) * (WS * s * (1 - s))
    # the cancellations inside a term
    with torch.no_grad():
        A = float(vertices.abs().max())
        h = float((ops['x0'] - ops['x1']).norm(dim=-1)[mask].min())
        w0, w1 = (ops['s1'] * ops['al1']).abs()[mask], (ops['s0'] * ops['al0']).abs()[mask]
        k_s = float(((w0 + w1) / torch.minimum(w0, w1)).max())
        vd = v[:topo['vd_cube'].shape[0]].detach()
        zc = fcm._interp(ops['s1'], -ops['s0'], ops['x0'], ops['x1'])
        d = float((zc - vd.unsqueeze(1)).norm(dim=-1)[mask].min())
        ue = fcm._interp(ops['s1'] * ops['al1'], -(ops['s0'] * ops['al0']), ops['x0'], ops['x1'])
        d = min(d, float((ue - vd.unsqueeze(1)).norm(dim=-1)[mask].min()))
        n_v, _, Avec = bounds(vertices, beta, alpha, gamma)
        live = cot_l.cpu() != 0
        assert not bool(live.any()) or float(l.abs()[live].min()) > (2 * n_v + 44) * U * float(Avec.norm()), \
            'the cotangent reaches an L_dev whose sign(dist - mean) hangs on rounding'
    return T, 1 + max(A / h * k_s, A / d)


def settle_cotangent(cot_l, l_dev64, inputs):
    """cot_l with zeros where the float64 L_dev lies within its bound of 0."""
    n_v, _, A = bounds(inputs[0], inputs[4], inputs[5], inputs[6])
    return torch.where(l_dev64.cpu().abs() > 2 * (2 * n_v + 44) * U * float(A.norm()), cot_l, torch.zeros_like(cot_l))


def derivative_units(name, raw):
    """What the derivative of the normalisation adds to the operation count of a raw weight's gradient."""
    if raw is None or name not in ('beta', 'alpha', 'gamma'):
        return 0.0
    raw = raw.double().cpu()
    if name == 'gamma':
        s = torch.sigmoid(raw)
        return float((4 * s / (1 - s)).max())
    t2 = torch.tanh(raw) ** 2
    return float((8 * t2 / (1 - t2)).max())


def check_grads(got, want, inputs, cot_v, cot_l, what):
    """got, want: dicts name -> gradient; want in float64."""
    _, n_c, _ = bounds(inputs[0], inputs[4], inputs[5], inputs[6])
    T, amp = term_sums(inputs, cot_v, cot_l)
    worst = 0.0
    raw = dict(beta=inputs[4], alpha=inputs[5], gamma=inputs[6])
    for name, w in want.items():
        if w is None:
            assert got[name] is None, name
            continue
        bound = (2 * n_c + 60 + derivative_units(name, raw.get(name))) * U * amp * T[name] + U * w.double().abs().cpu() + 1e-300
        worst = max(worst, assert_close(got[name], w, bound, f'{what} grad {name}'))
    return worst


def run_torch(case, training, dtype=torch.float32, features=None):
    v, s, c, res, beta, alpha, gamma = case_inputs(case)
    cast = [None if t is None else t.to(dtype) for t in (v, s, beta, alpha, gamma, features)]
    return FlexiCubes('cpu')(cast[0], cast[1], c, list(res), beta=cast[2], alpha=cast[3], gamma_f=cast[4], training=training,
                             voxelgrid_features=cast[5])


def forward_cases():
    cases = [('grid', False), ('grid', True), ('defaults', False), ('defaults', True), ('zeros', False), ('zeros', True)]
    return cases + [(f'invert{i}', False) for i in range(int(Golden.get()['invert_count']))]


def check_case(fn, case, training):
    """fn(vertices, sdf, cubes, res, beta, alpha, gamma, training) -> (vertices, faces, L_dev) against the stored float64."""
    tag = f'{case}_train' if training else case
    inputs = case_inputs(case)
    got = fn(*inputs, training)
    faces = tensor(f'{tag}_faces')
    num_vd = tensor(f'{tag}_verts_f64').shape[0] - (faces.shape[0] // 4 if training else 0)
    return check_forward(got, tensor(f'{tag}_verts_f64'), tensor(f'{tag}_ldev_f64'), faces, inputs, num_vd, tag)


def check_cases256(fn):
    """fn as in check_case, called once per sign pattern."""
    g = Golden.get()
    v, mag, c = tensor('cases256_vertices'), tensor('cases256_mag'), tensor('cases256_cubes')
    beta, alpha = tensor('cases256_beta'), tensor('cases256_alpha')
    nv, nl = np.cumsum(np.r_[0, g['cases256_nv']]), np.cumsum(np.r_[0, g['cases256_nl']])
    for case in range(256):
        bits = (case >> torch.arange(8)) & 1
        sdf = torch.zeros(8).scatter(0, c[0], torch.where(bits.bool(), -mag, mag))
        got = fn(v, sdf, c, (1, 1, 1), beta, alpha, None, False)
        check_forward(got, tensor('cases256_verts_f64')[nv[case]:nv[case + 1]], tensor('cases256_ldev_f64')[nl[case]:nl[case + 1]],
                      torch.zeros((0, 3), dtype=torch.long), (v, sdf, c, (1, 1, 1), beta, alpha, None), int(g['cases256_nv'][case]),
                      f'case {case}')


def torch_call(v, s, c, res, beta, alpha, gamma, training):
    return FlexiCubes('cpu')(v, s, c, list(res), beta=beta, alpha=alpha, gamma_f=gamma, training=training)


def test_table_is_generated():
    done = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_flexicubes_table.py'), '--check'], capture_output=True,
                          text=True)
    assert done.returncode == 0, done.stdout + done.stderr


def test_cases256():
    check_cases256(torch_call)


@pytest.mark.parametrize('case,training', forward_cases())
def test_golden_forward(case, training):
    check_case(torch_call, case, training)


@pytest.mark.parametrize('case,training', [('grid', True), ('invert0', False)])
def test_golden_forward_float64(case, training):
    """float64 inputs: float64 results, within float64 rounding of the reference's."""
    tag = f'{case}_train' if training else case
    got = run_torch(case, training, torch.float64)
    assert got[0].dtype == torch.float64 and got[2].dtype == torch.float64
    assert torch.equal(got[1], tensor(f'{tag}_faces'))
    assert torch.allclose(got[0], tensor(f'{tag}_verts_f64'), rtol=1e-12, atol=1e-13)
    assert torch.allclose(got[2], tensor(f'{tag}_ldev_f64'), rtol=0, atol=1e-12)


@pytest.mark.parametrize('name', ['empty_pos', 'empty_neg'])
def test_empty(name):
    got = torch_call(*case_inputs(name), False)
    assert got[0].shape == (0, 3) and got[1].shape == (0, 3) and got[2].shape == (0,)
    assert got[0].dtype == torch.float32 and got[1].dtype == torch.long and got[2].dtype == torch.float32
    v, s, c, res = case_inputs(name)[:4]
    got = FlexiCubes('cpu')(v, s, c, 2, voxelgrid_features=torch.zeros(v.shape[0], 5))
    assert len(got) == 4 and got[3].shape == (0, 5)


def test_features():
    feats = tensor('features_feats')
    got = run_torch('features', False, features=feats)
    inputs = case_inputs('features')
    check_forward(got[:3], tensor('features_verts_f64'), tensor('features_ldev_f64'), tensor('features_faces'), inputs,
                  got[0].shape[0], 'features')
    n_v = bounds(inputs[0], inputs[4], inputs[5], inputs[6])[0]
    want = tensor('features_feats_f64')
    assert_close(got[3], want, n_v * U * feats.double().abs().amax(0) + U * want.abs(), 'features feats')
    # training: the reference fails in its own cat; ours appends the centres' features, weighted like the centres
    got_t = run_torch('features', True, torch.float64, features=feats)
    nq = tensor('grid_train_faces').shape[0] // 4
    assert got_t[3].shape == (want.shape[0] + nq, 5) and torch.allclose(got_t[3][:-nq], want, rtol=1e-12, atol=1e-13)
    assert torch.allclose(got_t[0], tensor('grid_train_verts_f64'), rtol=1e-12, atol=1e-13)


def grads_of(fn, inputs, cot_v, cot_l, dtype, device='cpu'):
    v, s, c, res, beta, alpha, gamma = inputs
    leaves = [t.to(device=device, dtype=dtype).clone().requires_grad_() for t in (v, s, beta, alpha, gamma)]
    out = fn(leaves[0], leaves[1], c.to(device), res, leaves[2], leaves[3], leaves[4], True)
    ((out[0] * cot_v.to(device=device, dtype=dtype)).sum() + (out[2] * cot_l.to(device=device, dtype=dtype)).sum()).backward()
    return dict(zip(('vertices', 'sdf', 'beta', 'alpha', 'gamma'), [t.grad for t in leaves]))


def golden_grads(tag):
    return {n: tensor(f'grads_{n}_{tag}') for n in ('vertices', 'sdf', 'beta', 'alpha', 'gamma')}


def test_golden_grads():
    inputs = case_inputs('grid')
    cot_v, cot_l = tensor('grads_cot_verts'), tensor('grads_cot_ldev')
    got64 = grads_of(torch_call, inputs, cot_v, cot_l, torch.float64)
    for name, want in golden_grads('f64').items():
        assert torch.allclose(got64[name], want, rtol=1e-9, atol=1e-12), name
    got32 = grads_of(torch_call, inputs, cot_v, cot_l, torch.float32)
    check_grads(got32, golden_grads('f64'), inputs, cot_v, cot_l, 'torch f32')
    oracle.check_grads_local(got32, golden_grads('f64'), inputs, cot_v, cot_l, True, 'torch f32')


def test_reference_float32_passes_the_bound():
    """The condition on the bound: the reference's own float32 results lie within it of its float64 results."""
    g = Golden.get()
    for case, training in forward_cases():
        tag = f'{case}_train' if training else case
        check_case(lambda *a, tag=tag: (tensor(f'{tag}_verts_f32'), tensor(f'{tag}_faces'), tensor(f'{tag}_ldev_f32')), case, training)
    nv, nl = np.cumsum(np.r_[0, g['cases256_nv']]), np.cumsum(np.r_[0, g['cases256_nl']])
    state = {'case': 0}

    def stored(*_):
        k = state['case']
        state['case'] += 1
        return (tensor('cases256_verts_f32')[nv[k]:nv[k + 1]], torch.zeros((0, 3), dtype=torch.long),
                tensor('cases256_ldev_f32')[nl[k]:nl[k + 1]])
    check_cases256(stored)
    check_grads(golden_grads('f32'), golden_grads('f64'), case_inputs('grid'), tensor('grads_cot_verts'), tensor('grads_cot_ldev'),
                'reference f32')
    oracle.check_grads_local(golden_grads('f32'), golden_grads('f64'), case_inputs('grid'), tensor('grads_cot_verts'),
                             tensor('grads_cot_ldev'), True, 'reference f32')


def test_half_runs():
    v, s, c, res, beta, alpha, gamma = case_inputs('grid')
    got = FlexiCubes('cpu')(v.half(), s.half(), c, list(res), beta=beta.half(), alpha=alpha.half(), gamma_f=gamma.half(), training=True)
    assert got[0].dtype == torch.float16 and got[2].dtype == torch.float16 and got[1].shape[1] == 3


def test_errors():
    g = Golden.get()
    v, s, c, res, beta, alpha, gamma = case_inputs('grid')
    feats = tensor('features_feats')
    fc = FlexiCubes('cpu')
    nc = c.shape[0]
    calls = dict(vertices=lambda: fc(v[:, :2], s, c, res), sdf=lambda: fc(v, s[:-1], c, res), cubes=lambda: fc(v, s, c[:, :7], res),
                 beta=lambda: fc(v, s, c, res, beta=torch.zeros(nc, 11)), alpha=lambda: fc(v, s, c, res, alpha=torch.zeros(nc - 1, 8)),
                 gamma=lambda: fc(v, s, c, res, gamma_f=torch.zeros(nc, 1)),
                 features=lambda: fc(v, s, c, res, voxelgrid_features=feats[:-1]),
                 features_tetmesh=lambda: fc(v, s, c, res, voxelgrid_features=feats, output_tetmesh=True))
    for name, call in calls.items():
        kind, text = g[f'err_{name}']
        with pytest.raises(AssertionError if kind == 'AssertionError' else Exception) as err:
            call()
        assert type(err.value).__name__ == kind and str(err.value) == text, name


def test_not_implemented():
    v, s, c, res = case_inputs('grid')[:4]
    fc = FlexiCubes('cpu')
    with pytest.raises(NotImplementedError, match='output_tetmesh'):
        fc(v, s, c, res, output_tetmesh=True)
    with pytest.raises(NotImplementedError, match='grad_func'):
        fc(v, s, c, res, grad_func=lambda p: p)
    with pytest.raises(ValueError, match='cube_idx'):
        fc(v, s, c[:-1], res)


@pytest.mark.parametrize('i,res', [(0, 1), (1, 4), (2, (5, 3, 4)), (2, [5, 3, 4])])
def test_construct_voxel_grid(i, res):
    verts, cubes = FlexiCubes('cpu').construct_voxel_grid(res)
    assert verts.dtype == torch.float32 and cubes.dtype == torch.long
    assert torch.equal(verts, tensor(f'construct_{i}_verts')) and torch.equal(cubes, tensor(f'construct_{i}_cubes'))


def test_installs_as_kaolin():
    import kaolin_amd
    kaolin_amd.install_as_kaolin()
    import kaolin as kal
    assert kal.ops.conversions.FlexiCubes is FlexiCubes
    from kaolin.ops.conversions.flexicubes import FlexiCubes as same
    assert same is FlexiCubes
