"""The backward of ops.conversions.FlexiCubes (csrc/flexicubes.hip, fc_backward_kernel) past one workgroup and on the paths its
first tests never ran: the cases of tests/flexicubes_boundary_cases.py, every subset of the weights with and without training,
strided and sparse ids, non-contiguous floats, interleaved calls, a side stream, and every id width of the pair sort.

The yardstick of a gradient is float64 autograd of the torch formulation on the same GPU, judged by the per-term bound of
tests/flexicubes_gradient_oracle.py (check_grads_local); cotangents of L_dev come from settle_cotangent.  Where the kernel uses no
atomics (beta, alpha, gamma_f; the whole forward) two calls that see the same values must give the same bits."""
import itertools

import pytest
import torch

import flexicubes_boundary_cases as cases
import flexicubes_gradient_oracle as oracle
from kaolin_amd.ops.conversions import FlexiCubes
from kaolin_amd.ops.conversions.flexicubes import flexicubes as fcm
from test_flexicubes_cpu import WS, settle_cotangent

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FLOATS = ('vertices', 'sdf', 'beta', 'alpha', 'gamma')
WEIGHTS = ('beta', 'alpha', 'gamma')
_SETUPS = {}


def hip_fn(v, s, c, res, beta, alpha, gamma, training):
    return FlexiCubes(DEV)(v, s, c, list(res), beta=beta, alpha=alpha, gamma_f=gamma, training=training)


def formulation_fn(v, s, c, res, beta, alpha, gamma, training):
    return fcm.flexicubes_torch(v, s, c, res, WS, beta, alpha, gamma, training)[:3]


def leaves_of(inputs, dtype, requires=FLOATS):
    """name -> a fresh leaf on the GPU (None for a weight that is None); only the names in ``requires`` require a gradient."""
    v, s, _, _, beta, alpha, gamma = inputs
    return {n: None if t is None else t.to(device=DEV, dtype=dtype).clone().requires_grad_(n in requires)
            for n, t in zip(FLOATS, (v, s, beta, alpha, gamma))}


def backward(fn, inputs, cot_v, cot_l, dtype, training=True, requires=FLOATS, leaves=None, cubes=None):
    """-> (name -> gradient or None, the forward's results)."""
    leaves = leaves_of(inputs, dtype, requires) if leaves is None else leaves
    cubes = inputs[2].to(DEV) if cubes is None else cubes
    out = fn(leaves['vertices'], leaves['sdf'], cubes, inputs[3], leaves['beta'], leaves['alpha'], leaves['gamma'], training)
    ((out[0] * cot_v.to(device=DEV, dtype=dtype)).sum() + (out[2] * cot_l.to(device=DEV, dtype=dtype)).sum()).backward()
    return {n: None if t is None else t.grad for n, t in leaves.items()}, out


def cotangents(inputs, training, seed=29):
    """CPU float32 cotangents of (vertices, L_dev); those of an L_dev within twice its bound of 0 are zero."""
    with torch.no_grad():
        cast = [None if t is None else t.to(device=DEV, dtype=torch.float64) for t in (inputs[0], inputs[1], *inputs[4:7])]
        out = formulation_fn(cast[0], cast[1], inputs[2].to(DEV), inputs[3], cast[2], cast[3], cast[4], training)
    g = torch.Generator().manual_seed(seed)
    cot_v = (torch.rand(out[0].shape, generator=g) * 2 - 1).float()
    return cot_v, settle_cotangent((torch.rand(out[2].shape, generator=g) * 2 - 1).float(), out[2].cpu(), inputs)


def reference(inputs, training=True, requires=FLOATS):
    """(cot_v, cot_l, float64 autograd gradients on the CPU) of some inputs."""
    cot_v, cot_l = cotangents(inputs, training)
    want, _ = backward(formulation_fn, inputs, cot_v, cot_l, torch.float64, training, requires)
    return cot_v, cot_l, {n: None if w is None else w.cpu() for n, w in want.items()}


def setup(name):
    """(inputs, cot_v, cot_l, want) of a named case: training, all weights; computed once, shared and left unchanged."""
    if name not in _SETUPS:
        inputs = cases.case_inputs(name)
        _SETUPS[name] = (inputs, *reference(inputs))
    return _SETUPS[name]


def only(grads, names):
    return {n: grads[n] for n in names}


def assert_same_bits(a, b, names, what):
    for n in names:
        assert (a[n] is None) == (b[n] is None), f'{what}: {n}'
        assert a[n] is None or torch.equal(a[n], b[n]), f'{what}: the {n} gradients differ'


@pytest.mark.parametrize('name', list(cases.CASES))
def test_backward_at_every_case(name):
    inputs, cot_v, cot_l, want = setup(name)
    got, out = backward(hip_fn, inputs, cot_v, cot_l, torch.float32)
    assert out[0].shape == cot_v.shape and out[2].shape == cot_l.shape
    for n in FLOATS:
        assert got[n].dtype == torch.float32 and got[n].shape == want[n].shape, n
    oracle.check_grads_local(got, want, inputs, cot_v, cot_l, True, f'hip {name}')
    if cases.CASES[name][4] == 0:                               # no quads: gamma_f moves nothing, its gradient is zero -- not None
        assert out[1].shape[0] == 0 and got['gamma'] is not None and not bool(got['gamma'].any())


SUBSETS = [s for k in range(4) for s in itertools.combinations(WEIGHTS, k)]


@pytest.mark.parametrize('training', [False, True])
@pytest.mark.parametrize('given', SUBSETS, ids=lambda s: '+'.join(s) or 'none')
@pytest.mark.parametrize('name', cases.OPTION_CASES)
def test_option_matrix(name, given, training):
    """Every subset of the weights, with and without training: a gradient is None exactly for a weight that is None and for
    gamma_f without training (it only picks the split), and every other one lies within the bound."""
    full = cases.case_inputs(name)
    inputs = (*full[:4], *[w if n in given else None for n, w in zip(WEIGHTS, full[4:7])])
    cot_v, cot_l, want = reference(inputs, training)
    for n in WEIGHTS:
        assert (want[n] is None) == (n not in given or (n == 'gamma' and not training)), n
    got, _ = backward(hip_fn, inputs, cot_v, cot_l, torch.float32, training)
    oracle.check_grads_local(got, want, inputs, cot_v, cot_l, training, f'hip {name} {given} training={training}')


@pytest.mark.parametrize('requires', [('sdf',), WEIGHTS], ids=['sdf', 'weights'])
@pytest.mark.parametrize('name', cases.OPTION_CASES)
def test_requires_grad_on_a_part_of_the_inputs(name, requires):
    inputs, cot_v, cot_l, want = setup(name)
    got, _ = backward(hip_fn, inputs, cot_v, cot_l, torch.float32, True, requires)
    for n in FLOATS:
        assert (got[n] is None) == (n not in requires), n
    oracle.check_grads_local(only(got, requires), only(want, requires), inputs, cot_v, cot_l, True, f'hip {name} requires {requires}')


@pytest.mark.parametrize('name', ['S1024', 'signs_10x10x8'])
def test_weight_gradients_do_not_vary_from_run_to_run(name):
    """beta, alpha and gamma_f rows are written by their owner: the same bits every time.  Vertices and sdf take float atomics:
    within the bound every time."""
    inputs, cot_v, cot_l, want = setup(name)
    first, _ = backward(hip_fn, inputs, cot_v, cot_l, torch.float32)
    second, _ = backward(hip_fn, inputs, cot_v, cot_l, torch.float32)
    assert_same_bits(first, second, WEIGHTS, name)
    for k, got in enumerate((first, second)):
        oracle.check_grads_local(got, want, inputs, cot_v, cot_l, True, f'hip {name} run {k}')


def quad_keys(faces, num_vd):
    """One key per quad of a training result: its four dual vertices in corner order."""
    rows = faces.reshape(-1, 4, 3)[:, :, 0].cpu()
    return ((rows[:, 0] * num_vd + rows[:, 1]) * num_vd + rows[:, 2]) * num_vd + rows[:, 3]


def test_backward_through_strided_cubes_and_sparse_ids():
    """A transposed cube_idx whose ids are mapped sparsely, NOT monotonely, into [0, 70 001): the kernel reads ids through the
    strides and scatters by id.  The map changes the order of the quads (their edges rank by id) and nothing else: with the
    cotangents of the centres carried along, the weights' gradients have the dense contiguous call's bits, the gradients of
    vertices and sdf lie within the bound at the mapped rows and are exactly zero at all others."""
    inputs, cot_v, cot_l, want = setup('signs_8x8x5')
    v, s, c, res, beta, alpha, gamma = inputs
    dense, dense_out = backward(hip_fn, inputs, cot_v, cot_l, torch.float32)
    V = 70001
    ids = torch.randperm(V - 1, generator=torch.Generator().manual_seed(12))[:v.shape[0]]
    ids[int(c[c.shape[0] // 2, 3])] = V - 1
    assert not bool((ids[1:] > ids[:-1]).all())
    big_v, big_s = torch.zeros(V, 3), torch.full((V,), -1.0)
    big_v[ids], big_s[ids] = v, s
    sparse_inputs = (big_v, big_s, ids[c], res, beta, alpha, gamma)
    cubes = ids[c].to(DEV).t().contiguous().t()                 # strides (1, C)
    assert not cubes.is_contiguous()
    with torch.no_grad():
        out = hip_fn(big_v.to(DEV), big_s.to(DEV), cubes, res, beta.to(DEV), alpha.to(DEV), gamma.to(DEV), True)
    num_vd = out[0].shape[0] - out[1].shape[0] // 4
    dense_keys, sparse_keys = quad_keys(dense_out[1], num_vd), quad_keys(out[1], num_vd)
    assert dense_keys.unique().shape == dense_keys.shape and not torch.equal(dense_keys, sparse_keys)
    assert torch.equal(dense_keys.sort().values, sparse_keys.sort().values)
    sparse_cot = cot_v.clone()
    sparse_cot[num_vd:][sparse_keys.argsort()] = cot_v[num_vd:][dense_keys.argsort()]
    got, sparse_out = backward(hip_fn, sparse_inputs, sparse_cot, cot_l, torch.float32, cubes=cubes)
    assert torch.equal(sparse_out[0][:num_vd], dense_out[0][:num_vd]) and torch.equal(sparse_out[2], dense_out[2])
    assert_same_bits(got, dense, WEIGHTS, 'sparse ids')
    at = ids.to(DEV)
    mapped = dict(vertices=got['vertices'][at], sdf=got['sdf'][at])
    oracle.check_grads_local(mapped, only(want, ('vertices', 'sdf')), inputs, cot_v, cot_l, True, 'hip sparse ids')
    for n in ('vertices', 'sdf'):
        assert got[n].shape[0] == V
        off = got[n].clone()
        off[at] = 0
        assert not bool(off.any()), f'{n}: a gradient off the id map'


def test_non_contiguous_float_inputs():
    """Vertices and sdf as columns of one (V, 4) tensor, beta and alpha in transposed storage, gamma_f a step-2 slice."""
    inputs, cot_v, cot_l, want = setup('signs_8x8x5')
    v, s, c, res, beta, alpha, gamma = inputs
    dense, dense_out = backward(hip_fn, inputs, cot_v, cot_l, torch.float32)
    packed = torch.cat([v, s.unsqueeze(1)], 1).to(DEV)
    strided = dict(vertices=packed[:, :3], sdf=packed[:, 3], beta=beta.to(DEV).t().contiguous().t(),
                   alpha=alpha.to(DEV).t().contiguous().t(), gamma=torch.stack([gamma, -gamma], 1).to(DEV).reshape(-1)[::2])
    leaves = {n: t.detach().requires_grad_() for n, t in strided.items()}
    for n, t in leaves.items():
        assert not t.is_contiguous() and t.stride() == strided[n].stride(), n
    got, out = backward(hip_fn, inputs, cot_v, cot_l, torch.float32, leaves=leaves)
    for a, b in zip(out, dense_out):
        assert torch.equal(a, b)
    for n in FLOATS:
        assert got[n].shape == leaves[n].shape, n
    assert_same_bits(got, dense, WEIGHTS, 'non-contiguous')
    oracle.check_grads_local(got, want, inputs, cot_v, cot_l, True, 'hip non-contiguous')


def test_two_forwards_before_either_backward():
    """forward A, forward B (another size), backward A, backward B: each backward recomputes from its own saved state."""
    runs = {}
    for name in ('Q256', 'signs_8x8x5'):
        inputs, cot_v, cot_l, want = setup(name)
        alone = backward(hip_fn, inputs, cot_v, cot_l, torch.float32)[0]
        runs[name] = dict(inputs=inputs, cot_v=cot_v, cot_l=cot_l, want=want, alone=alone, leaves=leaves_of(inputs, torch.float32))
    for name, r in runs.items():
        lv = r['leaves']
        r['out'] = hip_fn(lv['vertices'], lv['sdf'], r['inputs'][2].to(DEV), r['inputs'][3], lv['beta'], lv['alpha'], lv['gamma'], True)
    for name, r in runs.items():
        ((r['out'][0] * r['cot_v'].to(DEV)).sum() + (r['out'][2] * r['cot_l'].to(DEV)).sum()).backward()
    for name, r in runs.items():
        got = {n: t.grad for n, t in r['leaves'].items()}
        assert_same_bits(got, r['alone'], WEIGHTS, f'interleaved {name}')
        oracle.check_grads_local(got, r['want'], r['inputs'], r['cot_v'], r['cot_l'], True, f'hip interleaved {name}')


def test_forward_and_backward_on_a_side_stream():
    inputs, cot_v, cot_l, want = setup('signs_8x8x5')
    alone, alone_out = backward(hip_fn, inputs, cot_v, cot_l, torch.float32)
    leaves = leaves_of(inputs, torch.float32)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        got, out = backward(hip_fn, inputs, cot_v, cot_l, torch.float32, leaves=leaves)
    torch.cuda.current_stream(DEV).wait_stream(side)
    side.synchronize()
    for a, b in zip(out, alone_out):
        assert torch.equal(a, b)
    assert_same_bits(got, alone, WEIGHTS, 'side stream')
    oracle.check_grads_local(got, want, inputs, cot_v, cot_l, True, 'hip side stream')


ID_WIDTH_GRID = ((4, 4, 4), 'signs', 341)                       # 125 vertices: below the smallest V


def id_width_grid():
    res, kind, seed = ID_WIDTH_GRID
    return cases.make_grid(res, seed, kind)


def id_width_setup():
    if 'id width' not in _SETUPS:
        dense_inputs = cases.relabel_for_id_width(id_width_grid(), 125)[0]
        cot_v, cot_l, want = reference(dense_inputs)
        dense = {t: hip_fn(*[x.to(DEV) if torch.is_tensor(x) else x for x in dense_inputs], t) for t in (False, True)}
        _SETUPS['id width'] = (dense_inputs, cot_v, cot_l, want, dense, backward(hip_fn, dense_inputs, cot_v, cot_l, torch.float32)[0])
    return _SETUPS['id width']


@pytest.mark.parametrize('V', [256, 257, 65536, 65537, 2 ** 24, 2 ** 24 + 1])
def test_id_width_of_the_pair_sort(V):
    """ss_passes_halves: 2 / 4 / 6 / 8 passes of the pair sort at ceil(log2 V) <= 8, 16, 24, 32.  The ids are mapped monotonely
    into [0, V), with 0 and V - 1 the ends of crossed edges that four cubes share (a quad's key has the lowest and the highest
    bits of a half set): every order is the dense call's, so the results are its bits."""
    dense_inputs, cot_v, cot_l, want, dense, dense_grads = id_width_setup()
    _, sparse_inputs, ids = cases.relabel_for_id_width(id_width_grid(), V)
    n = dense_inputs[0].shape[0]
    assert int(ids[0]) == 0 and int(ids[-1]) == V - 1 and bool((ids[1:] > ids[:-1]).all())
    for a, b in zip(sparse_inputs[4:7], dense_inputs[4:7]):
        assert torch.equal(a, b)
    with torch.no_grad():
        for training in (False, True):
            got = hip_fn(*[x.to(DEV) if torch.is_tensor(x) else x for x in sparse_inputs], training)
            for a, b in zip(got, dense[training]):
                assert torch.equal(a, b), f'V = {V}, training={training}'
    got, _ = backward(hip_fn, sparse_inputs, cot_v, cot_l, torch.float32)
    assert_same_bits(got, dense_grads, WEIGHTS, f'V = {V}')
    at = ids.to(DEV)
    mapped = dict(vertices=got['vertices'][at], sdf=got['sdf'][at])
    assert mapped['vertices'].shape[0] == n
    oracle.check_grads_local(mapped, only(want, ('vertices', 'sdf')), dense_inputs, cot_v, cot_l, True, f'hip V = {V}')
    for name in ('vertices', 'sdf'):
        got[name][at] = 0
        assert not bool(got[name].any()), f'{name}: a gradient off the id map'
