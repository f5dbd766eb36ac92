"""prepare_vertices, texture_mapping and mask_iou against the reference (VERDICT row f2), in two layers.

CPU (unmarked): the package's torch chains (``_prepare_vertices_torch``, ``_texture_mapping_torch``, ``_mask_iou_torch``)
reproduce tests/golden/render_helpers.npz -- made by tests/golden/make_golden_render_helpers.py from the reference's
render/mesh/utils.py and metrics/render.py in float64 -- within |x - golden| <= 1e-12 |golden| + 1e-13 max|golden| (the same ops
on the same device: rounding noise); `nearest` outputs bit-equal; a golden gradient of exactly 0 is exactly 0.  That makes the
chains the reference's definition on any input.

GPU (``-m gpu``): the public API, which must take the fused HIP path (the result's grad_fn is the ``_...Cuda`` node), against
the pinned chain run on the CPU in float64 (``ref64``), with the chain's own float32 error E32 = max |ref32 - ref64| per tensor
as the absolute floor, for every element of every output and gradient:
    float32   |x - ref64| <= 1e-5  |ref64| + 4    E32
    float64   |x - ref64| <= 1e-10 |ref64| + 1e-6 E32
(tests/render_helper_cases.py: the cases, ``reference`` and ``mismatch``).  Where E32 == 0 the bound is purely relative: the
`nearest` outputs (bit-equal in both dtypes) and uv gradient; gradients of vertices without a face and normals of
degenerate faces are checked to be exactly 0 besides.  ``test_floors_cannot_hide_a_failure`` keeps the floor honest on the CPU.

Worst measured |x - ref64| / bound on an MI355X over the kernel set (each test prints its own; the bound is 1):
    operator            float32   float64
    prepare_vertices    0.26      0.096     (gv of b13_f20/tf/batched; gv of repeat/rt/batched)
    texture_mapping     0.29      1.1e-4    (g_tex of t4x6_c3_dense_b3 bilinear; g_tex of t2x2_c5_n257 bilinear: atomic sums)
    mask_iou            0.0093    3.9e-4    (g_rhs of views; g_rhs of s2x127x129)
"""
import pytest
import torch

import render_helper_cases as rc

F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F32, id='f32'), pytest.param(F64, id='f64')]


@pytest.fixture(scope='module')
def fx():
    return rc.load_fixture()


# ---- CPU: the chains are the reference --------------------------------------------------------------------------------

def _pinned(got, golden, exact=False):
    assert got.dtype == golden.dtype == F64 and got.shape == golden.shape
    if exact or golden.numel() == 0:
        assert torch.equal(got, golden)
        return
    bound = 1e-12 * golden.abs() + 1e-13 * float(golden.abs().max())
    assert bool(((got - golden).abs() <= bound).all()), float(((got - golden).abs() - bound).max())
    assert bool((got[golden == 0] == 0).all())                       # what the reference leaves at exactly 0 stays exactly 0


def _check_inputs(fx, prefix, case, names):
    for k in names:
        stored = fx[f'{prefix}__{case["name"]}__in_{k}']
        assert torch.equal(stored if stored.dtype == torch.long else stored.double(), case[k]), (case['name'], k)


def _ids(entries):
    return ['-'.join('+'.join(p) if isinstance(p, tuple) else p for p in e) for e in entries]


@pytest.mark.parametrize('entry', rc.PV_PINNED, ids=_ids(rc.PV_PINNED))
def test_prepare_vertices_chain_is_the_reference(fx, entry):
    name, camera, layout, which = entry
    case = rc.pv_cases()[name]
    _check_inputs(fx, 'pv', case, rc.PV_INPUTS)
    ref64 = rc.pv_reference(*entry)[0]
    for k in rc.PV_TENSORS:
        _pinned(ref64[k], fx[f'{rc.pv_tag(*entry)}__{k}'])
    for f in rc.PV_ZERO_NORMALS.get(name, ()):
        assert bool((ref64['nrm'][:, f] == 0).all())


@pytest.mark.parametrize('entry', rc.TM_PINNED, ids=_ids(rc.TM_PINNED))
def test_texture_mapping_chain_is_the_reference(fx, entry):
    name, mode, need = entry
    _check_inputs(fx, 'tm', rc.tm_cases()[name], rc.TM_INPUTS)
    ref64 = rc.tm_reference(*entry)[0]
    assert set(ref64) == {'out'} | {'g_' + n for n in need}
    for k in ref64:
        _pinned(ref64[k], fx[f'{rc.tm_tag(*entry)}__{k}'], exact=(mode == 'nearest' and k in ('out', 'g_uv')))


@pytest.mark.parametrize('entry', rc.MI_PINNED, ids=_ids(rc.MI_PINNED))
def test_mask_iou_chain_is_the_reference(fx, entry):
    name, need = entry
    _check_inputs(fx, 'mi', rc.mi_cases()[name], rc.MI_INPUTS)
    ref64 = rc.mi_reference(*entry)[0]
    assert set(ref64) == {'loss'} | {'g_' + n for n in need}
    for k in ref64:
        _pinned(ref64[k], fx[f'{rc.mi_tag(*entry)}__{k}'])


def test_fixture_holds_exactly_the_pinning_sets(fx):
    tags = {rc.pv_tag(*e) for e in rc.PV_PINNED} | {rc.tm_tag(*e) for e in rc.TM_PINNED} | {rc.mi_tag(*e) for e in rc.MI_PINNED}
    assert {k.rsplit('__', 1)[0] for k in fx if '__in_' not in k} == tags


def test_floors_cannot_hide_a_failure():
    """The absolute floor of the GPU bound is the chain's float32 error E32 of the tensor at hand.  For every well-conditioned
    case of the kernel set it is at most 1e-5 of the tensor's largest entry; the ill-conditioned inputs sit in cases of their own
    of at most 16 faces (24 texture samples), so they cannot raise the floor of a large case."""
    def check(case, triples):
        for ref64, _, e32 in triples:
            for k, e in e32.items():
                if case['conditioned']:
                    assert e <= rc.CONDITIONED_E32 * float(ref64[k].abs().max()) if ref64[k].numel() else e == 0., (case['name'], k, e)
    for name in rc.PV_KERNEL_SET:
        case = rc.pv_cases()[name]
        assert case['conditioned'] or case['faces'].shape[0] <= rc.ILL_MAX_FACES
        check(case, [rc.pv_reference(name, cam, lay) for cam in rc.PV_CAMERAS for lay in rc.PV_LAYOUTS + ('strided',)])
    for name in rc.TM_KERNEL_SET:
        case = rc.tm_cases()[name]
        assert case['conditioned'] or case['uv'][0].numel() // 2 <= 24
        check(case, [rc.tm_reference(name, mode) for mode in rc.TM_MODES])
        for k in ('out', 'g_uv'):                                      # `nearest`: a copy of a texel, no uv gradient
            assert rc.tm_reference(name, 'nearest')[2][k] == 0.
    for name in rc.MI_KERNEL_SET:
        check(rc.mi_cases()[name], [rc.mi_reference(name)])


# ---- GPU: the kernels against the pinned chains -----------------------------------------------------------------------

def _compare(op, dtype, label, got, triple, names):
    ref64, _, e32 = triple
    problems = []
    for k in names:
        if k not in ref64:
            assert got[k] is None, f'{k}: a gradient nobody asked for'
            continue
        assert got[k] is not None and got[k].dtype == dtype and got[k].is_cuda, k
        worst, msg = rc.mismatch(got[k], ref64[k], e32[k], dtype)
        print(f'RATIO {op} {"f32" if dtype == F32 else "f64"} {label} {k} {worst:.4g} (E32 {e32[k]:.3e})')
        if msg is not None:
            problems.append(f'{k}: {msg}')
    assert not problems, '\n'.join(problems)


def _pv_api():
    import kaolin_amd as kal
    from kaolin_amd.render.mesh.utils import _PrepareVerticesCuda
    return kal.render.mesh.prepare_vertices, _PrepareVerticesCuda._backward_cls


def _pv_check(name, camera, layout, dtype, which=rc.PV_WHICH[0]):
    fn, node = _pv_api()
    case = rc.pv_cases()[name]
    got = rc.pv_run(fn, case, camera, layout, dtype, 'cuda', which=which)
    assert isinstance(got['node'], node), 'prepare_vertices did not take the fused path'
    _compare('prepare_vertices', dtype, f'{name}/{camera}/{layout}/{"+".join(which)}', got,
             rc.pv_reference(name, camera, layout, which), rc.PV_TENSORS)
    gv = got['gv'][..., :3]
    assert bool((gv[:, rc.unreferenced_vertices(case)] == 0).all())          # no face, no gradient: exactly
    for f in rc.PV_ZERO_NORMALS.get(name, ()):
        assert bool((got['nrm'][:, f] == 0).all())
    assert bool(torch.isfinite(got['gv']).all())
    if layout == 'strided':
        assert bool((got['gv'][..., 3] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('layout', rc.PV_LAYOUTS)
@pytest.mark.parametrize('camera', rc.PV_CAMERAS)
@pytest.mark.parametrize('name', rc.PV_KERNEL_SET)
def test_prepare_vertices_kernels(name, camera, layout, dtype):
    _pv_check(name, camera, layout, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('camera', rc.PV_CAMERAS)
@pytest.mark.parametrize('which', rc.PV_WHICH[1:], ids=lambda w: w[0])
@pytest.mark.parametrize('name', ['b3_f43', 'fan', 'repeat', 'collinear'])
def test_prepare_vertices_one_upstream_gradient(name, which, camera, dtype):
    """each output alone: the other two gradients reach the backward kernel as null pointers"""
    _pv_check(name, camera, 'batched', dtype, which)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('camera', rc.PV_CAMERAS)
def test_prepare_vertices_strided_vertices(camera, dtype):
    """(B, V, 4)[..., :3]: the gradient arrives in the base tensor, its fourth column untouched"""
    _pv_check('b3_f43', camera, 'strided', dtype)


class _DropGradient(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return None


@pytest.mark.gpu
def test_prepare_vertices_without_upstream_gradient():
    """every output's gradient undefined: the node is run, launches nothing and hands back None"""
    fn, node = _pv_api()
    case = rc.pv_cases()['b3_f21']
    leaf, verts = rc.pv_vertices(case, 'batched', F32, 'cuda')
    out = fn(verts, case['faces'].cuda(), case['proj'].float().cuda(), camera_rot=case['rot'].float().cuda(),
             camera_trans=case['trans'].float().cuda())
    assert isinstance(out[1].grad_fn, node)
    _DropGradient.apply(out[1]).sum().backward()
    assert leaf.grad is None


def _tm_check(name, mode, dtype, need=rc.TM_NEED[0]):
    from kaolin_amd.render.mesh.utils import texture_mapping, _TextureMappingCuda
    case = rc.tm_cases()[name]
    got = rc.tm_run(texture_mapping, case, mode, dtype, 'cuda', need=need)
    node = got['node']           # (the public function reshapes the node's (B, N, C) output to the coordinates' layout: a view)
    while node is not None and ('View' in type(node).__name__ or 'Reshape' in type(node).__name__):
        node = node.next_functions[0][0]
    assert isinstance(node, _TextureMappingCuda._backward_cls), 'texture_mapping did not take the fused path'
    assert got['out'].shape == tuple(case['uv'].shape[:-1]) + (case['tex'].shape[1],)
    triple = rc.tm_reference(name, mode, need)
    _compare('texture_mapping', dtype, f'{name}/{mode}/{"+".join(need)}', got, triple, rc.TM_TENSORS)
    if mode == 'nearest':
        assert torch.equal(got['out'].cpu().double(), triple[0]['out'])      # a copy of a texel: bit-equal in both dtypes
        if 'uv' in need:
            assert bool((got['g_uv'] == 0).all())


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('mode', rc.TM_MODES)
@pytest.mark.parametrize('name', rc.TM_KERNEL_SET)
def test_texture_mapping_kernels(name, mode, dtype):
    _tm_check(name, mode, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('need', rc.TM_NEED[1:], ids=lambda n: n[0])
@pytest.mark.parametrize('mode', rc.TM_MODES)
@pytest.mark.parametrize('name', ['t4x6_c3_dense_b3', 't2x2_c5_n257'])
def test_texture_mapping_one_gradient(name, mode, need, dtype):
    """the texture's gradient alone, the coordinates' alone: the other one is a null pointer in the backward kernel"""
    _tm_check(name, mode, dtype, need)


def _mi_check(name, dtype, need=rc.MI_NEED[0]):
    from kaolin_amd.metrics.render import mask_iou, _MaskIoUCuda
    got = rc.mi_run(mask_iou, rc.mi_cases()[name], dtype, 'cuda', need=need)
    assert isinstance(got['node'], _MaskIoUCuda._backward_cls), 'mask_iou did not take the fused path'
    assert got['loss'].shape == ()
    _compare('mask_iou', dtype, f'{name}/{"+".join(need)}', got, rc.mi_reference(name, need), rc.MI_TENSORS)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', rc.MI_KERNEL_SET)
def test_mask_iou_kernels(name, dtype):
    _mi_check(name, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('need', rc.MI_NEED[1:], ids=lambda n: n[0])
@pytest.mark.parametrize('name', ['kinds', 's5x33x31'])
def test_mask_iou_one_gradient(name, need, dtype):
    _mi_check(name, dtype, need)
