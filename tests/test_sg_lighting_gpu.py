"""kaolin_amd.render.lighting on the MI355X: the reduced SG inner product's HIP kernels (csrc/sg_lighting.hip), forward and
all six gradients, against a float64 oracle (tests/sg_oracle.py) and the reference's golden results; gradcheck through the
kernels; determinism; a DIB-R render lit end to end; the ``_C.render.sg`` shim; graph capture."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
from sg_oracle import reduced_oracle
from kaolin_amd.render import lighting
from kaolin_amd.render.lighting import sg as sgm
from kaolin_amd.utils.testing import elementwise_mismatch

pytestmark = pytest.mark.gpu

TOL = {torch.float32: 1e-5, torch.float64: 1e-10}
NAMES = ('ga', 'gd', 'gs', 'goa', 'god', 'gos')


def _check(a, b, dtype, term_abs_sum=None, what=''):
    msg = elementwise_mismatch(a, b, tol=TOL[dtype], term_abs_sum=term_abs_sum)
    assert msg is None, f'{what}: {msg}'


def _rand_inputs(n, m, dtype, seed=0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    shapes = ((n, 3), (n, 3), (n,), (m, 3), (m, 3), (m,))
    return [torch.rand(s, generator=g, dtype=dtype, device='cuda') for s in shapes], \
        torch.rand((n, 3), generator=g, dtype=dtype, device='cuda')


def _hip_forward_backward(args, go):
    args = [t.detach().clone().requires_grad_() for t in args]
    out = sgm.unbatched_reduced_sg_inner_product(*args)
    grads = torch.autograd.grad(out, args, go)
    return out, grads


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('num_other', [0, 1, 7, 8, 17, 64, 65, 511])
@pytest.mark.parametrize('num_sg', [0, 1, 17, 63, 64, 65, 511, 10000])
def test_reduced_vs_fp64_oracle(num_sg, num_other, dtype):
    args, go = _rand_inputs(num_sg, num_other, dtype, seed=num_sg * 1000 + num_other)
    out, grads = _hip_forward_backward(args, go)
    ref = reduced_oracle(*args, grad_out=go)
    _check(out, ref['out'], dtype, ref['out_abs'], 'out')
    for name, g in zip(NAMES, grads):
        assert g.shape == ref[name].shape and g.dtype == dtype
        _check(g, ref[name], dtype, ref[name + '_abs'], name)


@pytest.fixture(scope='module')
def gold():
    z = np.load(os.path.join(GOLDEN_DIR, 'sg_lighting.npz'))
    return {k: torch.from_numpy(z[k]) for k in z.files}


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('case', ['1_1', '17_7', '33_8', '64_17', '65_64', '100_65', '23_511', '7_1'])
def test_reduced_vs_golden(gold, case, dtype):
    tag = f'red_{case}'
    cpu = [gold[f'{tag}_{k}'] for k in ('a', 'd', 's', 'oa', 'od', 'os')]
    out, grads = _hip_forward_backward([t.to('cuda', dtype) for t in cpu], gold[f'{tag}_go'].to('cuda', dtype))
    ref = reduced_oracle(*cpu, grad_out=gold[f'{tag}_go'])
    _check(out, gold[f'{tag}_out'], dtype, gold[f'{tag}_out_abs'], 'out')
    for name, g in zip(NAMES, grads):
        _check(g, gold[f'{tag}_{name}'], dtype, ref[name + '_abs'], name)


def test_gradcheck_reduced_f64():
    args, _ = _rand_inputs(33, 17, torch.float64, seed=5)
    args = [t.requires_grad_() for t in args]
    assert torch.autograd.gradcheck(sgm.unbatched_reduced_sg_inner_product, args, eps=1e-6, atol=1e-7, rtol=1e-6)


def test_gradcheck_diffuse_constant_lobe_f64():
    g = torch.Generator(device='cuda').manual_seed(6)
    n = torch.nn.functional.normalize(torch.randn(40, 3, generator=g, dtype=torch.float64, device='cuda'), dim=1)
    la = torch.rand(9, 3, generator=g, dtype=torch.float64, device='cuda') + 0.1
    ld = torch.nn.functional.normalize(torch.randn(9, 3, generator=g, dtype=torch.float64, device='cuda'), dim=1)
    ls = torch.rand(9, generator=g, dtype=torch.float64, device='cuda') * 4 + 0.5
    albedo = torch.rand(40, 3, generator=g, dtype=torch.float64, device='cuda')
    inputs = [t.requires_grad_() for t in (la, ld, ls, n)]
    assert torch.autograd.gradcheck(lambda a, d, s, nn: lighting.sg_diffuse_inner_product(a, d, s, nn, albedo), inputs,
                                    eps=1e-6, atol=1e-7, rtol=1e-6)


def test_backward_is_deterministic():
    args, go = _rand_inputs(1 << 20, 32, torch.float32, seed=7)
    _, g1 = _hip_forward_backward(args, go)
    _, g2 = _hip_forward_backward(args, go)
    for name, a, b in zip(NAMES, g1, g2):
        assert torch.equal(a, b), name


def test_large_8x1024x1024_rows_32_lights():
    n, m = 8 * 1024 * 1024, 32
    args, go = _rand_inputs(n, m, torch.float32, seed=8)
    out, grads = _hip_forward_backward(args, go)
    rows = torch.randperm(n, device='cuda')[:65536].sort().values
    ref = reduced_oracle(*args, grad_out=go, pairs_per_chunk=1 << 22, rows=rows)
    _check(out[rows], ref['out'], torch.float32, ref['out_abs'], 'out')
    for name, g in zip(NAMES[:3], grads[:3]):
        _check(g[rows], ref[name], torch.float32, ref[name + '_abs'], name)
    for name, g in zip(NAMES[3:], grads[3:]):
        _check(g, ref[name], torch.float32, ref[name + '_abs'], name)


def _shading_inputs(n, m, dtype, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    normal = torch.nn.functional.normalize(torch.randn(n, 3, generator=g, dtype=dtype, device='cuda'), dim=1)
    la = torch.rand(m, 3, generator=g, dtype=dtype, device='cuda') * 2
    ld = torch.nn.functional.normalize(torch.randn(m, 3, generator=g, dtype=dtype, device='cuda'), dim=1)
    ls = torch.rand(m, generator=g, dtype=dtype, device='cuda') * 8 + 0.5
    view = torch.nn.functional.normalize(normal + 0.5 * torch.nn.functional.normalize(
        torch.randn(n, 3, generator=g, dtype=dtype, device='cuda'), dim=1), dim=1)
    rough = torch.rand(n, generator=g, dtype=dtype, device='cuda') * 0.6 + 0.3
    albedo = torch.rand(n, 3, generator=g, dtype=dtype, device='cuda')
    spec = torch.rand(n, 3, generator=g, dtype=dtype, device='cuda')
    return dict(normal=normal, la=la, ld=ld, ls=ls, view=view, rough=rough, albedo=albedo, spec=spec)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_public_functions_gpu_vs_cpu_f64(dtype):
    x = _shading_inputs(3000, 24, dtype, seed=9)
    gout = torch.rand(3000, 3, dtype=dtype, device='cuda')
    cases = {
        'irradiance': (lambda d: lighting.sg_irradiance_inner_product(d['la'], d['ld'], d['ls'], d['normal']),
                       ('la', 'ld', 'ls', 'normal')),
        'diffuse': (lambda d: lighting.sg_diffuse_inner_product(d['la'], d['ld'], d['ls'], d['normal'], d['albedo']),
                    ('la', 'ld', 'ls', 'normal', 'albedo')),
        'specular': (lambda d: lighting.sg_warp_specular_term(d['la'], d['ld'], d['ls'], d['normal'], d['rough'],
                                                              d['view'], d['spec']),
                     ('la', 'ld', 'ls', 'normal', 'rough', 'view', 'spec')),
    }
    for what, (fn, diff) in cases.items():
        dev = {k: v.clone().requires_grad_(k in diff) for k, v in x.items()}
        ref = {k: v.detach().cpu().double().requires_grad_(k in diff) for k, v in x.items()}
        out = fn(dev)
        out_ref = fn(ref)
        g_dev = torch.autograd.grad(out, [dev[k] for k in diff], gout)
        g_ref = torch.autograd.grad(out_ref, [ref[k] for k in diff], gout.cpu().double())
        # accumulation slack: every row sums 24 lights and every light gradient 3000 rows, each term at most the largest
        # element in magnitude -- a looser bound than the per-term sums of the reduced-op tests above (which pin the
        # kernels' arithmetic); here the composition around the kernels is what is checked
        _check(out, out_ref, dtype, out_ref.abs().max() * torch.ones_like(out_ref) * 24, what)
        for k, a, b in zip(diff, g_dev, g_ref):
            count = 3000 if k in ('la', 'ld', 'ls') else 24
            _check(a, b, dtype, b.abs().max() * torch.ones_like(b) * count, f'{what} d/d{k}')


def test_constant_lobe_matches_general_kernel():
    x = _shading_inputs(70000, 32, torch.float32, seed=10)
    gout = torch.rand(70000, 3, device='cuda')
    n1 = x['normal'].clone().requires_grad_()
    l1 = [x[k].clone().requires_grad_() for k in ('la', 'ld', 'ls')]
    out1 = lighting.sg_irradiance_inner_product(*l1, n1)
    g1 = torch.autograd.grad(out1, [n1] + l1, gout)
    n2 = x['normal'].clone().requires_grad_()
    l2 = [x[k].clone().requires_grad_() for k in ('la', 'ld', 'ls')]
    a, d, s = sgm.cosine_lobe_sg(n2)
    out2 = torch.clamp(sgm.unbatched_reduced_sg_inner_product(a, d, s, *l2), min=0.)
    g2 = torch.autograd.grad(out2, [n2] + l2, gout)
    _check(out1, out2, torch.float32, what='out')
    for name, p, q in zip(('normal', 'la', 'ld', 'ls'), g1, g2):
        _check(p, q, torch.float32, what=name)


def test_end_to_end_dibr_diffuse_lighting():
    from kaolin_amd.utils import testing as T
    import kaolin_amd as kal
    verts, faces = T.geodesic_sphere(16)
    verts = verts.float().cuda().requires_grad_()
    faces = faces.cuda()
    cams = T.fibonacci_cameras(2).cuda()
    g = torch.Generator(device='cuda').manual_seed(11)
    la = (torch.rand(16, 3, generator=g, device='cuda') * 2).requires_grad_()
    ld = torch.nn.functional.normalize(torch.randn(16, 3, generator=g, device='cuda'), dim=1).requires_grad_()
    ls = (torch.rand(16, generator=g, device='cuda') * 6 + 1).requires_grad_()
    w = torch.rand(2, 256, 256, 3, generator=g, device='cuda')

    def step(light):
        fz, fimg, nz = T.project_mesh(verts, faces, cams)
        vn = torch.nn.functional.normalize(verts, dim=1)
        feat = vn[faces].unsqueeze(0).expand(2, -1, -1, -1)
        (img,), mask, face_idx = kal.render.mesh.dibr_rasterization(256, 256, fz, fimg, [feat], nz)
        hard = face_idx >= 0
        n = torch.nn.functional.normalize(img[hard], dim=1)
        albedo = torch.full_like(n, 0.7)
        rgb = light(n, albedo)
        loss = (rgb * w[hard]).sum() + mask.sum() * 1e-3
        return loss, torch.autograd.grad(loss, [la, ld, ls, verts]), n.detach(), (w[hard] * 0.7 / math.pi)

    def oracle(n, albedo):
        lobe = sgm.cosine_lobe_sg(n.double())
        irr = sgm.unbatched_sg_inner_product(*lobe, la.double(), ld.double(), ls.double()).sum(1)
        return (torch.clamp(irr, min=0.) * albedo.double() / math.pi).float()

    loss, grads, n, _ = step(lambda n, a: lighting.sg_diffuse_inner_product(la, ld, ls, n, a))
    loss_ref, grads_ref, n_ref, gout = step(oracle)
    assert n.shape[0] > 10000 and torch.equal(n, n_ref)      # the same pixels and normals on both sides
    assert abs(float(loss) - float(loss_ref)) <= 1e-5 * abs(float(loss_ref))
    # light gradients: sums over the covered pixels, each with its terms' absolute sum from the pairwise oracle
    terms = reduced_oracle(*sgm.cosine_lobe_sg(n_ref), la, ld, ls, grad_out=gout)
    for name, a, b, k in zip(('amplitude', 'direction', 'sharpness'), grads[:3], grads_ref[:3], ('goa', 'god', 'gos')):
        msg = elementwise_mismatch(a, b, tol=1e-5, term_abs_sum=terms[k + '_abs'])
        assert msg is None, f'{name}: {msg}'
    # vertex gradient: both sides run the same f32 rasterizer backward, whose float-atomic pixel accumulation makes the
    # last bits of every vertex's sum order-dependent; the lighting's own difference is checked above at 1e-5, so the
    # vertex gradient is compared at 1e-4 of its largest element (a sum over up to thousands of pixels per vertex)
    gv, gv_ref = grads[3], grads_ref[3]
    assert torch.isfinite(gv).all()
    assert float((gv - gv_ref).abs().max()) <= 1e-4 * float(gv_ref.abs().max())


# ---- the _C.render.sg shim -------------------------------------------------------------------------------------------

def test_shim_names_and_argument_order():
    import kaolin_amd
    shim = kaolin_amd._C.render.sg
    args, go = _rand_inputs(100, 9, torch.float32, seed=12)
    out = shim.unbatched_reduced_sg_inner_product_forward_cuda(*args)
    ref = reduced_oracle(*args, grad_out=go)
    _check(out, ref['out'], torch.float32, ref['out_abs'])
    grads = shim.unbatched_reduced_sg_inner_product_backward_cuda(go, *args)
    assert isinstance(grads, list) and len(grads) == 6
    for name, g in zip(NAMES, grads):
        _check(g, ref[name], torch.float32, ref[name + '_abs'], name)
    kaolin = kaolin_amd.install_as_kaolin()
    assert kaolin._C.render.sg is shim and kaolin.render.lighting is lighting


def test_shim_errors():
    from kaolin_amd._C.render import sg as shim
    fwd = shim.unbatched_reduced_sg_inner_product_forward_cuda
    bwd = shim.unbatched_reduced_sg_inner_product_backward_cuda
    args, go = _rand_inputs(10, 4, torch.float32, seed=13)
    cpu = list(args)
    cpu[3] = cpu[3].cpu()
    with pytest.raises(RuntimeError, match="argument #4 'other_intensity' is on CPU"):
        fwd(*cpu)
    with pytest.raises(RuntimeError, match="argument #1 'grad_out' is on CPU"):
        bwd(go.cpu(), *args)
    nc = list(args)
    nc[1] = torch.rand(3, 10, device='cuda').t()
    with pytest.raises(RuntimeError, match="non-contiguous tensor for argument #2 'direction'"):
        fwd(*nc)
    mixed = list(args)
    mixed[5] = mixed[5].double()
    with pytest.raises(RuntimeError, match="same type as tensor for argument #6 'other_sharpness'"):
        fwd(*mixed)
    with pytest.raises(RuntimeError, match="same type"):
        bwd(go.double(), *args)
    wrong = list(args)
    wrong[2] = torch.rand(11, device='cuda')
    with pytest.raises(RuntimeError, match=r"Expected tensor of size \[10\].*argument #3 'sharpness'"):
        fwd(*wrong)
    wrong = list(args)
    wrong[4] = torch.rand(5, 3, device='cuda')
    with pytest.raises(RuntimeError, match=r"size \[4, 3\].*argument #5 'other_direction'"):
        fwd(*wrong)
    with pytest.raises(RuntimeError, match=r"size \[10, 3\].*argument #1 'grad_out'"):
        bwd(torch.rand(9, 3, device='cuda'), *args)
    with pytest.raises(RuntimeError, match='not implemented for'):
        fwd(*[t.half() for t in args])


def test_graph_capture_replays_bitwise():
    """Forward + backward of sg_diffuse_inner_product captured on one stream and replayed equals the eager result bitwise.
    The eager reference runs on its own leaf tensors: an autograd step on the default stream would bind the captured
    leaves' AccumulateGrad nodes to the default stream, which torch warns breaks capture."""
    x = _shading_inputs(200000, 32, torch.float32, seed=14)
    albedo, w = x['albedo'], torch.rand(200000, 3, device='cuda')

    def leaves():
        return [x[k].clone().requires_grad_() for k in ('normal', 'la', 'ld', 'ls')]

    def make_step(params, out):
        def step():
            n, la, ld, ls = params
            rgb = lighting.sg_diffuse_inner_product(la, ld, ls, n, albedo)
            grads = torch.autograd.grad((rgb * w).sum(), params)
            for k, v in zip(('rgb', 'gn', 'ga', 'gd', 'gs'), (rgb,) + grads):
                if k in out:
                    out[k].copy_(v)
                else:
                    out[k] = v.detach().clone()
        return step

    eager = {}
    make_step(leaves(), eager)()
    out = {}
    step = make_step(leaves(), out)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for k in out:
        out[k].zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in out:
        assert torch.equal(out[k], eager[k]), k
