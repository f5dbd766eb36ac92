"""weighted_sum of dibr_rasterization's outputs differentiated straight into the rasterizer's inputs (GPU only).

metrics.render.weighted_sum(feat, G1, soft, G2) on the outputs of one dibr_rasterization call takes the fused backward: the
DIB-R backward kernels read G1 / G2 and scale them by the loss' gradient where they read a gradient
(kamd_dibr_weighted_sum_backward_*).  Every case is compared with the loss written in torch, (feat * G1).sum() +
(soft * G2).sum(), which materialises both gradients and runs the rasterizer's own backward: the gradient terms are the
same, only the order of the float atomics differs (same_sum_other_order, as the DIB-R backward tests compare).

That yardstick runs the same backward kernels in their plain instantiation, at D = 3 and on whole tiles: the comparison with the CPU
oracle, element by element, at every D the launchers switch on, on partial tiles, 1 / 8 / 9 / 17 views and with the hot-face table in
use and over its limit lives in tests/test_weighted_sum_dibr_oracle_gpu.py."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = {torch.float: 1e-5, torch.double: 1e-10}


def kal():
    import kaolin_amd
    return kaolin_amd


def same_sum_other_order(a, b, tol):
    a, b = a.double().cpu(), b.double().cpu()
    scale = max(float(b.abs().max()), 1e-30)
    return float((a - b).abs().max()) <= tol * scale


_SCENES = {}


def _scene(name, dtype, views=8):
    """Config C4's set-up for `name` ('sphere': the 50 000-triangle geodesic sphere; 'knot': the ~49k-triangle knot with
    image-sized faces), `views` cameras on the Fibonacci ring, D = 3 features.  -> (fz, fimg, feat, nz) on the GPU."""
    key = (name, dtype, views)
    if key not in _SCENES:
        from kaolin_amd.utils import testing as T
        v, f = T.scene_mesh(name, 50)
        fz, fimg, feats, nz = T.mesh_scene(v, f, num_views=views, dtype=dtype)
        _SCENES[key] = (fz.cuda(), fimg.cuda(), torch.cat(feats, -1).cuda(), nz.cuda())
    return _SCENES[key]


def _weights(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    B, H, W, D = shape
    return (torch.rand((B, H, W, D), generator=g, dtype=torch.float64).to(dtype).cuda(),
            torch.rand((B, H, W), generator=g, dtype=torch.float64).to(dtype).cuda())


def _render(scene, H, W, learn_feat):
    fz, fimg, feat, nz = scene
    a = fimg.clone().requires_grad_()
    f = feat.clone().requires_grad_(learn_feat)
    out, soft, face_idx = kal().render.mesh.dibr_rasterization(H, W, fz, a, f, nz)
    return a, f, out, soft, face_idx


def _grads(loss, a, f, scale=1.):
    (scale * loss).backward()
    return a.grad, f.grad


def _fused(out, G1, soft=None, G2=None):
    loss = kal().metrics.render.weighted_sum(out, G1, soft, G2)
    assert type(loss.grad_fn).__name__ == '_WeightedSumDibrBackward'
    return loss


def _check(got, want, dtype):
    for g, w in zip(got, want):
        assert (g is None) == (w is None)
        if w is not None:
            assert torch.isfinite(g).all()
            assert same_sum_other_order(g, w, TOL[dtype])
    assert float(want[0].abs().max()) > 0


@pytest.mark.parametrize('name', ['sphere', 'knot'])
@pytest.mark.parametrize('dtype', [torch.float, torch.double])
@pytest.mark.parametrize('learn_feat', [False, True])
def test_fused_backward_matches_the_torch_loss(name, dtype, learn_feat):
    H = W = 1024
    scene = _scene(name, dtype)
    G1, G2 = _weights((8, H, W, 3), dtype, 1)
    a, f, out, soft, _ = _render(scene, H, W, learn_feat)
    loss = _fused(out, G1, soft, G2)
    unfused = kal().metrics.render._WeightedSum2Cuda.apply(out, G1, soft, G2)
    assert torch.equal(loss, unfused)              # the same forward pass
    got = _grads(loss, a, f)
    a2, f2, out2, soft2, _ = _render(scene, H, W, learn_feat)
    want = _grads((out2 * G1).sum() + (soft2 * G2).sum(), a2, f2)
    _check(got, want, dtype)


@pytest.mark.parametrize('dtype', [torch.float, torch.double])
def test_image_only_loss_and_a_scaled_gradient(dtype):
    """No soft-mask term (w_soft_mask = NULL at the C ABI: the soft mask's launch is skipped), and (3 * loss).backward(): the
    incoming gradient is not 1."""
    H, W = 512, 448
    scene = _scene('knot', dtype, views=4)
    G1, _ = _weights((4, H, W, 3), dtype, 2)
    for learn_feat in (False, True):
        a, f, out, _, _ = _render(scene, H, W, learn_feat)
        got = _grads(_fused(out, G1), a, f, scale=3.)
        a2, f2, out2, _, _ = _render(scene, H, W, learn_feat)
        want = _grads((out2 * G1).sum(), a2, f2, scale=3.)
        _check(got, want, dtype)
    G1, G2 = _weights((4, H, W, 3), dtype, 3)
    a, f, out, soft, _ = _render(scene, H, W, True)
    got = _grads(_fused(out, G1, soft, G2), a, f, scale=-0.375)
    a2, f2, out2, soft2, _ = _render(scene, H, W, True)
    want = _grads((out2 * G1).sum() + (soft2 * G2).sum(), a2, f2, scale=-0.375)
    _check(got, want, dtype)


def test_outputs_with_another_consumer():
    """feat also feeds a second loss term: the DIB-R node's own backward runs for that term, the fused node's for the
    weighted sum, and both land in the same input gradients."""
    H = W = 512
    scene = _scene('sphere', torch.float, views=4)
    G1, G2 = _weights((4, H, W, 3), torch.float, 4)
    a, f, out, soft, _ = _render(scene, H, W, True)
    got = _grads(_fused(out, G1, soft, G2) + 0.5 * (out * out).sum() + soft.sum(), a, f)
    a2, f2, out2, soft2, _ = _render(scene, H, W, True)
    want = _grads((out2 * G1).sum() + (soft2 * G2).sum() + 0.5 * (out2 * out2).sum() + soft2.sum(), a2, f2)
    _check(got, want, torch.float)


@pytest.mark.parametrize('name', ['sphere', 'knot'])
def test_second_backward_through_a_retained_graph(name):
    """The first backward takes the gradient buffer the forward cleared, the second one starts from zeros; the soft
    backward's hot-face partial sums (the knot's big faces) are left cleared by the first pass."""
    H = W = 1024
    scene = _scene(name, torch.float)
    G1, G2 = _weights((8, H, W, 3), torch.float, 5)
    a, f, out, soft, _ = _render(scene, H, W, True)
    loss = _fused(out, G1, soft, G2)
    first = torch.autograd.grad(loss, [a, f], retain_graph=True)
    second = torch.autograd.grad(loss, [a, f])
    a2, f2, out2, soft2, _ = _render(scene, H, W, True)
    want = _grads((out2 * G1).sum() + (soft2 * G2).sum(), a2, f2)
    _check(first, want, torch.float)
    _check(second, want, torch.float)
    assert same_sum_other_order(second[0], first[0], 1e-5)


def test_non_finite_weights_at_background_pixels():
    """G1 holds inf / NaN where nothing is rendered: the loss is NaN in both spellings, and neither backward reads the
    weights there -- the gradient is finite and the torch spelling's."""
    H = W = 512
    scene = _scene('sphere', torch.float, views=4)
    G1, G2 = _weights((4, H, W, 3), torch.float, 6)
    a, f, out, soft, face_idx = _render(scene, H, W, False)
    bg = (face_idx < 0).unsqueeze(-1).expand_as(G1)
    pattern = torch.tensor([math.inf, math.nan, -math.inf], device='cuda').expand_as(G1)
    G1 = torch.where(bg, pattern, G1).contiguous()
    loss = _fused(out, G1, soft, G2)
    assert torch.isnan(loss)
    got = _grads(loss, a, f)
    a2, f2, out2, soft2, _ = _render(scene, H, W, False)
    want = _grads((out2 * G1).sum() + (soft2 * G2).sum(), a2, f2)
    _check(got, want, torch.float)


def test_output_modified_in_place_falls_back():
    H = W = 256
    scene = _scene('sphere', torch.float, views=2)
    G1, G2 = _weights((2, H, W, 3), torch.float, 7)
    a, f, out, soft, _ = _render(scene, H, W, True)
    with torch.no_grad():
        out[..., 0] *= 2.
    loss = kal().metrics.render.weighted_sum(out, G1, soft, G2)
    assert type(loss.grad_fn).__name__ == '_WeightedSum2CudaBackward'
    got = _grads(loss, a, f)
    a2, f2, out2, soft2, _ = _render(scene, H, W, True)
    with torch.no_grad():
        out2[..., 0] *= 2.
    want = _grads((out2 * G1).sum() + (soft2 * G2).sum(), a2, f2)
    _check(got, want, torch.float)
    assert torch.allclose(loss, (out2 * G1).sum() + (soft2 * G2).sum(), rtol=1e-5)


def test_other_operands_take_the_unfused_path(monkeypatch):
    H = W = 128
    scene = _scene('sphere', torch.float, views=2)
    G1, G2 = _weights((2, H, W, 3), torch.float, 8)
    ws = kal().metrics.render.weighted_sum
    _, _, out, soft, _ = _render(scene, H, W, False)
    _, _, out_b, soft_b, _ = _render(scene, H, W, False)
    name = lambda t: type(t.grad_fn).__name__  # noqa: E731
    assert name(ws(out, G1, soft, G2)) == '_WeightedSumDibrBackward'
    assert name(ws(out, G1, soft_b, G2)) == '_WeightedSum2CudaBackward'          # two different nodes
    assert name(ws(out * 1., G1, soft, G2)) == '_WeightedSum2CudaBackward'       # not the node's output
    assert name(ws(out, G1.double(), soft, G2)) != '_WeightedSumDibrBackward'    # another dtype
    assert name(ws(out, G1.transpose(1, 2).contiguous().transpose(1, 2), soft, G2)) == '_WeightedSum2CudaBackward'
    monkeypatch.setenv('KAMD_WS_FUSED_BWD', '2')
    assert name(ws(out, G1, soft, G2)) == '_WeightedSum2CudaBackward'


def test_step_graph_capture_and_replay():
    """bench.py's step shape -- prepare_vertices, dibr_rasterization, the fused weighted sum, backward to the shared vertices --
    captured once and replayed: the same vertex gradient as the eager step."""
    from kaolin_amd.utils import testing as T
    V, H, W = 4, 384, 384
    verts, faces = T.geodesic_sphere(20)
    verts = verts.float().cuda().requires_grad_()
    faces = faces.cuda()
    cams = T.fibonacci_cameras(V, 2.5).cuda()
    rot, trans = kal().render.camera.generate_rotate_translate_matrices(
        cams, torch.zeros((V, 3), device='cuda'), torch.tensor([[0., 1., 0.]], device='cuda').repeat(V, 1))
    proj = kal().render.camera.generate_perspective_projection(math.pi / 4).cuda()
    F = faces.shape[0]
    feats = torch.rand((V, F, 3, 3), generator=torch.Generator().manual_seed(9)).cuda()
    G1, G2 = _weights((V, H, W, 3), torch.float, 10)
    out = {}

    def step():
        fv_cam, fv_img, normals = kal().render.mesh.prepare_vertices(
            verts.unsqueeze(0).expand(V, -1, -1), faces, proj, camera_rot=rot, camera_trans=trans)
        feat, soft, _ = kal().render.mesh.dibr_rasterization(H, W, fv_cam[..., 2], fv_img, feats, normals[..., 2])
        loss = kal().metrics.render.weighted_sum(feat, G1, soft, G2)
        assert type(loss.grad_fn).__name__ == '_WeightedSumDibrBackward'
        (g,) = torch.autograd.grad(loss, [verts])
        if 'g' in out:
            out['g'].copy_(g)
        else:
            out['g'] = g.detach().clone()
    step()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for scale in (1.0, 0.9):
        with torch.no_grad():
            G1.mul_(scale)
        graph.replay()
        got = out['g'].clone()
        step()
        assert float(out['g'].abs().max()) > 0
        assert same_sum_other_order(got, out['g'], 1e-5)
