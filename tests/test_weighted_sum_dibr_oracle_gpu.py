"""The fused weighted_sum backward (_WeightedSumDibr -> kamd_dibr_weighted_sum_backward_*) against the CPU ORACLE, element by element.

tests/test_weighted_sum_dibr.py compares the fused path with the torch spelling of the loss, which runs the same backward kernels in
their plain instantiation, under a bound scaled by the gradient's largest element.  Here the yardstick is oracle.rasterize_backward +
oracle.dibr_soft_mask_backward on the gradient g = scale * G the kernels form on the fly (one rounded product, formed here in the
tensor's dtype), the bound is the element-wise rel_close of the DIB-R suite (1e-5 float32 / 1e-9 float64, tests/dibr_fuzz_cases.py),
and the cases (tests/weighted_sum_dibr_cases.py; tests/test_weighted_sum_dibr_cases_cpu.py asserts what each one reaches) are
the ones the launchers branch on: every D of their switch (1 - 4, and 5 and 7 for the generic branch), with and without a feature
gradient, both dtypes, partial tiles, a batch of 1, 8 / 9 / 17 views, the hot-face table in use and over its limit.

The soft mask's backward is evaluated on the GPU forward's own mask and K-buffers (_soft_backward_on_the_gpu_forwards_outputs in
tests/test_dibr_gpu.py says why).  ragged / tiny / views meet plain rel_close, as the unfused path does on the same sphere scenes in
test_dibr_rasterization_vs_oracle; the hot cases get the accumulation slack 64 eps sum|terms| of the floor and stacked-faces tests
(faces that collect tens of thousands of float-atomic terms of both signs) and print how many elements needed it."""
import pytest
import torch

import oracle
import weighted_sum_dibr_cases as C
from test_dibr_gpu import _soft_backward_on_the_gpu_forwards_outputs, rel_close

pytestmark = pytest.mark.gpu

DTYPES = [torch.float, torch.double]
TOL = {torch.float: 1e-5, torch.double: 1e-9}


def kal():
    import kaolin_amd
    return kaolin_amd


_CASES = {}


def _case(family, key, dtype):
    """-> (case, oracle.dibr_rasterization of it), built once per module run and never modified."""
    k = (family, key, dtype)
    if k not in _CASES:
        case = getattr(C, family)(dtype) if key is None else getattr(C, family)(key, dtype)
        fz, fimg, feat, nz, H, W, knum, boxlen = case
        _CASES[k] = (case, oracle.dibr_rasterization(H, W, fz, fimg, feat, nz, boxlen=boxlen, knum=knum, omp=True))
    return _CASES[k]


class Run:
    """One forward pass on the GPU with the fused loss on top; `expected` gives the oracle's gradients for a scale."""

    def __init__(self, case, ref, dtype, learn_feat, with_soft, seed, soft_sum=False):
        fz, fimg, feat, nz, H, W, knum, boxlen = case
        self.case, self.ref, self.dtype, self.with_soft, self.soft_sum = case, ref, dtype, with_soft, soft_sum
        self.G1, self.G2 = C.loss_weights(fimg.shape[0], H, W, feat.shape[-1], dtype, seed)
        self.a = fimg.cuda().requires_grad_()
        self.f = feat.cuda().requires_grad_(learn_feat)
        out, soft, face_idx = kal().render.mesh.dibr_rasterization(H, W, fz.cuda(), self.a, self.f, nz.cuda(), boxlen=boxlen, knum=knum)
        ws = kal().metrics.render.weighted_sum
        self.loss = ws(out, self.G1.cuda(), soft, self.G2.cuda()) if with_soft else ws(out, self.G1.cuda())
        assert type(self.loss.grad_fn).__name__ == '_WeightedSumDibrBackward'
        if soft_sum:
            self.loss = self.loss + soft.sum()        # a second consumer: the DIB-R node's own backward runs as well
        # the backward comparison means nothing on another image
        assert torch.equal(face_idx.cpu(), ref['face_idx'])
        assert torch.equal(out.detach().cpu(), ref['features'])
        self.face_idx = face_idx

    def expected(self, scale):
        """-> (image-coordinate gradient, feature gradient, sum of the image gradient's terms' magnitudes) for d(scale * loss)."""
        fz, fimg, feat, nz, H, W, knum, boxlen = self.case
        s = torch.tensor(scale, dtype=self.dtype)
        g1 = s * self.G1                                # the single rounded product the kernels form
        gr_img, gr_feat, sr = oracle.rasterize_backward(g1, self.ref['face_idx'], self.ref['weights'], fimg, feat, 1e-8, return_abs=True)
        if not (self.with_soft or self.soft_sum):
            return gr_img, gr_feat, sr
        g2 = s * self.G2 if self.with_soft else torch.zeros_like(self.G2)
        if self.soft_sum:
            g2 = g2 + s
        gs_img, ss = _soft_backward_on_the_gpu_forwards_outputs(g2, fimg, self.face_idx, self.ref, boxlen, knum)
        return gr_img + gs_img, gr_feat, sr + ss


def _excess(got, want, tol):
    """max over the elements of |got - want| / (tol |want| + tol median|want != 0|): printed before every assertion (pytest -s)."""
    a, b = got.detach().double().cpu(), want.double()
    nz = b[b != 0].abs()
    bound = tol * b.abs() + tol * (float(nz.median()) if nz.numel() else 0.0)
    return float(((a - b).abs() / bound.clamp(min=1e-300)).max())


def _unfused_verdict(run, scale, want_img, tol):
    """The issue's triage of a small case that misses plain rel_close: the torch spelling of the loss on the same inputs against the
    same bound.  Both miss: the bound; only the fused path: a kernel bug."""
    from kaolin_amd.utils.testing import elementwise_mismatch
    fz, fimg, feat, nz, H, W, knum, boxlen = run.case
    a = fimg.cuda().requires_grad_()
    out, soft, _ = kal().render.mesh.dibr_rasterization(H, W, fz.cuda(), a, feat.cuda(), nz.cuda(), boxlen=boxlen, knum=knum)
    loss = (out * run.G1.cuda()).sum()
    if run.with_soft:
        loss = loss + (soft * run.G2.cuda()).sum()
    (scale * loss).backward()
    m = elementwise_mismatch(a.grad, want_img, tol)
    return 'the unfused spelling meets the same bound: a bug of the fused path' if m is None else f'the unfused spelling misses it too ({m})'


def _compare(run, got_img, got_feat, scale, slack, what=''):
    from kaolin_amd.utils.testing import elementwise_mismatch
    tol = TOL[run.dtype]
    want_img, want_feat, terms = run.expected(scale)
    assert float(want_img.abs().max()) > 0
    print(f'[{what}] image gradient: worst element at {_excess(got_img, want_img, tol):.3f} x the plain bound')
    if slack:
        assert rel_close(got_img, want_img, tol, term_abs_sum=terms)
    else:
        m = elementwise_mismatch(got_img, want_img, tol)
        assert m is None, f'{m}; {_unfused_verdict(run, scale, want_img, tol)}'
    if run.f.requires_grad:
        assert float(want_feat.abs().max()) > 0
        print(f'[{what}] feature gradient: worst element at {_excess(got_feat, want_feat, tol):.3f} x the plain bound')
        assert rel_close(got_feat, want_feat, tol)
    else:
        assert got_feat is None                       # "no feature gradient" means none, not zeros
    return want_img, want_feat


def _backward(run, scale):
    (scale * run.loss).backward()
    assert torch.isfinite(run.a.grad).all()
    return run.a.grad, run.f.grad


# ------------------------------------------------------------------ ragged: every D of the launchers' switch
@pytest.mark.parametrize('learn_feat', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('D', C.RAGGED_D)
def test_ragged_both_terms(D, dtype, learn_feat):
    case, ref = _case('ragged', D, dtype)
    run = Run(case, ref, dtype, learn_feat, True, 10 + D)
    got_img, got_feat = _backward(run, -0.375)
    _compare(run, got_img, got_feat, -0.375, False, f'ragged D={D}')
    if D in (3, 5) and learn_feat:
        # control: the same GPU gradient against the oracle at scale 1 -- what a kernel that dropped `gs *` would have to match --
        # is reported as a mismatch: the comparison tells a dropped scale from a correct one
        from kaolin_amd.utils.testing import elementwise_mismatch
        unscaled_img, unscaled_feat, _ = run.expected(1.0)
        assert elementwise_mismatch(got_img, unscaled_img, TOL[dtype]) is not None
        assert elementwise_mismatch(got_feat, unscaled_feat, TOL[dtype]) is not None


@pytest.mark.parametrize('learn_feat', [False, True])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('D', [3, 5])
def test_ragged_image_only(D, dtype, learn_feat):
    """w_soft_mask = NULL at the C ABI: the soft mask's launch is skipped, the rasterizer's runs alone."""
    case, ref = _case('ragged', D, dtype)
    run = Run(case, ref, dtype, learn_feat, False, 20 + D)
    got_img, got_feat = _backward(run, -0.375)
    _compare(run, got_img, got_feat, -0.375, False, f'ragged image-only D={D}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('D', [3, 5])
def test_ragged_zero_scale_gives_exact_zeros(D, dtype):
    """(0 * loss).backward(): every term is 0 * W[p] times something finite -- exactly zero (-0.0 allowed), not rounding noise, and
    the gradients exist."""
    case, ref = _case('ragged', D, dtype)
    run = Run(case, ref, dtype, True, True, 30 + D)
    got_img, got_feat = _backward(run, 0.0)
    assert got_img.shape == run.a.shape and bool((got_img == 0).all())
    assert got_feat.shape == run.f.shape and bool((got_feat == 0).all())


# ------------------------------------------------------------------ tiny, views
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('D', C.TINY_D)
def test_tiny(D, dtype):
    case, ref = _case('tiny', D, dtype)
    run = Run(case, ref, dtype, True, True, 40 + D)
    got_img, got_feat = _backward(run, 3.0)
    _compare(run, got_img, got_feat, 3.0, False, f'tiny D={D}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B', C.VIEWS_B)
def test_views(B, dtype):
    case, ref = _case('views', B, dtype)
    run = Run(case, ref, dtype, True, True, 50 + B)
    got_img, got_feat = _backward(run, 3.0)
    want_img, _ = _compare(run, got_img, got_feat, 3.0, False, f'views B={B}')
    # (the oracle's gradient is non-zero in EVERY view: one that the list kernel's groups skipped would have failed above)
    assert bool((want_img.reshape(B, -1).abs().amax(dim=1) > 0).all())


# ------------------------------------------------------------------ hot faces
HOT = [('hot', 40), ('hot', 2500), ('hot_slivers', None)]
HOT_IDS = ['40', '2500', 'slivers']


@pytest.mark.parametrize('with_soft', [True, False], ids=['both', 'image-only'])
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('family,key', HOT, ids=HOT_IDS)
def test_hot_faces_and_a_second_backward(family, key, dtype, with_soft):
    """The hot-face table in use (the recipe's 2 and 158 faces) and over its limit (the slivers), float32 (which uses the table) and
    float64 (which never does).  Image-only: the rasterizer's list launch still gets the table and folds zeros.  The second backward
    through the retained graph starts from a fresh gradient buffer and from partial sums the first one left cleared: the same
    oracle bound again."""
    case, ref = _case(family, key, dtype)
    run = Run(case, ref, dtype, False, with_soft, 60)
    first, = torch.autograd.grad(run.loss, [run.a], retain_graph=True)
    second, = torch.autograd.grad(run.loss, [run.a])
    _compare(run, first, None, 1.0, True, f'{family} {key} first')
    _compare(run, second, None, 1.0, True, f'{family} {key} second')


@pytest.mark.parametrize('family,key', [HOT[0], HOT[2]], ids=[HOT_IDS[0], HOT_IDS[2]])
def test_hot_faces_with_another_consumer_of_the_soft_mask(family, key):
    """loss + soft.sum(): the DIB-R node's own backward (gradient 1 on the soft mask) and the fused node's both land in the input
    gradient -- the oracle's with g2 + 1."""
    case, ref = _case(family, key, torch.float)
    run = Run(case, ref, torch.float, False, True, 61, soft_sum=True)
    got_img, got_feat = _backward(run, 1.0)
    _compare(run, got_img, got_feat, 1.0, True, f'{family} {key} + soft.sum()')
