"""ops.gaussians.transform_gaussians / transform_shs on the GPU: csrc/gaussian_transform.hip per element against the
extended-precision recurrence helper on the CPU (tests/gaussian_transforms_bruteforce.py),

    |hip - want| <= gamma_n * (sum of term magnitudes) + u |want|,     n counted from the kernel's operations,

and its backward against float64 autograd of the package's torch formulation under the same kind of bound.  Every test prints its
worst share of the bound and fails above 1.  The torch formulation is taken away while the device side runs, so a float32 / float64
GPU call that fell back to it fails.  The rotations are chosen so that every comparison of quat(R)'s branch rule is decided by more
than bf.MIN_MARGIN (asserted in float64 inside bf.reference; test_gaussian_transforms_cpu.py checks the seeds and that all four
branches occur): a float32 run cannot take another branch, and with it another sign."""
import contextlib

import numpy as np
import pytest
import torch

import gaussian_transforms_bruteforce as bf
from kaolin_amd.ops.gaussians import transform_gaussians, transform_shs, transforms

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FORMULATIONS = {n: getattr(transforms, n) for n in ('_torch_transform_gaussians', '_torch_transform_shs')}
DTYPES = ((torch.float32, 'float32'), (torch.float64, 'float64'))
NAMES = ('positions', 'orientations', 'scales', 'sh_coeff')
WORKGROUP = 128                                  # GT_THREADS of csrc/gaussian_transform.hip
assert set(bf.GPU_SIZES) == {1, 63, 64, 65, WORKGROUP - 1, WORKGROUP + 1, 2 * WORKGROUP + 1}


@pytest.fixture(autouse=True)
def hip_path_only(monkeypatch):
    """A float32 / float64 GPU call that reached a torch formulation would pass these tests without running a kernel."""
    for name in FORMULATIONS:
        monkeypatch.setattr(transforms, name, None)


@contextlib.contextmanager
def _formulations():
    """The torch formulations back in place while the CPU side of a test runs"""
    hidden = {n: getattr(transforms, n) for n in FORMULATIONS}
    for n, f in FORMULATIONS.items():
        setattr(transforms, n, f)
    try:
        yield
    finally:
        for n, f in hidden.items():
            setattr(transforms, n, f)


def _dev(a, dtype, grad=False):
    return None if a is None else torch.from_numpy(a).to(dtype).to(DEV).requires_grad_(grad)


def _scatter(t):
    """the same values as a view that is not contiguous: every second element of the last axis of a buffer twice as wide"""
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
    wide[..., ::2] = t.detach()
    view = wide[..., ::2]
    assert not view.is_contiguous() or view.numel() <= 1
    return view.requires_grad_(t.requires_grad)


def _autograd_reference(case, cot, logs, xyzw, shape):
    """float64 autograd of the torch formulation on the CPU -> {name: gradient}"""
    with _formulations():
        leaves = {k: torch.from_numpy(case[k]).requires_grad_() for k in NAMES if case[k] is not None}
        tf = torch.from_numpy(case['transform']).reshape(shape)
        outs = transform_gaussians(leaves['positions'], leaves['orientations'], leaves['scales'], tf, leaves.get('sh_coeff'),
                                   use_log_scales=logs, use_xyzw=xyzw)
        total = sum((o * torch.from_numpy(cot[k])).sum() for k, o in zip(NAMES, outs) if o is not None)
        grads = torch.autograd.grad(total, list(leaves.values()))
    return {k: g.numpy() for k, g in zip(leaves, grads)}


def _run(case, dtype, name, logs=False, xyzw=False, shape=None, scatter=False, seed=0):
    """Forward and backward of transform_gaussians at `case` against the helper; shape: how the transform is passed.  -> the
    outputs and gradients of the device run"""
    tf = case['transform'] if shape is None else case['transform'].reshape(shape)
    want = bf.reference(case['positions'], case['orientations'], case['scales'], case['transform'], case['sh_coeff'], logs, xyzw,
                        min_margin=bf.MIN_MARGIN)
    args = {k: _dev(case[k], dtype, grad=True) for k in NAMES}
    t = _dev(tf, dtype)
    if scatter:
        args = {k: None if v is None else _scatter(v) for k, v in args.items()}
        t = _scatter(t)
    outs = transform_gaussians(args['positions'], args['orientations'], args['scales'], t, args['sh_coeff'], use_log_scales=logs,
                               use_xyzw=xyzw)
    assert (outs[3] is None) == (case['sh_coeff'] is None)
    rng = np.random.default_rng(seed)
    cot = {k: bf.half_cotangents(case[k].shape, rng) for k in NAMES if case[k] is not None}
    live = [(k, o) for k, o in zip(NAMES, outs) if o is not None]
    grads = torch.autograd.grad([o for _, o in live], [args[k] for k, _ in live], [_dev(cot[k], dtype) for k, _ in live])
    torch.cuda.synchronize()
    for k, o in live:
        assert o.dtype == dtype and o.shape == args[k].shape and o.is_contiguous()
        bf.check_share(f'forward {k}', o.detach().cpu().numpy(), *want[k], bf.COUNTS[k], name)
    ref = _autograd_reference(case, cot, logs, xyzw, tf.shape)
    magnitudes = bf.grad_magnitudes(cot, case['orientations'], case['scales'], case['transform'], logs, xyzw)
    for (k, _), g in zip(live, grads):
        bf.check_share(f'backward {k}', g.cpu().numpy(), ref[k], magnitudes[k], bf.GRAD_COUNTS[k], name)
        if k == 'scales' and logs:                               # the derivative of scales + log(s): the cotangent itself
            assert np.array_equal(g.cpu().numpy().astype(np.float64), cot[k])
    return [o.detach() for _, o in live], list(grads)


@pytest.mark.parametrize('dtype,name', DTYPES)
@pytest.mark.parametrize('degree', [0, 1, 2, 3])
@pytest.mark.parametrize('n', bf.GPU_SIZES)
def test_per_gaussian_transform(n, degree, dtype, name):
    flags = (n + degree) % 4
    _run(bf.make_case(n, degree, True, seed=100 + n), dtype, name, logs=bool(flags & 1), xyzw=bool(flags & 2))


@pytest.mark.parametrize('dtype,name', DTYPES)
@pytest.mark.parametrize('degree', [0, 1, 2, 3])
@pytest.mark.parametrize('n', bf.GPU_SIZES)
def test_shared_transform(n, degree, dtype, name):
    """(4, 4) and (1, 4, 4), one branch of quat(R) per size"""
    flags = (n + degree + 1) % 4
    branch = bf.GPU_SHARED_BRANCHES[(n + degree) % 4]
    case = bf.make_case(n, degree, False, seed=200 + branch, branch=branch)
    first = _run(case, dtype, name, logs=bool(flags & 1), xyzw=bool(flags & 2), shape=(4, 4))
    second = _run(case, dtype, name, logs=bool(flags & 1), xyzw=bool(flags & 2), shape=(1, 4, 4))
    assert all(torch.equal(a, b) for a, b in zip(first[0] + first[1], second[0] + second[1]))


@pytest.mark.parametrize('dtype,name', DTYPES)
@pytest.mark.parametrize('logs', [False, True])
@pytest.mark.parametrize('xyzw', [False, True])
@pytest.mark.parametrize('per_gaussian', [False, True])
def test_flags_and_no_sh(per_gaussian, xyzw, logs, dtype, name):
    case = bf.make_case(WORKGROUP + 1, None, per_gaussian, seed=300)
    _run(case, dtype, name, logs=logs, xyzw=xyzw)
    case = bf.make_case(WORKGROUP + 1, 3, per_gaussian, seed=301)
    _run(case, dtype, name, logs=logs, xyzw=xyzw)


@pytest.mark.parametrize('dtype,name', DTYPES)
@pytest.mark.parametrize('degree', [0, 2, 3])
@pytest.mark.parametrize('per_gaussian', [False, True])
def test_views_that_are_not_contiguous(per_gaussian, degree, dtype, name):
    """every input a strided view, and transform_shs on a slice of a larger model (rows of degree 2 then start off a 16-byte
    boundary; test_rows_off_a_16_byte_boundary has the degrees whose rows are whole 16-byte chunks)"""
    case = bf.make_case(2 * WORKGROUP + 1, degree, per_gaussian, seed=310)
    _run(case, dtype, name, scatter=True)
    sh = _dev(case['sh_coeff'], dtype)[1:]
    R = _dev(bf.decompose(case['transform'])[3].astype(np.float64), dtype)
    R = R[1:] if per_gaussian else R
    want, magnitude = bf.reference_shs(sh.cpu().numpy(), R.cpu().numpy())
    bf.check_share('transform_shs on a slice', transform_shs(sh, R).cpu().numpy(), want, magnitude, bf.N_SH, name)


def _off_by_one_element(t):
    """the same values, contiguous, in a buffer that starts one element after a 16-byte boundary"""
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(t.shape)
    view.copy_(t.detach())
    assert view.is_contiguous() and view.data_ptr() % 16 == t.element_size()
    return view.requires_grad_(t.requires_grad)


@pytest.mark.parametrize('dtype,name', DTYPES)
@pytest.mark.parametrize('degree', [1, 3])
@pytest.mark.parametrize('per_gaussian', [False, True])
def test_rows_off_a_16_byte_boundary(per_gaussian, degree, dtype, name):
    """Degrees 1 and 3 have rows of whole 16-byte chunks and move them with 16-byte accesses when the bases allow; here the
    coefficients (forward) and the cotangent (backward) are contiguous but start one element off: the element-by-element path"""
    rng = np.random.default_rng(315)
    n = WORKGROUP + 1
    R = bf.rotations_with_margin(n if per_gaussian else 1, rng).astype(np.float32).astype(np.float64)
    sh = rng.standard_normal((n, (degree + 1) ** 2, 3)).astype(np.float32).astype(np.float64)
    cot = bf.half_cotangents(sh.shape, rng)
    x = _off_by_one_element(_dev(sh, dtype, grad=True))
    out = transform_shs(x, _dev(R, dtype))
    grad, = torch.autograd.grad(out, x, _off_by_one_element(_dev(cot, dtype)))
    bf.check_share('off-boundary rows', out.detach().cpu().numpy(), *bf.reference_shs(sh, R), bf.N_SH, name)
    bf.check_share('off-boundary rows backward', grad.cpu().numpy(), *bf.reference_shs(cot, R, True), bf.N_SH, name)
    aligned = transform_shs(_dev(sh, dtype), _dev(R, dtype))                      # the 16-byte path: the same bits
    assert torch.equal(out.detach(), aligned)


@pytest.mark.parametrize('dtype,name', DTYPES)
def test_transform_shs_and_shear(dtype, name):
    """transform_shs takes R as it is: proper rotations and sheared matrices, shared and per Gaussian, with its gradient"""
    rng = np.random.default_rng(320)
    n = 2 * WORKGROUP + 1
    R = bf.rotations_with_margin(n, rng)
    R[::2] += rng.uniform(-0.3, 0.3, (R[::2].shape))
    R = R.astype(np.float32).astype(np.float64)
    for degree in (0, 1, 2, 3):
        sh = rng.standard_normal((n, (degree + 1) ** 2, 3)).astype(np.float32).astype(np.float64)
        cot = bf.half_cotangents(sh.shape, rng)
        for matrices in (R, R[:1]):
            x = _dev(sh, dtype, grad=True)
            out = transform_shs(x, _dev(matrices, dtype))
            grad, = torch.autograd.grad(out, x, _dev(cot, dtype))
            bf.check_share(f'transform_shs degree {degree}', out.detach().cpu().numpy(), *bf.reference_shs(sh, matrices), bf.N_SH, name)
            bf.check_share(f'transform_shs backward degree {degree}', grad.cpu().numpy(), *bf.reference_shs(cot, matrices, True),
                           bf.N_SH, name)


@pytest.mark.parametrize('dtype,name', DTYPES)
def test_same_bits_and_shared_equals_per_gaussian(dtype, name):
    """Two calls give the same bits, forward and backward; and (DESIGN.md promises it) one matrix passed as a shared transform and
    repeated per Gaussian gives the same bits too, both already compared with the oracle above"""
    case = bf.make_case(2 * WORKGROUP + 1, 3, False, seed=330)
    runs = [_run(case, dtype, name, logs=True) for _ in range(2)]
    repeated = dict(case, transform=np.repeat(case['transform'], case['positions'].shape[0], axis=0))
    runs.append(_run(repeated, dtype, name, logs=True))
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0][0] + runs[0][1], other[0] + other[1]))


def test_no_gaussians():
    for dtype, _ in DTYPES:
        empty = [torch.zeros(0, k, dtype=dtype, device=DEV, requires_grad=True) for k in (3, 4, 3)]
        sh = torch.zeros(0, 16, 3, dtype=dtype, device=DEV, requires_grad=True)
        for tf in (torch.eye(4, dtype=dtype, device=DEV), torch.zeros(0, 4, 4, dtype=dtype, device=DEV)):
            outs = transform_gaussians(*empty, tf, sh)
            assert [o.shape for o in outs] == [e.shape for e in empty] + [sh.shape]
            grads = torch.autograd.grad([o.sum() for o in outs], empty + [sh])
            assert all(g.shape == e.shape for g, e in zip(grads, empty + [sh]))
        assert transform_shs(sh, torch.eye(3, dtype=dtype, device=DEV)[None]).shape == sh.shape


def test_graph_capture():
    """Forward and backward in one captured graph (a single chain: no parallel branches); the replay equals eager bit for bit."""
    case = bf.make_case(2 * WORKGROUP + 1, 3, True, seed=340)
    args = [_dev(case[k], torch.float32, grad=True) for k in NAMES]
    tf = _dev(case['transform'], torch.float32)
    cot = [torch.ones_like(a) for a in args]

    def step():
        outs = transform_gaussians(args[0], args[1], args[2], tf, args[3], use_log_scales=True)
        return list(outs) + list(torch.autograd.grad(outs, args, cot))

    eager = [t.detach().clone() for t in step()]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                                   # (warm the allocator on the capture stream)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for t in captured:
        t.detach().zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b.detach()) for a, b in zip(eager, captured))


def test_transform_that_requires_grad_falls_back(monkeypatch):
    """The kernels build no gradient for the transform: such a call runs the torch formulation and returns one"""
    monkeypatch.undo()
    case = bf.make_case(65, 3, True, seed=350)
    args = [_dev(case[k], torch.float64, grad=True) for k in NAMES]
    tf = _dev(case['transform'], torch.float64, grad=True)
    outs = transform_gaussians(args[0], args[1], args[2], tf, args[3])
    grad, = torch.autograd.grad(sum(o.sum() for o in outs), tf)
    with _formulations():
        cpu = [torch.from_numpy(case[k]).requires_grad_() for k in NAMES]
        tf_cpu = torch.from_numpy(case['transform']).requires_grad_()
        want, = torch.autograd.grad(sum(o.sum() for o in transform_gaussians(cpu[0], cpu[1], cpu[2], tf_cpu, cpu[3])), tf_cpu)
    torch.testing.assert_close(grad.cpu(), want, atol=1e-11, rtol=1e-11)
    R = tf.detach()[:, :3, :3].clone().requires_grad_()
    assert torch.autograd.grad(transform_shs(args[3], R).sum(), R)[0].shape == R.shape
    with torch.no_grad():                                        # no gradient is recorded: the kernels run
        monkeypatch.setattr(transforms, '_torch_transform_gaussians', None)
        assert transform_gaussians(args[0], args[1], args[2], tf, args[3])[0].shape == args[0].shape


@pytest.mark.parametrize('dtype,name', DTYPES)
def test_non_finite_rows_stay_in_their_row(dtype, name):
    """One NaN quaternion row and one zero column of A (per Gaussian): the other rows are what they are without them"""
    case = bf.make_case(WORKGROUP + 1, 3, True, seed=360)
    clean = transform_gaussians(*(_dev(case[k], dtype) for k in ('positions', 'orientations', 'scales', 'transform', 'sh_coeff')))
    bad = {k: v.copy() for k, v in case.items()}
    bad['orientations'][5] = np.nan
    bad['transform'][70, :3, 1] = 0
    out = transform_gaussians(*(_dev(bad[k], dtype) for k in ('positions', 'orientations', 'scales', 'transform', 'sh_coeff')))
    keep = torch.ones(WORKGROUP + 1, dtype=torch.bool, device=DEV)
    keep[[5, 70]] = False
    assert all(torch.equal(a[keep], b[keep]) for a, b in zip(clean, out))
