"""ops.gaussians.transform_gaussians / transform_shs without a GPU: the generated term lists against the projection oracle, the
torch formulation against the extended-precision recurrence helper (tests/gaussian_transforms_bruteforce.py: the bound
gamma_n * magnitude + u |want|, its counts n), and both against what the reference returned (tests/golden/gaussian_transforms.npz,
written by make_golden_gaussian_transforms.py).  The reference's bands 2 and 3 carry 4-digit coefficients: against it, the margin is
its own recorded deviation from the oracle, ``refdev``, plus our bound."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import gaussian_transforms_bruteforce as bf
from conftest import GOLDEN_DIR, ROOT
from kaolin_amd.ops.gaussians import transform_gaussians, transform_shs, transforms
from kaolin_amd.math import quat as quat_ops

GOLD = np.load(os.path.join(GOLDEN_DIR, 'gaussian_transforms.npz'))
DTYPES = (('f32', torch.float32, 'float32'), ('f64', torch.float64, 'float64'))
FIXTURE_TRANSFORMS = ('identity', 'translation', 'uniform_scale', 'trs45', 'yaw180', 'pitch180', 'roll180', 'batched_trs', 'batched_180',
                      'batched_translation', 'batched_scale')
ORACLE_NOISE = 4e-15        # the projection oracle itself (fit residual, D D^T - I: <= 3e-15)


def _t(a, dtype):
    return torch.from_numpy(np.asarray(a, dtype=np.float64)).to(dtype)


def _fixture(dtype, xyzw):
    ori = GOLD['fix_orientations']
    if xyzw:
        ori = np.concatenate([ori[:, 1:], ori[:, :1]], axis=1)
    return _t(GOLD['fix_positions'], dtype), _t(ori, dtype), _t(GOLD['fix_scales'], dtype), _t(GOLD['fix_sh'], dtype)


def test_generated_table_is_current():
    spec = importlib.util.spec_from_file_location('gen_sh_rotation_table', os.path.join(ROOT, 'tools', 'gen_sh_rotation_table.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    assert open(gen.HEADER).read() == gen.render_header()
    assert open(gen.MODULE).read() == gen.render_module()
    assert (len(bf.table.BAND2), len(bf.table.BAND3)) == (77, 189)


def test_recurrence_equals_projection_oracle():
    """pins the generated table: D^1..D^3 of 64 proper rotations against the least-squares projection, within 1e-13"""
    R = GOLD['rand_R']
    mats, _ = bf.recurrence_matrices(R, 3)
    worst = 0.0
    for k in range(R.shape[0]):
        D, residual = bf.projection_matrices(R[k])
        assert residual < 1e-14
        blocks = np.zeros((16, 16))
        blocks[0, 0] = 1
        for l, M in enumerate(mats, start=1):
            blocks[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = M[k].astype(np.float64)
        worst = max(worst, np.abs(D - blocks).max())
    print('recurrence - projection', worst)
    assert worst < 1e-13


@pytest.mark.parametrize('per_gaussian', [False, True])
@pytest.mark.parametrize('degree', [None, 0, 1, 2, 3])
@pytest.mark.parametrize('xyzw,logs', [(False, False), (True, True)])
def test_torch_formulation_float64(degree, per_gaussian, xyzw, logs):
    case = bf.make_case(33, degree, per_gaussian, seed=7)
    want = bf.reference(case['positions'], case['orientations'], case['scales'], case['transform'], case['sh_coeff'], logs, xyzw,
                        min_margin=bf.MIN_MARGIN)
    args = [_t(case[k], torch.float64) for k in ('positions', 'orientations', 'scales', 'transform')]
    sh = None if degree is None else _t(case['sh_coeff'], torch.float64)
    got = transform_gaussians(*args, sh, use_log_scales=logs, use_xyzw=xyzw)
    assert (got[3] is None) == (degree is None)
    for name, g in zip(('positions', 'orientations', 'scales', 'sh_coeff'), got):
        if g is not None:
            bf.check_share(name, g.numpy(), *want[name], bf.COUNTS[name], 'float64')


def test_transform_shs_sheared_matrix():
    """R is used as given: the same polynomials on a matrix that is no rotation"""
    rng = np.random.default_rng(3)
    R = (bf.rotations_with_margin(5, rng) + rng.uniform(-0.3, 0.3, (5, 3, 3))).astype(np.float32).astype(np.float64)
    sh = rng.standard_normal((5, 16, 3)).astype(np.float32).astype(np.float64)
    for tag, dtype, name in DTYPES:
        bf.check_share('sheared', transform_shs(_t(sh, dtype), _t(R, dtype)).numpy(), *bf.reference_shs(sh, R), bf.N_SH, name)


@pytest.mark.parametrize('tag,dtype,name', DTYPES)
@pytest.mark.parametrize('tf', FIXTURE_TRANSFORMS)
def test_geometry_against_reference(tf, tag, dtype, name):
    """positions, orientations and scales against the reference's returns in the same dtype, held to the derived bound: n = 4 for
    positions and scales (a few ulp in float64), 32 for orientations"""
    transform = _t(GOLD[f'tf_{tf}'], dtype)
    for xyzw in (0, 1):
        pos, ori, scl, _ = _fixture(dtype, xyzw)
        exact = bf.reference(pos.numpy(), ori.numpy(), scl.numpy(), transform.reshape(-1, 4, 4).numpy(), None, False, bool(xyzw))
        exact_log = bf.reference(pos.numpy(), ori.numpy(), scl.numpy(), transform.reshape(-1, 4, 4).numpy(), None, True, bool(xyzw))
        for logs in (0, 1):
            got = transform_gaussians(pos, ori, scl, transform, use_log_scales=bool(logs), use_xyzw=bool(xyzw))
            assert got[3] is None
            for key, field, g in zip(('pos', 'ori', 'scl'), ('positions', 'orientations', 'scales'), got):
                ref = GOLD[f'ret_{tf}_{tag}_x{xyzw}_l{logs}_{key}']
                assert g.dtype == dtype and g.shape == ref.shape
                magnitude = (exact_log if logs else exact)[field][1]
                bf.check_share(f'{tf} {field}', g.numpy(), ref, magnitude, bf.COUNTS[field], name)


@pytest.mark.parametrize('tag,dtype,name', DTYPES)
def test_sh_against_reference(tag, dtype, name):
    """|ours - reference| <= |refdev| (the reference's own deviation from the oracle) + the reference's rounding + our bound"""
    def held(label, got, ref, ref64, refdev, want, magnitude):
        u = bf.UNIT[name]
        margin = np.abs(refdev) + np.abs(ref - ref64) + ORACLE_NOISE * magnitude + bf.gamma(bf.N_SH, u) * magnitude + u * np.abs(want)
        ratio = (np.abs(got - ref) / margin).max()
        print(f'sh against reference {label} {name}: {float(ratio):.4f}; |refdev| up to {np.abs(refdev).max():.3e}')
        assert ratio <= 1

    sh, R = GOLD['rand_sh'], GOLD['rand_R']
    got = transform_shs(_t(sh, dtype), _t(R, dtype)).numpy()
    want, magnitude = bf.reference_shs(sh, _t(R, dtype).numpy())
    held('random', got, GOLD[f'rand_ret_{tag}'], GOLD['rand_ret_f64'], GOLD['rand_refdev'], want, magnitude)
    for tf in FIXTURE_TRANSFORMS:
        pos, ori, scl, fsh = _fixture(dtype, 0)
        transform = _t(GOLD[f'tf_{tf}'], dtype)
        got = transform_gaussians(pos, ori, scl, transform, fsh)[3].numpy()
        want, magnitude = bf.reference_shs(fsh.numpy(), bf.decompose(transform.reshape(-1, 4, 4).numpy())[3])
        held(tf, got, GOLD[f'ret_{tf}_{tag}_x0_l0_sh'], GOLD[f'ret_{tf}_f64_x0_l0_sh'], GOLD[f'refdev_{tf}'], want, magnitude)


@pytest.mark.parametrize('tag,dtype,name', DTYPES)
def test_exact_cases_of_the_reference_test(tag, dtype, name):
    """identity, translation and uniform scale leave the SH unchanged; the 180 degree rotations flip the golden's index sets"""
    pos, ori, scl, sh = _fixture(dtype, 0)
    for tf in ('identity', 'translation', 'uniform_scale', 'batched_translation', 'batched_scale'):
        out = transform_gaussians(pos, ori, scl, _t(GOLD[f'tf_{tf}'], dtype), sh)
        assert torch.equal(out[3], sh), tf
        assert torch.equal(out[1], ori), tf
    for tf in ('yaw180', 'pitch180', 'roll180', 'batched_180'):
        out = transform_gaussians(pos, ori, scl, _t(GOLD[f'tf_{tf}'], dtype), sh)[3]
        for g in range(3):
            flipped = [k for k in range(16) if (out[g, k] + sh[g, k]).abs().max() < 1e-5]
            assert flipped == [k for k in GOLD[f'flip_{tf}'][g] if k >= 0], (tf, g)
            kept = [k for k in range(16) if k not in flipped]
            torch.testing.assert_close(out[g, kept], sh[g, kept], atol=1e-5, rtol=0)


@pytest.mark.parametrize('xyzw,logs', [(False, False), (True, True), (False, True)])
def test_inverse_transform_recovers_the_input(xyzw, logs):
    """forward(T) then forward(T^-1), float64: a similarity with scale in [0.5, 2] has a condition number <= 4 and both passes are
    a few hundred operations, so 1e-12 is generous; quaternions are recovered normalized and up to sign"""
    case = bf.make_case(17, 3, True, seed=11)
    rng = np.random.default_rng(12)      # (make_case rounds its matrices to float32: similarities only to 6e-8)
    case['transform'][:, :3, :3] = bf.rotations_with_margin(17, rng) * rng.uniform(0.5, 2.0, (17, 1, 1))
    args = [_t(case[k], torch.float64) for k in ('positions', 'orientations', 'scales', 'transform', 'sh_coeff')]
    args[1] = quat_ops.quat_unit(args[1])
    fwd = transform_gaussians(*args, use_log_scales=logs, use_xyzw=xyzw)
    back = transform_gaussians(fwd[0], fwd[1], fwd[2], torch.linalg.inv(args[3]), fwd[3], use_log_scales=logs, use_xyzw=xyzw)
    for k in (0, 2, 4):
        torch.testing.assert_close(back[3 if k == 4 else k], args[k], atol=1e-12, rtol=1e-12)
    sign = torch.sign((back[1] * args[1]).sum(-1, keepdim=True))
    torch.testing.assert_close(back[1] * sign, args[1], atol=1e-12, rtol=1e-12)


def test_errors_match_the_reference():
    p, q, s, t = torch.zeros(3, 3), torch.zeros(3, 4), torch.zeros(3, 3), torch.eye(4)
    eye = torch.eye(3)[None]
    calls = {'err_dtype': lambda: transform_gaussians(p, q, s, t.double()),
             'err_sh_dtype': lambda: transform_gaussians(p, q, s, t, torch.zeros(3, 4, 3).double()),
             'err_shs_dtype': lambda: transform_shs(torch.zeros(3, 4, 3), eye.double()),
             'err_not_square': lambda: transform_shs(torch.zeros(3, 5, 3), eye),
             'err_degree': lambda: transform_shs(torch.zeros(3, 25, 3), eye),
             'err_channels': lambda: transform_shs(torch.zeros(3, 4, 2), eye),
             'err_batch': lambda: transform_shs(torch.zeros(3, 4, 3), eye.repeat(2, 1, 1)),
             'err_r_shape': lambda: transform_shs(torch.zeros(3, 4, 3), torch.eye(4)[None])}
    for key, call in calls.items():
        kind, text = GOLD[key]
        with pytest.raises({'AssertionError': AssertionError, 'NotImplementedError': NotImplementedError}[str(kind)]) as e:
            call()
        assert str(e.value) == str(text), key
    for bad in (torch.eye(4)[None].repeat(2, 1, 1), torch.eye(3), torch.eye(4)[None, None]):
        with pytest.raises(AssertionError):
            transform_gaussians(p, q, s, bad)
    with pytest.raises(NotImplementedError):
        transform_gaussians(p, q, s, t, torch.zeros(3, 25, 3))


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_half_and_bfloat16_run(dtype):
    case = bf.make_case(9, 3, True, seed=5)
    args = [_t(case[k], dtype) for k in ('positions', 'orientations', 'scales', 'transform', 'sh_coeff')]
    out = transform_gaussians(*args[:4], args[4])
    full = transform_gaussians(*(a.float() for a in args[:4]), args[4].float())
    eps = torch.finfo(dtype).eps
    for o, f, a in zip(out, full, (args[0], args[1], args[2], args[4])):
        assert o.dtype == dtype and o.shape == a.shape and torch.isfinite(o).all()
        assert (o.float() - f).abs().max() <= 64 * eps * (1 + f.abs().max())
    assert transform_shs(args[4], args[3][:1, :3, :3]).dtype == dtype


def test_dispatch_names_and_exports():
    import kaolin_amd
    from kaolin_amd import _C
    assert kaolin_amd.ops.gaussians.transform_gaussians is transform_gaussians
    assert not hasattr(kaolin_amd.ops.gaussian, 'transform_gaussians')     # the reference's second spelling does not export it
    assert callable(_C.ops.gaussians.transform_gaussians_forward_cuda) and callable(_C.ops.gaussians.transform_gaussians_backward_cuda)
    assert kaolin_amd.math.quat.quat_mul is quat_ops.quat_mul


def test_quat_helpers():
    rng = np.random.default_rng(2)
    for branch in range(4):
        R = bf.rotations_with_margin(4, rng, branch)
        want, b, _ = bf.quat_from_rot33(R)
        assert (b == branch).all()
        got = quat_ops.quat_from_rot33(torch.from_numpy(R))
        np.testing.assert_allclose(got.numpy(), want.astype(np.float64), atol=1e-14)
    a, b = torch.randn(5, 4, dtype=torch.float64), torch.randn(5, 4, dtype=torch.float64)
    np.testing.assert_allclose(quat_ops.quat_mul(a, b).numpy(), bf.quat_mul(a.numpy(), b.numpy()), atol=1e-15)
    np.testing.assert_allclose(quat_ops.quat_unit(a).norm(dim=-1).numpy(), 1, atol=1e-15)
    assert torch.equal(quat_ops.quat_unit(torch.zeros(1, 4)), torch.zeros(1, 4))


def test_gradcheck_float64():
    case = bf.make_case(3, 3, True, seed=13)
    for per, xyzw, logs in ((True, False, False), (False, True, True)):
        args = [_t(case[k], torch.float64).requires_grad_() for k in ('positions', 'orientations', 'scales', 'transform', 'sh_coeff')]
        if not per:
            args[3] = args[3].detach()[0].clone().requires_grad_()
        assert torch.autograd.gradcheck(
            lambda p, q, s, t, c: transform_gaussians(p, q, s, t, c, use_log_scales=logs, use_xyzw=xyzw), args, atol=1e-7)
    R = _t(case['transform'][:, :3, :3], torch.float64).requires_grad_()
    sh = _t(case['sh_coeff'], torch.float64).requires_grad_()
    assert torch.autograd.gradcheck(transform_shs, (sh, R), atol=1e-7)


def test_gpu_case_seeds_meet_the_branch_condition():
    """The condition on the GPU tests' inputs, checked here for the committed seeds: every comparison of quat(R)'s branch rule has a
    margin above MIN_MARGIN in every case, and all four branches occur (shared transforms: one case each)."""
    seen = set()
    for n in bf.GPU_SIZES:
        case = bf.make_case(n, None, True, seed=100 + n)
        _, branch, margin = bf.quat_from_rot33(bf.decompose(case['transform'])[3])
        assert margin.min() > bf.MIN_MARGIN
        seen.update(branch.tolist())
    assert seen == {0, 1, 2, 3}
    for b in bf.GPU_SHARED_BRANCHES:
        case = bf.make_case(5, None, False, seed=200 + b, branch=b)
        _, branch, margin = bf.quat_from_rot33(bf.decompose(case['transform'])[3])
        assert branch.tolist() == [b] and margin.min() > bf.MIN_MARGIN
    for name in ('yaw180', 'pitch180', 'roll180'):
        _, branch, margin = bf.quat_from_rot33(GOLD[f'tf_{name}'][:, :3, :3])
        assert margin.min() > bf.MIN_MARGIN
        seen.add(int(branch[0]))
    assert {1, 2, 3} <= seen
