"""ops.conversions.gs_to_voxelgrid without a GPU: the numpy oracle (tests/gs_to_spc_bruteforce.py) against the reference's own
recorded result (tests/golden/gs_to_voxelgrid.npz: level 7 of its 8 Gaussians, and the level-0 / level-1 expectations of its test
file), then the package's torch formulation -- what CPU tensors run -- against the oracle: the integer results and cov3d_invs bit
for bit, the integral within one float32 ulp of the oracle's float64 value w:  |got - w| <= 2^-23 |w| + 2^-149  (the final
rounding plus double-level noise of exp and of the summation order, which is free).  The helpers are shared with
tests/test_gs_to_spc_gpu.py."""
import functools
import os

import numpy as np
import pytest
import torch

import gs_to_spc_bruteforce as bf
from conftest import GOLDEN_DIR

import kaolin_amd as kal

C = kal._C.ops.conversions
ISO, TOL = 11.345, 1. / 8.
REF_TOL = dict(atol=1e-4, rtol=1e-4)           # the reference's own test tolerance (test_gaussians.py)


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(GOLDEN_DIR, 'gs_to_voxelgrid.npz')))


def reference_inputs():
    g = golden()
    return g['xyz'], g['scales'], g['rots'], g['opacities']


@functools.lru_cache(maxsize=None)
def oracle_level7():
    """the oracle on the reference's case at level 7, computed once: pairs, cov3d_invs and the float64 integral"""
    xyz, scales, rots, opacities = reference_inputs()
    points, gid, boundary, cov = bf.gs_to_spc(xyz, scales, rots, ISO, TOL, 7)
    integral = bf.integrate_gs(points, gid, xyz, cov, opacities, 7, 10)
    for a in (points, gid, boundary, cov, integral):
        a.setflags(write=False)
    return points, gid, boundary, cov, integral


def random_gaussians(G, level, seed, voxels=(0.3, 2.0)):
    """means in [-0.9, 0.9]^3, scales of `voxels` voxel sizes of `level`, random unit quaternions, opacities in [0, 1]"""
    rng = np.random.RandomState(seed)
    means = rng.uniform(-0.9, 0.9, (G, 3)).astype(np.float32)
    scales = (rng.uniform(voxels[0], voxels[1], (G, 3)) * 2.0 / (1 << level)).astype(np.float32)
    q = rng.normal(size=(G, 4))
    rots = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    opacities = rng.uniform(0.0, 1.0, G).astype(np.float32)
    return means, scales, rots, opacities


def centred_gaussians(cells, level):
    """one Gaussian far below the clamp at the centre of every listed cell (x, y, z) of `level`: clamped to tol * voxel, its iso
    ellipsoid (radius sqrt(iso) / 8 = 0.42 voxels) lies inside the cell and inside every ancestor, so each yields exactly one pair"""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3)
    vs = 2.0 / (1 << level)
    means = (-1.0 + (cells + 0.5) * vs).astype(np.float32)
    G = len(cells)
    scales = np.full((G, 3), 1e-6, np.float32)
    rots = np.tile(np.array([[1, 0, 0, 0]], np.float32), (G, 1))
    opacities = np.linspace(0.1, 0.9, G).astype(np.float32)
    return means, scales, rots, opacities


def t(a, device='cpu'):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def check_against_oracle(case, level, device, iso=ISO, tol=TOL):
    """gs_to_spc_cuda on `device` equals the oracle exactly in all four results -> (oracle results, package results)"""
    means, scales, rots, _ = case
    want = bf.gs_to_spc(means, scales, rots, iso, tol, level)
    got = C.gs_to_spc_cuda(t(means, device), t(scales, device), t(rots, device), iso, tol, level)
    assert [g.dtype for g in got] == [torch.int16, torch.long, torch.bool, torch.float32]
    assert tuple(got[0].shape) == (len(want[0]), 3) and tuple(got[3].shape) == (len(means), 6)
    for name, w, g in zip(('points', 'gaus_id', 'pack_boundary', 'cov3d_invs'), want, got):
        assert str(g.device).startswith(device), name
        assert np.array_equal(w, g.cpu().numpy(), equal_nan=True), f'{name} differs at level {level}'
    return want, got


def ulp_share(got, w):
    """|got - w| as a share of the bound 2^-23 |w| + 2^-149 (w: the oracle's float64 value)"""
    got = np.asarray(got, dtype=np.float64)
    return np.abs(got - w) / (2.0 ** -23 * np.abs(w) + 2.0 ** -149)


def check_integral(case, level, step, device, pairs=None):
    means, scales, rots, opacities = case
    points, gid, _, cov = pairs if pairs is not None else bf.gs_to_spc(means, scales, rots, ISO, TOL, level)
    w = bf.integrate_gs(points, gid, means, cov, opacities, level, step)
    got = C.integrate_gs_cuda(t(points, device), t(gid, device), t(means, device), t(cov, device), t(opacities, device), level, step)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(points),)
    share = ulp_share(got.cpu().numpy(), w).max() if len(points) else 0.0
    print(f'integrate_gs {device} level {level} step {step}: {len(points)} pairs, worst share of the bound {share:.3f}')
    assert share <= 1.0
    return share


def bad_arguments(device):
    """(callable, what) pairs: every argument check of the two operators"""
    m, s, r, o = (t(a, device) for a in random_gaussians(4, 2, 0))
    p = torch.zeros((5, 3), dtype=torch.int16, device=device)
    gid = torch.zeros(5, dtype=torch.long, device=device)
    cov = torch.ones((4, 6), dtype=torch.float32, device=device)
    sp, ig = C.gs_to_spc_cuda, C.integrate_gs_cuda
    bad = [
        (lambda: sp(m.double(), s, r, ISO, TOL, 2), 'means3D dtype'),
        (lambda: sp(m, s.half(), r, ISO, TOL, 2), 'scales dtype'),
        (lambda: sp(m, s, r.long(), ISO, TOL, 2), 'rotations dtype'),
        (lambda: sp(m.t().contiguous().t(), s, r, ISO, TOL, 2), 'means3D not contiguous'),
        (lambda: sp(m, s, r[:, :3], ISO, TOL, 2), 'rotations not contiguous / wrong size'),
        (lambda: sp(m[:, :2].contiguous(), s, r, ISO, TOL, 2), 'means3D (G, 2)'),
        (lambda: sp(m, s[:3], r, ISO, TOL, 2), 'scales (G - 1, 3)'),
        (lambda: sp(m, s, r[:, :3].contiguous(), ISO, TOL, 2), 'rotations (G, 3)'),
        (lambda: sp(m.reshape(-1), s, r, ISO, TOL, 2), 'means3D 1D'),
        (lambda: sp(m, s, r, ISO, TOL, -1), 'level -1'),
        (lambda: sp(m, s, r, ISO, TOL, 16), 'level 16'),
        (lambda: ig(p.int(), gid, m, cov, o, 2, 10), 'points dtype'),
        (lambda: ig(p, gid.int(), m, cov, o, 2, 10), 'gaus_id dtype'),
        (lambda: ig(p, gid, m.double(), cov, o, 2, 10), 'means3D dtype'),
        (lambda: ig(p[:, :2].contiguous(), gid, m, cov, o, 2, 10), 'points (N, 2)'),
        (lambda: ig(p[:, :2], gid, m, cov, o, 2, 10), 'points not contiguous'),
        (lambda: ig(p, gid[:4], m, cov, o, 2, 10), 'gaus_id (N - 1)'),
        (lambda: ig(p, gid, m, cov[:, :5].contiguous(), o, 2, 10), 'cov3d_invs (G, 5)'),
        (lambda: ig(p, gid, m, cov[:3], o, 2, 10), 'cov3d_invs (G - 1, 6)'),
        (lambda: ig(p, gid, m, cov, o[:3], 2, 10), 'numel(opacities) != G'),
        (lambda: ig(p, gid, m, cov, o, 16, 10), 'level 16'),
        (lambda: ig(p, gid, m, cov, o, 2, 0), 'step 0'),
    ]
    if device != 'cpu':
        bad += [(lambda: sp(m, s.cpu(), r, ISO, TOL, 2), 'scales on another device'),
                (lambda: ig(p, gid.cpu(), m, cov, o, 2, 10), 'gaus_id on another device')]
    return bad


def check_empty_cases(device):
    for G in (0, 3):
        means, scales, rots, opacities = random_gaussians(G, 3, 1)
        means = means + np.float32(5.0)                                   # wholly outside [-1, 1]^3: no pair survives the root
        args = [t(a, device) for a in (means, scales, rots)]
        points, gid, boundary, cov = C.gs_to_spc_cuda(*args, ISO, TOL, 3)
        assert (points.dtype, gid.dtype, boundary.dtype, cov.dtype) == (torch.int16, torch.long, torch.bool, torch.float32)
        assert tuple(points.shape) == (0, 3) and tuple(gid.shape) == (0,) and tuple(boundary.shape) == (0,)
        assert tuple(cov.shape) == (G, 6)
        assert np.array_equal(cov.cpu().numpy(), bf.prepare(means, scales, rots, ISO, TOL, 3)[0])
        integral = C.integrate_gs_cuda(points, gid, args[0], cov, t(opacities, device), 3, 10)
        assert integral.dtype == torch.float32 and tuple(integral.shape) == (0,)
        voxels, merged = kal.ops.conversions.gs_to_voxelgrid(*args, t(opacities, device), 3)
        assert voxels.dtype == torch.int16 and tuple(voxels.shape) == (0, 3)
        assert merged.dtype == torch.float32 and tuple(merged.shape) == (0,)


# ------------------------------------------------------------------------------------------- the oracle against the reference
def test_oracle_reproduces_the_reference_record_at_level_7():
    """voxels equal and in order; opacities within the reference's tolerance.  Observed: 1.2e-7 at the worst of the recorded
    (every second) opacities."""
    g = golden()
    points, gid, boundary, cov, integral = oracle_level7()
    voxels, merged = points[boundary], bf.merge(integral.astype(np.float32), boundary)
    assert voxels.dtype == np.int16 and np.array_equal(voxels, g['voxels_7'])
    k = int(g['opacity_stride'])
    print('level 7: worst opacity difference to the record', np.abs(merged[::k] - g['opacities_7']).max())
    assert np.allclose(merged[::k], g['opacities_7'], **REF_TOL)


@pytest.mark.parametrize('level', [0, 1])
def test_oracle_reproduces_the_reference_expectations(level):
    g = golden()
    voxels, merged = bf.gs_to_voxelgrid(*reference_inputs(), level, ISO, TOL, 10)
    assert np.array_equal(voxels, g[f'voxels_{level}'])
    assert np.allclose(merged, g[f'opacities_{level}'], **REF_TOL)


# ------------------------------------------------------------------------------------ the torch formulation against the oracle
@pytest.mark.parametrize('level', range(6))
@pytest.mark.parametrize('G', [1, 7, 64])
def test_torch_formulation_equals_oracle(G, level):
    check_against_oracle(random_gaussians(G, level, 100 * G + level), level, 'cpu')


@pytest.mark.parametrize('level', [0, 1])
def test_package_reproduces_the_reference_expectations_on_cpu(level):
    g = golden()
    voxels, merged = kal.ops.conversions.gs_to_voxelgrid(*(t(a) for a in reference_inputs()), level=level)
    assert torch.equal(voxels, t(g[f'voxels_{level}']))
    assert torch.allclose(merged, t(g[f'opacities_{level}']), **REF_TOL)


@pytest.mark.parametrize('step', [1, 2, 10])
def test_integrate_gs_cpu_within_one_ulp(step):
    check_integral(random_gaussians(64, 4, 5), 4, step, 'cpu')


def test_argument_checks():
    for call, what in bad_arguments('cpu'):
        with pytest.raises(RuntimeError):
            call()
            pytest.fail(f'{what}: no error')


def test_empty_cases():
    check_empty_cases('cpu')


def test_gaussian_outside_the_cube_yields_nothing():
    means, scales, rots, _ = random_gaussians(5, 3, 2)
    means[2] = (3.0, -4.0, 2.5)
    want, got = check_against_oracle((means, scales, rots, None), 3, 'cpu')
    ids = set(got[1].tolist())
    assert 2 not in ids and ids == {0, 1, 3, 4}


def test_scale_below_tol_is_clamped():
    level, vs = 3, 2.0 / 8
    tiny = centred_gaussians([[3, 4, 5]], level)
    want, got = check_against_oracle(tiny, level, 'cpu')
    assert got[0].tolist() == [[3, 4, 5]]
    clamped = (tiny[0], np.full((1, 3), TOL * vs, np.float32), tiny[2], tiny[3])
    assert torch.equal(got[3], check_against_oracle(clamped, level, 'cpu')[1][3])
    inv = 1.0 / (TOL * vs) ** 2
    assert np.allclose(got[3].numpy(), [[inv, 0, 0, inv, 0, inv]])


def test_opacities_with_a_trailing_dimension():
    means, scales, rots, opacities = (t(a) for a in random_gaussians(7, 3, 3))
    flat = kal.ops.conversions.gs_to_voxelgrid(means, scales, rots, opacities, 3)
    column = kal.ops.conversions.gs_to_voxelgrid(means, scales, rots, opacities[:, None], 3)
    assert flat[0].size(0) > 0 and torch.equal(flat[0], column[0]) and torch.equal(flat[1], column[1])


def test_merged_opacities_against_the_sequential_product_on_cpu():
    case = random_gaussians(64, 4, 7, voxels=(1.0, 2.0))
    voxels, merged = kal.ops.conversions.gs_to_voxelgrid(*(t(a) for a in case), 4)
    check_merged(case, 4, voxels, merged)


def check_merged(case, level, voxels, merged, step=10):
    """1 - prod(1 - integral) of every pack against the oracle's sequential float product, within (n + 2) 2^-24 for a pack of n"""
    means, scales, rots, opacities = case
    points, gid, boundary, cov = bf.gs_to_spc(means, scales, rots, ISO, TOL, level)
    integral = bf.integrate_gs(points, gid, means, cov, opacities, level, step).astype(np.float32)
    want = bf.merge(integral, boundary)
    starts = np.flatnonzero(boundary)
    n = np.diff(np.append(starts, len(boundary)))
    assert np.array_equal(voxels.cpu().numpy(), points[boundary])
    err = np.abs(merged.cpu().numpy().astype(np.float64) - want.astype(np.float64))
    share = (err / ((n + 2) * 2.0 ** -24)).max()
    print(f'merged opacities: {len(n)} packs, largest {n.max()}, worst share of the bound {share:.3f}')
    assert share <= 1.0
    return n


def test_reachable_through_install_as_kaolin():
    kaolin = kal.install_as_kaolin()
    import kaolin.ops.conversions as conversions
    assert conversions.gs_to_voxelgrid is kal.ops.conversions.gs_to_voxelgrid
    assert kaolin._C.ops.conversions.gs_to_spc_cuda is C.gs_to_spc_cuda
    assert kaolin._C.ops.conversions.integrate_gs_cuda is C.integrate_gs_cuda
