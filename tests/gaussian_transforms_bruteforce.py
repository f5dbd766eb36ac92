"""Oracles for ops.gaussians.transform_gaussians / transform_shs, numpy only.

1. ``projection_matrices``: the SH rotation matrices WITHOUT the recurrence.  B(d) = the 16 real-SH polynomials of a direction in
   the 3DGS sign convention; rotated coefficients c' must satisfy B(d) c' = B(R^T d) c for every d, so D = lstsq(B(dirs),
   B(dirs @ R)) over 200 fixed unit directions (16 unknowns a column, rank 16: exact to ~3e-15 in float64).
2. ``reference``: the whole operator in extended precision (np.longdouble), following the generated term lists
   (kaolin_amd/ops/gaussians/_sh_rotation_table.py), with, per output element, the SUM OF TERM MAGNITUDES that the rounding bound
   multiplies (the same expression on absolute values).
3. The rounding counts n of csrc/gaussian_transform.hip (DESIGN.md derives them) and ``check_share``:
       |got - want| <= gamma_n * magnitude + u * |want|,   gamma_n = n u / (1 - n u),  u = 2^-24 (float32) / 2^-53 (float64)
   The share is the left side over the right; a test fails above 1 and prints the worst.
"""
import numpy as np

from kaolin_amd.ops.gaussians import _sh_rotation_table as table

LD = np.longdouble
UNIT = {'float32': 2.0 ** -24, 'float64': 2.0 ** -53}

# ---- the rounding counts (first order, relative to the term magnitudes) -----------------------------------------------------------
E_R = 4            # an entry of R = A / column norm: (3 in the squared norm, halved by the root) + 1 root + 1 division, rounded up
N_D2 = 1 + 2 + 2 * E_R + (table.BAND2_MAX_TERMS_PER_ELEMENT - 1)              # c, two products, two entries of D^1, the additions
N_D3 = 1 + 2 + E_R + N_D2 + (table.BAND3_MAX_TERMS_PER_ELEMENT - 1)
N_SH = N_D3 + 1 + 6                                                           # the product with the coefficient, 6 additions
N_POSITIONS = 4                                                               # a product and three additions
N_SCALES = 4                                                                  # the norm (2.5) and a product; log scales: see below
N_ORIENTATIONS = 32                                                           # 28 to first order, rounded up
N_GRAD_POSITIONS = 3
N_GRAD_ORIENTATIONS = 42


def gamma(n, u):
    return n * u / (1 - n * u)


# ---- the projection oracle ----------------------------------------------------------------------------------------------------------
def sh_basis(dirs):
    """dirs (n, 3) unit -> (n, 16): the real SH polynomials, bands 0..3, 3DGS signs"""
    x, y, z = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    c0, c1 = 0.28209479177387814, 0.4886025119029199
    c2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
    c3 = (-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
          -0.5900435899266435)
    return np.stack([
        c0 * np.ones_like(x), -c1 * y, c1 * z, -c1 * x,
        c2[0] * xy, c2[1] * yz, c2[2] * (2 * zz - xx - yy), c2[3] * xz, c2[4] * (xx - yy),
        c3[0] * y * (3 * xx - yy), c3[1] * xy * z, c3[2] * y * (4 * zz - xx - yy), c3[3] * z * (2 * zz - 3 * xx - 3 * yy),
        c3[4] * x * (4 * zz - xx - yy), c3[5] * z * (xx - yy), c3[6] * x * (xx - 3 * yy)], axis=1)


def fixed_directions(n=200):
    d = np.random.default_rng(20260101).standard_normal((n, 3))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def projection_matrices(R):
    """R (3, 3) float64 -> (D (16, 16), fit residual): B(dirs) D = B(dirs @ R) in the least-squares sense"""
    dirs = fixed_directions()
    B = sh_basis(dirs)
    target = sh_basis(dirs @ R)
    D = np.linalg.lstsq(B, target, rcond=None)[0]
    return D, np.abs(B @ D - target).max()


def projection_transform_shs(sh, R):
    """sh (n, S, 3), R (n or 1, 3, 3) float64 -> rotated coefficients through the projection oracle"""
    out = np.empty_like(sh)
    S = sh.shape[1]
    for k in range(sh.shape[0]):
        D = projection_matrices(R[k if R.shape[0] > 1 else 0])[0]
        out[k] = D[:S, :S] @ sh[k]
    return out


# ---- the recurrence, in extended precision, with magnitudes ----------------------------------------------------------------------------
def recurrence_matrices(R, degree):
    """R (n, 3, 3) -> ([D^1..D^degree], [the same on absolute values]), longdouble"""
    R = np.asarray(R, dtype=LD)
    perm = [1, 2, 0]
    sign = np.array([[1, -1, 1], [-1, 1, -1], [1, -1, 1]], dtype=LD)
    mats, mags = [], []
    if degree >= 1:
        mats.append(R[:, perm][:, :, perm] * sign)
        mags.append(np.abs(mats[0]))
    for l in range(2, degree + 1):
        d = 2 * l + 1
        D, M = np.zeros((R.shape[0], d, d), dtype=LD), np.zeros((R.shape[0], d, d), dtype=LD)
        for c, m, n, i, j, p, q in table.BANDS[l]:
            D[:, m, n] += (LD(c) * mats[0][:, i, j]) * mats[-1][:, p, q]
            M[:, m, n] += (LD(abs(c)) * mags[0][:, i, j]) * mags[-1][:, p, q]
        mats.append(D)
        mags.append(M)
    return mats, mags


def reference_shs(sh, R, transposed=False):
    """sh (n, S, 3), R (n or 1, 3, 3) -> (rotated coefficients, magnitudes), longdouble.  transposed: D^T (the backward)"""
    sh = np.asarray(sh, dtype=LD)
    degree = int(round(np.sqrt(sh.shape[1]))) - 1
    mats, mags = recurrence_matrices(R, degree)
    out, mag = sh.copy(), np.abs(sh)
    for l, (D, M) in enumerate(zip(mats, mags), start=1):
        if transposed:
            D, M = D.transpose(0, 2, 1), M.transpose(0, 2, 1)
        band = slice(l * l, (l + 1) * (l + 1))
        out[:, band] = D @ sh[:, band]
        mag[:, band] = M @ np.abs(sh[:, band])
    return out, mag


def decompose(transform):
    """transform (n, 4, 4) -> A, t, column norms, R = A / norms; longdouble"""
    T = np.asarray(transform, dtype=LD)
    A, t = T[:, :3, :3], T[:, :3, 3]
    norms = np.sqrt((A * A).sum(axis=1))
    return A, t, norms, A / norms[:, None, :]


def quat_from_rot33(R):
    """(n, 3, 3) -> ((n, 4) xyzw by the branch rule, branch 0..3, the smallest margin of the comparisons that chose it)"""
    R = np.asarray(R, dtype=LD)
    out = np.empty((R.shape[0], 4), dtype=LD)
    branch = np.empty(R.shape[0], dtype=np.int64)
    margin = np.empty(R.shape[0], dtype=np.float64)
    for k, m in enumerate(R):
        tr = m[0, 0] + m[1, 1] + m[2, 2]
        margins = [abs(tr)]
        if tr > 0:
            s = LD(0.5) / np.sqrt(tr + 1)
            q, b = [(m[2, 1] - m[1, 2]) * s, (m[0, 2] - m[2, 0]) * s, (m[1, 0] - m[0, 1]) * s, LD(0.25) / s], 0
        else:
            d1, d2 = m[0, 0] - m[1, 1], m[0, 0] - m[2, 2]
            if d1 > 0 and d2 > 0:
                margins.append(min(d1, d2))
                s = 2 * np.sqrt(1 + m[0, 0] - m[1, 1] - m[2, 2])
                q, b = [s / 4, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s, (m[2, 1] - m[1, 2]) / s], 1
            else:
                margins.append(max(-d for d in (d1, d2) if not d > 0))       # every failing comparison would have to flip
                margins.append(abs(m[1, 1] - m[2, 2]))
                if m[1, 1] > m[2, 2]:
                    s = 2 * np.sqrt(1 + m[1, 1] - m[0, 0] - m[2, 2])
                    q, b = [(m[0, 1] + m[1, 0]) / s, s / 4, (m[1, 2] + m[2, 1]) / s, (m[0, 2] - m[2, 0]) / s], 2
                else:
                    s = 2 * np.sqrt(1 + m[2, 2] - m[0, 0] - m[1, 1])
                    q, b = [(m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, s / 4, (m[1, 0] - m[0, 1]) / s], 3
        out[k], branch[k], margin[k] = q, b, float(min(margins))
    return out, branch, margin


def quat_mul(a, b):
    ax, ay, az, aw = (a[..., k] for k in range(4))
    bx, by, bz, bw = (b[..., k] for k in range(4))
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], axis=-1)


def reference(positions, orientations, scales, transform, sh=None, use_log_scales=False, use_xyzw=False, min_margin=None):
    """The operator in longdouble -> {name: (want, magnitude)} for positions, orientations, scales and (sh given) sh_coeff, plus
    'branch' (n) and 'margin' (n) of quat(R).  transform (n or 1, 4, 4).  min_margin: assert every branch margin above it."""
    n = positions.shape[0]
    A, t, norms, R = decompose(transform)
    p, q, s = (np.asarray(x, dtype=LD) for x in (positions, orientations, scales))
    out = {'positions': ((A @ p[:, :, None])[:, :, 0] + t, (np.abs(A) @ np.abs(p)[:, :, None])[:, :, 0] + np.abs(t))}
    r, branch, margin = quat_from_rot33(R)
    if min_margin is not None:
        assert margin.min() > min_margin, f'a branch of quat(R) is decided by {margin.min():.2e}'
    u = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    if not use_xyzw:
        u = np.concatenate([u[:, 1:], u[:, :1]], axis=1)
    o = quat_mul(r, u)
    if not use_xyzw:
        o = np.concatenate([o[:, -1:], o[:, :-1]], axis=1)
    out['orientations'] = (np.broadcast_to(o, (n, 4)), np.broadcast_to(np.abs(u).sum(axis=1, keepdims=True), (n, 4)))
    if use_log_scales:
        L = np.log(norms)
        out['scales'] = (s * (L / s + 1), 1 + np.abs(L) + np.abs(s))
    else:
        out['scales'] = (s * norms, np.abs(s * norms))
    if sh is not None:
        out['sh_coeff'] = reference_shs(sh, R)
    out['branch'], out['margin'] = branch, margin
    return out


def grad_magnitudes(cotangents, orientations, scales, transform, use_log_scales=False, use_xyzw=False):
    """The sums of term magnitudes of the backward for the cotangents {name: array} of the forward's outputs -> {name: magnitude}
    (positions: |A|^T |g|; scales: |g s|; sh_coeff: |D|^T |g|; orientations: sum|G| (1 + |u_k| sum|u|) / |q|).  Log scales: the
    kernel returns g itself (exact); the magnitude |g| (1 + 2 |log(s) / scales|) is that of the AUTOGRAD REFERENCE, which
    differentiates scales * (log(s) / scales + 1) literally and so evaluates (log(s) / scales + 1) - log(s) / scales with its own
    rounding (in a float64 run that is the reference's error, not the kernel's)."""
    A, _, norms, R = decompose(transform)
    out = {}
    if 'positions' in cotangents:
        out['positions'] = (np.abs(A).transpose(0, 2, 1) @ np.abs(np.asarray(cotangents['positions'], dtype=LD))[:, :, None])[:, :, 0]
    if 'scales' in cotangents:
        g = np.abs(np.asarray(cotangents['scales'], dtype=LD))
        out['scales'] = g * (1 + 2 * np.abs(np.log(norms) / np.asarray(scales, dtype=LD))) if use_log_scales else g * norms
    if 'sh_coeff' in cotangents:
        out['sh_coeff'] = reference_shs(cotangents['sh_coeff'], R, transposed=True)[1]
    if 'orientations' in cotangents:
        q = np.asarray(orientations, dtype=LD)
        nq = np.sqrt((q * q).sum(axis=1, keepdims=True))
        u = np.abs(q / nq)
        G = np.abs(np.asarray(cotangents['orientations'], dtype=LD)).sum(axis=1, keepdims=True)
        out['orientations'] = G * (1 + u * u.sum(axis=1, keepdims=True)) / nq
    return out


GRAD_COUNTS = {'positions': N_GRAD_POSITIONS, 'orientations': N_GRAD_ORIENTATIONS, 'scales': N_SCALES, 'sh_coeff': N_SH}
# the GPU tests' cases (tests/test_gaussian_transforms_gpu.py): the sizes of the per-Gaussian ones (seed 100 + n) and the branches of
# quat(R) of the shared ones (seed 200 + branch); test_gaussian_transforms_cpu.py checks the branch condition for these seeds
GPU_SIZES = (1, 63, 64, 65, 127, 129, 257)
GPU_SHARED_BRANCHES = (0, 1, 2, 3)
MIN_MARGIN = 1e-3      # every comparison of quat(R)'s branch rule is decided by more than this in the cases below


def _rotation(rng):
    q, r = np.linalg.qr(rng.standard_normal((3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def rotations_with_margin(n, rng, branch=None):
    """n proper rotations whose quat(R) branch is decided by more than 2 MIN_MARGIN (so that float32 rounding of the matrix cannot
    change it); branch: only rotations of that branch"""
    out = []
    while len(out) < n:
        R = _rotation(rng)
        _, b, margin = quat_from_rot33(R[None])
        if margin[0] > 2 * MIN_MARGIN and (branch is None or b[0] == branch):
            out.append(R)
    return np.stack(out)


def make_case(n, degree, per_gaussian, seed, branch=None):
    """-> dict of float64 arrays holding float32 values: positions (n, 3), orientations (n, 4, not normalized), scales (n, 3) in
    [0.2, 2], transform (n or 1, 4, 4) = uniform scale in [0.5, 2] x rotation + translation, sh_coeff (n, (degree + 1)^2, 3) or
    None (degree None).  Shared transforms take the branch of quat(R) that `branch` names."""
    rng = np.random.default_rng(seed)
    m = n if per_gaussian else 1
    tf = np.zeros((m, 4, 4))
    tf[:, :3, :3] = rotations_with_margin(m, rng, branch) * rng.uniform(0.5, 2.0, (m, 1, 1))
    tf[:, :3, 3] = rng.uniform(-3, 3, (m, 3))
    tf[:, 3, 3] = 1
    case = {'positions': rng.uniform(-2, 2, (n, 3)), 'orientations': rng.standard_normal((n, 4)) * rng.uniform(0.5, 2, (n, 1)),
            'scales': rng.uniform(0.2, 2.0, (n, 3)), 'transform': tf,
            'sh_coeff': None if degree is None else rng.standard_normal((n, (degree + 1) ** 2, 3))}
    return {k: None if v is None else v.astype(np.float32).astype(np.float64) for k, v in case.items()}


def half_cotangents(shape, rng):
    """cotangents of exact halves in [-2, 2]"""
    return rng.integers(-4, 5, shape).astype(np.float64) / 2


COUNTS = {'positions': N_POSITIONS, 'orientations': N_ORIENTATIONS, 'scales': N_SCALES, 'sh_coeff': N_SH}


def share(got, want, magnitude, n, dtype_name):
    """-> the largest |got - want| / (gamma_n magnitude + u |want|) over the elements (0 for no element); NaN counts as inf"""
    u = UNIT[dtype_name]
    got = np.asarray(got, dtype=LD)
    want, magnitude = np.broadcast_to(np.asarray(want, dtype=LD), got.shape), np.broadcast_to(np.asarray(magnitude, dtype=LD), got.shape)
    if got.size == 0:
        return 0.0
    bound = gamma(n, u) * magnitude + u * np.abs(want)
    err = np.abs(got - want)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        ratio = np.where(err == 0, 0, err / np.where(bound == 0, np.finfo(LD).tiny, bound))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    return float(ratio.max())


def check_share(name, got, want, magnitude, n, dtype_name, limit=1.0):
    worst = share(got, want, magnitude, n, dtype_name)
    print(f'share {name} {dtype_name} n={n}: {worst:.4f}')
    assert worst <= limit, f'{name} ({dtype_name}): worst share {worst:.4f} of the bound gamma_{n} * magnitude + u |want|'
    return worst
