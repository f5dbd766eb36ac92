"""What make_golden_tetmesh_metrics.py, test_tetmesh_metrics_cpu.py and test_tetmesh_metrics_gpu.py share: the rules that build
the inputs of tests/golden/tetmesh_metrics.npz, the sums of term magnitudes that bound rounding error, and the comparisons.

Inputs are rebuilt from rules and from marching_tetrahedra.npz; the file holds the reference's float64 answers, how far its own
float32 answers are from them (``*_ref32_dev`` = ref32 - ref64) and the term-magnitude sums (``*_tas``).  Gradients with respect
to ``tet_vertices`` are recorded where a user reads them: gathered onto the mesh's vertices through ``vertices[:, tets]`` --
(B, V, 3) instead of (B, T, 4, 3), which is what keeps the file below the size of the largest golden.
"""
import os

import numpy as np
import torch

from kaolin_amd.utils.testing import elementwise_mismatch, kuhn_grid

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
DTYPES = [('f32', torch.float32), ('f64', torch.float64)]
TOL = {'f32': 1e-5, 'f64': 2e-14}          # the north star's 1e-5 for float32; the same multiple (~84) of eps for float64
EQUI_POWS = (1, 2, 4)
GIVEN_MEAN = 1e-4                          # the one-element mean of the `equi_given` case (a float32 value after rounding)
_CACHE = {}


def golden():
    if 'g' not in _CACHE:
        _CACHE['g'] = np.load(os.path.join(GOLDEN_DIR, 'tetmesh_metrics.npz'))
    return _CACHE['g']


def tensor(name):
    return torch.from_numpy(golden()[name])


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def grid9():
    """-> vertices (2, 1000, 3) float32 (item 0 jittered, item 1 the plain kuhn_grid(9)), tets (4444, 4): permuted corners (both
    signs of volume), 50 duplicates, 20 tets with a repeated corner (zero volume)"""
    if 'grid9' not in _CACHE:
        mt = np.load(os.path.join(GOLDEN_DIR, 'marching_tetrahedra.npz'))
        vertices = torch.stack([torch.from_numpy(mt['grid9_vertices'])[0], kuhn_grid(9)[0]])
        _CACHE['grid9'] = (vertices, torch.from_numpy(mt['grid9_tets']))
    return _CACHE['grid9']


def amips_tet_vertices(vertices, tets, zero_rows=True):
    """vertices (B, V, 3) -> tet_vertices (B, T, 4, 3) of the amips case: every 7th tet has corners 2 and 3 swapped (det ~ -1,
    masked out); with `zero_rows`, every 11th tet has corner 1, 2 or 3 (cycling) equal to corner 0 (a zero row of J: det is
    exactly +-0 in any arithmetic, mask 1).  Differentiable in `vertices`."""
    T = tets.shape[0]
    t = torch.arange(T, device=tets.device)
    corner = torch.arange(4, device=tets.device).repeat(T, 1)
    swap = t % 7 == 0
    corner[swap, 2], corner[swap, 3] = 3, 2
    if zero_rows:
        rows = t[t % 11 == 0]
        corner[rows, 1 + (rows // 11) % 3] = 0
    return vertices[:, torch.gather(tets, 1, corner)]


def zero_row_tets(T):
    return torch.arange(T) % 11 == 0


# ---- sums of term magnitudes (float64) ------------------------------------------------------------------------------------------------
def _abs_cross(b, c):
    b, c = b.abs(), c.abs()
    return torch.stack([b[..., 1] * c[..., 2] + b[..., 2] * c[..., 1], b[..., 2] * c[..., 0] + b[..., 0] * c[..., 2],
                        b[..., 0] * c[..., 1] + b[..., 1] * c[..., 0]], dim=-1)


def volume_terms(tet_vertices):
    """(B, T): the six products of a volume, in magnitude, over 6"""
    x = tet_vertices.double()
    a, b, c = x[:, :, 0] - x[:, :, 3], x[:, :, 1] - x[:, :, 3], x[:, :, 2] - x[:, :, 3]
    return (a.abs() * _abs_cross(b, c)).sum(-1) / 6


def volume_grad_terms(tet_vertices, g):
    """(B, T, 4, 3): per entry of the gradient of sum(g * volume), its products times |g| / 6 (corner D adds its three)"""
    x = tet_vertices.double()
    a, b, c = x[:, :, 0] - x[:, :, 3], x[:, :, 1] - x[:, :, 3], x[:, :, 2] - x[:, :, 3]
    s = (g.double().abs() / 6).unsqueeze(-1)
    da, db, dc = s * _abs_cross(b, c), s * _abs_cross(c, a), s * _abs_cross(a, b)
    return torch.stack([da, db, dc, da + db + dc], dim=2)


def equivolume_grad_terms(tet_vertices, mean, power, mean_computed):
    """(B, T, 4, 3) for grad_loss = 1: the volume's terms under |g_t| = p |v - m|^(p-1) / T, plus (mean computed) the branch
    through the mean, whose cotangent is bounded by sum_t |g_t| / T per tet; and that sum itself (the terms of grad mean)"""
    x = tet_vertices.double()
    T = x.shape[1]
    v = ((x[:, :, 0] - x[:, :, 3]) * torch.cross(x[:, :, 1] - x[:, :, 3], x[:, :, 2] - x[:, :, 3], dim=-1)).sum(-1) / 6
    d = v - mean.double().reshape(1, -1)
    g = power * d.abs() ** (power - 1) / T * (d != 0)
    total = g.sum(dim=-1, keepdim=True)
    if mean_computed:
        g = g + total / T
    return volume_grad_terms(x, g), total.sum()


def amips_grad_terms(tet_vertices, inv):
    """-> (B, T, 4, 3), (B, T, 3, 3) for grad_loss = 1: the magnitudes of the terms of dE/dJ = (2 J / den - kc cof) / T carried
    through dO = G M^T (corner A adds its three rows) and dM = O^T G"""
    x, m = tet_vertices.double(), inv.double().expand(tet_vertices.shape[0], -1, -1, -1)
    T = x.shape[1]
    o = x[:, :, 1:] - x[:, :, :1]
    j = o @ m
    j_abs = o.abs() @ m.abs()
    det = torch.det(j)
    tr = (j * j).sum((-1, -2))
    q = det * det + 1e-10
    den = q ** (1 / 3)
    kc = ((2 / 3) * tr * det / (den * q)).abs()[..., None, None]
    r = lambda i: ((i + 1) % 3, (i + 2) % 3)                                                   # noqa: E731
    cof_abs = torch.stack([torch.stack([j_abs[..., r(a)[0], r(b)[0]] * j_abs[..., r(a)[1], r(b)[1]] +
                                        j_abs[..., r(a)[0], r(b)[1]] * j_abs[..., r(a)[1], r(b)[0]] for b in range(3)], -1)
                           for a in range(3)], -2)
    g = (2 / den[..., None, None] * j_abs + kc * cof_abs) / T * (det >= 0)[..., None, None]
    d_o = g @ m.abs().transpose(-1, -2)
    return torch.cat([d_o.sum(2, keepdim=True), d_o], dim=2), o.abs().transpose(-1, -2) @ g


def to_vertices(per_corner, tets, num_vertices):
    """(B, T, 4, 3) -> (B, V, 3): what index_put accumulates through ``vertices[:, tets]``"""
    out = torch.zeros(per_corner.shape[0], num_vertices, 3, dtype=per_corner.dtype)
    return out.index_add_(1, tets.reshape(-1), per_corner.reshape(per_corner.shape[0], -1, 3))


# ---- comparisons ----------------------------------------------------------------------------------------------------------------------
WORST = {}          # name -> the largest fraction of a bound any comparison of this process has used (printed by the tests)


def check_elements(name, got, tag, ref64, tas):
    """Per-element results against the reference's float64 record: elementwise_mismatch with the recorded term sums."""
    msg = elementwise_mismatch(got, ref64.to(got.dtype) if tag == 'f64' else ref64, tol=TOL[tag], term_abs_sum=tas)
    a, b = got.detach().double().cpu(), ref64.double()
    nz = b[b != 0].abs()
    floor = float(nz.median()) if nz.numel() else 0.0
    eps = float(torch.finfo(got.dtype).eps)
    bound = TOL[tag] * b.abs() + TOL[tag] * floor + 64.0 * eps * tas.double()
    ratio = float(((a - b).abs() / bound.clamp(min=1e-300)).max()) if a.numel() else 0.0
    WORST[f'{name}_{tag}'] = max(WORST.get(f'{name}_{tag}', 0.0), ratio)
    print(f'{name} {tag}: worst |a-b| / bound = {ratio:.3f}; slack use {elementwise_mismatch.last_slack_use}')
    assert msg is None, f'{name} {tag}: {msg}'


def check_scalars(name, got, tag, ref64, ref32_dev, terms_over_t):
    """Losses: |got - ref64| <= max(4 |ref32 - ref64|, 64 eps sum|terms| / T), element by element."""
    eps = float(torch.finfo(got.dtype).eps)
    a, b = got.detach().double().cpu(), ref64.double()
    assert a.shape == b.shape, (name, a.shape, b.shape)
    floor = 64.0 * eps * terms_over_t.double()
    bound = torch.maximum(4.0 * ref32_dev.double().abs(), floor) if tag == 'f32' else floor
    ratio = float(((a - b).abs() / bound.clamp(min=1e-300)).max())
    WORST[f'{name}_{tag}'] = max(WORST.get(f'{name}_{tag}', 0.0), ratio)
    print(f'{name} {tag}: got {a.reshape(-1).tolist()} ref64 {b.reshape(-1).tolist()} |a-b| / bound = {ratio:.3f}')
    assert bool(((a - b).abs() <= bound).all()), f'{name} {tag}: {ratio:.3f}x the bound'


# ---- the recorded cases, run through the public functions on `device` (both test files) ----------------------------------------------
def leaf(x, device, dtype):
    return x.detach().clone().to(device, dtype).requires_grad_()


def records_volume(device, tag, dtype):
    from kaolin_amd.metrics.tetmesh import tetrahedron_volume
    gv, gt = grid9()
    p = leaf(gv, device, dtype)
    volumes = tetrahedron_volume(p[:, gt.to(device)])
    assert volumes.shape == (2, gt.shape[0]) and volumes.dtype == dtype
    (volumes * tensor('vol_grid9_cot').to(device, dtype)).sum().backward()
    check_elements('vol_grid9', volumes, tag, tensor('vol_grid9_f64'), tensor('vol_grid9_tas'))
    check_elements('vol_grid9_grad', p.grad, tag, tensor('vol_grid9_grad_f64'), tensor('vol_grid9_grad_tas'))


def records_equivolume(device, tag, dtype):
    from kaolin_amd.metrics.tetmesh import equivolume
    gv, gt = grid9()
    for b in range(2):
        for power in EQUI_POWS:
            name = f'equi_item{b}_pow{power}'
            p = leaf(gv[b:b + 1], device, dtype)
            loss = equivolume(p[:, gt.to(device)], pow=power)
            assert loss.shape == (1, 1) and loss.dtype == dtype
            loss.sum().backward()
            check_scalars(f'{name}_loss', loss, tag, tensor(f'{name}_loss_f64'), tensor(f'{name}_loss_ref32_dev'), tensor(f'{name}_loss_f64'))
            check_elements(f'{name}_grad', p.grad, tag, tensor(f'{name}_grad_f64'), tensor(f'{name}_grad_tas'))
    p, m = leaf(gv, device, dtype), leaf(torch.tensor([GIVEN_MEAN]), device, dtype)
    loss = equivolume(p[:, gt.to(device)], m, pow=4)
    assert loss.shape == (2, 1)
    loss.sum().backward()
    check_scalars('equi_given_loss', loss, tag, tensor('equi_given_loss_f64'), tensor('equi_given_loss_ref32_dev'), tensor('equi_given_loss_f64'))
    check_elements('equi_given_grad', p.grad, tag, tensor('equi_given_grad_f64'), tensor('equi_given_grad_tas'))
    check_elements('equi_given_grad_mean', m.grad, tag, tensor('equi_given_grad_mean_f64'), tensor('equi_given_grad_mean_tas'))


def records_amips(device, tag, dtype):
    from kaolin_amd.metrics.tetmesh import amips
    tets = kuhn_grid(6)[1]
    av, inv = tensor('amips_vertices'), tensor(f'amips_inv_{tag}')
    assert inv.shape == (1, tets.shape[0], 3, 3)                     # a batch of one against B = 2
    loss = amips(amips_tet_vertices(av.to(device, dtype), tets.to(device)), inv.to(device))
    assert loss.shape == (2, 1) and loss.dtype == dtype
    check_scalars('amips_loss', loss, tag, tensor('amips_loss_f64'), tensor('amips_loss_ref32_dev'), tensor('amips_loss_f64'))
    p, m = leaf(av, device, dtype), leaf(inv, device, dtype)
    loss = amips(amips_tet_vertices(p, tets.to(device), zero_rows=False), m)
    loss.sum().backward()
    check_scalars('amips_grad_loss', loss, tag, tensor('amips_grad_loss_f64'), tensor('amips_grad_loss_ref32_dev'), tensor('amips_grad_loss_f64'))
    check_elements('amips_grad_vertices', p.grad, tag, tensor('amips_grad_vertices_f64'), tensor('amips_grad_vertices_tas'))
    check_elements('amips_grad_inv', m.grad, tag, tensor('amips_grad_inv_f64'), tensor('amips_grad_inv_tas'))


def known_answers(device, tag, dtype):
    """The reference's docstring / unit-test inputs: what it RETURNS is pinned (for equivolume its own test expects other numbers)"""
    from kaolin_amd.metrics import tetmesh
    g = golden()
    for fn in ('tetrahedron_volume', 'equivolume', 'amips'):
        args = [torch.from_numpy(g[f'kat_{fn}_in{k}']).to(device, dtype) for k in range(2 if fn == 'amips' else 1)]
        got = getattr(tetmesh, fn)(*args, **({'pow': 4} if fn == 'equivolume' else {}))
        ret32, ret64 = tensor(f'kat_{fn}_ret_f32').double(), tensor(f'kat_{fn}_ret_f64')
        assert got.shape == ret64.shape and got.dtype == dtype
        # The bound is the reference's own conditioning: 4 x how far its float32 answer is from its float64 answer (the amips
        # example is ill-conditioned: 2e-3), in float64 scaled by the ratio of the two eps; never below 64 eps |answer|.
        eps = float(torch.finfo(dtype).eps)
        bound = torch.maximum(4 * (ret32 - ret64).abs() * (eps / float(torch.finfo(torch.float32).eps)), 64 * eps * ret64.abs())
        ratio = float(((got.detach().cpu().double() - ret64).abs() / bound).max())
        print(f'kat_{fn} {tag}: |got - ret64| / bound = {ratio:.3f}')
        assert ratio <= 1, (fn, tag, ratio)
    assert not np.allclose(g['kat_equivolume_ret_f32'], g['kat_equivolume_expected'], rtol=1e-2, atol=0)


def jittered_grid(n, batch, dtype, seed=3, jitter=0.1):
    """-> vertices (batch, V, 3), tets: kuhn_grid(n) with every vertex moved by up to jitter / 2 / n"""
    vertices, tets = kuhn_grid(n, dtype=dtype)
    g = torch.Generator().manual_seed(seed)
    return vertices[None] + (torch.rand((batch,) + vertices.shape, generator=g, dtype=dtype) - 0.5) * (jitter / n), tets
