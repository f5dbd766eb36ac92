"""kaolin_amd.physics.collisions without a GPU: the torch formulation of the detection contract against the all-pairs numpy
oracle, bit for bit, and of the contact terms against float64 autograd of the reference test's analytic energy
(tests/collisions_bruteforce.py).  Every figure is printed before it is asserted (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

import collisions_bruteforce as bf
from kaolin_amd import _C
from kaolin_amd.physics import Collision, collisions

# what each case must contain for its rule to bite
BITES = {
    'n257': lambda col, total: total > 100,
    'one_cell': lambda col, total: total > 100,
    'exact': lambda col, total: total == 1,
    'duplicates': lambda col, total: (col.collision_normals == 0).all(dim=1).sum() == 2,
    'nan': lambda col, total: total > 10 and not {11, 30} & set(col.collision_indices_a.tolist() + col.collision_indices_b.tolist()),
    'immune': lambda col, total: 0 < (col.collision_indices_a % 2 == col.collision_indices_b % 2).sum() < total,
    'static': lambda col, total: (col.collision_indices_a == -1).any() and (col.collision_indices_b >= 20).all() and total > 3,
    'none': lambda col, total: total == 0 and col.object_pairs == [] and col.collision_normals.shape == (0, 3),
}




def kept(name, col):
    """Of the kept contacts of a case without static points: (cells of a (C, 3), cells of b, d (C)), and floor(pos / S) of every point"""
    dx, x0, *_ = bf.detection_case(name)
    pos, (_, S) = x0 + dx, bf.radii()
    a, b = col.collision_indices_a.cpu().numpy(), col.collision_indices_b.cpu().numpy()
    e = pos[a] - pos[b]
    return bf.cell(pos[a], S), bf.cell(pos[b], S), np.sqrt(bf._dot(e, e)), np.floor(pos / S)


def straddle_bites(col, total):
    ca, cb, d, _ = kept('straddle', col)
    apart = ca != cb
    print(f'straddle: {total} contacts, {apart.any(axis=1).sum()} across a face, {(d == bf.radii()[0]).sum()} at d == R')
    return apart.any(axis=1).sum() >= 20 and apart.any(axis=0).all() and (d == bf.radii()[0]).sum() >= 5 and (apart.sum(axis=1) >= 2).any()


def clamp_bites(name, col, total):
    ca, cb, _, q = kept(name, col)
    edge, end = (32767, 65535) if name == 'clamp_hi' else (-32768, 0)
    print(f'{name}: {total} contacts, {(ca != cb).any(axis=1).sum()} between different cells')
    return (q > edge).any(axis=0).all() and (q < edge).any(axis=0).all() and (np.concatenate([ca, cb]) == end).all(axis=1).any() and \
        total >= 30 and (ca != cb).any(axis=1).sum() >= 15


def huge_bites(col, total):
    dx, x0, obj, static, _ = bf.detection_case('huge')
    n = len(x0) - bf.HUGE
    alone = bf.detect(dx[:n], x0[:n], obj[:n], static[:n], 0.05)
    with np.errstate(over='ignore'):
        assert not np.isfinite((x0 + dx)[n:, None] - (x0 + dx)[None, n:]).all() and np.isfinite(x0 + dx).all()
    return total == alone[0] > 10 and np.array_equal(col.collision_indices_a.cpu().numpy(), alone[1]) and \
        np.array_equal(col.collision_indices_b.cpu().numpy(), alone[2])


BITES.update({
    'straddle': straddle_bites,
    'clamp_hi': functools.partial(clamp_bites, 'clamp_hi'),
    'clamp_lo': functools.partial(clamp_bites, 'clamp_lo'),
    'huge': huge_bites,
    'n4097': lambda col, total: 2 * 4097 < total < bf.ROOM['n4097'],                      # three sort blocks of 2048 keys, five scan blocks of 1024
    'n65537': lambda col, total: 65537 < total < bf.ROOM['n65537'] and col.collision_indices_b.max() >= 65536,
})


@pytest.mark.parametrize('name', bf.DETECTION_CASES)
def test_detection(name, caplog):
    col, total = bf.check_detection(name, 'cpu', caplog)
    assert BITES.get(name, lambda *_: True)(col, total)


@pytest.mark.parametrize('name', bf.EDGE_DETECTION_CASES)
def test_detection_edges(name, caplog):
    col, total = bf.check_detection(name, 'cpu', caplog, max_pairs=bf.ROOM.get(name, 10000))
    assert BITES[name](col, total)


@pytest.mark.parametrize('name', ['n257', 'nan', 'static', 'duplicates', 'n4097'])
def test_sweep_oracle_is_the_all_pairs_oracle(name):
    dx, x0, obj, static, kw = bf.detection_case(name)
    for max_pairs in (bf.ROOM.get(name, 10000), 37):
        want = bf.detect(dx, x0, obj, static, kw['collision_particle_radius'], max_pairs=max_pairs)
        got = bf.detect_sweep(dx, x0, obj, static, kw['collision_particle_radius'], max_pairs=max_pairs, block=64)
        assert want[0] == got[0] > 3 and all(np.array_equal(p, q, equal_nan=True) for p, q in zip(want[1:], got[1:]))


@pytest.mark.parametrize('label', bf.MAX_PAIRS_EDGES)
def test_detection_max_pairs_edges(label, caplog):
    """check_detection asserts the first min(T, max_pairs) pairs of the oracle, and the warning exactly when T > max_pairs"""
    max_pairs = bf.max_pairs_edge(label)
    col, total = bf.check_detection('n257', 'cpu', caplog, max_pairs=max_pairs)
    assert col.num_contacts == min(total, max_pairs)


def test_detection_overflow_keeps_the_smallest_pairs(caplog):
    assert bf.check_detection('n257', 'cpu', caplog, max_pairs=37)[1] > 37


def test_object_pairs_and_jacobian():
    """The static scene: object 0 static against object 1 -> the reference's four pairs; J against the LBS rows of the points"""
    dx, x0, obj, static, kw = bf.detection_case('static')
    col = Collision(dt=0.01, **kw)
    col.detect_collisions(*(torch.from_numpy(t) for t in (dx, x0, obj, static)))
    assert col.object_pairs.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]
    w, x = torch.rand(42, 3, dtype=torch.float64), torch.from_numpy(x0).double()
    col.calculate_jacobian(w, x)
    B = torch.einsum('ph,pn,bc->pbhcn', w, torch.cat([x, torch.ones(42, 1)], dim=1).double(), torch.eye(3).double()).reshape(42, 3, 36)
    rows = lambda i: torch.where((i >= 0)[:, None, None], B[i.long().clamp(min=0)], torch.zeros(1).double())
    assert torch.equal(col.collision_J_dense, (rows(col.collision_indices_a) - rows(col.collision_indices_b)).reshape(-1, 36))
    with pytest.raises(NotImplementedError):
        col.get_bounds(None, None, None)


@functools.lru_cache(maxsize=None)
def contacts():
    d = bf.synthetic(300, 50, 3, seed=5, static=True)
    return d, bf.terms64(d)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_terms_against_autograd(dtype):
    """float64: the formulation is the energy's derivative up to the limit form of the first regime; float32: within the
    yardstick's own limit, e_def < 1e-4, on the inputs the GPU test uses"""
    d, (G64, H64) = contacts()
    col, dx, w, x0 = bf.collision_of(d, dtype, 'cpu')
    E, G, Hs = col.energy(dx, x0, bf.COEFF), col.gradient(dx, x0, bf.COEFF), col.hessian(dx, x0, bf.COEFF)
    offset = collisions._contact_offsets(d['dx'], d['dx0'], d['gaps'], d['ia'], d['ib'])
    E64 = bf.energy64(offset, d['normals'], torch.where(d['ib'] < 0, 1.0, 2.0).double() * bf.RADIUS)
    assert E.shape == (1,) and G.shape == (300, 3) and Hs.shape == (300, 3, 3) and E.dtype == G.dtype == Hs.dtype == dtype
    bound = bf.LIMIT_FORM if dtype == torch.float64 else 1e-4
    for name, got, ref in (('energy', E, E64.sum().reshape(1)), ('gradient', G, G64), ('hessian', Hs, H64)):
        e = (got.double() - ref).abs().max().item() / ref.abs().max().item()
        print(f'{name} {dtype}: e {e:.3e}')
        assert e < bound
    inactive = E64 == 0
    assert inactive.sum() > 30 and (G[inactive] == 0).all() and (Hs[inactive] == 0).all() and (G[~inactive] != 0).any(dim=1).all()
    total = torch.ones(1, dtype=dtype)
    assert col.energy(dx, x0, bf.COEFF, energy=total) is total and torch.equal(total, 1 + E)


def test_reduced_terms_cpu():
    d, _ = contacts()
    col, dx, w, x0 = bf.collision_of(d, torch.float64, 'cpu')
    E, g, K = col.reduced_terms(dx, w, x0, bf.COEFF)
    col.calculate_jacobian(w, x0)
    J, G, Hs = col.collision_J_dense, col.gradient(dx, x0, bf.COEFF), col.hessian(dx, x0, bf.COEFF)
    assert torch.equal(E, col.energy(dx, x0, bf.COEFF)) and torch.allclose(g, J.T @ G.reshape(-1), rtol=1e-12, atol=0)
    assert torch.allclose(K, J.T @ torch.block_diag(*Hs) @ J, rtol=1e-10, atol=1e-12 * K.abs().max().item())
    E2, g2, K2 = col.reduced_terms(dx, w, x0, bf.COEFF, hessian=False)
    assert K2 is None and torch.equal(E2, E) and torch.equal(g2, g)
    col.num_contacts, col.collision_indices_a = 0, col.collision_indices_a[:0]
    assert [t.abs().sum().item() for t in col.reduced_terms(dx, w, x0, bf.COEFF)] == [0, 0, 0]


@pytest.mark.parametrize('H', [5, 33])
def test_elementwise_bound_bites(H):
    """The float32 definition is within the per-element bound of the reduction at the kernel's slicing; the float64 sums without
    one chunk of 32 contacts, and with the blocks (b, b') = (0, 1) and (1, 2) of K swapped, are not"""
    C = 129
    col, dx, w, x0 = bf.collision_of(bf.synthetic(C, 40, H, seed=100 * H + C), torch.float32, 'cpu')
    per = _C.physics.collision_slice_contacts(C, H)
    G, Hs, ia, ib = col.gradient(dx, x0, bf.COEFF), col.hessian(dx, x0, bf.COEFF), col.collision_indices_a, col.collision_indices_b
    _, g, K = col.reduced_terms(dx, w, x0, bf.COEFF)
    bf.check_reduced_elementwise(f'definition H={H}', g, K, G, Hs, w, x0, ia, ib, per, -(-C // per))
    g_ref, K_ref, T_g, T_K = bf.reduced_sums(G, Hs, w, x0, ia, ib)
    keep = torch.ones(C, 1)
    keep[32:64] = 0
    g_cut, K_cut, _, _ = bf.reduced_sums(G * keep, Hs * keep[:, :, None], w, x0, ia, ib)
    blocks = K_ref.reshape(H, 3, 4, H, 3, 4)                                      # H_c is symmetric up to rounding: not (1, 0) for (0, 1)
    K_swap = blocks.clone()
    K_swap[:, 0, :, :, 1], K_swap[:, 1, :, :, 2] = blocks[:, 1, :, :, 2], blocks[:, 0, :, :, 1]
    shares = [bf.bound_share(x, ref, T, per, -(-C // per)) for x, ref, T in ((g_cut, g_ref, T_g), (K_cut, K_ref, T_K), (K_swap.reshape(12 * H, 12 * H), K_ref, T_K))]
    print(f'H={H}: share of the bound without a chunk g {shares[0]:.1f} K {shares[1]:.1f}, with two blocks swapped K {shares[2]:.1f}')
    assert min(shares) > 1


def test_regime_edges_cpu():
    d, d_hat, vtn = bf.regime_edges()
    bf.check_regime_edges('torch float32', bf.edge_terms(d, torch.float32), d, d_hat, vtn)
    col, dx = bf.edge_collision(d, torch.float32, 'cpu')                          # the same contacts through the Collision's own path
    E, G, Hs = bf.edge_terms(d, torch.float32)
    assert torch.equal(col.gradient(dx, None, bf.COEFF), G) and torch.equal(col.hessian(dx, None, bf.COEFF), Hs)
    assert torch.equal(col.energy(dx, None, bf.COEFF), E.sum().reshape(1))
