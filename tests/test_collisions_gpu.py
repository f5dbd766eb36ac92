"""kaolin_amd.physics.collisions on the GPU (csrc/collisions.hip, float32): detection against the all-pairs numpy oracle, bit for
bit; the contact terms against float64 autograd of the analytic energy; the reduced terms against the float64 definition
through collision_J_dense.  The measure and the yardstick are those of tests/test_physics_gpu.py (collisions_bruteforce.check):
e = max|X - X64| / max|X64|, e_hip <= 4 max(e_def, 2^-24) and e_def < 1e-4, where e_def is the float32 torch formulation (the
vectorised terms, the dense J), not the code under test.  Every figure is printed before it is asserted (pytest -s)."""
import functools

import pytest
import torch

import collisions_bruteforce as bf
from kaolin_amd import _C
from kaolin_amd.physics import collisions
from test_collisions_cpu import BITES, contacts

pytestmark = pytest.mark.gpu

CC = _C.physics.collision_chunk_contacts()
H_EDGES = (1, 4, 5, 17)   # 4 H: under one MFMA block, exactly one, a ragged one, two tiles with a ragged one (a diagonal and an off-diagonal tile)
SLICE = {H: _C.physics.collision_slice_contacts(CC, H) for H in H_EDGES}
EDGES = [(C, H) for H in (5, 17) for C in (CC - 1, CC, CC + 1, SLICE[H] - 1, SLICE[H], SLICE[H] + 1)]
EDGES += [(C, H) for H in (1, 4) for C in (CC + 1, SLICE[H] + 1)]


@pytest.mark.parametrize('name', bf.DETECTION_CASES)
def test_detection(name, caplog):
    col, total = bf.check_detection(name, 'cuda', caplog)
    assert BITES.get(name, lambda *_: True)(col, total)
    if name == 'static':
        assert col.object_pairs.tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]


def test_detection_overflow_keeps_the_smallest_pairs(caplog):
    assert bf.check_detection('n257', 'cuda', caplog, max_pairs=37)[1] > 37


def test_terms():
    """300 contacts (two workgroups), the three regimes, inactive contacts, static sides a and b"""
    d, (G64, H64) = contacts()
    col, dx, w, x0 = bf.collision_of(d, torch.float32, 'cuda')
    ref, dx32, _, x032 = bf.collision_of(d, torch.float32, 'cpu')
    E64 = bf.energy64(collisions._contact_offsets(d['dx'], d['dx0'], d['gaps'], d['ia'], d['ib']), d['normals'],
                      torch.where(d['ib'] < 0, 1.0, 2.0).double() * bf.RADIUS).sum().reshape(1)
    E, G, Hs = col.energy(dx, x0, bf.COEFF), col.gradient(dx, x0, bf.COEFF), col.hessian(dx, x0, bf.COEFF)
    assert E.shape == (1,) and G.shape == (300, 3) and Hs.shape == (300, 3, 3)
    bf.check('energy', E, ref.energy(dx32, x032, bf.COEFF), E64)
    bf.check('gradient', G, ref.gradient(dx32, x032, bf.COEFF), G64)
    bf.check('hessian', Hs, ref.hessian(dx32, x032, bf.COEFF), H64)
    inactive = (G64 == 0).all(dim=1).cuda()
    assert inactive.sum() > 30 and (G[inactive] == 0).all() and (Hs[inactive] == 0).all()
    assert all(torch.equal(a, b) for a, b in zip((E, G, Hs), (col.energy(dx, x0, bf.COEFF), col.gradient(dx, x0, bf.COEFF), col.hessian(dx, x0, bf.COEFF))))
    total = torch.ones(1, device='cuda')
    assert col.energy(dx, x0, bf.COEFF, energy=total) is total and torch.equal(total, 1 + E)


@functools.lru_cache(maxsize=None)
def case(C, H, static=False):
    assert _C.physics.collision_slice_contacts(C, H) == SLICE[H]
    d = bf.synthetic(C, 40, H, seed=100 * H + C, static=static)
    return bf.collision_of(d, torch.float64, 'cuda'), bf.collision_of(d, torch.float32, 'cuda')


def check_reduced(C, H, static=False):
    (col64, *args64), (col, dx, w, x0) = case(C, H, static)
    ref = col64.reduced_terms(*args64, bf.COEFF)
    definition = col._reduced_dense(col._contact_tensors(dx), w, x0, bf.COEFF, True)
    hip = col.reduced_terms(dx, w, x0, bf.COEFF)
    assert hip[0].shape == (1,) and hip[1].shape == (12 * H,) and hip[2].shape == (12 * H, 12 * H)
    for name, h, x, r in zip('EgK', hip, definition, ref):
        bf.check(f'reduced {name} C={C} H={H}', h, x, r)
    K = hip[2].reshape(H, 3, 4, H, 3, 4)
    assert torch.equal(K, K.permute(3, 1, 5, 0, 4, 2))        # K[12h+4b+n, 12h'+4b'+n'] == K[12h'+4b+n', 12h+4b'+n]
    return col, dx, w, x0, hip


@pytest.mark.parametrize('C,H', EDGES)
def test_reduced_terms(C, H):
    check_reduced(C, H)


def test_reduced_terms_static_sides_forms_and_repeats():
    col, dx, w, x0, (E, g, K) = check_reduced(SLICE[5] + 1, 5, static=True)
    for a, b in zip(col.reduced_terms(dx, w, x0, bf.COEFF), (E, g, K)):
        assert torch.equal(a, b)
    E2, g2, K2 = col.reduced_terms(dx, w, x0, bf.COEFF, hessian=False)
    assert K2 is None and torch.equal(E2, E) and torch.equal(g2, g)


def test_reduced_terms_graph_capture():
    (_, (col, dx, w, x0)) = case(SLICE[17] + 1, 17)
    eager = col.reduced_terms(dx, w, x0, bf.COEFF)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        col.reduced_terms(dx, w, x0, bf.COEFF)                # the allocator's warm-up
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = col.reduced_terms(dx, w, x0, bf.COEFF)
    for _ in range(3):
        for t in captured:
            t.fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(captured, eager))
