"""The cases of tet_boundary_cases.py without a GPU: every case sits on the boundary it names (crossing-edge instances n, unique
edges nu / E, tets T, radix passes, scan blocks, valence), each of three deliberately wrong formulations changes the answer of
the case aimed at it, and the float32 torch formulation's own gradients stay inside the bound the GPU tests apply.  The torch
formulations are the package's (pinned to the reference's records by test_marching_tetrahedra_cpu.py and
test_subdivide_tetmesh_cpu.py)."""
import functools

import pytest
import torch

import tet_boundary_cases as tbc
from kaolin_amd.ops.conversions import tetmesh as mt_module
from kaolin_amd.ops.mesh import tetmesh as st_module
from kaolin_amd.utils.testing import elementwise_mismatch, kuhn_grid
from subdivide_tetmesh_golden import same

MT = mt_module._torch_unbatched
ST = st_module._torch_subdivide
big_soup = functools.lru_cache(maxsize=None)(tbc.big_soup)


def mt_counts(case):
    vertices, tets, sdf, _ = case
    return tbc.mt_counts(MT, vertices[0], tets, sdf[0])


def num_edges(tets, V):
    new_vertices, new_tets = ST(torch.zeros(1, V, 3), tets, None)
    assert new_tets.shape == (8 * tets.shape[0], 4)
    return new_vertices.shape[1] - V


# ---- the cases are what they claim to be ---------------------------------------------------------------------------------
@pytest.mark.parametrize('n', tbc.INSTANCE_COUNTS)
def test_disjoint_instance_counts(n):
    counts = tbc.counts_for_instances(n)
    n_one, n_two, instances, nu = mt_counts(tbc.disjoint(counts, V_pad=n % 7, seed=n))
    assert n_one == sum(counts[c] for c in tbc.ONE_TRIANGLE_CASES) > 0
    assert n_two == sum(counts[c] for c in tbc.TWO_TRIANGLE_CASES) > 0
    assert instances == nu == n
    assert counts[0] > 0 and counts[15] > 0
    vertices, tets, sdf, _ = tbc.disjoint(counts, V_pad=n % 7, seed=n)
    assert tbc.fewest_cases_in_a_window(tbc.sign_cases(tets, sdf[0]), 64) == 16      # any 64 consecutive tets hold all 16 cases


@pytest.mark.parametrize('T', tbc.TET_COUNTS)
def test_disjoint_tet_counts(T):
    counts = tbc.counts_for_tets(T)
    vertices, tets, sdf, _ = tbc.disjoint(counts, seed=T)
    assert tets.shape == (T, 4) and sum(counts) == T and vertices.shape[1] == 4 * T
    assert T < 16 or all(c > 0 for c in counts)
    case = tbc.sign_cases(tets, sdf[0])
    assert torch.bincount(case, minlength=16).tolist() == counts
    if T >= 63:                                              # interleaved: any 32 consecutive tets hold all 16 cases
        assert tbc.fewest_cases_in_a_window(case, 32) == 16
    n_one, n_two, n, nu = mt_counts((vertices, tets, sdf, None))
    assert (n_one, n_two) == (sum(counts[c] for c in tbc.ONE_TRIANGLE_CASES), sum(counts[c] for c in tbc.TWO_TRIANGLE_CASES))
    assert n == nu and num_edges(tets, 4 * T) == 6 * T


def test_pass_counts():
    """8-bit passes per key half: one more whenever the largest id V - 1 needs another digit."""
    want = {2: 1, 5: 1, 255: 1, 256: 1, 257: 2, 65535: 2, 65536: 2, 65537: 3, 2 ** 24: 3, 2 ** 24 + 1: 4, tbc.BIG_V: 4,
            1000: 2, 54872: 2, 70001: 3}
    for V, passes in want.items():
        assert tbc.passes_per_half(V) == passes == max(1, ((V - 1).bit_length() + 7) // 8), V
    assert set(tbc.SOUP_V) <= set(want)


@pytest.mark.parametrize('V', tbc.SOUP_V)
def test_soup(V):
    T = 40 if V <= 5 else 3000
    vertices, tets, sdf, _ = tbc.random_soup(T, V, seed=V, B=2)
    assert tets.shape == (T, 4) and int(tets.max()) == V - 1 and int(tets.min()) >= 0 and vertices.shape == (2, V, 3)
    assert float(sdf.abs().min()) >= 0.05
    assert bool((tets[:, 3] == tets[:, 1]).any())
    assert torch.unique(tets, dim=0).shape[0] < T
    for b in range(2):
        n_one, n_two, n, nu = mt_counts((vertices[b:b + 1], tets, sdf[b:b + 1], None))
        assert n_one > 0 and n_two > 0 and nu <= n
        a, c = tbc.crossing_edges(tets, sdf[b])
        assert int(c.max()) == V - 1 and a.shape[0] == nu   # the top id reaches the sort, and the formulation agrees with the pairs
        if V > 5:
            assert n_one + n_two > 0.8 * T
    edges = tbc.unique_edges(tets)
    assert num_edges(tets, V) == edges.shape[0] and int(edges.max()) == V - 1
    assert bool((edges[:, 0] == edges[:, 1]).any())         # self-edges


def test_big_soup():
    vertices, tets, sdf, _ = big_soup()
    assert vertices.shape == (1, tbc.BIG_V, 3) and vertices.dtype == torch.float32 and tets.shape == (20000, 4)
    assert int(tets.max()) == tbc.BIG_V - 1
    n_one, n_two, n, nu = mt_counts((vertices, tets, sdf, None))
    a, b = tbc.crossing_edges(tets, sdf[0])
    assert nu == a.shape[0] and int(b.max()) == tbc.BIG_V - 1 and n_one + n_two > 16000
    # ids on both sides of 2^24 in either half of the keys, and pairs that differ in the top byte alone
    assert bool((a >= 2 ** 24).any()) and bool((a < 2 ** 24).any()) and bool((b >= 2 ** 24).any()) and bool((b < 2 ** 24).any())
    low = ((a & 0xffffff) << 32) | (b & 0xffffff)
    assert torch.unique(low).shape[0] < nu or not bool((low[1:] > low[:-1]).all())


def test_equal_key_runs():
    n_one, n_two, n, nu = mt_counts(tbc.repeated(5000))
    assert (n_one, n_two, n, nu) == (0, 5000, 20000, 4) and num_edges(tbc.repeated(5000)[1], 6) == 6
    vertices, tets, sdf, _ = tbc.repeated(5000, alternate=True)
    assert mt_counts((vertices, tets, sdf, None)) == (2500, 2500, 17500, 6) and num_edges(tets, 6) == 11
    vertices, tets, sdf, _ = tbc.fan(3000)
    assert mt_counts((vertices, tets, sdf, None)) == (3000, 0, 9000, 6001)
    assert bool(((tets == 0).sum(1) == 1).all()) and bool(((tets == 1).sum(1) == 1).all())
    assert tbc.cdiv(9000, 2048) == 5                          # the 3 000 keys (0, 1) span sort blocks
    assert num_edges(tets, 70000) == 1 + 4 * 3000 + 3000 and tbc.passes_per_half(70000) == 3


@pytest.mark.parametrize('K', [300, 2000])
def test_star_valence(K):
    for hub_last in (False, True):
        vertices, tets, sdf, _ = tbc.star(K, hub_last)
        V, hub = 3 * K + 1, (3 * K if hub_last else 0)
        assert mt_counts((vertices, tets, sdf, None)) == (K, 0, 3 * K, 3 * K)
        a, b = tbc.crossing_edges(tets, sdf[0])
        assert int(((a == hub) | (b == hub)).sum()) == 3 * K
        edges = tbc.unique_edges(tets)
        assert edges.shape[0] == 6 * K == num_edges(tets, V)
        assert int((edges[:, 1 if hub_last else 0] == hub).sum()) == 3 * K


def test_dense_signs():
    vertices, tets, sdf, _ = tbc.dense_signs(12)
    assert vertices.shape == (3, 13 ** 3, 3) and tets.shape == (6 * 12 ** 3, 4) and sdf.shape == (3, 13 ** 3)
    assert not bool((tets[:, 1:] > tets[:, :-1]).all(dim=1).all())          # corner order is random
    case = ((sdf > 0)[:, tets].long() << torch.arange(4)).sum(-1)           # (3, T)
    for item in (0, 2):
        # independent random signs: the fewest distinct cases that any 64 consecutive tets hold (13 and 12 with this seed), and
        # every 256 consecutive tets (a round of the compaction) hold all 16
        assert tbc.fewest_cases_in_a_window(case[item], 64) == (13 if item == 0 else 12)
        assert tbc.fewest_cases_in_a_window(case[item], 256) == 16
        valid = ((case[item] > 0) & (case[item] < 15)).float().mean()
        assert 0.8 < float(valid) < 0.95                                    # 7/8 of the tets
    assert bool((case[1] == 15).all()) and mt_counts((vertices[1:2], tets, sdf[1:2], None)) == (0, 0, 0, 0)
    special = sdf[2]
    assert bool(torch.isnan(special).any()) and bool(torch.isinf(special).any())
    zeros = special[special == 0]
    assert bool(torch.signbit(zeros).any()) and not bool(torch.signbit(zeros).all())
    assert bool(torch.isnan(MT(vertices[2], tets, sdf[2], False)[0]).any())


def test_scan_block_counts():
    """The two subdivision cases whose scans have more than 1 024 blocks of 1 024."""
    assert kuhn_grid(3)[1].shape[0] == 6 * 3 ** 3
    T31, T62 = 6 * 31 ** 3, 6 * 62 ** 3
    assert 6 * T31 == 1072476 and tbc.cdiv(6 * T31, 1024) == 1048 > 1024
    assert 6 * T62 == 8579808 and tbc.cdiv(6 * T62, 2048) * 256 == 1072640 > 2 ** 20
    assert tbc.cdiv(tbc.cdiv(6 * T62, 2048) * 256, 1024) > 1024
    assert tbc.cdiv(6 * 93750, 1024) < 1024                  # (grid25, the largest case before these)


@pytest.mark.parametrize('T', tbc.ST_TET_COUNTS)
def test_subdivision_key_counts(T):
    around = [b for b in (256, 1024, 2048, 4096) if abs(6 * T - b) <= 6]
    assert around or T in (1, 2, 255, 256, 257)
    tets = tbc.random_soup(T, 5000, seed=T)[1]
    assert tets.shape == (T, 4) and 0 < num_edges(tets, 5000) <= 6 * T


def test_dmtet_rounds():
    states = tbc.dmtet_rounds(ST, 6, 2)
    assert [s[1].shape[0] for s in states] == [1296, 10368, 82944]
    for (vertices, tets, feature), (nv, nt, nf) in zip(states[:-1], states[1:]):
        V = vertices.shape[1]
        assert nv.shape[1] == nf.shape[1] == V + tbc.unique_edges(tets).shape[0] and nf.shape[2] == 1
        assert int(nt.max()) == nv.shape[1] - 1 and bool((nt[:tets.shape[0], 1:] >= V).all())
    for vertices, tets, feature in states:
        n_one, n_two, n, nu = tbc.mt_counts(MT, vertices[0], tets, feature[0, :, 0])
        assert n_one > 0 and n_two > 0


# ---- the cases bite: three wrong formulations -------------------------------------------------------------------------------
def mt_variant(vertices, tets, sdf, low24=False, swap=True, reverse_two=False):
    """_torch_unbatched(..., True) with three switches: keys compared on the low 24 bits of each half only; the ends of an edge
    not ordered; the two-triangle tets emitted in reverse tet order."""
    slot_a = torch.tensor([e[0] for e in mt_module.EDGE_CORNERS])
    slot_b = torch.tensor([e[1] for e in mt_module.EDGE_CORNERS])
    case = ((sdf > 0)[tets].long() << torch.arange(4)).sum(-1)
    num_tri = torch.tensor(mt_module.NUM_TRIANGLES)[case]
    valid = torch.nonzero(num_tri > 0).reshape(-1)
    case, num_tri, corners = case[valid], num_tri[valid], tets[valid]
    ea, eb = corners[:, slot_a], corners[:, slot_b]
    lo, hi = (torch.minimum(ea, eb), torch.maximum(ea, eb)) if swap else (ea, eb)
    if low24:
        lo, hi = lo & 0xffffff, hi & 0xffffff
    keys = (lo << 32) | hi
    crossing = (((case.unsqueeze(1) >> slot_a) ^ (case.unsqueeze(1) >> slot_b)) & 1).bool()
    unique_keys = torch.unique(keys[crossing])
    a, b = unique_keys >> 32, unique_keys & 0xffffffff
    rank = torch.searchsorted(unique_keys, keys)
    table = torch.tensor(mt_module.TRIANGLE_SLOTS)
    one, two = num_tri == 1, num_tri == 2
    faces_two = torch.gather(rank[two], 1, table[case[two]])
    idx_two = valid[two]
    if reverse_two:
        faces_two, idx_two = faces_two.flip(0), idx_two.flip(0)
    faces = torch.cat((torch.gather(rank[one], 1, table[case[one]][:, :3]), faces_two.reshape(-1, 3)), dim=0)
    sa, nsb = sdf[a].unsqueeze(1), -sdf[b].unsqueeze(1)
    verts = (vertices[a] * nsb + vertices[b] * sa) / (sa + nsb)
    return verts, faces, torch.cat((valid[one], idx_two.repeat_interleave(2)), dim=0)


def st_variant(vertices, tets, low24=False, swap=True):
    slot_a = torch.tensor([e[0] for e in st_module.EDGE_CORNERS])
    slot_b = torch.tensor([e[1] for e in st_module.EDGE_CORNERS])
    ea, eb = tets[:, slot_a], tets[:, slot_b]
    lo, hi = (torch.minimum(ea, eb), torch.maximum(ea, eb)) if swap else (ea, eb)
    if low24:
        lo, hi = lo & 0xffffff, hi & 0xffffff
    keys = (lo << 32) | hi
    unique_keys = torch.unique(keys)
    lo, hi = unique_keys >> 32, unique_keys & 0xffffffff
    rank = torch.searchsorted(unique_keys, keys) + vertices.shape[1]
    columns = torch.cat((tets, rank), dim=1)
    new_tets = columns[:, torch.tensor(st_module.CHILD_TETS)].permute(1, 0, 2).reshape(-1, 4)
    return torch.cat((vertices, (vertices[:, lo] + vertices[:, hi]) * 0.5), dim=1), new_tets


def mt_same(case, **switches):
    vertices, tets, sdf, _ = case
    want = MT(vertices[0], tets, sdf[0], True)
    got = mt_variant(vertices[0], tets, sdf[0], **switches)
    return all(same(g, w) for g, w in zip(got, want))


def st_same(case, **switches):
    vertices, tets, _, _ = case
    want = ST(vertices, tets, None)
    got = st_variant(vertices, tets, **switches)
    return all(same(g, w) for g, w in zip(got, want))


def test_variants_without_a_switch_are_the_formulations():
    for case in (tbc.random_soup(3000, 65537, seed=65537), tbc.disjoint(tbc.counts_for_instances(257), seed=257), tbc.star(300)):
        assert mt_same(case) and st_same(case)


def test_low_24_bits_only_is_caught():
    assert not mt_same(big_soup(), low24=True) and not st_same(big_soup(), low24=True)
    small = tbc.random_soup(3000, 65537, seed=65537)
    assert mt_same(small, low24=True) and st_same(small, low24=True)


def test_unordered_edge_ends_are_caught():
    for V in (257, 65537):
        soup = tbc.random_soup(3000, V, seed=V)
        assert not mt_same(soup, swap=False) and not st_same(soup, swap=False)
    assert not mt_same(tbc.fan(3000), swap=False)
    ascending = tbc.star(300)                                # every tet's corners ascend: nothing to swap
    assert mt_same(ascending, swap=False) and st_same(ascending, swap=False)


def test_two_triangle_order_is_caught():
    for n in (257, 2049):
        assert not mt_same(tbc.disjoint(tbc.counts_for_instances(n), seed=n), reverse_two=True)
    assert not mt_same(tbc.repeated(5000, alternate=True), reverse_two=True)      # (tet_idx alone differs)
    assert mt_same(tbc.star(300), reverse_two=True)          # no two-triangle tet
    assert mt_same(tbc.disjoint(tbc.counts_for_tets(1), seed=1), reverse_two=True)


# ---- the reference alone stays inside the gradient bound -------------------------------------------------------------------
def run_mt(p, tets, s):
    return MT(p[0], tets, s[0], False)[0]


def check(got, want, tas, label):
    msg = elementwise_mismatch(got, want, tol=1e-5, term_abs_sum=tas)
    print(label, 'slack use', elementwise_mismatch.last_slack_use, msg)
    assert msg is None, (label, msg)


@pytest.mark.parametrize('name,K', [('star', 100), ('star', 300), ('star', 2000), ('star_hub_last', 2000), ('fan', 3000)])
def test_mt_float32_gradients_inside_the_bound(name, K):
    vertices, tets, sdf, _ = tbc.fan(K) if name == 'fan' else tbc.star(K, name == 'star_hub_last')
    cot = tbc.cotangent((mt_counts((vertices, tets, sdf, None))[3], 3), seed=K)
    want = tbc.mt_gradients(run_mt, vertices, tets, sdf, cot, torch.float64)
    got = tbc.mt_gradients(run_mt, vertices, tets, sdf, cot, torch.float32)
    tas = tbc.mt_term_abs_sums(vertices[0], tets, sdf[0], cot)
    for g, w, t, what in zip(got, want, tas, ('vertices', 'sdf')):
        check(g, w, t, f'{name} K={K} {what}')


@pytest.mark.parametrize('hub_last', [False, True])
@pytest.mark.parametrize('K', [300, 2000])
def test_st_float32_gradients_inside_the_bound(K, hub_last):
    vertices, tets, _, _ = tbc.star(K, hub_last)
    V, E = 3 * K + 1, 6 * K
    features = tbc.cotangent((1, V, 2), seed=1)
    cot_v, cot_f = tbc.cotangent((1, V + E, 3), seed=2), tbc.cotangent((1, V + E, 2), seed=3)
    want = tbc.st_gradients(ST, vertices, tets, features, cot_v, cot_f, torch.float64)
    got = tbc.st_gradients(ST, vertices, tets, features, cot_v, cot_f, torch.float32)
    edges = tbc.unique_edges(tets)
    for g, w, cot, what in zip(got, want, (cot_v, cot_f), ('vertices', 'features')):
        check(g, w, tbc.st_term_abs_sums(V, edges, cot), f'star K={K} hub_last={hub_last} {what}')
