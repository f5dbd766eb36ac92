"""The HIP pipelines of marching_tetrahedra and subdivide_tetmesh at every stage boundary of the sort / scan / compaction they
share (csrc/sort_scan.h), on the cases of tet_boundary_cases.py (test_tet_boundary_cases_cpu.py shows that each case sits on the
boundary it names).  The CPU side is the package's torch formulation, which the two CPU test files pin to the reference's
records; forward results are compared bit for bit (`same`: integers are exact, floats are the same separately rounded
operations), gradients with the project's element-wise bound against float64 CPU autograd.  No test here passes an
out-of-range index."""
import functools
import time

import pytest
import torch

import tet_boundary_cases as tbc
from kaolin_amd.ops.conversions import marching_tetrahedra
from kaolin_amd.ops.conversions import tetmesh as mt_module
from kaolin_amd.ops.mesh import subdivide_tetmesh
from kaolin_amd.ops.mesh import tetmesh as st_module
from kaolin_amd.utils.testing import elementwise_mismatch, kuhn_grid
from subdivide_tetmesh_golden import same

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MT_FORMULATION = mt_module._torch_unbatched      # (the autouse fixture hides the module attributes; the CPU files pin them)
ST_FORMULATION = st_module._torch_subdivide
F32, F64 = torch.float32, torch.float64
BOTH = (F32, F64)

disjoint = functools.lru_cache(maxsize=None)(lambda counts, V_pad, seed: tbc.disjoint(counts, V_pad, seed))
soup = functools.lru_cache(maxsize=None)(lambda V: tbc.random_soup(40 if V <= 5 else 3000, V, seed=V))
big_soup = functools.lru_cache(maxsize=None)(tbc.big_soup)
star = functools.lru_cache(maxsize=None)(tbc.star)
fan = functools.lru_cache(maxsize=None)(tbc.fan)


@pytest.fixture(autouse=True)
def hip_path_only(monkeypatch):
    """A float32 / float64 GPU call that reached a torch formulation would pass these tests without running a kernel."""
    monkeypatch.setattr(mt_module, '_torch_unbatched', None)
    monkeypatch.setattr(st_module, '_torch_subdivide', None)


def mt_reference(vertices, tets, sdf, dtype):
    return [MT_FORMULATION(vertices[b].to(dtype), tets, sdf[b].to(dtype), True) for b in range(vertices.shape[0])]


def mt_matches(out, want, label):
    assert len(out) == 3 and all(len(o) == len(want) for o in out), label
    for b, (verts, faces, tet_idx) in enumerate(want):
        assert out[0][b].device == out[1][b].device == out[2][b].device == torch.device(DEV)
        assert same(out[0][b].cpu(), verts), (label, b, 'verts', tuple(out[0][b].shape), tuple(verts.shape))
        assert same(out[1][b].cpu(), faces), (label, b, 'faces')
        assert same(out[2][b].cpu(), tet_idx), (label, b, 'tet_idx')


def check_mt(case, dtypes=BOTH):
    vertices, tets, sdf, name = case
    for dtype in dtypes:
        out = marching_tetrahedra(vertices.to(DEV, dtype), tets.to(DEV), sdf.to(DEV, dtype), True)
        mt_matches(out, mt_reference(vertices, tets, sdf, dtype), (name, dtype))


def check_st(vertices, tets, features, name, dtypes=BOTH):
    for dtype in dtypes:
        f = None if features is None else features.to(dtype)
        want = ST_FORMULATION(vertices.to(dtype), tets, f)
        args = (vertices.to(DEV, dtype), tets.to(DEV), None if f is None else f.to(DEV))
        torch.cuda.synchronize(DEV)
        start = time.perf_counter()
        out = subdivide_tetmesh(*args)
        torch.cuda.synchronize(DEV)
        check_st.last_seconds = time.perf_counter() - start      # the HIP call alone, end to end
        assert len(out) == len(want) and all(o.device == torch.device(DEV) for o in out)
        for k, (o, w) in enumerate(zip(out, want)):
            assert same(o.cpu(), w), (name, dtype, ('new_vertices', 'new_tets', 'new_features')[k], tuple(o.shape), tuple(w.shape))
        assert tets.shape[0] == 0 or int(out[1].max()) == out[0].shape[1] - 1


def features_for(vertices, D=2):
    return tbc.cotangent(vertices.shape[:2] + (D,), seed=vertices.shape[1])


def check_gradient(got, want, tas, label):
    msg = elementwise_mismatch(got, want, tol=1e-5, term_abs_sum=tas)
    print(label, 'slack use', elementwise_mismatch.last_slack_use, msg)
    assert msg is None, (label, msg)


# ---- marching tetrahedra ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', tbc.INSTANCE_COUNTS)
def test_mt_exact_instance_counts(n):
    """n = nu crossing-edge instances exactly: on and next to the blocks of the key scan (1 024), the heads / unique kernels
    (256) and the radix sort (2 048)."""
    check_mt(disjoint(tuple(tbc.counts_for_instances(n)), n % 7, n))


@pytest.mark.parametrize('T', tbc.TET_COUNTS)
def test_mt_tet_count_edges(T):
    """T on and next to a wavefront (64), a round of the compaction (256) and a chunk of the count scan (1 024), all 16 sign
    cases interleaved."""
    check_mt(disjoint(tuple(tbc.counts_for_tets(T)), 0, T))


@pytest.mark.parametrize('V', tbc.SOUP_V + (tbc.BIG_V,))
def test_mt_radix_pass_widths(V):
    """1, 2, 3 and 4 radix passes per key half, with the largest id in a crossing edge on either side of every switch."""
    if V == tbc.BIG_V:
        check_mt(big_soup(), (F32,))
    else:
        check_mt(soup(V))


def test_mt_equal_key_runs():
    check_mt(tbc.repeated(5000))
    check_mt(tbc.repeated(5000, alternate=True))
    check_mt(fan(3000))


def test_mt_dense_random_signs():
    check_mt(tbc.dense_signs(12))


def test_mt_misaligned_tets_view():
    vertices, tets, sdf, name = soup(65537)
    shifted = torch.zeros(tets.numel() + 1, dtype=torch.long, device=DEV)[1:].view(-1, 4)
    shifted.copy_(tets)
    assert shifted.data_ptr() % 16 == 8 and shifted.is_contiguous()
    out = marching_tetrahedra(vertices.to(DEV), shifted, sdf.to(DEV), True)
    mt_matches(out, mt_reference(vertices, tets, sdf, F32), name)


def test_mt_side_stream():
    """The pipeline follows the current stream: two calls on a side stream, whose input is made on that stream, around one on
    the default stream."""
    vertices, tets, sdf, name = soup(65536)
    other = soup(257)
    p, t, s = vertices.to(DEV), tets.to(DEV), sdf.to(DEV)
    op, ot, os_ = (x.to(DEV) for x in other[:3])
    side = torch.cuda.Stream(device=DEV)
    assert side != torch.cuda.current_stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        # the sdf the pipeline reads is written on the side stream, behind a product that keeps that stream busy: kernels
        # launched on any other stream would read the buffer before it is filled
        busy = torch.ones(4096, 4096, device=DEV)
        keep = (busy @ busy).sum() > 0
        s_side = torch.where(keep, s, -s)
        first = marching_tetrahedra(p, t, s_side, True)
    between = marching_tetrahedra(op, ot, os_, True)
    with torch.cuda.stream(side):
        second = marching_tetrahedra(p, t, s_side, True)
    torch.cuda.current_stream(DEV).wait_stream(side)
    want = mt_reference(vertices, tets, sdf, F32)
    mt_matches(first, want, name)
    mt_matches(second, want, name)
    mt_matches(between, mt_reference(*other[:3], F32), other[3])


def run_mt_formulation(p, tets, s):
    return MT_FORMULATION(p[0], tets, s[0], False)[0]


def run_mt_hip(p, tets, s):
    return marching_tetrahedra(p, tets, s)[0][0]


@pytest.mark.parametrize('dtype', BOTH)
@pytest.mark.parametrize('shape,K', [('star', 300), ('star', 2000), ('fan', 3000)])
def test_mt_high_valence_gradients(shape, K, dtype):
    """3 K (star) or 2 K + 1 (fan) atomic adds into each of the hub's four addresses."""
    vertices, tets, sdf, name = star(K) if shape == 'star' else fan(K)
    nu = 3 * K if shape == 'star' else 2 * K + 1
    cot = tbc.cotangent((nu, 3), seed=K)
    want = tbc.mt_gradients(run_mt_formulation, vertices, tets, sdf, cot, F64)
    got = tbc.mt_gradients(run_mt_hip, vertices, tets, sdf, cot, dtype, DEV)
    tas = tbc.mt_term_abs_sums(vertices[0], tets, sdf[0], cot)
    for g, w, t, what in zip(got, want, tas, ('vertices', 'sdf')):
        assert g.dtype == dtype
        check_gradient(g, w, t, f'mt {name} {dtype} {what}')


# ---- subdivision ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', tbc.ST_TET_COUNTS)
def test_st_tet_count_edges(T):
    """6 T keys on either side of 256, 1 024, 2 048 and 4 096."""
    vertices, tets, _, name = tbc.random_soup(T, 5000, seed=T, B=2)
    check_st(vertices, tets, features_for(vertices), name)


@pytest.mark.parametrize('V', tbc.SOUP_V + (tbc.BIG_V,))
def test_st_radix_pass_widths(V):
    if V == tbc.BIG_V:
        vertices, tets, _, name = big_soup()
        check_st(vertices, tets, None, name, (F32,))
    else:
        vertices, tets, _, name = soup(V)
        check_st(vertices, tets, features_for(vertices), name)


def test_st_equal_key_runs():
    for vertices, tets, _, name in (tbc.repeated(5000), tbc.repeated(5000, alternate=True), fan(3000)):
        check_st(vertices, tets, features_for(vertices), name)


def test_st_scan_beyond_1024_blocks():
    """kuhn_grid(31): 1 072 476 keys, 1 048 blocks of the key scan.  kuhn_grid(62): 8 579 808 keys, 1 072 640 entries (1 048
    blocks) in the scan of the sort's histograms."""
    vertices, tets = tbc.permuted_kuhn_grid(31)
    assert tbc.cdiv(6 * tets.shape[0], 1024) == 1048
    check_st(vertices[None], tets, features_for(vertices[None]), 'grid31', (F32,))
    print(f'grid31 subdivide_tetmesh on the GPU, end to end: {check_st.last_seconds * 1e3:.2f} ms')
    vertices, tets = kuhn_grid(62)
    assert tbc.cdiv(6 * tets.shape[0], 2048) * 256 == 1072640
    check_st(vertices[None], tets, None, 'grid62', (F32,))
    print(f'grid62 subdivide_tetmesh on the GPU, end to end: {check_st.last_seconds * 1e3:.2f} ms')


@pytest.mark.parametrize('dtype', BOTH)
@pytest.mark.parametrize('K', [300, 2000])
def test_st_high_valence_gradients(K, dtype):
    """The hub is the min end of 3 K edges (one serial run of the min kernel) or, relabelled, the max end (3 K atomic adds into
    one row)."""
    for hub_last in (False, True):
        vertices, tets, _, name = star(K, hub_last)
        V, E = 3 * K + 1, 6 * K
        features = features_for(vertices)
        cot_v, cot_f = tbc.cotangent((1, V + E, 3), seed=2), tbc.cotangent((1, V + E, 2), seed=3)
        want = tbc.st_gradients(ST_FORMULATION, vertices, tets, features, cot_v, cot_f, F64)
        got = tbc.st_gradients(subdivide_tetmesh, vertices, tets, features, cot_v, cot_f, dtype, DEV)
        edges = tbc.unique_edges(tets)
        for g, w, cot, what in zip(got, want, (cot_v, cot_f), ('vertices', 'features')):
            assert g.dtype == dtype
            check_gradient(g, w, tbc.st_term_abs_sums(V, edges, cot), f'st {name} {dtype} {what}')


# ---- the loop -----------------------------------------------------------------------------------------------------------------
def test_dmtet_rounds():
    """subdivide_tetmesh's own output (ids V + e, eight blocks of T rows) subdivided again and marched, round by round."""
    hip = tbc.dmtet_rounds(subdivide_tetmesh, 6, 2, DEV)
    cpu = tbc.dmtet_rounds(ST_FORMULATION, 6, 2)
    assert [s[1].shape[0] for s in cpu] == [1296, 10368, 82944]
    for r, (got, want) in enumerate(zip(hip, cpu)):
        for g, w, what in zip(got, want, ('vertices', 'tets', 'feature')):
            assert same(g.cpu(), w), (r, what)
        out = marching_tetrahedra(got[0], got[1], got[2][..., 0], True)
        mt_matches(out, mt_reference(want[0], want[1], want[2][..., 0], F32), ('round', r))
