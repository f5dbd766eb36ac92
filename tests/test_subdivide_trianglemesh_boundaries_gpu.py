"""The HIP pipeline of ops.mesh.subdivide_trianglemesh (csrc/subdivide_trianglemesh.hip) at the boundaries of its two sorts, its
scans, its id widths and its batch loop, against the numpy brute force of subdivide_trianglemesh_bruteforce.py (which
test_subdivide_trianglemesh_bruteforce_cpu.py pins to the reference's records): the topology bit for bit, the values within the
bounds derived in the brute force's docstring, in float32 and float64, with alpha given and default.  The meshes come from
subdivide_trianglemesh_boundary_cases.py; every test asserts from the brute force's own counts that its mesh sits where its
parameter says.  Every mesh is valid: no test passes an out-of-range id or a misaligned pointer.  Every value check prints the
share of its bound it used (pytest -s)."""
import numpy as np
import pytest
import torch

import subdivide_trianglemesh_boundary_cases as cases
import subdivide_trianglemesh_bruteforce as bf
from kaolin_amd import _C
from kaolin_amd.ops.mesh import subdivide_trianglemesh, trianglemesh
from subdivide_trianglemesh_golden import SMALL_CASES, case_inputs, check_small_forward, small_inputs

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OPS = _C.ops.mesh


def _refuse(*args):
    raise AssertionError('a float32 / float64 GPU call reached the torch formulation')


@pytest.fixture(scope='module', autouse=True)
def worst_shares():
    """After the last test of this file that ran: the largest share of a bound that any of them used, per direction and dtype"""
    yield
    cases.report()


@pytest.fixture(autouse=True)
def hip_path_only(monkeypatch):
    """A float32 / float64 GPU call that reached the torch formulation would pass these tests without running a kernel."""
    monkeypatch.setattr(trianglemesh, '_torch_iteration', _refuse)


def on_host(array):
    return torch.from_numpy(np.ascontiguousarray(array))


def hip_topology(faces, V):
    new_faces, topo = OPS.subdivide_trianglemesh_cuda(faces.to(DEV), V)
    assert all(t.device == torch.device(DEV) for t in (new_faces,) + tuple(topo))
    return new_faces, topo


def check_topology(tp, new_faces, topo):
    """new_faces, edges, count and tlist in full; opp with its two slots sorted where count == 2 (elsewhere it is uninitialised by
    design); runs and valence in full where the brute force holds them, else at the rows of every used id and its two
    neighbours and at rows 0, V - 1 and V; runs non-decreasing; the valences add up to 2 E less the self-edges."""
    edges, count, opp, tlist, runs, valence = topo
    assert edges.shape == (tp.E, 2) and runs.shape == (tp.V + 1, 2) and valence.shape == (tp.V,)
    assert torch.equal(new_faces.cpu(), on_host(tp.new_faces)), 'new_faces'
    assert torch.equal(edges.cpu(), on_host(tp.edges)), 'edges'
    assert torch.equal(count.cpu(), on_host(tp.count)), 'count'
    assert torch.equal(tlist.cpu(), on_host(tp.tlist)), 'tlist'
    two = on_host(tp.count == 2)
    assert torch.equal(opp.cpu()[two].sort(dim=1).values, on_host(tp.opp)[two]), 'opp'
    if tp.runs is not None:
        assert torch.equal(runs.cpu(), on_host(tp.runs)), 'runs'
        assert torch.equal(valence.cpu(), on_host(tp.valence)), 'valence'
    else:
        used = np.unique(tp.edges)
        rows = np.unique(np.clip(np.concatenate([used - 1, used, used + 1, [0, tp.V - 1, tp.V]]), 0, tp.V))
        assert torch.equal(runs[torch.from_numpy(rows).to(DEV)].cpu(), on_host(tp.runs_at(rows))), 'runs'
        assert torch.equal(valence[torch.from_numpy(rows[:-1]).to(DEV)].cpu(), on_host(tp.valence_at(rows[:-1]))), 'valence'
    assert bool((runs[1:] >= runs[:-1]).all()) and runs[0].tolist() == [0, 0] and runs[-1].tolist() == [tp.E, tp.E]
    assert int(valence.sum(dtype=torch.long)) == 2 * tp.E - tp.self_edges


def check_values(faces, V, tp, topo, new_faces, label, B=1, dtypes=cases.DTYPES, settings=cases.SETTINGS, views=None):
    """The two value operators under both cotangents, and the public function with its autograd backward (one iteration: no
    gradient arrives for new_alpha), in every dtype and setting.  `views`: a function that turns the inputs into the views to
    pass (the brute force gets what the views hold)."""
    for dtype in dtypes:
        x, alpha, gx, ga = (t.to(DEV) for t in cases.inputs(B, V, tp.E, dtype, seed=V + tp.E))
        if views is not None:
            x, alpha = views(x, alpha)
        for setting in settings:
            a = alpha if setting == 'alpha' else None
            tag = f'{label} {setting}'
            new_x, new_alpha = OPS.trianglemesh_loop_forward_cuda(x, a, topo)
            assert new_x.dtype == dtype and new_x.shape == (B, V + tp.E, 3)
            cases.check_forward(tp, new_x, new_alpha, x, a, tag)
            dx, da = OPS.trianglemesh_loop_backward_cuda(gx, None if a is None else ga, x, a, topo, a is not None)
            assert (da is None) == (a is None)
            cases.check_backward(tp, dx, da, x, a, gx, None if a is None else ga, tag)
            p, q = x.clone().requires_grad_(), (None if a is None else a.clone().requires_grad_())
            out_x, out_faces = subdivide_trianglemesh(p, faces.to(DEV), 1, q)
            assert torch.equal(out_x, new_x) and torch.equal(out_faces, new_faces)
            (out_x * gx).sum().backward()
            cases.check_backward(tp, p.grad, None if q is None else q.grad, x, a, gx, None, tag + ' autograd')


def run_case(faces, V, label, tp=None, **kwargs):
    tp = bf.topology(faces.numpy(), V) if tp is None else tp
    new_faces, topo = hip_topology(faces, V)
    check_topology(tp, new_faces, topo)
    check_values(faces, V, tp, topo, new_faces, label, **kwargs)
    return tp


# ---- the first sort, the head scan and the scan of the histograms: 3 F keys -----------------------------------------------
@pytest.mark.parametrize('F', cases.KEY_FACES)
def test_key_counts(F):
    """3 F next to a block of the head scan (1 024), of the sort (2 048), two of them (4 096), and on either side of the
    histogram scan's second block (256 entries per sort block: 1 024 entries at 8 190 keys, 1 280 at 8 193)."""
    faces, V = cases.mesh_for_keys(F)
    keys = 3 * faces.shape[0]
    assert keys == 3 * F == cases.KEY_COUNTS[cases.KEY_FACES.index(F)]
    assert min(abs(keys - edge) for edge in (0, 1024, 2048, 4096, 8192)) <= 3
    if keys in (8190, 8193):
        assert cases.cdiv(256 * cases.cdiv(keys, cases.SORT_BLOCK), cases.SCAN_BLOCK) == (1 if keys == 8190 else 2)
    run_case(faces, V, f'keys {keys}')


# ---- the second sort and the launches over E ------------------------------------------------------------------------------
@pytest.mark.parametrize('E', cases.EDGE_COUNTS)
def test_edge_counts(E):
    """E on and next to a block of the edge launches (256), of the scan (1 024) and of the sort (2 048, 4 096); E = 1 is the
    face (a, a, a), E = 257, 1 025, 2 049 and 4 097 leave a last block of one."""
    faces, V = cases.mesh_for_edges(E)
    tp = bf.topology(faces.numpy(), V)
    assert tp.E == E
    run_case(faces, V, f'edges {E}', tp)


# ---- radix passes per key half ----------------------------------------------------------------------------------------------
def id_width_case(V):
    faces, V, ids = cases.mesh_for_id_width(V)
    tp = bf.topology(faces.numpy(), V)
    used = set(np.unique(tp.edges).tolist())
    assert used == set(ids.tolist()) and {0, V - 1} | {s for s in cases.ID_WIDTH_SPECIAL if s < V} <= used and tp.E == 81
    return faces, V, tp


@pytest.mark.parametrize('V', cases.ID_WIDTH_FULL)
def test_id_widths(V):
    """The largest id on either side of the switch from 1 to 2 and from 2 to 3 passes per half: an id with a bit above the sorted
    digits would sort as if that bit were 0."""
    faces, V, tp = id_width_case(V)
    assert cases.passes_per_half(V) == {256: 1, 257: 2, 65536: 2, 65537: 3}[V]
    run_case(faces, V, f'ids below {V}', tp)


@pytest.mark.parametrize('V', cases.ID_WIDTH_TOPOLOGY)
def test_id_widths_topology_only(V):
    """3 and 4 passes per half.  No vertex tensor of that size is made: the topology alone, its per-vertex tensors at the rows
    that can differ from their neighbours'."""
    faces, V, tp = id_width_case(V)
    assert cases.passes_per_half(V) == {1 << 24: 3, (1 << 24) + 1: 4}[V] and tp.runs is None
    new_faces, topo = hip_topology(faces, V)
    check_topology(tp, new_faces, topo)


# ---- more than 1 024 blocks of the head scan ------------------------------------------------------------------------------------
@pytest.mark.parametrize('F', cases.BIG_FACES)
def test_second_scan_level(F):
    """The apply kernel of the scan adds up, in block b, the b block sums before it, thread t taking t, t + 1 024, ...  349 526
    faces (1 048 578 keys, 1 025 blocks): the last block adds up 1 024 sums, every thread one, and no thread goes round twice --
    one block short of the loop.  349 868 faces (1 049 604 keys, 1 026 blocks): the last block adds up 1 025, thread 0 two of
    them.  The two large cases: the topology against the vectorised brute force, and a float32 forward."""
    faces, V = cases.big_grid(F)
    keys = 3 * faces.shape[0]
    sums_of_last_block = cases.cdiv(keys, cases.SCAN_BLOCK) - 1
    assert faces.shape[0] == F and keys == {349526: 1048578, 349868: 1049604}[F]
    assert sums_of_last_block == 1024 if F == cases.BIG_FACES[0] else sums_of_last_block > 1024
    tp = bf.topology_vectorised(faces.numpy(), V)
    new_faces, topo = hip_topology(faces, V)
    check_topology(tp, new_faces, topo)
    x, alpha, _, _ = (t.to(DEV) for t in cases.inputs(1, V, tp.E, torch.float32, seed=1))
    for a in (alpha, None):
        new_x, new_alpha = OPS.trianglemesh_loop_forward_cuda(x, a, topo)
        cases.check_forward(tp, new_x, new_alpha, x, a, 'grid ' + ('default' if a is None else 'alpha'))


# ---- valences and counts ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', SMALL_CASES)
def test_small_cases(case):
    """Runs of 3 .. 300 neighbours in the edge list (hub first) and in the transposed list (hub last), valences 1 and 2,
    self-edges, counts 1 .. 4, an unused id: against the brute force and, in float32 on the recorded inputs, against the rows
    the reference defines."""
    vertices, faces, alpha = small_inputs(case)
    V = vertices.shape[1]
    run_case(faces, V, case)
    for setting in cases.SETTINGS:
        out = subdivide_trianglemesh(vertices.to(DEV), faces.to(DEV), 1, alpha.to(DEV) if setting == 'alpha' else None)
        check_small_forward(case, setting, *out)


# ---- the batch loop -------------------------------------------------------------------------------------------------------------
def batch_mesh(mesh):
    return (case_inputs('doc')[1], 4) if mesh == 'doc' else cases.wheel(6, seed=6)


@pytest.mark.parametrize('mesh', ['doc', 'wheel6'])
@pytest.mark.parametrize('B', cases.BATCHES)
def test_batches(B, mesh):
    """gridDim.y = min(B, 1024): B below, on and above it, and above twice it; every item different.  The forward has no
    atomics: an item of the batch has the bits of the same item run alone."""
    faces, V = batch_mesh(mesh)
    tp = bf.topology(faces.numpy(), V)
    new_faces, topo = hip_topology(faces, V)
    check_topology(tp, new_faces, topo)
    check_values(faces, V, tp, topo, new_faces, f'{mesh} B = {B}', B=B)
    for dtype in cases.DTYPES:
        x, alpha, _, _ = (t.to(DEV) for t in cases.inputs(B, V, tp.E, dtype, seed=V + tp.E))
        assert x.shape[0] == B and torch.unique(x.reshape(B, -1), dim=0).shape[0] == B
        for a in (None, alpha):
            new_x, new_alpha = OPS.trianglemesh_loop_forward_cuda(x, a, topo)
            alone = [OPS.trianglemesh_loop_forward_cuda(x[b:b + 1], None if a is None else a[b:b + 1], topo) for b in range(B)]
            assert torch.equal(new_x, torch.cat([one[0] for one in alone]))
            assert a is None or torch.equal(new_alpha, torch.cat([one[1] for one in alone]))


@pytest.mark.parametrize('mesh', ['doc', 'wheel6'])
def test_expanded_batch(mesh):
    """B = 1025 items that are one item (batch stride 0): every result row block equals that of item 0"""
    B = 1025
    faces, V = batch_mesh(mesh)
    tp = bf.topology(faces.numpy(), V)
    new_faces, topo = hip_topology(faces, V)

    def expanded(x, alpha):
        x, alpha = x[:1].expand(B, -1, -1), alpha[:1].expand(B, -1)
        assert x.stride(0) == 0 and alpha.stride(0) == 0
        return x, alpha

    check_values(faces, V, tp, topo, new_faces, f'{mesh} expanded', B=B, views=expanded)
    for dtype in cases.DTYPES:
        x, alpha = expanded(*(t.to(DEV) for t in cases.inputs(B, V, tp.E, dtype, seed=V + tp.E)[:2]))
        for a in (None, alpha):
            new_x, new_alpha = OPS.trianglemesh_loop_forward_cuda(x, a, topo)
            assert torch.equal(new_x, new_x[:1].expand(B, -1, -1))
            assert a is None or torch.equal(new_alpha, new_alpha[:1].expand(B, -1))


# ---- one iteration of autograd ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mesh', ['wheel', 'counts234'])
def test_one_iteration_backward(mesh):
    """alpha requires a gradient and the loss reads new_vertices only: no gradient arrives for new_alpha, the gather runs with a
    result for alpha and no cotangent for it, the opposite-corner kernel over three channels.  And alpha given as a constant."""
    faces, V = cases.wheel(7, hub_last=True, seed=3) if mesh == 'wheel' else (small_inputs('counts234')[1], 5)
    tp = bf.topology(faces.numpy(), V)
    assert int((tp.count == 2).sum()) > 0
    for dtype in cases.DTYPES:
        x, alpha, gx, _ = (t.to(DEV) for t in cases.inputs(2, V, tp.E, dtype, seed=V))
        calls = []
        backward_cuda = OPS.trianglemesh_loop_backward_cuda

        def spy(grad_new_vertices, grad_new_alpha, vertices, alpha_, topo, alpha_needs_grad):
            calls.append((grad_new_alpha is None, alpha_ is not None, alpha_needs_grad))
            return backward_cuda(grad_new_vertices, grad_new_alpha, vertices, alpha_, topo, alpha_needs_grad)

        for alpha_needs_grad in (True, False):
            p, q = x.clone().requires_grad_(), alpha.clone().requires_grad_(alpha_needs_grad)
            with pytest.MonkeyPatch.context() as patch:
                patch.setattr(OPS, 'trianglemesh_loop_backward_cuda', spy)
                (subdivide_trianglemesh(p, faces.to(DEV), 1, q)[0] * gx).sum().backward()
            assert calls[-1] == (True, True, alpha_needs_grad)
            assert (q.grad is not None) == alpha_needs_grad
            bw = cases.check_backward(tp, p.grad, q.grad, x, alpha, gx, None, f'{mesh} alpha_needs_grad={alpha_needs_grad}')
            assert alpha_needs_grad or bw.da is not None              # (the brute force computes it; nothing is compared with it)
        assert len(calls) == 2


# ---- the same bits twice ----------------------------------------------------------------------------------------------------------
def test_repeatable():
    faces, V = cases.mesh_for_edges(2049)
    first_faces, first = hip_topology(faces, V)
    second_faces, second = hip_topology(faces, V)
    assert first[0].shape[0] == 2049 and torch.equal(first_faces, second_faces)
    two = first[1] == 2
    for name, s, t in zip(_C.ops.LOOP_TOPOLOGY, first, second):
        if name == 'opp':
            assert torch.equal(s[two].sort(dim=1).values, t[two].sort(dim=1).values)
        else:
            assert torch.equal(s, t), name
    for dtype in cases.DTYPES:
        x, alpha, _, _ = (t.to(DEV) for t in cases.inputs(2, V, 2049, dtype, seed=5))
        for a in (None, alpha):
            s, t = OPS.trianglemesh_loop_forward_cuda(x, a, first), OPS.trianglemesh_loop_forward_cuda(x, a, second)
            assert torch.equal(s[0], t[0]) and (a is None or torch.equal(s[1], t[1]))
