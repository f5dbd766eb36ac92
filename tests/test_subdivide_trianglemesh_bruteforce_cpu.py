"""The numpy brute force of one Loop iteration (subdivide_trianglemesh_bruteforce.py) against everything the reference recorded
(tests/golden/subdivide_trianglemesh.npz and subdivide_trianglemesh_edges.npz, both written by
make_golden_subdivide_trianglemesh.py), and the package's CPU path against the brute force on the boundary cases that
test_subdivide_trianglemesh_boundaries_gpu.py runs on the HIP pipeline (those with V <= 65537), within the bounds derived in the
brute force's docstring: the bounds are shown to hold for a correct implementation before a GPU sees them.  Every value check
prints the share of its bound it used (pytest -s)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import subdivide_trianglemesh_boundary_cases as cases
import subdivide_trianglemesh_bruteforce as bf
from kaolin_amd.ops.mesh import subdivide_trianglemesh, trianglemesh
from subdivide_trianglemesh_golden import (FORWARD_CASES, G_SMALL, GRAD_CASES, SETTINGS, SMALL_CASES, case_inputs, check_forward,
                                           check_gradients, check_small_forward, small_inputs, tensor)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module', autouse=True)
def worst_shares():
    """After the last test of this file that ran: the largest share of a bound that any of them used, per direction and dtype"""
    yield
    cases.report()


def iterate(vertices, faces, alpha, iterations):
    """The brute force chained -> per iteration (topology, x, alpha) going in, and the final new_x, new_faces"""
    x, a, f, steps = vertices.numpy(), None if alpha is None else alpha.numpy(), faces.numpy(), []
    for _ in range(iterations):
        tp = bf.topology(f, x.shape[1])
        fw = bf.forward(tp, x, a)
        steps.append((tp, x, a))
        x, a, f = fw.new_x, fw.new_alpha, tp.new_faces
    return steps, x, f


# ---- the brute force against the reference's records ----------------------------------------------------------------------
@pytest.mark.parametrize('setting', SETTINGS)
@pytest.mark.parametrize('case,iterations', FORWARD_CASES)
def test_bruteforce_matches_reference(case, iterations, setting):
    vertices, faces, alpha = case_inputs(case)
    _, x, f = iterate(vertices, faces, alpha if setting == 'alpha' else None, iterations)
    check_forward(case, iterations, setting, torch.from_numpy(x), torch.from_numpy(f))


@pytest.mark.parametrize('setting', SETTINGS)
@pytest.mark.parametrize('case', SMALL_CASES)
def test_bruteforce_matches_reference_small(case, setting):
    vertices, faces, alpha = small_inputs(case)
    _, x, f = iterate(vertices, faces, alpha if setting == 'alpha' else None, 1)
    rows = check_small_forward(case, setting, torch.from_numpy(x), torch.from_numpy(f))
    assert rows == x.shape[1] - (case == 'tet_gap')


def test_small_cases_hold_what_they_are_for():
    """The valences and counts each case of the second file was made for, from the brute force's own counts"""
    assert len(SMALL_CASES) == 20 and not [k for k in G_SMALL.files if k.startswith('err_')]
    for n in (3, 4, 6, 255, 256, 257, 300):
        first, last = (bf.topology(small_inputs(f'wheel{n}_hub_{end}')[1].numpy(), n + 1) for end in ('first', 'last'))
        for tp, hub in ((first, 0), (last, n)):
            assert tp.E == 2 * n and tp.valence[hub] == n and sorted(tp.count.tolist()) == [1] * n + [2] * n
            assert all(tp.valence[v] == 3 for v in range(n + 1) if v != hub)
        assert first.runs[1, 0] - first.runs[0, 0] == n and last.runs[n + 1, 1] - last.runs[n, 1] == n     # edges | tlist
    tp = bf.topology(small_inputs('triangle')[1].numpy(), 3)
    assert tp.valence.tolist() == [2, 2, 2] and tp.count.tolist() == [1, 1, 1]
    tp = bf.topology(small_inputs('aba')[1].numpy(), 2)
    assert tp.edges.tolist() == [[0, 1], [1, 1]] and tp.count.tolist() == [2, 1] and tp.opp.tolist() == [[1, 1], [-1, -1]]
    assert tp.valence.tolist() == [1, 2] and tp.self_edges == 1 and tp.tlist.tolist() == [[0, 0], [1, 1]]
    tp = bf.topology(small_inputs('aaa')[1].numpy(), 1)
    assert tp.E == 1 and tp.count.tolist() == [3] and tp.valence.tolist() == [1] and tp.runs.tolist() == [[0, 0], [1, 1]]
    assert sorted(set(bf.topology(small_inputs('pair4')[1].numpy(), 4).count.tolist())) == [1, 3, 4]
    assert sorted(set(bf.topology(small_inputs('counts234')[1].numpy(), 5).count.tolist())) == [1, 2, 3, 4]
    tp = bf.topology(small_inputs('tet_gap')[1].numpy(), 5)
    assert tp.valence.tolist() == [3, 3, 0, 3, 3] and set(tp.count.tolist()) == {2}


@pytest.mark.parametrize('case', GRAD_CASES)
def test_bruteforce_gradients_match_reference(case):
    vertices, faces, alpha = case_inputs(case)
    steps, _, _ = iterate(vertices, faces, alpha, 2)
    gx, ga = tensor(f'grads_{case}_cot').numpy(), None
    for tp, x, a in reversed(steps):
        bw = bf.backward(tp, x, a, gx, ga)
        gx, ga = bw.dx, bw.da
    # (rounded to the records' float32: check_gradients sizes its accumulation slack by the dtype it is given, and the slack is
    # there for the float32 sums of the reference itself)
    check_gradients(case, torch.from_numpy(gx).float(), torch.from_numpy(ga).float())


def test_vectorised_twin_equals_plain():
    meshes = [small_inputs(case)[1:2] + (small_inputs(case)[0].shape[1],) for case in SMALL_CASES]
    meshes += [(case_inputs(case)[1], case_inputs(case)[0].shape[1]) for case in ('doc', 'ico', 'sphere6', 'open_messy')]
    meshes += [cases.mesh_for_keys(F) for F in cases.KEY_FACES[:4]] + [cases.mesh_for_edges(E) for E in cases.EDGE_COUNTS[:6]]
    meshes += [cases.mesh_for_id_width(V)[:2] for V in cases.ID_WIDTH_FULL]
    for faces, V in meshes:
        assert bf.same_topology(bf.topology(faces.numpy(), V), bf.topology_vectorised(faces.numpy(), V)), (tuple(faces.shape), V)
    faces, V, ids = cases.mesh_for_id_width(1 << 24)                    # no per-vertex arrays: the rows asked for
    plain, twin = bf.topology(faces.numpy(), V), bf.topology_vectorised(faces.numpy(), V)
    assert plain.runs is None and bf.same_topology(plain, twin)
    rows = [0, 1, 255, 256, 257, V - 1, V]
    assert np.array_equal(plain.runs_at(rows)[[0, -1]], [[0, 0], [81, 81]]) and plain.valence_at(rows[:-1]).sum() > 0


# ---- the package's CPU path against the brute force, at the shapes of the GPU boundary tests -----------------------------
def cpu_values(faces, V, B, label, tp, views=None):
    """float32 and float64, default and given alpha: the torch formulation's forward and autograd backward within the bounds; the
    public function returns the same rows, and its one-iteration autograd backward (alpha requiring a gradient, and alpha a
    constant) stays within them too.  `views`: a function that turns x and alpha into the views to pass."""
    for dtype in cases.DTYPES:
        x, alpha, gx, ga = cases.inputs(B, V, tp.E, dtype, seed=V + tp.E)
        if views is not None:
            x, alpha = views(x, alpha)
        for setting in cases.SETTINGS:
            a = alpha.clone().requires_grad_() if setting == 'alpha' else None
            p = x.clone().requires_grad_()
            new_x, new_faces, new_alpha = trianglemesh._torch_iteration(p, faces, a)
            assert torch.equal(new_faces, torch.from_numpy(tp.new_faces))
            cases.check_forward(tp, new_x.detach(), None if a is None else new_alpha.detach(), x, None if a is None else alpha,
                                f'cpu {label} {setting}')
            public = subdivide_trianglemesh(x, faces, 1, None if a is None else alpha)
            assert torch.equal(public[0], new_x.detach()) and torch.equal(public[1], new_faces)
            loss = (new_x * gx).sum() if a is None else (new_x * gx).sum() + (new_alpha * ga).sum()
            loss.backward()
            cases.check_backward(tp, p.grad, None if a is None else a.grad, x, None if a is None else alpha, gx,
                                 None if a is None else ga, f'cpu {label} {setting}')
            # one iteration of the public function under autograd: no cotangent reaches new_alpha
            p, q = x.clone().requires_grad_(), (None if a is None else alpha.clone().requires_grad_())
            (subdivide_trianglemesh(p, faces, 1, q)[0] * gx).sum().backward()
            cases.check_backward(tp, p.grad, None if q is None else q.grad, x, None if a is None else alpha, gx, None,
                                 f'cpu {label} {setting} autograd')
            if a is not None:                                           # alpha given, but a constant
                p = x.clone().requires_grad_()
                (subdivide_trianglemesh(p, faces, 1, alpha)[0] * gx).sum().backward()
                assert alpha.grad is None
                cases.check_backward(tp, p.grad, None, x, alpha, gx, None, f'cpu {label} constant alpha autograd')


def cpu_topology(faces, V, tp):
    new_faces, (lo, hi, proper, slot_edge, slot_opp, two, valence) = trianglemesh._torch_topology(faces, V)
    assert torch.equal(new_faces, torch.from_numpy(tp.new_faces))
    assert torch.equal(torch.stack((lo, hi), dim=1), torch.from_numpy(tp.edges))
    assert torch.equal(torch.bincount(slot_edge, minlength=tp.E).int(), torch.from_numpy(tp.count))
    assert torch.equal(two, torch.from_numpy(tp.count == 2)) and int((~proper).sum()) == tp.self_edges
    assert torch.equal(valence.int(), torch.from_numpy(tp.valence))


@pytest.mark.parametrize('F', cases.KEY_FACES)
def test_cpu_path_key_counts(F):
    faces, V = cases.mesh_for_keys(F)
    tp = bf.topology(faces.numpy(), V)
    assert 3 * faces.shape[0] == 3 * F == cases.KEY_COUNTS[cases.KEY_FACES.index(F)]
    cpu_topology(faces, V, tp)
    cpu_values(faces, V, 1, f'keys {3 * F}', tp)


@pytest.mark.parametrize('E', cases.EDGE_COUNTS)
def test_cpu_path_edge_counts(E):
    faces, V = cases.mesh_for_edges(E)
    tp = bf.topology(faces.numpy(), V)
    assert tp.E == E
    cpu_topology(faces, V, tp)
    cpu_values(faces, V, 1, f'edges {E}', tp)


@pytest.mark.parametrize('V', cases.ID_WIDTH_FULL)
def test_cpu_path_id_widths(V):
    faces, V, ids = cases.mesh_for_id_width(V)
    tp = bf.topology(faces.numpy(), V)
    assert tp.E == 81 and set(faces.reshape(-1).tolist()) == set(ids.tolist())
    assert {0, V - 1} | {s for s in cases.ID_WIDTH_SPECIAL if s < V} <= set(ids.tolist())
    cpu_topology(faces, V, tp)
    cpu_values(faces, V, 1, f'ids below {V}', tp)


@pytest.mark.parametrize('case', SMALL_CASES)
def test_cpu_path_small_cases(case):
    vertices, faces, _ = small_inputs(case)
    V = vertices.shape[1]
    tp = bf.topology(faces.numpy(), V)
    cpu_topology(faces, V, tp)
    cpu_values(faces, V, 1, case, tp)


@pytest.mark.parametrize('mesh', ['doc', 'wheel6'])
def test_cpu_path_batches(mesh):
    """The batches of the GPU test: every item different"""
    faces, V = (case_inputs('doc')[1], 4) if mesh == 'doc' else cases.wheel(6, seed=6)
    tp = bf.topology(faces.numpy(), V)
    for B in cases.BATCHES:
        cpu_values(faces, V, B, f'{mesh} B = {B}', tp)


@pytest.mark.parametrize('mesh', ['doc', 'wheel6'])
def test_cpu_path_expanded_batch(mesh):
    """1 025 items that are one item (batch stride 0)"""
    B = 1025
    faces, V = (case_inputs('doc')[1], 4) if mesh == 'doc' else cases.wheel(6, seed=6)
    tp = bf.topology(faces.numpy(), V)

    def expanded(x, alpha):
        x, alpha = x[:1].expand(B, -1, -1), alpha[:1].expand(B, -1)
        assert x.stride(0) == 0 and alpha.stride(0) == 0
        return x, alpha

    cpu_values(faces, V, B, f'{mesh} expanded', tp, views=expanded)
    for dtype in cases.DTYPES:
        x, alpha = expanded(*cases.inputs(B, V, tp.E, dtype, seed=V + tp.E)[:2])
        for a in (None, alpha):
            new_x = subdivide_trianglemesh(x, faces, 1, a)[0]
            assert torch.equal(new_x, new_x[:1].expand(B, -1, -1))


@pytest.mark.parametrize('mesh', ['wheel', 'counts234'])
def test_cpu_path_one_iteration_backward(mesh):
    """The meshes of the GPU test of the same name: B = 2; cpu_values runs the public function's one-iteration backward with
    alpha requiring a gradient and with alpha a constant"""
    faces, V = cases.wheel(7, hub_last=True, seed=3) if mesh == 'wheel' else (small_inputs('counts234')[1], 5)
    tp = bf.topology(faces.numpy(), V)
    assert int((tp.count == 2).sum()) > 0
    cpu_topology(faces, V, tp)
    cpu_values(faces, V, 2, f'{mesh} one iteration', tp)


# ---- the radix passes the id widths need: host arithmetic ---------------------------------------------------------------------
def lsd_sorted(keys, passes):
    """keys (n) uint64 through `passes` stable 8-bit passes over the low half, then as many over the high half"""
    for half in range(2):
        for p in range(passes):
            digit = (keys >> np.uint64(32 * half + 8 * p)) & np.uint64(255)
            keys = keys[np.argsort(digit, kind='stable')]
    return keys


def test_pass_count_sorts_the_id_width_keys(tmp_path):
    """The pass count the pipeline uses, st_passes_per_half as csrc/subdivide_trianglemesh_host.h includes it (from
    subdivide_tetmesh_host.h; compiled here as it stands, with the host compiler), sorts the keys of the id-width meshes, and one pass fewer does not where the widest id needs the last pass: a pass count that is one short at 257,
    65 537 or 2^24 + 1 fails here, without a GPU, and in the GPU test of the same meshes."""
    compiler = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert compiler is not None, 'no host C++ compiler'
    source = tmp_path / 'passes.cpp'
    source.write_text(f'#include "{ROOT}/kaolin_amd/csrc/subdivide_trianglemesh_host.h"\n'
                      'extern "C" int passes(long long V) { return st_passes_per_half(V); }\n')
    lib = tmp_path / 'passes.so'
    subprocess.run([compiler, '-std=c++17', '-shared', '-fPIC', str(source), '-o', str(lib)], check=True)
    passes = ctypes.CDLL(str(lib)).passes
    passes.argtypes, passes.restype = [ctypes.c_longlong], ctypes.c_int
    for V in cases.ID_WIDTH_FULL + cases.ID_WIDTH_TOPOLOGY:
        faces, _, ids = cases.mesh_for_id_width(V)
        f = faces.numpy().astype(np.uint64)
        p, q = f.reshape(-1), np.roll(f, -1, axis=1).reshape(-1)
        keys = (np.minimum(p, q) << np.uint64(32)) | np.maximum(p, q)
        assert np.array_equal(lsd_sorted(keys, passes(V)), np.sort(keys)), f'{passes(V)} passes per half do not sort ids below {V}'
        assert passes(V) == cases.passes_per_half(V), V
        if passes(V) > passes(V - 1):                                     # V - 1 is the first id to need the last pass
            assert not np.array_equal(lsd_sorted(keys, passes(V) - 1), np.sort(keys)), V
    assert [passes(V) for V in cases.ID_WIDTH_FULL + cases.ID_WIDTH_TOPOLOGY] == [1, 2, 2, 3, 3, 4]
