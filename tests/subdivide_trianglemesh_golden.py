"""What the subdivide_trianglemesh test files share: the reference's recorded answers (tests/golden/subdivide_trianglemesh.npz
and, for the small meshes at the bottom, subdivide_trianglemesh_edges.npz; both written by
make_golden_subdivide_trianglemesh.py) decoded into inputs and expected tensors.  The reference computes in float32 and for one
item at a time; every record is float32."""
import os

import numpy as np
import torch

from conftest import GOLDEN_DIR

G = np.load(os.path.join(GOLDEN_DIR, 'subdivide_trianglemesh.npz'))
SPARSE_V = 70001
# (case, iterations) of every recorded forward; both settings ('default': no alpha, 'alpha': the case's alpha) are recorded
FORWARD_CASES = [('doc', 1), ('ico', 1), ('sphere6', 1), ('sphere6', 2), ('open_messy', 2), ('sparse_ids', 1)]
SETTINGS = ['default', 'alpha']
GRAD_CASES = ['sphere6', 'open_messy']


def tensor(name):
    t = torch.from_numpy(G[name])
    return t if t.is_floating_point() else t.long()


def child_faces(faces, slots):
    """new faces from the corners (a b c) and the new ids (ab bc ca) of every face: four consecutive rows per face (the generator
    asserts that this rebuilds the reference's result from the ``slots`` it stores; it is a copy of
    make_golden_subdivide_trianglemesh.py::child_faces: keep the two in step)."""
    a, b, c = faces.unbind(1)
    ab, bc, ca = slots.unbind(1)
    return torch.stack((b, bc, ab, a, ab, ca, c, ca, bc, ca, ab, bc), dim=1).reshape(-1, 3)


def unused_rows(rows, channels):
    """The generator's rule for the values of the sparse_ids vertices nobody uses."""
    r = torch.arange(rows, dtype=torch.long).unsqueeze(1)
    c = torch.arange(channels, dtype=torch.long).unsqueeze(0)
    return ((r * 7 + c * 3) % 17 - 8).float() / 8


_INPUTS = {}


def case_inputs(case):
    """-> vertices (B, V, 3) float32, faces (F, 3) int64, alpha (B, V) float32 (computed once; do not modify)"""
    if case not in _INPUTS:
        if case == 'open_messy':
            vertices, _, alpha = case_inputs('sphere6')
            _INPUTS[case] = (vertices[:1], tensor('open_messy_faces'), alpha[:1])
        elif case == 'sparse_ids':
            vertices, faces, alpha = case_inputs('sphere6')
            ids = tensor('sparse_ids_map')
            pv, pa = unused_rows(SPARSE_V, 3)[None].clone(), unused_rows(SPARSE_V, 1)[None, :, 0].abs().clone()
            pv[0, ids], pa[0, ids] = vertices[1], alpha[0]
            _INPUTS[case] = (pv, ids[faces], pa)
        else:
            _INPUTS[case] = (tensor(f'{case}_vertices'), tensor(f'{case}_faces'), tensor(f'{case}_alpha'))
    return _INPUTS[case]


def expected_faces(case, iterations):
    """-> the reference's new faces after `iterations` iterations, rebuilt from the recorded slots"""
    faces = case_inputs(case)[1]
    for i in range(1, iterations + 1):
        faces = child_faces(faces, tensor(f'{case}_slots_{i}'))
    return faces


def split_rows(case, new_vertices):
    """new_vertices of a call on case_inputs(case) -> (the rows the reference recorded, the other rows or None, what the other
    rows must be): for sparse_ids the rows of the unused ids are not recorded (the reference returns NaN there); they must be the
    inputs, bit for bit."""
    if case != 'sparse_ids':
        return new_vertices, None, None
    ids = tensor('sparse_ids_map')
    rest = torch.ones(SPARSE_V, dtype=torch.bool)
    rest[ids] = False
    recorded = torch.cat([new_vertices[:, ids], new_vertices[:, SPARSE_V:]], dim=1)
    return recorded, new_vertices[:, :SPARSE_V][:, rest], case_inputs(case)[0][:, rest]


def check_forward(case, iterations, setting, new_vertices, new_faces, tol=1e-5, verbose=False):
    """faces with torch.equal, float rows within elementwise_mismatch(tol) of the float32 records, unused rows passed through"""
    from kaolin_amd.utils.testing import elementwise_mismatch
    new_vertices, new_faces = new_vertices.detach().cpu(), new_faces.cpu()
    assert new_faces.dtype == torch.long and torch.equal(new_faces, expected_faces(case, iterations)), (case, iterations)
    recorded, rest, want_rest = split_rows(case, new_vertices)
    if rest is not None:
        assert torch.equal(rest, want_rest.to(rest.dtype))
    want = tensor(f'{case}_{setting}_{iterations}_vertices')
    assert not bool(torch.isnan(want).any())
    msg = elementwise_mismatch(recorded, want, tol=tol)
    if verbose:
        print(case, iterations, setting, 'max abs diff', float((recorded.double() - want.double()).abs().max()), msg)
    assert msg is None, msg


# ---- the second file: small meshes at the valences and edge counts the first has none of (one iteration, B = 1) ----------------
G_SMALL = np.load(os.path.join(GOLDEN_DIR, 'subdivide_trianglemesh_edges.npz'))
SMALL_CASES = [name[:-len('_faces')] for name in G_SMALL.files if name.endswith('_faces')]


def small_inputs(case):
    """-> vertices (1, V, 3) float32, faces (F, 3) int64, alpha (1, V) float32 of a case of the second file"""
    return (torch.from_numpy(G_SMALL[f'{case}_vertices']), torch.from_numpy(G_SMALL[f'{case}_faces']).long(),
            torch.from_numpy(G_SMALL[f'{case}_alpha']))


def check_small_forward(case, setting, new_vertices, new_faces, tol=1e-5):
    """check_forward for a case of the second file: the faces, and every row the reference defines (it returns NaN for the row of
    an unused id: those rows are marked, not recorded, and must be the inputs, bit for bit) -> the number of rows compared"""
    from kaolin_amd.utils.testing import elementwise_mismatch
    assert f'err_{case}_{setting}' not in G_SMALL.files                   # (the reference raised for none of them)
    vertices, faces, _ = small_inputs(case)
    new_vertices, new_faces = new_vertices.detach().cpu(), new_faces.cpu()
    slots = torch.from_numpy(G_SMALL[f'{case}_slots_1']).long()
    assert new_faces.dtype == torch.long and torch.equal(new_faces, child_faces(faces, slots)), case
    want = torch.from_numpy(G_SMALL[f'{case}_{setting}_1_vertices'])
    defined = torch.ones(want.shape[1], dtype=torch.bool)
    if f'{case}_{setting}_1_nanrows' in G_SMALL.files:
        defined = ~torch.from_numpy(G_SMALL[f'{case}_{setting}_1_nanrows'])
        rest = torch.nonzero(~defined).reshape(-1)
        assert int(rest.max()) < vertices.shape[1] and torch.equal(new_vertices[:, rest], vertices[:, rest].to(new_vertices.dtype))
    assert not bool(torch.isnan(want).any())
    msg = elementwise_mismatch(new_vertices[:, defined], want[:, defined], tol=tol)
    assert msg is None, (case, setting, msg)
    return int(defined.sum())


def check_gradients(case, grad_vertices, grad_alpha, verbose=False):
    """Recorded gradients within elementwise_mismatch(tol=1e-5, term_abs_sum=...)"""
    from kaolin_amd.utils.testing import elementwise_mismatch
    for got, name in ((grad_vertices, 'vertices'), (grad_alpha, 'alpha')):
        msg = elementwise_mismatch(got.cpu(), tensor(f'grads_{case}_{name}'), tol=1e-5, term_abs_sum=tensor(f'grads_{case}_{name}_tas'))
        if verbose:
            print(case, name, 'slack use', elementwise_mismatch.last_slack_use, msg)
        assert msg is None, msg
