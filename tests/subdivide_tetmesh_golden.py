"""What test_subdivide_tetmesh_cpu.py and test_subdivide_tetmesh_gpu.py share: the reference's recorded answers
(tests/golden/subdivide_tetmesh.npz, written by make_golden_subdivide_tetmesh.py) decoded into inputs and expected tensors."""
import os

import numpy as np
import torch

from conftest import GOLDEN_DIR
from kaolin_amd.utils.testing import kuhn_grid

G = np.load(os.path.join(GOLDEN_DIR, 'subdivide_tetmesh.npz'))
MT = np.load(os.path.join(GOLDEN_DIR, 'marching_tetrahedra.npz'))     # grid9's topology and item 0, the id map of sparse_ids
DTYPES = [('f32', torch.float32), ('f64', torch.float64)]
CASES = ['doc', 'kat1', 'kat2', 'grid9', 'sparse_ids']
SPARSE_V, SPARSE_T = 70001, 1500


def tensor(name):
    return torch.from_numpy(G[name])


def child_blocks(tets, slots):
    """new_tetrahedrons from the corners (a b c d) and the new ids (ab ac ad bc bd cd) of every tet: eight blocks of T rows (the
    generator asserts that this rebuilds the reference's result from the ``slot_ids`` it stores; it is a copy of
    make_golden_subdivide_tetmesh.py::child_blocks: keep the two in step)."""
    a, b, c, d = tets.unbind(1)
    ab, ac, ad, bc, bd, cd = slots.unbind(1)
    rows = ((a, ab, ac, ad), (b, bc, ab, bd), (c, ac, bc, cd), (d, ad, cd, bd),
            (ab, ac, ad, bd), (ab, ac, bd, bc), (cd, ac, bd, ad), (cd, ac, bc, bd))
    return torch.cat([torch.stack(r, dim=1) for r in rows], dim=0)


def case_inputs(case):
    """-> vertices (B, V, 3) float32, tets (T, 4) int64, features (B, V, D) float32"""
    if case in ('grid9', 'sparse_ids'):
        vertices = torch.stack([torch.from_numpy(MT['grid9_vertices'])[0], kuhn_grid(9)[0]])
        tets, features = torch.from_numpy(MT['grid9_tets']), tensor('grid9_features')
        if case == 'grid9':
            return vertices, tets, features
        ids = torch.from_numpy(MT['sparse_ids_map'])
        sv, sf = torch.zeros(1, SPARSE_V, 3), torch.zeros(1, SPARSE_V, 5)
        sv[0, ids], sf[0, ids] = vertices[1], features[0]
        return sv, torch.from_numpy(MT['sparse_ids_tets'])[:SPARSE_T], sf
    return tensor(f'{case}_vertices'), tensor(f'{case}_tets'), tensor(f'{case}_features')


def expected(case, tag, dtype):
    """-> the reference's new_vertices, new_tetrahedrons, new_features for case_inputs(case) in `dtype`"""
    vertices, tets, features = case_inputs(case)
    new_vertices = torch.cat([vertices.to(dtype), tensor(f'{case}_mid_vertices_{tag}')], dim=1)
    new_features = torch.cat([features.to(dtype), tensor(f'{case}_mid_features_{tag}')], dim=1)
    if f'{case}_new_tets' in G:
        return new_vertices, tensor(f'{case}_new_tets'), new_features
    return new_vertices, child_blocks(tets, tensor(f'{case}_slot_ids').long()), new_features


def unused_cotangent(rows, channels):
    """The generator's rule for the cotangent rows of the sparse_ids vertices nobody uses."""
    r = torch.arange(rows, dtype=torch.long).unsqueeze(1)
    c = torch.arange(channels, dtype=torch.long).unsqueeze(0)
    return ((r * 7 + c * 3) % 17 - 8).float() / 8


def cotangents(case):
    """-> the cotangents of new_vertices and new_features the recorded gradients were taken under"""
    cot_v, cot_f = tensor(f'grads_{case}_cot_vertices'), tensor(f'grads_{case}_cot_features')
    if case != 'sparse_ids':
        return cot_v, cot_f
    ids = torch.from_numpy(MT['sparse_ids_map'])
    full = []
    for used, channels in ((cot_v, 3), (cot_f, 5)):
        c = torch.cat([unused_cotangent(SPARSE_V, channels)[None], used[:, 1000:]], dim=1)
        c[0, ids] = used[0, :1000]
        full.append(c)
    return full


def same(a, b):
    """dtype, shape and every bit-pattern class equal (NaN matches NaN)"""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=12345.), torch.nan_to_num(b, nan=12345.))


def check_gradients(case, tag, grad_vertices, grad_features, cot_v, cot_f, verbose=False):
    """Recorded gradients within elementwise_mismatch(tol=1e-5, term_abs_sum=...); for sparse_ids the rows of the unused ids must
    be exactly the pass-through cotangent."""
    from kaolin_amd.utils.testing import elementwise_mismatch
    grad_vertices, grad_features = grad_vertices.cpu(), grad_features.cpu()
    if case == 'sparse_ids':
        ids = torch.from_numpy(MT['sparse_ids_map'])
        rest = torch.ones(SPARSE_V, dtype=torch.bool)
        rest[ids] = False
        assert torch.equal(grad_vertices[0, rest], cot_v[0, :SPARSE_V][rest].to(grad_vertices.dtype))
        assert torch.equal(grad_features[0, rest], cot_f[0, :SPARSE_V][rest].to(grad_features.dtype))
        grad_vertices, grad_features = grad_vertices[:, ids], grad_features[:, ids]
    for got, name in ((grad_vertices, 'vertices'), (grad_features, 'features')):
        msg = elementwise_mismatch(got, tensor(f'grads_{case}_{name}_{tag}'), tol=1e-5, term_abs_sum=tensor(f'grads_{case}_{name}_tas'))
        if verbose:
            print(case, tag, name, 'slack use', elementwise_mismatch.last_slack_use, msg)
        assert msg is None, msg
