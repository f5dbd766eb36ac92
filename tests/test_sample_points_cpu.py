"""ops.mesh.face_areas / sample_points without a GPU: the numpy oracle (tests/sample_points_bruteforce.py) and the package's torch
formulation against what the reference recorded (tests/golden/sample_points.npz, written by make_golden_sample_points.py), the
reference's own TestFaceAreas / TestSamplePoints restated on that file's data, the draw contract, and the argument checks."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR
import kaolin_amd as kal
from kaolin_amd.ops import mesh
from kaolin_amd.ops.mesh import sampling
from kaolin_amd.utils.testing import check_allclose, check_tensor, with_seed
import sample_points_bruteforce as oracle

G = np.load(os.path.join(GOLDEN_DIR, 'sample_points.npz'))
DTYPES = [('f32', torch.float32), ('f64', torch.float64)]
NAMES = ['face_areas', 'packed_face_areas', 'sample_points', 'packed_sample_points']


def tensor(name, dtype=None):
    t = torch.from_numpy(G[name])
    return t if dtype is None else t.to(dtype)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=12345.), torch.nan_to_num(b, nan=12345.))


def test_exported():
    assert all(name in mesh.__all__ and callable(getattr(mesh, name)) for name in NAMES)
    assert sampling.__all__ == NAMES
    assert kal.ops.mesh.sample_points is sampling.sample_points


# ---- areas ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_areas_of_the_reference_tables(tag, dtype):
    vertices, faces = tensor('tables_areas_vertices', dtype), tensor('tables_areas_faces')
    got = mesh.face_areas(vertices, faces)
    assert same(got, tensor(f'tables_areas_out_{tag}')) and torch.equal(got, tensor(f'tables_areas_expected_{tag}'))   # its torch.equal
    assert np.array_equal(oracle.face_areas(vertices.numpy(), faces.numpy()), G[f'tables_areas_out_{tag}'])
    packed = mesh.packed_face_areas(tensor('tables_packed_vertices', dtype), tensor('tables_packed_first_idx_vertices'),
                                    tensor('tables_packed_faces'), tensor('tables_packed_num_faces_per_mesh'))
    assert same(packed, tensor(f'tables_packed_out_{tag}'))
    check_allclose(packed, tensor(f'tables_packed_expected_{tag}'))                                                  # its check_allclose


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_areas_of_the_icosphere(tag, dtype):
    vertices, faces = tensor('ico_vertices', dtype), tensor('ico_faces')
    want = tensor(f'ico_areas_{tag}')
    assert float(want[0, 100]) == 0.0                                               # the degenerate face
    assert same(mesh.face_areas(vertices, faces), want)
    assert same(mesh.face_areas(vertices, faces.int()), want)                       # another id dtype: the torch formulation
    packed = mesh.packed_face_areas(tensor('ico_packed_vertices', dtype), tensor('ico_packed_first_idx_vertices'), faces,
                                    tensor('ico_packed_num_faces_per_mesh'))
    assert same(packed, tensor(f'ico_packed_areas_{tag}'))
    # with the correctly rounded root (the contract): the oracle and the torch formulation, every face
    ieee = tensor(f'ico_areas_ieee_{tag}')
    assert int((ieee != want).sum()) <= 0.02 * want.numel() and torch.allclose(ieee, want, rtol=4 * torch.finfo(dtype).eps, atol=0)
    assert np.array_equal(oracle.face_areas(vertices.numpy(), faces.numpy()), G[f'ico_areas_ieee_{tag}'])
    assert same(sampling.face_areas_torch(vertices, faces, sqrt=oracle.ieee_sqrt), ieee)
    merged = faces + torch.repeat_interleave(tensor('ico_packed_first_idx_vertices')[:-1], tensor('ico_packed_num_faces_per_mesh'))[:, None]
    assert np.array_equal(oracle.face_areas(G['ico_packed_vertices'].astype(G[f'ico_areas_{tag}'].dtype)[None], merged.numpy())[0],
                          G[f'ico_packed_areas_ieee_{tag}'])


# ---- the blend --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_blend_matches_the_reference(tag, dtype):
    vertices, faces, feats = tensor('ico_vertices', dtype), tensor('ico_faces'), tensor('blend_features', dtype)
    choices = tensor('blend_choices')
    uv = torch.stack([tensor(f'blend_u_{tag}'), tensor(f'blend_v_{tag}')], dim=-1)
    assert uv.dtype == dtype
    points = oracle.points_of(vertices.numpy(), faces.numpy(), choices.numpy(), uv.numpy())
    features = oracle.features_of(feats.numpy(), choices.numpy(), uv.numpy())
    assert points.dtype == G[f'blend_points_{tag}'].dtype and np.array_equal(points, G[f'blend_points_ieee_{tag}'])
    assert np.array_equal(features, G[f'blend_feats_ieee_{tag}'])
    corners = [torch.gather(c, 1, choices.unsqueeze(-1).expand(-1, -1, 3)) for c in sampling._face_corners(vertices, faces)]
    chosen = torch.gather(feats, 1, choices[..., None, None].expand(-1, -1, 3, feats.shape[-1]))
    for root, kind in ((torch.sqrt, ''), (oracle.ieee_sqrt, '_ieee')):       # as the reference stands / with the contract's root
        assert same(sampling.blend_torch(uv, *corners, sqrt=root), tensor(f'blend_points{kind}_{tag}'))
        assert same(sampling.blend_torch(uv, chosen[:, :, 0], chosen[:, :, 1], chosen[:, :, 2], sqrt=root), tensor(f'blend_feats{kind}_{tag}'))
    assert int((G[f'blend_points_{tag}'] != G[f'blend_points_ieee_{tag}']).sum()) <= 0.03 * points.size


def test_operator_reproduces_the_blend_through_its_own_choice():
    """r placed in the middle of the chosen face's cdf interval makes the operator choose the recorded faces"""
    vertices, faces, choices = tensor('ico_vertices', torch.float64), tensor('ico_faces'), tensor('blend_choices').clone()
    areas = tensor('ico_areas_f64')
    choices[choices == 100] = 99                                                    # (the degenerate face cannot be chosen)
    cdf = torch.cumsum(areas, 1)
    lower = torch.cat([torch.zeros(2, 1, dtype=torch.float64), cdf[:, :-1]], 1)
    r = (torch.gather(lower, 1, choices) + torch.gather(cdf, 1, choices)) / 2 / cdf[:, -1:]
    uv = torch.stack([tensor('blend_u_f64'), tensor('blend_v_f64')], dim=-1)
    points, got, features = sampling.sample_points_torch(vertices, faces, None, r, uv, tensor('blend_features', torch.float64),
                                                         sqrt=oracle.ieee_sqrt)
    assert torch.equal(got, choices)
    res = oracle.sample_points(vertices.numpy(), faces.numpy(), r.numpy(), uv.numpy(), face_features=G['blend_features'].astype(np.float64))
    assert np.array_equal(res['choices'], choices.numpy()) and np.array_equal(res['points'], points.numpy())
    assert np.array_equal(res['features'], features.numpy()) and float(res['margin'].min()) > 1
    keep = tensor('blend_choices') != 100
    assert torch.equal(points[keep], tensor('blend_points_ieee_f64')[keep])
    assert torch.equal(features[keep], tensor('blend_feats_ieee_f64')[keep])


# ---- gradients ----------------------------------------------------------------------------------------------------------------------
def test_area_gradients_match_the_reference():
    p = tensor('ico_vertices', torch.float64).requires_grad_()
    (mesh.face_areas(p, tensor('ico_faces')) * tensor('grads_areas_cot')).sum().backward()
    assert same(p.grad, tensor('grads_areas_vertices')) and bool(torch.isnan(p.grad).any())


def test_blend_gradients_match_the_reference():
    """the float64 autograd of the torch formulation at the recorded choices and draws"""
    p, q = tensor('ico_vertices', torch.float64).requires_grad_(), tensor('blend_features', torch.float64).requires_grad_()
    faces, choices = tensor('ico_faces'), tensor('blend_choices')
    uv = torch.stack([tensor('blend_u_f64'), tensor('blend_v_f64')], dim=-1)
    corners = [torch.gather(c, 1, choices.unsqueeze(-1).expand(-1, -1, 3)) for c in sampling._face_corners(p, faces)]
    chosen = torch.gather(q, 1, choices[..., None, None].expand(-1, -1, 3, 2))
    loss = (sampling.blend_torch(uv, *corners) * tensor('grads_blend_cot_points')).sum() + \
        (sampling.blend_torch(uv, chosen[:, :, 0], chosen[:, :, 1], chosen[:, :, 2]) * tensor('grads_blend_cot_feats')).sum()
    loss.backward()
    check_allclose(p.grad, tensor('grads_blend_vertices'), rtol=1e-13, atol=1e-13)
    check_allclose(q.grad, tensor('grads_blend_features'), rtol=1e-13, atol=1e-13)


def test_nothing_flows_through_the_areas():
    vertices, faces = tensor('cases_vertices', torch.float64).requires_grad_(), tensor('cases_faces')
    areas = mesh.face_areas(vertices.detach(), faces).requires_grad_()
    points, choices = mesh.sample_points(vertices, faces, 50, areas)
    assert points.requires_grad and not choices.requires_grad
    points.sum().backward()
    assert areas.grad is None and bool(vertices.grad.abs().sum() > 0)


# ---- the reference's TestSamplePoints, restated on its recorded fixtures ----------------------------------------------------------
def _calls(name, tag, use_features):
    rows = [row for row in G['cases_calls'] if row[0] == name and row[1] == tag and row[3] == str(int(use_features))]
    assert len(rows) == 1
    return int(rows[0][2]), [x for x in rows[0][4:] if x]


def _check_like_recorded(results, recorded):
    assert len(results) == len(recorded)
    for got, want in zip(results, recorded):
        assert f'{tuple(got.shape)}:{str(got.dtype).replace("torch.", "")}' == want


def _on_face_and_inside(points, face_vertices_choices, dtype):
    batch_size, num_samples = points.shape[:2]
    face_normals = mesh.face_normals(face_vertices_choices, unit=True)
    v0_p = points - face_vertices_choices[:, :, 0]
    dist = torch.matmul(v0_p.reshape(-1, 1, 3), face_normals.reshape(-1, 3, 1)).reshape(batch_size, num_samples)
    check_allclose(dist, torch.zeros((batch_size, num_samples), dtype=dtype), atol=1e-4, rtol=1e-5)
    for k in range(3):
        edge = face_vertices_choices[:, :, (k + 1) % 3] - face_vertices_choices[:, :, k]
        normal = torch.cross(edge, points - face_vertices_choices[:, :, k], dim=-1)
        assert torch.all(torch.matmul(normal.reshape(-1, 1, 3), face_normals.reshape(-1, 3, 1)) >= 0.)


@pytest.mark.parametrize('use_features', [False, True])
@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_reference_sample_points(tag, dtype, use_features):
    vertices, faces, face_features = tensor('cases_vertices', dtype), tensor('cases_faces'), tensor('cases_face_features', dtype)
    num_samples, recorded = _calls('sample_points', tag, use_features)
    batch_size = vertices.shape[0]
    torch.manual_seed(11)
    out = mesh.sample_points(vertices, faces, num_samples, face_features=face_features) if use_features else \
        mesh.sample_points(vertices, faces, num_samples)
    _check_like_recorded(out, recorded)
    points, face_choices = out[:2]
    check_tensor(points, shape=(batch_size, num_samples, 3), dtype=dtype, device='cpu')
    check_tensor(face_choices, shape=(batch_size, num_samples), dtype=torch.long, device='cpu')
    num_0 = torch.sum(face_choices == 0, dim=1)
    assert torch.all(num_0 + torch.sum(face_choices == 1, dim=1) == num_samples)
    sampling_prob = num_samples / 2
    tolerance = sampling_prob * 0.2
    assert torch.all(num_0 < sampling_prob + tolerance) and torch.all(num_0 > sampling_prob - tolerance)
    face_vertices = mesh.index_vertices_by_faces(vertices, faces)
    chosen = torch.gather(face_vertices, 1, face_choices[:, :, None, None].repeat(1, 1, 3, 3))
    _on_face_and_inside(points, chosen, dtype)
    if use_features:
        feat_dim = face_features.shape[-1]
        check_tensor(out[2], shape=(batch_size, num_samples, feat_dim), dtype=dtype, device='cpu')
        ax, ay, bx, by = chosen[:, :, 0, 0], chosen[:, :, 0, 1], chosen[:, :, 1, 0], chosen[:, :, 1, 1]
        cx, cy = chosen[:, :, 2, 0], chosen[:, :, 2, 1]
        m, p, n, q = bx - ax, by - ay, cx - ax, cy - ay
        s, t = points[:, :, 0] - ax, points[:, :, 1] - ay
        k1, k2, k3 = s * q - n * t, m * t - s * p, m * q - n * p
        w1, w2 = k1 / (k3 + 1e-7), k2 / (k3 + 1e-7)
        weights = torch.stack([(1. - w1) - w2, w1, w2], dim=-1)
        check_allclose(points, torch.sum(chosen * weights.unsqueeze(-1), dim=-2), atol=1e-4, rtol=1e-5)
        chosen_features = torch.gather(face_features, 1, face_choices[..., None, None].repeat(1, 1, 3, feat_dim))
        check_allclose(out[2], torch.sum(chosen_features * weights.unsqueeze(-1), dim=-2), atol=1e-4, rtol=1e-5)


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_reference_with_areas_and_other_seed(tag, dtype):
    vertices, faces, face_features = tensor('cases_vertices', dtype), tensor('cases_faces'), tensor('cases_face_features', dtype)
    areas = mesh.face_areas(vertices, faces)
    one = with_seed(1234)(mesh.sample_points)(vertices, faces, 1000, areas)
    two = with_seed(1234)(mesh.sample_points)(vertices, faces, 1000)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])
    one = with_seed(1234)(mesh.sample_points)(vertices, faces, 1000, areas, face_features=face_features)
    two = with_seed(1234)(mesh.sample_points)(vertices, faces, 1000, face_features=face_features)
    assert all(torch.equal(a, b) for a, b in zip(one, two)) and len(one) == 3
    other = with_seed(1235)(mesh.sample_points)(vertices, faces, 1000)
    assert not torch.equal(two[0], other[0]) and not torch.equal(two[1], other[1])


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_reference_packed_sample_points(tag, dtype):
    vertices, first_idx = tensor('cases_packed_vertices', dtype), tensor('cases_packed_first_idx_vertices')
    faces, num_faces = tensor('cases_packed_faces'), tensor('cases_packed_num_faces_per_mesh')
    num_samples, recorded = _calls('packed_sample_points', tag, False)
    torch.manual_seed(12)
    points, face_choices = mesh.packed_sample_points(vertices, first_idx, faces, num_faces, num_samples)
    _check_like_recorded((points, face_choices), recorded)
    assert torch.all(face_choices[1] == 2)                                          # merged indices
    num_0 = torch.sum(face_choices[0] == 0)
    assert num_0 + torch.sum(face_choices[0] == 1) == num_samples
    sampling_prob = num_samples / 3.
    assert sampling_prob * 0.8 < num_0 < sampling_prob * 1.2
    merged = faces + torch.repeat_interleave(first_idx[:-1], num_faces).unsqueeze(1)
    face_vertices = vertices[merged.reshape(-1)].reshape(-1, 3, 3)
    chosen = face_vertices[face_choices.reshape(-1)].reshape(2, num_samples, 3, 3)
    _on_face_and_inside(points, chosen, dtype)
    areas = mesh.packed_face_areas(vertices, first_idx, faces, num_faces)
    one = with_seed(1234)(mesh.packed_sample_points)(vertices, first_idx, faces, num_faces, 1000, areas)
    two = with_seed(1234)(mesh.packed_sample_points)(vertices, first_idx, faces, num_faces, 1000)
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])


# ---- the contract -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,dtype', DTYPES + [('bf16', torch.bfloat16)])
def test_draw_contract(tag, dtype):
    """seeding, drawing r and uv by hand and calling the operator equals sample_points under the same seed"""
    vertices, faces = tensor('ico_vertices', dtype), tensor('ico_faces')
    feats = tensor('blend_features', dtype)
    torch.manual_seed(99)
    points, choices, features = mesh.sample_points(vertices, faces, 300, face_features=feats)
    torch.manual_seed(99)
    r = torch.rand((2, 300), dtype=torch.float64)
    uv = torch.rand((2, 300, 2), dtype=dtype)
    want = sampling.sample_points_torch(vertices, faces, None, r, uv, feats)
    assert same(points, want[0]) and same(choices, want[1]) and same(features, want[2]) and points.dtype == dtype
    assert not bool((choices == 100).any())
    if dtype != torch.bfloat16:
        points, choices, features = sampling.sample_points_torch(vertices, faces, None, r, uv, feats, sqrt=oracle.ieee_sqrt)
        res = oracle.sample_points(vertices.numpy(), faces.numpy(), r.numpy(), uv.numpy(), face_features=feats.numpy())
        assert float(res['margin'].min()) > 1 and np.array_equal(res['choices'], choices.numpy())
        assert np.array_equal(res['points'], points.numpy()) and np.array_equal(res['features'], features.numpy())


def test_items_without_area_and_no_samples():
    vertices, faces = tensor('ico_vertices', torch.float32), tensor('ico_faces')
    areas = mesh.face_areas(vertices, faces)
    areas[1] = 0
    points, choices, features = mesh.sample_points(vertices, faces, 40, areas, tensor('blend_features'))
    assert bool(torch.isnan(points[1]).all()) and bool(torch.isnan(features[1]).all()) and bool((choices[1] == 0).all())
    assert bool(torch.isfinite(points[0]).all()) and bool(torch.isfinite(features[0]).all())
    points, choices, features = mesh.sample_points(vertices.double(), faces, 0, face_features=tensor('blend_features', torch.float64))
    assert points.shape == (2, 0, 3) and points.dtype == torch.float64 and choices.shape == (2, 0) and choices.dtype == torch.long
    assert features.shape == (2, 0, 2) and features.dtype == torch.float64
    points, choices = mesh.packed_sample_points(tensor('cases_packed_vertices'), tensor('cases_packed_first_idx_vertices'),
                                                tensor('cases_packed_faces'), tensor('cases_packed_num_faces_per_mesh'), 0)
    assert points.shape == (2, 0, 3) and choices.shape == (2, 0)


def test_argument_errors():
    vertices, faces = tensor('cases_vertices'), tensor('cases_faces')
    quads = torch.zeros((2, 4), dtype=torch.long)
    for name, call in (('face_areas', lambda: mesh.face_areas(vertices, quads)),
                       ('packed_face_areas', lambda: mesh.packed_face_areas(vertices[0], torch.LongTensor([0, 4]), quads, torch.LongTensor([2]))),
                       ('sample_points', lambda: mesh.sample_points(vertices, quads, 10)),
                       ('packed_sample_points', lambda: mesh.packed_sample_points(vertices[0], torch.LongTensor([0, 4]), quads,
                                                                                  torch.LongTensor([2]), 10))):
        with pytest.raises(NotImplementedError, match=f'^{name} is only implemented for triangle meshes$'):
            call()
    bad = [lambda: mesh.face_areas(vertices[0], faces), lambda: mesh.face_areas(vertices[..., :2], faces),
           lambda: mesh.face_areas(vertices, faces[None]), lambda: mesh.face_areas(vertices, faces.float()),
           lambda: mesh.face_areas(vertices, faces[:0]), lambda: mesh.face_areas(vertices.long(), faces),
           lambda: mesh.sample_points(vertices, faces, -1), lambda: mesh.sample_points(vertices, faces, 2.5),
           lambda: mesh.sample_points(vertices, faces, 10, areas=torch.ones(2, 3)),
           lambda: mesh.sample_points(vertices, faces, 10, areas=torch.ones(2, 2, dtype=torch.long)),
           lambda: mesh.sample_points(vertices, faces, 10, face_features=torch.ones(2, 2, 2, 5)),
           lambda: mesh.sample_points(vertices, faces, 10, face_features=torch.ones(2, 2, 3)),
           lambda: mesh.packed_sample_points(vertices[0], torch.LongTensor([0, 4]), faces, torch.LongTensor([1]), 10),
           lambda: mesh.packed_sample_points(vertices[0], torch.LongTensor([0, 9]), faces, torch.LongTensor([2]), 10),
           lambda: mesh.packed_sample_points(vertices[0], torch.LongTensor([0, 4]), faces, torch.LongTensor([2]), 10, areas=torch.ones(3)),
           lambda: mesh.packed_face_areas(vertices[0], torch.LongTensor([0, 2, 4]), faces, torch.LongTensor([2]))]
    for call in bad:
        with pytest.raises(ValueError):
            call()
    with pytest.raises(IndexError):
        mesh.face_areas(vertices, faces + 2)
    with pytest.raises(IndexError):
        mesh.sample_points(vertices, faces - 1, 10)
    with pytest.raises(IndexError):                                                 # local ids against the item's own vertex count
        mesh.packed_face_areas(tensor('cases_packed_vertices'), tensor('cases_packed_first_idx_vertices'),
                               torch.tensor([[0, 1, 2], [1, 0, 3], [0, 1, 3]]), tensor('cases_packed_num_faces_per_mesh'))
