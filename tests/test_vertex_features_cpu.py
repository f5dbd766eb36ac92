"""ops.mesh.vertex_features without a GPU: the torch formulation (the reference's scatter_add_ expression restated) against the numpy
brute force of vertex_features_bruteforce.py bit for bit, the reference's own small cases restated, unindex_vertices_by_faces,
vertex_tangents on the reference's recorded example, and the argument checks."""
import numpy as np
import pytest
import torch

import vertex_features_bruteforce as bf
from kaolin_amd.ops import mesh
from kaolin_amd.ops.mesh import vertex_features
from vertex_features_cases import random_faces, random_features, tangents_example

# (F, K, V, B, N): a tiny mesh, a mesh of ordinary valence, a quad mesh with many unused vertices, every corner on two vertices
SHAPES = [(7, 3, 6, 1, 3), (500, 3, 260, 3, 3), (300, 4, 1000, 2, 10), (5000, 3, 2, 1, 4)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('shape', SHAPES)
def test_torch_formulation_equals_bruteforce(shape, dtype):
    F, K, V, B, N = shape
    faces = random_faces(F, K, V, seed=F + V)
    x = random_features((B, F, K, N), dtype, seed=F)
    got = mesh.average_face_vertex_features(torch.from_numpy(faces), torch.from_numpy(x), num_vertices=V)
    assert got.dtype == dtype and got.shape == (B, V, N)
    assert np.array_equal(got.numpy(), bf.vertex_gather(faces, x, V, mean=True))
    total = vertex_features._torch_vertex_gather(torch.from_numpy(faces), torch.from_numpy(x), V, False)
    assert np.array_equal(total.numpy(), bf.vertex_gather(faces, x, V, mean=False))


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32, torch.float64])
def test_reference_case_unused_vertex(dtype):
    """the reference's test_average_face_vertex_features: 4 faces, 7 vertices, vertex 3 in no face"""
    faces = torch.tensor([[0, 1, 2], [1, 2, 4], [2, 4, 5], [2, 5, 6]], dtype=torch.long)
    B, V, N = 3, 7, 10
    torch.manual_seed(0)
    x = torch.rand((B, 4, 3, N), dtype=torch.float32).to(dtype)
    expected = torch.zeros((B, V, N), dtype=dtype)
    for b in range(B):
        expected[b, 0] = x[b, 0, 0]
        expected[b, 1] = (x[b, 0, 1] + x[b, 1, 0]) / 2
        expected[b, 2] = (x[b, 0, 2] + x[b, 1, 1] + x[b, 2, 0] + x[b, 3, 0]) / 4
        expected[b, 4] = (x[b, 1, 2] + x[b, 2, 1]) / 2
        expected[b, 5] = (x[b, 2, 2] + x[b, 3, 1]) / 2
        expected[b, 6] = x[b, 3, 2]
    got = mesh.average_face_vertex_features(faces, x)
    assert got.dtype == dtype and got.shape == (B, V, N)
    if dtype == torch.float16:
        assert torch.allclose(expected, got, rtol=1e-3, atol=1e-3)                    # the reference's own tolerances
    else:
        assert torch.allclose(expected, got)
        assert np.array_equal(got.numpy(), bf.vertex_gather(faces.numpy(), x.numpy(), V))
    assert torch.equal(got[:, 3], torch.zeros((B, N), dtype=dtype))


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_reference_case_fan(dtype):
    """the reference's test_compute_vertex_normals: a fan around vertex 0, with num_vertices = 6 (one unused) and with None"""
    faces = torch.tensor([[0, 2, 1], [0, 3, 2], [0, 4, 3]], dtype=torch.long)
    B, V = 3, 6
    torch.manual_seed(1)
    n = torch.rand((B, 3, 3, 3), dtype=dtype)
    expected = torch.zeros((B, V, 3), dtype=dtype)
    for b in range(B):
        expected[b, 0] = (n[b, 0, 0] + n[b, 1, 0] + n[b, 2, 0]) / 3
        expected[b, 1] = n[b, 0, 2]
        expected[b, 2] = (n[b, 0, 1] + n[b, 1, 2]) / 2
        expected[b, 3] = (n[b, 1, 1] + n[b, 2, 2]) / 2
        expected[b, 4] = n[b, 2, 1]
    got = mesh.compute_vertex_normals(faces, n, num_vertices=V)
    assert torch.allclose(expected, got)
    assert np.array_equal(got.numpy(), bf.vertex_gather(faces.numpy(), n.numpy(), V))
    assert torch.equal(mesh.compute_vertex_normals(faces, n), got[:, :5])


def test_differentiable_on_cpu():
    faces = torch.from_numpy(random_faces(7, 3, 6, seed=3))
    x = torch.from_numpy(random_features((2, 7, 3, 4), torch.float64, seed=3)).requires_grad_()
    g = torch.from_numpy(random_features((2, 6, 4), torch.float64, seed=4))
    mesh.average_face_vertex_features(faces, x, 6).backward(g)
    assert np.array_equal(x.grad.numpy(), bf.vertex_gather_backward(faces.numpy(), g.numpy(), mean=True))


def test_no_faces_and_no_vertices():
    out = mesh.average_face_vertex_features(torch.zeros((0, 3), dtype=torch.long), torch.zeros((2, 0, 3, 4)), num_vertices=5)
    assert out.shape == (2, 5, 4) and not out.any()
    out = mesh.average_face_vertex_features(torch.zeros((0, 3), dtype=torch.long), torch.zeros((2, 0, 3, 4)), num_vertices=0)
    assert out.shape == (2, 0, 4)


def test_unindex_vertices_by_faces():
    """the reference's test restated: unbatched and with a batch of 4"""
    nfaces, fsize, channels = 5, 3, 2
    torch.manual_seed(2)
    for lead in ((), (4,), (2, 3)):
        x = torch.rand(lead + (nfaces, fsize, channels))
        flat, index = mesh.unindex_vertices_by_faces(x)
        assert flat.shape == lead + (nfaces * fsize, channels)
        assert index.shape == (nfaces, fsize) and index.dtype == torch.long
        assert torch.equal(index, torch.arange(nfaces * fsize).reshape(nfaces, fsize))
        assert torch.equal(flat[..., index, :], x)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
def test_vertex_tangents_recorded_example(dtype):
    faces, face_vertices, face_uvs, normals, expected, atol, rtol = tangents_example(dtype)
    got = mesh.vertex_tangents(faces, face_vertices, face_uvs, normals)
    assert got.dtype == dtype and got.shape == expected.shape
    assert torch.allclose(got, expected, atol=atol, rtol=rtol)
    assert mesh.trianglemesh.vertex_tangents is mesh.vertex_tangents


def test_vertex_tangents_differentiable_on_cpu():
    faces, face_vertices, face_uvs, normals, _, _, _ = tangents_example(torch.float64)
    inputs = [t.clone().requires_grad_() for t in (face_vertices, face_uvs, normals)]
    with torch.autograd.detect_anomaly(check_nan=True):
        out = mesh.vertex_tangents(faces, *inputs)
    out.sum().backward()
    assert all(t.grad is not None and torch.isfinite(t.grad).all() for t in inputs)


def test_argument_errors():
    faces = torch.zeros((4, 3), dtype=torch.long)
    x = torch.zeros((2, 4, 3, 5))
    for bad_faces, bad_x, word in ((faces[0], x, r'\(3,\)'), (faces, x[0], r'\(4, 3, 5\)'), (faces[:3], x, r'\(3, 3\)'),
                                   (faces[:, :2], x, r'\(4, 2\)'), (faces, x.long(), 'int64'), (faces.float(), x, 'float32')):
        with pytest.raises(ValueError, match=word):
            mesh.average_face_vertex_features(bad_faces, bad_x, num_vertices=3)
    fv, uv, vn = torch.zeros((4, 3, 3)), torch.zeros((4, 3, 2)), torch.zeros((6, 3))
    for args, word in (((faces[:, :2], fv, uv, vn), r'\(4, 2\)'), ((faces, fv[:3], uv, vn), r'\(3, 3, 3\)'),
                       ((faces, fv, uv[..., :1], vn), r'\(4, 3, 1\)'), ((faces, fv, uv, vn[None]), r'\(1, 6, 3\)')):
        with pytest.raises(ValueError, match=word):
            mesh.vertex_tangents(*args)
