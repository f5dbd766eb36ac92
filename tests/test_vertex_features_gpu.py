"""The HIP path of ops.mesh.vertex_features (csrc/vertex_features.hip) on the GPU: bit for bit against the numpy brute force of
vertex_features_bruteforce.py and against the torch formulation on CPU tensors, at the smallest shapes that cross each boundary of
the code; strided inputs; the gradient; run-to-run equality; vertex_tangents; the topology cache; graph capture.  Every value check
is ``torch.equal`` unless its docstring derives a bound."""
import numpy as np
import pytest
import torch

import vertex_features_bruteforce as bf
from kaolin_amd import _C
from kaolin_amd.ops import mesh
from kaolin_amd.ops.mesh import vertex_features as vf
from vertex_features_cases import random_faces, random_features, tangents_example

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
DTYPES = [torch.float32, torch.float64]


@pytest.fixture(autouse=True)
def hip_path_only(monkeypatch):
    """A float32 / float64 GPU call that reached the torch formulation would pass these tests without running a kernel; every
    test starts without a cache entry."""
    formulation = vf._torch_vertex_gather

    def cpu_only(faces, face_features, num_vertices, mean):
        assert not face_features.is_cuda, 'a float32 / float64 GPU call reached the torch formulation'
        return formulation(faces, face_features, num_vertices, mean)

    monkeypatch.setattr(vf, '_torch_vertex_gather', cpu_only)
    vf._clear_vertex_corners_cache()
    yield
    vf._clear_vertex_corners_cache()


def hip(faces, x, V, mean):
    """the public path: the cache, the autograd function, the kernels"""
    if mean:
        return mesh.average_face_vertex_features(faces, x, num_vertices=V)
    return vf._vertex_gather(faces, x, V, False)


def check_against_both(faces_np, x_np, V):
    """HIP == brute force == torch formulation on CPU tensors, mean and sum"""
    faces, x = torch.from_numpy(faces_np), torch.from_numpy(x_np)
    for mean in (True, False):
        got = hip(faces.to(DEV), x.to(DEV), V, mean)
        assert got.device == torch.device(DEV) and got.dtype == x.dtype and got.shape == (x.shape[0], V, x.shape[3])
        want = bf.vertex_gather(faces_np, x_np, V, mean=mean)
        assert np.array_equal(got.cpu().numpy(), want), f'HIP != brute force (mean={mean})'
        assert np.array_equal(vf._torch_vertex_gather(faces, x, V, mean).numpy(), want), f'torch formulation != brute force (mean={mean})'


# (F, K, V, B, N): corner counts K F around the sort block (2047, 2048, 2049) and its half (1023, 1025); V = 1 (no pass: the copy),
# 2 and 256 (one pass), 257 (two), 65 537 (three: both parities of the ping-pong); K = 1, 3, 4; B = 1, 3; N = 1 .. 130 (group widths
# 1, 4, 8, 64 and the strided loop)
BOUNDARY_SHAPES = [(2047, 1, 257, 1, 3), (2048, 1, 256, 1, 1), (2049, 1, 2, 1, 4), (1023, 1, 1, 3, 5), (1025, 1, 65537, 1, 3),
                   (683, 3, 257, 3, 64), (512, 4, 256, 1, 65), (341, 3, 2, 1, 130), (342, 3, 65537, 3, 4), (512, 4, 1, 1, 3)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', BOUNDARY_SHAPES, ids=lambda s: 'F{}_K{}_V{}_B{}_N{}'.format(*s))
def test_boundaries(shape, dtype):
    F, K, V, B, N = shape
    check_against_both(random_faces(F, K, V, seed=F + K + V), random_features((B, F, K, N), dtype, seed=F + N), V)


@pytest.mark.parametrize('dtype', DTYPES)
def test_unused_vertices_first_last_and_middle(dtype):
    V = 300
    allowed = np.array([v for v in range(V) if v not in (0, 150, 151, V - 1)])
    faces = allowed[random_faces(200, 3, allowed.size, seed=5)]
    x = random_features((3, 200, 3, 3), dtype, seed=5)
    check_against_both(faces, x, V)
    got = mesh.average_face_vertex_features(torch.from_numpy(faces).to(DEV), torch.from_numpy(x).to(DEV), num_vertices=V)
    assert not got[:, [0, 150, 151, V - 1]].any()
    # num_vertices=None: the largest id + 1, one host read
    auto = mesh.average_face_vertex_features(torch.from_numpy(faces).to(DEV), torch.from_numpy(x).to(DEV))
    assert auto.shape[1] == int(faces.max()) + 1 and torch.equal(auto, got[:, :auto.shape[1]])


@pytest.mark.parametrize('dtype', DTYPES)
def test_one_vertex_holds_every_corner(dtype):
    faces = np.ones((5000, 3), dtype=np.int64)
    check_against_both(faces, random_features((1, 5000, 3, 3), dtype, seed=6), 2)


@pytest.mark.parametrize('dtype', DTYPES)
def test_face_that_repeats_a_vertex(dtype):
    """[2, 2, 5] counts twice for vertex 2, as in the reference"""
    faces = np.array([[2, 2, 5], [0, 1, 2], [5, 5, 5], [3, 4, 2]], dtype=np.int64)
    x = random_features((2, 4, 3, 3), dtype, seed=7)
    check_against_both(faces, x, 6)
    got = mesh.average_face_vertex_features(torch.from_numpy(faces).to(DEV), torch.from_numpy(x).to(DEV), num_vertices=6)
    two = torch.from_numpy(((x[:, 0, 0] + x[:, 0, 1] + x[:, 1, 2] + x[:, 3, 2]) / np.asarray(4, dtype=x.dtype))).to(DEV)
    assert torch.equal(got[:, 2], two)


# ---- strides ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mean', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
def test_strided_inputs_equal_their_contiguous_copies(dtype, mean):
    F, K, V, B, N = 300, 3, 100, 3, 5
    faces_np = random_faces(F, K, V, seed=8)
    faces = torch.from_numpy(faces_np).to(DEV)
    per_face = torch.from_numpy(random_features((B, F, N), dtype, seed=8)).to(DEV)
    one_item = torch.from_numpy(random_features((F, K, N), dtype, seed=9)).to(DEV)
    wide = torch.from_numpy(random_features((B, F, K, 2 * N + 1), dtype, seed=10)).to(DEV)
    views = {'expanded over K (stride 0)': per_face[:, :, None, :].expand(B, F, K, N),
             'expanded over B (stride 0)': one_item[None].expand(B, F, K, N),
             'sliced in N (stride 2)': wide[..., 1::2]}
    for name, view in views.items():
        assert not view.is_contiguous() and view.shape == (B, F, K, N), name
        copy = view.contiguous()
        want = hip(faces, copy, V, mean)
        assert np.array_equal(want.cpu().numpy(), bf.vertex_gather(faces_np, copy.cpu().numpy(), V, mean=mean)), name
        assert torch.equal(hip(faces, view, V, mean), want), name
    x = views['sliced in N (stride 2)'].contiguous()
    want = hip(faces, x, V, mean)
    transposed = faces.t().contiguous().t()
    assert not transposed.is_contiguous() and transposed.stride() == (1, F)
    assert torch.equal(hip(transposed, x, V, mean), want), 'faces as a transposed view'
    assert torch.equal(hip(faces.int(), x, V, mean), want), 'int32 faces'
    assert torch.equal(hip(faces.int().t().contiguous().t(), x, V, mean), want), 'int32 faces as a transposed view'
    assert torch.equal(hip(faces.short(), x, V, mean), want), 'int16 faces'


# ---- backward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mean', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
def test_backward_materialised_equals_cpu_autograd(dtype, mean):
    F, K, V, B, N = 683, 3, 257, 3, 5
    faces_np = random_faces(F, K, V, seed=11)
    x_np, g_np = random_features((B, F, K, N), dtype, seed=11), random_features((B, V, N), dtype, seed=12)
    x_cpu = torch.from_numpy(x_np).requires_grad_()
    vf._torch_vertex_gather(torch.from_numpy(faces_np), x_cpu, V, mean).backward(torch.from_numpy(g_np))
    x = torch.from_numpy(x_np).to(DEV).requires_grad_()
    hip(torch.from_numpy(faces_np).to(DEV), x, V, mean).backward(torch.from_numpy(g_np).to(DEV))
    assert x.grad.shape == x.shape and x.grad.is_contiguous()
    assert torch.equal(x.grad.cpu(), x_cpu.grad)
    assert np.array_equal(x.grad.cpu().numpy(), bf.vertex_gather_backward(faces_np, g_np, mean=mean))
    # a cotangent with stride 0 everywhere (what .sum().backward() sends)
    x.grad = None
    hip(torch.from_numpy(faces_np).to(DEV), x, V, mean).sum().backward()
    ones = np.ones((B, V, N), dtype=x_np.dtype)
    assert np.array_equal(x.grad.cpu().numpy(), bf.vertex_gather_backward(faces_np, ones, mean=mean))


@pytest.mark.parametrize('dtype', DTYPES)
def test_backward_of_input_expanded_over_corners(dtype):
    """compute_vertex_normals' usual input: one normal per face expanded over the K corners.  The operator's gradient pieces g_k
    (K per face, each bit-exact: the test above) are summed by autograd's expand backward, K - 1 rounded additions in an order we
    do not control: |got - sum_k g_k| <= (K - 1) u sum_k |g_k| per element, u the unit roundoff, the exact sum taken in long
    double."""
    F, K, V, B, N = 300, 3, 100, 2, 3
    faces_np = random_faces(F, K, V, seed=13)
    per_face = torch.from_numpy(random_features((B, F, N), dtype, seed=13)).to(DEV).requires_grad_()
    g_np = random_features((B, V, N), dtype, seed=14)
    mesh.compute_vertex_normals(torch.from_numpy(faces_np).to(DEV), per_face[:, :, None, :].expand(B, F, K, N), V) \
        .backward(torch.from_numpy(g_np).to(DEV))
    pieces = bf.vertex_gather_backward(faces_np, g_np, mean=True).astype(np.longdouble)          # (B, F, K, N)
    u = np.finfo(g_np.dtype).eps / 2
    err = np.abs(per_face.grad.cpu().numpy().astype(np.longdouble) - pieces.sum(axis=2))
    bound = (K - 1) * u * np.abs(pieces).sum(axis=2)
    print(f'expanded backward {dtype}: worst share of the bound {float((err / bound).max()):.3f}')
    assert per_face.grad.shape == (B, F, N) and (err <= bound).all()


def test_gradcheck():
    faces = torch.from_numpy(random_faces(7, 3, 6, seed=15)).to(DEV)
    x = torch.from_numpy(random_features((2, 7, 3, 4), torch.float64, seed=15)).to(DEV).requires_grad_()
    assert torch.autograd.gradcheck(lambda t: mesh.average_face_vertex_features(faces, t, 6), (x,))
    assert torch.autograd.gradcheck(lambda t: vf._vertex_gather(faces, t, 6, False), (x,))


@pytest.mark.parametrize('dtype', DTYPES)
def test_run_to_run(dtype):
    F, K, V, B, N = 2000, 3, 50, 3, 3
    faces = torch.from_numpy(random_faces(F, K, V, seed=16)).to(DEV)
    g = torch.from_numpy(random_features((B, V, N), dtype, seed=17)).to(DEV)
    runs = []
    for _ in range(2):
        x = torch.from_numpy(random_features((B, F, K, N), dtype, seed=16)).to(DEV).requires_grad_()
        out = mesh.average_face_vertex_features(faces, x, V)
        out.backward(g)
        runs.append((out.detach(), x.grad))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


# ---- vertex_tangents ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_vertex_tangents_recorded_example(dtype):
    faces, face_vertices, face_uvs, normals, expected, atol, rtol = tangents_example(dtype, DEV)
    got = mesh.vertex_tangents(faces, face_vertices, face_uvs, normals)
    assert got.device == torch.device(DEV) and got.dtype == dtype
    assert torch.allclose(got, expected, atol=atol, rtol=rtol)


def uv_grid(dtype):
    """A 17 x 9 grid of vertices over a height field, two triangles per cell: positions (i / 16, j / 8, h / 32) with integer h in
    [0, 4] and UVs (i / 16, j / 8): small integers over powers of two.  -> faces (256, 3), face_vertices, face_uvs, unit normals"""
    i, j = np.meshgrid(np.arange(17), np.arange(9), indexing='ij')
    h = (i * i + 3 * j + i * j) % 5
    pos = np.stack([i / 16.0, j / 8.0, h / 32.0], axis=-1).reshape(-1, 3)
    uv = np.stack([i / 16.0, j / 8.0], axis=-1).reshape(-1, 2)
    vid = (i * 9 + j)
    a, b, c, d = vid[:-1, :-1], vid[1:, :-1], vid[1:, 1:], vid[:-1, 1:]
    faces = np.concatenate([np.stack([a, b, c], -1).reshape(-1, 3), np.stack([a, c, d], -1).reshape(-1, 3)])
    faces_t = torch.from_numpy(faces)
    pos_t, uv_t = torch.from_numpy(pos).to(dtype), torch.from_numpy(uv).to(dtype)
    face_vertices = pos_t[faces_t]
    face_normals = mesh.face_normals(face_vertices[None], unit=True)                                          # (1, F, 3)
    normals = mesh.compute_vertex_normals(faces_t, face_normals[:, :, None, :].expand(1, faces.shape[0], 3, 3), pos.shape[0])[0]
    return faces_t, face_vertices, uv_t[faces_t], torch.nn.functional.normalize(normals, dim=1)


@pytest.mark.parametrize('dtype', DTYPES)
def test_vertex_tangents_uv_grid_against_cpu(dtype):
    """The same inputs on both devices.  Every coordinate and UV is a small integer over a power of two and every UV determinant is
    +-1 / 128, so the per-face tangents and every per-vertex sum t are EXACT in either dtype: both devices hold the same t, whatever
    the order.  What follows differs only by the roundings of torch's own kernels.  With u the unit roundoff, first order in u, all
    vectors of length ~1:
      normalize(t):    sum of squares 3 u, halved by the root 1.5 u, the root itself <= 1 ulp = 2 u, the division u: each component
                       within 4.5 u of exact;
      projection:      d = <t1, n>: 4.5 u from t1 plus 3 u of its own (three products, two additions) = 7.5 u; p = t1 - d n:
                       4.5 u + 7.5 u + u (the product) + u (the subtraction) = 14.5 u per component, |dp| <= sqrt(3) 14.5 u = 25.2 u;
      normalize(p):    |p| = sin(angle between tangent and normal) >= sin 45 deg (asserted below), so 25.2 u / 0.7071 = 35.6 u, plus
                       4.5 u of its own: 40.1 u per path.
    Two paths: |gpu - cpu| <= 81 u per component."""
    faces, face_vertices, face_uvs, normals = uv_grid(dtype)
    cpu = mesh.vertex_tangents(faces, face_vertices, face_uvs, normals)
    assert torch.isfinite(cpu).all()
    # the angle that conditions the projection: between the normalised sum (before the projection) and the normal
    corner_tangents = _face_tangents(face_vertices, face_uvs)[None, :, None, :].expand(1, faces.shape[0], 3, 3)
    t1 = torch.nn.functional.normalize(vf._torch_vertex_gather(faces, corner_tangents, normals.shape[0], False)[0], dim=1)
    assert float((t1 * normals).sum(-1).abs().max()) <= 0.7071, 'a tangent within 45 degrees of its normal'
    got = mesh.vertex_tangents(faces.to(DEV), face_vertices.to(DEV), face_uvs.to(DEV), normals.to(DEV))
    u = torch.finfo(dtype).eps / 2
    err = float((got.cpu() - cpu).abs().max())
    print(f'vertex_tangents uv grid {dtype}: worst share of the bound {err / (81 * u):.3f}')
    assert err <= 81 * u


def _face_tangents(face_vertices, face_uvs):
    """the per-face tangent of vertex_tangents (exact on the uv grid)"""
    uve1, uve2 = face_uvs[:, 1] - face_uvs[:, 0], face_uvs[:, 2] - face_uvs[:, 0]
    pe1, pe2 = face_vertices[:, 1] - face_vertices[:, 0], face_vertices[:, 2] - face_vertices[:, 0]
    nom = pe1 * uve2[:, 1:2] - pe2 * uve1[:, 1:2]
    denom = uve1[:, 0:1] * uve2[:, 1:2] - uve1[:, 1:2] * uve2[:, 0:1]
    assert bool((denom.abs() == 1.0 / 128).all())
    return nom / denom


# ---- the topology cache -------------------------------------------------------------------------------------------------------------
@pytest.fixture
def builds(monkeypatch):
    """counts the calls of the operator that builds the corner lists"""
    calls = []
    build = _C.ops.mesh.vertex_corners_cuda

    def counted(faces, num_vertices):
        calls.append(num_vertices)
        return build(faces, num_vertices)

    monkeypatch.setattr(_C.ops.mesh, 'vertex_corners_cuda', counted)
    return calls


def test_cache(builds):
    F, K, V, B, N = 100, 3, 40, 2, 3
    faces_np = random_faces(F, K, V, seed=18)
    faces = torch.from_numpy(faces_np).to(DEV)
    x_np = random_features((B, F, K, N), torch.float32, seed=18)
    x = torch.from_numpy(x_np).to(DEV)
    first = mesh.average_face_vertex_features(faces, x, V)
    assert len(builds) == 1
    assert torch.equal(mesh.average_face_vertex_features(faces, x, V), first) and len(builds) == 1, 'same faces: a hit'
    vf._vertex_gather(faces, x, V, False)
    assert len(builds) == 1, 'the sum shares the lists of the mean'
    # an in-place write bumps the version: rebuilt, and the new result
    moved = (int(faces_np[0, 0]) + 1) % V
    faces[0, 0] = moved
    faces_np[0, 0] = moved
    second = mesh.average_face_vertex_features(faces, x, V)
    assert len(builds) == 2
    assert np.array_equal(second.cpu().numpy(), bf.vertex_gather(faces_np, x_np, V))
    # another tensor with the same contents: rebuilt (its address differs: the entry keeps the first one alive)
    assert torch.equal(mesh.average_face_vertex_features(faces.clone(), x, V), second) and len(builds) == 3
    # another number of vertices: rebuilt
    assert mesh.average_face_vertex_features(faces, x, V + 1).shape[1] == V + 1 and len(builds) == 4


@pytest.mark.parametrize('bad_id', [40, -1])
def test_out_of_range_id_raises_and_leaves_no_entry(builds, bad_id):
    """the key kernel counts the ids outside [0, V) and files them under vertex 0; the host raises before the lists are used"""
    F, K, V = 100, 3, 40
    faces = torch.from_numpy(random_faces(F, K, V, seed=19)).to(DEV)
    x = torch.from_numpy(random_features((1, F, K, 3), torch.float32, seed=19)).to(DEV)
    mesh.average_face_vertex_features(faces, x, V)
    assert len(vf._vertex_corners_cache) == 1
    faces[17, 1] = bad_id
    with pytest.raises(IndexError, match='outside'):
        mesh.average_face_vertex_features(faces, x, V)
    assert len(builds) == 2 and len(vf._vertex_corners_cache) == 0


def test_limits_raise_before_any_launch():
    faces = torch.zeros((4, 3), dtype=torch.long, device=DEV)
    with pytest.raises(ValueError, match='2\\^31'):
        _C.ops.mesh.vertex_corners_cuda(faces, 2 ** 31 - 1)
    with pytest.raises(ValueError, match='2\\^31'):
        _C.ops.mesh.vertex_corners_cuda(faces.t()[:, :1].expand(3, 2 ** 30), 5)


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
def test_graph_capture_forward_and_backward():
    """cache warm: the forward and backward of compute_vertex_normals are one launch each without a host read"""
    F, K, V, B = 500, 3, 260, 2
    faces = torch.from_numpy(random_faces(F, K, V, seed=20)).to(DEV)
    normals = torch.from_numpy(random_features((B, F, 3), torch.float32, seed=20)).to(DEV).requires_grad_()
    cotangent = torch.from_numpy(random_features((B, V, 3), torch.float32, seed=21)).to(DEV)

    def step():
        out = mesh.compute_vertex_normals(faces, normals[:, :, None, :].expand(B, F, K, 3), V)
        (grad,) = torch.autograd.grad(out, normals, cotangent)
        return out, grad

    step()                                                                                     # warms the cache
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grad = step()
    with torch.no_grad():
        normals.copy_(torch.from_numpy(random_features((B, F, 3), torch.float32, seed=22)).to(DEV))
        cotangent.copy_(torch.from_numpy(random_features((B, V, 3), torch.float32, seed=23)).to(DEV))
    out.detach().fill_(-7)
    grad.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    eager_out, eager_grad = step()
    assert torch.equal(out.detach(), eager_out.detach()) and torch.equal(grad, eager_grad)
