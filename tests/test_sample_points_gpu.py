"""ops.mesh.face_areas / sample_points on the GPU: the HIP pipeline (csrc/sample_points.hip) against the numpy oracle
(tests/sample_points_bruteforce.py) and the package's torch formulation on the CPU, bit for bit wherever the contract fixes the
bits.  The CPU expressions are evaluated with the correctly rounded square root (``oracle.ieee_sqrt``): torch's own CPU sqrt,
built on MKL's vector maths, is one unit in the last place off for about 0.6 % of its arguments; the contract and the kernels
round correctly.

Gradient bounds (``gamma_n sum|term|``, ``gamma_n = n u / (1 - n u)``; both sides of a comparison round, so the
bound is the sum over the kernel's unit roundoff and the float64 reference's):

* sample_points: an element of grad_vertices / grad_face_features is the sum of m terms ``w_k g``.  A weight takes at most three
  operations (sqrt, a subtraction from 1, a product) and the term one more: n = 4 + m.  ``1 - u`` and ``1 - uv1`` cancel, so a
  term's magnitude is taken over the operands of those subtractions: ``(1 + u) |g|``, ``u (1 + uv1) |g|``, ``u uv1 |g|``;
* face_areas: a corner's gradient is ``(g / 2) (n x e)`` with n = d / |d| the unit normal from the cross product d of the rounded
  differences x, y.  With ``D_i = |x_j y_k| + |x_k y_j|`` (the operands of the subtraction that gives d_i), ``kappa_i = D_i / |d|``
  and ``c_i = kappa_i + |n_i| sum_j |n_j| kappa_j``, the computed n_i is off by at most ``gamma_8 c_i`` (4 operations to d_i, 4 more
  through the sums, the root and the division); five more operations reach the corner value and m corners meet at the vertex:
  n = 13 + m and a term's magnitude is ``(|g| / 2) c_i |e_j|``.  A vertex of a zero-area face is NaN on both sides."""
import functools
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN_DIR, ROOT
from kaolin_amd import _C
from kaolin_amd.metrics.pointcloud import chamfer_distance
from kaolin_amd.ops import mesh
from kaolin_amd.ops.conversions import marching_tetrahedra
from kaolin_amd.ops.mesh import sampling
from kaolin_amd.utils.testing import kuhn_grid
import sample_points_bruteforce as oracle

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G = np.load(os.path.join(GOLDEN_DIR, 'sample_points.npz'))
DTYPES = [('f32', torch.float32), ('f64', torch.float64)]
HEADER = open(os.path.join(ROOT, 'kaolin_amd', 'csrc', 'sample_points.h')).read()
K = {name: int(value) for name, value in re.findall(r'constexpr int (SP_\w+) = (\d+);', HEADER)}
SCAN_TILE = K['SP_SCAN_THREADS'] * K['SP_SCAN_PER_THREAD']
LANES_FROM = K['SP_FEATURE_LANES_FROM']
FACE_COUNTS = [1, 63, 64, 65, 255, 256, 257, 1025]
SCAN_COUNTS = [SCAN_TILE + 1, 64 * SCAN_TILE + 1]          # one above a tile; one above 64 tiles (the second level crosses a wavefront)
SAMPLE_COUNTS = [1, 63, 64, 65, 257, 4096]
# the functions of the torch formulation, kept for the CPU side of the comparisons (the fixture below removes them from the module)
AREAS_TORCH, SAMPLE_TORCH, BLEND_TORCH = sampling.face_areas_torch, sampling.sample_points_torch, sampling.blend_torch
ops = _C.ops.mesh


@pytest.fixture(autouse=True)
def hip_path_only(monkeypatch):
    """A float32 / float64 GPU call that reached the torch formulation would pass these tests without running a kernel."""
    monkeypatch.setattr(sampling, 'face_areas_torch', None)
    monkeypatch.setattr(sampling, 'sample_points_torch', None)


def tensor(name, dtype=None):
    t = torch.from_numpy(G[name])
    return t if dtype is None else t.to(dtype)


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=12345.), torch.nan_to_num(b, nan=12345.))


@functools.lru_cache(maxsize=None)
def soup(F, B):
    """A seeded triangle soup on the CPU, float32-exact: (vertices (B, V, 3) float32, faces (F, 3)).  Random ids repeat now and
    then (zero-area faces) and face F // 2 repeats a vertex when F >= 3; face 0 has area."""
    g = torch.Generator().manual_seed(1000 * B + F)
    V = max(3, min(F // 2 + 3, 4096))
    vertices = (torch.rand(B, V, 3, generator=g) * 2 - 1).float()
    faces = torch.randint(0, V, (F, 3), generator=g)
    faces[0] = torch.tensor([0, 1, 2])
    if F >= 3:
        faces[F // 2, 2] = faces[F // 2, 0]
    return vertices, faces


def draws(B, N, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((B, N), dtype=torch.float64, generator=g), torch.rand((B, N, 2), dtype=dtype, generator=g)


def cpu_areas(vertices, faces):
    return AREAS_TORCH(vertices, faces, sqrt=oracle.ieee_sqrt)


def cpu_blend(vertices, faces, choices, uv):
    corners = [torch.gather(c, 1, choices.unsqueeze(-1).expand(-1, -1, 3)) for c in sampling._face_corners(vertices, faces)]
    return BLEND_TORCH(uv, *corners, sqrt=oracle.ieee_sqrt)


def cpu_feature_blend(face_features, choices, uv):
    chosen = torch.gather(face_features, 1, choices[..., None, None].expand(-1, -1, 3, face_features.shape[-1]))
    return BLEND_TORCH(uv, chosen[:, :, 0], chosen[:, :, 1], chosen[:, :, 2], sqrt=oracle.ieee_sqrt)


# ---- areas ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,dtype', DTYPES)
@pytest.mark.parametrize('F', FACE_COUNTS)
def test_areas_equal_the_cpu_expression(F, tag, dtype):
    for B in (1, 3):
        vertices, faces = soup(F, B)
        vertices = vertices.to(dtype)
        got = mesh.face_areas(vertices.to(DEV), faces.to(DEV))
        assert got.device == torch.device(DEV) and same(got.cpu(), cpu_areas(vertices, faces)), (F, B)
        assert np.array_equal(got.cpu().numpy(), oracle.face_areas(vertices.numpy(), faces.numpy()))


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_areas_of_the_golden_meshes(tag, dtype):
    got = mesh.face_areas(tensor('tables_areas_vertices', dtype).to(DEV), tensor('tables_areas_faces').to(DEV))
    assert torch.equal(got.cpu(), tensor(f'tables_areas_expected_{tag}'))              # the reference's own test
    got = mesh.face_areas(tensor('ico_vertices', dtype).to(DEV), tensor('ico_faces').to(DEV))
    assert same(got.cpu(), tensor(f'ico_areas_ieee_{tag}'))


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_areas_of_non_contiguous_vertices(tag, dtype):
    vertices, faces = soup(257, 3)
    vertices, want = vertices.to(dtype), cpu_areas(vertices.to(dtype), faces)
    transposed = vertices.transpose(1, 2).contiguous().to(DEV).transpose(1, 2)
    wide = torch.zeros(3, vertices.shape[1], 7, dtype=dtype)
    wide[..., 2:5] = vertices
    sliced = wide.to(DEV)[..., 2:5]
    strided_faces = torch.stack([faces, faces], dim=1).reshape(-1, 3).to(DEV)[::2]
    assert not transposed.is_contiguous() and not sliced.is_contiguous() and not strided_faces.is_contiguous()
    assert same(mesh.face_areas(transposed, faces.to(DEV)).cpu(), want)
    assert same(mesh.face_areas(sliced, strided_faces).cpu(), want)


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_packed_areas(tag, dtype):
    counts, nv = [2, 1, 65], [4, 7, 40]
    g = torch.Generator().manual_seed(5)
    vertices = (torch.rand(sum(nv), 3, generator=g) * 2 - 1).to(dtype)
    faces = torch.cat([torch.randint(0, v, (c, 3), generator=g) for c, v in zip(counts, nv)])
    first = torch.tensor([0, 4, 11, 51])
    got = mesh.packed_face_areas(vertices.to(DEV), first, faces.to(DEV), torch.tensor(counts))
    merged = faces + torch.repeat_interleave(first[:-1], torch.tensor(counts))[:, None]
    assert got.shape == (68,) and same(got.cpu(), cpu_areas(vertices[None], merged)[0])


# ---- the face choice ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,dtype', DTYPES)
@pytest.mark.parametrize('F', FACE_COUNTS + SCAN_COUNTS)
def test_choices_points_equal_the_oracle(F, tag, dtype):
    B = 1 if F % 2 == 0 or F > 4096 else 3
    vertices, faces = soup(F, B)
    vertices = vertices.to(dtype)
    v, f = vertices.to(DEV), faces.to(DEV)
    areas = mesh.face_areas(v, f)
    zero = torch.nonzero(areas[0].cpu() == 0).reshape(-1)
    assert F < 3 or zero.numel() >= 1
    for N in SAMPLE_COUNTS:
        r, uv = draws(B, N, dtype, 7 * F + N)
        want, margin, live = oracle.choose_faces(areas.cpu().numpy(), r.numpy())
        assert live.all() and float(margin.min()) > 1, 'the seed puts a sample within rounding of a cdf entry: change it'   # the cap is zero
        points, choices, features, areas_out, cdf = ops.sample_points_forward_cuda(v, f, None, None, r.to(DEV), uv.to(DEV))
        assert features is None and same(areas_out, areas) and cdf.dtype == torch.float64 and cdf.shape == (B, F)
        assert choices.dtype == torch.long and np.array_equal(choices.cpu().numpy(), want), (F, N)
        assert not bool(torch.isin(choices[0].cpu(), zero).any())                    # a face without area is never chosen
        assert same(points.cpu(), cpu_blend(vertices, faces, choices.cpu(), uv)), (F, N)
        given = ops.sample_points_forward_cuda(v, f, None, areas.double(), r.to(DEV), uv.to(DEV))     # areas of the other dtype
        assert torch.equal(given[1], choices) and same(given[0], points)
    again = ops.sample_points_forward_cuda(v, f, None, (areas, cdf), r.to(DEV), uv.to(DEV))            # the cdf of an earlier call
    assert torch.equal(again[1], choices) and same(again[0], points)
    sequential = torch.cumsum(areas.cpu().double(), 1)
    assert torch.allclose(cdf.cpu(), sequential, rtol=2 * F * 2.0 ** -52, atol=0)


def _proportional(vertices, faces, dtype, N):
    B, F = vertices.shape[0], faces.shape[0]
    v, f = vertices.to(DEV, dtype), faces.to(DEV)
    r = ((torch.arange(N, dtype=torch.float64) + 0.5) / N).expand(B, N).contiguous()
    uv = draws(B, N, dtype, N)[1]
    _, choices, _, areas, _ = ops.sample_points_forward_cuda(v, f, None, None, r.to(DEV), uv.to(DEV))
    areas = areas.cpu().double()
    expected = N * areas / torch.cumsum(areas, 1)[:, -1:]
    worst = 0.0
    for b in range(B):
        counts = torch.bincount(choices[b].cpu(), minlength=F).double()
        assert counts.shape == (F,) and not bool(counts[areas[b] == 0].any())
        worst = max(worst, float((counts - expected[b]).abs().max()))
    print(f'proportionality F={F} N={N}: largest |count - N area / total| = {worst:.4f}')
    assert worst < 1 + 4 * N * F * 2.0 ** -52


@pytest.mark.parametrize('N', [4096, 100003])
@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_exact_proportionality(tag, dtype, N):
    _proportional(tensor('ico_vertices'), tensor('ico_faces'), dtype, N)
    _proportional(*soup(1025, 3), dtype, N)


# ---- features -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,dtype', DTYPES)
@pytest.mark.parametrize('D', sorted({1, 3, LANES_FROM - 1, LANES_FROM, LANES_FROM + 1, 33, 65}))
def test_features_equal_the_cpu_blend(D, tag, dtype):
    B, F, N = 3, 257, 321
    vertices, faces = soup(F, B)
    vertices = vertices.to(dtype)
    g = torch.Generator().manual_seed(D)
    feats = (torch.rand(B, F, 3, D, generator=g) * 4 - 2).to(dtype)
    r, uv = draws(B, N, dtype, 31 * D)
    v, f = vertices.to(DEV), faces.to(DEV)
    points, choices, features, _, _ = ops.sample_points_forward_cuda(v, f, None, None, r.to(DEV), uv.to(DEV), feats.to(DEV))
    assert features.shape == (B, N, D) and same(features.cpu(), cpu_feature_blend(feats, choices.cpu(), uv))
    assert same(points.cpu(), cpu_blend(vertices, faces, choices.cpu(), uv))
    again = ops.sample_points_forward_cuda(v, f, None, None, r.to(DEV), uv.to(DEV), feats.to(DEV))
    assert all(same(a, b) for a, b in zip(again[:3], (points, choices, features)))    # the same bits on every call
    # stride 0: one feature row per face for its three corners, one set of features for the whole batch; a sliced last dimension
    per_face = feats[:, :, :1].to(DEV).expand(B, F, 3, D)
    shared = feats[:1].to(DEV).expand(B, F, 3, D)
    wide = torch.zeros(B, F, 3, D + 3, dtype=dtype)
    wide[..., 1:D + 1] = feats
    for strided, dense in ((per_face, feats[:, :, :1].expand(B, F, 3, D)), (shared, feats[:1].expand(B, F, 3, D)),
                           (wide.to(DEV)[..., 1:D + 1], feats)):
        assert not strided.is_contiguous() or D == 1
        got = ops.sample_points_forward_cuda(v, f, None, None, r.to(DEV), uv.to(DEV), strided)[2]
        assert same(got.cpu(), cpu_feature_blend(dense, choices.cpu(), uv))


def test_public_function_draws_on_the_device():
    """the draw contract on the GPU: seeding, drawing r and uv by hand and calling the operator equals sample_points"""
    vertices, faces = tensor('ico_vertices').to(DEV), tensor('ico_faces').to(DEV)
    feats = tensor('blend_features').to(DEV)
    torch.manual_seed(5)
    points, choices, features = mesh.sample_points(vertices, faces, 1000, face_features=feats)
    torch.manual_seed(5)
    r = torch.rand((2, 1000), dtype=torch.float64, device=DEV)
    uv = torch.rand((2, 1000, 2), dtype=torch.float32, device=DEV)
    want = ops.sample_points_forward_cuda(vertices, faces, None, None, r, uv, feats)
    assert same(points, want[0]) and same(choices, want[1]) and same(features, want[2])
    torch.manual_seed(5)
    with_areas = mesh.sample_points(vertices, faces, 1000, mesh.face_areas(vertices, faces))
    assert len(with_areas) == 2 and same(with_areas[0], points) and same(with_areas[1], choices)
    torch.manual_seed(6)
    other = mesh.sample_points(vertices, faces, 1000)
    assert not torch.equal(other[0], points) and not torch.equal(other[1], choices)
    count = torch.bincount(choices[0], minlength=322)
    assert int(count[100]) == 0                                                     # the degenerate face


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_packed_sample_points(tag, dtype):
    counts, nv = [2, 1, 65], [4, 7, 40]
    g = torch.Generator().manual_seed(6)
    vertices = (torch.rand(sum(nv), 3, generator=g) * 2 - 1).to(dtype)
    faces = torch.cat([torch.stack([torch.randperm(v, generator=g)[:3] for _ in range(c)]) for c, v in zip(counts, nv)])
    first, per_mesh = torch.tensor([0, 4, 11, 51]), torch.tensor(counts)
    torch.manual_seed(8)
    points, choices = mesh.packed_sample_points(vertices.to(DEV), first, faces.to(DEV), per_mesh, 257)
    torch.manual_seed(8)
    r = torch.rand((3, 257), dtype=torch.float64, device=DEV).cpu()
    uv = torch.rand((3, 257, 2), dtype=dtype, device=DEV).cpu()
    merged = faces + torch.repeat_interleave(first[:-1], per_mesh)[:, None]
    areas = cpu_areas(vertices[None], merged)[0]
    begin = 0
    for b, c in enumerate(counts):
        want, margin, live = oracle.choose_faces(areas[None, begin:begin + c].numpy(), r[b:b + 1].numpy())
        assert live.all() and float(margin.min()) > 1
        assert np.array_equal(choices[b].cpu().numpy(), want[0] + begin)             # merged indices
        begin += c
    assert same(points.cpu(), cpu_blend(vertices[None].expand(3, -1, -1), merged, choices.cpu(), uv))
    torch.manual_seed(8)
    with_areas = mesh.packed_sample_points(vertices.to(DEV), first, faces.to(DEV), per_mesh, 257, areas.to(DEV))
    assert same(with_areas[0], points) and same(with_areas[1], choices)


# ---- items without area -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_items_without_area_and_no_samples(tag, dtype):
    B, F, N, D = 3, 65, 130, LANES_FROM
    vertices, faces = soup(F, B)
    vertices = vertices.to(dtype)
    feats = torch.ones(B, F, 3, D, dtype=dtype)
    v, f = vertices.to(DEV), faces.to(DEV)
    areas = mesh.face_areas(v, f)
    areas[1] = 0
    r, uv = draws(B, N, dtype, 3)
    for features_in in (feats.to(DEV), feats[..., :2].to(DEV)):
        points, choices, features, _, _ = ops.sample_points_forward_cuda(v, f, None, areas, r.to(DEV), uv.to(DEV), features_in)
        want, margin, live = oracle.choose_faces(areas.cpu().numpy(), r.numpy())
        assert list(live) == [True, False, True] and float(margin.min()) > 1
        assert bool(torch.isnan(points[1]).all()) and bool(torch.isnan(features[1]).all()) and bool((choices[1] == 0).all())
        assert np.array_equal(choices.cpu().numpy(), want)
        keep = [0, 2]
        assert same(points.cpu()[keep], cpu_blend(vertices, faces, choices.cpu(), uv)[keep])
        assert same(features.cpu()[keep], cpu_feature_blend(features_in.cpu(), choices.cpu(), uv)[keep])
    collapsed = v.clone()
    collapsed[2] = collapsed[2, :1]                                                 # every vertex of item 2 in one place
    points, choices = mesh.sample_points(collapsed, f, N)
    assert bool(torch.isnan(points[2]).all()) and bool((choices[2] == 0).all()) and bool(torch.isfinite(points[:2]).all())
    points, choices, features = mesh.sample_points(v, f, 0, face_features=feats.to(DEV))
    assert points.shape == (B, 0, 3) and points.dtype == dtype and choices.shape == (B, 0) and choices.dtype == torch.long
    assert features.shape == (B, 0, D) and features.dtype == dtype and points.device == torch.device(DEV)


# ---- gradients ----------------------------------------------------------------------------------------------------------------------
def gamma(n, dtype):
    u = 2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53
    return n * u / (1 - n * u)


def share_of_bound(got, want, term_abs_sum, n, dtype):
    """the largest |got - want| over (gamma_n(u) + gamma_n(u64)) sum|term|; NaN exactly where the reference has NaN"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    fine = ~torch.isnan(want)
    bound = (gamma(n.double(), dtype) + gamma(n.double(), torch.float64)) * term_abs_sum.detach()
    err = (got - want).abs()
    assert bool((err[fine & (bound == 0)] == 0).all())
    mask = fine & (bound > 0)
    return float((err[mask] / bound[mask]).max()) if bool(mask.any()) else 0.0


def sample_gradient_shares(dtype, vertices, faces, feats, choices, uv, cot_p, cot_f, got_v, got_f):
    """all on the CPU; vertices / feats / uv / cotangents in `dtype`"""
    B, V, F, D = vertices.shape[0], vertices.shape[1], faces.shape[0], feats.shape[-1]
    p, q = vertices.detach().double().clone().requires_grad_(), feats.detach().double().clone().requires_grad_()
    loss = (cpu_blend(p, faces, choices, uv.double()) * cot_p.double()).sum() + \
        (cpu_feature_blend(q, choices, uv.double()) * cot_f.double()).sum()
    p_grad, q_grad = torch.autograd.grad(loss, (p, q))
    u, w = torch.sqrt(uv[..., 0].double()), uv[..., 1].double()
    magnitude = (1 + u, u * (1 + w), u * w)
    tas_v, m_v = torch.zeros(B, V, 3, dtype=torch.float64), torch.zeros(B, V, 3, dtype=torch.float64)
    tas_f, m_f = torch.zeros(B, F, 3, D, dtype=torch.float64), torch.zeros(B, F, 3, D, dtype=torch.float64)
    for k in range(3):
        ids = faces[:, k][choices].unsqueeze(-1).expand(-1, -1, 3)
        tas_v.scatter_add_(1, ids, magnitude[k].unsqueeze(-1) * cot_p.double().abs())
        m_v.scatter_add_(1, ids, torch.ones_like(cot_p, dtype=torch.float64))
        rows = choices.unsqueeze(-1).expand(-1, -1, D)
        tas_f[:, :, k].scatter_add_(1, rows, magnitude[k].unsqueeze(-1) * cot_f.double().abs())
        m_f[:, :, k].scatter_add_(1, rows, torch.ones_like(cot_f, dtype=torch.float64))
    return share_of_bound(got_v, p_grad, tas_v, 4 + m_v, dtype), share_of_bound(got_f, q_grad, tas_f, 4 + m_f, dtype)


@pytest.mark.parametrize('tag,dtype', DTYPES)
@pytest.mark.parametrize('D', [3, LANES_FROM + 1])
def test_sample_points_gradients(D, tag, dtype):
    B, F, N = 2, 257, 4096                              # 16 samples per face on average: long sums at every vertex
    vertices, faces = soup(F, B)
    vertices = vertices.to(dtype)
    g = torch.Generator().manual_seed(17 + D)
    feats = (torch.rand(B, F, 3, D, generator=g) * 4 - 2).to(dtype)
    r, uv = draws(B, N, dtype, 5)
    cot_p, cot_f = (torch.rand(B, N, 3, generator=g) * 2 - 1).to(dtype), (torch.rand(B, N, D, generator=g) * 2 - 1).to(dtype)
    v, q = vertices.to(DEV).requires_grad_(), feats.to(DEV).requires_grad_()
    points, choices, features = sampling._SamplePoints.apply(v, q, faces.to(DEV), None, None, r.to(DEV), uv.to(DEV))
    assert points.requires_grad and features.requires_grad and not choices.requires_grad
    ((points * cot_p.to(DEV)).sum() + (features * cot_f.to(DEV)).sum()).backward()
    shares = sample_gradient_shares(dtype, vertices, faces, feats, choices.cpu(), uv, cot_p, cot_f, v.grad, q.grad)
    print(f'sample_points gradients {tag} D={D}: share of the bound: vertices {shares[0]:.4f}, face_features {shares[1]:.4f}')
    assert max(shares) < 1
    only_v = vertices.to(DEV).requires_grad_()
    points, _, _ = sampling._SamplePoints.apply(only_v, feats.to(DEV), faces.to(DEV), None, None, r.to(DEV), uv.to(DEV))
    (points * cot_p.to(DEV)).sum().backward()
    assert torch.allclose(only_v.grad, v.grad, rtol=1e-4 if dtype == torch.float32 else 1e-12, atol=1e-5 if dtype == torch.float32 else 1e-13)


def area_gradient_share(dtype, vertices, faces, cot, got):
    B, V = vertices.shape[:2]
    p = vertices.detach().double().clone().requires_grad_()
    want, = torch.autograd.grad((AREAS_TORCH(p, faces) * cot.double()).sum(), p)
    v0, v1, v2 = (c.double() for c in sampling._face_corners(vertices.detach(), faces))
    x, y = v0 - v1, v1 - v2
    d = torch.cross(x, y, dim=-1)
    big = torch.stack([(x[..., (i + 1) % 3] * y[..., (i + 2) % 3]).abs() + (x[..., (i + 2) % 3] * y[..., (i + 1) % 3]).abs()
                       for i in range(3)], dim=-1)
    root = d.norm(dim=-1, keepdim=True)
    n, kappa = d / root, big / root
    c = kappa + n.abs() * (n.abs() * kappa).sum(-1, keepdim=True)                       # (B, F, 3)
    half = cot.double().abs().unsqueeze(-1) / 2

    def crossed(e):       # the magnitude of (g / 2) (n x e), component by component, with the conditioning of n
        return half * torch.stack([c[..., (i + 1) % 3] * e[..., (i + 2) % 3].abs() + c[..., (i + 2) % 3] * e[..., (i + 1) % 3].abs()
                                   for i in range(3)], dim=-1)
    gx, gy = crossed(y), crossed(x)
    tas, m = torch.zeros(B, V, 3, dtype=torch.float64), torch.zeros(B, V, 3, dtype=torch.float64)
    for k, mag in enumerate((gx, gx + gy, gy)):
        ids = faces[:, k].reshape(1, -1, 1).expand(B, -1, 3)
        tas.scatter_add_(1, ids, torch.nan_to_num(mag, nan=0.0, posinf=0.0))
        m.scatter_add_(1, ids, torch.ones_like(mag))
    return share_of_bound(got, want, tas, 13 + m, dtype)


@pytest.mark.parametrize('tag,dtype', DTYPES)
def test_face_areas_gradients(tag, dtype):
    cases = {'ico': (tensor('ico_vertices'), tensor('ico_faces')), 'soup1025': soup(1025, 3)}
    for name, (vertices, faces) in cases.items():
        vertices = vertices.to(dtype)
        g = torch.Generator().manual_seed(23)
        cot = (torch.rand(vertices.shape[0], faces.shape[0], generator=g) * 2 - 1).to(dtype)
        v = vertices.to(DEV).requires_grad_()
        areas = mesh.face_areas(v, faces.to(DEV))
        grad, = torch.autograd.grad((areas * cot.to(DEV)).sum(), v, retain_graph=True)
        again, = torch.autograd.grad((areas * cot.to(DEV)).sum(), v)
        assert same(grad, again)                                                    # no atomics: the same bits
        assert bool(torch.isnan(grad).any())                                        # the vertices of the zero-area faces
        share = area_gradient_share(dtype, vertices, faces, cot, grad)
        print(f'face_areas gradient {tag} {name}: share of the bound {share:.4f}')
        assert share < 1
    # packed: the same mesh as two items
    pv, first, per_mesh = tensor('ico_packed_vertices', dtype), tensor('ico_packed_first_idx_vertices'), tensor('ico_packed_num_faces_per_mesh')
    faces = tensor('ico_faces')
    cot = (torch.rand(faces.shape[0], generator=torch.Generator().manual_seed(29)) * 2 - 1).to(dtype)
    v = pv.to(DEV).requires_grad_()
    grad, = torch.autograd.grad((mesh.packed_face_areas(v, first, faces.to(DEV), per_mesh) * cot.to(DEV)).sum(), v)
    merged = faces + torch.repeat_interleave(first[:-1], per_mesh)[:, None]
    share = area_gradient_share(dtype, pv[None], merged, cot[None], grad[None])
    print(f'packed_face_areas gradient {tag}: share of the bound {share:.4f}')
    assert share < 1


def test_gradcheck():
    vertices, faces = tensor('cases_vertices', torch.float64), tensor('cases_faces')
    vertices = vertices + torch.rand(vertices.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(2)) * 0.1
    feats = tensor('cases_face_features', torch.float64)
    r, uv = draws(2, 12, torch.float64, 9)
    v, q, f = vertices.to(DEV).requires_grad_(), feats.to(DEV).requires_grad_(), faces.to(DEV)
    assert torch.autograd.gradcheck(lambda a: mesh.face_areas(a, f), (v,))
    assert torch.autograd.gradcheck(lambda a, b: sampling._SamplePoints.apply(a, b, f, None, None, r.to(DEV), uv.to(DEV))[::2], (v, q),
                                    nondet_tol=1e-12)


# ---- graph capture ------------------------------------------------------------------------------------------------------------------
def test_operator_is_graph_capturable():
    B, F, N, D, dtype = 2, SCAN_TILE + 1, 1000, 3, torch.float32      # (three scan launches)
    vertices, faces = soup(F, B)
    g = torch.Generator().manual_seed(41)
    feats = torch.rand(B, F, 3, D, generator=g)
    r, uv = draws(B, N, dtype, 43)
    cot_p, cot_f = torch.rand(B, N, 3, generator=g) * 2 - 1, torch.rand(B, N, D, generator=g) * 2 - 1
    v, f, q, rr, uu, gp, gf = (t.to(DEV) for t in (vertices, faces, feats, r, uv, cot_p, cot_f))
    out = {}

    def step():
        points, choices, features, _, cdf = ops.sample_points_forward_cuda(v, f, None, None, rr, uu, q)
        grad_v, grad_q = ops.sample_points_backward_cuda(gp, gf, f, None, cdf, uu, choices, vertices.shape[1], D)
        out.update(points=points, choices=choices, features=features, grad_v=grad_v, grad_q=grad_q)
    step()
    eager = {k: t.clone() for k, t in out.items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for t in out.values():
        t.fill_(-7)
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(out[k], eager[k]) for k in ('points', 'choices', 'features'))
    for grads in (out, eager):
        shares = sample_gradient_shares(dtype, vertices, faces, feats, eager['choices'].cpu(), uv, cot_p, cot_f, grads['grad_v'],
                                        grads['grad_q'])
        assert max(shares) < 1, shares


# ---- the loop closes ----------------------------------------------------------------------------------------------------------------
def test_fitting_loop_closes():
    grid_vertices, tets = kuhn_grid(6)
    g = torch.Generator().manual_seed(3)
    grid_vertices = (grid_vertices + (torch.rand(grid_vertices.shape, generator=g) - 0.5) * 0.05).float()
    sdf = (0.37 - (grid_vertices - torch.tensor([0.48, 0.52, 0.5])).norm(dim=-1)).float()
    target = torch.nn.functional.normalize(torch.randn(1, 500, 3, generator=g), dim=-1) * 0.33 + 0.5
    p, s = grid_vertices[None].to(DEV).requires_grad_(), sdf[None].to(DEV).requires_grad_()
    verts, faces = marching_tetrahedra(p, tets.to(DEV), s)
    assert faces[0].shape[0] > 100
    torch.manual_seed(77)
    points, choices = mesh.sample_points(verts[0][None], faces[0], 257)
    chamfer_distance(points, target.to(DEV)).sum().backward()
    for grad in (p.grad, s.grad):
        assert bool(torch.isfinite(grad).all()) and bool(grad.abs().sum() > 0)
    # the CPU run under the same seed: the torch formulation on the draws this device's generator makes under that seed (the CPU
    # generator's stream under one seed is another one) and on this mesh's areas
    torch.manual_seed(77)
    r = torch.rand((1, 257), dtype=torch.float64, device=DEV).cpu()
    uv = torch.rand((1, 257, 2), dtype=torch.float32, device=DEV).cpu()
    mesh_v, mesh_f = verts[0][None].detach().cpu(), faces[0].cpu()
    areas = cpu_areas(mesh_v, mesh_f)
    assert same(mesh.face_areas(verts[0][None].detach(), faces[0]).cpu(), areas)
    cpu_points, cpu_choices, _ = SAMPLE_TORCH(mesh_v, mesh_f, areas, r, uv, sqrt=oracle.ieee_sqrt)
    assert float(oracle.choose_faces(areas.numpy(), r.numpy())[1].min()) > 1
    assert torch.equal(choices.cpu(), cpu_choices) and same(points.detach().cpu(), cpu_points)
