"""kaolin.ops.conversions.voxelgrids_to_cubic_meshes on the GPU: the sort-free HIP pipeline (csrc/cubic_meshes.hip) against the
reference's recorded answers for every golden case and both modes, against the package's CPU path at sizes the goldens do not
reach, at 256^3 against closed forms, and end to end into point_to_mesh_distance.  torch.equal everywhere but the last."""
import re

import pytest
import torch

import kaolin_amd as kal
from kaolin_amd import _C
from kaolin_amd.ops.conversions import voxelgrids_to_cubic_meshes
from cubic_meshes_golden import CASES, assert_same_meshes, check_binary_invariants, expected, grid, signed_volume

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
MODES = pytest.mark.parametrize('is_trimesh', [True, False], ids=['tri', 'quad'])
HIP_DTYPES = [torch.bool, torch.uint8, torch.float16, torch.float32]          # read in place by the kernels
CAST_DTYPES = [torch.int32, torch.int64, torch.float64, torch.bfloat16]       # cast once with .float()


@MODES
@pytest.mark.parametrize('name', CASES)
def test_matches_reference(name, is_trimesh):
    got = voxelgrids_to_cubic_meshes(grid(name).float().to(DEV), is_trimesh)
    assert_same_meshes(got, expected(name, is_trimesh), device=DEV)


@MODES
@pytest.mark.parametrize('dtype', HIP_DTYPES + CAST_DTYPES, ids=lambda d: str(d).split('.')[-1])
def test_dtypes(dtype, is_trimesh):
    for name in ('rand12', 'wave_tail'):
        got = voxelgrids_to_cubic_meshes(grid(name).to(DEV).to(dtype), is_trimesh)
        assert_same_meshes(got, expected(name, is_trimesh), device=DEV)


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32, torch.float64], ids=lambda d: str(d).split('.')[-1])
def test_values(dtype):
    """Non-binary values (all exact in half): faces follow rint(hi - lo), inverted only at -1."""
    x = grid('values').to(DEV).to(dtype)
    assert_same_meshes(voxelgrids_to_cubic_meshes(x), expected('values', True), device=DEV)
    assert_same_meshes(voxelgrids_to_cubic_meshes(x, is_trimesh=False), expected('values', False), device=DEV)


def test_shim_is_the_hip_path():
    """The public function hands GPU tensors to _C.ops.conversions.voxelgrids_to_cubic_meshes_cuda, which rejects CPU tensors
    (no fallback inside the shim)."""
    x = grid('hollow').to(DEV)
    assert_same_meshes(_C.ops.conversions.voxelgrids_to_cubic_meshes_cuda(x, False), expected('hollow', False), device=DEV)
    with pytest.raises(RuntimeError, match='must be a CUDA tensor'):
        _C.ops.conversions.voxelgrids_to_cubic_meshes_cuda(grid('hollow'))


@pytest.mark.parametrize('name', ['wave_tail', 'rand12', 'batch'])
def test_non_contiguous(name):
    want = expected(name, True)
    x = grid(name).to(DEV).float()
    permuted = x.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)           # Z is the slowest axis in memory
    assert not permuted.is_contiguous()
    assert_same_meshes(voxelgrids_to_cubic_meshes(permuted), want, device=DEV)
    padded = torch.full((x.shape[0], x.shape[1] + 2, x.shape[2] + 3, 2 * x.shape[3] + 1), 7., device=DEV)
    sliced = padded[:, 1:-1, 2:-1, 1::2]                                        # offsets and a step of 2 along Z
    sliced.copy_(x)
    assert not sliced.is_contiguous()
    assert_same_meshes(voxelgrids_to_cubic_meshes(sliced), want, device=DEV)
    half = padded.half()[:, 1:-1, 2:-1, 1::2]
    assert half.dtype == torch.float16 and not half.is_contiguous()
    assert_same_meshes(voxelgrids_to_cubic_meshes(half, False), expected(name, False), device=DEV)
    flipped = x.flip(1, 3)
    assert_same_meshes(voxelgrids_to_cubic_meshes(flipped), voxelgrids_to_cubic_meshes(flipped.cpu()), device=DEV)
    one = x[:1, :, :, :1].expand(2, -1, -1, 5)                                   # strides of 0 along the batch and Z
    assert_same_meshes(voxelgrids_to_cubic_meshes(one), voxelgrids_to_cubic_meshes(one.cpu()), device=DEV)


def test_repeatable_and_stream_independent():
    x = grid('wave_tail').to(DEV)
    y = grid('rand12').to(DEV).float()
    first, second = voxelgrids_to_cubic_meshes(x), voxelgrids_to_cubic_meshes(x)
    assert_same_meshes(second, first, device=DEV)
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        on_side = voxelgrids_to_cubic_meshes(x)
        on_side_quads = voxelgrids_to_cubic_meshes(y, is_trimesh=False)
    side.synchronize()
    assert_same_meshes(on_side, first, device=DEV)
    assert_same_meshes(on_side_quads, expected('rand12', False), device=DEV)


def test_edge_arguments():
    assert voxelgrids_to_cubic_meshes(torch.zeros(0, 3, 3, 3, device=DEV)) == ([], [])
    for shape in ((3, 4, 5), (1, 1, 3, 4, 5)):
        with pytest.raises(ValueError, match=re.escape(f'Expected voxelgrids to have 4 dimensions but got {len(shape)} dimensions.')):
            voxelgrids_to_cubic_meshes(torch.zeros(shape, device=DEV))
    for shape in ((2, 3, 4, 5), (2, 0, 4, 5), (1, 3, 4, 0)):
        for is_trimesh in (True, False):
            verts, faces = voxelgrids_to_cubic_meshes(torch.zeros(shape, device=DEV), is_trimesh)
            assert_same_meshes((verts, faces), voxelgrids_to_cubic_meshes(torch.zeros(shape), is_trimesh), device=DEV)
    out = voxelgrids_to_cubic_meshes(grid('hollow').float().to(DEV).requires_grad_())
    assert_same_meshes(out, expected('hollow', True), device=DEV)               # (checks requires_grad of both results too)
    huge = torch.zeros(1, device=DEV).expand(1, 2048, 1024, 1024)                # 2049 * 1025 * 1025 lattice points >= 2^31
    with pytest.raises(RuntimeError, match=re.escape('must stay below 2^31')):
        voxelgrids_to_cubic_meshes(huge)


@MODES
def test_cpu_path_equals_gpu_path_random(is_trimesh):
    """(2, 33, 17, 65): odd sizes, Z + 1 = 66 just past a wavefront, 34 * 18 * 66 = 40392 lattice points = 157.8 workgroups per
    item, so the second item starts in a workgroup of its own after a partial one."""
    g = torch.Generator().manual_seed(11)
    x = torch.rand((2, 33, 17, 65), generator=g) < 0.5
    assert_same_meshes(voxelgrids_to_cubic_meshes(x.to(DEV), is_trimesh), voxelgrids_to_cubic_meshes(x, is_trimesh), device=DEV)
    # 258 small items: the prefix over the batch walks it in rounds of 256, so the last two items start after a carried round
    many = torch.rand((258, 2, 3, 2), generator=g) < 0.5
    assert_same_meshes(voxelgrids_to_cubic_meshes(many.to(DEV), is_trimesh), voxelgrids_to_cubic_meshes(many, is_trimesh), device=DEV)


@pytest.fixture(scope='module')
def sphere96():
    """bool (1, 96, 96, 96) on the GPU: the voxelized geodesic sphere, filled."""
    from kaolin_amd.utils.testing import geodesic_sphere
    v, f = geodesic_sphere(16)
    shell = kal.ops.conversions.trianglemeshes_to_voxelgrids(v.float()[None].to(DEV), f.to(DEV), 96)
    return kal.ops.voxelgrid.fill(shell)


@pytest.fixture(scope='module')
def sphere96_meshes(sphere96):
    return voxelgrids_to_cubic_meshes(sphere96), voxelgrids_to_cubic_meshes(sphere96, is_trimesh=False)


def test_cpu_path_equals_gpu_path_sphere(sphere96, sphere96_meshes):
    tri, quad = sphere96_meshes
    x = sphere96.cpu()
    assert 300000 < int(x.sum()) < 96 ** 3 // 2 + 50000
    assert_same_meshes(tri, voxelgrids_to_cubic_meshes(x), device=DEV)
    assert_same_meshes(quad, voxelgrids_to_cubic_meshes(x, is_trimesh=False), device=DEV)
    check_binary_invariants(sphere96[0], quad[0][0], quad[1][0], tri[1][0])


@pytest.mark.parametrize('dtype', [torch.bool, torch.float16], ids=['bool', 'half'])
def test_box_256(dtype):
    """An axis-aligned solid box a x b x c strictly inside a 256^3 grid: V = (a+1)(b+1)(c+1) - (a-1)(b-1)(c-1) lattice points on
    its surface, N = 2 (ab + bc + ca) quads, signed volume abc.  257^3 lattice points = 66307 workgroups."""
    a, b, c = 200, 101, 57
    x = torch.zeros((1, 256, 256, 256), dtype=dtype, device=DEV)
    x[0, 13:13 + a, 70:70 + b, 100:100 + c] = 1
    verts, quads = voxelgrids_to_cubic_meshes(x, is_trimesh=False)
    verts_t, tris = voxelgrids_to_cubic_meshes(x)
    n = 2 * (a * b + b * c + c * a)
    assert verts[0].shape == ((a + 1) * (b + 1) * (c + 1) - (a - 1) * (b - 1) * (c - 1), 3)
    assert quads[0].shape == (n, 4) and tris[0].shape == (2 * n, 3) and torch.equal(verts[0], verts_t[0])
    assert signed_volume(verts[0], tris[0]) == float(a * b * c)
    lo, hi = verts[0].amin(0).tolist(), verts[0].amax(0).tolist()
    assert lo == [13., 70., 100.] and hi == [13. + a, 70. + b, 100. + c]
    assert torch.equal(torch.unique(quads[0]), torch.arange(verts[0].shape[0], device=DEV))
    # lexicographic order of the vertices
    key = (verts[0][:, 0].long() * 257 + verts[0][:, 1].long()) * 257 + verts[0][:, 2].long()
    assert bool((key[1:] > key[:-1]).all())


def test_into_point_to_mesh_distance(sphere96, sphere96_meshes):
    """The cubified sphere is a mesh the package's own consumers take: through index_vertices_by_faces into
    point_to_mesh_distance.  The centre of a voxel of the thin surface shell (an occupied voxel with an empty 6-neighbour) is
    0.5 from the exposed face between them and no point of the mesh, which lies on voxel boundaries, is nearer: the squared
    distance is 0.25.  Tolerance: coordinates are below 2^7 and exact in float32, the closest-point arithmetic loses a few
    ulps of 2^7 * 2^-24 = 8e-6 per coordinate, so the squared distance is within 1e-4 of 0.25."""
    (verts, tris), _ = sphere96_meshes
    shell = kal.ops.voxelgrid.extract_surface(sphere96, mode='thin')
    centres = torch.nonzero(shell[0]).float() + 0.5
    centres = centres[::max(1, centres.shape[0] // 4096)]
    assert centres.shape[0] >= 4096
    face_vertices = kal.ops.mesh.index_vertices_by_faces(verts[0].unsqueeze(0), tris[0])
    dist, face_idx, _ = kal.metrics.trianglemesh.point_to_mesh_distance(centres.unsqueeze(0), face_vertices)
    assert float(dist.max()) <= 0.25 + 1e-4, float(dist.max())
    assert float(dist.min()) >= 0.25 - 1e-4, float(dist.min())
    assert int(face_idx.min()) >= 0 and int(face_idx.max()) < tris[0].shape[0]
