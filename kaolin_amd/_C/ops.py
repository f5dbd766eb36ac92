"""Host shims of ``kaolin._C.ops`` operators, plus the fused voxelizer (the reference has no ``kaolin._C`` operator for
it: the op is pure PyTorch, kaolin/ops/conversions/trianglemesh.py:29-110; that entry point exists only on our side)."""
import ctypes

import torch

from .. import _lib
from .._checks import torch_check


def trianglemeshes_to_voxelgrids_cuda(vertices, faces, resolution, origin=None, scale=None, return_sparse=False):
    """vertices (B, V, 3) raw; faces (F, 3) int64 shared by the batch; origin (B, 3) / scale (B) of the normalisation
    ``(vertices - origin) / scale`` or None (per-mesh minimum / largest extent, computed on the device)
    -> dense (B, R, R, R) grid of 0/1 in the vertices' dtype; ``return_sparse``: the same as a coalesced sparse COO tensor built
    from a BIT grid (R^3 / 8 bytes per mesh) -- R^3 scalars are never allocated (reference: the COO of the unique voxel indices,
    kaolin/ops/conversions/pointcloud.py:66-73)."""
    fn = 'trianglemeshes_to_voxelgrids_cuda'
    torch_check(vertices.is_cuda and faces.is_cuda, f'{fn}: vertices and faces must be CUDA tensors')
    torch_check(vertices.dim() == 3 and vertices.size(2) == 3, 'vertices must of size {batch_size, num_vertices, 3}')
    torch_check(faces.dim() == 2 and faces.size(1) == 3, 'faces must of size {num_faces, 3}')
    torch_check(faces.dtype == torch.long, 'faces must be long')
    v = vertices.contiguous()
    f = faces.contiguous()
    sfx = _lib.dtype_suffix(v.dtype, fn)
    B, V, F, R = v.size(0), v.size(1), f.size(0), int(resolution)
    if origin is not None:
        torch_check(origin.is_cuda and tuple(origin.shape) == (B, 3), 'origin must be a CUDA tensor of size {batch_size, 3}')
        origin = origin.to(v.dtype).contiguous()
    if scale is not None:
        torch_check(scale.is_cuda and scale.numel() == B, 'scale must be a CUDA tensor of size {batch_size}')
        scale = scale.to(v.dtype).reshape(B).contiguous()
    from .render.mesh import faces_in_range
    if not faces_in_range(f, V):
        # the kernels gather vertices unchecked; the reference's indexing raises (a device assert) on such a mesh
        raise IndexError(f'{fn}: faces hold an index outside [0, num_vertices)')
    lib = _lib.load()
    if return_sparse:
        with _lib.on_device(v.device):
            words = int(lib.kamd_trianglemeshes_to_voxelbits_words(R))
            bits = torch.empty((B, words), dtype=torch.int32, device=v.device)
            norm = _lib.workspace(lib.kamd_trianglemeshes_to_voxelgrids_workspace(B, V, v.element_size()), v.device)
            st = getattr(lib, f'kamd_trianglemeshes_to_voxelbits_{sfx}')(
                _lib.stream_ptr(v.device), B, V, F, R, _lib.ptr(v), _lib.ptr(f), _lib.ptr(origin), _lib.ptr(scale), _lib.ptr(norm),
                _lib.ptr(bits))
        _lib.check(st, fn)
        # compaction, sized by the occupied words: (mesh, word) of every non-zero word, its 32 bits, the set ones -> linear
        # voxel indices in ascending order per mesh (= the order of a coalesced COO tensor)
        nzw = torch.nonzero(bits)                                           # (n_words, 2), lexicographic
        w = bits[nzw[:, 0], nzw[:, 1]]
        on = ((w.unsqueeze(1) >> torch.arange(32, device=v.device, dtype=torch.int32)) & 1).bool()   # (n_words, 32)
        sel = torch.nonzero(on)                                             # (nnz, 2): (word slot, bit), lexicographic
        lin = nzw[sel[:, 0], 1] * 32 + sel[:, 1]
        idx = torch.stack([nzw[sel[:, 0], 0], lin // (R * R), (lin // R) % R, lin % R])
        return torch.sparse_coo_tensor(idx, torch.ones(idx.shape[1], dtype=v.dtype, device=v.device), (B, R, R, R),
                                       is_coalesced=True)
    with _lib.on_device(v.device):
        grid = torch.empty((B, R, R, R), dtype=v.dtype, device=v.device)
        norm = _lib.workspace(lib.kamd_trianglemeshes_to_voxelgrids_workspace(B, V, v.element_size()), v.device)
        st = getattr(lib, f'kamd_trianglemeshes_to_voxelgrids_{sfx}')(
            _lib.stream_ptr(v.device), B, V, F, R, _lib.ptr(v), _lib.ptr(f), _lib.ptr(origin), _lib.ptr(scale), _lib.ptr(norm),
            _lib.ptr(grid))
    _lib.check(st, fn)
    return grid


def unbatched_mesh_intersection_cuda(points, verts_1, verts_2, verts_3):
    """reference: kaolin/csrc/ops/mesh/mesh_intersection.cpp (bindings.cpp, ``_C.ops.mesh.unbatched_mesh_intersection_cuda``):
    points (N,3), verts_k (F,3) -> (N) tensor, the number of faces the +x ray from every point crosses."""
    fn = 'unbatched_mesh_intersection_cuda'
    for name, t in (('points', points), ('verts_1', verts_1), ('verts_2', verts_2), ('verts_3', verts_3)):
        torch_check(t.is_cuda, f'{name} must be a CUDA tensor')
    for name, t in (('points', points), ('verts_1', verts_1), ('verts_2', verts_2), ('verts_3', verts_3)):
        torch_check(t.is_contiguous(), f'{name} must be contiguous')
    n, m = points.size(0), verts_1.size(0)
    torch_check(list(points.shape) == [n, 3], 'points must of size {num_points, 3}')
    for name, t in (('verts_1', verts_1), ('verts_2', verts_2), ('verts_3', verts_3)):
        torch_check(list(t.shape) == [m, 3], f'{name} must of size {{num_faces, 3}}')
        torch_check(t.dtype == points.dtype, 'expected points and vertices to have the same scalar type')
    sfx = _lib.dtype_suffix(points.dtype, fn)
    lib = _lib.load()
    with _lib.on_device(points.device):
        result = torch.empty(n, dtype=points.dtype, device=points.device)
        st = getattr(lib, f'kamd_mesh_intersection_{sfx}')(
            _lib.stream_ptr(points.device), n, m, _lib.ptr(points), _lib.ptr(verts_1), _lib.ptr(verts_2),
            _lib.ptr(verts_3), _lib.ptr(result))
    _lib.check(st, fn)
    return result


def mesh_to_spc_cuda(face_vertices, level):
    """reference: kaolin/csrc/ops/conversions/mesh_to_spc/mesh_to_spc.cpp:27-42 (``_C.ops.conversions.mesh_to_spc_cuda``):
    face_vertices (F,3,3) float32 in [-1,1]^3 -> [octree uint8 (num_nodes), face_ids int64 (num_voxels),
    barycoords float (num_voxels, 2)]; nothing occupied -> sizes (0,), (0,), (0, 3) as in the reference.

    Result sizes depend on the data, so the host reads one count per stage of three octree levels and the level
    sizes once (the reference reads one count per level, twice); see include/kaolin_amd.h for the sequence."""
    fn = 'mesh_to_spc_cuda'
    torch_check(face_vertices.is_cuda, 'face_vertices must be a CUDA tensor')
    torch_check(face_vertices.is_contiguous(), 'face_vertices must be contiguous')
    torch_check(face_vertices.dim() == 3, f'face_vertices must have 3 dimensions, but got {face_vertices.dim()}')
    torch_check(face_vertices.size(1) == 3, f'face_vertices must have size 3 on dimension 1, but got {face_vertices.size(1)}')
    torch_check(face_vertices.size(2) == 3, f'face_vertices must have size 3 on dimension 2, but got {face_vertices.size(2)}')
    torch_check(face_vertices.dtype == torch.float32, 'expected scalar type Float but found ' + _lib.pretty_dtype(face_vertices.dtype))
    level = int(level)
    torch_check(0 <= level <= 15, 'level must be in [0, 15]')
    dev = face_vertices.device
    lib = _lib.load()
    sp = _lib.stream_ptr(dev)
    depth = lib.kamd_mesh_to_spc_stage_levels()

    def empty_result():
        return [torch.empty(0, dtype=torch.uint8, device=dev), torch.empty(0, dtype=torch.long, device=dev),
                torch.zeros((0, 3), dtype=torch.float32, device=dev)]

    with _lib.on_device(dev):
        n = face_vertices.size(0)
        if n == 0:
            return empty_result()
        morton = torch.zeros(n, dtype=torch.long, device=dev)
        tri = torch.arange(n, dtype=torch.long, device=dev)
        level_from, tested = 0, 0
        while True:
            level_to = min(level_from + depth, level)
            counts = torch.empty(n, dtype=torch.int32, device=dev)
            offsets = torch.empty(n + 1, dtype=torch.long, device=dev)
            scan_ws = torch.empty(lib.kamd_mesh_to_spc_scan_workspace(n), dtype=torch.uint8, device=dev)
            _lib.check(lib.kamd_mesh_to_spc_stage_count(sp, n, _lib.ptr(face_vertices), _lib.ptr(morton), _lib.ptr(tri),
                                                        level_from, level_to, tested, _lib.ptr(counts), _lib.ptr(offsets),
                                                        _lib.ptr(scan_ws)), fn)
            total = int(offsets[n].item())                     # data-dependent size: one host read per stage
            if total == 0:
                return empty_result()
            morton_out = torch.empty(total, dtype=torch.long, device=dev)
            tri_out = torch.empty(total, dtype=torch.long, device=dev)
            _lib.check(lib.kamd_mesh_to_spc_stage_emit(sp, n, _lib.ptr(face_vertices), _lib.ptr(morton), _lib.ptr(tri),
                                                       level_from, level_to, tested, _lib.ptr(offsets), _lib.ptr(morton_out),
                                                       _lib.ptr(tri_out)), fn)
            morton, tri, n = morton_out, tri_out, total
            if level_to == level:
                break
            level_from, tested = level_to, 1
        nbytes = lib.kamd_mesh_to_spc_build_workspace(n, level)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        sizes = torch.empty(1 + level, dtype=torch.long, device=dev)
        _lib.check(lib.kamd_mesh_to_spc_build(sp, n, level, _lib.ptr(morton), _lib.ptr(tri), _lib.ptr(ws), nbytes,
                                              _lib.ptr(sizes)), fn)
        host_sizes = sizes.tolist()                            # voxels + nodes per octree level: one host read
        num_voxels, octree_bytes = host_sizes[0], sum(host_sizes[1:])
        octree = torch.empty(octree_bytes, dtype=torch.uint8, device=dev)
        face_ids = torch.empty(num_voxels, dtype=torch.long, device=dev)
        bary = torch.empty((num_voxels, 2), dtype=torch.float32, device=dev)
        _lib.check(lib.kamd_mesh_to_spc_results(sp, n, level, _lib.ptr(face_vertices), _lib.ptr(ws), num_voxels, octree_bytes,
                                                _lib.ptr(octree), _lib.ptr(face_ids), _lib.ptr(bary)), fn)
    return [octree, face_ids, bary]


def _gs_float_args(fn, named):
    """float32, one device, contiguous"""
    for name, t in named:
        torch_check(t.dtype == torch.float32, f'{fn}: expected scalar type Float for {name} but found ' + _lib.pretty_dtype(t.dtype))
        torch_check(t.is_contiguous(), f'{fn}: {name} must be contiguous')


def _gs_one_device(fn, named):
    devices = {t.device for _, t in named}
    torch_check(len(devices) == 1, f'{fn}: expected every tensor on one device, got {[str(t.device) for _, t in named]}')
    return next(iter(devices))


def _gs_level(fn, level):
    level = int(level)
    torch_check(0 <= level <= 15, f'{fn}: level must be in [0, 15]')
    return level


def gs_to_spc_cuda(means3D, scales, rotations, iso, tol, level):
    """reference: kaolin/csrc/ops/conversions/gs_to_spc/gs_to_spc.cpp (``_C.ops.conversions.gs_to_spc_cuda``): means3D (G,3),
    scales (G,3), rotations (G,4) float32 -> [points int16 (N,3), gaus_id int64 (N), pack_boundary bool (N), cov3d_invs float (G,6)]:
    one pair per (voxel of ``level``, Gaussian whose iso ellipsoid overlaps it and all its ancestors), ordered by (Morton code,
    Gaussian id); pack_boundary marks the first pair of every voxel.  No pair (G = 0 included): N = 0 and cov3d_invs still (G, 6).

    Launches: 1 (prepare) + 4 per stage of three levels (count, two of the scan, emit; max(1, ceil(level / 3)) stages) + 4 per
    sort pass (ceil(3 level / 8) passes; one copy at level 0) + 2 (run heads, points); one host read per stage: not capturable.  CPU tensors run the torch formulation of kaolin_amd/ops/conversions/gaussians.py (the same integer results)."""
    fn = 'gs_to_spc_cuda'
    named = (('means3D', means3D), ('scales', scales), ('rotations', rotations))
    _gs_float_args(fn, named)
    dev = _gs_one_device(fn, named)
    G = means3D.size(0) if means3D.dim() > 0 else -1
    torch_check(list(means3D.shape) == [G, 3], f'{fn}: means3D must be of size {{num_gaussians, 3}}, got {list(means3D.shape)}')
    torch_check(list(scales.shape) == [G, 3], f'{fn}: scales must be of size {{num_gaussians, 3}}, got {list(scales.shape)}')
    torch_check(list(rotations.shape) == [G, 4], f'{fn}: rotations must be of size {{num_gaussians, 4}}, got {list(rotations.shape)}')
    level = _gs_level(fn, level)
    iso, tol = float(iso), float(tol)
    if not means3D.is_cuda:
        from ..ops.conversions.gaussians import gs_to_spc_torch
        return gs_to_spc_torch(means3D, scales, rotations, iso, tol, level)
    lib = _lib.load()
    sp = _lib.stream_ptr(dev)
    depth = lib.kamd_gs_to_spc_stage_levels()
    with _lib.on_device(dev):
        cov = torch.empty((G, 6), dtype=torch.float32, device=dev)

        def empty_result():
            return [torch.empty((0, 3), dtype=torch.int16, device=dev), torch.empty(0, dtype=torch.long, device=dev),
                    torch.empty(0, dtype=torch.bool, device=dev), cov]

        if G == 0:
            return empty_result()
        prep = torch.empty(lib.kamd_gs_to_spc_prepare_workspace(G), dtype=torch.uint8, device=dev)
        _lib.check(lib.kamd_gs_to_spc_prepare(sp, G, _lib.ptr(means3D), _lib.ptr(scales), _lib.ptr(rotations), iso, tol, level,
                                              _lib.ptr(cov), _lib.ptr(prep)), fn)
        n = G
        morton = torch.zeros(n, dtype=torch.long, device=dev)
        gid = torch.arange(n, dtype=torch.long, device=dev)
        level_from, tested = 0, 0
        while True:
            level_to = min(level_from + depth, level)
            counts = torch.empty(n, dtype=torch.int32, device=dev)
            offsets = torch.empty(n + 1, dtype=torch.long, device=dev)
            scan_ws = torch.empty(lib.kamd_gs_to_spc_scan_workspace(n), dtype=torch.uint8, device=dev)
            head = (sp, n, G, _lib.ptr(means3D), _lib.ptr(cov), _lib.ptr(prep), iso, _lib.ptr(morton), _lib.ptr(gid), level_from,
                    level_to, tested)
            _lib.check(lib.kamd_gs_to_spc_stage_count(*head, _lib.ptr(counts), _lib.ptr(offsets), _lib.ptr(scan_ws)), fn)
            total = int(offsets[n].item())                     # data-dependent size: one host read per stage
            if total == 0:
                return empty_result()
            morton_out = torch.empty(total, dtype=torch.long, device=dev)
            gid_out = torch.empty(total, dtype=torch.long, device=dev)
            _lib.check(lib.kamd_gs_to_spc_stage_emit(*head, _lib.ptr(offsets), total, _lib.ptr(morton_out), _lib.ptr(gid_out)), fn)
            morton, gid, n = morton_out, gid_out, total
            if level_to == level:
                break
            level_from, tested = level_to, 1
        nbytes = lib.kamd_gs_to_spc_finish_workspace(n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        points = torch.empty((n, 3), dtype=torch.int16, device=dev)
        gaus_id = torch.empty(n, dtype=torch.long, device=dev)
        boundary = torch.empty(n, dtype=torch.bool, device=dev)
        _lib.check(lib.kamd_gs_to_spc_finish(sp, n, level, _lib.ptr(morton), _lib.ptr(gid), _lib.ptr(ws), nbytes, _lib.ptr(points),
                                             _lib.ptr(gaus_id), _lib.ptr(boundary)), fn)
    return [points, gaus_id, boundary, cov]


def integrate_gs_cuda(points, gaus_id, means3D, cov3d_invs, opacities, level, step):
    """reference: gs_to_spc.cpp (``_C.ops.conversions.integrate_gs_cuda``): points int16 (N,3), gaus_id int64 (N), means3D (G,3),
    cov3d_invs (G,6), opacities (G) or (G,1) float32 -> float32 (N): opacity times the mean of exp(-q / 2) over ``step``^3 samples of
    the voxel, accumulated in float64 in a fixed order (the same bits every run).  One launch, no host read: capturable."""
    fn = 'integrate_gs_cuda'
    floats = (('means3D', means3D), ('cov3d_invs', cov3d_invs), ('opacities', opacities))
    _gs_float_args(fn, floats)
    torch_check(points.dtype == torch.int16, f'{fn}: expected scalar type Short for points but found ' + _lib.pretty_dtype(points.dtype))
    torch_check(gaus_id.dtype == torch.long, f'{fn}: expected scalar type Long for gaus_id but found ' + _lib.pretty_dtype(gaus_id.dtype))
    torch_check(points.is_contiguous() and gaus_id.is_contiguous(), f'{fn}: points and gaus_id must be contiguous')
    dev = _gs_one_device(fn, (('points', points), ('gaus_id', gaus_id)) + floats)
    N = points.size(0) if points.dim() > 0 else -1
    G = means3D.size(0) if means3D.dim() > 0 else -1
    torch_check(list(points.shape) == [N, 3], f'{fn}: points must be of size {{num_pairs, 3}}, got {list(points.shape)}')
    torch_check(list(gaus_id.shape) == [N], f'{fn}: gaus_id must be of size {{num_pairs}}, got {list(gaus_id.shape)}')
    torch_check(list(means3D.shape) == [G, 3], f'{fn}: means3D must be of size {{num_gaussians, 3}}, got {list(means3D.shape)}')
    torch_check(list(cov3d_invs.shape) == [G, 6], f'{fn}: cov3d_invs must be of size {{num_gaussians, 6}}, got {list(cov3d_invs.shape)}')
    torch_check(opacities.numel() == G, f'{fn}: {opacities.numel()} opacities for {G} Gaussians')
    level, step = _gs_level(fn, level), int(step)
    torch_check(1 <= step <= 1024, f'{fn}: step must be in [1, 1024]')
    if not points.is_cuda:
        from ..ops.conversions.gaussians import integrate_gs_torch
        return integrate_gs_torch(points, gaus_id, means3D, cov3d_invs, opacities, level, step)
    with _lib.on_device(dev):
        values = torch.empty(N, dtype=torch.float32, device=dev)
        if N > 0:
            _lib.check(_lib.load().kamd_integrate_gs(_lib.stream_ptr(dev), N, G, _lib.ptr(points), _lib.ptr(gaus_id), _lib.ptr(means3D),
                                                     _lib.ptr(cov3d_invs), _lib.ptr(opacities), level, step, _lib.ptr(values)), fn)
    return values


_FILL_SUFFIX = {torch.bool: 'u8', torch.uint8: 'u8', torch.int32: 'i32', torch.int64: 'i64', torch.float16: 'f16',
                torch.float32: 'f32', torch.float64: 'f64'}


def voxelgrid_fill_cuda(voxelgrids, stats=None):
    """voxelgrids (N, X, Y, Z), any strides; bool / uint8 / int32 / int64 / half / float / double -> bool (N, X, Y, Z): the
    walls (value != 0) and every cavity the outside does not reach through faces (csrc/voxelgrid_fill.hip).  No reference
    operator: kaolin.ops.voxelgrid.fill raises on a GPU tensor.  The call synchronises the current stream (the host reads
    a flag every few passes), so it cannot be captured in a graph.  ``stats``: a dict that receives ``passes`` (passes that
    worked), ``launched`` and ``polls``."""
    fn = 'voxelgrid_fill_cuda'
    torch_check(voxelgrids.is_cuda, f'{fn}: voxelgrids must be a CUDA tensor')
    torch_check(voxelgrids.dim() == 4, f'{fn}: voxelgrids must of size {{batch_size, X, Y, Z}}')
    sfx = _FILL_SUFFIX.get(voxelgrids.dtype)
    if sfx is None:
        raise RuntimeError(f'"{fn}" not implemented for \'{_lib.pretty_dtype(voxelgrids.dtype)}\'')
    N, X, Y, Z = voxelgrids.shape
    torch_check(max(X, Y, Z) < 2 ** 31, f'{fn}: a grid dimension exceeds the 32-bit range')
    dev = voxelgrids.device
    lib = _lib.load()
    host = (ctypes.c_int32 * 3)()
    with _lib.on_device(dev):
        out = torch.empty((N, X, Y, Z), dtype=torch.bool, device=dev)
        if out.numel() > 0:
            ws = _lib.workspace(lib.kamd_voxelgrid_fill_workspace(N, X, Y, Z), dev)
            st = getattr(lib, f'kamd_voxelgrid_fill_{sfx}')(
                _lib.stream_ptr(dev), N, X, Y, Z, _lib.ptr(voxelgrids), *voxelgrids.stride(), _lib.ptr(out), _lib.ptr(ws),
                ctypes.cast(host, ctypes.c_void_p))
            _lib.check(st, fn)
    if stats is not None:
        stats.update(passes=host[0], launched=host[1], polls=host[2])
    return out


_CUBIC_SUFFIX = {torch.bool: 'u8', torch.uint8: 'u8', torch.float16: 'f16', torch.float32: 'f32'}


def voxelgrids_to_cubic_meshes_cuda(voxelgrids, is_trimesh=True):
    """kaolin.ops.conversions.voxelgrids_to_cubic_meshes on the sort-free HIP pipeline of csrc/cubic_meshes.hip (the reference has
    no ``_C`` operator here: its voxelgrid.py is conv3d, nonzero and a torch.unique(dim=0) per item).  voxelgrids (B, X, Y, Z),
    any strides; bool / uint8 / half / float are read in place, any other dtype is cast once with ``.float()`` as the reference
    does -> (verts, faces): two lists of B tensors, verts[b] (V_b, 3) float32 and faces[b] (2 N_b, 3) or (N_b, 4) int64, views of
    one vertex buffer and one face buffer for the batch.  Result sizes depend on the data: the host reads the B x 4 totals
    once, so the call synchronises the current stream and cannot be captured in a graph (like the reference, whose nonzero and
    torch.unique synchronise)."""
    fn = 'voxelgrids_to_cubic_meshes_cuda'
    torch_check(voxelgrids.is_cuda, f'{fn}: voxelgrids must be a CUDA tensor')
    torch_check(voxelgrids.dim() == 4, f'{fn}: voxelgrids must of size {{batch_size, X, Y, Z}}')
    v = voxelgrids.detach()
    sfx = _CUBIC_SUFFIX.get(v.dtype)
    if sfx is None:
        v = v.float()
        sfx = 'f32'
    B, X, Y, Z = v.shape
    width = 3 if is_trimesh else 4
    dev = v.device
    if B == 0:
        return [], []
    torch_check((X + 1) * (Y + 1) * (Z + 1) < 2 ** 31,
                f'{fn}: the lattice (X + 1)(Y + 1)(Z + 1) = {(X + 1) * (Y + 1) * (Z + 1)} of one item must stay below 2^31')
    lib = _lib.load()
    sp = _lib.stream_ptr(dev)
    totals = None
    with _lib.on_device(dev):
        if v.numel() > 0:
            nbytes = lib.kamd_cubic_meshes_workspace(B, X, Y, Z)
            torch_check(nbytes > 0, f'{fn}: a batch of {B} grids of {X} x {Y} x {Z} is beyond the launch range')
            ws = _lib.workspace(nbytes, dev)
            _lib.check(getattr(lib, f'kamd_cubic_meshes_classify_{sfx}')(
                sp, B, X, Y, Z, _lib.ptr(v), *v.stride(), _lib.ptr(ws)), fn)
            host = (ctypes.c_uint32 * (4 * B))()
            _lib.check(lib.kamd_cubic_meshes_scan(sp, B, X, Y, Z, _lib.ptr(ws), ctypes.cast(host, ctypes.c_void_p)), fn)
            totals = list(host)                                # data-dependent sizes: the one host read
        nv = [totals[4 * b] for b in range(B)] if totals else [0] * B
        nq = [sum(totals[4 * b + 1:4 * b + 4]) for b in range(B)] if totals else [0] * B
        verts = torch.empty((sum(nv), 3), dtype=torch.float32, device=dev)
        faces = torch.empty(((2 if is_trimesh else 1) * sum(nq), width), dtype=torch.long, device=dev)
        if faces.numel() > 0:
            _lib.check(lib.kamd_cubic_meshes_emit_vertices(sp, B, X, Y, Z, _lib.ptr(ws), _lib.ptr(verts)), fn)
            _lib.check(lib.kamd_cubic_meshes_emit_faces(sp, B, X, Y, Z, _lib.ptr(ws), int(bool(is_trimesh)), _lib.ptr(faces)), fn)
    return (list(torch.split(verts, nv)), list(torch.split(faces, [(2 if is_trimesh else 1) * n for n in nq])))


def _mcube_forward(fn, voxelgrids, iso_value, border):
    """The four steps of csrc/mcube.hip on voxelgrids (B, X, Y, Z), B >= 1 and X, Y, Z >= 1 -> (verts (sum V_b, 3) float32,
    faces (sum F_b, 3) int64, [V_b], [F_b], the grid as the kernels read it, the workspace).  The last two are what the backward
    needs: the case bytes and every cell's first vertex id live in the workspace."""
    v = voxelgrids.detach()
    sfx = _CUBIC_SUFFIX.get(v.dtype)
    if sfx is None:
        v = v.float()
        sfx = 'f32'
    B, X, Y, Z = v.shape
    dev = v.device
    lattice = (X + 1) * (Y + 1) * (Z + 1) if border else X * Y * Z
    torch_check(3 * lattice < 2 ** 31, f'{fn}: a lattice of {lattice} points holds up to {3 * lattice} vertices: '
                                       f'more than 32-bit indices cover')
    iso_value = float(iso_value)
    torch_check(iso_value == iso_value, f'{fn}: iso_value must not be NaN')
    lib = _lib.load()
    sp = _lib.stream_ptr(dev)
    border = 1 if border else 0
    with _lib.on_device(dev):
        nbytes = lib.kamd_mcube_workspace(B, X, Y, Z, border)
        torch_check(nbytes > 0, f'{fn}: a batch of {B} grids of {X} x {Y} x {Z} is beyond the launch range')
        ws = _lib.workspace(nbytes, dev)
        grid = (sp, B, X, Y, Z, border, _lib.ptr(v), *v.stride(), iso_value, _lib.ptr(ws))
        _lib.check(getattr(lib, f'kamd_mcube_classify_{sfx}')(*grid), fn)
        host = (ctypes.c_uint32 * (2 * B))()
        _lib.check(lib.kamd_mcube_scan(sp, B, X, Y, Z, border, _lib.ptr(ws), ctypes.cast(host, ctypes.c_void_p)), fn)
        totals = list(host)                                    # data-dependent sizes: the one host read
        nv, nf = totals[0::2], totals[1::2]
        verts = torch.empty((sum(nv), 3), dtype=torch.float32, device=dev)
        faces = torch.empty((sum(nf), 3), dtype=torch.long, device=dev)
        if verts.numel() > 0:
            _lib.check(getattr(lib, f'kamd_mcube_emit_vertices_{sfx}')(*grid, _lib.ptr(verts), verts.shape[0]), fn)
        if faces.numel() > 0:
            _lib.check(lib.kamd_mcube_emit_faces(sp, B, X, Y, Z, border, _lib.ptr(ws), _lib.ptr(faces), faces.shape[0]), fn)
    return verts, faces, nv, nf, v, ws


def _mcube_check(fn, voxelgrids):
    torch_check(isinstance(voxelgrids, torch.Tensor) and voxelgrids.is_cuda, f'{fn}: voxelgrids must be a CUDA tensor')
    torch_check(voxelgrids.dim() == 4, f'{fn}: voxelgrids must of size {{batch_size, X, Y, Z}}')
    torch_check(voxelgrids.shape[0] == 0 or min(voxelgrids.shape[1:]) >= 1, f'{fn}: X, Y and Z must be at least 1')


def voxelgrids_to_trianglemeshes_cuda(voxelgrids, iso_value=0.5):
    """kaolin.ops.conversions.voxelgrids_to_trianglemeshes on the HIP pipeline of csrc/mcube.hip, batched (the reference's
    operator is ``unbatched_mcube_forward_cuda`` below, once per item, on a padded float copy).  voxelgrids (B, X, Y, Z), any
    strides; bool / uint8 / half / float are read in place, any other dtype is cast once with ``.float()``; the border of zeros
    is implicit -> (verts, faces): two lists of B tensors, verts[b] (V_b, 3) float32 and faces[b] (F_b, 3) int64, views of one
    vertex buffer and one face buffer for the batch.  Result sizes depend on the data: the host reads the B x 2 totals once, so
    the call synchronises the current stream and cannot be captured in a graph."""
    fn = 'voxelgrids_to_trianglemeshes_cuda'
    _mcube_check(fn, voxelgrids)
    if voxelgrids.shape[0] == 0:
        return [], []
    verts, faces, nv, nf = _mcube_forward(fn, voxelgrids, iso_value, True)[:4]
    return list(torch.split(verts, nv)), list(torch.split(faces, nf))


def mcube_forward_cuda(voxelgrids, iso_value):
    """The forward of the differentiable operator: voxelgrids (B, X, Y, Z) half or float, B >= 1 -> (the vertex buffer, the
    face buffer, [V_b], [F_b], state); ``state`` is the pipeline's workspace, for ``mcube_backward_cuda`` with the same grid."""
    fn = 'mcube_forward_cuda'
    _mcube_check(fn, voxelgrids)
    torch_check(voxelgrids.dtype in (torch.float16, torch.float32) and voxelgrids.shape[0] > 0,
                f'{fn}: voxelgrids must be a non-empty batch of half or float')
    verts, faces, nv, nf, _, ws = _mcube_forward(fn, voxelgrids, iso_value, True)
    return verts, faces, nv, nf, ws


def mcube_backward_cuda(grad_verts, voxelgrids, iso_value, state):
    """grad_verts (sum V_b, 3), the grid and the state of ``mcube_forward_cuda`` -> the gradient of the grid, contiguous, in its
    dtype: one launch, one thread per grid value gathering over its six lattice edges in a fixed order (float32), no atomics."""
    fn = 'mcube_backward_cuda'
    _mcube_check(fn, voxelgrids)
    sfx = {torch.float16: 'f16', torch.float32: 'f32'}.get(voxelgrids.dtype)
    torch_check(sfx is not None and voxelgrids.shape[0] > 0, f'{fn}: voxelgrids must be a non-empty batch of half or float')
    v = voxelgrids.detach()
    B, X, Y, Z = v.shape
    dev = v.device
    lib = _lib.load()
    torch_check(isinstance(state, torch.Tensor) and state.device == dev and state.dtype == torch.int64 and state.is_contiguous()
                and state.numel() * 8 >= lib.kamd_mcube_workspace(B, X, Y, Z, 1) > 0,
                f'{fn}: state is not the workspace of this grid')
    torch_check(grad_verts.device == dev and grad_verts.dim() == 2 and grad_verts.shape[1] == 3,
                f'{fn}: grad_verts must be of size {{num_vertices, 3}} on the device of voxelgrids')
    g = grad_verts.detach().float().contiguous()
    with _lib.on_device(dev):
        grad = torch.empty((B, X, Y, Z), dtype=v.dtype, device=dev)
        _lib.check(getattr(lib, f'kamd_mcube_backward_{sfx}')(_lib.stream_ptr(dev), B, X, Y, Z, _lib.ptr(v), *v.stride(),
                                                              float(iso_value), _lib.ptr(state), _lib.ptr(g), g.shape[0],
                                                              _lib.ptr(grad)), fn)
    return grad


def unbatched_mcube_forward_cuda(voxelgrid, iso_value):
    """The reference's operator, by its name: one (X, Y, Z) float grid AS GIVEN -- no implicit border: the cells between the given
    points, coordinates equal to the index -> (vertices (V, 3) float32, faces (F, 3) int64), in this package's vertex and
    triangle order (see ops.conversions.voxelgrids_to_trianglemeshes).  The reference's Python layer pads the grid and calls this
    per item; bound to this ``_C`` it gives the meshes of our public function.  Unlike the reference's kernel there is no cap on
    the vertices, a grid that is not a cube is indexed correctly, and the last layer of points starts no cells."""
    fn = 'unbatched_mcube_forward_cuda'
    torch_check(isinstance(voxelgrid, torch.Tensor) and voxelgrid.is_cuda, f'{fn}: voxelgrid must be a CUDA tensor')
    torch_check(voxelgrid.dim() == 3, f'{fn}: voxelgrid must of size {{X, Y, Z}}')
    torch_check(voxelgrid.dtype == torch.float32, f'{fn}: voxelgrid must be a float tensor')
    if min(voxelgrid.shape) < 2:                               # no cell between the points
        return (torch.zeros((0, 3), dtype=torch.float32, device=voxelgrid.device),
                torch.zeros((0, 3), dtype=torch.long, device=voxelgrid.device))
    verts, faces = _mcube_forward(fn, voxelgrid.unsqueeze(0), iso_value, False)[:2]
    return verts, faces


def _flexicubes_args(fn, vertices, scalar_field, cube_idx, beta, alpha, gamma_f):
    """Checks before any launch -> the tensors as the kernels read them (cube_idx keeps its strides)."""
    torch_check(isinstance(vertices, torch.Tensor) and vertices.is_cuda, f'{fn}: voxelgrid_vertices must be a CUDA tensor')
    dev = vertices.device
    torch_check(vertices.dim() == 2 and vertices.shape[1] == 3 and vertices.dtype == torch.float32,
                f'{fn}: voxelgrid_vertices must be a float tensor of size {{num_vertices, 3}}')
    V = vertices.shape[0]
    torch_check(scalar_field.shape == (V,) and scalar_field.dtype == torch.float32 and scalar_field.device == dev,
                f'{fn}: scalar_field must be a float tensor of size {{num_vertices}} on the device of voxelgrid_vertices')
    torch_check(cube_idx.dim() == 2 and cube_idx.shape[1] == 8 and cube_idx.dtype == torch.int64 and cube_idx.device == dev,
                f'{fn}: cube_idx must be a long tensor of size {{num_cubes, 8}} on the device of voxelgrid_vertices')
    C = cube_idx.shape[0]
    torch_check(0 < V < 2 ** 31 and 0 < 12 * C < 2 ** 31, f'{fn}: {V} vertices and {C} cubes are beyond the 32-bit ranks')
    weights = []
    for name, w, shape in (('beta', beta, (C, 12)), ('alpha', alpha, (C, 8)), ('gamma_f', gamma_f, (C,))):
        torch_check(w is None or (w.shape == shape and w.dtype == torch.float32 and w.device == dev),
                    f'{fn}: {name} must be a float tensor of size {shape} on the device of voxelgrid_vertices')
        weights.append(None if w is None else w.detach().contiguous())
    return vertices.detach().contiguous(), scalar_field.detach().contiguous(), cube_idx.detach(), weights


def flexicubes_forward_cuda(vertices, scalar_field, cube_idx, resolution, weight_scale, beta=None, alpha=None, gamma_f=None,
                            training=False):
    """FlexiCubes on the HIP pipeline of csrc/flexicubes.hip (ours: the reference is pure PyTorch).  vertices (V, 3) and
    scalar_field (V,) float32, cube_idx (C, 8) int64 of any strides with C = rx ry rz, raw weights beta (C, 12), alpha (C, 8),
    gamma_f (C,) or None -> (vertices (N [+ Q], 3) float32, faces (F, 3) int64, L_dev (I,) float32, state); ``state`` is the
    integer state ``flexicubes_backward_cuda`` needs.  An entry of cube_idx outside [0, V) raises ``IndexError`` (a flag the
    classify kernel sets; nothing is read through such an id).  Two host reads (the sizes with the flag; the number of quads):
    the call synchronises the current stream and cannot be captured in a graph."""
    fn = 'flexicubes_forward_cuda'
    x, s, cubes, (beta, alpha, gamma_f) = _flexicubes_args(fn, vertices, scalar_field, cube_idx, beta, alpha, gamma_f)
    rx, ry, rz = (int(r) for r in resolution)
    V, C = x.shape[0], cubes.shape[0]
    torch_check(min(rx, ry, rz) >= 1 and rx * ry * rz == C, f'{fn}: cube_idx holds {C} cubes, not {rx} x {ry} x {rz}')
    weight_scale, training = float(weight_scale), bool(training)
    dev = x.device
    lib = _lib.load()
    sp = _lib.stream_ptr(dev)
    grid = (_lib.ptr(s), _lib.ptr(cubes), *cubes.stride())
    with _lib.on_device(dev):
        ws = _lib.workspace(lib.kamd_flexicubes_workspace(C), dev)
        host = (ctypes.c_uint32 * 9)()
        _lib.check(lib.kamd_flexicubes_classify(sp, V, C, rx, ry, rz, *grid, _lib.ptr(ws), ctypes.cast(host, ctypes.c_void_p)), fn)
        totals = list(host)                                    # host read 1: data-dependent sizes and the index-error flag
        if totals[8]:
            raise IndexError(f'{fn}: cube_idx holds an index outside [0, num_vertices = {V})')
        S = sum(totals[0:4])
        num_vd = sum((k + 1) * totals[k] for k in range(4))
        num_inc = sum(totals[4:8])
        if S == 0:
            return (torch.zeros((0, 3), dtype=torch.float32, device=dev), torch.zeros((0, 3), dtype=torch.long, device=dev),
                    torch.zeros((0,), dtype=torch.float32, device=dev), [])
        surf = torch.empty((S, 4), dtype=torch.int32, device=dev)
        ews = _lib.workspace(lib.kamd_flexicubes_edges_workspace(S), dev)
        nq = ctypes.c_int64(0)
        _lib.check(lib.kamd_flexicubes_edges(sp, V, C, S, *grid, _lib.ptr(ws), _lib.ptr(surf), _lib.ptr(ews),
                                             ctypes.cast(ctypes.byref(nq), ctypes.c_void_p)), fn)
        Q = int(nq.value)                                      # host read 2
        verts = torch.empty((num_vd + (Q if training else 0), 3), dtype=torch.float32, device=dev)
        faces = torch.empty((Q * (4 if training else 2), 3), dtype=torch.long, device=dev)
        l_dev = torch.empty((num_inc,), dtype=torch.float32, device=dev)
        vd_gamma = torch.empty((num_vd,), dtype=torch.float32, device=dev)
        quads = torch.empty((Q, 4), dtype=torch.int32, device=dev)
        quad_of = torch.empty((12 * S,), dtype=torch.int32, device=dev)
        if Q > 0:
            _lib.check(lib.kamd_flexicubes_faces(sp, C, S, num_vd, Q, _lib.ptr(gamma_f), weight_scale, int(training), _lib.ptr(surf),
                                                 _lib.ptr(ews), _lib.ptr(quads), _lib.ptr(quad_of), _lib.ptr(faces), faces.shape[0]),
                       fn)
        _lib.check(lib.kamd_flexicubes_forward(sp, V, C, S, num_vd, num_inc, _lib.ptr(x), *grid, _lib.ptr(beta), _lib.ptr(alpha),
                                               _lib.ptr(gamma_f), weight_scale, _lib.ptr(surf), _lib.ptr(verts), _lib.ptr(vd_gamma),
                                               _lib.ptr(l_dev)), fn)
        if training and Q > 0:
            _lib.check(lib.kamd_flexicubes_centers(sp, num_vd, Q, _lib.ptr(quads), _lib.ptr(vd_gamma), _lib.ptr(verts)), fn)
    return verts, faces, l_dev, [surf, quads, quad_of, vd_gamma]


def flexicubes_backward_cuda(grad_vertices, grad_l_dev, vertices, scalar_field, cube_idx, weight_scale, beta, alpha, gamma_f, training,
                             out_vertices, state):
    """The cotangents of the two float results of ``flexicubes_forward_cuda``, its inputs, its vertices and its state -> the
    gradients of (vertices, scalar_field, beta, alpha, gamma_f), None for a weight that is None (and for gamma_f without training:
    it only picks the split).  One launch, one thread per surface cube, recomputing from the inputs; the rows of the weights are
    written by their owner, the shared grid vertices and sdf values take float atomic adds."""
    fn = 'flexicubes_backward_cuda'
    x, s, cubes, (beta, alpha, gamma_f) = _flexicubes_args(fn, vertices, scalar_field, cube_idx, beta, alpha, gamma_f)
    dev = x.device
    V, C = x.shape[0], cubes.shape[0]
    training = bool(training)
    gx, gs = torch.zeros_like(x), torch.zeros_like(s)
    gb = None if beta is None else torch.zeros_like(beta)
    ga = None if alpha is None else torch.zeros_like(alpha)
    gg = None if gamma_f is None or not training else torch.zeros_like(gamma_f)
    if len(state) == 0:                                        # an empty surface
        return gx, gs, gb, ga, gg
    surf, quads, quad_of, vd_gamma = state
    S, Q, num_vd = surf.shape[0], quads.shape[0], vd_gamma.shape[0]
    torch_check(surf.shape == (S, 4) and quads.shape == (Q, 4) and quad_of.shape == (12 * S,) and
                all(t.dtype == torch.int32 and t.device == dev and t.is_contiguous() for t in (surf, quads, quad_of)) and
                vd_gamma.dtype == torch.float32 and vd_gamma.device == dev, f'{fn}: state is not the state of a forward call')
    out = out_vertices.detach()
    torch_check(out.shape == (num_vd + (Q if training else 0), 3) and out.dtype == torch.float32 and out.device == dev
                and out.is_contiguous(), f'{fn}: out_vertices are not the vertices of that forward call')
    torch_check(grad_vertices.shape == out.shape and grad_vertices.device == dev and grad_l_dev.dim() == 1
                and grad_l_dev.device == dev, f'{fn}: the cotangents must have the shapes of vertices and L_dev')
    gv = grad_vertices.detach().float().contiguous()
    gl = grad_l_dev.detach().float().contiguous()
    lib = _lib.load()
    with _lib.on_device(dev):
        _lib.check(lib.kamd_flexicubes_backward(_lib.stream_ptr(dev), V, C, S, num_vd, gl.shape[0], Q, _lib.ptr(x), _lib.ptr(s),
                                                _lib.ptr(cubes), *cubes.stride(), _lib.ptr(beta), _lib.ptr(alpha), _lib.ptr(gamma_f),
                                                float(weight_scale), int(training), _lib.ptr(surf), _lib.ptr(quads),
                                                _lib.ptr(quad_of), _lib.ptr(out), _lib.ptr(vd_gamma), _lib.ptr(gv), _lib.ptr(gl),
                                                _lib.ptr(gx), _lib.ptr(gs), _lib.ptr(gb), _lib.ptr(ga), _lib.ptr(gg)), fn)
    return gx, gs, gb, ga, gg


def check_tets_in_range(tets, num_vertices, fn='marching_tetrahedra'):
    """tets (T, 4) of an integer dtype on any device: raises IndexError when an entry lies outside [0, num_vertices).  Pure
    torch (one min / max pass and one host read); called before any kernel sees the ids -- an id out of range would make the
    HIP path read outside its buffers."""
    torch_check(tets.dim() == 2 and tets.size(1) == 4, f'{fn}: tets must of size {{num_tetrahedrons, 4}}')
    torch_check(not tets.dtype.is_floating_point and not tets.dtype.is_complex, f'{fn}: tets must be of an integer type')
    if tets.numel() == 0:
        return
    lo, hi = torch.stack(torch.aminmax(tets)).tolist()
    if lo < 0 or hi >= num_vertices:
        raise IndexError(f'{fn}: tets hold the index {lo if lo < 0 else hi}, outside [0, num_vertices = {num_vertices})')


def _marching_tetrahedra_args(fn, tensors):
    dev = tensors[0][1].device
    for name, t in tensors:
        torch_check(t.is_cuda, f'{fn}: {name} must be a CUDA tensor')
        torch_check(t.device == dev, f'{fn}: {name} must be on the same device as {tensors[0][0]}')
    return dev


def marching_tetrahedra_cuda(vertices, tets, sdf, return_tet_idx=False):
    """One item of kaolin.ops.conversions.marching_tetrahedra on the HIP pipeline of csrc/marching_tetrahedra.hip (the reference
    has no ``_C`` operator here: its tetmesh.py is a chain of torch kernels).  vertices (V, 3) and sdf (V) float32 or float64,
    tets (T, 4) int64 -> verts (Nv, 3), faces (F, 3) int64, edges (Nv, 2) int64 [, tet_idx (F) int64]: vertex i lies on the edge
    ``edges[i] = (a, b)``, a < b -- what marching_tetrahedra_backward_cuda needs.  Result sizes depend on the data: the host
    reads the number of surface tets and then the number of vertices, so the call synchronises the current stream twice and
    cannot be captured in a graph (like the reference, whose torch.unique and mask indexing synchronise)."""
    fn = 'marching_tetrahedra_cuda'
    dev = _marching_tetrahedra_args(fn, (('vertices', vertices), ('tets', tets), ('sdf', sdf)))
    torch_check(vertices.dim() == 2 and vertices.size(1) == 3, f'{fn}: vertices must of size {{num_vertices, 3}}')
    torch_check(sdf.dim() == 1 and sdf.size(0) == vertices.size(0), f'{fn}: sdf must of size {{num_vertices}}')
    torch_check(tets.dtype == torch.long, f'{fn}: tets must be long')
    torch_check(sdf.dtype == vertices.dtype, f'{fn}: expected vertices and sdf to have the same scalar type')
    sfx = _lib.dtype_suffix(vertices.dtype, fn)
    V, T = vertices.size(0), tets.size(0) if tets.dim() == 2 else 0
    torch_check(V < 2 ** 32, f'{fn}: more than 2^32 - 1 vertices')
    check_tets_in_range(tets, V, fn)
    v, s, t = vertices.detach().contiguous(), sdf.detach().contiguous(), tets.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()                                          # the kernels read a tet as two 16-byte words
    lib = _lib.load()
    sp = _lib.stream_ptr(dev)
    n_one = n_two = nu = 0
    with _lib.on_device(dev):
        if T > 0 and V > 0:
            ws = _lib.workspace(lib.kamd_marching_tetrahedra_workspace(T, V), dev)
            counts = (ctypes.c_int64 * 2)()
            _lib.check(getattr(lib, f'kamd_marching_tetrahedra_classify_{sfx}')(
                sp, T, V, _lib.ptr(t), _lib.ptr(s), _lib.ptr(ws), ctypes.cast(counts, ctypes.c_void_p)), fn)
            n_one, n_two = counts[0], counts[1]                # data-dependent sizes: the first host read
        if n_one + n_two > 0:
            ews = _lib.workspace(lib.kamd_marching_tetrahedra_edges_workspace(n_one, n_two), dev)
            unique = ctypes.c_int64(0)
            _lib.check(lib.kamd_marching_tetrahedra_edges(sp, T, V, _lib.ptr(t), _lib.ptr(ws), n_one, n_two, _lib.ptr(ews),
                                                          ctypes.cast(ctypes.pointer(unique), ctypes.c_void_p)), fn)
            nu = unique.value                                  # ... and the second
        nf = n_one + 2 * n_two
        verts = torch.empty((nu, 3), dtype=v.dtype, device=dev)
        edges = torch.empty((nu, 2), dtype=torch.long, device=dev)
        faces = torch.empty((nf, 3), dtype=torch.long, device=dev)
        tet_idx = torch.empty(nf, dtype=torch.long, device=dev) if return_tet_idx else None
        if nf > 0:
            _lib.check(getattr(lib, f'kamd_marching_tetrahedra_emit_{sfx}')(
                sp, V, _lib.ptr(t), _lib.ptr(v), _lib.ptr(s), _lib.ptr(ews), n_one, n_two, nu, _lib.ptr(verts), _lib.ptr(edges),
                _lib.ptr(faces), _lib.ptr(tet_idx)), fn)
    return (verts, faces, edges, tet_idx) if return_tet_idx else (verts, faces, edges)


def marching_tetrahedra_backward_cuda(grad_verts, vertices, sdf, edges):
    """grad_verts (Nv, 3), vertices (V, 3), sdf (V), edges (Nv, 2) of marching_tetrahedra_cuda -> grad_vertices (V, 3), grad_sdf (V):
    one thread per output vertex, atomic adds into the two zeroed results."""
    fn = 'marching_tetrahedra_backward_cuda'
    dev = _marching_tetrahedra_args(fn, (('grad_verts', grad_verts), ('vertices', vertices), ('sdf', sdf), ('edges', edges)))
    nu, V = edges.size(0), vertices.size(0)
    torch_check(vertices.dim() == 2 and vertices.size(1) == 3, f'{fn}: vertices must of size {{num_vertices, 3}}')
    torch_check(tuple(sdf.shape) == (V,), f'{fn}: sdf must of size {{num_vertices}}')
    torch_check(tuple(edges.shape) == (nu, 2) and edges.dtype == torch.long, f'{fn}: edges must be long, of size {{num_edges, 2}}')
    torch_check(tuple(grad_verts.shape) == (nu, 3), f'{fn}: grad_verts must of size {{num_edges, 3}}')
    torch_check(sdf.dtype == vertices.dtype and grad_verts.dtype == vertices.dtype,
                f'{fn}: expected grad_verts, vertices and sdf to have the same scalar type')
    sfx = _lib.dtype_suffix(vertices.dtype, fn)
    torch_check(V < 2 ** 32, f'{fn}: more than 2^32 - 1 vertices')
    g, v, s, e = grad_verts.contiguous(), vertices.detach().contiguous(), sdf.detach().contiguous(), edges.contiguous()
    lib = _lib.load()
    with _lib.on_device(dev):
        grad_vertices = torch.zeros((V, 3), dtype=v.dtype, device=dev)
        grad_sdf = torch.zeros(V, dtype=v.dtype, device=dev)
        if nu > 0 and V > 0:
            _lib.check(getattr(lib, f'kamd_marching_tetrahedra_backward_{sfx}')(
                _lib.stream_ptr(dev), nu, V, _lib.ptr(e), _lib.ptr(v), _lib.ptr(s), _lib.ptr(g), _lib.ptr(grad_vertices),
                _lib.ptr(grad_sdf)), fn)
    return grad_vertices, grad_sdf


def subdivide_tetmesh_cuda(tets, num_vertices):
    """The topology of kaolin.ops.mesh.subdivide_tetmesh on the HIP pipeline of csrc/subdivide_tetmesh.hip (the reference has no
    ``_C`` operator here: its tetmesh.py is torch.unique(dim=0) and a chain of gathers).  tets (T, 4) int64, ids in
    [0, num_vertices) -> edges (E, 2) int64: the unique (min, max) edges in ascending order, edge e being the new vertex
    ``num_vertices + e``; new_tets (8 T, 4) int64.  The host reads E back: the call synchronises the current stream once and cannot
    be captured in a graph (like the reference, whose torch.unique synchronises)."""
    fn = 'subdivide_tetmesh_cuda'
    V = int(num_vertices)
    check_tets_in_range(tets, V, fn)
    torch_check(tets.is_cuda, f'{fn}: tets must be a CUDA tensor')
    torch_check(tets.dtype == torch.long, f'{fn}: tets must be long')
    torch_check(0 <= V < 2 ** 32, f'{fn}: more than 2^32 - 1 vertices')
    dev, T = tets.device, tets.size(0)
    t = tets.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()                                          # the kernels read a tet as two 16-byte words
    lib = _lib.load()
    sp = _lib.stream_ptr(dev)
    with _lib.on_device(dev):
        num_edges = 0
        if T > 0:
            ws = _lib.workspace(lib.kamd_subdivide_tetmesh_workspace(T, V), dev)
            count = ctypes.c_int64(0)
            _lib.check(lib.kamd_subdivide_tetmesh_edges(sp, T, V, _lib.ptr(t), _lib.ptr(ws),
                                                        ctypes.cast(ctypes.pointer(count), ctypes.c_void_p)), fn)
            num_edges = count.value                            # data-dependent size: the one host read
        edges = torch.empty((num_edges, 2), dtype=torch.long, device=dev)
        new_tets = torch.empty((8 * T, 4), dtype=torch.long, device=dev)
        if T > 0:
            _lib.check(lib.kamd_subdivide_tetmesh_emit(sp, T, V, _lib.ptr(t), _lib.ptr(ws), num_edges, _lib.ptr(edges),
                                                       _lib.ptr(new_tets)), fn)
    return edges, new_tets


def _tetmesh_midpoints_args(fn, named, edges, num_vertices, check_edges):
    """named: ((name, tensor or None, channels or None), ...) of (B, rows, channels) tensors of one dtype on edges' device.
    check_edges: raise IndexError when an entry of edges lies outside [0, num_vertices) -- the kernels gather by them unchecked
    (one torch min / max pass and a host read; the autograd function skips it for the edges the topology stage has just made)."""
    torch_check(edges.is_cuda, f'{fn}: edges must be a CUDA tensor')
    torch_check(edges.dim() == 2 and edges.size(1) == 2 and edges.dtype == torch.long, f'{fn}: edges must be long, of size {{num_edges, 2}}')
    torch_check(edges.is_contiguous(), f'{fn}: edges must be contiguous')
    if check_edges and edges.numel() > 0:
        lo, hi = torch.stack(torch.aminmax(edges)).tolist()
        if lo < 0 or hi >= num_vertices:
            raise IndexError(f'{fn}: edges hold the index {lo if lo < 0 else hi}, outside [0, num_vertices = {num_vertices})')
    first = next(t for _, t, _ in named if t is not None)
    for name, t, channels in named:
        if t is None:
            continue
        torch_check(t.is_cuda and t.device == edges.device, f'{fn}: {name} must be a CUDA tensor on the device of edges')
        torch_check(t.dim() == 3 and (channels is None or t.size(2) == channels), f'{fn}: {name} must of size {{batch_size, num_rows, {channels or "feature_dim"}}}')
        torch_check(t.dtype == first.dtype, f'{fn}: expected every tensor to have the same scalar type')
        torch_check(t.shape[:2] == first.shape[:2], f'{fn}: {name} must have the batch size and the rows of the other tensor')
    return _lib.dtype_suffix(first.dtype, fn), first


def _batch_items(t):
    """(tensor, batch stride): items contiguous, the batch stride free (0 for an expanded batch); anything else is copied"""
    if t.size(0) == 0 or t[0].is_contiguous():
        return t, (t.stride(0) if t.size(0) > 1 else 0)
    t = t.contiguous()
    return t, t.stride(0)


def tetmesh_midpoints_forward_cuda(vertices, features, edges, check_edges=True):
    """vertices (B, V, 3), features (B, V, D) or None, edges (E, 2) of subdivide_tetmesh_cuda -> new_vertices (B, V + E, 3),
    new_features (B, V + E, D) or None: rows [0, V) are the inputs, row V + e is ``(x[min] + x[max]) * 0.5``; one launch writes
    both results.  float32 / float64.  ``check_edges``: IndexError for an entry of edges outside [0, V) (skipped by the autograd
    function, whose edges come straight from subdivide_tetmesh_cuda)."""
    fn = 'tetmesh_midpoints_forward_cuda'
    sfx, _ = _tetmesh_midpoints_args(fn, (('vertices', vertices, 3), ('features', features, None)), edges, vertices.size(1),
                                     check_edges)
    B, V, E = vertices.size(0), vertices.size(1), edges.size(0)
    D = features.size(2) if features is not None else 0
    torch_check(V < 2 ** 32, f'{fn}: more than 2^32 - 1 vertices')
    dev = vertices.device
    v, vbs = _batch_items(vertices.detach())
    f, fbs = _batch_items(features.detach()) if features is not None and D > 0 else (None, 0)
    lib = _lib.load()
    with _lib.on_device(dev):
        new_vertices = torch.empty((B, V + E, 3), dtype=v.dtype, device=dev)
        new_features = torch.empty((B, V + E, D), dtype=v.dtype, device=dev) if features is not None else None
        if B > 0 and V + E > 0:
            _lib.check(getattr(lib, f'kamd_tetmesh_midpoints_forward_{sfx}')(
                _lib.stream_ptr(dev), B, V, E, D, _lib.ptr(v), vbs, _lib.ptr(f), fbs, _lib.ptr(edges), _lib.ptr(new_vertices),
                _lib.ptr(new_features if f is not None else None)), fn)
    return new_vertices, new_features


def tetmesh_midpoints_backward_cuda(grad_new_vertices, grad_new_features, edges, num_vertices, check_edges=True):
    """grad_new_vertices (B, V + E, 3) or None, grad_new_features (B, V + E, D) or None (not both), any strides, edges (E, 2)
    -> grad_vertices (B, V, 3) or None, grad_features (B, V, D) or None: ``g[b, v]`` plus half of ``g[b, V + e]`` for every
    unique edge that holds v (a self-edge counts twice).  The edges with min = v are one run of the sorted list, summed in
    order and stored; the halves of the max side are added with native floating-point atomics."""
    fn = 'tetmesh_midpoints_backward_cuda'
    torch_check(grad_new_vertices is not None or grad_new_features is not None, f'{fn}: no gradient given')
    sfx, first = _tetmesh_midpoints_args(fn, (('grad_new_vertices', grad_new_vertices, 3), ('grad_new_features', grad_new_features, None)),
                                         edges, int(num_vertices), check_edges)
    B, V, E = first.size(0), int(num_vertices), edges.size(0)
    torch_check(first.size(1) == V + E, f'{fn}: the gradients must have num_vertices + num_edges rows')
    torch_check(0 <= V < 2 ** 32, f'{fn}: more than 2^32 - 1 vertices')
    dev = first.device
    gv = grad_new_vertices.contiguous() if grad_new_vertices is not None else None
    gf = grad_new_features.contiguous() if grad_new_features is not None else None
    D = gf.size(2) if gf is not None else 0
    lib = _lib.load()
    with _lib.on_device(dev):
        grad_vertices = torch.empty((B, V, 3), dtype=first.dtype, device=dev) if gv is not None else None
        grad_features = torch.empty((B, V, D), dtype=first.dtype, device=dev) if gf is not None else None
        if B > 0 and V > 0:
            _lib.check(getattr(lib, f'kamd_tetmesh_midpoints_backward_{sfx}')(
                _lib.stream_ptr(dev), B, V, E, D, _lib.ptr(gv), _lib.ptr(gf if D > 0 else None), _lib.ptr(edges),
                _lib.ptr(grad_vertices), _lib.ptr(grad_features if D > 0 else None)), fn)
    return grad_vertices, grad_features


def check_faces_in_range(faces, num_vertices, fn='subdivide_trianglemesh'):
    """faces (F, 3) of an integer dtype on any device: raises IndexError when an entry lies outside [0, num_vertices).  Pure
    torch (one min / max pass and one host read); called before any kernel sees the ids -- an id out of range would make the
    HIP path read outside its buffers."""
    torch_check(faces.dim() == 2 and faces.size(1) == 3, f'{fn}: faces must of size {{num_faces, 3}}')
    torch_check(not faces.dtype.is_floating_point and not faces.dtype.is_complex, f'{fn}: faces must be of an integer type')
    if faces.numel() == 0:
        return
    lo, hi = torch.stack(torch.aminmax(faces)).tolist()
    if lo < 0 or hi >= num_vertices:
        raise IndexError(f'{fn}: faces hold the index {lo if lo < 0 else hi}, outside [0, num_vertices = {num_vertices})')


# the topology tensors of one Loop iteration, in the order the C ABI takes them
LOOP_TOPOLOGY = ('edges', 'count', 'opp', 'tlist', 'runs', 'valence')


def subdivide_trianglemesh_cuda(faces, num_vertices, check_faces=True):
    """The topology of one iteration of kaolin.ops.mesh.subdivide_trianglemesh on the HIP pipeline of
    csrc/subdivide_trianglemesh.hip (the reference has no ``_C`` operator here).  faces (F, 3) int64, F > 0, ids in
    [0, num_vertices) -> new_faces (4 F, 3) int64 and the tuple LOOP_TOPOLOGY: edges (E, 2) int64, the unique (min, max) edges in
    ascending order, edge e being the new vertex ``num_vertices + e``; count (E) int32, the face slots per edge; opp (E, 2) int64,
    two opposite corners (meaningful where count == 2); tlist (E, 2) int64, (min end, edge id) in ascending (max, min) order; runs
    (V + 1, 2) int64, the starts of every vertex's runs in edges and tlist; valence (V) int32.  The host reads E back: the call
    synchronises the current stream once and cannot be captured in a graph (like the reference, whose torch.unique synchronises).
    ``check_faces``: IndexError for an entry of faces outside [0, num_vertices) -- the kernels gather by them unchecked (skipped
    by the public function, which has checked the first iteration's faces and makes the later ones itself)."""
    fn = 'subdivide_trianglemesh_cuda'
    V = int(num_vertices)
    if check_faces:
        check_faces_in_range(faces, V, fn)
    torch_check(faces.dim() == 2 and faces.size(1) == 3, f'{fn}: faces must of size {{num_faces, 3}}')
    torch_check(faces.is_cuda, f'{fn}: faces must be a CUDA tensor')
    torch_check(faces.dtype == torch.long, f'{fn}: faces must be long')
    torch_check(0 < V < 2 ** 32, f'{fn}: the number of vertices must be in [1, 2^32)')
    dev, F = faces.device, faces.size(0)
    torch_check(F > 0, f'{fn}: no faces')
    f = faces.contiguous()
    lib = _lib.load()
    sp = _lib.stream_ptr(dev)
    with _lib.on_device(dev):
        ws = _lib.workspace(lib.kamd_subdivide_trianglemesh_workspace(F, V), dev)
        torch_check(ws is not None, f'{fn}: {F} faces are more than the pipeline takes')
        count = ctypes.c_int64(0)
        _lib.check(lib.kamd_subdivide_trianglemesh_edges(sp, F, V, _lib.ptr(f), _lib.ptr(ws),
                                                         ctypes.cast(ctypes.pointer(count), ctypes.c_void_p)), fn)
        E = count.value                                        # data-dependent size: the one host read
        new_faces = torch.empty((4 * F, 3), dtype=torch.long, device=dev)
        topo = (torch.empty((E, 2), dtype=torch.long, device=dev), torch.empty(E, dtype=torch.int32, device=dev),
                torch.empty((E, 2), dtype=torch.long, device=dev), torch.empty((E, 2), dtype=torch.long, device=dev),
                torch.empty((V + 1, 2), dtype=torch.long, device=dev), torch.empty(V, dtype=torch.int32, device=dev))
        for t in (ws, new_faces) + topo:
            torch_check(t.data_ptr() % 16 == 0, f'{fn}: an allocation is not 16-byte aligned')
        _lib.check(lib.kamd_subdivide_trianglemesh_emit(sp, F, V, _lib.ptr(f), _lib.ptr(ws), E, _lib.ptr(topo[0]), _lib.ptr(new_faces),
                                                        *(_lib.ptr(t) for t in topo[1:])), fn)
    return new_faces, topo


def _loop_args(fn, vertices, alpha, topo, rows):
    """vertices-like (B, rows, 3) and alpha-like (B, rows) or None, of one float32 / float64 dtype, on the device of the topology
    tuple of subdivide_trianglemesh_cuda -> (dtype suffix, V, E)"""
    torch_check(isinstance(topo, (tuple, list)) and len(topo) == len(LOOP_TOPOLOGY), f'{fn}: topo must be the tuple {LOOP_TOPOLOGY}')
    edges, count, opp, tlist, runs, valence = topo
    V, E = valence.size(0), edges.size(0)
    for name, t, shape, dtype in (('edges', edges, (E, 2), torch.long), ('count', count, (E,), torch.int32), ('opp', opp, (E, 2), torch.long),
                                  ('tlist', tlist, (E, 2), torch.long), ('runs', runs, (V + 1, 2), torch.long),
                                  ('valence', valence, (V,), torch.int32)):
        torch_check(t.is_cuda and t.device == edges.device and t.dtype == dtype and tuple(t.shape) == shape and t.is_contiguous(),
                    f'{fn}: {name} must be a contiguous CUDA {dtype} tensor of size {shape}')
        torch_check(t.data_ptr() % 16 == 0, f'{fn}: {name} must be 16-byte aligned')
    torch_check(0 < V < 2 ** 32, f'{fn}: the number of vertices must be in [1, 2^32)')
    torch_check(vertices.is_cuda and vertices.device == edges.device, f'{fn}: expected a CUDA tensor on the device of the topology')
    torch_check(vertices.dim() == 3 and tuple(vertices.shape[1:]) == (rows(V, E), 3), f'{fn}: expected size {{batch_size, {rows(V, E)}, 3}}')
    if alpha is not None:
        torch_check(alpha.is_cuda and alpha.device == edges.device and alpha.dtype == vertices.dtype,
                    f'{fn}: expected every tensor to have the same device and scalar type')
        torch_check(tuple(alpha.shape) == (vertices.size(0), rows(V, E)), f'{fn}: expected size {{batch_size, {rows(V, E)}}}')
    return _lib.dtype_suffix(vertices.dtype, fn), V, E


def trianglemesh_loop_forward_cuda(vertices, alpha, topo):
    """vertices (B, V, 3), alpha (B, V) or None (the Loop weights from the valences), topo of subdivide_trianglemesh_cuda ->
    new_vertices (B, V + E, 3), new_alpha (B, V + E) or None.  One launch, gathers only: two calls give the same bits."""
    fn = 'trianglemesh_loop_forward_cuda'
    sfx, V, E = _loop_args(fn, vertices, alpha, topo, lambda V, E: V)
    B, dev = vertices.size(0), vertices.device
    v, vbs = _batch_items(vertices.detach())
    a, abs_ = _batch_items(alpha.detach()) if alpha is not None else (None, 0)
    lib = _lib.load()
    with _lib.on_device(dev):
        new_vertices = torch.empty((B, V + E, 3), dtype=v.dtype, device=dev)
        new_alpha = torch.empty((B, V + E), dtype=v.dtype, device=dev) if a is not None else None
        if B > 0:
            _lib.check(getattr(lib, f'kamd_trianglemesh_loop_forward_{sfx}')(
                _lib.stream_ptr(dev), B, V, E, _lib.ptr(v), vbs, _lib.ptr(a), abs_, *(_lib.ptr(t) for t in topo),
                _lib.ptr(new_vertices), _lib.ptr(new_alpha)), fn)
    return new_vertices, new_alpha


def trianglemesh_loop_backward_cuda(grad_new_vertices, grad_new_alpha, vertices, alpha, topo, alpha_needs_grad):
    """grad_new_vertices (B, V + E, 3), grad_new_alpha (B, V + E) or None, any strides; vertices, alpha and topo of the forward ->
    grad_vertices (B, V, 3), grad_alpha (B, V) or None (``alpha_needs_grad`` False, or no alpha).  A gather with plain stores, then
    native floating-point atomic adds of the opposite corners' 1/8 terms."""
    fn = 'trianglemesh_loop_backward_cuda'
    sfx, V, E = _loop_args(fn, grad_new_vertices, grad_new_alpha, topo, lambda V, E: V + E)
    _loop_args(fn, vertices, alpha, topo, lambda V, E: V)
    torch_check(vertices.dtype == grad_new_vertices.dtype and vertices.size(0) == grad_new_vertices.size(0),
                f'{fn}: expected every tensor to have the same batch size and scalar type')
    B, dev = vertices.size(0), vertices.device
    gv = grad_new_vertices.contiguous()
    ga = grad_new_alpha.contiguous() if grad_new_alpha is not None else None
    v, vbs = _batch_items(vertices.detach())
    a, abs_ = _batch_items(alpha.detach()) if alpha is not None else (None, 0)
    lib = _lib.load()
    with _lib.on_device(dev):
        grad_vertices = torch.empty((B, V, 3), dtype=v.dtype, device=dev)
        grad_alpha = torch.empty((B, V), dtype=v.dtype, device=dev) if (a is not None and alpha_needs_grad) else None
        if B > 0:
            _lib.check(getattr(lib, f'kamd_trianglemesh_loop_backward_{sfx}')(
                _lib.stream_ptr(dev), B, V, E, _lib.ptr(gv), _lib.ptr(ga), _lib.ptr(v), vbs, _lib.ptr(a), abs_,
                *(_lib.ptr(t) for t in topo), _lib.ptr(grad_vertices), _lib.ptr(grad_alpha)), fn)
    return grad_vertices, grad_alpha


# ---- kaolin._C.ops.spc: the SPC core on csrc/spc.hip ---------------------------------------------------------------------
SPC_MAX_LEVEL = 15      # KAOLIN_SPC_MAX_LEVELS


def _spc_points_arg(fn, points):
    torch_check(points.is_cuda, f'{fn}: points must be a CUDA tensor')
    torch_check(points.dtype == torch.int16, f'{fn}: points must be short')
    torch_check(points.dim() == 2 and points.size(1) == 3, f'{fn}: points must be Nx3')
    torch_check(points.is_contiguous(), f'{fn}: points must be contiguous')


def points_to_morton_cuda(points):
    """reference: point_utils.cpp ``points_to_morton_cuda``: points (N, 3) int16 -> Morton codes (N) int64 (bit 3i = z, 3i + 1 = y,
    3i + 2 = x, the low 15 bits of every coordinate).  One launch, capturable."""
    fn = 'points_to_morton_cuda'
    _spc_points_arg(fn, points)
    lib = _lib.load()
    with _lib.on_device(points.device):
        morton = torch.empty(points.size(0), dtype=torch.long, device=points.device)
        _lib.check(lib.kamd_spc_points_to_morton(_lib.stream_ptr(points.device), points.size(0), _lib.ptr(points), _lib.ptr(morton)), fn)
    return morton


def morton_to_points_cuda(morton):
    """reference: point_utils.cpp ``morton_to_points_cuda``: codes (N) int64 -> points (N, 3) int16.  One launch, capturable."""
    fn = 'morton_to_points_cuda'
    torch_check(morton.is_cuda, f'{fn}: morton must be a CUDA tensor')
    torch_check(morton.dtype == torch.long and morton.dim() == 1, f'{fn}: morton must be long, of size {{num_points}}')
    torch_check(morton.is_contiguous(), f'{fn}: morton must be contiguous')
    lib = _lib.load()
    with _lib.on_device(morton.device):
        points = torch.empty((morton.size(0), 3), dtype=torch.int16, device=morton.device)
        _lib.check(lib.kamd_spc_morton_to_points(_lib.stream_ptr(morton.device), morton.size(0), _lib.ptr(morton), _lib.ptr(points)), fn)
    return points


def points_to_corners_cuda(points):
    """reference: point_utils.cpp ``points_to_corners_cuda``: points (N, 3) int16 -> (N, 8, 3) int16, corner j = point +
    (j >> 2, (j >> 1) & 1, j & 1).  One launch, capturable."""
    fn = 'points_to_corners_cuda'
    _spc_points_arg(fn, points)
    lib = _lib.load()
    with _lib.on_device(points.device):
        corners = torch.empty((points.size(0), 8, 3), dtype=torch.int16, device=points.device)
        _lib.check(lib.kamd_spc_points_to_corners(_lib.stream_ptr(points.device), points.size(0), _lib.ptr(points), _lib.ptr(corners)), fn)
    return corners


def morton_to_octree(mortons, level, sorted=True):
    """reference: spc.cpp ``morton_to_octree``: Morton codes (N) int64 of points of ``level`` -> octree (num_bytes) uint8, levels root
    first.  ``sorted=True`` is the reference's contract (unique codes in ascending order); ``sorted=False`` (ours) takes any order and
    duplicates: the codes go through the keys-only radix sort over their 3 * level significant bits.  Bits above those are
    dropped.  The host reads the level sizes once (the reference: once per level): the call synchronises the current stream and
    cannot be captured in a graph."""
    fn = 'morton_to_octree'
    torch_check(mortons.is_cuda, f'{fn}: mortons must be a CUDA tensor')
    torch_check(mortons.dtype == torch.long and mortons.dim() == 1, f'{fn}: mortons must be long, of size {{num_points}}')
    torch_check(mortons.is_contiguous(), f'{fn}: mortons must be contiguous')
    level, n, dev = int(level), mortons.size(0), mortons.device
    torch_check(0 <= level <= SPC_MAX_LEVEL, f'{fn}: level must be in [0, {SPC_MAX_LEVEL}]')
    torch_check(n > 0, f'{fn}: no points')
    if level == 0:
        return torch.empty(0, dtype=torch.uint8, device=dev)
    lib = _lib.load()
    sp = _lib.stream_ptr(dev)
    with _lib.on_device(dev):
        nbytes = lib.kamd_spc_octree_workspace(n, level)
        ws = _lib.workspace(nbytes, dev)
        sizes = (ctypes.c_int64 * (1 + level))()
        _lib.check(lib.kamd_spc_octree_build(sp, n, level, _lib.ptr(mortons), int(bool(sorted)), _lib.ptr(ws), nbytes,
                                             ctypes.cast(sizes, ctypes.c_void_p)), fn)
        octree_bytes = sum(sizes[1:])                          # data-dependent size: the one host read
        octree = torch.empty(octree_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.kamd_spc_octree_gather(sp, n, level, _lib.ptr(ws), octree_bytes, _lib.ptr(octree)), fn)
    return octree


def points_to_octree(points, level, sorted=True):
    """reference: spc.cpp ``points_to_octree``: points (N, 3) int16 of ``level`` -> octree; see morton_to_octree."""
    _spc_points_arg('points_to_octree', points)
    torch_check(points.size(0) > 0, 'points_to_octree: no points')
    return morton_to_octree(points_to_morton_cuda(points), level, sorted=sorted)


def scan_octrees_cuda(octrees, lengths):
    """reference: spc.cpp:79-107 ``scan_octrees_cuda``: octrees (num_bytes) uint8 CUDA, lengths (B) int32 CPU -> (max_level,
    pyramids (B, 2, max_level + 2) int32 CPU, exsum (num_bytes) int32 CUDA: per octree the inclusive sum of the bit counts).
    Four launches and ONE host read for the batch (the reference: one read per level and item).  ValueError when the items differ
    in depth or an item does not account for its bytes exactly."""
    fn = 'scan_octrees_cuda'
    torch_check(octrees.is_cuda, f'{fn}: octrees must be a CUDA tensor')
    torch_check(octrees.dtype == torch.uint8 and octrees.dim() == 1, f'{fn}: octrees must be a 1D byte tensor')
    torch_check(octrees.is_contiguous(), f'{fn}: octrees must be contiguous')
    torch_check(not lengths.is_cuda and lengths.dim() == 1, f'{fn}: lengths must be a 1D CPU tensor')
    lens = [int(v) for v in lengths.tolist()]
    B, total, dev = len(lens), sum(lens), octrees.device
    if B == 0 or min(lens) < 1:
        raise ValueError(f'{fn}: every octree needs at least one byte, got lengths {lens}')
    if total != octrees.numel():
        raise ValueError(f'{fn}: lengths sum to {total}, octrees holds {octrees.numel()} bytes')
    if total * 8 >= 2 ** 31:
        raise ValueError(f'{fn}: {total} bytes: sum(lengths) * 8 must stay below 2^31')
    lib = _lib.load()
    host = (ctypes.c_int32 * (35 * B))()
    with _lib.on_device(dev):
        starts = torch.tensor([0] + lens, dtype=torch.long).cumsum(0).to(dev)
        exsum = torch.empty(total, dtype=torch.int32, device=dev)
        ws = _lib.workspace(lib.kamd_spc_scan_workspace(total, B), dev)
        _lib.check(lib.kamd_spc_scan_octrees(_lib.stream_ptr(dev), total, B, _lib.ptr(octrees), _lib.ptr(starts), _lib.ptr(exsum),
                                             _lib.ptr(ws), ctypes.cast(host, ctypes.c_void_p)), fn)
    full = torch.tensor(list(host), dtype=torch.int32).reshape(B, 35)      # the one host read, for the whole batch
    return finish_scan(fn, full[:, :34].reshape(B, 2, 17), full[:, 34].tolist(), lens) + (exsum,)


def finish_scan(fn, full_pyramids, depths, lens):
    """The checks scan_octrees makes after its read-back: one depth for the batch, every byte accounted for."""
    max_level = depths[0]
    if any(d != max_level for d in depths):
        raise ValueError(f'{fn}: all octrees of a batch must have the same depth, got {depths}')
    used = full_pyramids[:, 0, :max_level].sum(1).tolist()
    if used != lens:
        raise ValueError(f'{fn}: the levels of the octrees account for {used} bytes, lengths says {lens} '
                         '(an octree is truncated, padded or deeper than 15 levels)')
    return max_level, full_pyramids[:, :, :max_level + 2].contiguous()


def _spc_exsum_arg(fn, exsum, num_bytes):
    torch_check(exsum.is_cuda and exsum.dtype == torch.int32 and exsum.dim() == 1, f'{fn}: exsum must be a 1D CUDA int tensor')
    torch_check(exsum.is_contiguous(), f'{fn}: exsum must be contiguous')
    if exsum.numel() != num_bytes:
        raise ValueError(f'{fn}: exsum has {exsum.numel()} entries for {num_bytes} octree bytes; only the current layout '
                         '(num_bytes entries, inclusive sums) is accepted, not the legacy one with a leading 0 per octree')


def spc_generate_meta(pyramids):
    """(meta rows (B, 2 + 2 (max_level + 2)) int64 CPU, num_bytes, num_points, largest level) of a CPU pyramid"""
    p = pyramids.to(torch.long)
    L = p.size(2) - 2
    nbytes, npoints = p[:, 1, L], p[:, 1, L + 1]
    ostart = torch.cumsum(nbytes, 0) - nbytes
    pstart = torch.cumsum(npoints, 0) - npoints
    meta = torch.cat([ostart[:, None], pstart[:, None], p[:, 0, :], p[:, 1, :]], dim=1).contiguous()
    return meta, int(nbytes.sum()), int(npoints.sum()), int(p[:, 0, :].max()) if p.numel() else 0


def generate_points_cuda(octrees, pyramid, exsum):
    """reference: spc.cpp:109-134 ``generate_points_cuda``: octrees (num_bytes) uint8, pyramid (B, 2, max_level + 2) int32 CPU, exsum
    (num_bytes) int32 -> point hierarchies (num_points, 3) int16.  max_level launches for the whole batch, no host read (the
    reference: a launch per level and item, and a host write per item)."""
    fn = 'generate_points_cuda'
    torch_check(octrees.is_cuda, f'{fn}: octrees must be a CUDA tensor')
    torch_check(octrees.dtype == torch.uint8 and octrees.dim() == 1 and octrees.is_contiguous(), f'{fn}: octrees must be a contiguous 1D byte tensor')
    torch_check(not pyramid.is_cuda and pyramid.dim() == 3 and pyramid.size(1) == 2, f'{fn}: pyramid must be a CPU tensor of size {{batch_size, 2, max_level + 2}}')
    _spc_exsum_arg(fn, exsum, octrees.numel())
    B, L, dev = pyramid.size(0), pyramid.size(2) - 2, octrees.device
    torch_check(0 <= L <= SPC_MAX_LEVEL, f'{fn}: max_level must be in [0, {SPC_MAX_LEVEL}]')
    torch_check(B <= 65535, f'{fn}: more than 65535 octrees in a batch')
    meta, nbytes, npoints, widest = spc_generate_meta(pyramid)
    if nbytes != octrees.numel():
        raise ValueError(f'{fn}: the pyramids describe {nbytes} octree bytes, octrees holds {octrees.numel()}')
    lib = _lib.load()
    with _lib.on_device(dev):
        points = torch.zeros((npoints, 3), dtype=torch.int16, device=dev) if L == 0 else \
            torch.empty((npoints, 3), dtype=torch.int16, device=dev)
        if npoints > 0 and L > 0:
            meta = meta.to(dev)
            _lib.check(lib.kamd_spc_generate_points(_lib.stream_ptr(dev), B, L, nbytes, npoints, _lib.ptr(octrees), _lib.ptr(exsum),
                                                    _lib.ptr(meta), widest, _lib.ptr(points)), fn)
    return points


def _spc_query(fn, multiscale, octree, exsum, query_coords, level):
    torch_check(octree.is_cuda and exsum.is_cuda and query_coords.is_cuda, f'{fn}: octree, prefix_sum and query_coords must be CUDA tensors')
    torch_check(octree.device == exsum.device == query_coords.device, f'{fn}: expected every tensor on the same device')
    torch_check(octree.dtype == torch.uint8 and octree.dim() == 1, f'{fn}: octree must be a 1D byte tensor')
    torch_check(octree.is_contiguous() and query_coords.is_contiguous(), f'{fn}: expected contiguous tensors')
    torch_check(query_coords.dim() == 2 and query_coords.size(1) == 3, f'{fn}: query_coords must be Nx3')
    _spc_exsum_arg(fn, exsum, octree.numel())
    sfx = _lib.dtype_suffix(query_coords.dtype, fn, allowed=('f16', 'f32', 'f64'))
    level = int(level)
    torch_check(0 <= level <= SPC_MAX_LEVEL, f'{fn}: level must be in [0, {SPC_MAX_LEVEL}]')
    Q, dev = query_coords.size(0), octree.device
    lib = _lib.load()
    with _lib.on_device(dev):
        if octree.numel() == 0:
            return torch.full((Q, level + 1) if multiscale else (Q,), -1, dtype=torch.long, device=dev)
        pidx = torch.empty((Q, level + 1) if multiscale else (Q,), dtype=torch.long, device=dev)
        _lib.check(getattr(lib, f'kamd_spc_query_{"multiscale_" if multiscale else ""}{sfx}')(
            _lib.stream_ptr(dev), Q, level, octree.numel(), _lib.ptr(octree), _lib.ptr(exsum), _lib.ptr(query_coords), _lib.ptr(pidx)), fn)
    return pidx


def query_cuda(octree, prefix_sum, query_coords, target_level):
    """reference: query.cpp:49-73 ``query_cuda``: octree (num_bytes) uint8, prefix_sum (num_bytes) int32, query_coords (Q, 3) half /
    float / double in [-1, 1], read in place -> point index (Q), -1 for a miss; int64 here (the reference returns int32 and its
    Python layer converts).  One launch, no host read: capturable."""
    return _spc_query('query_cuda', False, octree, prefix_sum, query_coords, target_level)


def query_multiscale_cuda(octree, prefix_sum, query_coords, target_level):
    """reference: query.cpp:75-99 ``query_multiscale_cuda``: as query_cuda -> (Q, target_level + 1): the index of the point and of
    every ancestor, -1 from the first level that misses."""
    return _spc_query('query_multiscale_cuda', True, octree, prefix_sum, query_coords, target_level)


def _spc_to_dense(fn, backward, points, level, pyramid, features, grad_outputs=None):
    torch_check(points.is_cuda and features.is_cuda, f'{fn}: points and features must be CUDA tensors')
    torch_check(not pyramid.is_cuda and pyramid.dim() == 3 and pyramid.size(1) == 2, f'{fn}: pyramid must be a CPU tensor of size {{batch_size, 2, max_level + 2}}')
    torch_check(points.dtype == torch.int16 and points.dim() == 2 and points.size(1) == 3 and points.is_contiguous(),
                f'{fn}: points must be a contiguous short tensor of size {{num_points, 3}}')
    torch_check(features.dim() == 2 and features.is_contiguous(), f'{fn}: features must be a contiguous tensor of size {{num_inputs, feature_dim}}')
    sfx = _lib.dtype_suffix(features.dtype, fn)
    level = int(level)
    B, L = pyramid.size(0), pyramid.size(2) - 2
    torch_check(0 <= level <= L <= SPC_MAX_LEVEL, f'{fn}: level must be in [0, max_level], max_level at most {SPC_MAX_LEVEL}')
    p = pyramid.to(torch.long)
    counts = p[:, 0, level]
    rows, C, E, dev = int(counts.sum()), features.size(1), 1 << level, features.device
    torch_check(features.size(0) == rows, f'{fn}: features has {features.size(0)} rows, level {level} of the batch has {rows} points')
    npoints = p[:, 1, L + 1]
    first = torch.cumsum(npoints, 0) - npoints + p[:, 1, level]
    meta = torch.cat([torch.zeros(1, dtype=torch.long), torch.cumsum(counts, 0), first])
    lib = _lib.load()
    with _lib.on_device(dev):
        if backward:
            torch_check(grad_outputs.is_cuda and grad_outputs.is_contiguous() and grad_outputs.dtype == features.dtype and
                        tuple(grad_outputs.shape) == (B, C, E, E, E), f'{fn}: grad_outputs must be a contiguous CUDA tensor of size {(B, C, E, E, E)}')
            out = torch.empty_like(features)
            src = grad_outputs
        else:
            out = torch.empty((B, C, E, E, E), dtype=features.dtype, device=dev)
            src = features
        if out.numel() > 0:
            meta = meta.to(dev)
            _lib.check(getattr(lib, f'kamd_spc_to_dense_{"backward" if backward else "forward"}_{sfx}')(
                _lib.stream_ptr(dev), B, C, level, rows, points.size(0), _lib.ptr(points), _lib.ptr(meta), _lib.ptr(src), _lib.ptr(out)), fn)
    return out


def to_dense_forward(points, level, pyramid, features):
    """reference: feature_grids.cpp:47-78 ``to_dense_forward``: points = packed point hierarchies (num_points, 3) int16, pyramid CPU,
    features (rows at ``level``, C) float32 / float64 -> (B, C, 2^level, 2^level, 2^level): a zero fill and one thread per (point,
    channel), the whole batch in one launch (the reference: one launch per item, float only)."""
    return _spc_to_dense('to_dense_forward', False, points, level, pyramid, features)


def to_dense_backward(points, level, pyramid, features, grad_outputs):
    """reference: feature_grids.cpp:81-106 ``to_dense_backward``: the matching gather -> grad_features, of the size of features."""
    return _spc_to_dense('to_dense_backward', True, points, level, pyramid, features, grad_outputs)


# ---- kaolin._C.ops.spc: feature grids on csrc/spc_trilinear.hip ------------------------------------------------------------
SPC_DUAL_MAX_LEVEL = 14     # a corner of level l reaches 2^l: int16 and the 15-bit Morton codes hold it up to level 14


def _spc_pyramid_row(fn, pyramid, what, rows):
    """row 1 of a (2, max_level + 2) CPU pyramid as a ctypes int64 array, after checking that it starts at 0, does not decrease,
    agrees with row 0 and ends at `rows`"""
    torch_check(not pyramid.is_cuda and pyramid.dim() == 2 and pyramid.size(0) == 2 and pyramid.size(1) >= 2,
                f'{fn}: {what} must be a CPU tensor of size {{2, max_level + 2}}')
    count, first = pyramid[0].tolist(), pyramid[1].tolist()
    L = len(first) - 2
    if L > SPC_DUAL_MAX_LEVEL:
        raise ValueError(f'{fn}: max_level {L}: the corners of level 15 reach 32768, which neither int16 nor the 15-bit Morton '
                         f'codes hold; dual octrees go up to level {SPC_DUAL_MAX_LEVEL}')
    if first[0] != 0 or first[L + 1] != rows or any(c < 0 or first[l] + c != first[l + 1] for l, c in enumerate(count[:L + 1])):
        raise ValueError(f'{fn}: {what} does not describe the {rows} rows of its hierarchy: {pyramid.tolist()}')
    return L, (ctypes.c_int64 * (L + 2))(*first)


def make_dual_cuda(point_hierarchy, pyramid):
    """ours (the reference builds the dual in Python, level by level): point_hierarchy (num_points, 3) int16 CUDA, pyramid (2,
    max_level + 2) int32 CPU -> (point_hierarchy_dual (num_dual, 3) int16, pyramid_dual like pyramid).  All levels in one sort;
    ONE host read (the level sizes): the call synchronises the current stream and cannot be captured in a graph."""
    fn = 'make_dual_cuda'
    _spc_points_arg(fn, point_hierarchy)
    n, dev = point_hierarchy.size(0), point_hierarchy.device
    L, first = _spc_pyramid_row(fn, pyramid, 'pyramid', n)
    torch_check(n > 0, f'{fn}: no points')
    lib = _lib.load()
    sp = _lib.stream_ptr(dev)
    with _lib.on_device(dev):
        nbytes = lib.kamd_spc_dual_workspace(n, L)
        ws = _lib.workspace(nbytes, dev)
        starts = (ctypes.c_int64 * (L + 2))()
        _lib.check(lib.kamd_spc_dual_build(sp, n, L, _lib.ptr(point_hierarchy), ctypes.cast(first, ctypes.c_void_p), _lib.ptr(ws),
                                           nbytes, ctypes.cast(starts, ctypes.c_void_p)), fn)
        starts = list(starts)                                   # data-dependent sizes: the one host read
        dual = torch.empty((starts[L + 1], 3), dtype=torch.int16, device=dev)
        _lib.check(lib.kamd_spc_dual_emit(sp, n, L, _lib.ptr(ws), starts[L + 1], _lib.ptr(dual)), fn)
    pyramid_dual = torch.tensor([[starts[l + 1] - starts[l] for l in range(L + 1)] + [0], starts], dtype=pyramid.dtype)
    return dual, pyramid_dual


def make_trinkets_cuda(point_hierarchy, pyramid, point_hierarchy_dual, pyramid_dual):
    """ours (the reference looks Morton codes up in Python dictionaries): -> (trinkets (num_points, 8) int32: the index of every
    corner in its level of the dual, relative to the level; parents (num_points) int32: absolute, -1 for the root).  One launch, no
    host read, no allocation besides the results: capturable."""
    fn = 'make_trinkets_cuda'
    _spc_points_arg(fn, point_hierarchy)
    _spc_points_arg(fn, point_hierarchy_dual)
    torch_check(point_hierarchy.device == point_hierarchy_dual.device, f'{fn}: expected every tensor on the same device')
    n, nd, dev = point_hierarchy.size(0), point_hierarchy_dual.size(0), point_hierarchy.device
    L, first = _spc_pyramid_row(fn, pyramid, 'pyramid', n)
    Ld, first_dual = _spc_pyramid_row(fn, pyramid_dual, 'pyramid_dual', nd)
    torch_check(L == Ld, f'{fn}: pyramid and pyramid_dual differ in depth')
    torch_check(n > 0, f'{fn}: no points')
    lib = _lib.load()
    with _lib.on_device(dev):
        trinkets = torch.empty((n, 8), dtype=torch.int32, device=dev)
        parents = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(lib.kamd_spc_trinkets(_lib.stream_ptr(dev), n, nd, L, _lib.ptr(point_hierarchy), _lib.ptr(point_hierarchy_dual),
                                         ctypes.cast(first, ctypes.c_void_p), ctypes.cast(first_dual, ctypes.c_void_p),
                                         _lib.ptr(trinkets), _lib.ptr(parents)), fn)
    return trinkets, parents


def coords_to_trilinear_cuda(coords, points, level):
    """reference: point_utils.cpp ``coords_to_trilinear_cuda``: coords (n, 3) half / float / double, points (n, 3) int16 -> (n, 8)
    coefficients c000, c001, ... in coords' dtype.  Unlike the reference, coords are the NORMALISED coordinates in [-1, 1] and
    ``level`` is an argument: the kernel evaluates ``2^level (c / 2 + 1 / 2) - p`` in double itself.  One launch, capturable."""
    fn = 'coords_to_trilinear_cuda'
    torch_check(coords.is_cuda and points.is_cuda, f'{fn}: coords and points must be CUDA tensors')
    torch_check(coords.device == points.device, f'{fn}: expected every tensor on the same device')
    torch_check(coords.dim() == 2 and coords.size(1) == 3 and coords.is_contiguous(), f'{fn}: coords must be contiguous, of size {{num_coords, 3}}')
    torch_check(points.dtype == torch.int16 and tuple(points.shape) == tuple(coords.shape) and points.is_contiguous(),
                f'{fn}: points must be a contiguous short tensor of the size of coords')
    sfx = _lib.dtype_suffix(coords.dtype, fn, allowed=('f16', 'f32', 'f64'))
    level = int(level)
    torch_check(0 <= level <= SPC_MAX_LEVEL, f'{fn}: level must be in [0, {SPC_MAX_LEVEL}]')
    lib = _lib.load()
    with _lib.on_device(coords.device):
        out = torch.empty((coords.size(0), 8), dtype=coords.dtype, device=coords.device)
        _lib.check(getattr(lib, f'kamd_spc_trilinear_coeffs_{sfx}')(_lib.stream_ptr(coords.device), coords.size(0), level,
                                                                  _lib.ptr(coords), _lib.ptr(points), _lib.ptr(out)), fn)
    return out


def _spc_interpolate_args(fn, coords, pidx, point_hierarchy, trinkets, feats, level, grad_out=None):
    """the checks of the reference's interpolate_trilinear_cuda (point_utils.cpp) -> (suffix, N, S, D, level)"""
    tensors = [coords, pidx, point_hierarchy, trinkets, feats] + ([grad_out] if grad_out is not None else [])
    torch_check(all(x.is_cuda for x in tensors), f'{fn}: coords, pidx, point_hierarchy, trinkets and feats must be CUDA tensors')
    torch_check(all(x.device == coords.device for x in tensors), f'{fn}: expected every tensor on the same device')
    torch_check(all(x.is_contiguous() for x in tensors), f'{fn}: expected contiguous tensors')
    torch_check(coords.dtype == torch.float32 and coords.dim() == 3 and coords.size(2) == 3 and coords.size(1) >= 1,
                f'{fn}: coords must be a float tensor of size {{num_voxels, num_samples, 3}}')
    torch_check(pidx.dtype == torch.int32 and pidx.dim() == 1 and pidx.size(0) == coords.size(0),
                f'{fn}: pidx must be an int tensor of size {{num_voxels}}')
    _spc_points_arg(fn, point_hierarchy)
    torch_check(trinkets.dtype == torch.int32 and trinkets.dim() == 2 and trinkets.size(1) == 8 and
                trinkets.size(0) == point_hierarchy.size(0), f'{fn}: trinkets must be an int tensor of size {{num_points, 8}}')
    torch_check(trinkets.data_ptr() % 16 == 0, f'{fn}: trinkets must be 16-byte aligned')
    torch_check(feats.dim() == 2 and feats.size(1) >= 1, f'{fn}: feats must be of size {{num_feats, feature_dim}}')
    sfx = _lib.dtype_suffix(feats.dtype, fn, allowed=('f16', 'f32', 'f64'))
    N, S, D = coords.size(0), coords.size(1), feats.size(1)
    if grad_out is not None:
        torch_check(grad_out.dtype == feats.dtype and tuple(grad_out.shape) == (N, S, D),
                    f'{fn}: grad_output must be a {_lib.pretty_dtype(feats.dtype)} tensor of size {(N, S, D)}')
    level = int(level)
    torch_check(0 <= level <= SPC_MAX_LEVEL, f'{fn}: level must be in [0, {SPC_MAX_LEVEL}]')
    return sfx, N, S, D, level


def interpolate_trilinear_cuda(coords, pidx, point_hierarchy, trinkets, feats, level):
    """reference: point_utils.cpp ``interpolate_trilinear_cuda``: coords (N, S, 3) float32 in [-1, 1], pidx (N) int32 (-1: a miss),
    point_hierarchy (num_points, 3) int16, trinkets (num_points, 8) int32, feats (num_feats, D) half / float / double -> (N, S, D).
    Lanes along D, a group of lanes per sample.  A pidx or a trinket out of range is a miss.  One launch, capturable."""
    fn = 'interpolate_trilinear_cuda'
    sfx, N, S, D, level = _spc_interpolate_args(fn, coords, pidx, point_hierarchy, trinkets, feats, level)
    dev = coords.device
    lib = _lib.load()
    with _lib.on_device(dev):
        out = torch.empty((N, S, D), dtype=feats.dtype, device=dev)
        _lib.check(getattr(lib, f'kamd_spc_interpolate_forward_{sfx}')(
            _lib.stream_ptr(dev), N, S, D, level, point_hierarchy.size(0), feats.size(0), _lib.ptr(coords), _lib.ptr(pidx),
            _lib.ptr(point_hierarchy), _lib.ptr(trinkets), _lib.ptr(feats), _lib.ptr(out)), fn)
    return out


def interpolate_trilinear_backward_feats_cuda(coords, pidx, point_hierarchy, trinkets, feats, level, grad_output):
    """ours (the reference chains torch operators): -> grad_feats, of the size and dtype of feats.  One fused kernel: coefficients
    recomputed, the samples of a voxel summed in registers, float (double for double) atomic adds into a zeroed buffer; half
    accumulates in float32 and is rounded once.  Results may differ in the last bits from run to run.  Capturable."""
    fn = 'interpolate_trilinear_backward_feats_cuda'
    sfx, N, S, D, level = _spc_interpolate_args(fn, coords, pidx, point_hierarchy, trinkets, feats, level, grad_output)
    dev = coords.device
    lib = _lib.load()
    with _lib.on_device(dev):
        grad = torch.empty_like(feats)
        sums = torch.empty(feats.shape, dtype=torch.float32, device=dev) if sfx == 'f16' else None     # alive until after the call
        extra = [_lib.ptr(sums)] if sums is not None else []
        _lib.check(getattr(lib, f'kamd_spc_interpolate_backward_feats_{sfx}')(
            _lib.stream_ptr(dev), N, S, D, level, point_hierarchy.size(0), feats.size(0), _lib.ptr(coords), _lib.ptr(pidx),
            _lib.ptr(point_hierarchy), _lib.ptr(trinkets), _lib.ptr(grad_output), *extra, _lib.ptr(grad)), fn)
    return grad


def interpolate_trilinear_backward_coords_cuda(coords, pidx, point_hierarchy, trinkets, feats, level, grad_output):
    """ours: -> (N, S, 3) float32, the derivative by the LOCAL cell coordinate (the reference's convention: no factor 2^(level - 1)).
    Lanes along D, a reduction across the group of a sample.  One launch, capturable."""
    fn = 'interpolate_trilinear_backward_coords_cuda'
    sfx, N, S, D, level = _spc_interpolate_args(fn, coords, pidx, point_hierarchy, trinkets, feats, level, grad_output)
    dev = coords.device
    lib = _lib.load()
    with _lib.on_device(dev):
        grad = torch.empty_like(coords)
        _lib.check(getattr(lib, f'kamd_spc_interpolate_backward_coords_{sfx}')(
            _lib.stream_ptr(dev), N, S, D, level, point_hierarchy.size(0), feats.size(0), _lib.ptr(coords), _lib.ptr(pidx),
            _lib.ptr(point_hierarchy), _lib.ptr(trinkets), _lib.ptr(feats), _lib.ptr(grad_output), _lib.ptr(grad)), fn)
    return grad


# ---- kaolin._C.ops.spc: sparse convolutions on csrc/spc_conv.hip -----------------------------------------------------------
def spc_conv_check(fn, transposed, octrees, point_hierarchies, level, pyramids, exsum, input, weight, kernel_vectors, jump,
                   bias=None, grad_output=None):
    """What conv3d / conv_transpose3d ask of their arguments on every device, before anything runs (ValueError; the reference's are
    asserts that are compiled out) -> (input level, output level).  ``level`` is the level of ``input``."""
    if not isinstance(pyramids, torch.Tensor) or pyramids.is_cuda or pyramids.dim() != 3 or pyramids.size(1) != 2 or \
            pyramids.size(2) < 2 or pyramids.is_floating_point():
        raise ValueError(f'{fn}: pyramids must be an integer CPU tensor of size (batch_size, 2, max_level + 2)')
    max_level = pyramids.size(2) - 2
    level, jump = int(level), int(jump)
    if max_level > SPC_MAX_LEVEL or pyramids.size(0) < 1:
        raise ValueError(f'{fn}: pyramids of {pyramids.size(0)} octrees of max_level {max_level}; at most {SPC_MAX_LEVEL}')
    if not 0 <= level <= max_level:
        raise ValueError(f'{fn}: level {level} outside [0, max_level = {max_level}]')
    if jump < 0:
        raise ValueError(f'{fn}: jump must not be negative, got {jump}')
    out_level = level + jump if transposed else level - jump
    if not 0 <= out_level <= max_level:
        raise ValueError(f'{fn}: level {level} and jump {jump} give the output level {out_level}, outside [0, max_level = {max_level}]')
    p = pyramids.tolist()                # plain integers from here on: a few dozen of them, cheaper than tensor arithmetic
    n_in, n_out = sum(item[0][level] for item in p), sum(item[0][out_level] for item in p)
    if input.dim() != 2 or input.size(0) != n_in or input.size(1) < 1:
        raise ValueError(f'{fn}: input must be of size ({n_in}, in_channels) for level {level}, got {tuple(input.shape)}')
    if kernel_vectors.dim() != 2 or kernel_vectors.size(1) != 3 or kernel_vectors.dtype != torch.int16 or kernel_vectors.size(0) < 1:
        raise ValueError(f'{fn}: kernel_vectors must be short, of size (num_weights, 3), got {kernel_vectors.dtype} '
                         f'{tuple(kernel_vectors.shape)}')
    K = kernel_vectors.size(0)
    if weight.dim() != 3 or weight.size(0) != K or weight.size(1) != input.size(1) or weight.size(2) < 1:
        raise ValueError(f'{fn}: weight must be of size ({K}, {input.size(1)}, out_channels), got {tuple(weight.shape)}')
    if bias is not None and tuple(bias.shape) != (weight.size(2),):
        raise ValueError(f'{fn}: bias must be of size ({weight.size(2)},), got {tuple(bias.shape)}')
    if grad_output is not None and tuple(grad_output.shape) != (n_out, weight.size(2)):
        raise ValueError(f'{fn}: grad_outputs must be of size {(n_out, weight.size(2))}, got {tuple(grad_output.shape)}')
    named = [('octrees', octrees), ('point_hierarchies', point_hierarchies), ('exsum', exsum), ('input', input), ('weight', weight),
             ('kernel_vectors', kernel_vectors)] + ([('bias', bias)] if bias is not None else []) + \
        ([('grad_outputs', grad_output)] if grad_output is not None else [])
    for name, x in named:
        if x.device != input.device:
            raise ValueError(f'{fn}: {name} is on {x.device}, input on {input.device}; pyramids alone stays on the CPU')
    for name, x in named[4:5] + named[6:]:
        if x.dtype != input.dtype:
            raise ValueError(f'{fn}: {name} is {x.dtype}, input {input.dtype}: input, weight and bias must be of one dtype')
    if not input.is_floating_point():
        raise ValueError(f'{fn}: input must be floating point, got {input.dtype}')
    if K * max(n_in, n_out) >= 2 ** 31:
        raise ValueError(f'{fn}: {K} kernel vectors x {max(n_in, n_out)} points: the neighbour table must stay below 2^31 entries')
    nbytes, npoints = sum(item[1][max_level] for item in p), sum(item[1][max_level + 1] for item in p)
    if octrees.dim() != 1 or octrees.dtype != torch.uint8 or octrees.numel() != nbytes:
        raise ValueError(f'{fn}: octrees must be a byte tensor of the {nbytes} bytes the pyramids describe, got {octrees.dtype} '
                         f'{tuple(octrees.shape)}')
    if point_hierarchies.dim() != 2 or point_hierarchies.size(1) != 3 or point_hierarchies.dtype != torch.int16 or \
            point_hierarchies.size(0) != npoints:
        raise ValueError(f'{fn}: point_hierarchies must be short, of the {npoints} points the pyramids describe, got '
                         f'{point_hierarchies.dtype} {tuple(point_hierarchies.shape)}')
    if exsum.dim() != 1 or exsum.numel() != nbytes or exsum.dtype != torch.int32:
        raise ValueError(f'{fn}: exsum has {exsum.numel()} {exsum.dtype} entries for {nbytes} octree bytes; only the current layout '
                         '(num_bytes int entries, inclusive sums) is accepted, not the legacy one with a leading 0 per octree')
    return level, out_level


def spc_conv_meta(pyramids, row_level, target_level):
    """The per-item table of kamd_spc_conv_map (int64, CPU) for rows at ``row_level`` and neighbours at ``target_level``."""
    p = pyramids.tolist()
    L = len(p[0][0]) - 2
    prefix, per_item = [0], []
    first_byte = first_point = first_target = 0
    for count, first in p:
        prefix.append(prefix[-1] + count[row_level])
        per_item += [first_byte, first[L], first_point + first[row_level], first[target_level], count[target_level], first_target]
        first_byte, first_point, first_target = first_byte + first[L], first_point + first[L + 1], first_target + count[target_level]
    return torch.tensor(prefix + per_item, dtype=torch.long)


def _spc_conv(fn, transposed, backward, octree, points, level, pyramid, exsum, inputs, grad_outputs, params, kernel_vectors, jump,
              needs=(True, True)):
    """The four convolution operators.  ``level`` is the level of ``inputs`` for a forward and -- as in the reference -- the
    level of the OUTPUT (what the forward returned) for a backward.  One neighbour map per call: the forward's is indexed by the
    output rows, the backward's by the input rows (the same triples, read the other way round), so both gradients are gathers."""
    tensors = [octree, points, exsum, inputs, params, kernel_vectors] + ([grad_outputs] if backward else [])
    torch_check(all(x.is_cuda for x in tensors), f'{fn}: octree, points, exsum, inputs, params and kernel_vectors must be CUDA tensors')
    jump = int(jump)
    if jump < 0:
        raise ValueError(f'{fn}: jump must not be negative, got {jump}')
    in_level = int(level) if not backward else (int(level) - jump if transposed else int(level) + jump)
    in_level, out_level = spc_conv_check(fn, transposed, octree, points, in_level, pyramid, exsum, inputs, params, kernel_vectors,
                                         jump, grad_output=grad_outputs if backward else None)
    sfx = _lib.dtype_suffix(inputs.dtype, fn)
    torch_check(all(x.is_contiguous() for x in tensors), f'{fn}: expected contiguous tensors')
    torch_check(pyramid.size(0) <= 65535, f'{fn}: more than 65535 octrees in a batch')
    K, cin, cout = params.shape
    torch_check(K <= 65535, f'{fn}: more than 65535 kernel vectors')
    counts = pyramid[:, 0].tolist()
    n_in, n_out = sum(c[in_level] for c in counts), sum(c[out_level] for c in counts)
    dev = inputs.device
    lib = _lib.load()
    sp = _lib.stream_ptr(dev)
    with _lib.on_device(dev):
        # forward: rows = outputs, neighbours = inputs; backward: rows = inputs, neighbours = outputs, the other mode
        row_level, target_level, n, targets = (in_level, out_level, n_in, n_out) if backward else (out_level, in_level, n_out, n_in)
        mode = int(transposed) ^ int(backward)
        meta = spc_conv_meta(pyramid, row_level, target_level).to(dev)
        table = torch.empty((K, n), dtype=torch.int32, device=dev)
        _lib.check(lib.kamd_spc_conv_map(sp, mode, pyramid.size(0), K, n, row_level, jump, octree.numel(), points.size(0), targets,
                                         _lib.ptr(octree), _lib.ptr(exsum), _lib.ptr(points), _lib.ptr(kernel_vectors),
                                         _lib.ptr(meta), _lib.ptr(table)), fn)
        gather = getattr(lib, f'kamd_spc_conv_gather_{sfx}')
        if not backward:
            out = torch.empty((n_out, cout), dtype=inputs.dtype, device=dev)
            _lib.check(gather(sp, n_out, K, n_in, cin, cout, 0, _lib.ptr(table), _lib.ptr(inputs), _lib.ptr(params), _lib.ptr(out)), fn)
            return out, out_level
        grad_inputs = grad_params = None
        if needs[0]:
            grad_inputs = torch.empty_like(inputs)
            _lib.check(gather(sp, n_in, K, n_out, cout, cin, 1, _lib.ptr(table), _lib.ptr(grad_outputs), _lib.ptr(params),
                              _lib.ptr(grad_inputs)), fn)
        if needs[1]:
            grad_params = torch.empty_like(params)
            nbytes = lib.kamd_spc_conv_workspace(K, cin, cout, inputs.element_size())
            ws = _lib.workspace(nbytes, dev)
            _lib.check(getattr(lib, f'kamd_spc_conv_wgrad_{sfx}')(sp, n_in, K, n_out, cin, cout, _lib.ptr(table), _lib.ptr(inputs),
                                                                 _lib.ptr(grad_outputs), _lib.ptr(ws), nbytes, _lib.ptr(grad_params)), fn)
    return [grad_inputs, grad_params]


def Conv3d_forward(octree, points, level, pyramid, exsum, inputs, params, kernel_vectors, jump):
    """reference: convolution.cpp ``Conv3d_forward``: inputs (points of ``level`` in the batch, in), params (K, in, out),
    kernel_vectors (K, 3) int16 -> (outputs (points of level - jump, out), level - jump).  Two launches (neighbour map,
    gather-GEMM) for the whole batch, no host read, no atomics (the reference: per item a scan, a compaction, K host reads and a
    kernel per offset that adds with float atomics)."""
    return _spc_conv('Conv3d_forward', False, False, octree, points, level, pyramid, exsum, inputs, None, params, kernel_vectors, jump)


def Conv3d_backward(octree, points, level, pyramid, exsum, inputs, grad_outputs, params, kernel_vectors, jump, needs=(True, True)):
    """reference: convolution.cpp ``Conv3d_backward``: ``level`` is the forward's OUTPUT level -> [grad_inputs, grad_params].
    Four launches (transposed map over the input rows, gather-GEMM with W^T, weight gradient, its finishing sum); ``needs`` (ours)
    skips a gradient nobody asked for (None in its place)."""
    return _spc_conv('Conv3d_backward', False, True, octree, points, level, pyramid, exsum, inputs, grad_outputs, params,
                     kernel_vectors, jump, needs)


def ConvTranspose3d_forward(octree, points, level, pyramid, exsum, inputs, params, kernel_vectors, jump):
    """reference: convolution.cpp ``ConvTranspose3d_forward``: -> (outputs (points of level + jump, out), level + jump)."""
    return _spc_conv('ConvTranspose3d_forward', True, False, octree, points, level, pyramid, exsum, inputs, None, params,
                     kernel_vectors, jump)


def ConvTranspose3d_backward(octree, points, level, pyramid, exsum, inputs, grad_outputs, params, kernel_vectors, jump,
                             needs=(True, True)):
    """reference: convolution.cpp ``ConvTranspose3d_backward``: ``level`` is the forward's OUTPUT level -> [grad_inputs,
    grad_params]; the direct map over the (coarse) input rows."""
    return _spc_conv('ConvTranspose3d_backward', True, True, octree, points, level, pyramid, exsum, inputs, grad_outputs, params,
                     kernel_vectors, jump, needs)


# ---- kaolin._C.ops.spc: Bayesian-fusion reconstruction on csrc/spc_bf.hip ----------------------------------------------------------
def _bf_need(fn, cond, msg):
    if not cond:
        raise ValueError(f'{fn}: {msg}')


def _bf_tensor(fn, t, name, dtype, cols=None, cuda=True):
    _bf_need(fn, isinstance(t, torch.Tensor) and t.dtype == dtype, f'{name} must be a {_lib.pretty_dtype(dtype)} tensor')
    _bf_need(fn, t.is_cuda == cuda, f'{name} must be a {"CUDA" if cuda else "CPU"} tensor')
    _bf_need(fn, t.is_contiguous(), f'{name} must be contiguous')
    if cols is None:
        _bf_need(fn, t.dim() == 1, f'{name} must be 1D, got {tuple(t.shape)}')
    else:
        _bf_need(fn, t.dim() == 2 and t.size(1) == cols, f'{name} must be of size (n, {cols}), got {tuple(t.shape)}')


def _bf_same_device(fn, *tensors):
    _bf_need(fn, len({t.device for t in tensors}) == 1, 'expected every CUDA tensor on the same device')


def _bf_level(fn, level):
    level = int(level)
    _bf_need(fn, 0 <= level <= SPC_MAX_LEVEL, f'level must be in [0, {SPC_MAX_LEVEL}], got {level}')
    return level


def bf_transform(cam, level):
    """T = M * cam as 16 float32 (numpy, row major): M = diag(s, s, s, 1) with last row (-1, -1, -1, 1), s = 2^(1 - level); every
    element is the sum over k = 0..3, in that order, of float32 products (the arithmetic contract)."""
    import numpy as np
    c = cam.detach().cpu().numpy().astype(np.float32).reshape(4, 4)
    s = np.float32(2.0 ** (1 - level))
    M = np.array([[s, 0, 0, 0], [0, s, 0, 0], [0, 0, s, 0], [-1, -1, -1, 1]], dtype=np.float32)
    T = np.zeros((4, 4), dtype=np.float32)
    with np.errstate(all='ignore'):         # (a non-finite cam is the caller's to refuse)
        for i in range(4):
            for j in range(4):
                acc = M[i, 0] * c[0, j]
                for k in range(1, 4):
                    acc = np.float32(acc + np.float32(M[i, k] * c[k, j]))
                T[i, j] = acc
    return T


def _bf_cam(fn, cam, level):
    _bf_need(fn, isinstance(cam, torch.Tensor) and tuple(cam.shape) == (4, 4) and cam.dtype == torch.float32,
             'cam must be a float tensor of size (4, 4)')
    T = bf_transform(cam, level)
    _bf_need(fn, bool(torch.isfinite(cam).all()) and bool(torch.isfinite(torch.from_numpy(T)).all()),
             'cam, and its product with the level\'s scaling, must be finite')
    return (ctypes.c_float * 16)(*[float(v) for v in T.reshape(-1)])


def _bf_depth(fn, depth_map):
    _bf_need(fn, isinstance(depth_map, torch.Tensor) and depth_map.dtype == torch.float32 and depth_map.dim() == 2,
             'depth_map must be a float tensor of size (height, width)')
    _bf_need(fn, depth_map.is_cuda and depth_map.is_contiguous(), 'depth_map must be a contiguous CUDA tensor')
    _bf_need(fn, depth_map.numel() > 0, 'depth_map is empty')
    return depth_map.size(0), depth_map.size(1)


def _bf_mip_size(fn, h, w, mip_levels):
    mip_levels = int(mip_levels)
    size = _lib.load().kamd_spc_bf_mip_size(h, w, mip_levels)
    _bf_need(fn, size >= 0, f'mip_levels must be in [1, 15] and divide the {h} x {w} depth map into whole 2^mip_levels blocks, '
                            f'got {mip_levels}')
    return mip_levels, size


def build_mip2d(depth_map, intrinsics, mip_levels, max_depth, true_depth):
    """reference: recon.cpp ``build_mip2d``: depth_map (h, w) float CUDA, intrinsics (4, 4) float (fx, fy at [0, 0], [1, 1]; cx, cy
    at [2, 0], [2, 1]) -> the min / max pyramid (size, 2), coarsest level first.  With ``true_depth`` depth_map is converted IN PLACE
    from ray length to z depth (pixels equal to max_depth stay).  mip_levels launches, capturable."""
    fn = 'build_mip2d'
    h, w = _bf_depth(fn, depth_map)
    mip_levels, size = _bf_mip_size(fn, h, w, mip_levels)
    _bf_need(fn, isinstance(intrinsics, torch.Tensor) and tuple(intrinsics.shape) == (4, 4), 'intrinsics must be of size (4, 4)')
    k = intrinsics.detach().cpu().float().reshape(-1).tolist()
    _bf_need(fn, k[0] != 0.0 and k[5] != 0.0, 'the focal lengths must not be zero')
    lib, dev = _lib.load(), depth_map.device
    with _lib.on_device(dev):
        mip = torch.empty((size, 2), dtype=torch.float32, device=dev)
        _lib.check(lib.kamd_spc_bf_build_mip2d(_lib.stream_ptr(dev), h, w, mip_levels, k[0], k[5], k[8], k[9], float(max_depth),
                                               int(bool(true_depth)), _lib.ptr(depth_map), _lib.ptr(mip)), fn)
    return mip


def oracleB(points, level, sigma, cam, depth_map, mips, mip_levels):
    """reference: bf.cpp ``oracleB``: points (n, 3) short of ``level`` against the depth pyramid -> (occupancy, state) int32 (n):
    state 0 empty, 1 unseen, 2 occupied; occupancy 1 = keep and split.  One launch, capturable."""
    fn = 'oracleB'
    _bf_tensor(fn, points, 'points', torch.int16, 3)
    level = _bf_level(fn, level)
    h, w = _bf_depth(fn, depth_map)
    mip_levels, size = _bf_mip_size(fn, h, w, mip_levels)
    _bf_tensor(fn, mips, 'mips', torch.float32, 2)
    _bf_need(fn, mips.size(0) == size, f'mips has {mips.size(0)} rows, a {h} x {w} map with {mip_levels} levels has {size}')
    _bf_same_device(fn, points, depth_map, mips)
    _bf_need(fn, float(sigma) != 0.0, "sigma can't be zero")
    T = _bf_cam(fn, cam, level)
    lib, dev, n = _lib.load(), points.device, points.size(0)
    with _lib.on_device(dev):
        occ = torch.empty(n, dtype=torch.int32, device=dev)
        state = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(lib.kamd_spc_bf_oracle(_lib.stream_ptr(dev), n, _lib.ptr(points), level, ctypes.cast(T, ctypes.c_void_p), float(sigma),
                                          _lib.ptr(depth_map), h, w, mip_levels, _lib.ptr(mips), _lib.ptr(occ), _lib.ptr(state)), fn)
    return occ, state


def oracleB_final(points, level, sigma, cam, depth_map):
    """reference: bf.cpp ``oracleB_final``: the profile curve at the eight corners of every point -> (occupancy, state,
    probabilities (n) float: the curve at corner 0).  One launch, capturable."""
    fn = 'oracleB_final'
    _bf_tensor(fn, points, 'points', torch.int16, 3)
    level = _bf_level(fn, level)
    h, w = _bf_depth(fn, depth_map)
    _bf_same_device(fn, points, depth_map)
    _bf_need(fn, float(sigma) != 0.0, "sigma can't be zero")
    T = _bf_cam(fn, cam, level)
    lib, dev, n = _lib.load(), points.device, points.size(0)
    with _lib.on_device(dev):
        occ = torch.empty(n, dtype=torch.int32, device=dev)
        state = torch.empty(n, dtype=torch.int32, device=dev)
        probs = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(lib.kamd_spc_bf_oracle_final(_lib.stream_ptr(dev), n, _lib.ptr(points), level, ctypes.cast(T, ctypes.c_void_p),
                                                float(sigma), _lib.ptr(depth_map), h, w, _lib.ptr(occ), _lib.ptr(state),
                                                _lib.ptr(probs)), fn)
    return occ, state, probs


def colorsB_final(points, level, cam, sigma, image, depth_map, probabilities):
    """reference: bf.cpp ``colorsB_final``: -> (colors (n, 4) uint8 in B, G, R, 0 order, normals (n, 3) float).  A normal that is
    not finite is a zero row (the reference writes NaN).  One launch, capturable."""
    fn = 'colorsB_final'
    _bf_tensor(fn, points, 'points', torch.int16, 3)
    level = _bf_level(fn, level)
    h, w = _bf_depth(fn, depth_map)
    n = points.size(0)
    _bf_need(fn, isinstance(image, torch.Tensor) and image.dtype == torch.float32 and tuple(image.shape) == (h, w, 3) and
             image.is_cuda and image.is_contiguous(), f'image must be a contiguous CUDA float tensor of size ({h}, {w}, 3)')
    _bf_tensor(fn, probabilities, 'probabilities', torch.float32)
    _bf_need(fn, probabilities.numel() == n, f'probabilities has {probabilities.numel()} entries for {n} points')
    _bf_same_device(fn, points, depth_map, image, probabilities)
    _bf_need(fn, float(sigma) > 0.0, 'sigma must be strictly positive')
    T = _bf_cam(fn, cam, level)
    lib, dev = _lib.load(), points.device
    with _lib.on_device(dev):
        colors = torch.empty((n, 4), dtype=torch.uint8, device=dev)
        normals = torch.empty((n, 3), dtype=torch.float32, device=dev)
        _lib.check(lib.kamd_spc_bf_colors_final(_lib.stream_ptr(dev), n, _lib.ptr(points), ctypes.cast(T, ctypes.c_void_p), float(sigma),
                                                _lib.ptr(image), _lib.ptr(depth_map), h, w, _lib.ptr(probabilities), _lib.ptr(colors),
                                                _lib.ptr(normals)), fn)
    return colors, normals


def inclusive_sum(inputs):
    """reference: recon.cpp ``inclusive_sum``: int32 (n) -> its inclusive sum, int32 (the two-level block scan of the octree build).
    Two launches, capturable."""
    fn = 'inclusive_sum'
    _bf_tensor(fn, inputs, 'inputs', torch.int32)
    lib, dev, n = _lib.load(), inputs.device, inputs.numel()
    with _lib.on_device(dev):
        out = torch.empty_like(inputs)
        if n > 0:
            ws = _lib.workspace(lib.kamd_spc_bf_scan_workspace(n), dev)
            _lib.check(lib.kamd_spc_bf_inclusive_sum(_lib.stream_ptr(dev), n, _lib.ptr(inputs), _lib.ptr(out), _lib.ptr(ws)), fn)
    return out


def _bf_compact(fn, points, insum, subdivide):
    _bf_tensor(fn, points, 'points', torch.int16, 3)
    _bf_tensor(fn, insum, 'insum', torch.int32)
    _bf_same_device(fn, points, insum)
    n, dev = points.size(0), points.device
    _bf_need(fn, insum.numel() == n, f'insum has {insum.numel()} entries for {n} points')
    lib = _lib.load()
    with _lib.on_device(dev):
        npass = int(insum[-1]) if n > 0 else 0          # the host read
        _bf_need(fn, 0 <= npass <= n, f'insum ends at {npass} for {n} points: not an inclusive sum of 0 / 1 flags')
        new_points = torch.zeros((8 * npass if subdivide else npass, 3), dtype=torch.int16, device=dev)
        nvsum = torch.zeros(npass, dtype=torch.int32 if subdivide else torch.long, device=dev)
        op = lib.kamd_spc_bf_subdivide if subdivide else lib.kamd_spc_bf_compactify
        _lib.check(op(_lib.stream_ptr(dev), n, npass, _lib.ptr(points), _lib.ptr(insum), _lib.ptr(new_points), _lib.ptr(nvsum)), fn)
    return new_points, nvsum


def subdivide(points, insum):
    """reference: recon.cpp ``subdivide``: the kept points (insum steps) -> (their 8 children each (8 * pass, 3) short, nvsum (pass)
    int32: the index of every kept point).  One host read (pass), one launch."""
    return _bf_compact('subdivide', points, insum, True)


def compactify(points, insum):
    """reference: recon.cpp ``compactify``: -> (the kept points (pass, 3), nvsum (pass) int64)."""
    return _bf_compact('compactify', points, insum, False)


def process_final_voxels(num_nodes, total_nodes, state, nvsum, occupancies, prev_state, octree, empty):
    """reference: bf.cpp ``process_final_voxels``: the states of 8 * num_nodes sibling voxels -> the nodes' octree / empty bytes and
    occupancies, written IN PLACE at ``size - total_nodes`` of the three buffers, and the parents' states into prev_state at nvsum.
    Returns (octree, empty, occupancies).  One launch, capturable."""
    fn = 'process_final_voxels'
    num_nodes, total_nodes = int(num_nodes), int(total_nodes)
    for t, name, dt in ((state, 'state', torch.int32), (nvsum, 'nvsum', torch.int32), (occupancies, 'occupancies', torch.int32),
                        (prev_state, 'prev_state', torch.int32), (octree, 'octree', torch.uint8), (empty, 'empty', torch.uint8)):
        _bf_tensor(fn, t, name, dt)
    _bf_same_device(fn, state, nvsum, occupancies, prev_state, octree, empty)
    size = octree.numel()
    _bf_need(fn, empty.numel() == size and occupancies.numel() == size, 'octree, empty and occupancies must have the same size')
    _bf_need(fn, 0 <= num_nodes <= total_nodes <= size, f'expected 0 <= num_nodes ({num_nodes}) <= total_nodes ({total_nodes}) <= '
                                                        f'the buffers\' size ({size})')
    _bf_need(fn, state.numel() >= 8 * num_nodes and nvsum.numel() >= num_nodes,
             f'state has {state.numel()} entries and nvsum {nvsum.numel()} for {num_nodes} nodes')
    lib, dev, at = _lib.load(), octree.device, size - total_nodes
    with _lib.on_device(dev):
        _lib.check(lib.kamd_spc_bf_process_final_voxels(
            _lib.stream_ptr(dev), num_nodes, _lib.ptr(state), _lib.ptr(nvsum), prev_state.numel(), occupancies.data_ptr() + 4 * at,
            _lib.ptr(prev_state), octree.data_ptr() + at, empty.data_ptr() + at), fn)
    return octree, empty, occupancies


def compactify_nodes(total_nodes, insum, octree, empty):
    """reference: bf.cpp ``compactify_nodes``: the first total_nodes bytes of octree / empty whose insum steps -> (octree, empty)
    compacted.  Reads the scan's prefix of total_nodes entries only.  One host read, one launch."""
    fn = 'compactify_nodes'
    total_nodes = int(total_nodes)
    _bf_tensor(fn, insum, 'insum', torch.int32)
    _bf_tensor(fn, octree, 'octree', torch.uint8)
    _bf_tensor(fn, empty, 'empty', torch.uint8)
    _bf_same_device(fn, insum, octree, empty)
    _bf_need(fn, 0 <= total_nodes <= min(insum.numel(), octree.numel(), empty.numel()),
             f'total_nodes {total_nodes} exceeds insum ({insum.numel()}), octree ({octree.numel()}) or empty ({empty.numel()})')
    lib, dev = _lib.load(), octree.device
    with _lib.on_device(dev):
        npass = int(insum[total_nodes - 1]) if total_nodes > 0 else 0       # the host read
        _bf_need(fn, 0 <= npass <= total_nodes, f'insum reaches {npass} after {total_nodes} nodes: not an inclusive sum of 0 / 1 flags')
        new_octree = torch.zeros(npass, dtype=torch.uint8, device=dev)
        new_empty = torch.zeros(npass, dtype=torch.uint8, device=dev)
        _lib.check(lib.kamd_spc_bf_compactify_nodes(_lib.stream_ptr(dev), total_nodes, npass, _lib.ptr(insum), _lib.ptr(octree),
                                                    _lib.ptr(empty), _lib.ptr(new_octree), _lib.ptr(new_empty)), fn)
    return new_octree, new_empty


def _bf_tree(fn, octree, empty, exsum, k=''):
    _bf_tensor(fn, octree, f'octree{k}', torch.uint8)
    _bf_tensor(fn, empty, f'empty{k}', torch.uint8)
    _bf_tensor(fn, exsum, f'exsum{k}', torch.int32)
    _bf_need(fn, empty.numel() == octree.numel(), f'empty{k} has {empty.numel()} bytes, octree{k} {octree.numel()}')
    if exsum.numel() != octree.numel():
        raise ValueError(f'{fn}: exsum{k} has {exsum.numel()} entries for {octree.numel()} octree bytes; only the current layout '
                         '(num_bytes entries, inclusive sums) is accepted, not the legacy one with a leading 0 per octree')


def merge_empty(points, level, octree0, octree1, empty0, empty1, exsum0, exsum1):
    """reference: bf.cpp ``merge_empty``: points of ``level`` looked up in two (octree, empty) trees -> (occupancy, state): empty
    where either tree is empty, unseen where both are unseen, occupied otherwise.  One launch, capturable."""
    fn = 'merge_empty'
    _bf_tensor(fn, points, 'points', torch.int16, 3)
    level = _bf_level(fn, level)
    _bf_tree(fn, octree0, empty0, exsum0, '0')
    _bf_tree(fn, octree1, empty1, exsum1, '1')
    _bf_same_device(fn, points, octree0, octree1, empty0, empty1, exsum0, exsum1)
    lib, dev, n = _lib.load(), points.device, points.size(0)
    with _lib.on_device(dev):
        occ = torch.empty(n, dtype=torch.int32, device=dev)
        state = torch.empty(n, dtype=torch.int32, device=dev)
        _lib.check(lib.kamd_spc_bf_merge_empty(_lib.stream_ptr(dev), n, _lib.ptr(points), level, octree0.numel(), octree1.numel(),
                                               _lib.ptr(octree0), _lib.ptr(octree1), _lib.ptr(empty0), _lib.ptr(empty1),
                                               _lib.ptr(exsum0), _lib.ptr(exsum1), _lib.ptr(occ), _lib.ptr(state)), fn)
    return occ, state


def bq_merge(points, level, octree0, octree1, empty0, empty1, pyramid0, pyramid1, probs0, probs1, colors0, colors1, normals0,
             normals1, exsum0, exsum1):
    """reference: bf.cpp ``bq_merge``: the closed-form fusion p0 p1 / (p0 p1 + (1 - p0)(1 - p1)) of two trees at the points of
    ``level`` -> (occupancy, state, probabilities, colors, normals); unoccupied rows are zero, normals are all zero (as in the
    reference).  One launch, capturable."""
    fn = 'bq_merge'
    _bf_tensor(fn, points, 'points', torch.int16, 3)
    level = _bf_level(fn, level)
    _bf_tree(fn, octree0, empty0, exsum0, '0')
    _bf_tree(fn, octree1, empty1, exsum1, '1')
    offs = []
    for k, (pyr, probs, colors) in enumerate(((pyramid0, probs0, colors0), (pyramid1, probs1, colors1))):
        _bf_need(fn, isinstance(pyr, torch.Tensor) and not pyr.is_cuda and pyr.dim() == 3 and pyr.size(1) == 2 and
                 pyr.size(2) >= level + 2, f'pyramid{k} must be a CPU tensor of size (1, 2, max_level + 2) with max_level >= {level}')
        _bf_tensor(fn, probs, f'probs{k}', torch.float32)
        _bf_tensor(fn, colors, f'colors{k}', torch.uint8, 4)
        _bf_need(fn, colors.size(0) == probs.numel(), f'colors{k} has {colors.size(0)} rows, probs{k} {probs.numel()}')
        offs.append(int(pyr[0, 1, level]))
    _bf_same_device(fn, points, octree0, octree1, empty0, empty1, exsum0, exsum1, probs0, probs1, colors0, colors1)
    lib, dev, n = _lib.load(), points.device, points.size(0)
    with _lib.on_device(dev):
        occ = torch.empty(n, dtype=torch.int32, device=dev)
        state = torch.empty(n, dtype=torch.int32, device=dev)
        probs = torch.empty(n, dtype=torch.float32, device=dev)
        colors = torch.empty((n, 4), dtype=torch.uint8, device=dev)
        normals = torch.zeros((n, 3), dtype=torch.float32, device=dev)
        _lib.check(lib.kamd_spc_bf_merge(_lib.stream_ptr(dev), n, _lib.ptr(points), level, octree0.numel(), octree1.numel(),
                                         _lib.ptr(octree0), _lib.ptr(octree1), _lib.ptr(empty0), _lib.ptr(empty1), _lib.ptr(exsum0),
                                         _lib.ptr(exsum1), offs[0], offs[1], probs0.numel(), probs1.numel(), _lib.ptr(probs0),
                                         _lib.ptr(probs1), _lib.ptr(colors0), _lib.ptr(colors1), _lib.ptr(occ), _lib.ptr(state),
                                         _lib.ptr(probs), _lib.ptr(colors)), fn)
    return occ, state, probs, colors, normals


def query_cuda_empty(octree, empty, exsum, query_coords, level):
    """reference: query.cpp ``query_cuda_empty``: query_coords (Q, 3) half / float / double in [-1, 1] -> int32 (Q): >= 0 the point
    index, -1 empty space or outside the cube, -2 - depth unseen space (``depth`` levels left below the node where the walk
    stopped).  Quantised as floor(2^level (q / 2 + 1 / 2)) in double.  One launch, capturable."""
    fn = 'query_cuda_empty'
    _bf_tree(fn, octree, empty, exsum)
    level = _bf_level(fn, level)
    _bf_need(fn, isinstance(query_coords, torch.Tensor) and query_coords.is_cuda and query_coords.is_contiguous() and
             query_coords.dim() == 2 and query_coords.size(1) == 3, 'query_coords must be a contiguous CUDA tensor of size (Q, 3)')
    _bf_same_device(fn, octree, empty, exsum, query_coords)
    sfx = _lib.dtype_suffix(query_coords.dtype, fn, allowed=('f16', 'f32', 'f64'))
    lib, dev, Q = _lib.load(), octree.device, query_coords.size(0)
    with _lib.on_device(dev):
        if octree.numel() == 0 and level > 0:
            return torch.full((Q,), -1, dtype=torch.int32, device=dev)
        out = torch.empty(Q, dtype=torch.int32, device=dev)
        _lib.check(getattr(lib, f'kamd_spc_bf_query_{sfx}')(_lib.stream_ptr(dev), Q, level, octree.numel(), _lib.ptr(octree),
                                                           _lib.ptr(empty), _lib.ptr(exsum), _lib.ptr(query_coords), _lib.ptr(out)), fn)
    return out


def bf_cells_cuda(octree, empty, level):
    """(no reference counterpart) The cells of ``level`` that query_cuda_empty does not answer with -1 -- occupied leaves and every
    cell of an unseen block -- as (K, 3) short in ascending Morton order: what the reference's densifier gets from querying all
    8^level cells of a dense grid, with work proportional to K.  A count per node, level by level from the leaves up (an occupied
    leaf bit counts 1, an unseen bit at depth d counts 8^(level - 1 - d), an inner bit its child's count), one host read of K, and
    one thread per output cell that walks down from the root skipping whole subtrees by their counts."""
    fn = 'bf_cells_cuda'
    _bf_tensor(fn, octree, 'octree', torch.uint8)
    _bf_tensor(fn, empty, 'empty', torch.uint8)
    _bf_same_device(fn, octree, empty)
    _bf_need(fn, empty.numel() == octree.numel(), f'empty has {empty.numel()} bytes, octree {octree.numel()}')
    level = _bf_level(fn, level)
    _bf_need(fn, level <= 14, 'the count of an unseen root bit, 8^(level - 1), must fit the walk: level at most 14')
    lib, dev, nb = _lib.load(), octree.device, octree.numel()
    with _lib.on_device(dev):
        if level == 0:
            return torch.zeros((1, 3), dtype=torch.int16, device=dev)
        if nb == 0:
            return torch.zeros((0, 3), dtype=torch.int16, device=dev)
        _bf_need(fn, nb * 8 < 2 ** 31, f'{nb} bytes: the octree must stay below 2^28 bytes')
        ws = _lib.workspace(lib.kamd_spc_bf_cells_workspace(nb), dev)
        host = (ctypes.c_int64 * 2)()
        sp = _lib.stream_ptr(dev)
        _lib.check(lib.kamd_spc_bf_cells_count(sp, nb, level, _lib.ptr(octree), _lib.ptr(empty), _lib.ptr(ws),
                                               ctypes.cast(host, ctypes.c_void_p)), fn)
        K, used = int(host[0]), int(host[1])            # the one host read
        _bf_need(fn, used == nb, f'{level} levels of the octree account for {used} bytes, it holds {nb}')
        _bf_need(fn, 0 <= K <= 8 ** level, f'the counts of the octree give {K} cells, level {level} has {8 ** level}')
        cells = torch.empty((K, 3), dtype=torch.int16, device=dev)
        _lib.check(lib.kamd_spc_bf_cells_emit(sp, nb, level, _lib.ptr(octree), _lib.ptr(empty), _lib.ptr(ws), K, _lib.ptr(cells)), fn)
    return cells


# ---- kaolin._C.ops.conversions: point clouds on csrc/pointcloud.hip (no reference counterpart: pure PyTorch there) -----------------
_PC_DTYPES = {torch.bool: 0, torch.uint8: 1, torch.int8: 2, torch.int16: 3, torch.int32: 4, torch.int64: 5, torch.float16: 6,
              torch.float32: 7, torch.float64: 8}


def pointcloud_to_spc_cuda(pointcloud, level, features=None):
    """pointcloud (N, 3) float / double of any strides, or short (quantised by the caller, contiguous); features (N, D) of any strides,
    bool / uint8 / int8 / int16 / int32 / int64 / half / float / double, or None -> (octree (num_bytes) uint8, features (U, D) or
    None): the octree of the occupied cells of ``level`` and the mean feature of every cell, in Morton order.

    Launches: 1 (keys) + 4 per 8 key bits (the pair sort) + 4 (run heads, scan, run starts) + 5 + 4 * level (the octree build) + 1
    (gather) + 2 (the mean).  ONE host read (unique cells and level sizes together); the call synchronises the current stream and
    cannot be captured in a graph."""
    fn = 'pointcloud_to_spc_cuda'
    torch_check(pointcloud.is_cuda, f'{fn}: pointcloud must be a CUDA tensor')
    torch_check(pointcloud.dim() == 2 and pointcloud.size(1) == 3, f'{fn}: pointcloud must be Nx3')
    torch_check(pointcloud.dtype in (torch.float32, torch.float64, torch.int16), f'{fn}: pointcloud must be float, double or short')
    level, n, dev = int(level), pointcloud.size(0), pointcloud.device
    torch_check(1 <= level <= SPC_MAX_LEVEL, f'{fn}: level must be in [1, {SPC_MAX_LEVEL}]')
    torch_check(n > 0, f'{fn}: no points')
    if features is not None:
        torch_check(features.is_cuda and features.device == dev, f'{fn}: features must be on the pointcloud\'s device')
        torch_check(features.dim() == 2 and features.size(0) == n and features.size(1) >= 1, f'{fn}: features must be NxD, D >= 1')
        torch_check(features.dtype in _PC_DTYPES, f'{fn}: features of {features.dtype} are not supported')
    lib = _lib.load()
    sp = _lib.stream_ptr(dev)
    with _lib.on_device(dev):
        nbytes = lib.kamd_pointcloud_spc_workspace(n, level)
        ws = _lib.workspace(nbytes, dev)
        sizes = (ctypes.c_int64 * (1 + level))()
        host = ctypes.cast(sizes, ctypes.c_void_p)
        if pointcloud.dtype == torch.int16:
            torch_check(pointcloud.is_contiguous(), f'{fn}: quantised points must be contiguous')
            st = lib.kamd_pointcloud_spc_build_i16(sp, n, level, _lib.ptr(pointcloud), _lib.ptr(ws), nbytes, host)
        else:
            sfx = 'f32' if pointcloud.dtype == torch.float32 else 'f64'
            st = getattr(lib, f'kamd_pointcloud_spc_build_{sfx}')(sp, n, level, _lib.ptr(pointcloud), pointcloud.stride(0),
                                                                   pointcloud.stride(1), _lib.ptr(ws), nbytes, host)
        _lib.check(st, fn)
        U, octree_bytes = int(sizes[0]), sum(sizes[1:])        # data-dependent sizes: the one host read
        if not (1 <= U <= n and 1 <= octree_bytes <= level * n):
            raise RuntimeError(f'{fn}: the build reports {U} cells and {octree_bytes} octree bytes for {n} points')
        octree = torch.empty(octree_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.kamd_pointcloud_spc_octree(sp, n, level, _lib.ptr(ws), octree_bytes, _lib.ptr(octree)), fn)
        feats = None
        if features is not None:
            f = features.detach()
            D = f.size(1)
            feats = torch.empty((U, D), dtype=f.dtype, device=dev)
            mws = _lib.workspace(lib.kamd_pointcloud_spc_mean_workspace(n, D), dev)
            _lib.check(lib.kamd_pointcloud_spc_mean(sp, _PC_DTYPES[f.dtype], n, level, U, D, _lib.ptr(f), f.stride(0), f.stride(1),
                                                    _lib.ptr(ws), _lib.ptr(mws), _lib.ptr(feats)), fn)
    return octree, feats


def pointclouds_to_voxelgrids_cuda(pointclouds, resolution, origin, scale, return_sparse=False):
    """pointclouds (B, P, 3) half / float / double, origin (B, 3), scale (B) of the same dtype -> dense (B, R, R, R) grid of 0/1 in
    that dtype (a zero fill and one launch, no host read), or with ``return_sparse`` the coalesced sparse COO tensor of the same
    voxels, compacted from a BIT grid (R^3 / 8 bytes per item; R^3 scalars are never allocated) as trianglemeshes_to_voxelgrids_cuda
    does: two ``nonzero`` calls, i.e. two host reads."""
    fn = 'pointclouds_to_voxelgrids_cuda'
    torch_check(pointclouds.is_cuda, f'{fn}: pointclouds must be a CUDA tensor')
    torch_check(pointclouds.dim() == 3 and pointclouds.size(2) == 3, f'{fn}: pointclouds must be of size {{batch_size, num_points, 3}}')
    sfx = _lib.dtype_suffix(pointclouds.dtype, fn, allowed=('f16', 'f32', 'f64'))
    p = pointclouds.detach().contiguous()
    B, P, R, dev, dtype = p.size(0), p.size(1), int(resolution), p.device, p.dtype
    torch_check(1 <= R <= 2048, f'{fn}: resolution must be in [1, 2048]')
    for name, t, shape in (('origin', origin, (B, 3)), ('scale', scale, (B,))):
        torch_check(t.is_cuda and t.device == dev and t.dtype == dtype and tuple(t.shape) == shape,
                    f'{fn}: {name} must be a {dtype} tensor of size {shape} on the pointclouds\' device')
    origin, scale = origin.detach().contiguous(), scale.detach().contiguous()
    mult = float((torch.ones(1, dtype=dtype) * (R - 1)).item())            # R - 1 as the dtype holds it (CPU arithmetic: no read)
    lib = _lib.load()
    call = getattr(lib, f'kamd_pointcloud_voxelgrids_{sfx}')
    with _lib.on_device(dev):
        if not return_sparse:
            grid = torch.empty((B, R, R, R), dtype=dtype, device=dev)
            _lib.check(call(_lib.stream_ptr(dev), B, P, R, mult, _lib.ptr(p), _lib.ptr(origin), _lib.ptr(scale), 0, _lib.ptr(grid)), fn)
            return grid
        words = (R ** 3 + 31) // 32
        bits = torch.empty((B, words), dtype=torch.int32, device=dev)
        _lib.check(call(_lib.stream_ptr(dev), B, P, R, mult, _lib.ptr(p), _lib.ptr(origin), _lib.ptr(scale), 1, _lib.ptr(bits)), fn)
        # compaction, sized by the occupied words (see trianglemeshes_to_voxelgrids_cuda): ascending linear indices per item
        nzw = torch.nonzero(bits)
        w = bits[nzw[:, 0], nzw[:, 1]]
        on = ((w.unsqueeze(1) >> torch.arange(32, device=dev, dtype=torch.int32)) & 1).bool()
        sel = torch.nonzero(on)
        lin = nzw[sel[:, 0], 1] * 32 + sel[:, 1]
        idx = torch.stack([nzw[sel[:, 0], 0], lin // (R * R), (lin // R) % R, lin % R])
        return torch.sparse_coo_tensor(idx, torch.ones(idx.shape[1], dtype=dtype, device=dev), (B, R, R, R), is_coalesced=True)


# ---- kaolin._C.ops.mesh: per-vertex sums / means on csrc/vertex_features.hip (no reference counterpart: scatter_add_ there) ---------
def _vf_extents(fn, F, K, V):
    if not (F >= 1 and K >= 1 and V >= 1):
        raise ValueError(f'{fn}: faces of shape ({F}, {K}) and {V} vertices: every extent must be at least 1')
    if F * K >= 2 ** 31 - 1:
        raise ValueError(f'{fn}: {F} x {K} face corners: the corner lists hold int32, K F must stay below 2^31 - 1')
    if V >= 2 ** 31 - 1:
        raise ValueError(f'{fn}: {V} vertices: the corner lists hold int32, V must stay below 2^31 - 1')


def _vf_faces(fn, faces):
    torch_check(isinstance(faces, torch.Tensor) and faces.is_cuda and faces.dim() == 2, f'{fn}: faces must be a CUDA tensor of size (F, K)')
    torch_check(faces.dtype in (torch.int32, torch.int64), f'{fn}: faces must be int or long')
    return faces.detach()


def vertex_corners_cuda(faces, num_vertices):
    """faces (F, K) int / long of any strides -> (offsets (V + 1) int32, corners (K F) int32): ``corners[offsets[v]:offsets[v + 1]]``
    are the corners ``i = k F + f`` with ``faces[f, k] == v`` in ascending ``i``, i.e. (corner slot, then face) order.

    Launches: 2 (clear, keys) + 4 per 8 bits of ceil(log2 V) (the keys-only sort; V = 1: one copy) + 1 (lists).  ONE host read (the
    count of ids outside [0, V): ``IndexError``); the call synchronises the current stream and cannot be captured in a graph.
    ``ValueError`` before any launch when K F or V reaches 2^31 - 1."""
    fn = 'vertex_corners_cuda'
    faces = _vf_faces(fn, faces)
    F, K, V, dev = faces.size(0), faces.size(1), int(num_vertices), faces.device
    _vf_extents(fn, F, K, V)
    lib = _lib.load()
    with _lib.on_device(dev):
        nbytes = lib.kamd_vertex_corners_workspace(F, K, V)
        ws = _lib.workspace(nbytes, dev)
        offsets = torch.empty(V + 1, dtype=torch.int32, device=dev)
        corners = torch.empty(F * K, dtype=torch.int32, device=dev)
        bad = ctypes.c_int32(0)
        _lib.check(lib.kamd_vertex_corners_build(_lib.stream_ptr(dev), F, K, V, _lib.ptr(faces), faces.element_size(), faces.stride(0),
                                                 faces.stride(1), _lib.ptr(ws), nbytes, _lib.ptr(offsets), _lib.ptr(corners),
                                                 ctypes.cast(ctypes.pointer(bad), ctypes.c_void_p)), fn)
    if bad.value != 0:                                                       # the one host read
        raise IndexError(f'{fn}: {bad.value} of the {F * K} face corners hold a vertex id outside [0, {V})')
    return offsets, corners


def _vf_lists(fn, offsets, corners, V, n, dev):
    torch_check(isinstance(offsets, torch.Tensor) and offsets.dtype == torch.int32 and offsets.device == dev and
                offsets.is_contiguous() and tuple(offsets.shape) == (V + 1,), f'{fn}: offsets must be a contiguous int tensor of size ({V + 1},)')
    if corners is not None:
        torch_check(isinstance(corners, torch.Tensor) and corners.dtype == torch.int32 and corners.device == dev and
                    corners.is_contiguous() and tuple(corners.shape) == (n,), f'{fn}: corners must be a contiguous int tensor of size ({n},)')


def vertex_gather_forward_cuda(face_features, offsets, corners, num_vertices, mean):
    """face_features (B, F, K, N) float / double of any strides (0 included) + the lists of vertex_corners_cuda -> (B, V, N): per
    vertex the sum of its corners' features in list order, one rounded addition per corner; ``mean``: divided once by
    max(count, 1).  One launch, no atomics, no host read: capturable, and two calls give the same bits."""
    fn = 'vertex_gather_forward_cuda'
    torch_check(isinstance(face_features, torch.Tensor) and face_features.is_cuda and face_features.dim() == 4,
                f'{fn}: face_features must be a CUDA tensor of size (B, F, K, N)')
    sfx = _lib.dtype_suffix(face_features.dtype, fn)
    x = face_features.detach()
    (B, F, K, N), V, dev = x.shape, int(num_vertices), x.device
    _vf_extents(fn, F, K, V)
    torch_check(B >= 1 and N >= 1, f'{fn}: face_features of size {tuple(x.shape)}: every extent must be at least 1')
    _vf_lists(fn, offsets, corners, V, F * K, dev)
    lib = _lib.load()
    with _lib.on_device(dev):
        out = torch.empty((B, V, N), dtype=x.dtype, device=dev)
        _lib.check(getattr(lib, f'kamd_vertex_gather_{sfx}')(_lib.stream_ptr(dev), B, F, K, V, N, _lib.ptr(x), x.stride(0), x.stride(1),
                                                            x.stride(2), x.stride(3), _lib.ptr(offsets), _lib.ptr(corners),
                                                            1 if mean else 0, _lib.ptr(out)), fn)
    return out


def vertex_gather_backward_cuda(grad_out, faces, offsets, mean):
    """grad_out (B, V, N) float / double of any strides, faces (F, K) int / long, offsets (V + 1) -> contiguous (B, F, K, N):
    ``grad[b, f, k, :] = grad_out[b, faces[f, k], :]``, divided by max(count, 1) with ``mean`` (the reference's autograd expression:
    one division).  One launch, no host read."""
    fn = 'vertex_gather_backward_cuda'
    torch_check(isinstance(grad_out, torch.Tensor) and grad_out.is_cuda and grad_out.dim() == 3,
                f'{fn}: grad_out must be a CUDA tensor of size (B, V, N)')
    sfx = _lib.dtype_suffix(grad_out.dtype, fn)
    faces = _vf_faces(fn, faces)
    g = grad_out.detach()
    (B, V, N), (F, K), dev = g.shape, faces.shape, g.device
    torch_check(faces.device == dev, f'{fn}: faces must be on the device of grad_out')
    _vf_extents(fn, F, K, V)
    torch_check(B >= 1 and N >= 1, f'{fn}: grad_out of size {tuple(g.shape)}: every extent must be at least 1')
    _vf_lists(fn, offsets, None, V, F * K, dev)
    lib = _lib.load()
    with _lib.on_device(dev):
        grad = torch.empty((B, F, K, N), dtype=g.dtype, device=dev)
        _lib.check(getattr(lib, f'kamd_vertex_gather_backward_{sfx}')(_lib.stream_ptr(dev), B, F, K, V, N, _lib.ptr(g), g.stride(0),
                                                                     g.stride(1), g.stride(2), _lib.ptr(faces), faces.element_size(),
                                                                     faces.stride(0), faces.stride(1), _lib.ptr(offsets),
                                                                     1 if mean else 0, _lib.ptr(grad)), fn)
    return grad


# ---- kaolin._C.ops.mesh: face areas and surface sampling on csrc/sample_points.hip (no reference counterpart: pure torch there) -------
def _sp_mesh(fn, vertices, faces, items):
    """Checks of the mesh arguments shared by the four operators -> (sfx, B, F, V, items, max_faces, vertex strides)"""
    torch_check(isinstance(vertices, torch.Tensor) and vertices.is_cuda, f'{fn}: vertices must be a CUDA tensor')
    sfx = _lib.dtype_suffix(vertices.dtype, fn)
    torch_check(isinstance(faces, torch.Tensor) and faces.is_cuda and faces.dim() == 2 and faces.size(1) == 3 and
                faces.dtype == torch.long and faces.device == vertices.device,
                f'{fn}: faces must be a long CUDA tensor of size (num_faces, 3) on the device of vertices')
    F = faces.size(0)
    torch_check(F >= 1, f'{fn}: no faces')
    if items is None:
        torch_check(vertices.dim() == 3 and vertices.size(2) == 3, f'{fn}: vertices must be of size (batch_size, num_vertices, 3)')
        B, V = vertices.size(0), vertices.size(1)
        strides, max_faces = vertices.stride(), F
    else:
        torch_check(vertices.dim() == 2 and vertices.size(1) == 3, f'{fn}: packed vertices must be of size (num_vertices, 3)')
        torch_check(isinstance(items, tuple) and len(items) == 2 and isinstance(items[0], torch.Tensor) and
                    items[0].dtype == torch.long and items[0].device == vertices.device and items[0].dim() == 2 and
                    items[0].size(1) == 3 and items[0].is_contiguous(),
                    f'{fn}: items must be (a contiguous long tensor of size (batch_size, 3) on the device of vertices, max_faces)')
        items, max_faces = items[0], int(items[1])
        B, V = items.size(0), vertices.size(0)
        torch_check(1 <= max_faces <= F, f'{fn}: max_faces must be in [1, num_faces]')
        strides = (0,) + tuple(vertices.stride())
    torch_check(B >= 1 and V >= 1, f'{fn}: vertices of size {tuple(vertices.shape)}: every extent must be at least 1')
    return sfx, B, F, V, items, max_faces, strides


def _sp_per_face(fn, t, name, B, F, packed, dev):
    want = (F,) if packed else (B, F)
    torch_check(isinstance(t, torch.Tensor) and t.device == dev and tuple(t.shape) == want and
                t.dtype in (torch.float32, torch.float64), f'{fn}: {name} must be a float / double tensor of size {want} on the device of vertices')


def face_areas_forward_cuda(vertices, faces, items=None):
    """vertices (B, V, 3) float / double of any strides, faces (F, 3) long of any strides -> areas (B, F); with ``items`` =
    (the device table (B, 3) of (face_begin, face_end, vertex_base) rows, the largest item's face count): packed vertices (V, 3)
    and faces (F, 3) with ids local to their item -> (F,).  The reference's expression, one rounding per operation: the bits of the
    torch expression on the CPU.  One launch, no host read.  The ids are NOT checked against V on the host (the callers do, see
    ``faces_in_range``); the kernel writes NaN for a face with an id outside the vertices."""
    fn = 'face_areas_forward_cuda'
    sfx, B, F, V, table, _, vs = _sp_mesh(fn, vertices, faces, items)
    v, f, dev = vertices.detach(), faces.detach(), vertices.device
    lib = _lib.load()
    with _lib.on_device(dev):
        areas = torch.empty((F,) if table is not None else (B, F), dtype=v.dtype, device=dev)
        _lib.check(getattr(lib, f'kamd_face_areas_{sfx}')(_lib.stream_ptr(dev), B, F, V, _lib.ptr(table), _lib.ptr(v), vs[0], vs[1], vs[2],
                                                         _lib.ptr(f), f.stride(0), f.stride(1), _lib.ptr(areas)), fn)
    return areas


def face_areas_backward_cuda(grad_areas, vertices, faces, items=None):
    """-> the gradient of the areas per face corner, contiguous (B, F, 3, 3) (packed: (F, 3, 3)), written by plain stores: the
    reference's autograd expression operation by operation (NaN at a zero-area face, from 0 * inf).  One launch; the sum per
    vertex is ``vertex_gather_forward_cuda`` in its sum mode."""
    fn = 'face_areas_backward_cuda'
    sfx, B, F, V, table, _, vs = _sp_mesh(fn, vertices, faces, items)
    v, f, dev = vertices.detach(), faces.detach(), vertices.device
    torch_check(isinstance(grad_areas, torch.Tensor) and grad_areas.dtype == v.dtype, f'{fn}: grad_areas must have the dtype of vertices')
    _sp_per_face(fn, grad_areas, 'grad_areas', B, F, table is not None, dev)
    g = grad_areas.detach()
    gs = (0, g.stride(0)) if table is not None else g.stride()
    lib = _lib.load()
    with _lib.on_device(dev):
        grad = torch.empty((F, 3, 3) if table is not None else (B, F, 3, 3), dtype=v.dtype, device=dev)
        _lib.check(getattr(lib, f'kamd_face_areas_backward_{sfx}')(_lib.stream_ptr(dev), B, F, V, _lib.ptr(table), _lib.ptr(v), vs[0],
                                                                  vs[1], vs[2], _lib.ptr(f), f.stride(0), f.stride(1), _lib.ptr(g),
                                                                  gs[0], gs[1], _lib.ptr(grad)), fn)
    return grad


def sample_cdf_cuda(areas, items=None):
    """areas (B, F) float / double (packed: (F,) with ``items``) -> cdf of the same shape in float64: per item the inclusive sums
    of its areas, widened to float64 and added in float64 in a fixed order (the same bits run after run).  One launch when the
    largest item fits one tile of the scan (2048 faces), else three; no host read."""
    fn = 'sample_cdf_cuda'
    torch_check(isinstance(areas, torch.Tensor) and areas.is_cuda and areas.dtype in (torch.float32, torch.float64),
                f'{fn}: areas must be a float / double CUDA tensor')
    dev = areas.device
    if items is None:
        torch_check(areas.dim() == 2 and areas.size(0) >= 1 and areas.size(1) >= 1, f'{fn}: areas must be of size (batch_size, num_faces)')
        B, F, table, max_faces = areas.size(0), areas.size(1), None, areas.size(1)
    else:
        table, max_faces = items[0], int(items[1])
        torch_check(areas.dim() == 1 and areas.size(0) >= 1, f'{fn}: packed areas must be of size (num_faces,)')
        torch_check(isinstance(table, torch.Tensor) and table.dtype == torch.long and table.device == dev and table.dim() == 2 and
                    table.size(0) >= 1 and table.size(1) == 3 and table.is_contiguous() and 1 <= max_faces <= areas.size(0),
                    f'{fn}: items must be (a contiguous long tensor of size (batch_size, 3) on the device of areas, max_faces)')
        B, F = table.size(0), areas.size(0)
    a = areas.detach().contiguous()
    lib = _lib.load()
    with _lib.on_device(dev):
        nbytes = lib.kamd_sample_cdf_workspace(B, max_faces)
        torch_check(nbytes > 0, f'{fn}: {B} items of {max_faces} faces are more than the scan takes')
        ws = _lib.workspace(nbytes, dev)
        cdf = torch.empty(a.shape, dtype=torch.float64, device=dev)
        _lib.check(getattr(lib, f'kamd_sample_cdf_{_lib.dtype_suffix(a.dtype, fn)}')(
            _lib.stream_ptr(dev), B, F, max_faces, _lib.ptr(table), _lib.ptr(a), _lib.ptr(cdf), _lib.ptr(ws), nbytes), fn)
    return cdf


def sample_points_forward_cuda(vertices, faces, items, cdf_or_areas, r, uv, face_features=None):
    """The deterministic part of ``sample_points``: a function of its arguments alone, bit for bit the same on every call.

    vertices (B, V, 3) float / double of any strides, faces (F, 3) long, ``items`` None (or the packed table of
    ``face_areas_forward_cuda`` with packed vertices (V, 3)); ``cdf_or_areas``: None (the areas are computed), the areas (B, F)
    float / double (packed: (F,)), or the pair (areas, cdf) of an earlier call (``sample_cdf_cuda``); r (B, N) float64 and uv
    (B, N, 2) in the dtype of vertices, N >= 1; face_features (B, F, 3, D) in the dtype of vertices, any strides (0 included), or
    None -> (points (B, N, 3), face_choices (B, N) long (packed: merged ids), features (B, N, D) or None, areas, cdf).

    Launches: areas (1, when not given) + cdf (1 or 3) + sampling (1): at most 5.  No host read, no atomics: capturable."""
    fn = 'sample_points_forward_cuda'
    sfx, B, F, V, table, max_faces, vs = _sp_mesh(fn, vertices, faces, items)
    v, f, dev = vertices.detach(), faces.detach(), vertices.device
    packed = table is not None
    torch_check(isinstance(r, torch.Tensor) and r.device == dev and r.dtype == torch.float64 and r.dim() == 2 and r.size(0) == B and
                r.size(1) >= 1, f'{fn}: r must be a double tensor of size ({B}, num_samples >= 1) on the device of vertices')
    N = r.size(1)
    torch_check(isinstance(uv, torch.Tensor) and uv.device == dev and uv.dtype == v.dtype and tuple(uv.shape) == (B, N, 2),
                f'{fn}: uv must be of size ({B}, {N}, 2) with the dtype and device of vertices')
    cdf = None
    if isinstance(cdf_or_areas, (tuple, list)):
        torch_check(len(cdf_or_areas) == 2, f'{fn}: cdf_or_areas must be None, the areas or the pair (areas, cdf)')
        areas, cdf = cdf_or_areas
    else:
        areas = cdf_or_areas
    if areas is None:
        areas = face_areas_forward_cuda(v, f, items)
    _sp_per_face(fn, areas, 'areas', B, F, packed, dev)
    areas = areas.detach().contiguous()
    if cdf is None:
        cdf = sample_cdf_cuda(areas, items)
    torch_check(isinstance(cdf, torch.Tensor) and cdf.dtype == torch.float64 and cdf.device == dev and cdf.shape == areas.shape and
                cdf.is_contiguous(), f'{fn}: cdf must be a contiguous double tensor of the size of areas')
    D, ff, fs = 0, None, (0, 0, 0, 0)
    if face_features is not None:
        torch_check(not packed, f'{fn}: face_features are not taken with packed meshes')
        torch_check(isinstance(face_features, torch.Tensor) and face_features.device == dev and face_features.dtype == v.dtype and
                    face_features.dim() == 4 and tuple(face_features.shape[:3]) == (B, F, 3) and face_features.size(3) >= 1,
                    f'{fn}: face_features must be of size ({B}, {F}, 3, feature_dim >= 1) with the dtype and device of vertices')
        ff = face_features.detach()
        D, fs = ff.size(3), ff.stride()
    rr, uu = r.detach().contiguous(), uv.detach().contiguous()
    lib = _lib.load()
    with _lib.on_device(dev):
        points = torch.empty((B, N, 3), dtype=v.dtype, device=dev)
        choices = torch.empty((B, N), dtype=torch.long, device=dev)
        features = torch.empty((B, N, D), dtype=v.dtype, device=dev) if D > 0 else None
        _lib.check(getattr(lib, f'kamd_sample_points_{sfx}')(
            _lib.stream_ptr(dev), B, F, V, N, D, _lib.ptr(table), _lib.ptr(v), vs[0], vs[1], vs[2], _lib.ptr(f), f.stride(0), f.stride(1),
            _lib.ptr(areas), areas.element_size(), _lib.ptr(cdf), _lib.ptr(rr), _lib.ptr(uu), _lib.ptr(ff), fs[0], fs[1], fs[2], fs[3],
            _lib.ptr(points), _lib.ptr(choices), _lib.ptr(features)), fn)
    return points, choices, features, areas, cdf


def sample_points_backward_cuda(grad_points, grad_features, faces, items, cdf, uv, face_choices, num_vertices, feature_dim=0):
    """-> (grad_vertices (B, V, 3) (packed: (V, 3)) or None, grad_face_features (B, F, 3, D) or None), for the cotangents that are
    not None: ONE launch that recomputes the weights from uv and adds ``w_k g`` to the three vertices and the three feature rows of
    every sample's face with float atomics, into buffers zero-filled here.  The sums vary from run to run in their last bits (the
    order of the additions is not fixed).  No host read: capturable."""
    fn = 'sample_points_backward_cuda'
    torch_check(isinstance(uv, torch.Tensor) and uv.is_cuda and uv.dim() == 3 and uv.size(2) == 2, f'{fn}: uv must be a CUDA tensor of size (B, N, 2)')
    sfx = _lib.dtype_suffix(uv.dtype, fn)
    dev, (B, N), V, D = uv.device, uv.shape[:2], int(num_vertices), int(feature_dim)
    torch_check(isinstance(faces, torch.Tensor) and faces.device == dev and faces.dim() == 2 and faces.size(1) == 3 and
                faces.dtype == torch.long and faces.size(0) >= 1, f'{fn}: faces must be a long tensor of size (num_faces >= 1, 3) on the device of uv')
    F, f = faces.size(0), faces.detach()
    table = None
    if items is not None:
        table = items[0]
        torch_check(isinstance(table, torch.Tensor) and table.dtype == torch.long and table.device == dev and table.is_contiguous() and
                    tuple(table.shape) == (B, 3), f'{fn}: items must hold a contiguous long tensor of size ({B}, 3) on the device of uv')
    torch_check(B >= 1 and N >= 1 and V >= 1 and D >= 0, f'{fn}: every extent must be at least 1')
    torch_check(isinstance(cdf, torch.Tensor) and cdf.dtype == torch.float64 and cdf.device == dev and cdf.is_contiguous() and
                tuple(cdf.shape) == ((F,) if table is not None else (B, F)), f'{fn}: cdf must be the contiguous double cdf of the forward')
    torch_check(isinstance(face_choices, torch.Tensor) and face_choices.dtype == torch.long and face_choices.device == dev and
                tuple(face_choices.shape) == (B, N), f'{fn}: face_choices must be a long tensor of size ({B}, {N}) on the device of uv')
    gp = gf = None
    if grad_points is not None:
        torch_check(isinstance(grad_points, torch.Tensor) and grad_points.dtype == uv.dtype and grad_points.device == dev and
                    tuple(grad_points.shape) == (B, N, 3), f'{fn}: grad_points must be of size ({B}, {N}, 3) like uv')
        gp = grad_points.detach().contiguous()
    if grad_features is not None:
        torch_check(table is None and D >= 1, f'{fn}: grad_features need feature_dim >= 1 and a batched mesh')
        torch_check(isinstance(grad_features, torch.Tensor) and grad_features.dtype == uv.dtype and grad_features.device == dev and
                    tuple(grad_features.shape) == (B, N, D), f'{fn}: grad_features must be of size ({B}, {N}, {D}) like uv')
        gf = grad_features.detach().contiguous()
    uu, choices = uv.detach().contiguous(), face_choices.contiguous()
    lib = _lib.load()
    with _lib.on_device(dev):
        grad_vertices = torch.zeros((V, 3) if table is not None else (B, V, 3), dtype=uv.dtype, device=dev) if gp is not None else None
        grad_ff = torch.zeros((B, F, 3, D), dtype=uv.dtype, device=dev) if gf is not None else None
        if gp is not None or gf is not None:
            _lib.check(getattr(lib, f'kamd_sample_points_backward_{sfx}')(
                _lib.stream_ptr(dev), B, F, V, N, D if gf is not None else 0, _lib.ptr(table), _lib.ptr(f), f.stride(0), f.stride(1),
                _lib.ptr(cdf), _lib.ptr(uu), _lib.ptr(choices), _lib.ptr(gp), _lib.ptr(gf),
                _lib.ptr(grad_vertices), _lib.ptr(grad_ff)), fn)
    return grad_vertices, grad_ff


# ---- kaolin._C.ops.gaussians: transform_gaussians / transform_shs on csrc/gaussian_transform.hip (no reference counterpart: pure torch
# there).  One launch per call, nothing reads back or synchronises: the operators capture into a graph.
def _gt_args(fn, named, transform, rotation_given):
    """named: [(name, tensor or None, trailing shape)]; every tensor float32 / float64 on the GPU of `transform`, N rows each
    -> (suffix, N, transform made contiguous, its stride in elements, its row stride, the tensors made contiguous)"""
    torch_check(torch.is_tensor(transform) and transform.is_cuda, f'{fn}: transform must be a CUDA tensor')
    sfx = _lib.dtype_suffix(transform.dtype, fn)
    side = 3 if rotation_given else 4
    torch_check(transform.dim() == 3 and tuple(transform.shape[1:]) == (side, side),
                f'{fn}: transform must of size {{num_gaussians or 1, {side}, {side}}}')
    given = [(name, t, tail) for name, t, tail in named if t is not None]
    torch_check(len(given) > 0, f'{fn}: nothing to transform')
    n = given[0][1].size(0) if given[0][1].dim() else -1
    out = []
    for name, t, tail in named:
        if t is None:
            out.append(None)
            continue
        torch_check(t.is_cuda and t.device == transform.device, f'{fn}: {name} must be a CUDA tensor on the device of transform')
        torch_check(t.dtype == transform.dtype, f'{fn}: expected {name} to have the scalar type of transform')
        torch_check(t.dim() == 1 + len(tail) and t.size(0) == n and all(a == b or b is None for a, b in zip(t.shape[1:], tail)),
                    f'{fn}: {name} must of size {{num_gaussians, {", ".join("S" if b is None else str(b) for b in tail)}}}')
        out.append(t.detach().contiguous())
    torch_check(transform.size(0) in (1, n), f'{fn}: transform must of size {{num_gaussians or 1, {side}, {side}}}')
    tf = transform.detach().contiguous()
    return sfx, n, tf, (side * side if tf.size(0) == n and n != 1 else 0), side, out


def _gt_degree(fn, sh):
    if sh is None:
        return 0
    degree = {1: 0, 4: 1, 9: 2, 16: 3}.get(sh.size(1))
    torch_check(degree is not None, f'{fn}: sh must hold 1, 4, 9 or 16 coefficients, got {sh.size(1)}')
    return degree


def _gt_flags(use_log_scales, use_xyzw, rotation_given):
    return (1 if use_xyzw else 0) | (2 if use_log_scales else 0) | (4 if rotation_given else 0)


def transform_gaussians_forward_cuda(positions, orientations, scales, transform, sh_coeff=None, use_log_scales=False, use_xyzw=False,
                                     rotation_given=False):
    """positions (N, 3), orientations (N, 4), scales (N, 3): all three or all None; sh_coeff (N, 1 | 4 | 9 | 16, 3) or None;
    transform (N or 1, 4, 4), or with ``rotation_given`` the rotations themselves, (N or 1, 3, 3), and no geometry
    -> (new_positions, new_orientations, new_scales, new_sh_coeff), None where the input is.  Inputs that are not contiguous are
    copied.  N = 0 launches nothing."""
    fn = 'transform_gaussians_forward_cuda'
    geometry = [positions is not None, orientations is not None, scales is not None]
    torch_check(all(geometry) or not any(geometry), f'{fn}: positions, orientations and scales are given together or not at all')
    torch_check(not (rotation_given and any(geometry)), f'{fn}: a given rotation transforms sh_coeff only')
    sfx, n, tf, stride, row, (pos, ori, scl, sh) = _gt_args(
        fn, [('positions', positions, (3,)), ('orientations', orientations, (4,)), ('scales', scales, (3,)),
             ('sh_coeff', sh_coeff, (None, 3))], transform, rotation_given)
    degree = _gt_degree(fn, sh)
    dev = tf.device
    lib = _lib.load()
    with _lib.on_device(dev):
        outs = [None if t is None else torch.empty_like(t) for t in (pos, ori, scl, sh)]
        if n > 0:
            _lib.check(getattr(lib, f'kamd_gaussian_transform_forward_{sfx}')(
                _lib.stream_ptr(dev), n, degree, _gt_flags(use_log_scales, use_xyzw, rotation_given), _lib.ptr(tf), stride, row,
                _lib.ptr(pos), _lib.ptr(ori), _lib.ptr(scl), _lib.ptr(sh), *(_lib.ptr(t) for t in outs)), fn)
    return tuple(outs)


def transform_gaussians_backward_cuda(grad_new_positions, grad_new_orientations, grad_new_scales, grad_new_sh_coeff, orientations,
                                      transform, use_log_scales=False, use_xyzw=False, rotation_given=False,
                                      need=(True, True, True, True)):
    """The gradients of the forward's outputs (any of them None) -> (grad_positions, grad_orientations, grad_scales, grad_sh_coeff):
    entry k is computed when ``need[k]`` and its output's gradient is given, else None.  ``orientations`` is the forward's input
    (needed for grad_orientations only).  No gradient with respect to ``transform``."""
    fn = 'transform_gaussians_backward_cuda'
    grads = [grad_new_positions, grad_new_orientations, grad_new_scales, grad_new_sh_coeff]
    grads = [g if k else None for g, k in zip(grads, need)]
    if all(g is None for g in grads):
        return (None, None, None, None)
    torch_check(not (rotation_given and any(g is not None for g in grads[:3])), f'{fn}: a given rotation transforms sh_coeff only')
    torch_check(grads[1] is None or orientations is not None, f'{fn}: grad_orientations needs the orientations')
    sfx, n, tf, stride, row, (gp, go, gs, gsh, ori) = _gt_args(
        fn, [('grad_new_positions', grads[0], (3,)), ('grad_new_orientations', grads[1], (4,)), ('grad_new_scales', grads[2], (3,)),
             ('grad_new_sh_coeff', grads[3], (None, 3)), ('orientations', orientations if grads[1] is not None else None, (4,))],
        transform, rotation_given)
    degree = _gt_degree(fn, gsh)
    dev = tf.device
    lib = _lib.load()
    with _lib.on_device(dev):
        outs = [None if t is None else torch.empty_like(t) for t in (gp, go, gs, gsh)]
        if n > 0:
            _lib.check(getattr(lib, f'kamd_gaussian_transform_backward_{sfx}')(
                _lib.stream_ptr(dev), n, degree, _gt_flags(use_log_scales, use_xyzw, rotation_given), _lib.ptr(tf), stride, row,
                _lib.ptr(ori), _lib.ptr(gp), _lib.ptr(go), _lib.ptr(gs), _lib.ptr(gsh), *(_lib.ptr(t) for t in outs)), fn)
    return tuple(outs)


# the reference groups these operators in sub-modules: kaolin._C.ops.mesh / kaolin._C.ops.conversions (bindings.cpp)
import types as _types  # noqa: E402
gaussians = _types.SimpleNamespace(transform_gaussians_forward_cuda=transform_gaussians_forward_cuda,
                                   transform_gaussians_backward_cuda=transform_gaussians_backward_cuda)
mesh = _types.SimpleNamespace(unbatched_mesh_intersection_cuda=unbatched_mesh_intersection_cuda,
                              vertex_corners_cuda=vertex_corners_cuda,
                              vertex_gather_forward_cuda=vertex_gather_forward_cuda,
                              vertex_gather_backward_cuda=vertex_gather_backward_cuda,
                              face_areas_forward_cuda=face_areas_forward_cuda,
                              face_areas_backward_cuda=face_areas_backward_cuda,
                              sample_cdf_cuda=sample_cdf_cuda,
                              sample_points_forward_cuda=sample_points_forward_cuda,
                              sample_points_backward_cuda=sample_points_backward_cuda,
                              subdivide_trianglemesh_cuda=subdivide_trianglemesh_cuda,
                              trianglemesh_loop_forward_cuda=trianglemesh_loop_forward_cuda,
                              trianglemesh_loop_backward_cuda=trianglemesh_loop_backward_cuda,
                              subdivide_tetmesh_cuda=subdivide_tetmesh_cuda,
                              tetmesh_midpoints_forward_cuda=tetmesh_midpoints_forward_cuda,
                              tetmesh_midpoints_backward_cuda=tetmesh_midpoints_backward_cuda)
conversions = _types.SimpleNamespace(mesh_to_spc_cuda=mesh_to_spc_cuda, marching_tetrahedra_cuda=marching_tetrahedra_cuda,
                                     marching_tetrahedra_backward_cuda=marching_tetrahedra_backward_cuda,
                                     voxelgrids_to_cubic_meshes_cuda=voxelgrids_to_cubic_meshes_cuda,
                                     voxelgrids_to_trianglemeshes_cuda=voxelgrids_to_trianglemeshes_cuda,
                                     unbatched_mcube_forward_cuda=unbatched_mcube_forward_cuda,
                                     mcube_forward_cuda=mcube_forward_cuda, mcube_backward_cuda=mcube_backward_cuda,
                                     flexicubes_forward_cuda=flexicubes_forward_cuda,
                                     flexicubes_backward_cuda=flexicubes_backward_cuda,
                                     gs_to_spc_cuda=gs_to_spc_cuda, integrate_gs_cuda=integrate_gs_cuda,
                                     pointcloud_to_spc_cuda=pointcloud_to_spc_cuda,
                                     pointclouds_to_voxelgrids_cuda=pointclouds_to_voxelgrids_cuda)
spc = _types.SimpleNamespace(points_to_morton_cuda=points_to_morton_cuda, morton_to_points_cuda=morton_to_points_cuda,
                             points_to_corners_cuda=points_to_corners_cuda, points_to_octree=points_to_octree,
                             morton_to_octree=morton_to_octree, scan_octrees_cuda=scan_octrees_cuda,
                             generate_points_cuda=generate_points_cuda, query_cuda=query_cuda,
                             query_multiscale_cuda=query_multiscale_cuda, to_dense_forward=to_dense_forward,
                             to_dense_backward=to_dense_backward, make_dual_cuda=make_dual_cuda,
                             make_trinkets_cuda=make_trinkets_cuda, coords_to_trilinear_cuda=coords_to_trilinear_cuda,
                             interpolate_trilinear_cuda=interpolate_trilinear_cuda,
                             interpolate_trilinear_backward_feats_cuda=interpolate_trilinear_backward_feats_cuda,
                             interpolate_trilinear_backward_coords_cuda=interpolate_trilinear_backward_coords_cuda,
                             Conv3d_forward=Conv3d_forward, Conv3d_backward=Conv3d_backward,
                             ConvTranspose3d_forward=ConvTranspose3d_forward, ConvTranspose3d_backward=ConvTranspose3d_backward,
                             build_mip2d=build_mip2d, oracleB=oracleB, oracleB_final=oracleB_final, colorsB_final=colorsB_final,
                             inclusive_sum=inclusive_sum, subdivide=subdivide, compactify=compactify,
                             process_final_voxels=process_final_voxels, compactify_nodes=compactify_nodes,
                             merge_empty=merge_empty, bq_merge=bq_merge, query_cuda_empty=query_cuda_empty,
                             bf_cells_cuda=bf_cells_cuda)
