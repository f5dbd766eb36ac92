"""Reads tests/golden/cubic_meshes.npz (the reference's outputs recorded by golden/make_golden_cubic_meshes.py) for the CPU and
GPU tests of kaolin.ops.conversions.voxelgrids_to_cubic_meshes, and holds the checks the two share.  Loaded once; the tensors
are shared and never modified."""
import functools
import os

import numpy as np
import torch

from conftest import GOLDEN_DIR


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(GOLDEN_DIR, 'cubic_meshes.npz')) as f:
        return {k: f[k] for k in f.files}


CASES = tuple(str(s) for s in golden()['cases'])
BINARY_CASES = tuple(c for c in CASES if c != 'values')


@functools.lru_cache(maxsize=None)
def grid(name):
    """The input of a case on the CPU: torch.bool for the bit-packed ones, float32 for `values`."""
    g = golden()
    if f'{name}_in' in g:
        return torch.from_numpy(g[f'{name}_in'])
    shape = tuple(int(s) for s in g[f'{name}_in_shape'])
    n = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(g[f'{name}_in_bits'])[:n].reshape(shape).astype(bool))


@functools.lru_cache(maxsize=None)
def expected(name, is_trimesh):
    """(verts, faces): two lists over the items, float32 (V, 3) and int64 (2 N, 3) or (N, 4), as the reference returns them."""
    g = golden()
    kind = 'tri' if is_trimesh else 'quad'
    n = grid(name).shape[0]
    return ([torch.from_numpy(g[f'{name}_verts_{b}'].astype(np.float32)) for b in range(n)],
            [torch.from_numpy(g[f'{name}_{kind}_{b}'].astype(np.int64)) for b in range(n)])


def assert_same_meshes(got, want, device=None):
    """Bitwise: the same number of items, shapes, dtypes (float32 / int64) and values; `device`: where the results must live."""
    assert isinstance(got[0], list) and isinstance(got[1], list) and len(got[0]) == len(got[1]) == len(want[0])
    for b, (v, f, wv, wf) in enumerate(zip(got[0], got[1], want[0], want[1])):
        assert v.dtype == torch.float32 and f.dtype == torch.int64, (b, v.dtype, f.dtype)
        assert not v.requires_grad and not f.requires_grad
        if device is not None:
            assert v.device == torch.device(device) and f.device == torch.device(device)
        assert v.shape == wv.shape and f.shape == wf.shape, (b, v.shape, wv.shape, f.shape, wf.shape)
        assert torch.equal(v.cpu(), wv.cpu()) and torch.equal(f.cpu(), wf.cpu()), b


def exposed_faces(binary):
    """The number of voxel faces of a bool (X, Y, Z) grid between an occupied voxel and an empty one or the outside, by shifted
    comparisons (independent of the lattice formulation under test)."""
    g = binary.bool()
    n = 0
    for d in range(3):
        size = g.shape[d]
        n += int(g.select(d, 0).sum()) + int(g.select(d, size - 1).sum())
        if size > 1:
            n += int((g.narrow(d, 0, size - 1) != g.narrow(d, 1, size - 1)).sum())
    return n


def signed_volume(verts, tris):
    """float64 signed volume of a closed triangle mesh, sum of a . (b x c) / 6: exact for lattice meshes of these sizes (every
    product and every partial sum is an integer far below 2^53)."""
    a, b, c = verts.double()[tris].unbind(1)
    return float((a * torch.cross(b, c, dim=1)).sum() / 6)


def check_binary_invariants(binary, verts, quads, tris):
    """binary: bool (X, Y, Z) on any device; the item's outputs in both modes."""
    assert quads.shape[0] == exposed_faces(binary)
    assert tris.shape == (2 * quads.shape[0], 3)
    # every quad is a unit lattice square: consecutive corners one unit apart along one axis, all four in one plane
    c = verts[quads]                                                # (N, 4, 3)
    edges = c.roll(-1, 1) - c
    assert torch.equal(edges.abs().sum(2), torch.ones_like(edges[..., 0]))
    assert torch.equal(edges.sum(1), torch.zeros_like(edges[:, 0]))
    extent = c.amax(1) - c.amin(1)
    assert torch.equal(extent.sort(1).values, torch.tensor([0., 1., 1.], device=verts.device).expand_as(extent))
    # every vertex is referenced, ids are in range
    assert torch.equal(torch.unique(quads), torch.arange(verts.shape[0], device=verts.device))
    assert torch.equal(torch.unique(tris), torch.arange(verts.shape[0], device=verts.device))
    assert signed_volume(verts, tris) == float(binary.sum())
