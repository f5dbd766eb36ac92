"""ops.pointcloud on the CPU: the torch path of farthest_point_sampling against the rule restated in numpy (the oracle below, which
tests/test_fps_gpu.py shares), the reference's assertions, the workspace arithmetic, and center_points against float64.

Lattice inputs (coordinates k / 1024): float64 sums of them are exact in any order, so the centre and every index have one right
answer, and squared distances are multiples of 2^-20, so exact ties occur."""
import numpy as np
import pytest
import torch

from kaolin_amd import _lib
from kaolin_amd.ops import pointcloud as pc


def lattice(B, N, seed=0):
    return torch.randint(0, 1024, (B, N, 3), generator=torch.Generator().manual_seed(seed)) / 1024


def special(N, kind):
    """One lattice cloud with points[1:N // 2] made NaN, inf or copies of points[0]; 'overflow': every coordinate scaled to
    +-3e19, where d between finite points overflows (the float64 sums stay exact: 24-bit values within 2^10 of each other)."""
    p = lattice(1, N, seed=N)
    if kind == 'overflow':
        return (p * 2 - 1) * 3e19
    p[0, 1:N // 2] = {'nan': float('nan'), 'inf': float('inf'), 'dup': p[0, 0]}[kind]
    return p


def fps_oracle(points, k, first=None, ties=None):
    """The rule for one (N, 3) cloud in numpy float32, one ufunc per operation.  `first`: start from this index instead of the
    centre's; `ties`: a list that receives True for every arg-max over a non-negative D that two points share."""
    p = np.asarray(points, dtype=np.float32)

    def dist(q):
        sq = (p - q) * (p - q)
        return (sq[:, 0] + sq[:, 1]) + sq[:, 2]

    with np.errstate(all='ignore'):
        finite = np.isfinite(p).all(axis=1)
        c = (p[finite].astype(np.float64).sum(axis=0) / finite.sum()).astype(np.float32)
        d = dist(c if np.isfinite(c).all() else np.zeros(3, np.float32))
        D = np.where(np.isfinite(d), d, np.float32(-1))
        out = []
        for r in range(k):
            s = int(np.argmax(D)) if (r or first is None) else first    # np.argmax: the first of the largest
            if ties is not None and D[s] >= 0:
                ties.append(int((D == D[s]).sum()) > 1)
            out.append(s)
            d = dist(p[s])
            D = np.where(np.isfinite(d), np.minimum(D, d) if r else d, D if r else np.float32(-1))
            D[s] = -2
    return out


def oracle_batch(points, k, ties=None):
    return torch.tensor([fps_oracle(c.numpy(), k, ties=ties) for c in points], dtype=torch.int64).reshape(len(points), k)


@pytest.mark.parametrize('N,k,B', [(1, 1, 1), (2, 2, 1), (63, 63, 1), (65, 65, 1), (1025, 300, 1), (3000, 32, 3), (3000, 0, 1)])
def test_torch_path_lattice(N, k, B):
    points = lattice(B, N, seed=N)
    out = pc.farthest_point_sampling(points, k)
    assert out.dtype == torch.int64 and out.shape == (B, k)
    assert torch.equal(out, oracle_batch(points, k))


@pytest.mark.parametrize('N,k', [(20, 15), (3000, 32)])
@pytest.mark.parametrize('kind', ['nan', 'inf', 'dup', 'overflow'])
def test_torch_path_special_values(N, k, kind):
    points = special(N, kind)
    out = pc.farthest_point_sampling(points, k)
    assert torch.equal(out, oracle_batch(points, k))
    assert len(set(out[0].tolist())) == k
    if k == 32 and kind in ('nan', 'inf'):
        assert torch.isfinite(points[0, out[0]]).all()


def test_lattice_meets_ties():
    ties = []
    oracle_batch(lattice(1, 1025, seed=1025), 300, ties=ties)
    oracle_batch(lattice(3, 3000, seed=3000), 32, ties=ties)
    assert any(ties)


def test_assertions():
    with pytest.raises(AssertionError, match='unexpected shape'):
        pc.farthest_point_sampling(torch.zeros(10, 3), 2)
    with pytest.raises(AssertionError, match='dtype float32'):
        pc.farthest_point_sampling(torch.zeros(1, 10, 3, dtype=torch.float64), 2)
    for k in (-1, 11):
        with pytest.raises(AssertionError, match='k.*<=.*num_points'):
            pc.farthest_point_sampling(torch.zeros(1, 10, 3), k)


def test_workspace():
    lib = _lib.load()
    L, ws = lib.kamd_fps_block_limit(), lib.kamd_fps_workspace
    assert L >= 1024 and ws(1, L, 64, 0) == 0 and ws(3, 1, 1, 0) == 0 and ws(1, L, 64, 1) == 0
    assert 0 < ws(1, L + 1, 64, 0) < ws(1, 4 * L, 64, 0) < ws(2, 4 * L, 64, 0)
    assert ws(1, 65, 65, 2) > 0 and ws(0, 65, 65, 2) == 0 and ws(1, 65, 0, 2) == 0


@pytest.mark.parametrize('normalize', [False, True])
def test_center_points(normalize):
    points = torch.rand(3, 50, 3, generator=torch.Generator().manual_seed(5)) * torch.tensor([1., 3., 0.5]) + 2
    points[2] = points[2, 0]                                    # identical points: the eps clip
    p = points.double()
    lo, hi = p.min(dim=1, keepdim=True)[0], p.max(dim=1, keepdim=True)[0]
    expected = p - (lo + hi) / 2
    if normalize:
        expected = expected / (hi - lo).max(dim=-1, keepdim=True)[0].clip(min=1e-6)
    out = pc.center_points(points, normalize=normalize)
    assert out.dtype == points.dtype and torch.allclose(out.double(), expected, rtol=1e-6, atol=1e-6)
    assert torch.equal(out[2], torch.zeros(50, 3))
