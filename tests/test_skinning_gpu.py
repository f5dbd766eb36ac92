"""SimplicitsMLP on the GPU (csrc/skinning_mlp.hip, float32) against the same module in float64 on the CPU (torch forward mode),
per element, within a running float32 error bound carried through the float64 reference: no fixed tolerance.

u = 2^-24, gamma_n = n u / (1 - n u); a layer of fan-in K with value input a +- e_a and tangent input T +- e_T gives
    e_y = gamma_{K+1} (|W||a| + |b|) + |W| e_a          e_s = gamma_K |W||T| + |W| e_T
and the ELU (1-Lipschitz, like its derivative d = elu'(y) <= 1, also through the kink) gives
    e_a' = e_y + c u |a'|                               e_T' = d e_s + |s| (e_y + c u d) + u |T'|
The inputs start at e_a = 2 u |xn| (a subtraction and a division) and e_s = u |s| (W0 / extent, one division).  c = C_ULP is twice
the largest error, in ulps, of the device's expm1f and expf against float64 on [-30, 0] (tools/time_skinning.py, DESIGN.md: no
table of the device library's bounds is at hand).  The bound grows with the product of the layers' |W| row sums: measured on the
MI355X the worst share of it used is 0.060 (W = 16, L = 0), and below 0.001 at L = 6, where it only rules out a gross error.
Every figure is printed before it is asserted (pytest -s)."""
import copy
import functools

import pytest
import torch

from kaolin_amd import _C
from kaolin_amd.physics import simplicits

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
C_ULP = 2 * 0.8493       # measured on the MI355X: expm1f 0.8493 ulp, expf 0.8260 ulp (profiles/skinning_time.jsonl)
BB_MIN, BB_MAX = (-1.0, 0.5, 2.0), (3.0, 1.0, 2.25)
GROUPS = _C.physics.skinning_max_groups()
SHAPES = [(N, 64, 6, 32) for N in (1, 15, 16, 17, 63, 64, 65)] + [(64 * GROUPS + 1, 16, 1, 4)]   # the last: a workgroup's second tile
SHAPES += [(65, W, L, 8) for W in (16, 48, 128) for L in (0, 1)]
SHAPES += [(65, 64, 2, H) for H in (2, 16, 17, 18, 33, 128)]        # H - 1: padded, full and just-over blocks of 16 rows


@functools.lru_cache(maxsize=None)
def case(N, W, L, H):
    """(the module on the GPU, pts on the GPU, float64 weights, Jacobian and their bounds); parameters: the default init times 3"""
    torch.manual_seed(1000 * W + 10 * H + L)
    mod = simplicits.SimplicitsMLP(3, W, H, L, bb_min=BB_MIN, bb_max=BB_MAX).requires_grad_(False)
    for p in mod.parameters():
        p.mul_(3)
    lo, hi = mod.bb_min, mod.bb_max
    pts = (lo + (hi - lo) * torch.rand(N, 3)).clamp(lo, hi)
    ref, x = copy.deepcopy(mod).double(), pts.double()       # float32 parameters cast exactly
    want_w, want_j = ref.compute_weights_and_dwdx(x)
    gam = lambda n: n * U / (1 - n * U)
    lin, ext = ref._linears(), (hi - lo).double()
    a = (x - lo.double()) / ext
    e_a = 2 * U * a.abs()
    s = (lin[0].weight / ext).T[None].expand(N, 3, W)
    e_s = U * s.abs()
    y = a @ lin[0].weight.T + lin[0].bias
    e_y = gam(4) * (a.abs() @ lin[0].weight.abs().T + lin[0].bias.abs()) + e_a @ lin[0].weight.abs().T
    for m in lin[1:]:
        assert 0.2 <= (y < 0).double().mean() <= 0.8, 'both ELU branches must be in play at every hidden layer'
        d, a, Wa, K = torch.exp(y.clamp(max=0)), torch.nn.functional.elu(y), m.weight.abs().T, m.in_features
        e_a = e_y + C_ULP * U * a.abs()
        T = d[:, None] * s
        e_T = d[:, None] * e_s + s.abs() * (e_y + C_ULP * U * d)[:, None] + U * T.abs()
        y, s = a @ m.weight.T + m.bias, T @ m.weight.T
        e_y = gam(K + 1) * (a.abs() @ Wa + m.bias.abs()) + e_a @ Wa
        e_s = gam(K) * (T.abs() @ Wa) + e_T @ Wa
    for mine, theirs in ((y, want_w[:, :-1]), (s.transpose(1, 2), want_j[:, :-1])):      # the recurrence walked the module's own path
        assert (mine - theirs).abs().max() <= 1e-12 * theirs.abs().max()
    zero = torch.zeros(N, 1, dtype=torch.float64)
    return mod.cuda(), pts.cuda(), want_w, want_j, torch.cat([e_y, zero], 1), torch.cat([e_s.transpose(1, 2), zero[:, :, None].expand(N, 1, 3)], 1)


@pytest.mark.parametrize('N,W,L,H', SHAPES)
def test_weights_and_jacobian_within_the_bound(N, W, L, H, monkeypatch):
    mod, pts, want_w, want_j, bound_w, bound_j = case(N, W, L, H)
    calls, kernel = [], _C.physics.skinning_mlp_cuda
    monkeypatch.setattr(_C.physics, 'skinning_mlp_cuda', lambda *args: calls.append(1) or kernel(*args))
    w, j = mod.compute_weights_and_dwdx(pts)
    assert w.shape == (N, H) and j.shape == (N, H, 3) and w.dtype == j.dtype == torch.float32 and torch.isfinite(j).all()
    err_w, err_j = (w.double().cpu() - want_w).abs(), (j.double().cpu() - want_j).abs()
    share = max((err_w[:, :-1] / bound_w[:, :-1]).max().item(), (err_j[:, :-1] / bound_j[:, :-1]).max().item())
    print(f'skinning N={N} W={W} L={L} H={H}: worst share of the bound {share:.3f}')
    assert (err_w <= bound_w).all() and (err_j <= bound_j).all(), share
    again = mod.compute_weights_and_dwdx(pts)
    assert torch.equal(again[0], w) and torch.equal(again[1], j)
    assert torch.equal(mod.compute_skinning_weights(pts), w) and torch.equal(mod.compute_dwdx(pts), j)
    assert len(calls) == 4                                   # every call above took the HIP path
    with pytest.raises(ValueError):
        mod.compute_weights_and_dwdx(pts.T)
    w2, _ = mod.compute_weights_and_dwdx(pts.T.contiguous().T)   # the same values at other strides
    assert torch.equal(w2, w)


def test_gradients_take_the_torch_path(monkeypatch):
    mod, pts = case(17, 64, 6, 32)[:2]
    mod = copy.deepcopy(mod).requires_grad_(True)
    monkeypatch.setattr(_C.physics, 'skinning_mlp_cuda', lambda *args: pytest.fail('no autograd through the kernel'))
    w, j = mod.compute_weights_and_dwdx(pts)
    (w.sum() + j.sum()).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in mod.parameters())


def test_captured_graph_replays_on_new_points():
    mod, pts = case(65, 64, 6, 32)[:2]
    other = case(65, 64, 2, 33)[1]
    eager = [mod.compute_weights_and_dwdx(x) for x in (pts, other)]
    buf = pts.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        w, j = mod.compute_weights_and_dwdx(buf)
    for x, (want_w, want_j) in ((other, eager[1]), (pts, eager[0]), (other, eager[1])):
        buf.copy_(x)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(w, want_w) and torch.equal(j, want_j)


def test_outputs_feed_the_reduced_terms():
    """z = 0 is the rest state, F = I at every point: no energy, and a symmetric finite K; the layouts of the two kernels agree"""
    N, H = 65, 8
    mod, pts = case(N, 64, 6, H)[:2]
    w, j = mod.compute_weights_and_dwdx(pts)
    mu, lam, vol = (torch.full((N,), v, device='cuda') for v in (1.5, 3.0, 0.1))
    E, g, K = simplicits.reduced_neohookean_terms(torch.zeros(12 * H, device='cuda'), pts, w, j, mu, lam, vol)
    F = simplicits.get_defo_grad(torch.zeros(12 * H, device='cuda'), w, j, pts)
    assert torch.equal(F, torch.eye(3, device='cuda').expand(N, 3, 3))
    assert E.abs().item() <= U * (vol * (mu + lam)).sum().item()
    assert K.shape == (12 * H, 12 * H) and torch.isfinite(K).all() and torch.equal(K, K.T)
