"""kaolin_amd.physics.simplicits: SkinningModule, SimplicitsMLP and linear blend skinning, the torch path on the CPU."""
import pytest
import torch

import kaolin_amd
from kaolin_amd.physics import simplicits

BB_MIN, BB_MAX = (-1.0, 0.5, 2.0), (3.0, 1.0, 2.25)


def points(N, dtype=torch.float64):
    lo, hi = torch.tensor(BB_MIN, dtype=dtype), torch.tensor(BB_MAX, dtype=dtype)
    return lo + (hi - lo) * torch.rand(N, 3, dtype=dtype, generator=torch.Generator().manual_seed(N))


def test_structure_and_state_dict():
    W, L, H = 32, 2, 5
    mod = simplicits.SimplicitsMLP(3, W, H, L, bb_min=BB_MIN, bb_max=BB_MAX)
    kinds = [type(m) for m in mod.linear_elu_stack]
    assert kinds == [torch.nn.Linear, torch.nn.ELU] * (L + 1) + [torch.nn.Linear]
    shapes = {'bb_min': (3,), 'bb_max': (3,),
              'linear_elu_stack.0.weight': (W, 3), 'linear_elu_stack.0.bias': (W,),
              'linear_elu_stack.2.weight': (W, W), 'linear_elu_stack.2.bias': (W,),
              'linear_elu_stack.4.weight': (W, W), 'linear_elu_stack.4.bias': (W,),
              'linear_elu_stack.6.weight': (H - 1, W), 'linear_elu_stack.6.bias': (H - 1,)}
    assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == shapes
    made = {k: torch.full(s, 0.01 * i) for i, (k, s) in enumerate(shapes.items())}
    made['bb_min'], made['bb_max'] = torch.tensor(BB_MIN), torch.tensor(BB_MAX)
    mod.load_state_dict(made)
    assert torch.equal(mod.linear_elu_stack[6].weight, made['linear_elu_stack.6.weight'])
    with pytest.raises(AssertionError):
        simplicits.SkinningModule(bb_min=[0, 0, 0], bb_max=[1, 0, 1])
    kaolin_amd.install_as_kaolin()
    import kaolin
    assert kaolin.physics.simplicits.SimplicitsMLP is simplicits.SimplicitsMLP


@pytest.mark.parametrize('W,L,H', [(16, 0, 2), (32, 2, 5)])
def test_forward_mode_jacobian_equals_jacrev(W, L, H):
    torch.manual_seed(W)
    mod = simplicits.SimplicitsMLP(3, W, H, L, bb_min=BB_MIN, bb_max=BB_MAX).double()
    pts = points(7)
    w, j = mod.compute_weights_and_dwdx(pts)
    assert w.shape == (7, H) and j.shape == (7, H, 3)
    assert (w[:, -1] == 1).all() and (j[:, -1] == 0).all()
    assert torch.equal(w, mod.compute_skinning_weights(pts)) and torch.equal(j, mod.compute_dwdx(pts))
    assert torch.equal(w[:, :-1], mod((pts - mod.bb_min) / (mod.bb_max - mod.bb_min)))      # the non-unit box is in play
    want = simplicits.SkinningModule.compute_dwdx(mod, pts)                                # jacrev under vmap
    assert want.abs().max() > 1e-3 and (j - want).abs().max() <= 1e-12 * want.abs().max()
    with pytest.raises(ValueError):
        mod.compute_weights_and_dwdx(pts[:, :2])


def test_gradients_reach_parameters_and_points():
    mod = simplicits.SimplicitsMLP(3, 16, 4, 1)
    pts = points(5, torch.float32).requires_grad_(True)
    w, j = mod.compute_weights_and_dwdx(pts)
    (w.sum() + j.square().sum()).backward()
    assert pts.grad is not None and all(p.grad is not None for p in mod.parameters())


def test_from_function_takes_jacrev():
    A = torch.tensor([[1.0, 2.0, 3.0], [0.0, -1.0, 0.5]], dtype=torch.float64)
    mod = simplicits.SkinningModule.from_function(lambda x: torch.sin(x @ A.T), bb_min=[0.0, 0.0, 0.0], bb_max=[2.0, 2.0, 2.0]).double()
    pts = points(4)
    w, j = mod.compute_weights_and_dwdx(pts)
    assert w.shape == (4, 3) and j.shape == (4, 3, 3) and (w[:, -1] == 1).all() and (j[:, -1] == 0).all()
    assert torch.allclose(j[:, :2], torch.cos(pts / 2 @ A.T)[:, :, None] * A / 2, rtol=1e-12, atol=0)
    mod.grad = lambda x: (torch.cos(x @ A.T)[:, :, None] * A)          # the hook, on normalised points
    assert torch.allclose(mod.compute_dwdx(pts), j, rtol=1e-12, atol=1e-15)


def test_standard_lbs_against_a_loop():
    gen = torch.Generator().manual_seed(3)
    N, B, H = 5, 2, 3
    x0, tfms, w = (torch.randn(*s, dtype=torch.float64, generator=gen) for s in ((N, 3), (B, H, 3, 4), (N, H)))
    out = simplicits.standard_lbs(x0, tfms, w)
    assert out.shape == (N, B, 1, 3)
    for n in range(N):
        for b in range(B):
            want = x0[n] + sum(w[n, h] * (tfms[b, h] @ torch.cat([x0[n], x0.new_ones(1)])) for h in range(H))
            assert torch.allclose(out[n, b, 0], want, rtol=1e-13, atol=1e-15)
    assert torch.equal(simplicits.weight_function_lbs(x0, tfms, lambda x: w), out)
