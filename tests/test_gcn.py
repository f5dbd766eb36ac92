"""kaolin_amd.ops.gcn against plain float64 on the CPU, per element, at the group-width, row-length and stride edges of csrc/gcn.hip.

The bound of a sum: the kernel adds deg_i products sequentially, one rounded multiply and one rounded add each, so
|got - ref| <= (deg_i + 3) eps T_i with T_i = sum_e |val_e x_e| (the dense expression on absolute values).  test_graph_conv's
docstring extends it, per row and per column, to the normalised layer and its gradients.
"""
import copy

import pytest
import torch

from kaolin_amd.ops import gcn

# the degrees 0 (an empty row), 1, G - 1, G, G + 1 for the group widths 4, 8, 16 and 64 of the shapes below, and a hub of all 150
_DEGREES = [0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 150]
# (B, P): C = B P columns -> G = 1, 4, 8, 64, 16 (vec), 64 + chunks, 64 (vec, C = 132), 64 + chunks (vec)
_SHAPES = [(1, 1), (1, 3), (2, 3), (1, 63), (1, 64), (1, 65), (3, 44), (1, 260)]
# every shape on the coalesced adjacency; strided operands and the uncoalesced adjacency at a scalar and a vector shape
_CASES = [(B, P, 'plain') for B, P in _SHAPES] + \
    [(B, P, layout) for layout in ('transposed', 'expanded', 'duplicates') for B, P in ((2, 3), (3, 44))] + [(1, 260, 'duplicates')]


def _adjacency(M, N, dtype, duplicates=False, seed=0):
    """A sparse (M, N) CPU matrix with positive values: the rows of _DEGREES first, then degrees 1 .. 9; with ``duplicates`` the
    entries are in random order, some twice, and the tensor is not coalesced"""
    gen = torch.Generator().manual_seed(seed)
    degrees = _DEGREES + torch.randint(1, 10, (M - len(_DEGREES),), generator=gen).tolist()
    rows = torch.cat([torch.full((d,), r) for r, d in enumerate(degrees)])
    cols = torch.cat([torch.randperm(N, generator=gen)[:d] for d in degrees])
    if duplicates:
        order = torch.randperm(rows.numel() + 40, generator=gen) % rows.numel()
        rows, cols = rows[order], cols[order]
    values = torch.rand(rows.numel(), generator=gen).to(dtype) + 0.5
    adj = torch.sparse_coo_tensor(torch.stack([rows, cols]), values, (M, N))
    return adj if duplicates else adj.coalesce()


def _bound(adj, dtype, T):
    """(M, 1) * (B, M, P): the docstring's bound, deg_i counting every entry of row i"""
    return (torch.bincount(adj._indices()[0], minlength=adj.shape[0]) + 3).double()[:, None] * torch.finfo(dtype).eps * T


def _assert_within(got, ref, bound):
    got, nan = got.detach().cpu().double(), ref.isnan()
    assert torch.equal(got.isnan(), nan)
    excess = ((got - ref).abs() - bound)[~nan]
    assert (excess <= 0).all(), f'largest excess over the bound {excess.max().item():.3e}'


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('B,P,layout', _CASES)
def test_sparse_bmm(B, P, layout, dtype):
    M, N = 201, 150
    adj = _adjacency(M, N, dtype, duplicates=layout == 'duplicates')
    gen = torch.Generator().manual_seed(B * 1000 + P)
    if layout == 'transposed':
        x = torch.randn(B, P, N, generator=gen).to(dtype).cuda().transpose(1, 2)
    elif layout == 'expanded':
        x = torch.randn(1, N, P, generator=gen).to(dtype).cuda().expand(B, N, P)
    else:
        x = torch.randn(B, N, P, generator=gen).to(dtype).cuda()
    x.requires_grad_()
    g = torch.randn(B, M, P, generator=gen).to(dtype)
    out = gcn.sparse_bmm(adj.cuda(), x)
    grad, = torch.autograd.grad(out, x, g.cuda())
    A, x64 = adj.to_dense().double(), x.detach().cpu().double()
    _assert_within(out, A @ x64, _bound(adj, dtype, A.abs() @ x64.abs()))
    _assert_within(grad, A.t() @ g.double(), _bound(adj.t(), dtype, A.t().abs() @ g.double().abs()))


def _layer64(layer, adj, h, normalize):
    """The reference layer restated in float64 on the CPU (sparse, so that an empty row's 0 / 0 stays in its own row)"""
    feat = torch.nn.functional.linear(h, layer.linear.weight, layer.linear.bias)
    out = torch.stack([torch.sparse.mm(adj, f) for f in feat])
    if normalize:
        out = out / torch.sparse.mm(adj, torch.ones(adj.shape[1], 1, dtype=torch.float64))
    if layer.self_layer:
        out = out + torch.nn.functional.linear(h, layer.linear_self.weight, layer.linear_self.bias)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('normalize', [True, False])
@pytest.mark.parametrize('self_layer', [True, False])
@pytest.mark.parametrize('O', [7, 12, 35, 132])   # C = 2 O columns: scalar, G = 16 | vec, G = 8 | scalar + chunks | vec + chunks
def test_graph_conv(O, self_layer, normalize, bias, dtype):
    """Output and gradients are sums of products of the inputs; to first order |got - ref| <= eps sum_terms n_term |term|, n_term
    the roundings the term passes.  With T = the same expression evaluated on the absolute values of its inputs (adj is positive:
    its row sums do not cancel), deg_i the entries of row i and cdeg_j those of column j:
      * output, row i: the row's sum with its multiplies (deg_i + 3, the bound of a sum); normalised, the row sum that divides it
        carries the same bound (numerator and denominator combine to first order: twice); the GEMM in front of the kernel (K + 2)
        and the self term's addition: n_i = (2 | 1) (deg_i + 3) + K + 4, the same for the pre-normalised adj;
      * input gradient, column j: the column's sum (cdeg_j + 3, division and multiply included) and the GEMM over O behind it:
        n_j = cdeg_j + O + 6; normalised, a term through row r also carries norm_r's deg_r + 3 roundings: Tw, the expression
        evaluated on |g| scaled by deg_r + 3 per row, is added (it counts the self term's branch too: slack of deg_j + 3 there);
      * parameter gradients: a reduction over the B N rows of terms that are column sums: n = B N + max cdeg + 6, plus Tw."""
    B, N, K = 2, 150, 5
    adj = _adjacency(N, N, dtype)
    deg, cdeg = (torch.bincount(adj._indices()[d], minlength=N).double() for d in (0, 1))
    torch.manual_seed(7)
    layer = gcn.GraphConv(K, O, self_layer=self_layer, bias=bias).to(dtype)
    h, g = torch.randn(B, N, K, dtype=dtype), torch.randn(B, N, O, dtype=dtype)

    def run(layer_, forward, h_, g_):
        h_ = h_.clone().requires_grad_()
        out = forward(layer_, h_)
        return [out] + list(torch.autograd.grad(out, [h_] + list(layer_.parameters()), g_))

    def layer64(m, t):
        return _layer64(m, adj.double(), t, normalize)

    dev = copy.deepcopy(layer).cuda()
    got = run(dev, lambda m, t: m(t, adj.cuda(), normalize_adj=normalize), h.cuda(), g.cuda())
    ref_layer = copy.deepcopy(layer).double()
    ref = run(ref_layer, layer64, h.double(), g.double())
    for p in ref_layer.parameters():
        p.data.abs_()
    T = run(ref_layer, layer64, h.double().abs(), g.double().abs())
    Tw = run(ref_layer, layer64, h.double().abs(), g.double().abs() * (deg + 3)[:, None]) if normalize else [0.0] * len(T)
    eps, n_out = torch.finfo(dtype).eps, ((2 if normalize else 1) * (deg + 3) + K + 4)[:, None]
    counts = [n_out, (cdeg + O + 6)[:, None]] + [B * N + cdeg.max() + 6] * (len(T) - 2)
    assert bool(ref[0][:, 0].isnan().all()) == normalize                 # row 0 has no entries: NaN exactly when normalised
    _assert_within(got[0], ref[0], eps * n_out * T[0])
    for a, b, t, tw, n in list(zip(got, ref, T, Tw, counts))[1:]:
        _assert_within(a, b, eps * (n * t + tw))
    if normalize:                                                # a pre-normalised adj agrees with the in-layer normalisation
        pre = dev(h.cuda(), gcn.normalize_adj(adj.cuda()), normalize_adj=False)
        rows = torch.arange(1, N)                                # (row 0 is empty: NaN in the layer, 0 on the pre-normalised adj)
        _assert_within(pre[:, rows], ref[0][:, rows], (eps * n_out * T[0])[:, rows])


@pytest.mark.gpu
def test_determinism_cache_and_torch_path():
    adj, x = _adjacency(201, 150, torch.float32, duplicates=True).cuda(), torch.randn(2, 150, 12, device='cuda')
    first = gcn.sparse_bmm(adj, x)
    assert torch.equal(first, gcn.sparse_bmm(adj, x))
    cpu = gcn._torch_sparse_bmm(adj.cpu(), x.cpu())                 # the torch formulation: within the bound, not bit for bit
    _assert_within(first, cpu.double(), _bound(adj.cpu(), torch.float32, adj.cpu().to_dense().double().abs() @ x.cpu().double().abs()))
    adj._values().mul_(2)                                          # through torch: the version counter moves, the lists are rebuilt
    assert torch.equal(gcn.sparse_bmm(adj, x), 2 * first)
    bad = torch.sparse_coo_tensor(torch.tensor([[0, 3], [1, 2]]), torch.ones(2), (4, 4)).cuda()
    bad._indices()[0, 1] = 4
    with pytest.raises(ValueError):
        gcn.sparse_bmm(bad, torch.ones(1, 4, 3, device='cuda'))


def test_cpu_paths_and_state_dict():
    node_feat = torch.rand(1, 3, 5)
    adj = torch.sparse_coo_tensor(torch.tensor([[0, 1, 1, 2, 2, 0], [1, 0, 2, 1, 0, 2]]), torch.ones(6), (3, 3))
    model = gcn.GraphConv(5, 10)
    out = model(node_feat, adj)
    assert out.shape == (1, 3, 10)
    pre = gcn.normalize_adj(adj)
    assert pre.is_sparse and torch.equal(pre._indices(), adj._indices()) and torch.allclose(pre.to_dense().sum(1), torch.ones(3))
    assert torch.allclose(model(node_feat, pre, normalize_adj=False), out, atol=1e-6)
    assert torch.allclose(model(node_feat, adj.to_dense()), out, atol=1e-6)          # a dense adj
    assert torch.allclose(gcn.normalize_adj(adj.to_dense()), pre.to_dense())
    assert torch.allclose(gcn.sparse_bmm(adj, node_feat), adj.to_dense() @ node_feat, atol=1e-6)
    half = model.half()(node_feat.half(), adj.to_dense().half())                     # half precision: the torch formulation
    assert half.dtype == torch.float16 and torch.allclose(half.float(), out, atol=2e-2)
    state = {'linear.weight': torch.ones(10, 5), 'linear.bias': torch.zeros(10),
             'linear_self.weight': torch.ones(10, 5), 'linear_self.bias': torch.zeros(10)}
    gcn.GraphConv(5, 10).load_state_dict(state)                                      # the reference module's parameter names
    assert set(gcn.GraphConv(5, 10, self_layer=False, bias=False).state_dict()) == {'linear.weight'}
