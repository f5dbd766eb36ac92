"""Graph convolution: ``sparse_bmm``, ``normalize_adj`` and ``GraphConv`` (API mirror of kaolin/ops/gcn.py) -- the layers of the
mesh-deformation networks that feed the DIB-R renderer.

The reference moves the dense operand ``(B, N, P) -> (N, B P)``, calls ``torch.sparse.mm`` (on a GPU a library SpMM that adds with
atomics, so its sums change from run to run) and moves the result back; ``GraphConv`` adds a row-sum product, a division and the
self term as kernels of their own.  Here the product is one gather over lists built once per graph.

The arithmetic contract.  Per output element the value is a sequential sum over the row's entries in list order, starting from
+0, one rounded multiply and one rounded add per entry (no fused multiply-add).  List order is the order of the COO entries after a
stable sort by row: ascending column order for a coalesced tensor; the duplicate entries of an uncoalesced one are simply more
terms.  With normalisation the row sum ``norm_i`` is the sequential sum of the row's values in the same order, the result is
``sum / norm_i`` (ONE division) and the self term is then added once.  A row without entries gives ``0 / 0 = NaN`` under
normalisation, as in the reference: nothing is clamped.  The gradient with respect to the dense operand is the same sum over the
column's entries in COO order, each term reading ``grad[b, row, :] / norm[row]`` when normalised.  The two paths:

* a sparse COO CUDA ``adj`` of float32 / float64 that needs no gradient, with M, N and nnz below 2^31 - 1 (the lists hold int32),
  a dense operand of the same device and dtype and no empty dimension, runs csrc/gcn.hip: the contract above to the letter, no
  atomics, and two calls give the same bits.  The lists (``_C.ops.gcn.gcn_lists_cuda``: two stable sorts, one host read,
  ``ValueError`` for an entry outside the matrix) are built once per graph; every step is then ONE launch per direction that reads
  the dense operand in place through its strides, and in ``GraphConv`` fuses aggregation, normalisation and the self term;
* everything else (CPU tensors, half, bfloat16, a dense ``adj``, an ``adj`` that needs a gradient, mixed devices or dtypes, empty
  inputs, 2^31 - 1 rows, columns or entries and more) runs the torch formulation below, the reference's expressions restated: the same mathematical expression with the same
  single division and the same NaN for an empty row, in the summation order and with the multiply-add rounding of torch's own
  kernels, which torch does not document.  The two paths agree within the rounding bound of a sum of ``deg_i`` terms, not bit for bit.

The list cache.  The lists of the last ``adj`` are kept, ONE entry per device: the entry holds the ``_indices()`` and ``_values()``
tensors themselves (strong references: their storage cannot be handed to another tensor while the entry lives) and the lists.  A call
hits the entry when both tensors have the same ``data_ptr()``, ``_version``, shape, strides and dtype and ``adj`` the same shape; any
other call rebuilds the lists and replaces the entry.  In-place writes through torch bump ``_version`` and are seen.  A WRITE THAT
BYPASSES THE VERSION COUNTER (through ``.data``, ``detach()``-ed aliases written by a raw kernel, another library) IS NOT SEEN: the
lists of the old contents are used.  Pass a new tensor in that case.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from .. import _C

__all__ = ['sparse_bmm', 'normalize_adj', 'GraphConv']

_HIP_DTYPES = (torch.float32, torch.float64)

# device index -> (signature, indices, values, the six lists)
_gcn_lists_cache = {}


def _gcn_lists(adj):
    """The lists of ``adj`` from the cache, or built and cached -> (row_offsets, cols, row_vals, col_offsets, rows, col_vals)"""
    indices, values = adj._indices(), adj._values()
    slot = values.device.index
    signature = tuple((t.data_ptr(), t._version, tuple(t.shape), t.stride(), t.dtype) for t in (indices, values)) + (tuple(adj.shape),)
    entry = _gcn_lists_cache.get(slot)
    if entry is not None and entry[0] == signature:
        return entry[3]
    _gcn_lists_cache.pop(slot, None)                      # a failed build leaves no entry behind
    lists = _C.ops.gcn.gcn_lists_cuda(indices, values, adj.shape[0], adj.shape[1])
    _gcn_lists_cache[slot] = (signature, indices, values, lists)
    return lists


def _is_hip_adj(adj):
    return isinstance(adj, torch.Tensor) and adj.layout == torch.sparse_coo and adj.is_cuda and adj.dtype in _HIP_DTYPES and \
        adj.dim() == 2 and adj.dense_dim() == 0 and not adj.requires_grad and adj._nnz() >= 1 and min(adj.shape) >= 1 and \
        max(adj.shape[0], adj.shape[1], adj._nnz()) < 2 ** 31 - 1                # the lists hold int32


def _is_hip_pair(adj, dense):
    return _is_hip_adj(adj) and dense.dim() == 3 and dense.device == adj.device and dense.dtype == adj.dtype and \
        dense.shape[1] == adj.shape[1] and min(dense.shape) >= 1


class _Aggregate(torch.autograd.Function):
    """(B, N, P) [+ (B, M, P)] -> (B, M, P): ``adj @ dense`` in list order, optionally / row sum, optionally + addend"""

    @staticmethod
    def forward(ctx, dense, addend, lists, normalize):
        row_offsets, cols, row_vals, col_offsets, rows, col_vals = lists
        out, norm = _C.ops.gcn.gcn_aggregate_cuda(row_offsets, cols, row_vals, dense, normalize=normalize, addend=addend)
        ctx.save_for_backward(col_offsets, rows, col_vals, norm)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        col_offsets, rows, col_vals, norm = ctx.saved_tensors
        grad_dense = None
        if ctx.needs_input_grad[0]:
            grad_dense, _ = _C.ops.gcn.gcn_aggregate_cuda(col_offsets, rows, col_vals, grad_out, src_norm=norm)
        return grad_dense, grad_out if ctx.needs_input_grad[1] else None, None, None


def _torch_sparse_bmm(sparse_matrix, dense_matrix_batch):
    """The reference's expression (kaolin/ops/gcn.py:39-45): torch.sparse.mm on the batch stacked into columns"""
    m = sparse_matrix.shape[0]
    b, n, p = dense_matrix_batch.shape
    dense_matrix = dense_matrix_batch.transpose(0, 1).reshape(n, b * p)
    result = torch.sparse.mm(sparse_matrix, dense_matrix)
    return result.reshape(m, b, p).transpose(0, 1)


def _torch_row_sums(adj):
    """(M, 1): ``adj @ 1`` (the reference's expression, kaolin/ops/gcn.py:68, 76, with ones of ``adj``'s dtype and column count)"""
    ones = torch.ones((adj.shape[1], 1), dtype=adj.dtype, device=adj.device)
    return torch.sparse.mm(adj, ones) if adj.is_sparse else torch.matmul(adj, ones)


def _torch_normalize_adj(adj):
    """The reference's expression (kaolin/ops/gcn.py:67-78)"""
    norm = _torch_row_sums(adj)
    if adj.is_sparse:
        indices = adj._indices()
        values = adj._values() / norm.squeeze(1).gather(dim=0, index=indices[0, :])
        return torch.sparse_coo_tensor(indices, values, adj.shape)
    return adj / norm


def _torch_graph_conv(adj, feat, self_feat, normalize):
    """The reference's expression (kaolin/ops/gcn.py:177-199) on the outputs of the two linears"""
    result = _torch_sparse_bmm(adj, feat) if adj.is_sparse else torch.matmul(adj, feat)
    if normalize:
        result = result / _torch_row_sums(adj)
    if self_feat is not None:
        result = result + self_feat
    return result


def sparse_bmm(sparse_matrix, dense_matrix_batch):
    r"""Perform torch.bmm on an unbatched sparse matrix and a batched dense matrix (reference: kaolin/ops/gcn.py:24-45).

    On float / double CUDA tensors one HIP launch that reads ``dense_matrix_batch`` in place, without atomics: per element a
    sequential sum over the row's entries in COO order, the same bits on every run (the module's docstring has the contract, the
    paths and THE RULE OF THE LIST CACHE: writes to ``sparse_matrix`` that bypass its version counter are not seen).  Differentiable
    in ``dense_matrix_batch``; a ``sparse_matrix`` that needs a gradient takes the torch formulation.

    Args:
        sparse_matrix (torch.sparse.FloatTensor): Input sparse matrix, of shape :math:`(\text{M}, \text{N})`, coalesced or not.
        dense_matrix_batch (torch.FloatTensor): Input batched dense matrix, of shape :math:`(\text{batch_size}, \text{N}, \text{P})`,
            any strides (expanded dimensions included).

    Returns:
        (torch.FloatTensor): Result of the batched matrix multiplication, of shape :math:`(\text{batch_size}, \text{M}, \text{P})`.
    """
    if _is_hip_pair(sparse_matrix, dense_matrix_batch):
        return _Aggregate.apply(dense_matrix_batch, None, _gcn_lists(sparse_matrix), False)
    return _torch_sparse_bmm(sparse_matrix, dense_matrix_batch)


def normalize_adj(adj):
    r"""Normalize the adjacency matrix such that the sum of each row is 1 (reference: kaolin/ops/gcn.py:48-78).

    This supports both sparse tensor and regular tensor. The return type will be the same as the input type: a sparse ``adj`` gives
    a sparse tensor on the same indices, in the same entry order.  On a float / double sparse CUDA ``adj`` the row sums are
    sequential sums in COO order on HIP kernels over the cached lists (see the module's docstring); a row without entries has none
    to scale, a row whose values sum to zero gives inf / NaN as in the reference.

    Args:
        adj (torch.sparse.FloatTensor or torch.FloatTensor): Input adjacency matrix, of shape
            :math:`(\text{num_nodes}, \text{num_nodes})`.

    Returns:
        (torch.sparse.FloatTensor or torch.FloatTensor): A new adjacency matrix with the same connectivity as the input, but with
        the sum of each row normalized to 1.
    """
    if _is_hip_adj(adj):
        row_offsets, _, row_vals = _gcn_lists(adj)[:3]
        norm = _C.ops.gcn.gcn_row_sums_cuda(row_offsets, row_vals)
        values = _C.ops.gcn.gcn_scale_values_cuda(adj._indices(), adj._values(), norm)
        return torch.sparse_coo_tensor(adj._indices(), values, adj.shape, is_coalesced=adj.is_coalesced())
    return _torch_normalize_adj(adj)


class GraphConv(nn.Module):
    r"""A simple graph convolution layer, similar to the one defined by *Kipf et al.* in
    `Semi-Supervised Classification with Graph Convolutional Networks`_ ICLR 2017 (reference: kaolin/ops/gcn.py:80-199).

    With ``self_layer=False`` it computes :math:`(A H W)`: :math:`H` the node features, of shape
    :math:`(\text{batch_size}, \text{num_nodes}, \text{input_dim})`, :math:`W` a weight matrix of shape
    :math:`(\text{input_dim}, \text{output_dim})` and :math:`A` the adjacency matrix, of shape
    :math:`(\text{num_nodes}, \text{num_nodes})`, which can include self-loops.  With ``normalize_adj=True`` it computes
    :math:`(D^{-1} A H W)`, :math:`D_{ii}` being the sum of the i-th row of :math:`A`.  With ``self_layer=True`` it adds
    :math:`(H W_{\text{self}})`, a separate weight matrix that filters each node's own features; :math:`A` should then not include
    self-loops.

    ``linear`` and ``linear_self`` are ``nn.Linear`` modules as in the reference (state dicts interchange) and run on torch's GEMM;
    on the HIP path (see the module's docstring) everything after them is ONE launch.

    Args:
        input_dim (int): The number of features in each input node.
        output_dim (int): The number of features in each output node.
        self_layer (bool): Whether to add the node's own filtered features. Default: True.
        bias (bool): Whether to add bias after the node-wise linear layer. Default: True.

    Example:
        >>> node_feat = torch.rand(1, 3, 5)
        >>> i = torch.LongTensor(
        ...     [[0, 1, 1, 2, 2, 0], [1, 0, 2, 1, 0, 2]])
        >>> v = torch.FloatTensor([1, 1, 1, 1, 1, 1])
        >>> adj = torch.sparse_coo_tensor(i, v, torch.Size([3, 3]))
        >>> model = GraphConv(5, 10)
        >>> output = model(node_feat, adj)
        >>> # pre-normalize adj
        >>> adj = normalize_adj(adj)
        >>> output = model(node_feat, adj, normalize_adj=False)

    .. _Semi-Supervised Classification with Graph Convolutional Networks:
        https://arxiv.org/abs/1609.02907
    """

    def __init__(self, input_dim, output_dim, self_layer=True, bias=True):
        super().__init__()
        self.self_layer = self_layer
        self.linear = nn.Linear(input_dim, output_dim, bias=bias)
        self.linear_self = nn.Linear(input_dim, output_dim, bias=bias) if self_layer else None
        self.initialize()

    def initialize(self):
        for linear in (self.linear, self.linear_self):
            if linear is not None:
                nn.init.xavier_uniform_(linear.weight.data)
                if linear.bias is not None:
                    linear.bias.data.uniform_(-1.0, 1.0)

    def forward(self, node_feat, adj, normalize_adj=True):
        r"""
        Args:
            node_feat (torch.FloatTensor): The input features of each node, of shape
                :math:`(\text{batch_size}, \text{num_nodes}, \text{input_dim})`.
            adj (torch.sparse.FloatTensor or torch.FloatTensor): The adjacency matrix. ``adj[i, j]`` is non-zero if there's an
                incoming edge from ``j`` to ``i``. Should not include self-loop if ``self_layer`` is ``True``, of shape
                :math:`(\text{num_nodes}, \text{num_nodes})`.
            normalize_adj (optional, bool): Set this to true to apply normalization to adjacency; that is, each output feature
                will be divided by the number of incoming neighbors. If normalization is not desired, or if the adjacency matrix
                is pre-normalized, set this to False to improve performance. Default: True.

        Returns:
            (torch.FloatTensor): The output features of each node, of shape
            :math:`(\text{batch_size}, \text{num_nodes}, \text{output_dim})`.
        """
        feat = self.linear(node_feat)
        self_feat = self.linear_self(node_feat) if self.self_layer else None
        if _is_hip_pair(adj, feat) and (self_feat is None or adj.shape[0] == adj.shape[1]):
            return _Aggregate.apply(feat, self_feat, _gcn_lists(adj), bool(normalize_adj))
        return _torch_graph_conv(adj, feat, self_feat, normalize_adj)
