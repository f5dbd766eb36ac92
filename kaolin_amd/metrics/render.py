"""Render metrics.

``mask_iou`` is the silhouette loss paired with ``dibr_soft_mask`` in the DIB-R training loop.  Behaviour follows
kaolin/metrics/render.py:18-40: soft intersection = product, soft union = sum - product,
loss = 1 - mean_b(I_b / (U_b + 1e-10)).  On the GPU (float / double) it is one fused HIP pass each way
(kaolin_amd/csrc/render_metrics.hip); other inputs take the torch formulation below, which is also the
definition the fused path is tested against.
"""
import os

import torch

from .. import _C

__all__ = ['mask_iou', 'weighted_sum']


class _MaskIoUCuda(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lhs_mask, rhs_mask):
        lhs, rhs = lhs_mask.contiguous(), rhs_mask.contiguous()
        loss, sums = _C.render.mesh.mask_iou_forward_fused(lhs, rhs)
        ctx.save_for_backward(lhs, rhs, sums)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        lhs, rhs, sums = ctx.saved_tensors
        g_lhs = _C.render.mesh.mask_iou_backward_fused(grad_loss, rhs, sums) if ctx.needs_input_grad[0] else None
        g_rhs = _C.render.mesh.mask_iou_backward_fused(grad_loss, lhs, sums) if ctx.needs_input_grad[1] else None
        return g_lhs, g_rhs


def _mask_iou_torch(lhs_mask, rhs_mask):
    inter = (lhs_mask * rhs_mask).flatten(1)
    union = (lhs_mask + rhs_mask).flatten(1) - inter
    per_item = inter.sum(dim=1) / (union.sum(dim=1) + 1e-10)
    return 1.0 - per_item.mean()


def mask_iou(lhs_mask, rhs_mask):
    r"""IoU loss between two (soft) segmentation masks of shape :math:`(B, H, W)`.

    Returns:
        (torch.Tensor): scalar ``1 - mean IoU`` over the batch.
    """
    if lhs_mask.shape != rhs_mask.shape or lhs_mask.dim() != 3:
        raise AssertionError('mask_iou expects two masks of identical shape (B, H, W)')
    if (lhs_mask.is_cuda and rhs_mask.is_cuda and lhs_mask.device == rhs_mask.device and lhs_mask.dtype == rhs_mask.dtype and
            lhs_mask.dtype in (torch.float32, torch.float64) and lhs_mask.numel() > 0 and
            lhs_mask.shape[0] <= 65535):      # (the kernels put the batch on a grid dimension)
        return _MaskIoUCuda.apply(lhs_mask, rhs_mask)
    return _mask_iou_torch(lhs_mask, rhs_mask)


class _WeightedSum2Cuda(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x1, w1, x2, w2):
        x1, w1 = x1.contiguous(), w1.contiguous()
        if x2 is not None:
            x2, w2 = x2.contiguous(), w2.contiguous()
        ctx.w = (w1, w2)
        return _C.render.mesh.weighted_sum2_forward(x1, w1, x2, w2)

    @staticmethod
    def backward(ctx, grad_out):
        w1, w2 = ctx.w
        g1, g2 = _C.render.mesh.weighted_sum2_backward(grad_out, w1, w2, ctx.needs_input_grad[0],
                                                       w2 is not None and ctx.needs_input_grad[2])
        return g1, None, g2, None


class _WeightedSumDibr(torch.autograd.Function):
    """``weighted_sum`` of the two outputs of ONE ``dibr_rasterization`` node, differentiated straight into that node's inputs.

    Its differentiable inputs are the DIB-R node's own (``face_vertices_image``, ``face_features``), not the outputs: autograd
    adds what this node returns to whatever the DIB-R node contributes when its outputs have other consumers.  Forward: the
    loss of the detached outputs, as ``_WeightedSum2Cuda`` computes it.  Backward: the DIB-R backward kernels read the weights
    and scale them by the incoming gradient where they read a gradient (``kamd_dibr_weighted_sum_backward_*``) -- the two
    output-sized gradients ``g * w`` are never written."""

    @staticmethod
    def forward(ctx, face_vertices_image, face_features, node, saved, x1, w1, x2, w2):
        # `saved`: the DIB-R node's saved tensors, unpacked once.  Kept as they are, not through save_for_backward (a second
        # pack / unpack of ten tensors on the step's host path): they live as long as the node does anyway (its own backward
        # does not run when the loss is the outputs' only consumer), and this node holds the node.  The one of them an in-place
        # operation could change, the soft mask, is checked by hand.
        ctx.node, ctx.saved, ctx.w = node, saved, (w1, w2)
        ctx.soft_version = saved[2]._version
        return _C.render.mesh.weighted_sum2_forward(x1, w1, x2, w2)

    @staticmethod
    def backward(ctx, grad_out):
        node, saved = ctx.node, ctx.saved
        face_idx, weights, soft_mask, face_vertices_image, face_features = saved[:5]
        if soft_mask._version != ctx.soft_version:
            raise RuntimeError('weighted_sum: the soft mask of dibr_rasterization, needed for gradient computation, has been '
                               'modified by an inplace operation')
        sigmainv, knum, multiplier, eps = node.cfg
        # the gradient buffer the forward cleared, if the DIB-R node has not used it yet (DibrRasterizationCuda.backward)
        zeroed, node.zeroed_grad = node.zeroed_grad, None
        w1, w2 = ctx.w
        g_img, g_feat = _C.render.mesh.dibr_weighted_sum_backward_fused(
            grad_out, w1, w2, face_idx, weights, soft_mask, saved[5:], face_vertices_image, face_features,
            sigmainv, knum, multiplier, eps, need_feature_grad=ctx.needs_input_grad[1], zeroed_grad_image=zeroed)
        return (g_img if ctx.needs_input_grad[0] else None), g_feat, None, None, None, None, None, None


def _fused_dibr_backward_enabled():
    # KAMD_WS_FUSED_BWD=2: weighted_sum of dibr_rasterization's outputs takes the materialised path (A/B runs); as the library's
    # knobs, a positive integer, anything else is the default
    v = os.environ.get('KAMD_WS_FUSED_BWD')
    return not (v and v.isdigit() and int(v) == 2)


_DIBR_NODE = None    # the class of DibrRasterizationCuda's autograd nodes (imported on first use)


def _dibr_node(image, image_weights, mask, mask_weights):
    """The ``DibrRasterizationCuda`` node whose outputs 0 (and 1) ``image`` (and ``mask``) are, untouched since it made them, when
    the weights fit its gradients' layout; else None."""
    global _DIBR_NODE
    if _DIBR_NODE is None:
        from ..render.mesh.dibr import DibrRasterizationCuda
        _DIBR_NODE = DibrRasterizationCuda._backward_cls
    node = image.grad_fn
    if (node is None or type(node) is not _DIBR_NODE or image.output_nr != 0 or
            image.dtype not in (torch.float32, torch.float64)):
        return None
    versions = getattr(node, 'output_versions', None)
    if versions is None or image._version != versions[0]:
        return None
    pairs = [(image, image_weights)]
    if mask is not None:
        if mask.grad_fn is not node or mask.output_nr != 1 or mask._version != versions[1]:
            return None
        pairs.append((mask, mask_weights))
    for x, w in pairs:
        if not (w.device == x.device and w.dtype == x.dtype and w.shape == x.shape and w.is_contiguous() and
                not w.requires_grad):
            return None
    return node


def _saved_tensors(node):
    try:
        return node.saved_tensors
    except RuntimeError:    # (freed by a backward pass through the node: the unfused path reports what is wrong, if anything)
        return None


def _fusable(x, w):
    return (x.is_cuda and w.is_cuda and x.device == w.device and x.dtype == w.dtype and
            x.dtype in (torch.float32, torch.float64) and x.shape == w.shape and not w.requires_grad)


def weighted_sum(image, image_weights, mask=None, mask_weights=None):
    r"""The linear loss :math:`\sum image \cdot image\_weights + \sum mask \cdot mask\_weights` of one render's G-buffers
    against fixed weights (what gradient checks and benchmarks of a renderer back-propagate).

    Not a reference operator: in torch it is ``(image * image_weights).sum() + (mask * mask_weights).sum()`` -- two
    reductions, an add and two full-size products backward.  On the GPU both sums are one fused pass forward and both
    gradients one pass backward (kaolin_amd/csrc/render_metrics.hip); other inputs take the torch formulation.  When
    ``image`` (and ``mask``) are outputs 0 (and 1) of one :func:`~kaolin_amd.render.mesh.dibr_rasterization` call, not modified
    in place since, the backward goes straight into that call's inputs: its backward kernels read the weights where they read
    a gradient and scale them by the loss' gradient (``_WeightedSumDibr``), so the two gradients are never materialised.

    Args:
        image, image_weights (torch.Tensor): same shape and dtype.
        mask, mask_weights (torch.Tensor, optional): same shape and dtype as each other.

    Returns:
        (torch.Tensor): scalar.
    """
    if (mask is None) != (mask_weights is None):
        raise ValueError('weighted_sum expects mask and mask_weights together')
    pair2 = mask is not None
    node = (_dibr_node(image, image_weights, mask, mask_weights)
            if image.requires_grad and image.numel() > 0 and _fused_dibr_backward_enabled() else None)
    saved = _saved_tensors(node) if node is not None else None
    # (face_idx, weights, soft_mask, face_vertices_image, face_features, *hits).  Index 3 and 4 must be the node's inputs
    # themselves (DibrRasterizationCuda.forward saves them as given when they are contiguous): a copy made inside its forward
    # carries no gradient
    if saved is not None and (saved[3].requires_grad == node.needs_input_grad[3] and
                              saved[4].requires_grad == node.needs_input_grad[4]):
        return _WeightedSumDibr.apply(saved[3], saved[4], node, saved, image.detach(), image_weights,
                                      mask.detach() if pair2 else None, mask_weights)
    if (_fusable(image, image_weights) and image.numel() > 0 and
            (not pair2 or (_fusable(mask, mask_weights) and mask.dtype == image.dtype and mask.device == image.device))):
        return _WeightedSum2Cuda.apply(image, image_weights, mask, mask_weights)
    out = (image * image_weights).sum()
    if pair2:
        out = out + (mask * mask_weights).sum()
    return out
