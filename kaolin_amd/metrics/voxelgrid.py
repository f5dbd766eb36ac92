"""Voxelgrid metrics.  Behaviour follows kaolin/metrics/voxelgrid.py:19-50."""
import torch

__all__ = ['iou']


def iou(pred, gt):
    r"""Intersection over union of two batches of (binary) voxelgrids of shape :math:`(N, X, Y, Z)`, per batch item.

    Anything non-zero counts as occupied.  An item whose union is empty gives ``nan`` (0 / 0), as in the reference.

    Returns:
        (torch.FloatTensor): of shape :math:`(N)`.
    """
    if pred.shape != gt.shape:
        raise ValueError(
            f"Expected predicted voxelgrids and ground truth voxelgrids to have "
            f"the same shape, but got {pred.shape} for predicted and {gt.shape} for ground truth.")
    a, b = pred.bool(), gt.bool()
    both = (a & b).sum(dim=(1, 2, 3)).float()
    either = (a | b).sum(dim=(1, 2, 3)).float()
    return both / either
