"""Bytes <-> bits helpers of ``kaolin.ops.spc`` (reference: kaolin/ops/spc/uint8.py; pure torch there and here).  Bit k of a byte is
entry k of the last dimension: the child ``x << 2 | y << 1 | z`` of an octree node."""
import torch

__all__ = ['uint8_to_bits', 'uint8_bits_sum', 'bits_to_uint8']


def _shifts(device):
    return torch.arange(8, dtype=torch.uint8, device=device)


def uint8_to_bits(uint8_t):
    """uint8 tensor of any shape -> bool tensor of that shape + (8,), least significant bit first."""
    return ((uint8_t.unsqueeze(-1) >> _shifts(uint8_t.device)) & 1).bool()


def uint8_bits_sum(uint8_t):
    """uint8 tensor -> int64 tensor of the same shape: the number of set bits of every byte."""
    return uint8_to_bits(uint8_t).sum(dim=-1)


def bits_to_uint8(bool_t):
    """tensor of last dimension 8 (non-zero = set, least significant bit first) -> uint8 tensor of shape ``bool_t.shape[:-1]``."""
    weights = torch.bitwise_left_shift(torch.ones(8, dtype=torch.long, device=bool_t.device),
                                       torch.arange(8, dtype=torch.long, device=bool_t.device))
    return ((bool_t != 0).long() * weights).sum(dim=-1).byte()
