"""Reads tests/golden/voxelgrid_ops.npz (reference outputs recorded by golden/make_golden_voxelgrid_ops.py) for the CPU and
GPU tests of kaolin.ops.voxelgrid / kaolin.metrics.voxelgrid.  Loaded once; the tensors are shared and never modified."""
import functools
import os

import numpy as np
import torch

from conftest import GOLDEN_DIR


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(os.path.join(GOLDEN_DIR, 'voxelgrid_ops.npz')) as f:
        return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def grid(name):
    """The boolean grid stored as ``<name>_bits`` / ``<name>_shape``, as a torch.bool CPU tensor."""
    g = golden()
    shape = tuple(int(s) for s in g[f'{name}_shape'])
    n = int(np.prod(shape))
    return torch.from_numpy(np.unpackbits(g[f'{name}_bits'])[:n].reshape(shape).astype(bool))


def tensor(name):
    return torch.from_numpy(golden()[name])


def error(name):
    """(exception type name, message) the reference raised."""
    kind, text = golden()[f'err_{name}']
    return str(kind), str(text)


FILL_BINARY_CASES = tuple(str(s) for s in golden()['fill_cases'])
