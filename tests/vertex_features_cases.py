"""Inputs shared by test_vertex_features_cpu.py and test_vertex_features_gpu.py: random meshes whose features are scaled by
random integers up to 1000, so that the order of the additions shows in the last bits of a sum."""
import json
import os

import numpy as np
import torch

from conftest import GOLDEN_DIR

NP_DTYPES = {torch.float16: np.float16, torch.float32: np.float32, torch.float64: np.float64}


def random_faces(F, K, V, seed, lo=0, hi=None):
    """(F, K) int64 ids drawn from [lo, hi) (default: all V vertices)"""
    rng = np.random.default_rng(seed)
    return rng.integers(lo, V if hi is None else hi, size=(F, K), dtype=np.int64)


def random_features(shape, dtype, seed):
    """uniform [0, 1) times an integer in [1, 1000], in the numpy dtype of the torch `dtype`"""
    rng = np.random.default_rng(seed + 1)
    return (rng.random(shape) * rng.integers(1, 1001, size=shape)).astype(NP_DTYPES[dtype])


def tangents_example(dtype, device='cpu'):
    """-> faces, face_vertices, face_uvs, vertex_normals, expected, atol, rtol of the reference's recorded example"""
    with open(os.path.join(GOLDEN_DIR, 'vertex_tangents_example.json')) as fh:
        rec = json.load(fh)
    faces = torch.tensor(rec['faces'], dtype=torch.long, device=device)
    vertices = torch.tensor(rec['vertices'], dtype=dtype, device=device)
    return (faces, vertices[faces], torch.tensor(rec['face_uvs'], dtype=dtype, device=device),
            torch.tensor(rec['vertex_normals'], dtype=dtype, device=device),
            torch.tensor(rec['expected_tangents'], dtype=dtype, device=device), rec['atol'], rec['rtol'])
