"""The per-vertex sum / mean of per-face-corner features restated in numpy, the oracle of both paths of
kaolin_amd.ops.mesh.vertex_features (the torch formulation and the HIP gather).

Contract: out[b, v, :] = the sum over the corners (f, k) with faces[f, k] == v in the order (k ascending, then f ascending), one
rounded addition in the array's dtype per corner, starting from +0; with ``mean`` divided ONCE by max(count, 1), the count converted
to the dtype.  The loop below walks all corners in (k, f) order and adds each to the row of its vertex: every vertex then sees its
own corners in exactly that order, one numpy addition (one rounding) at a time.  Nothing is vectorised across corners."""
import numpy as np


def vertex_gather(faces, face_features, num_vertices, mean=True):
    """faces (F, K) integers, face_features (B, F, K, N) float16 / float32 / float64 -> (B, V, N) in the dtype of face_features"""
    faces = np.asarray(faces)
    x = np.asarray(face_features)
    B, F, K, N = x.shape
    assert faces.shape == (F, K)
    out = np.zeros((B, num_vertices, N), dtype=x.dtype)
    count = np.zeros(num_vertices, dtype=np.int64)
    for k in range(K):
        for f in range(F):
            v = int(faces[f, k])
            assert 0 <= v < num_vertices
            out[:, v, :] = out[:, v, :] + x[:, f, k, :]            # one rounded addition per corner
            count[v] += 1
    if mean:
        out = out / np.maximum(count, 1).astype(x.dtype)[None, :, None]
        assert out.dtype == x.dtype
    return out


def vertex_gather_backward(faces, grad_out, mean=True):
    """grad_out (B, V, N) -> (B, F, K, N): grad[b, f, k, :] = grad_out[b, faces[f, k], :] (/ max(count, 1)): one division"""
    faces = np.asarray(faces)
    g = np.asarray(grad_out)
    if mean:
        count = np.bincount(faces.reshape(-1), minlength=g.shape[1])
        g = g / np.maximum(count, 1).astype(g.dtype)[None, :, None]
    return g[:, faces, :]
