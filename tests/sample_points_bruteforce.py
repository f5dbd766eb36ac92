"""A numpy oracle of ops.mesh.face_areas / sample_points, written from the contract (DESIGN.md "ops.mesh.sample_points"), not from
the kernels: areas in the input dtype with one rounding per operation, a SEQUENTIAL float64 cumsum, ``searchsorted(side='right')``
and the blend in the input dtype.  Besides the results it returns every sample's ``margin``: the distance of ``t`` to the nearest
cdf entry over ``2 F 2^-52 total`` -- a fixed-order parallel sum may choose a neighbouring face only where the margin is <= 1."""
import numpy as np
import torch


def ieee_sqrt(t):
    """The correctly rounded square root of a CPU tensor (numpy's: the hardware instruction).  torch's CPU sqrt, built on MKL's
    vector maths, is one unit in the last place off for about 0.6 % of its arguments (measured, float and double); the contract
    and the HIP kernels round correctly, so the tests evaluate the torch formulation with this root where they compare bits."""
    with np.errstate(invalid='ignore'):
        return torch.from_numpy(np.sqrt(t.detach().numpy()))


def face_areas(vertices, faces):
    """vertices (B, V, 3) float32 / float64, faces (F, 3) -> (B, F) in the dtype of vertices"""
    dt = vertices.dtype.type
    v0, v1, v2 = (vertices[:, faces[:, k]] for k in range(3))
    x, y = v0 - v1, v1 - v2
    d1 = x[..., 1] * y[..., 2] - x[..., 2] * y[..., 1]
    d2 = x[..., 2] * y[..., 0] - x[..., 0] * y[..., 2]
    d3 = x[..., 0] * y[..., 1] - x[..., 1] * y[..., 0]
    with np.errstate(invalid='ignore'):
        return np.sqrt((d1 * d1 + d2 * d2) + d3 * d3) * dt(0.5)


def choose_faces(areas, r):
    """areas (B, F), r (B, N) float64 -> (choices (B, N) int64, margin (B, N), live (B,))"""
    B, F = areas.shape
    cdf = np.cumsum(areas.astype(np.float64), axis=1)
    total = cdf[:, -1]
    live = (total > 0) & np.isfinite(total)
    choices = np.zeros(r.shape, dtype=np.int64)
    margin = np.full(r.shape, np.inf)
    for b in range(B):
        if not live[b]:
            continue
        t = np.minimum(r[b] * total[b], np.nextafter(total[b], 0.0))
        c = np.searchsorted(cdf[b], t, side='right')
        assert c.max() < F
        choices[b] = c
        nearest = np.minimum(np.abs(t - cdf[b][c]), np.abs(t - cdf[b][np.maximum(c - 1, 0)]))
        margin[b] = nearest / (2.0 * F * 2.0 ** -52 * total[b])
    return choices, margin, live


def weights(uv):
    """uv (..., 2) -> (w0, w1, w2), each (..., 1), in the dtype of uv"""
    one = uv.dtype.type(1)
    u = np.sqrt(uv[..., 0:1])
    v = uv[..., 1:2]
    return one - u, u * (one - v), u * v


def blend(uv, c0, c1, c2):
    w0, w1, w2 = weights(uv)
    return (w0 * c0 + w1 * c1) + w2 * c2


def points_of(vertices, faces, choices, uv, live=None):
    """the blend of the chosen faces' corners: (B, N, 3); items that are not live are NaN"""
    B = vertices.shape[0]
    corners = [np.stack([vertices[b][faces[choices[b], k]] for b in range(B)]) for k in range(3)]
    out = blend(uv, *corners)
    if live is not None:
        out[~live] = np.nan
    return out


def features_of(face_features, choices, uv, live=None):
    """face_features (B, F, 3, D) -> (B, N, D)"""
    B = face_features.shape[0]
    chosen = np.stack([face_features[b][choices[b]] for b in range(B)])        # (B, N, 3, D)
    out = blend(uv, chosen[:, :, 0], chosen[:, :, 1], chosen[:, :, 2])
    if live is not None:
        out[~live] = np.nan
    return out


def sample_points(vertices, faces, r, uv, areas=None, face_features=None):
    """-> dict(areas, choices, margin, live, points, features)"""
    if areas is None:
        areas = face_areas(vertices, faces)
    choices, margin, live = choose_faces(areas, r)
    return dict(areas=areas, choices=choices, margin=margin, live=live, points=points_of(vertices, faces, choices, uv, live),
                features=None if face_features is None else features_of(face_features, choices, uv, live))
