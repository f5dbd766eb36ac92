"""Inputs of ``prepare_vertices``, ``texture_mapping`` and ``mask_iou`` at the shapes and edges where their kernels can go
wrong, shared by the fixture generator (tests/golden/make_golden_render_helpers.py) and tests/test_render_helpers_reference.py.
Plain torch and numpy; nothing here reads the reference.  Every value is drawn in float64 from a seeded CPU generator (or
written down), rounded to float32 and widened again, so that a float32 and a float64 run see the same numbers.

A case is a dict of float64 CPU tensors; ``pv_run`` / ``tm_run`` / ``mi_run`` feed it, in a dtype and on a device, to ANY
implementation of the operator (the reference's function, the package's torch chain, the public API) and return the
outputs and the gradients of sum(output * upstream gradient) as a dict.  ``reference(...)`` runs the package's torch chain
on the CPU in float64 and in float32 and returns (ref64, ref32, E32) with E32 = max |ref32 - ref64| per tensor: the
reference arithmetic's own float32 error, which is the absolute floor of the kernels' bound (``mismatch``).

prepare_vertices (``PV_CASES``; cameras ``rt`` = camera_rot + camera_trans, ``tf`` = (B, 4, 3) camera_transform; vertex layouts
``shared`` (1, V, 3), ``expanded`` = that tensor expanded to B views, ``batched`` (B, V, 3), ``strided`` = (B, V, 4)[..., :3]):
    b1_f1 b3_f21 b1_f64 b1_f65 b3_f43 b13_f20   geodesic spheres of frequency 1 / 2 (20 / 80 faces) cut to F faces and
                  perturbed; B * F = 1, 63, 64, 65, 129, 260 one-lane-per-face items: one lane, no full wavefront, exactly one,
                  one plus a one-lane tail, wavefronts that span two views, two workgroups.  Cutting leaves vertices without
                  a face (gradient exactly 0)
    fan           one hub vertex in 65 faces (a long adjacency row)
    f0            no face at all
    repeat        6 faces, two with a repeated vertex index (normal exactly 0)           } ill-conditioned: the gradient of a
    collinear     4 faces under the identity camera, one exactly collinear (normal 0)    } zero normal is g / 1e-10
    ill           16 faces: 8 slivers of aspect 1e-3, 8 with vertices at |z_cam| ~ 1e-2   } (CONDITIONED is False)

texture_mapping (``TM_CASES``; every case runs ``nearest`` and ``bilinear``):
    t1x1_c1_n1, t1x5_c3_n255_b3, t2x2_c5_n257, t4x6_c3_dense_b3, t17x23_c3_n257_b3, t17x23_c1_dense, t2x2_c3_n2000
    Coordinates: random in [-0.2, 1.2]; exactly 0, 1, 0.5; on the sizes where float32 holds them exactly (1, 2, 4 and the
    middle of 6) texel edges -- `nearest` lands on x.5 source indices there and must round half to even -- and texel
    centres, the first and last of which sit on the border clip, where grid_sample's uv gradient is exactly 0.
    centres_inexact  the centres (i + 0.5) / 6 and (j + 0.5) / 4 of a 4 x 6 texture: 1 / 12 is not a float32, so the source
                  index is an integer give or take a rounding and the uv gradient's cell is a coin toss (CONDITIONED False)

mask_iou (``MI_CASES``): soft left mask, hard right mask at (1, 1, 1), (1, 7, 5), (5, 33, 31), (2, 127, 129), (1, 129, 127)
    (1023, 16383 elements per item: around the 64 x 256 lanes of the partial-sum pass); ``kinds`` = four items: both empty,
    identical hard masks, empty against full, soft; ``views`` = a transposed view against an expanded row.
    The upstream gradient is ``MI_UPSTREAM``, not 1.
"""
import functools
import math
import os

import numpy as np
import torch

from kaolin_amd.render import camera as _cam
from kaolin_amd.utils.testing import fibonacci_cameras, geodesic_sphere

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURE = os.path.join(GOLDEN_DIR, 'render_helpers.npz')

F32_REL, F32_FLOOR = 1e-5, 4.0          # float32: |x - ref64| <= 1e-5 |ref64| + 4 E32
F64_REL, F64_FLOOR = 1e-10, 1e-6        # float64: |x - ref64| <= 1e-10 |ref64| + 1e-6 E32
CONDITIONED_E32 = 1e-5                  # a well-conditioned case: E32 <= 1e-5 max|ref64| for every tensor
ILL_MAX_FACES = 16
MI_UPSTREAM = 1.75


def r32(t):
    """float64 tensor holding float32 values"""
    return t.to(torch.float64).to(torch.float32).to(torch.float64)


def _leaf(t, dtype, device, requires_grad=True):
    """a fresh copy of a case's tensor (the cases are shared: nothing may set requires_grad on them)"""
    return t.detach().to(dtype=dtype, device=device, copy=True).requires_grad_(requires_grad)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(shape, g, lo=0., hi=1.):
    return r32(torch.rand(shape, generator=g, dtype=torch.float64) * (hi - lo) + lo)


# ---- prepare_vertices ----------------------------------------------------------------------------------------------------

PV_CAMERAS = ('rt', 'tf')
PV_LAYOUTS = ('shared', 'expanded', 'batched')
PV_OUTPUTS = ('cam', 'img', 'nrm')
PV_SHAPES = ((1, 1), (3, 21), (1, 64), (1, 65), (3, 43), (13, 20))
PV_WHICH = (('cam', 'img', 'nrm'), ('cam',), ('img',), ('nrm',))


def _cameras(B, identity):
    if identity:
        rot = torch.eye(3, dtype=torch.float64).repeat(B, 1, 1)
        trans = torch.zeros(B, 3, dtype=torch.float64)
    else:
        pos = fibonacci_cameras(B, 2.5, torch.float64)
        up = torch.tensor([[0., 1., 0.]], dtype=torch.float64).repeat(B, 1)
        rot, trans = _cam.generate_rotate_translate_matrices(pos, torch.zeros_like(pos), up)
    rot, trans = r32(rot), r32(trans)
    # [v, 1] M = R (v - t), rounded on its own: the two parametrisations are two (close) cameras, each with its own reference
    transform = r32(torch.cat([rot.transpose(1, 2), (-(rot @ trans.unsqueeze(-1))).transpose(1, 2)], dim=1))
    proj = r32(_cam.generate_perspective_projection(math.pi / 4, dtype=torch.float64))
    return dict(rot=rot, trans=trans, transform=transform, proj=proj)


def _pv_case(name, B, verts, faces, seed, identity=False, noise=0.01, conditioned=True):
    g = _gen(seed)
    V, F = verts.shape[0], faces.shape[0]
    x = dict(name=name, B=B, conditioned=conditioned, faces=faces.long().contiguous(), verts1=r32(verts).unsqueeze(0))
    x['vertsB'] = r32(x['verts1'] + noise * torch.randn(B, V, 3, generator=g, dtype=torch.float64))
    x.update(_cameras(B, identity))
    x['g_cam'], x['g_img'], x['g_nrm'] = _rand((B, F, 3, 3), g, -1., 1.), _rand((B, F, 3, 2), g, -1., 1.), _rand((B, F, 3), g, -1., 1.)
    return x


def _sphere_case(B, F):
    v, f = geodesic_sphere(1 if F <= 20 else 2)
    v = v + 0.02 * torch.randn(v.shape, generator=_gen(100 + F), dtype=torch.float64)
    return _pv_case(f'b{B}_f{F}', B, v, f[:F], seed=200 + 7 * B + F)


def _fan_case():
    n = 65
    a = torch.arange(n + 1, dtype=torch.float64) * (2 * math.pi / (n + 1))
    g = _gen(11)
    rim = torch.stack([0.5 * torch.cos(a), 0.5 * torch.sin(a), 0.1 * torch.rand(n + 1, generator=g, dtype=torch.float64)], dim=1)
    v = torch.cat([torch.tensor([[0.02, -0.03, 0.25]], dtype=torch.float64), rim])
    i = torch.arange(1, n + 1)
    return _pv_case('fan', 2, v, torch.stack([torch.zeros_like(i), i, i + 1], dim=1), seed=12)


PV_ZERO_NORMALS = {'repeat': (1, 4), 'collinear': (1,)}      # case -> the faces whose normal is exactly 0


def _repeat_case():
    v = torch.randn(7, 3, generator=_gen(21), dtype=torch.float64) * 0.3
    # faces 1 and 4 repeat a vertex so that ONE EDGE is exactly 0 (0 x d == 0 in any arithmetic; with two equal edges a x a is 0
    # only without fused multiply-adds, which torch's CPU cross product uses)
    f = torch.tensor([[0, 1, 2], [3, 3, 4], [2, 1, 5], [0, 2, 6], [6, 5, 6], [4, 0, 1]])
    return _pv_case('repeat', 2, v, f, seed=22, conditioned=False)


def _collinear_case():
    # identity camera: camera space is world space, every product with 0 / 1 is exact, and (1, .5, -1) x (2, 1, -2) == 0
    v = torch.tensor([[0., 0., -2.], [1., 0.5, -3.], [2., 1., -4.], [0.5, -0.25, -2.5], [-0.75, 0.5, -3.5], [0.25, 1., -2.25]],
                     dtype=torch.float64)
    f = torch.tensor([[3, 4, 5], [0, 1, 2], [0, 3, 5], [2, 4, 1]])
    return _pv_case('collinear', 1, v, f, seed=31, identity=True, noise=0., conditioned=False)


def _ill_case():
    g = _gen(41)
    cams = _cameras(2, False)
    R0, t0 = cams['rot'][0], cams['trans'][0]
    pts = []
    for i in range(8):                          # slivers: base 0.3, height 3e-4, around the origin
        e = torch.randn(3, generator=g, dtype=torch.float64)
        e = e / e.norm()
        n = torch.linalg.cross(e, torch.randn(3, generator=g, dtype=torch.float64))
        n = n / n.norm()
        p0 = (torch.rand(3, generator=g, dtype=torch.float64) - 0.5) * 0.4
        pts += [p0, p0 + 0.3 * e, p0 + 0.15 * e + 3e-4 * n]
    for i in range(8):                          # in view 0's camera space: 0.05 across, 1e-2 .. 2e-2 in front of the pinhole
        c = torch.cat([(torch.rand(3, 2, generator=g, dtype=torch.float64) - 0.5) * 0.1,
                       -0.01 * (1. + torch.rand(3, 1, generator=g, dtype=torch.float64))], dim=1)
        pts += list(c @ R0 + t0)                # world = R^T c + t
    v = torch.stack(pts)
    x = _pv_case('ill', 2, v, torch.arange(48).reshape(16, 3), seed=42, noise=0., conditioned=False)
    zc = (x['verts1'][0] - x['trans'][:, None]) @ x['rot'].transpose(1, 2)
    assert float(zc[0, 24:, 2].abs().max()) < 2.1e-2 and float(zc[0, 24:, 2].abs().min()) > 0.9e-2
    assert float(zc[1, :, 2].abs().min()) > 0.1 and float(zc[0, :24, 2].abs().min()) > 0.1
    return x


def _f0_case():
    v = geodesic_sphere(1)[0]
    return _pv_case('f0', 2, v, torch.zeros((0, 3), dtype=torch.long), seed=51)


@functools.lru_cache(maxsize=None)
def pv_cases():
    cases = [_sphere_case(B, F) for B, F in PV_SHAPES] + [_fan_case(), _f0_case(), _repeat_case(), _collinear_case(), _ill_case()]
    return {c['name']: c for c in cases}


PV_SPHERES = tuple(f'b{B}_f{F}' for B, F in PV_SHAPES)
PV_KERNEL_SET = PV_SPHERES + ('fan', 'f0', 'repeat', 'collinear', 'ill')
# (case, camera, layout, upstream gradients) of the fixture: the smallest members and every edge
PV_PINNED = tuple(
    [(c, cam, lay, PV_WHICH[0]) for c in ('b1_f1', 'b3_f21') for cam in PV_CAMERAS for lay in PV_LAYOUTS] +
    [('b3_f21', 'rt', 'batched', w) for w in PV_WHICH[1:]] + [('b3_f21', 'tf', 'strided', PV_WHICH[0])] +
    [(c, cam, 'batched', PV_WHICH[0]) for c in ('fan', 'f0', 'repeat', 'ill') for cam in PV_CAMERAS] +
    [('repeat', 'rt', 'batched', ('nrm',))] +
    [('collinear', cam, lay, w) for cam in PV_CAMERAS for lay in ('shared', 'batched') for w in (PV_WHICH[0], ('nrm',))])


def pv_vertices(case, layout, dtype, device):
    """-> (leaf that collects the gradient, the vertices argument)"""
    if layout in ('shared', 'expanded'):
        leaf = _leaf(case['verts1'], dtype, device)
        return leaf, (leaf if layout == 'shared' else leaf.expand(case['B'], -1, -1))
    if layout == 'batched':
        leaf = _leaf(case['vertsB'], dtype, device)
        return leaf, leaf
    assert layout == 'strided'
    leaf = _leaf(torch.nn.functional.pad(case['vertsB'], (0, 1), value=0.5), dtype, device)
    return leaf, leaf[..., :3]


def pv_run(fn, case, camera, layout, dtype, device='cpu', which=PV_WHICH[0]):
    """fn(vertices, faces, proj, camera_rot=, camera_trans= | camera_transform=) -> dict cam, img, nrm, gv (detached), node"""
    to = lambda t: t.to(dtype).to(device)  # noqa: E731
    leaf, verts = pv_vertices(case, layout, dtype, device)
    kw = dict(camera_rot=to(case['rot']), camera_trans=to(case['trans'])) if camera == 'rt' else dict(camera_transform=to(case['transform']))
    out = fn(verts, case['faces'].to(device), to(case['proj']), **kw)
    res = dict(zip(PV_OUTPUTS, (o.detach() for o in out)))
    res['node'] = out[0].grad_fn
    sum((out[PV_OUTPUTS.index(k)] * to(case['g_' + k])).sum() for k in which).backward()
    res['gv'] = leaf.grad
    return res


PV_TENSORS = ('cam', 'img', 'nrm', 'gv')


# ---- texture_mapping -----------------------------------------------------------------------------------------------------

TM_MODES = ('nearest', 'bilinear')
TM_NEED = (('tex', 'uv'), ('tex',), ('uv',))
TM_TENSORS = ('out', 'g_tex', 'g_uv')
_SPECIAL = [[0., 0.], [1., 1.], [0.5, 0.5], [1., 0.], [0., 1.], [0.5, 0.], [1., 0.5]]


def _grid(us, vs):
    return [[u, v] for v in vs for u in us]


def _tm_case(name, B, C, th, tw, n, seed, fixed=(), dense=None, conditioned=True):
    """`fixed` coordinates lead every batch item, random ones in [-0.2, 1.2] fill up to n; dense = (h, w) with h * w == n"""
    g = _gen(seed)
    uv = _rand((B, n, 2), g, -0.2, 1.2)
    if len(fixed):
        fx = torch.tensor(list(fixed), dtype=torch.float64)[:n]
        uv[:, :fx.shape[0]] = r32(fx)
    if dense is not None:
        assert dense[0] * dense[1] == n
        uv = uv.reshape(B, dense[0], dense[1], 2)
    return dict(name=name, conditioned=conditioned, tex=_rand((B, C, th, tw), g, -1., 2.), uv=uv.contiguous(),
                go=_rand(tuple(uv.shape[:-1]) + (C,), g, -1., 1.))


@functools.lru_cache(maxsize=None)
def tm_cases():
    half, quarters = [0., 0.5, 1.], [0.25, 0.5, 0.75]
    cases = [
        _tm_case('t1x1_c1_n1', 1, 1, 1, 1, 1, 61, fixed=[[0.3, 0.6]]),
        _tm_case('t1x1_c3_n9', 1, 3, 1, 1, 9, 62, fixed=_SPECIAL),                 # the lone texel IS the first and last centre
        _tm_case('t1x5_c3_n255_b3', 3, 3, 1, 5, 255, 63, fixed=_SPECIAL),
        # 2 x 2: edges k / 2 (u = 0.5 -> source index 0.5: a tie) and the centres 0.25, 0.75 = the first and last (index 0 and 1)
        _tm_case('t2x2_c5_n257', 1, 5, 2, 2, 257, 64, fixed=_SPECIAL + _grid(half, half) + _grid([0.25, 0.75], [0.25, 0.75]) +
                 _grid([0.25, 0.75], [0.4]) + _grid([0.6], [0.25, 0.75])),
        # 4 x 6: v = k / 4 -> source rows 2.5, 1.5, 0.5 (ties -> 2, 2, 0), u = 0.5 -> column 2.5 (tie -> 2); the row centres
        # (j + 0.5) / 4 are exact, the first and last among them
        _tm_case('t4x6_c3_dense_b3', 3, 3, 4, 6, 63, 65, dense=(9, 7), fixed=_SPECIAL + _grid([0.5, 0.3, 0.9], quarters) +
                 _grid([0.5, 0.7], [0.125, 0.375, 0.625, 0.875])),
        _tm_case('t17x23_c3_n257_b3', 3, 3, 17, 23, 257, 66, fixed=_SPECIAL),
        _tm_case('t17x23_c1_dense', 1, 1, 17, 23, 35, 67, dense=(5, 7), fixed=_SPECIAL),
        _tm_case('t2x2_c3_n2000', 1, 3, 2, 2, 2000, 68),
        _tm_case('centres_inexact', 1, 3, 4, 6, 24, 69, conditioned=False,
                 fixed=_grid([(i + 0.5) / 6 for i in range(6)], [(j + 0.5) / 4 for j in range(4)])),
    ]
    return {c['name']: c for c in cases}


TM_KERNEL_SET = ('t1x1_c1_n1', 't1x1_c3_n9', 't1x5_c3_n255_b3', 't2x2_c5_n257', 't4x6_c3_dense_b3', 't17x23_c3_n257_b3',
                 't17x23_c1_dense', 't2x2_c3_n2000', 'centres_inexact')
TM_PINNED = tuple([(c, m, TM_NEED[0]) for c in ('t1x1_c1_n1', 't1x1_c3_n9', 't2x2_c5_n257', 't4x6_c3_dense_b3', 't17x23_c1_dense',
                                                 'centres_inexact') for m in TM_MODES] +
                  [('t4x6_c3_dense_b3', 'bilinear', need) for need in TM_NEED[1:]])
TM_TIE_CASES = ('t2x2_c5_n257', 't4x6_c3_dense_b3')


def tm_source_index(case, dtype=torch.float64):
    """grid_sample's unclipped source index (x, y) of every coordinate, in `dtype` arithmetic -> (B, N, 2)"""
    th, tw = case['tex'].shape[2:]
    uv = torch.clamp(case['uv'].reshape(case['uv'].shape[0], -1, 2).to(dtype), 0., 1.)
    gx, gy = uv[..., 0] * 2 - 1, -(uv[..., 1] * 2 - 1)
    return torch.stack([((gx + 1) * tw - 1) / 2, ((gy + 1) * th - 1) / 2], dim=-1)


def tm_run(fn, case, mode, dtype, device='cpu', need=TM_NEED[0]):
    """fn(uv, texture_maps, mode) -> dict out, g_tex, g_uv (None when not asked for), node"""
    uv, tex = _leaf(case['uv'], dtype, device, 'uv' in need), _leaf(case['tex'], dtype, device, 'tex' in need)
    out = fn(uv, tex, mode)
    (out * case['go'].to(dtype).to(device)).sum().backward()
    return dict(out=out.detach(), g_tex=tex.grad, g_uv=uv.grad, node=out.grad_fn)


# ---- mask_iou ------------------------------------------------------------------------------------------------------------

MI_SHAPES = ((1, 1, 1), (1, 7, 5), (5, 33, 31), (2, 127, 129), (1, 129, 127))
MI_NEED = (('lhs', 'rhs'), ('lhs',), ('rhs',))
MI_TENSORS = ('loss', 'g_lhs', 'g_rhs')


def _mi_case(name, shape, seed):
    g = _gen(seed)
    return dict(name=name, conditioned=True, views=False, lhs=_rand(shape, g),
                rhs=(torch.rand(shape, generator=g, dtype=torch.float64) > 0.5).to(torch.float64))


@functools.lru_cache(maxsize=None)
def mi_cases():
    cases = [_mi_case('s' + 'x'.join(map(str, s)), s, 80 + i) for i, s in enumerate(MI_SHAPES)]
    g = _gen(90)
    hard = (torch.rand(9, 11, generator=g, dtype=torch.float64) > 0.4).to(torch.float64)
    kinds = dict(name='kinds', conditioned=True, views=False,
                 lhs=torch.stack([torch.zeros(9, 11, dtype=torch.float64), hard, torch.zeros(9, 11, dtype=torch.float64), _rand((9, 11), g)]),
                 rhs=torch.stack([torch.zeros(9, 11, dtype=torch.float64), hard, torch.ones(9, 11, dtype=torch.float64), _rand((9, 11), g)]))
    # lhs = base.transpose(1, 2) is (3, 7, 5); rhs = one row per item expanded over the 7 rows
    views = dict(name='views', conditioned=True, views=True, lhs=_rand((3, 5, 7), g), rhs=_rand((3, 1, 5), g))
    return {c['name']: c for c in cases + [kinds, views]}


MI_KERNEL_SET = tuple('s' + 'x'.join(map(str, s)) for s in MI_SHAPES) + ('kinds', 'views')
MI_PINNED = tuple([(c, MI_NEED[0]) for c in ('s1x1x1', 's1x7x5', 'kinds', 'views')] + [('kinds', need) for need in MI_NEED[1:]])


def mi_run(fn, case, dtype, device='cpu', need=MI_NEED[0]):
    """fn(lhs_mask, rhs_mask) -> dict loss, g_lhs, g_rhs (of the leaves: the base of the views), node"""
    lhs, rhs = _leaf(case['lhs'], dtype, device, 'lhs' in need), _leaf(case['rhs'], dtype, device, 'rhs' in need)
    a, b = (lhs.transpose(1, 2), rhs.expand(-1, lhs.shape[2], -1)) if case['views'] else (lhs, rhs)
    loss = fn(a, b)
    (loss * MI_UPSTREAM).backward()
    return dict(loss=loss.detach(), g_lhs=lhs.grad, g_rhs=rhs.grad, node=loss.grad_fn)


# ---- the pinned chains as the reference, and the bound --------------------------------------------------------------------

def _chains():
    from kaolin_amd.metrics.render import _mask_iou_torch
    from kaolin_amd.render.mesh.utils import _prepare_vertices_torch, _texture_mapping_torch
    return _prepare_vertices_torch, _texture_mapping_torch, _mask_iou_torch


def _triple(run, names):
    r64, r32_ = run(torch.float64), run(torch.float32)
    ref64 = {k: r64[k] for k in names if r64[k] is not None}
    ref32 = {k: r32_[k] for k in names if r32_[k] is not None}
    e32 = {k: (float((ref32[k].double() - ref64[k]).abs().max()) if ref64[k].numel() else 0.) for k in ref64}
    return ref64, ref32, e32


@functools.lru_cache(maxsize=None)
def pv_reference(name, camera, layout, which=PV_WHICH[0]):
    chain = _chains()[0]
    return _triple(lambda dt: pv_run(chain, pv_cases()[name], camera, layout, dt, which=which), PV_TENSORS)


@functools.lru_cache(maxsize=None)
def tm_reference(name, mode, need=TM_NEED[0]):
    chain = _chains()[1]
    return _triple(lambda dt: tm_run(chain, tm_cases()[name], mode, dt, need=need), TM_TENSORS)


@functools.lru_cache(maxsize=None)
def mi_reference(name, need=MI_NEED[0]):
    chain = _chains()[2]
    return _triple(lambda dt: mi_run(chain, mi_cases()[name], dt, need=need), MI_TENSORS)


def mismatch(x, ref64, e32, dtype):
    """-> (worst |x - ref64| / bound over the elements, message or None).  The bound of the module's head; an element whose
    bound is 0 passes only when it is equal (ratio 0) and fails with ratio inf otherwise; a NaN fails."""
    rel, floor = (F32_REL, F32_FLOOR) if dtype == torch.float32 else (F64_REL, F64_FLOOR)
    x = x.detach().cpu().double()
    if x.shape != ref64.shape:
        return math.inf, f'shape {tuple(x.shape)} vs {tuple(ref64.shape)}'
    if x.numel() == 0:
        return 0., None
    err = (x - ref64).abs()
    bound = rel * ref64.abs() + floor * e32
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp(min=1e-300))
    bad = ~(err <= bound)                                   # (a NaN fails)
    worst = math.inf if bool(torch.isnan(err).any()) else float(ratio.max())
    if not bool(bad.any()):
        return worst, None
    i = int(torch.where(bad, torch.nan_to_num(ratio, nan=math.inf), torch.zeros_like(err)).reshape(-1).argmax())
    return worst, (f'{int(bad.sum())} of {x.numel()} elements outside {rel:g} |ref| + {floor:g} * {e32:.3e}; worst at flat index {i}: '
                   f'{float(x.reshape(-1)[i])!r} vs {float(ref64.reshape(-1)[i])!r}, {float(ratio.reshape(-1)[i]):.3g} x the bound')


def unreferenced_vertices(case):
    used = torch.zeros(case['verts1'].shape[1], dtype=torch.bool)
    used[case['faces'].reshape(-1)] = True
    return ~used


# ---- the fixture ---------------------------------------------------------------------------------------------------------

def pv_tag(name, camera, layout, which):
    return f'pv__{name}__{camera}__{layout}__{"-".join(which)}'


def tm_tag(name, mode, need):
    return f'tm__{name}__{mode}__{"-".join(need)}'


def mi_tag(name, need):
    return f'mi__{name}__{"-".join(need)}'


PV_INPUTS = ('faces', 'verts1', 'vertsB', 'rot', 'trans', 'transform', 'proj', 'g_cam', 'g_img', 'g_nrm')
TM_INPUTS = ('tex', 'uv', 'go')
MI_INPUTS = ('lhs', 'rhs')


def load_fixture():
    z = np.load(FIXTURE)
    return {k: torch.from_numpy(z[k]) for k in z.files}
