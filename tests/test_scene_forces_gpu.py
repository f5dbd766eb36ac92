"""kaolin_amd.physics.scene_forces on the GPU (csrc/scene_forces.hip, float32) against the float64 torch definition on the same
float32 values.

The yardstick is that of test_physics_gpu.py: e = max|X - X64| / max|X64| per quantity, e_hip <= 4 max(e_def, u) with e_def the
same measure for the float32 torch definition (dense B and matmul, not the code under test), u = 2^-24, and e_def < 1e-4 so
that the yardstick cannot go soft.  Asserted on the inputs: in float64 no point lies within 1e-3 of the floor along its axis (the
Hessian jumps there, so a float32 classification flip would say nothing about the kernel), and every energy is a sum of positive
terms.  Every figure is printed before it is asserted (pytest -s)."""
import functools

import pytest
import torch

from kaolin_amd import _C
from kaolin_amd.physics import reduced_scene_terms, scene_forces
from test_scene_forces_cpu import HEIGHT, TERMS, floor_margin, make_scene, scene_args, skinned

pytestmark = pytest.mark.gpu

CR = _C.physics.scene_chunk_rows()
SLICE = {H: _C.physics.scene_slice_rows(CR, H) for H in (1, 4, 5, 17)}
P = 5   # pins: the point / pin boundary falls strictly inside a chunk at every row count below
ROWS = [(R, H) for H in (5, 17) for R in (CR - 1, CR, CR + 1, SLICE[H] - 1, SLICE[H], SLICE[H] + 1)]
ROWS += [(R, H) for H in (1, 4) for R in (CR + 1, SLICE[H] + 1)]
CASES = [(R, H, P, 'all') for R, H in ROWS] + [(SLICE[5] + 1, 5, 0, 'all')] + [(SLICE[5] + 1, 5, P, name) for name in TERMS if name != 'all']


def run(s, name, **kw):
    args, kwargs = scene_args(s, TERMS[name], **kw)
    return reduced_scene_terms(*args, **kwargs), args, kwargs


@functools.lru_cache(maxsize=None)
def scene_case(R, H, pins, name, axis=1, flip=False, zero_z=False):
    """A scene of R rows with its input conditions asserted -> (scene, the definition in float64)"""
    assert _C.physics.scene_slice_rows(R, H) == SLICE[H] and (pins == 0 or (R - pins) % CR != 0)
    s = make_scene(R - pins, H, pins, seed=100 * H + R + axis, axis=axis, flip=flip, zero_z=zero_z)
    margin = floor_margin(s)
    assert (margin[1:] if zero_z else margin).min() >= 1e-3 and (not zero_z or margin[0] == 0)
    return s, run(s, name)[0]


@functools.lru_cache(maxsize=None)
def results(*case):
    """(HIP float32, the definition in float32 on the same GPU tensors, the definition in float64, the HIP call's arguments)"""
    s, ref = scene_case(*case)
    hip, args, kwargs = run(s, case[3], dtype=torch.float32, device='cuda')
    definition = scene_forces._reduced_scene_definition(*scene_forces._scene_arguments(*args, kwargs['inertia']), kwargs['pe_scale'], True)
    return hip, definition, ref, (args, kwargs)


def check(name, hip, definition, ref):
    scale = ref.abs().max().item() or 1.0   # a reference of zeros: the absolute error, so exact zeros are asked for
    e_hip, e_def = ((x.double().cpu() - ref).abs().max().item() / scale for x in (hip, definition))
    print(f'{name}: e_hip {e_hip:.3e} e_def {e_def:.3e}')
    assert torch.isfinite(hip).all() and e_def < 1e-4 and e_hip <= 4 * max(e_def, 2.0 ** -24), (name, e_hip, e_def)


def check_structure(K, H):
    blocks = K.reshape(H, 3, 4, H, 3, 4)
    assert torch.equal(K, K.T) and all(not blocks[:, b, :, :, bp].any() for b in range(3) for bp in range(3) if b != bp)


@pytest.mark.parametrize('R,H,pins,name', CASES)
def test_reduced_scene_terms(R, H, pins, name):
    hip, definition, ref, _ = results(R, H, pins, name)
    assert hip[0].shape == (1,) and hip[1].shape == (12 * H,) and hip[2].shape == (12 * H, 12 * H)
    for q, h, x, r in zip('EgK', hip, definition, ref):
        if name == 'gravity' and q == 'K':
            assert not h.any() and not r.any()
        else:
            check(f'{name} {q} R={R} H={H} pins={pins}', h, x, r)
    check_structure(hip[2], H)


@pytest.mark.parametrize('axis,flip', [(0, True), (2, False)])
def test_floor_axes_and_point_on_floor(axis, flip):
    """z = 0 and point 0 exactly on the floor: inactive under the strict comparison, whichever side is penalised"""
    H = 4
    hip, definition, ref, gpu = results(CR + 1, H, 0, 'floor', axis, flip, True)
    for q, h, x, r in zip('EgK', hip, definition, ref):
        check(f'floor axis {axis} flip {flip} {q}', h, x, r)
    check_structure(hip[2], H)
    floor, pts = gpu[0][3][0][0], gpu[0][1]
    assert not floor.hessian(torch.zeros_like(pts), pts, 1.0)[0].any() and floor.hessian(torch.zeros_like(pts), pts, 1.0).any()


def test_forms_and_repeats():
    hip, _, _, gpu = results(SLICE[5] + 1, 5, P, 'all')
    again = reduced_scene_terms(*gpu[0], **gpu[1])
    E2, g2, K2 = reduced_scene_terms(*gpu[0], hessian=False, **gpu[1])
    assert all(torch.equal(a, b) for a, b in zip(again, hip)) and K2 is None and torch.equal(E2, hip[0]) and torch.equal(g2, hip[1])


@pytest.mark.parametrize('N', [1, 63, 64, 65])
def test_classes(N):
    """The per-point terms of the three classes (the boundary's with a duplicate pin and a pin on point N - 1)"""
    s = make_scene(N, 2, min(N + 1, 7), seed=N, axis=0)
    dx = skinned(s, s['z']).float().double()
    assert ((s['pts'] + dx)[:, 0] - HEIGHT).abs().min() >= 1e-3
    for kind in ('gravity', 'floor', 'boundary'):
        objs = []
        for kw in (dict(dtype=torch.float32, device='cuda'), dict(dtype=torch.float32), dict()):
            obj = scene_args(s, (kind,), **kw)[0][3][-1][0]
            if kind == 'boundary':
                obj.set_pinned(s['idx'].to(kw.get('device', 'cpu')), s['y'].to(**kw))
            objs.append((obj, dx.to(**kw), s['pts'].to(**kw)))
        for which, shape in (('energy', (1,)), ('gradient', (N, 3)), ('hessian', (N, 3, 3))):
            hip, definition, ref = (getattr(o, which)(d, x, 1.5) for o, d, x in objs)
            assert hip.shape == shape and hip.is_cuda
            if kind == 'gravity' and which == 'hessian':
                assert not hip.any()
            else:
                check(f'{kind} {which} N={N}', hip, definition, ref)
        assert torch.equal(objs[0][0].gradient(*objs[0][1:], 1.5), objs[0][0].gradient(*objs[0][1:], 1.5))
