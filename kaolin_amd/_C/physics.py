"""Host shims of csrc/physics.hip, csrc/skinning_mlp.hip, csrc/skinning_mlp_backward.hip, csrc/simplicits_loss.hip, csrc/collisions.hip, csrc/scene_forces.hip and csrc/spd_solve.hip (no reference operator: the reference runs NVIDIA Warp kernels, a dense torch reduction and torch.linalg.solve).
Every argument is a contiguous float32 (indices: int32) tensor on one GPU; shapes are checked by the public layer, kaolin_amd/physics."""
import ctypes

import torch

from .. import _lib
from .._checks import torch_check


def _f32_cuda(fn, **tensors):
    dev = None
    for name, t in tensors.items():
        torch_check(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(),
                    f'{fn}: {name} must be a contiguous float CUDA tensor')
        torch_check(dev is None or t.device == dev, f'{fn}: {name} is on another device')
        dev = t.device
    return dev


def chunk_points():
    """Points of one staging step of the reduced kernel"""
    return int(_lib.load().kamd_physics_chunk_points())


def slice_points(num_points, num_handles):
    """Points of one slice (= one partial sum) of the reduced kernel at this size"""
    return int(_lib.load().kamd_physics_slice_points(num_points, num_handles))


def max_handles():
    """The most handles the reduced kernel takes (its LDS image)"""
    return int(_lib.load().kamd_physics_max_handles())


def neohookean_cuda(defo_grads, mu, lam, vol, coeff, energy=True, gradient=True, hessian=True):
    """defo_grads (N, 3, 3), mu, lam, vol (N) -> (energy (1), gradient (N, 3, 3), hessian (N, 9, 9)), each scaled by
    vol * coeff; None where not asked for.  N == 0 returns zeros without a launch."""
    fn = 'neohookean_cuda'
    dev = _f32_cuda(fn, defo_grads=defo_grads, mu=mu, lam=lam, vol=vol)
    N = defo_grads.size(0)
    torch_check(tuple(defo_grads.shape) == (N, 3, 3) and mu.shape == lam.shape == vol.shape == (N,),
                f'{fn}: defo_grads must be of size {{num_points, 3, 3}} and mu, lam, vol of size {{num_points}}')
    lib = _lib.load()
    with _lib.on_device(dev):
        E = torch.zeros(1, dtype=torch.float32, device=dev) if energy else None
        G = torch.empty((N, 3, 3), dtype=torch.float32, device=dev) if gradient else None
        Hs = torch.empty((N, 9, 9), dtype=torch.float32, device=dev) if hessian else None
        if N > 0:
            ws = _lib.workspace(lib.kamd_physics_neohookean_workspace(N), dev) if energy else None
            _lib.check(lib.kamd_physics_neohookean_f32(_lib.stream_ptr(dev), N, _lib.ptr(defo_grads), _lib.ptr(mu), _lib.ptr(lam),
                                                       _lib.ptr(vol), float(coeff), _lib.ptr(E), _lib.ptr(G), _lib.ptr(Hs),
                                                       _lib.ptr(ws)), fn)
    return E, G, Hs


def reduced_neohookean_cuda(z, pts, weights, weights_jac, mu, lam, vol, coeff, hessian=True):
    """z (12 H), pts (N, 3), weights (N, H), weights_jac (N, H, 3), mu, lam, vol (N), N >= 1, H <= max_handles()
    -> (E (1), g (12 H), K (12 H, 12 H) or None)"""
    fn = 'reduced_neohookean_cuda'
    dev = _f32_cuda(fn, z=z, pts=pts, weights=weights, weights_jac=weights_jac, mu=mu, lam=lam, vol=vol)
    torch_check(weights.dim() == 2, f'{fn}: weights must be of size {{num_points, num_handles}}')
    N, H = weights.shape
    torch_check(N >= 1 and 1 <= H <= max_handles(), f'{fn}: needs a point and 1 to {max_handles()} handles')
    torch_check(tuple(z.shape) == (12 * H,) and tuple(pts.shape) == (N, 3) and tuple(weights_jac.shape) == (N, H, 3) and
                mu.shape == lam.shape == vol.shape == (N,), f'{fn}: sizes do not agree')
    D = 12 * H
    lib = _lib.load()
    with _lib.on_device(dev):
        E = torch.empty(1, dtype=torch.float32, device=dev)
        g = torch.empty(D, dtype=torch.float32, device=dev)
        K = torch.empty((D, D), dtype=torch.float32, device=dev) if hessian else None
        nbytes = lib.kamd_physics_reduced_workspace(N, H, int(bool(hessian)))
        ws = _lib.workspace(nbytes, dev)
        _lib.check(lib.kamd_physics_reduced_neohookean_f32(
            _lib.stream_ptr(dev), N, H, _lib.ptr(z), _lib.ptr(pts), _lib.ptr(weights), _lib.ptr(weights_jac), _lib.ptr(mu),
            _lib.ptr(lam), _lib.ptr(vol), float(coeff), int(bool(hessian)), _lib.ptr(E), _lib.ptr(g), _lib.ptr(K), _lib.ptr(ws),
            nbytes), fn)
    return E, g, K


def skinning_max_groups():
    """The most workgroups of one skinning_mlp_cuda launch; each strides over tiles of 64 points"""
    return int(_lib.load().kamd_physics_skinning_max_groups())


def skinning_mlp_cuda(pts, bb_min, bb_max, params, width, num_layers, num_handles):
    """pts (N, 3), N >= 1, bb_min, bb_max (3), params: the Linear layers of Linear(3, width), ELU, (Linear(width, width), ELU) x
    num_layers, Linear(width, num_handles - 1), as a list of (weight, bias) -> (weights (N, num_handles), weights_jac
    (N, num_handles, 3)) with the constant handle, in one launch.  width a multiple of 16 in [16, 128], num_handles in
    [2, max_handles()]."""
    fn = 'skinning_mlp_cuda'
    sizes = [(width, 3)] + [(width, width)] * num_layers + [(num_handles - 1, width)]
    torch_check(len(params) == len(sizes) and all(tuple(w.shape) == s and tuple(b.shape) == s[:1] for (w, b), s in zip(params, sizes)),
                f'{fn}: params must be (weight, bias) of sizes {sizes}')
    packed = torch.cat([t.detach().reshape(-1) for wb in params for t in wb])
    dev = _f32_cuda(fn, pts=pts, bb_min=bb_min, bb_max=bb_max, params=packed)
    N = pts.size(0)
    torch_check(tuple(pts.shape) == (N, 3) and N >= 1 and tuple(bb_min.shape) == tuple(bb_max.shape) == (3,),
                f'{fn}: pts must be of size {{num_points >= 1, 3}} and bb_min, bb_max of size {{3}}')
    torch_check(width % 16 == 0 and 16 <= width <= 128 and num_layers >= 0 and 2 <= num_handles <= max_handles(),
                f'{fn}: needs a width in 16, 32 ... 128 and 2 to {max_handles()} handles')
    lib = _lib.load()
    with _lib.on_device(dev):
        weights = torch.empty((N, num_handles), dtype=torch.float32, device=dev)
        weights_jac = torch.empty((N, num_handles, 3), dtype=torch.float32, device=dev)
        _lib.check(lib.kamd_physics_skinning_mlp_f32(_lib.stream_ptr(dev), N, width, num_layers, num_handles, _lib.ptr(pts),
                                                     _lib.ptr(bb_min), _lib.ptr(bb_max), _lib.ptr(packed), _lib.ptr(weights),
                                                     _lib.ptr(weights_jac)), fn)
    return weights, weights_jac


def skinning_elu_cuda(y):
    """y (n) -> (elu(y), elu'(y)) as csrc/skinning_mlp.hip evaluates them (a measuring hook: tools/time_skinning.py)"""
    fn = 'skinning_elu_cuda'
    dev = _f32_cuda(fn, y=y)
    lib = _lib.load()
    with _lib.on_device(dev):
        a, d = torch.empty_like(y), torch.empty_like(y)
        _lib.check(lib.kamd_debug_skinning_elu(_lib.stream_ptr(dev), y.numel(), _lib.ptr(y), _lib.ptr(a), _lib.ptr(d)), fn)
    return a, d


# ---- csrc/skinning_mlp_backward.hip, csrc/simplicits_loss.hip: training --------------------------------------------------------------
def skinning_train_max_groups():
    """The most workgroups (= partial gradient images) of the training launches; each strides over tiles of 64 points"""
    return int(_lib.load().kamd_physics_skinning_train_max_groups())


def _train_sizes(fn, pts, packed, width, num_layers, num_handles):
    dev = _f32_cuda(fn, pts=pts, params=packed)
    N = pts.size(0)
    torch_check(tuple(pts.shape) == (N, 3) and N >= 1, f'{fn}: pts must be of size {{num_points >= 1, 3}}')
    torch_check(width % 16 == 0 and 16 <= width <= 64 and num_layers >= 0 and 2 <= num_handles <= max_handles(),
                f'{fn}: needs a width in 16, 32, 48, 64 and 2 to {max_handles()} handles')
    torch_check(packed.numel() == 4 * width + num_layers * (width * width + width) + (num_handles - 1) * (width + 1),
                f'{fn}: params must be every Linear in order, weight then bias, flat')
    return dev, N


def skinning_mlp_forward_save_cuda(pts, packed, width, num_layers, num_handles):
    """The network of skinning_mlp_cuda on pts (N, 3) as they are, without the constant handle; packed: its parameters, flat ->
    (weights (N, num_handles - 1), weights_jac (N, num_handles - 1, 3), stash for skinning_mlp_backward_cuda).  width <= 64."""
    fn = 'skinning_mlp_forward_save_cuda'
    dev, N = _train_sizes(fn, pts, packed, width, num_layers, num_handles)
    lib = _lib.load()
    with _lib.on_device(dev):
        weights = torch.empty((N, num_handles - 1), dtype=torch.float32, device=dev)
        weights_jac = torch.empty((N, num_handles - 1, 3), dtype=torch.float32, device=dev)
        stash = torch.empty(lib.kamd_physics_skinning_stash_workspace(N, width, num_layers) // 4, dtype=torch.float32, device=dev)
        _lib.check(lib.kamd_physics_skinning_forward_save_f32(_lib.stream_ptr(dev), N, width, num_layers, num_handles, _lib.ptr(pts),
                                                              _lib.ptr(packed), _lib.ptr(weights), _lib.ptr(weights_jac),
                                                              _lib.ptr(stash)), fn)
    return weights, weights_jac, stash


def skinning_mlp_backward_cuda(pts, packed, stash, grad_weights, grad_weights_jac, width, num_layers, num_handles):
    """The reverse pass of skinning_mlp_forward_save_cuda: gradients of its two outputs -> the gradient of `packed`, flat"""
    fn = 'skinning_mlp_backward_cuda'
    dev, N = _train_sizes(fn, pts, packed, width, num_layers, num_handles)
    torch_check(_f32_cuda(fn, stash=stash, grad_weights=grad_weights, grad_weights_jac=grad_weights_jac) == dev,
                f'{fn}: the gradients are on another device')
    lib = _lib.load()
    torch_check(tuple(grad_weights.shape) == (N, num_handles - 1) and tuple(grad_weights_jac.shape) == (N, num_handles - 1, 3) and
                stash.numel() * 4 == lib.kamd_physics_skinning_stash_workspace(N, width, num_layers), f'{fn}: sizes do not agree')
    with _lib.on_device(dev):
        grad = torch.empty_like(packed)
        nbytes = lib.kamd_physics_skinning_backward_workspace(N, width, num_layers, num_handles)
        ws = _lib.workspace(nbytes, dev)
        _lib.check(lib.kamd_physics_skinning_backward_f32(_lib.stream_ptr(dev), N, width, num_layers, num_handles, _lib.ptr(pts),
                                                          _lib.ptr(packed), _lib.ptr(stash), _lib.ptr(grad_weights),
                                                          _lib.ptr(grad_weights_jac), _lib.ptr(grad), _lib.ptr(ws), nbytes), fn)
    return grad


def _loss_sizes(fn, weights, weights_jac, pts, transforms, mu, lam):
    """B == 0 (transforms None): the orthogonality loss alone, of `weights` alone"""
    torch_check(weights.dim() == 2, f'{fn}: weights must be of size {{num_points, num_weights}}')
    N, HP = weights.shape
    torch_check(N >= 1 and 1 <= HP <= max_handles() - 1, f'{fn}: needs a point and 1 to {max_handles() - 1} weights')
    if transforms is None:
        return _f32_cuda(fn, weights=weights), N, 0, HP
    dev = _f32_cuda(fn, weights=weights, weights_jac=weights_jac, pts=pts, transforms=transforms, mu=mu, lam=lam)
    B = transforms.size(0)
    torch_check(B >= 1 and tuple(transforms.shape) == (B, HP, 3, 4) and tuple(weights_jac.shape) == (N, HP, 3) and
                tuple(pts.shape) == (N, 3) and mu.shape == lam.shape == (N,), f'{fn}: sizes do not agree')
    return dev, N, B, HP


def simplicits_loss_cuda(weights, weights_jac, pts, transforms, mu, lam, interp, scale_le, scale_lo):
    """weights (N, H'), weights_jac (N, H', 3), pts (N, 3), transforms (B, H', 3, 4), mu, lam (N) -> (le (), lo (), G - I (H', H'))
    of csrc/simplicits_loss.hip; transforms None: lo alone (le = 0), the other inputs unread"""
    fn = 'simplicits_loss_cuda'
    dev, N, B, HP = _loss_sizes(fn, weights, weights_jac, pts, transforms, mu, lam)
    opt = [_lib.ptr(t) if B else None for t in (weights_jac, pts, transforms, mu, lam)]
    lib = _lib.load()
    with _lib.on_device(dev):
        le = torch.empty((), dtype=torch.float32, device=dev)
        lo = torch.empty((), dtype=torch.float32, device=dev)
        gmi = torch.empty((HP, HP), dtype=torch.float32, device=dev)
        nbytes = lib.kamd_physics_simplicits_loss_workspace(N, HP)
        ws = _lib.workspace(nbytes, dev)
        _lib.check(lib.kamd_physics_simplicits_loss_f32(_lib.stream_ptr(dev), N, B, HP, _lib.ptr(weights), *opt, float(interp),
                                                        float(scale_le), float(scale_lo), _lib.ptr(le), _lib.ptr(lo), _lib.ptr(gmi),
                                                        _lib.ptr(ws), nbytes), fn)
    return le, lo, gmi


def simplicits_loss_backward_cuda(weights, weights_jac, pts, transforms, mu, lam, interp, scale_le, scale_lo, gmi, grad_le, grad_lo):
    """The gradient of simplicits_loss_cuda: grad_le, grad_lo (one float each, on the device) -> (grad_weights, grad_weights_jac)"""
    fn = 'simplicits_loss_backward_cuda'
    dev, N, B, HP = _loss_sizes(fn, weights, weights_jac, pts, transforms, mu, lam)
    torch_check(_f32_cuda(fn, gmi=gmi, grad_le=grad_le, grad_lo=grad_lo) == dev and tuple(gmi.shape) == (HP, HP) and
                grad_le.numel() == grad_lo.numel() == 1, f'{fn}: needs G - I of size {{{HP}, {HP}}} and two scalar gradients')
    opt = [_lib.ptr(t) if B else None for t in (weights_jac, pts, transforms, mu, lam)]
    lib = _lib.load()
    with _lib.on_device(dev):
        grad_w = torch.empty((N, HP), dtype=torch.float32, device=dev)
        grad_j = torch.empty((N, HP, 3), dtype=torch.float32, device=dev)
        _lib.check(lib.kamd_physics_simplicits_loss_backward_f32(_lib.stream_ptr(dev), N, B, HP, _lib.ptr(weights), *opt,
                                                                 float(interp), float(scale_le), float(scale_lo), _lib.ptr(gmi),
                                                                 _lib.ptr(grad_le), _lib.ptr(grad_lo), _lib.ptr(grad_w),
                                                                 _lib.ptr(grad_j)), fn)
    return grad_w, grad_j


# ---- csrc/collisions.hip ----------------------------------------------------------------------------------------------------------------
def _i32_cuda(fn, dev, **tensors):
    for name, t in tensors.items():
        torch_check(t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.device == dev,
                    f'{fn}: {name} must be a contiguous int CUDA tensor on the device of the others')


def collision_chunk_contacts():
    """Contacts of one staging step of the reduced collision kernel"""
    return int(_lib.load().kamd_collision_chunk_contacts())


def collision_slice_contacts(num_contacts, num_handles):
    """Contacts of one slice (= one partial sum) of the reduced collision kernel at this size"""
    return int(_lib.load().kamd_collision_slice_contacts(num_contacts, num_handles))


def collision_detect_cuda(dx, x0, obj_ids, is_static, detection_radius, immune_radius, max_pairs):
    """dx, x0 (N, 3), obj_ids, is_static (N) int32, N >= 1, max_pairs >= 1 -> (number of contacts found, indices_a, indices_b (C)
    int32, normals, gaps (C, 3), pair_objects (C, 2) int32) for the C = min(found, max_pairs) smallest (a, b), sorted.  ONE host read: not capturable."""
    fn = 'collision_detect_cuda'
    dev = _f32_cuda(fn, dx=dx, x0=x0)
    _i32_cuda(fn, dev, obj_ids=obj_ids, is_static=is_static)
    N = x0.size(0)
    torch_check(N >= 1 and tuple(dx.shape) == tuple(x0.shape) == (N, 3) and tuple(obj_ids.shape) == tuple(is_static.shape) == (N,) and
                max_pairs >= 1, f'{fn}: needs dx, x0 of size {{num_points >= 1, 3}}, obj_ids, is_static of size {{num_points}}')
    lib = _lib.load()
    with _lib.on_device(dev):
        nbytes = lib.kamd_collision_detect_workspace(N)
        ws = _lib.workspace(nbytes, dev)
        counts = (ctypes.c_int64 * 2)()
        args = (_lib.ptr(x0), _lib.ptr(obj_ids), _lib.ptr(is_static), float(detection_radius), float(immune_radius), int(max_pairs),
                _lib.ptr(ws), nbytes)
        _lib.check(lib.kamd_collision_count_f32(_lib.stream_ptr(dev), N, _lib.ptr(dx), *args, counts), fn)
        total, emitted = int(counts[0]), int(counts[1])
        C = min(total, int(max_pairs))
        ia = torch.empty(C, dtype=torch.int32, device=dev)
        ib = torch.empty(C, dtype=torch.int32, device=dev)
        normals = torch.empty((C, 3), dtype=torch.float32, device=dev)
        gaps = torch.empty((C, 3), dtype=torch.float32, device=dev)
        pair_objects = torch.empty((C, 2), dtype=torch.int32, device=dev)
        if C > 0:
            ebytes = lib.kamd_collision_emit_workspace(emitted)
            es = _lib.workspace(ebytes, dev)
            _lib.check(lib.kamd_collision_emit_f32(_lib.stream_ptr(dev), N, *args, emitted, C, _lib.ptr(es), ebytes, _lib.ptr(ia),
                                                   _lib.ptr(ib), _lib.ptr(normals), _lib.ptr(gaps), _lib.ptr(pair_objects)), fn)
    return total, ia, ib, normals, gaps, pair_objects


def _contact_args(fn, dx, dx0, gaps, normals, indices_a, indices_b):
    dev = _f32_cuda(fn, dx=dx, dx0=dx0, gaps=gaps, normals=normals)
    _i32_cuda(fn, dev, indices_a=indices_a, indices_b=indices_b)
    N, C = dx.size(0), indices_a.size(0)
    torch_check(tuple(dx.shape) == tuple(dx0.shape) == (N, 3) and tuple(gaps.shape) == tuple(normals.shape) == (C, 3) and
                tuple(indices_a.shape) == tuple(indices_b.shape) == (C,), f'{fn}: sizes do not agree')
    return dev, N, C


def collision_terms_cuda(dx, dx0, gaps, normals, indices_a, indices_b, coeff, radius, barrier_ratio, mu, dt, nu, which):
    """The contact terms of C contacts among the N points of dx, dx0 (N, 3): `which` = 'energy' -> (1), 'gradient' -> (C, 3),
    'hessian' -> (C, 3, 3), scaled by coeff.  C == 0 returns zeros without a launch."""
    fn = 'collision_terms_cuda'
    dev, N, C = _contact_args(fn, dx, dx0, gaps, normals, indices_a, indices_b)
    shape = {'energy': (1,), 'gradient': (C, 3), 'hessian': (C, 3, 3)}[which]
    lib = _lib.load()
    with _lib.on_device(dev):
        out = torch.zeros(shape, dtype=torch.float32, device=dev) if C == 0 else torch.empty(shape, dtype=torch.float32, device=dev)
        if C > 0:
            ws = _lib.workspace(lib.kamd_collision_terms_workspace(C), dev) if which == 'energy' else None
            outs = [_lib.ptr(out) if which == name else None for name in ('energy', 'gradient', 'hessian')]
            _lib.check(lib.kamd_collision_terms_f32(_lib.stream_ptr(dev), C, N, _lib.ptr(dx), _lib.ptr(dx0), _lib.ptr(gaps),
                                                    _lib.ptr(normals), _lib.ptr(indices_a), _lib.ptr(indices_b), float(coeff),
                                                    float(radius), float(barrier_ratio), float(mu), float(dt), float(nu), *outs,
                                                    _lib.ptr(ws)), fn)
    return out


def collision_reduced_cuda(dx, dx0, gaps, normals, indices_a, indices_b, weights, x0, coeff, radius, barrier_ratio, mu, dt, nu,
                           hessian=True):
    """As collision_terms_cuda with weights (N, H), x0 (N, 3), C >= 1, H <= max_handles() -> (E (1), g (12 H), K (12 H, 12 H) or None)"""
    fn = 'collision_reduced_cuda'
    dev, N, C = _contact_args(fn, dx, dx0, gaps, normals, indices_a, indices_b)
    torch_check(_f32_cuda(fn, weights=weights, x0=x0) == dev and weights.dim() == 2, f'{fn}: weights must be of size {{num_points, num_handles}}')
    H = weights.size(1)
    torch_check(C >= 1 and 1 <= H <= max_handles() and tuple(weights.shape) == (N, H) and tuple(x0.shape) == (N, 3),
                f'{fn}: needs a contact, 1 to {max_handles()} handles and weights, x0 of {N} points')
    D = 12 * H
    lib = _lib.load()
    with _lib.on_device(dev):
        E = torch.empty(1, dtype=torch.float32, device=dev)
        g = torch.empty(D, dtype=torch.float32, device=dev)
        K = torch.empty((D, D), dtype=torch.float32, device=dev) if hessian else None
        nbytes = lib.kamd_collision_reduced_workspace(C, H, int(bool(hessian)))
        ws = _lib.workspace(nbytes, dev)
        _lib.check(lib.kamd_collision_reduced_f32(
            _lib.stream_ptr(dev), C, N, H, _lib.ptr(dx), _lib.ptr(dx0), _lib.ptr(gaps), _lib.ptr(normals), _lib.ptr(indices_a),
            _lib.ptr(indices_b), _lib.ptr(weights), _lib.ptr(x0), float(coeff), float(radius), float(barrier_ratio), float(mu),
            float(dt), float(nu), int(bool(hessian)), _lib.ptr(E), _lib.ptr(g), _lib.ptr(K), _lib.ptr(ws), nbytes), fn)
    return E, g, K


# ---- csrc/scene_forces.hip --------------------------------------------------------------------------------------------------------------
def scene_chunk_rows():
    """Rows (points, then pins) of one staging step of the reduced scene kernel"""
    return int(_lib.load().kamd_scene_chunk_rows())


def scene_slice_rows(num_rows, num_handles):
    """Rows of one slice (= one partial sum) of the reduced scene kernel at this size"""
    return int(_lib.load().kamd_scene_slice_rows(num_rows, num_handles))


def _scene_class_args(fn, dev, N, gravity, floor):
    """gravity (g (3 floats), rho (N), vol (N)) or None, floor (height, axis, flip, vol (N)) or None -> their C arguments, coefficients apart"""
    g, rho, gvol = gravity if gravity is not None else ((0.0, 0.0, 0.0), None, None)
    fh, axis, flip, fvol = floor if floor is not None else (0.0, 0, False, None)
    per_point = {k: t for k, t in (('density', rho), ('gravity volume', gvol), ('floor volume', fvol)) if t is not None}
    torch_check(all(_f32_cuda(fn, **{k: t}) == dev and tuple(t.shape) == (N,) for k, t in per_point.items()) and axis in (0, 1, 2),
                f'{fn}: needs density and volume of size {{{N}}} on the device of the points and a floor axis in 0, 1, 2')
    return ((_lib.ptr(rho), _lib.ptr(gvol), float(g[0]), float(g[1]), float(g[2])), (_lib.ptr(fvol), float(fh), int(axis), int(bool(flip))))


def scene_terms_cuda(dx, x0, coeff, which, gravity=None, floor=None, pins=None):
    """The terms of ONE class on dx, x0 (N, 3): gravity, floor as in _scene_class_args, pins (sorted (P) int32 ascending, order (P)
    int32, pinned_x (P, 3)), P >= 1; `which` = 'energy' -> (1), 'gradient' -> (N, 3), 'hessian' -> (N, 3, 3), scaled by coeff.
    N == 0 returns zeros without a launch."""
    fn = 'scene_terms_cuda'
    dev = _f32_cuda(fn, dx=dx, x0=x0)
    N = x0.size(0)
    torch_check(tuple(dx.shape) == tuple(x0.shape) == (N, 3) and (gravity is not None) + (floor is not None) + (pins is not None) == 1,
                f'{fn}: needs dx, x0 of size {{num_points, 3}} and one class of terms')
    gargs, fargs = _scene_class_args(fn, dev, N, gravity, floor)
    P, pargs = 0, (None, None, None)
    if pins is not None:
        _i32_cuda(fn, dev, pins_sorted=pins[0], pins_order=pins[1])
        P = pins[0].size(0)
        torch_check(_f32_cuda(fn, pinned_x=pins[2]) == dev and P >= 1 and tuple(pins[1].shape) == (P,) and
                    tuple(pins[2].shape) == (P, 3), f'{fn}: needs at least one pin and pinned_x of size {{num_pins, 3}}')
        pargs = tuple(_lib.ptr(t) for t in pins)
    shape = {'energy': (1,), 'gradient': (N, 3), 'hessian': (N, 3, 3)}[which]
    lib = _lib.load()
    with _lib.on_device(dev):
        out = torch.zeros(shape, dtype=torch.float32, device=dev) if N == 0 else torch.empty(shape, dtype=torch.float32, device=dev)
        if N > 0:
            ws = _lib.workspace(lib.kamd_scene_terms_workspace(N), dev) if which == 'energy' else None
            outs = [_lib.ptr(out) if which == name else None for name in ('energy', 'gradient', 'hessian')]
            _lib.check(lib.kamd_scene_terms_f32(_lib.stream_ptr(dev), N, _lib.ptr(dx), _lib.ptr(x0), *gargs, *fargs, P, *pargs,
                                                float(coeff), *outs, _lib.ptr(ws)), fn)
    return out


def scene_reduced_cuda(z, x0, weights, gravity=None, gravity_coeff=0.0, floor=None, floor_coeff=0.0, pins=None, inertia=None,
                       hessian=True):
    """z (12 H), x0 (N, 3), weights (N, H), H <= max_handles(); gravity, floor as in _scene_class_args with their coefficients, pins
    (indices (P) int32, pinned_x (P, 3), coefficients (P)), inertia (mass (N), z_prev (12 H), z_dot (12 H), dt); N + P >= 1
    -> (E (1), g (12 H), K (12 H, 12 H) or None)"""
    fn = 'scene_reduced_cuda'
    dev = _f32_cuda(fn, z=z, x0=x0, weights=weights)
    torch_check(weights.dim() == 2, f'{fn}: weights must be of size {{num_points, num_handles}}')
    N, H = weights.shape
    D = 12 * H
    torch_check(1 <= H <= max_handles() and tuple(z.shape) == (D,) and tuple(x0.shape) == (N, 3),
                f'{fn}: needs 1 to {max_handles()} handles, z of size {{12 num_handles}} and x0 of size {{num_points, 3}}')
    gargs, fargs = _scene_class_args(fn, dev, N, gravity, floor)
    P, pargs = 0, (None, None, None)
    if pins is not None and pins[0].size(0) > 0:
        _i32_cuda(fn, dev, pinned_indices=pins[0])
        P = pins[0].size(0)
        torch_check(_f32_cuda(fn, pinned_x=pins[1], pinned_coeff=pins[2]) == dev and tuple(pins[1].shape) == (P, 3) and
                    tuple(pins[2].shape) == (P,), f'{fn}: needs pinned_x of size {{num_pins, 3}} and a coefficient per pin')
        pargs = tuple(_lib.ptr(t) for t in pins)
    iargs = (None, None, None, 0.0)
    if inertia is not None:
        mass, z_prev, z_dot, dt = inertia
        torch_check(_f32_cuda(fn, mass=mass, z_prev=z_prev, z_dot=z_dot) == dev and tuple(mass.shape) == (N,) and
                    tuple(z_prev.shape) == tuple(z_dot.shape) == (D,), f'{fn}: needs a mass per point and z_prev, z_dot of the size of z')
        iargs = (_lib.ptr(mass), _lib.ptr(z_prev), _lib.ptr(z_dot), float(dt))
    torch_check(N + P >= 1, f'{fn}: needs a point or a pin')
    lib = _lib.load()
    with _lib.on_device(dev):
        E = torch.empty(1, dtype=torch.float32, device=dev)
        g = torch.empty(D, dtype=torch.float32, device=dev)
        K = torch.empty((D, D), dtype=torch.float32, device=dev) if hessian else None
        nbytes = lib.kamd_scene_reduced_workspace(N + P, H, int(bool(hessian)))
        ws = _lib.workspace(nbytes, dev)
        _lib.check(lib.kamd_scene_reduced_f32(
            _lib.stream_ptr(dev), N, P, H, _lib.ptr(z), _lib.ptr(x0), _lib.ptr(weights), *gargs, float(gravity_coeff), *fargs,
            float(floor_coeff), *pargs, *iargs, int(bool(hessian)), _lib.ptr(E), _lib.ptr(g), _lib.ptr(K), _lib.ptr(ws), nbytes), fn)
    return E, g, K


# ---- csrc/spd_solve.hip -----------------------------------------------------------------------------------------------------------------
def spd_panel():
    """Columns of one panel (= the tile side) of the blocked Cholesky factorisation"""
    return int(_lib.load().kamd_spd_panel())


def spd_max_n():
    """The most rows spd_factor_cuda takes: 12 max_handles()"""
    return int(_lib.load().kamd_spd_max_n())


def spd_factor_cuda(A):
    """A (n, n) symmetric positive definite, 1 <= n <= spd_max_n(); only its lower triangle is read -> (L (n, n) lower triangular
    with A = L L^T, info (1) int32: 0 or the 1-based column of the first pivot that is <= 0 or not finite, the workspace that
    spd_solve_cuda takes).  No host read."""
    fn = 'spd_factor_cuda'
    dev = _f32_cuda(fn, A=A)
    n = A.size(0)
    torch_check(tuple(A.shape) == (n, n) and 1 <= n <= spd_max_n(), f'{fn}: A must be of size {{n, n}}, n in 1 to {spd_max_n()}')
    lib = _lib.load()
    with _lib.on_device(dev):
        L = torch.empty((n, n), dtype=torch.float32, device=dev)
        info = torch.empty(1, dtype=torch.int32, device=dev)
        ws = _lib.workspace(lib.kamd_spd_workspace(n), dev)
        _lib.check(lib.kamd_spd_factor_f32(_lib.stream_ptr(dev), n, _lib.ptr(A), _lib.ptr(L), _lib.ptr(info), _lib.ptr(ws)), fn)
    return L, info, ws


def spd_solve_cuda(L, b, info, workspace):
    """L, info, workspace of spd_factor_cuda, b (n) -> x (n) with L L^T x = b (unspecified where info != 0).  No host read."""
    fn = 'spd_solve_cuda'
    dev = _f32_cuda(fn, L=L, b=b)
    n = L.size(0)
    lib = _lib.load()
    torch_check(tuple(L.shape) == (n, n) and 1 <= n <= spd_max_n() and tuple(b.shape) == (n,),
                f'{fn}: L must be of size {{n, n}}, n in 1 to {spd_max_n()}, and b of size {{n}}')
    torch_check(info.device == dev and info.dtype == torch.int32 and info.numel() == 1 and workspace is not None and
                workspace.device == dev and workspace.numel() * 8 >= lib.kamd_spd_workspace(n),
                f'{fn}: needs the info and the workspace that spd_factor_cuda returned for this L')
    with _lib.on_device(dev):
        x = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(lib.kamd_spd_solve_f32(_lib.stream_ptr(dev), n, _lib.ptr(L), _lib.ptr(b), _lib.ptr(x), _lib.ptr(info),
                                          _lib.ptr(workspace)), fn)
    return x
