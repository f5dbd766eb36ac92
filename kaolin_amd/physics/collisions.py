r"""Point-to-point contacts of a scene (the reference's kaolin/physics/common/collisions.py, on torch tensors): detection, the
barrier and friction energy of every contact with its gradient and Hessian, and their reduction to the Simplicits degrees of
freedom.  float32 tensors on a GPU run csrc/collisions.hip; everything else (CPU, float64, more handles than
``kaolin_amd._C.physics.max_handles()``) runs the torch formulation of the same contracts in this file.

**The detection contract** (the reference's contact order is the outcome of an ``atomic_add`` race; this one is fixed).  In float32,
one rounding per operation, unfused: ``pos = x0 + dx``, ``e = pos_a - pos_b``, ``d = sqrt((ex ex + ey ey) + ez ez)`` correctly
rounded, and ``R`` the Python double ``2.0 * radius * detection_ratio`` rounded once to float32.  A pair ``a < b`` is a contact iff

* ``d <= R``,
* not both points are static (the reference records such pairs), and
* not (same object and ``|x0_a - x0_b|^2 < radius * ignore_self_collision_ratio``): the reference's comparison of a squared
  length with an unsquared radius, kept literally (the product is a Python double rounded once to float32).

A NaN or infinite position is in no contact.  Stored per contact: ``normal = e / d``, or the zero vector when ``d == 0``;
``gap = dot(e, normal) normal``; ``-1`` for the index of a static point, whose displacement delta counts as zero on either side
(the reference guards side b only and reads element ``-1`` for a static side a).  The contacts are sorted by ``(a, b)``: the same
input gives the same tensors, bit for bit, on every call and on CPU and GPU alike.  With more than ``max_contacting_pairs``
contacts the first ``max_contacting_pairs`` of that order are kept and the reference's warning is logged.  No contact gives empty
tensors and ``object_pairs == []``.  ``detect_collisions`` reads the number of contacts back (one host read, and another for
``object_pairs``): it cannot be captured into a graph.  The three terms and :meth:`Collision.reduced_terms` can.
"""
import logging

import torch

from .. import _C
from .materials import _check_floating, _on_hip

__all__ = ['Collision']

_PAIR_CHUNK = 1 << 22   # (a, b) candidates of one step of the all-pairs detection


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _sqrt32(x):
    """The correctly rounded float32 root (torch's vectorised float32 sqrt on a CPU is not): through float64, whose 53 bits make the
    second rounding exact"""
    return torch.sqrt(x.double()).float()


def _detect_definition(dx, x0, obj_ids, is_static, detection_radius, immune_radius, max_pairs):
    """The detection contract over all pairs, in chunks of rows; float32 whatever the inputs are"""
    dev = x0.device
    x0, N = x0.float(), x0.shape[0]
    pos = x0 + dx.float()
    R = torch.tensor(detection_radius, dtype=torch.float32, device=dev)
    immune = torch.tensor(immune_radius, dtype=torch.float32, device=dev)
    static = is_static == 1
    index = torch.arange(N, device=dev)
    total, kept = 0, []
    step = max(1, _PAIR_CHUNK // max(N, 1))
    for s in range(0, N, step):
        rows = slice(s, min(N, s + step))
        e = pos[rows, None] - pos[None]
        mask = (_sqrt32(_dot(e, e)) <= R) & (index[None] > index[rows, None]) & ~(static[rows, None] & static[None])
        r = x0[rows, None] - x0[None]
        mask &= ~((obj_ids[rows, None] == obj_ids[None]) & (_dot(r, r) < immune))
        pairs = mask.nonzero()
        pairs[:, 0] += s
        if total < max_pairs:
            kept.append(pairs[:max_pairs - total])
        total += pairs.shape[0]
    pairs = torch.cat(kept) if kept else torch.zeros((0, 2), dtype=torch.int64, device=dev)
    a, b = pairs[:, 0], pairs[:, 1]
    e = pos[a] - pos[b]
    d = _sqrt32(_dot(e, e))[:, None]
    normals = torch.where(d == 0, torch.zeros_like(e), e / d)
    gaps = _dot(e, normals)[:, None] * normals
    ia = torch.where(static[a], -1, a).to(torch.int32)
    ib = torch.where(static[b], -1, b).to(torch.int32)
    return total, ia, ib, normals, gaps, torch.stack((obj_ids[a], obj_ids[b]), dim=1)


def _contact_offsets(dx, dx0, gaps, ia, ib):
    """(dx_a - dx0_a) + gap - (dx_b - dx0_b), the delta of a static side (-1) zero"""
    a, b = ia.long(), ib.long()
    delta = dx - dx0
    off = torch.where((a >= 0)[:, None], delta[a.clamp(min=0)] + gaps, gaps)
    return torch.where((b >= 0)[:, None], off - delta[b.clamp(min=0)], off)


def _contact_terms(offset, nor, static_b, coeff, radius, rp, mu, dt, nu, gradient=False, hessian=False):
    """The reference's three kernels as vectorised expressions -> (energy (C), gradient (C, 3) or None, hessian (C, 3, 3) or None)"""
    rc = torch.where(static_b, 1.0, 2.0).to(offset.dtype) * radius
    d = _dot(offset, nor)
    d_hat = d / rc
    active = (rp < d_hat) & (d_hat <= 1.0)
    dc, dp = d_hat - 1.0, d_hat - rp
    lg = torch.log(dp)
    barrier = 2.0 * lg
    dE = -dc * (barrier + dc / dp)
    vt = (offset - d[:, None] * nor) / dt
    vtn = torch.sqrt(_dot(vt, vt))
    mu_fn = -mu * dE / rc
    stick = vtn < 1.0
    h_vt = 0.5 * nu * vtn * vtn + torch.where(stick, vtn * vtn * (1.0 - vtn / 3.0), vtn - 1.0 / 3.0)
    zero = torch.zeros((), dtype=offset.dtype, device=offset.device)
    E = coeff * torch.where(active, -(dc * dc) * lg + mu_fn * dt * h_vt, zero)
    if not (gradient or hessian):
        return E, None, None
    f1_nu = torch.where(stick, 2.0 - vtn, 1.0 / vtn) + nu
    dbar, ddcdp = 2.0 / dp, (dp - dc) / (dp * dp)
    d2E = -(barrier + dc / dp) - dc * (dbar + ddcdp)
    G = Hs = None
    if gradient:
        G = (dE / rc)[:, None] * nor + (mu_fn * f1_nu)[:, None] * vt + (-mu * dt * h_vt * d2E / (rc * rc))[:, None] * nor
        G = coeff * torch.where(active[:, None], G, zero)
    if hessian:
        eps = 1.0e-4
        nn, vv = nor[:, :, None] * nor[:, None, :], vt[:, :, None] * vt[:, None, :]
        tangent = torch.eye(3, dtype=offset.dtype, device=offset.device) - nn
        col = lambda x: x[:, None, None]
        Hs = col(d2E / (rc * rc)) * nn
        vsafe = torch.where(vtn > 0, vtn, torch.ones_like(vtn))
        rest = col(mu_fn / dt * f1_nu) * tangent
        stick_h = col(mu_fn / dt) * (col(f1_nu) * tangent - vv / col(vsafe))
        slip_h = col(mu_fn) * (col(-1.0 / (vsafe * vsafe) / (vsafe * dt)) * vv + col(f1_nu / dt) * tangent)
        Hs = Hs + torch.where(col(vtn < eps), rest, torch.where(col(stick), stick_h, slip_h))
        Hs = Hs + col(-mu * d2E / rc * f1_nu / rc) * (vt[:, :, None] * nor[:, None, :])
        h_vt_p = torch.where(stick, nu * vtn + 2.0 * vtn - vtn * vtn, nu * vtn + 1.0)
        d2bar, dddcdp = -2.0 / (dp * dp), -2.0 * ddcdp / dp
        d3E = -(dbar + ddcdp) - (d2bar + dddcdp) * dc - (dbar + ddcdp)
        dvtn = torch.where((vtn > eps)[:, None], vt / (vsafe * dt)[:, None], zero)
        Hs = Hs + col(-mu * dt / (rc * rc)) * (col(d2E * h_vt_p) * (nor[:, :, None] * dvtn[:, None, :]) + col(h_vt * d3E / rc) * nn)
        Hs = coeff * torch.where(col(active), Hs, zero)
    return E, G, Hs


def _collision_jacobian(cp_w, cp_x0, ia, ib):
    """Dense J = J_a - J_b (3 C, 12 H): row 3 c + b of J_a holds w[a][h] (x0_a, 1) in the columns 12 h + 4 b .. 12 h + 4 b + 3"""
    C, H = ia.shape[0], cp_w.shape[1]
    xt = torch.cat([cp_x0, torch.ones_like(cp_x0[:, :1])], dim=1)

    def side(i):
        i = i.long()
        m = cp_w[i.clamp(min=0)][:, :, None] * xt[i.clamp(min=0)][:, None, :]                    # (C, H, 4)
        return torch.where((i >= 0)[:, None, None], m, torch.zeros((), dtype=m.dtype, device=m.device))
    m = side(ia) - side(ib)
    J = torch.zeros((C, 3, H, 3, 4), dtype=cp_w.dtype, device=cp_w.device)
    for b in range(3):
        J[:, b, :, b, :] = m
    return J.reshape(3 * C, 12 * H)


def _reduced_definition(G, Hs, J):
    """J^T grad and J^T blockdiag(H_c) J through the dense J"""
    C, D = G.shape[0], J.shape[1]
    return J.T @ G.reshape(3 * C), (J.T @ torch.bmm(Hs, J.reshape(C, 3, D)).reshape(3 * C, D) if Hs is not None else None)


class Collision:
    r"""Contacts between the collision points of a scene; the reference's constructor, on torch tensors.

    Args:
        dt (float): time step.
        collision_particle_radius (float): radius of a collision particle, where the penalty begins. Default: 0.1.
        detection_ratio (float): detection radius as a ratio of the particle radius. Default: 1.5.
        impenetrable_barrier_ratio (float): barrier radius as a ratio of the particle radius. Default: 0.5.
        ignore_self_collision_ratio (float): immune radius within one object, as a ratio of the particle radius (see the
            module's contract). Default: 100000.0.
        collision_penalty_stiffness (float): kept for the scene that scales the terms. Default: 100.0.
        friction_regularization (float): keeps friction forces proportional to the time step. Default: 0.1.
        friction_fluid (float): damps the friction forces. Default: 0.1.
        friction (float): friction coefficient. Default: 0.5.
        max_contacting_pairs (int): the most contacts kept. Default: 10000.
        bounds (bool): kept for the line search (:meth:`get_bounds` is not built). Default: True.
    """

    def __init__(self, dt, collision_particle_radius=0.1, detection_ratio=1.5, impenetrable_barrier_ratio=0.5,
                 ignore_self_collision_ratio=100000.0, collision_penalty_stiffness=100.0, friction_regularization=0.1,
                 friction_fluid=0.1, friction=0.5, max_contacting_pairs=10000, bounds=True):
        self.num_contacts = 0
        self.bounds = bounds
        self.collision_radius = collision_particle_radius
        self.collision_detection_ratio = detection_ratio
        self.collision_barrier_ratio = impenetrable_barrier_ratio
        self.ignore_self_collision_ratio = ignore_self_collision_ratio
        self.collision_penalty_stiffness = collision_penalty_stiffness
        self.friction_reg = friction_regularization
        self.friction_fluid = friction_fluid
        self.friction = friction
        self.dt = dt
        self.max_contacting_pairs = int(max_contacting_pairs)
        self.collision_indices_a = self.collision_indices_b = None
        self.collision_normals = self.collision_kinematic_gaps = None
        self.collision_J_dense = None
        self.cp_dx_at_nm_iteration_0 = None
        self.object_pairs = []

    def detect_collisions(self, cp_dx, cp_x0, cp_obj_ids, cp_is_static=None):
        r"""Finds the contacts of the points ``cp_x0 + cp_dx`` by the module's contract and sets ``num_contacts``,
        ``collision_indices_a``, ``collision_indices_b`` (int32, ``-1`` for a static point), ``collision_normals``,
        ``collision_kinematic_gaps`` :math:`(C, 3)`, ``cp_dx_at_nm_iteration_0`` (a clone of ``cp_dx``) and ``object_pairs``
        (the reference's array of interacting object pairs, from the object ids of every contact's two points).

        float32 tensors on a GPU run a HIP pipeline (cell sort, count, scan, emit, sort; no atomics) around one host read;
        otherwise an all-pairs mask in chunks applies the same float32 rule.  Not capturable into a graph.

        Args:
            cp_dx (torch.Tensor): displacements of the collision points, of shape :math:`(N, 3)`.
            cp_x0 (torch.Tensor): their rest positions, of shape :math:`(N, 3)`.
            cp_obj_ids (torch.Tensor): object id per point, integer, of shape :math:`(N,)`.
            cp_is_static (torch.Tensor, optional): 1 for a static point, of shape :math:`(N,)`. Default: none is static.
        """
        _check_floating(cp_dx=cp_dx, cp_x0=cp_x0)
        N = cp_x0.shape[0]
        if tuple(cp_dx.shape) != (N, 3) or tuple(cp_x0.shape) != (N, 3) or tuple(cp_obj_ids.shape) != (N,):
            raise ValueError(f'cp_dx, cp_x0 must be of shape (N, 3) and cp_obj_ids of shape (N,), got {tuple(cp_dx.shape)}, '
                             f'{tuple(cp_x0.shape)}, {tuple(cp_obj_ids.shape)}')
        cp_dx, cp_x0 = cp_dx.detach(), cp_x0.detach()
        obj_ids = cp_obj_ids.to(torch.int32)
        is_static = torch.zeros_like(obj_ids) if cp_is_static is None else cp_is_static.to(torch.int32)
        self.cp_dx_at_nm_iteration_0 = cp_dx.clone()
        R = 2.0 * self.collision_radius * self.collision_detection_ratio
        immune = self.collision_radius * self.ignore_self_collision_ratio
        if _on_hip(cp_dx, cp_x0) and N >= 1 and self.max_contacting_pairs >= 1:
            found = _C.physics.collision_detect_cuda(cp_dx.contiguous(), cp_x0.contiguous(), obj_ids.contiguous(),
                                                     is_static.contiguous(), R, immune, self.max_contacting_pairs)
        else:
            found = _detect_definition(cp_dx, cp_x0, obj_ids, is_static, R, immune, self.max_contacting_pairs)
        total, ia, ib, normals, gaps, pair_objects = found
        if total > self.max_contacting_pairs:
            logging.warning('contact buffer size exceed, some have been ignored')
        self.num_contacts = ia.shape[0]
        self.collision_indices_a, self.collision_indices_b = ia, ib
        self.collision_normals, self.collision_kinematic_gaps = normals.to(cp_dx.dtype), gaps.to(cp_dx.dtype)
        if self.num_contacts > 0:
            unique_pairs = torch.unique(pair_objects, dim=0).cpu()
            object_pairs = torch.vstack((unique_pairs[:, [0, 1]], unique_pairs[:, [1, 0]], unique_pairs[:, [0, 0]],
                                         unique_pairs[:, [1, 1]]))
            self.object_pairs = torch.unique(object_pairs, dim=0).numpy()
        else:
            self.object_pairs = []

    def calculate_jacobian(self, cp_w, cp_x0, cp_is_static=None):
        r"""Sets ``collision_J_dense``, the dense Jacobian :math:`J = J_a - J_b` of the contact gaps with respect to the flat
        transforms, of shape :math:`(3 C, 12 H)`, in plain torch: the definition :meth:`reduced_terms` is tested against, and fit
        for small problems.  The static points are those :meth:`detect_collisions` marked ``-1``; ``cp_is_static`` is accepted for
        the reference's signature.  ``qr_tfm`` is not built."""
        _check_floating(cp_w=cp_w, cp_x0=cp_x0)
        self._need_contacts()
        self.collision_J_dense = _collision_jacobian(cp_w.detach(), cp_x0.detach(), self.collision_indices_a, self.collision_indices_b)

    def get_bounds(self, cp_delta_dx, cp_dx, cp_x0):
        r"""Not built.  The reference's kernel reads ``offsets[3 c]`` only, so it bounds the columns of the first row of each
        contact's Jacobian block per handle; what it should bound needs a decision of its own."""
        raise NotImplementedError('Collision.get_bounds is not built: the reference bounds only the first row\'s columns of each handle')

    def _need_contacts(self):
        if self.collision_indices_a is None:
            raise RuntimeError('call detect_collisions first')

    def _params(self):
        return (self.collision_radius, self.collision_barrier_ratio, self.friction, self.dt * self.friction_reg,
                self.friction_fluid * self.friction_reg)

    def _contact_tensors(self, dx):
        self._need_contacts()
        _check_floating(dx=dx, cp_dx_at_nm_iteration_0=self.cp_dx_at_nm_iteration_0, normals=self.collision_normals)
        return (dx.detach(), self.cp_dx_at_nm_iteration_0, self.collision_kinematic_gaps, self.collision_normals,
                self.collision_indices_a, self.collision_indices_b)

    def _terms(self, dx, coeff, which):
        tensors = self._contact_tensors(dx)
        if _on_hip(*tensors[:4]):
            return _C.physics.collision_terms_cuda(*(t.contiguous() for t in tensors), coeff, *self._params(), which)
        offset = _contact_offsets(*tensors[:3], *tensors[4:])
        E, G, Hs = _contact_terms(offset, tensors[3], tensors[5] < 0, coeff, *self._params(), gradient=which == 'gradient',
                                  hessian=which == 'hessian')
        return {'energy': E.sum().reshape(1), 'gradient': G, 'hessian': Hs}[which]

    def energy(self, dx, x0, coeff, energy=None):
        r"""The contact energy at the displacements ``dx`` :math:`(N, 3)`, scaled by ``coeff``, of shape :math:`(1,)`; added
        into ``energy`` when one is given.  ``x0`` is accepted for the reference's signature."""
        E = self._terms(dx, coeff, 'energy')
        if energy is None:
            return E
        energy += E
        return energy

    def gradient(self, dx, x0, coeff):
        r"""The gradient of every contact's energy with respect to its offset, of shape :math:`(C, 3)`; exact zeros for a
        contact outside the active range :math:`rp < \hat d \le 1`."""
        return self._terms(dx, coeff, 'gradient')

    def hessian(self, dx, x0, coeff):
        r"""The Hessian block of every contact, of shape :math:`(C, 3, 3)`; not symmetric (the friction cross terms)."""
        return self._terms(dx, coeff, 'hessian')

    def reduced_terms(self, dx, cp_w, cp_x0, coeff, hessian=True):
        r"""The contact energy, :math:`J^T \operatorname{grad}` and :math:`J^T \operatorname{blockdiag}(H_c) J` for the collision
        Jacobian :math:`J = J_a - J_b` of :meth:`calculate_jacobian`, in the column order of
        :func:`~kaolin_amd.physics.simplicits.reduced_neohookean_terms`: the two :math:`K` add directly.

        float32 tensors on a GPU with at most ``kaolin_amd._C.physics.max_handles()`` handles run one HIP kernel and a finishing
        launch: neither :math:`J` nor the :math:`(C, 3, 3)` blocks are formed, the nine :math:`4H \times 4H` blocks are GEMMs of
        depth :math:`C` on the matrix cores, the same inputs give the same bits on every call, and
        ``K[12h+4b+n, 12h'+4b'+n'] == K[12h'+4b+n', 12h+4b'+n]`` to the bit.  No host read: capturable.  Everything else goes
        through the dense :math:`J`.

        Args:
            dx (torch.Tensor): current displacements of the collision points, of shape :math:`(N, 3)`.
            cp_w (torch.Tensor): their skinning weights, of shape :math:`(N, H)`.
            cp_x0 (torch.Tensor): their rest positions, of shape :math:`(N, 3)`.
            coeff (float): scales all three results.
            hessian (bool): compute :math:`K`. Default: True.

        Returns:
            (torch.Tensor, torch.Tensor, torch.Tensor or None): :math:`E` of shape :math:`(1,)`, :math:`g` of shape
            :math:`(12 H,)` and :math:`K` of shape :math:`(12 H, 12 H)`, or None without ``hessian``.
        """
        tensors = self._contact_tensors(dx)
        _check_floating(dx=dx, cp_w=cp_w, cp_x0=cp_x0)
        N = dx.shape[0]
        if cp_w.dim() != 2 or cp_w.shape[0] != N or cp_w.shape[1] < 1 or tuple(cp_x0.shape) != (N, 3):
            raise ValueError(f'cp_w must be of shape ({N}, H) and cp_x0 of shape ({N}, 3), got {tuple(cp_w.shape)}, {tuple(cp_x0.shape)}')
        D = 12 * cp_w.shape[1]
        cp_w, cp_x0 = cp_w.detach(), cp_x0.detach()
        if self.num_contacts == 0:
            zeros = dx.new_zeros
            return zeros(1), zeros(D), zeros((D, D)) if hessian else None
        if _on_hip(*tensors[:4], cp_w, cp_x0) and cp_w.shape[1] <= _C.physics.max_handles():
            return _C.physics.collision_reduced_cuda(*(t.contiguous() for t in tensors), cp_w.contiguous(), cp_x0.contiguous(),
                                                     coeff, *self._params(), hessian=hessian)
        return self._reduced_dense(tensors, cp_w, cp_x0, coeff, hessian)

    def _reduced_dense(self, tensors, cp_w, cp_x0, coeff, hessian):
        """The definition: the vectorised terms and the dense J"""
        offset = _contact_offsets(*tensors[:3], *tensors[4:])
        E, G, Hs = _contact_terms(offset, tensors[3], tensors[5] < 0, coeff, *self._params(), gradient=True, hessian=hessian)
        g, K = _reduced_definition(G, Hs, _collision_jacobian(cp_w, cp_x0, tensors[4], tensors[5]))
        return E.sum().reshape(1), g, K
