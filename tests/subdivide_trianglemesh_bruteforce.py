"""Numpy reference of ONE iteration of Loop subdivision with a per-vertex alpha (helper, not collected; no project code).

Written from the definition in the header comment of csrc/subdivide_trianglemesh.hip, not from the package's torch formulation:

    edge slots of a face (a, b, c)   ab bc ca, opposite corners c a b; an edge is the pair (min, max) of its ends, a self-edge
                                     (v, v) included; the E unique edges are numbered in ascending (min, max) order
    count[e]                         the face slots holding edge e
    neighbours of v                  the max ends of the edges with min = v, then the min ends of the edges with max = v (the
                                     self-edge is in the first list already): n[v] of them
    old row v, n[v] > 0              (1 - alpha[v]) x[v] + alpha[v] / n[v] * sum of x[u] over the neighbours; alpha given, or
                                     5/8 - (3/8 + cos(2 pi / n) / 4)^2; n[v] = 0: the row is copied
    new row V + e                    count[e] == 2: (3 (x[lo] + x[hi]) + x[opp0] + x[opp1]) / 8, else (x[lo] + x[hi]) / 2; the
                                     channels are x y z and alpha
    new_faces                        (b bc ab) (a ab ca) (c ca bc) (ca ab bc)
    tlist                            (min end, edge id) of every edge, in ascending (max, min) order
    runs[v], v in [0, V]             (edges with min < v, edges with max < v): where the runs of v start in edges and in tlist

``topology`` keeps a Python set of pairs; ``topology_vectorised`` is its twin on np.unique / np.searchsorted for meshes too large
for that (the CPU test asserts them equal on every small case).  The values are accumulated in ``ACC`` -- numpy's long double,
on x86 a 64-bit significand, so that the float64 results it is rounded to carry half a unit of float64 roundoff instead of an
accumulation error of the size of the one under test -- and returned as float64, each with the sum of the magnitudes of the terms
it adds (``tas``) and, for gradients, the number of terms (``terms``).

THE BOUNDS (``forward_bound``, ``gradient_bound``), with u the unit roundoff of the dtype under test, gamma_k = k u / (1 - k u):

    old row, valence n       gamma_(n+3) tas + d_alpha (|x_v| + sum |x_u| / n)
                             the neighbour terms pass n - 1 additions, the division a / n, the product with the sum and the final
                             addition: n + 2 roundings (the own term (1 - a) x_v: 3), and one more for this reference's rounding
    edge row                 gamma_4 tas: ends, times 3, far, the sum (times 1/8 is exact), and one for this reference
    gradient element         gamma_(t+3) tas: t terms added in any order (t - 1 roundings), a coefficient a_u / n_u times g (2),
                             one spare, one for this reference.  The vertex-rule term of alpha's gradient,
                             sum_c g[v, c] (S[v, c] / n - x[v, c]), counts its 3 (n + 1) leaves as terms.  (A computed default alpha
                             is a coefficient here too, but the bound carries no d_alpha term: no result of the CPU path or of the
                             HIP pipeline on the tests' cases comes near needing one.)
    d_alpha                  0 when alpha is given.  With the default alpha 8 u: the argument 2 pi / n carries 2 roundings, which
                             move cos by at most 2 u x |sin x| <= 3.2 u (x = 2 pi / n, largest at n = 4; n = 3 takes the exact
                             branch), cos itself is within 2 ulp = 4 u: 7.2 u; s = 3/8 + cos / 4 then has 1.8 u + u; s^2 has
                             2 s * 2.8 u + u <= 6.6 u (|s| < 1), the last subtraction 0.625 u: 7.3 u < 8 u.
"""
import bisect
from types import SimpleNamespace

import numpy as np

ACC = np.longdouble
F64, I64, I32 = np.float64, np.int64, np.int32
DENSE_LIMIT = 1 << 20          # per-vertex arrays (runs, valence) are built up to this V; beyond it, ask runs_at / valence_at


def unit_roundoff(dtype):
    return {'float32': 2.0 ** -24, 'float64': 2.0 ** -53}[str(dtype).replace('torch.', '')]


def gamma(k, u):
    k = np.asarray(k, dtype=F64)
    return k * u / (1 - k * u)


# ---- topology -----------------------------------------------------------------------------------------------------------------
class Topology(SimpleNamespace):
    """V, E, edges (E, 2), count (E), new_faces (4 F, 3), opp (E, 2) the two opposite corners in ascending order where count == 2
    (-1 elsewhere), tlist (E, 2), self_edges (number of edges (v, v)); neighbour pairs nbr_v, nbr_u (one row per (vertex,
    neighbour), in list order); runs (V + 1, 2) and valence (V) when V <= DENSE_LIMIT, else None"""

    def runs_at(self, rows):
        """rows of ``runs`` for any ids in [0, V], without the dense array"""
        mins, maxs = self.edges[:, 0].tolist(), sorted(self.edges[:, 1].tolist())
        return np.array([[bisect.bisect_left(mins, int(v)), bisect.bisect_left(maxs, int(v))] for v in rows], dtype=I64).reshape(-1, 2)

    def valence_at(self, rows):
        lists = {}
        for v, u in zip(self.nbr_v.tolist(), self.nbr_u.tolist()):
            lists.setdefault(v, []).append(u)
        return np.array([len(lists.get(int(v), ())) for v in rows], dtype=I32)


def _finish(V, edges, count, new_faces, opp, tlist, nbr_v, nbr_u):
    E = edges.shape[0]
    runs = valence = None
    if V <= DENSE_LIMIT:
        ids = np.arange(V + 1)
        runs = np.stack([np.searchsorted(edges[:, 0], ids, side='left'), np.searchsorted(np.sort(edges[:, 1]), ids, side='left')], 1).astype(I64)
        valence = np.bincount(nbr_v, minlength=V).astype(I32)
    return Topology(V=V, E=E, edges=edges, count=count, new_faces=new_faces, opp=opp, tlist=tlist, nbr_v=nbr_v, nbr_u=nbr_u,
                    runs=runs, valence=valence, self_edges=int((edges[:, 0] == edges[:, 1]).sum()))


def topology(faces, V):
    """The plain version: a set of (min, max) pairs numbered in ascending order, Python lists per edge and per vertex."""
    faces = [tuple(int(i) for i in f) for f in np.asarray(faces).reshape(-1, 3)]
    assert all(0 <= i < V for f in faces for i in f)
    pairs = set()
    for a, b, c in faces:
        for p, q in ((a, b), (b, c), (c, a)):
            pairs.add((min(p, q), max(p, q)))
    order = sorted(pairs)
    number = {pair: e for e, pair in enumerate(order)}
    E = len(order)
    count, corners, new_faces = [0] * E, [[] for _ in range(E)], []
    for a, b, c in faces:
        ids = []
        for (p, q), far in (((a, b), c), ((b, c), a), ((c, a), b)):
            e = number[(min(p, q), max(p, q))]
            count[e] += 1
            corners[e].append(far)
            ids.append(V + e)
        ab, bc, ca = ids
        new_faces += [(b, bc, ab), (a, ab, ca), (c, ca, bc), (ca, ab, bc)]
    opp = [sorted(corners[e]) if count[e] == 2 else [-1, -1] for e in range(E)]
    transposed = sorted((hi, lo, e) for e, (lo, hi) in enumerate(order))
    tlist = [(lo, e) for hi, lo, e in transposed]
    neighbours = {}
    for lo, hi in order:                           # ascending (min, max): the max ends of the run of min = lo
        neighbours.setdefault(lo, []).append(hi)
    for hi, lo, e in transposed:                   # ascending (max, min): the min ends of the run of max = hi
        if lo != hi:
            neighbours.setdefault(hi, []).append(lo)
    nbr = [(v, u) for v in sorted(neighbours) for u in neighbours[v]]
    arr = lambda rows, width: np.array(rows, dtype=I64).reshape(-1, width)
    nbr = arr(nbr, 2)
    return _finish(V, arr(order, 2), np.array(count, dtype=I32), arr(new_faces, 3), arr(opp, 2), arr(tlist, 2), nbr[:, 0], nbr[:, 1])


def topology_vectorised(faces, V):
    """The same products from np.unique(axis=0) and np.searchsorted, for the meshes the plain version is too slow for."""
    f = np.asarray(faces, dtype=I64).reshape(-1, 3)
    assert f.size and f.min() >= 0 and f.max() < V
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    p, q, far = np.stack([a, b, c], 1).reshape(-1), np.stack([b, c, a], 1).reshape(-1), np.stack([c, a, b], 1).reshape(-1)
    slots = np.stack([np.minimum(p, q), np.maximum(p, q)], 1)
    edges, inverse, count = np.unique(slots, axis=0, return_inverse=True, return_counts=True)
    inverse = inverse.reshape(-1)
    E = edges.shape[0]
    ab, bc, ca = (V + inverse.reshape(-1, 3)[:, k] for k in range(3))
    new_faces = np.stack([b, bc, ab, a, ab, ca, c, ca, bc, ca, ab, bc], 1).reshape(-1, 3)
    opp = np.full((E, 2), -1, dtype=I64)
    two = count[inverse] == 2
    by_edge = np.lexsort((far[two], inverse[two]))                      # the slots of the count-2 edges, edge by edge, corners ascending
    opp[inverse[two][by_edge][0::2]] = far[two][by_edge].reshape(-1, 2)
    by_max = np.lexsort((edges[:, 0], edges[:, 1]))
    tlist = np.stack([edges[by_max, 0], by_max], 1).astype(I64)
    proper = tlist[:, 0] != edges[by_max, 1]
    nbr_v = np.concatenate([edges[:, 0], edges[by_max, 1][proper]])
    nbr_u = np.concatenate([edges[:, 1], tlist[proper, 0]])
    keep = np.argsort(nbr_v, kind='stable')                             # vertex by vertex, the first list before the second
    return _finish(V, edges.astype(I64), count.astype(I32), new_faces, opp, tlist, nbr_v[keep], nbr_u[keep])


TOPOLOGY_FIELDS = ('edges', 'count', 'new_faces', 'opp', 'tlist', 'nbr_v', 'nbr_u', 'runs', 'valence')


def same_topology(s, t):
    return s.V == t.V and s.E == t.E and s.self_edges == t.self_edges and all(
        (getattr(s, k) is None and getattr(t, k) is None) or
        (getattr(s, k).dtype == getattr(t, k).dtype and np.array_equal(getattr(s, k), getattr(t, k))) for k in TOPOLOGY_FIELDS)


# ---- values -------------------------------------------------------------------------------------------------------------------
def default_alpha(n):
    """The Loop weight of the valences n > 0, in ACC"""
    n = np.asarray(n).astype(ACC)
    two_pi = ACC(8) * np.arctan(ACC(1))
    s = ACC(3) / 8 + np.cos(two_pi / n) / 4
    return np.where(n == 3, ACC(9) / 16, ACC(5) / 8 - s * s)


def _sizes(tp):
    n = np.bincount(tp.nbr_v, minlength=tp.V) if tp.valence is None else tp.valence.astype(I64)
    return n, n > 0, np.maximum(n, 1).astype(ACC)


def _alphas(tp, alpha, B):
    n, used, nd = _sizes(tp)
    if alpha is None:
        a = np.where(used, default_alpha(np.maximum(n, 1)), ACC(0))[None].repeat(B, 0)
    else:
        a = np.where(used[None], np.asarray(alpha).astype(ACC), ACC(0))
    return a, n, used, nd


def forward(tp, x, alpha=None):
    """x (B, V, 3), alpha (B, V) or None (the default alpha) -> new_x (B, V + E, 3), new_alpha (B, V + E) or None, their term
    magnitude sums tas_x, tas_alpha, n_row (V + E: the valence of an old row, -1 for an edge row) and dal (B, V + E, 3): what a
    unit error of a computed alpha moves the element by, |x_v| + sum |x_u| / n (0 for edge rows and unused vertices)."""
    x = np.asarray(x).astype(ACC)
    B, V, E = x.shape[0], tp.V, tp.E
    a, n, used, nd = _alphas(tp, alpha, B)
    lo, hi, two = tp.edges[:, 0], tp.edges[:, 1], tp.count == 2
    o = np.where(tp.opp >= 0, tp.opp, 0)

    def edge_rows(val):                                        # val (B, V, C)
        ends = val[:, lo] + val[:, hi]
        far = val[:, o[:, 0]] + val[:, o[:, 1]]
        return np.where(two[None, :, None], (3 * ends + far) / 8, ends / 2)

    S, SA = np.zeros_like(x), np.zeros_like(x)
    np.add.at(S, (slice(None), tp.nbr_v), x[:, tp.nbr_u])
    np.add.at(SA, (slice(None), tp.nbr_v), np.abs(x[:, tp.nbr_u]))
    a3, n3, used3 = a[..., None], nd[None, :, None], used[None, :, None]
    old = np.where(used3, (1 - a3) * x + a3 / n3 * S, x)
    old_tas = np.where(used3, np.abs(1 - a3) * np.abs(x) + np.abs(a3) / n3 * SA, np.abs(x))
    dal = np.where(used3, np.abs(x) + SA / n3, 0)
    out = SimpleNamespace(
        new_x=np.concatenate([old, edge_rows(x)], 1).astype(F64), tas_x=np.concatenate([old_tas, edge_rows(np.abs(x))], 1).astype(F64),
        n_row=np.concatenate([n, np.full(E, -1)]), dal=np.concatenate([dal, np.zeros((B, E, 3), ACC)], 1).astype(F64),
        new_alpha=None, tas_alpha=None)
    if alpha is not None:
        al = np.asarray(alpha).astype(ACC)[..., None]
        out.new_alpha = np.concatenate([al, edge_rows(al)], 1)[..., 0].astype(F64)
        out.tas_alpha = np.concatenate([np.abs(al), edge_rows(np.abs(al))], 1)[..., 0].astype(F64)
    return out


class _Sum:
    """An accumulator that keeps, next to the sum, the sum of the magnitudes and the number of the terms added"""

    def __init__(self, shape):
        self.value, self.tas, self.terms = np.zeros(shape, ACC), np.zeros(shape, ACC), np.zeros(shape, I64)

    def add_at(self, rows, term, leaves=1):
        """+= term (B, len(rows), ...) at the rows `rows` of axis 1, repeated rows included"""
        np.add.at(self.value, (slice(None), rows), term)
        np.add.at(self.tas, (slice(None), rows), np.abs(term))
        np.add.at(self.terms, (slice(None), rows), np.broadcast_to(np.asarray(leaves, dtype=I64), term.shape))


def backward(tp, x, alpha, gx, ga=None):
    """The transposed maps, term by term.  x (B, V, 3), alpha (B, V) or None, gx (B, V + E, 3) the cotangent on new_x, ga
    (B, V + E) or None the cotangent on new_alpha -> dx, tas_dx, terms_dx (B, V, 3) and, when alpha is given, da, tas_da,
    terms_da (B, V)."""
    x, gx = np.asarray(x).astype(ACC), np.asarray(gx).astype(ACC)
    B, V, E = x.shape[0], tp.V, tp.E
    a, n, used, nd = _alphas(tp, alpha, B)
    lo, hi, two = tp.edges[:, 0], tp.edges[:, 1], tp.count == 2
    every, pair = np.arange(V), np.nonzero(two)[0]
    weight = np.where(two, ACC(3) / 8, ACC(1) / 2)
    a3, n3, used3 = a[..., None], nd[None, :, None], used[None, :, None]

    def edge_terms(acc, g):                                    # g (B, V + E, C): the rows V + e spread to their ends and corners
        ge = g[:, V:]
        acc.add_at(lo, weight[None, :, None] * ge)
        acc.add_at(hi, weight[None, :, None] * ge)
        for k in range(2):
            acc.add_at(tp.opp[pair, k], ge[:, pair] / 8)

    gv = gx[:, :V]
    dx = _Sum((B, V, 3))
    dx.add_at(every, np.where(used3, 1 - a3, ACC(1)) * gv)                             # new_x[v] holds (1 - a_v) x[v], or x[v]
    dx.add_at(tp.nbr_u, (a3 / n3 * gv)[:, tp.nbr_v])                                   # new_x[v] holds a_v / n_v x[u]
    edge_terms(dx, gx)
    out = SimpleNamespace(dx=dx.value.astype(F64), tas_dx=dx.tas.astype(F64), terms_dx=dx.terms, da=None, tas_da=None, terms_da=None)
    if alpha is not None:
        da = _Sum((B, V, 1))
        if ga is not None:
            g1 = np.asarray(ga).astype(ACC)[..., None]
            da.add_at(every, g1[:, :V])
            edge_terms(da, g1)
        # new_x[v, c] holds alpha_v (S[v, c] / n_v - x[v, c]): per channel n_v + 1 leaves
        S, SA = np.zeros_like(x), np.zeros_like(x)
        np.add.at(S, (slice(None), tp.nbr_v), x[:, tp.nbr_u])
        np.add.at(SA, (slice(None), tp.nbr_v), np.abs(x[:, tp.nbr_u]))
        rule = np.where(used3, gv * (S / n3 - x), 0).sum(-1, keepdims=True)
        rule_tas = np.where(used3, np.abs(gv) * (SA / n3 + np.abs(x)), 0).sum(-1, keepdims=True)
        np.add.at(da.value, (slice(None), every), rule)
        np.add.at(da.tas, (slice(None), every), rule_tas)
        np.add.at(da.terms, (slice(None), every), np.broadcast_to(np.where(used, 3 * (n + 1), 0)[None, :, None], rule.shape))
        out.da, out.tas_da, out.terms_da = da.value[..., 0].astype(F64), da.tas[..., 0].astype(F64), da.terms[..., 0]
    return out


# ---- bounds -------------------------------------------------------------------------------------------------------------------
def forward_bound(fw, dtype, default):
    """-> the bounds of new_x (B, V + E, 3) and of new_alpha (or None) of a forward in `dtype`; `default`: the alpha was computed"""
    u = unit_roundoff(dtype)
    g = np.where(fw.n_row >= 0, gamma(np.maximum(fw.n_row, 0) + 3, u), gamma(4, u))
    bound_x = g[None, :, None] * fw.tas_x + (8 * u * fw.dal if default else 0)
    return bound_x, (None if fw.tas_alpha is None else g[None] * fw.tas_alpha)


def gradient_bound(bw, dtype):
    """-> the bounds of dx (B, V, 3) and of da (or None)"""
    u = unit_roundoff(dtype)
    return gamma(bw.terms_dx + 3, u) * bw.tas_dx, (None if bw.da is None else gamma(bw.terms_da + 3, u) * bw.tas_da)


def share(got, want, bound):
    """The largest |got - want| / bound (an element whose bound is 0 must be equal: inf otherwise); NaN in `got` gives inf"""
    got, want = np.asarray(got, dtype=F64), np.asarray(want, dtype=F64)
    assert got.shape == want.shape == np.broadcast(want, bound).shape, (got.shape, want.shape)
    diff = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(diff == 0, 0.0, diff / np.broadcast_to(bound, diff.shape))
    ratio = np.where(np.isnan(ratio), np.inf, ratio)
    return float(ratio.max()) if ratio.size else 0.0
