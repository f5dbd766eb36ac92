"""A numpy oracle of ops.conversions.voxelgrids_to_trianglemeshes: per-cell loops in float32, written from the stated rules and
INDEPENDENT of the committed case table (kaolin_amd/csrc/mcube_table.h) and of its generator: the segments of a cell face are found
by walking the face's corner cycle, not from corner cut-offs and a triple product.

    corners  0:(0,0,0) 1:(0,0,1) 2:(0,1,1) 3:(0,1,0) 4:(1,0,0) 5:(1,0,1) 6:(1,1,1) 7:(1,1,0)     (dim0, dim1, dim2)
    case     bit k set iff value(corner k) < iso
    edges    (0,1) (1,2) (2,3) (3,0) (4,5) (5,6) (6,7) (7,4) (0,4) (1,5) (2,6) (3,7)

Face rule: walk the four corners of a cell face counter-clockwise as seen from outside the cell.  Every maximal run of SET corners
(unless all four are set) is cut off by one segment, directed from the crossing where the walk LEAVES the run to the crossing where
it ENTERED it.  On the ambiguous face that is one segment around each set corner.  The segments of a cell chain into loops whose
triangles then have normals pointing from the clear side (>= iso) to the set side (< iso).

Two checkers:
  closed_oriented(faces)              every directed edge occurs once, and its opposite once
  surface_segments(vertices, faces)   the set of directed edges, keyed by end coordinates, whose two ends lie on one unit lattice
                                      square: exactly the loop segments, whatever the triangulation of the loops (no triangulation
                                      in use has a diagonal inside a cell face)
"""
import functools

import numpy as np

CORNERS = ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0))
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
_EDGE_OF = {frozenset(e): n for n, e in enumerate(EDGES)}


def _face_cycles():
    """The six faces as corner cycles, counter-clockwise seen from outside."""
    cycles = []
    for axis in range(3):
        u, v = [d for d in range(3) if d != axis]
        for side in (0, 1):
            ring = []
            for a, b in ((0, 0), (1, 0), (1, 1), (0, 1)):
                off = [0, 0, 0]
                off[axis], off[u], off[v] = side, a, b
                ring.append(CORNERS.index(tuple(off)))
            p = [np.array(CORNERS[c]) for c in ring]
            outward = np.zeros(3)
            outward[axis] = 2 * side - 1
            if np.dot(np.cross(p[1] - p[0], p[2] - p[1]), outward) < 0:
                ring.reverse()
            cycles.append(ring)
    return cycles


_CYCLES = _face_cycles()
# pairs of edges on one cell face
_ON_ONE_FACE = set()
for _ring in _CYCLES:
    _es = [_EDGE_OF[frozenset((_ring[i], _ring[(i + 1) % 4]))] for i in range(4)]
    _ON_ONE_FACE |= {(a, b) for a in _es for b in _es if a != b}


@functools.lru_cache(maxsize=None)
def cell_loops(case):
    """The directed loops of one case as tuples of edge ids, each starting at its smallest id, ordered by that id."""
    bit = [(case >> k) & 1 for k in range(8)]
    follow = {}
    for ring in _CYCLES:
        b = [bit[c] for c in ring]
        if sum(b) in (0, 4):
            continue
        for i in range(4):
            if b[i] and not b[(i + 1) % 4]:                     # the walk leaves a run of set corners here
                j = i
                while b[(j - 1) % 4]:
                    j -= 1                                      # ... which it entered before corner j
                leave = _EDGE_OF[frozenset((ring[i], ring[(i + 1) % 4]))]
                enter = _EDGE_OF[frozenset((ring[(j - 1) % 4], ring[j % 4]))]
                assert leave not in follow
                follow[leave] = enter
    crossed = {n for n, (a, c) in enumerate(EDGES) if bit[a] != bit[c]}
    assert set(follow) == crossed and set(follow.values()) == crossed
    loops, left = [], set(crossed)
    while left:
        start = min(left)
        loop, e = [], start
        while not loop or e != start:
            loop.append(e)
            left.discard(e)
            e = follow[e]
        loops.append(tuple(loop))
    return tuple(loops)


def _triangulate(loop):
    """The first triangulation, in depth-first order (apex ascending; the triangle, the low part, the high part), none of whose
    interior diagonals joins two crossings of one cell face."""
    n = len(loop)

    def allowed(i, j):
        return abs(i - j) in (1, n - 1) or (loop[i], loop[j]) not in _ON_ONE_FACE

    def solve(lo, hi):
        if hi - lo == 1:
            return ()
        for k in range(lo + 1, hi):
            if allowed(lo, k) and allowed(k, hi):
                low = solve(lo, k)
                high = solve(k, hi) if low is not None else None
                if high is not None:
                    return ((loop[lo], loop[k], loop[hi]),) + low + high
        return None

    return solve(0, n - 1)


@functools.lru_cache(maxsize=None)
def cell_triangles(case):
    tris = ()
    for loop in cell_loops(case):
        t = _triangulate(loop)
        assert t is not None and len(t) == len(loop) - 2
        tris += t
    return tris


def marching_cubes(grid, iso_value=0.5, border=True):
    """grid (X, Y, Z) -> vertices (V, 3) float32, faces (F, 3) int64, as the operator defines them: the field is the grid with a
    border of zeros (``border=False``: the grid as given), vertices ordered by the lower end of their lattice edge in raster order
    and then by axis, faces by cell in raster order and then as ``cell_triangles`` lists them."""
    g = np.asarray(grid).astype(np.float32)
    if border:
        g = np.pad(g, 1)
    iso = np.float32(iso_value)
    X, Y, Z = g.shape
    keys, tris = set(), []
    for i in range(X - 1):
        for j in range(Y - 1):
            for k in range(Z - 1):
                case = 0
                for c, (a, b, d) in enumerate(CORNERS):
                    case |= int(g[i + a, j + b, k + d] < iso) << c
                for tri in cell_triangles(case):
                    row = []
                    for e in tri:
                        p, q = (np.array(CORNERS[c]) for c in EDGES[e])
                        lo = np.minimum(p, q)
                        axis = int(np.argmax(np.abs(p - q)))
                        row.append(((i + int(lo[0]), j + int(lo[1]), k + int(lo[2])), axis))
                    keys.update(row)
                    tris.append(row)
    keys = sorted(keys)
    index = {key: n for n, key in enumerate(keys)}
    verts = np.zeros((len(keys), 3), dtype=np.float32)
    with np.errstate(all='ignore'):
        for n, (lo, axis) in enumerate(keys):
            hi = list(lo)
            hi[axis] += 1
            f_lo, f_hi = g[lo], g[tuple(hi)]
            verts[n] = lo
            if axis == 0:
                verts[n, axis] = np.float32(lo[axis]) + (iso - f_lo) / (f_hi - f_lo)
            else:
                verts[n, axis] = np.float32(hi[axis]) - (iso - f_hi) / (f_lo - f_hi)
    faces = np.array([[index[key] for key in row] for row in tris], dtype=np.int64).reshape(-1, 3)
    return verts, faces


def closed_oriented(faces):
    """True when every directed edge of the triangles occurs exactly once and its opposite exactly once."""
    f = np.asarray(faces).reshape(-1, 3)
    directed = [(int(t[a]), int(t[(a + 1) % 3])) for t in f for a in range(3)]
    seen = set(directed)
    return len(seen) == len(directed) and all((b, a) in seen for a, b in seen)


def surface_segments(vertices, faces):
    """The directed triangle edges whose two ends lie on one unit lattice square, as a set of coordinate pairs."""
    v = np.asarray(vertices, dtype=np.float64)
    out = set()
    for t in np.asarray(faces).reshape(-1, 3):
        for a in range(3):
            p, q = v[t[a]], v[t[(a + 1) % 3]]
            for d in range(3):
                if p[d] != q[d] or p[d] != np.floor(p[d]):
                    continue
                rest = [x for x in range(3) if x != d]
                if all(max(p[x], q[x]) <= np.floor(min(p[x], q[x])) + 1 for x in rest):
                    out.add((tuple(p), tuple(q)))
                    break
    return out


def vertex_gradient_terms(grid, iso_value, grad_vertices):
    """In float64, for the (X, Y, Z) grid of an item (values taken as float32, border of zeros) and the gradient (V, 3) of its
    vertices: per grid value the sum of its at most six terms ``grad_vertices[v, axis] * d position_v / d value`` -- one per crossed
    lattice edge at the voxel --, the sum of their magnitudes, and the sum of |g / d| over those edges.  On an edge of ends lo, hi
    with d = f_hi - f_lo the position moves by +(iso - f_hi) / d^2 per unit of f_lo and by -(iso - f_lo) / d^2 per unit of f_hi,
    on every axis.  (Autograd through t = n / d forms g / d and g n / d^2, each at most |g / d| since iso lies between the two
    values: the third result bounds ITS intermediate quantities, the second the terms of the closed form.)"""
    g32 = np.pad(np.asarray(grid).astype(np.float32), 1)
    g, iso = g32.astype(np.float64), float(np.float32(iso_value))
    grad_vertices = np.asarray(grad_vertices, dtype=np.float64)
    below = g32 < np.float32(iso_value)
    own = np.zeros(g.shape + (3,), dtype=bool)
    own[:-1, :, :, 0] = below[:-1] != below[1:]
    own[:, :-1, :, 1] = below[:, :-1] != below[:, 1:]
    own[:, :, :-1, 2] = below[:, :, :-1] != below[:, :, 1:]
    ids = (np.cumsum(own.reshape(-1)) - 1).reshape(own.shape)          # the vertex order: lattice point, then axis
    assert int(own.sum()) == grad_vertices.shape[0]
    total, magnitude, edges = np.zeros_like(g), np.zeros_like(g), np.zeros_like(g)
    for axis in range(3):
        lo = np.nonzero(own[..., axis])
        hi = tuple(x + (n == axis) for n, x in enumerate(lo))
        gv = grad_vertices[ids[..., axis][lo], axis]
        d = g[hi] - g[lo]
        for at, term in ((lo, gv * (iso - g[hi]) / d ** 2), (hi, -gv * (iso - g[lo]) / d ** 2)):
            np.add.at(total, at, term)
            np.add.at(magnitude, at, np.abs(term))
            np.add.at(edges, at, np.abs(gv / d))
    inner = (slice(1, -1),) * 3
    return total[inner], magnitude[inner], edges[inner]


def gamma(k, unit=2.0 ** -24):
    """Higham's gamma_k = k u / (1 - k u): the relative error bound of k rounded operations in a row."""
    return k * unit / (1 - k * unit)
