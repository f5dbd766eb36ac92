"""Brute-force SPC convolutions in numpy float64: the oracle of tests/test_spc_conv_cpu.py and tests/test_spc_conv_gpu.py.

Per item a dictionary from the coordinates of a level's points to their packed rows (from the hierarchies tests/spc_bruteforce.py
decodes), and the two neighbourhoods exactly as the operators' contract words them:

* direct (``conv3d``): output point p of level P = Q - jump takes input point ``2^jump p + v_k`` of level Q;
* transposed (``conv_transpose3d``): output point p of level P = Q + jump takes input point ``(p - v_k) / 2^jump`` of level Q where
  every component of ``p - v_k`` is non-negative and divisible by 2^jump.

A neighbour outside ``[0, 2^Q)`` or absent from the octree is a miss; duplicate vectors each contribute.  Beside every result
element the sum of the absolute products that went into it and their count T, which `conv_bound` turns into the error any
summation order of T rounded products can have.  tests/test_spc_conv_cpu.py pins the forward to torch's dense convolutions.  It
must not import kaolin_amd."""
import numpy as np


class Case:
    """triples (list of (k, output row, input row)), n_in, n_out, level, out_level"""


def level_rows(decoded, level):
    """per item {(x, y, z): packed row among the points of `level` of the batch}, and the number of rows"""
    tables, first = [], 0
    for d in decoded:
        pts = d.level_points[level]
        tables.append({tuple(int(c) for c in p): first + i for i, p in enumerate(pts)})
        first += len(pts)
    return tables, first


def triples(decoded, level, jump, kernel_vectors, transposed):
    """every (k, output row, input row) of the operator on the batch `decoded` (list of spc_bruteforce.Decoded), input at `level`"""
    out_level = level + jump if transposed else level - jump
    s = 2 ** jump
    inputs, n_in = level_rows(decoded, level)
    outputs, n_out = level_rows(decoded, out_level)
    found = []
    for b in range(len(decoded)):
        for p, row in outputs[b].items():
            for k, v in enumerate(np.asarray(kernel_vectors, dtype=np.int64).reshape(-1, 3)):
                if transposed:
                    u = [p[a] - int(v[a]) for a in range(3)]
                    if any(c < 0 or c % s for c in u):
                        continue
                    q = tuple(c // s for c in u)
                else:
                    q = tuple(s * p[a] + int(v[a]) for a in range(3))
                if any(c < 0 or c >= 2 ** level for c in q):
                    continue
                if q in inputs[b]:
                    found.append((k, row, inputs[b][q]))
    c = Case()
    c.triples, c.n_in, c.n_out, c.level, c.out_level = found, n_in, n_out, level, out_level
    return c


def _by_offset(case):
    """{k: (output rows, input rows)} as index arrays, in the order the triples were found"""
    groups = {}
    for k, o, i in case.triples:
        groups.setdefault(k, ([], []))
        groups[k][0].append(o)
        groups[k][1].append(i)
    return {k: (np.array(o, dtype=np.int64), np.array(i, dtype=np.int64)) for k, (o, i) in groups.items()}


def _wide(a):
    """the sums below are taken in numpy's long double (a 64-bit mantissa where the platform has one), so that the oracle's own
    rounding is far below the float64 bound it is compared within"""
    return np.asarray(a, dtype=np.float64).astype(np.longdouble)


def _gathered(case, shape, a, rows_of_a, rows_of_result, b_of):
    """result[r] += a[row] @ b_of(k) over the triples -> (sum, sum of |a| @ |b|, number of products per element)"""
    value, abs_sum, count = np.zeros(shape, dtype=np.longdouble), np.zeros(shape), np.zeros(shape)
    for k, rows in _by_offset(case).items():
        src, dst = rows[rows_of_a], rows[rows_of_result]
        np.add.at(value, dst, _wide(a[src]) @ _wide(b_of(k)))          # an offset names a result row at most once
        np.add.at(abs_sum, dst, np.abs(a[src]) @ np.abs(b_of(k)))
        np.add.at(count, dst, float(a.shape[1]))
    return value, abs_sum, count


def forward(case, x, w):
    """Y (n_out, out) = sum over the triples of X[input row] @ W[k] -> (Y, sum |a b|, T)"""
    x, w = np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64)
    return _gathered(case, (case.n_out, w.shape[2]), x, 1, 0, lambda k: w[k])


def grad_input(case, g, w):
    """dL/dX (n_in, in) for dL/dY = g: sum over the triples of g[output row] @ W[k]^T"""
    g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
    return _gathered(case, (case.n_in, w.shape[1]), g, 0, 1, lambda k: w[k].T)


def grad_weight(case, x, g, K):
    """dL/dW (K, in, out): sum over the triples of k of X[input row]^T g[output row]: ONE product per triple and element"""
    x, g = np.asarray(x, dtype=np.float64), np.asarray(g, dtype=np.float64)
    shape = (K, x.shape[1], g.shape[1])
    value, abs_sum, count = np.zeros(shape, dtype=np.longdouble), np.zeros(shape), np.zeros(shape)
    for k, (o, i) in _by_offset(case).items():
        value[k] = _wide(x[i]).T @ _wide(g[o])
        abs_sum[k] = np.abs(x[i]).T @ np.abs(g[o])
        count[k] = len(o)
    return value, abs_sum, count


UNIT = {'float64': 2.0 ** -53, 'float32': 2.0 ** -24, 'float16': 2.0 ** -11, 'bfloat16': 2.0 ** -8}


def conv_bound(abs_sum, count, want, dtype, accumulate=None):
    """|got - want64| allowed for a sum of `count` products, each rounded once, added in ANY order, fused or not, in `accumulate`
    (default `dtype`): gamma sum |a b|, gamma = (T + 1) u / (1 - (T + 1) u) (Higham, Accuracy and Stability, lemma 3.1 and (3.4):
    T products and at most T - 1 additions touch a term), plus u(dtype) |want| for the rounding of the value compared -- and, for
    half, half a spacing of its subnormals.  An element without products must be exact: its bound is 0."""
    u = UNIT[accumulate or dtype]
    t = (np.asarray(count, dtype=np.float64) + 1.0) * u
    bound = t / (1.0 - t) * abs_sum + UNIT[dtype] * np.abs(want)
    if dtype == 'float16':
        bound = bound + np.where(np.asarray(count) > 0, 2.0 ** -25, 0.0)
    return bound
