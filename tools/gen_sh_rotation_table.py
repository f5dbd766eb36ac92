#!/usr/bin/env python3
"""Generates the term lists of the real spherical-harmonic rotation matrices D^2 and D^3 from the Ivanic-Ruedenberg recurrence
(J. Phys. Chem. 100 (1996) 6342, with the corrected tables of the erratum, J. Phys. Chem. A 102 (1998) 9099) and writes them as

    kaolin_amd/csrc/sh_rotation_table.h              X-macro lists for csrc/gaussian_transform.hip
    kaolin_amd/ops/gaussians/_sh_rotation_table.py   the same lists for the torch formulation and the tests' float64 helper

    python tools/gen_sh_rotation_table.py            rewrite both files
    python tools/gen_sh_rotation_table.py --check    exit 1 when a committed file differs from what the rule gives

Written from the paper: the recursion R^l = u U + v V + w W is its section 8, the coefficients u, v, w are its Table 1 and the functions U, V, W
and P its Table 2, both tables in the corrected form of the erratum; the text below restates them with the paper's letters.  The order
of the terms -- rows m, columns n, then u, v, w, then the summands of P as the tables print them -- is the order in which the tables
are read, and is what any expansion of them element by element gives.

THE RULE.  With R^1 the 3 x 3 matrix of band 1 (rows / columns m, n = -1, 0, 1) and R^{l-1} the matrix of the band below,

    R^l[m][n] = u U + v V + w W,     d = (l + n)(l - n) for |n| < l,  2l (2l - 1) for |n| = l
    u =        sqrt((l + m)(l - m) / d)
    v =  1/2   sqrt((1 + [m = 0]) (l + |m| - 1)(l + |m|) / d) (1 - 2 [m = 0])
    w = -1/2   sqrt((l - |m| - 1)(l - |m|) / d) (1 - [m = 0])
    P(i, a, b) = R^1[i][0] R^{l-1}[a][b]                                            |b| < l
                 R^1[i][1] R^{l-1}[a][l - 1] - R^1[i][-1] R^{l-1}[a][-l + 1]        b = l
                 R^1[i][1] R^{l-1}[a][-l + 1] + R^1[i][-1] R^{l-1}[a][l - 1]        b = -l
    U = P(0, m, n)
    V = P(1, 1, n) + P(-1, -1, n)                                                   m = 0
        P(1, m - 1, n) sqrt(1 + [m = 1]) - P(-1, -m + 1, n) (1 - [m = 1])           m > 0
        P(1, m + 1, n) (1 - [m = -1]) + P(-1, -m - 1, n) sqrt(1 + [m = -1])         m < 0
    W = P(1, m + 1, n) + P(-1, -m - 1, n)                                           m > 0
        P(1, m - 1, n) - P(-1, -m + 1, n)                                           m < 0

A TERM is (c, m, n, i, j, p, q), all indices counted from 0:  R^l[m][n] += c * R^1[i][j] * R^{l-1}[p][q].  Every coefficient is
sign * sqrt(a / b) with integers a, b (the product of u, v or w with the factor inside V); it is carried as that exact fraction,
evaluated once in double as sqrt(a / b), and written as a hexadecimal floating-point literal, which names that double exactly.
Terms are listed by (m, n), inside an element in the order u, v, w.
"""
import argparse
import math
import os
import sys
from fractions import Fraction

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'kaolin_amd', 'csrc', 'sh_rotation_table.h')
MODULE = os.path.join(ROOT, 'kaolin_amd', 'ops', 'gaussians', '_sh_rotation_table.py')


def _p(l, i, a, b):
    """P(i, a, b) as [(sign, row of R^1, column of R^1, row of R^{l-1}, column of R^{l-1})], indices counted from 0"""
    k = l - 1
    if b == l:
        return [(1, i + 1, 2, a + k, 2 * k), (-1, i + 1, 0, a + k, 0)]
    if b == -l:
        return [(1, i + 1, 2, a + k, 0), (1, i + 1, 0, a + k, 2 * k)]
    return [(1, i + 1, 1, a + k, b + k)]


def band_terms(l):
    """-> [(sign, squared coefficient as a Fraction, m, n, i, j, p, q)] of band l"""
    terms = []

    def add(m, n, sign, square, factors):
        if square == 0:
            return
        for s, i, j, p, q in factors:
            terms.append((sign * s, square, m + l, n + l, i, j, p, q))

    for m in range(-l, l + 1):
        for n in range(-l, l + 1):
            d = (l + n) * (l - n) if abs(n) < l else 2 * l * (2 * l - 1)
            am = abs(m)
            add(m, n, 1, Fraction((l + m) * (l - m), d), _p(l, 0, m, n))                             # u U
            v2 = Fraction((1 + (m == 0)) * (l + am - 1) * (l + am), 4 * d)
            if m == 0:                                                                               # v V
                add(m, n, -1, v2, _p(l, 1, 1, n) + _p(l, -1, -1, n))
            elif m > 0:
                add(m, n, 1, v2 * (1 + (m == 1)), _p(l, 1, m - 1, n))
                if m != 1:
                    add(m, n, -1, v2, _p(l, -1, -m + 1, n))
            else:
                if m != -1:
                    add(m, n, 1, v2, _p(l, 1, m + 1, n))
                add(m, n, 1, v2 * (1 + (m == -1)), _p(l, -1, -m - 1, n))
            w2 = Fraction((l - am - 1) * (l - am), 4 * d)                                            # w W
            if m > 0:
                add(m, n, -1, w2, _p(l, 1, m + 1, n) + _p(l, -1, -m - 1, n))
            elif m < 0:
                add(m, n, -1, w2, _p(l, 1, m - 1, n))
                add(m, n, 1, w2, _p(l, -1, -m + 1, n))
    return terms


def coefficient(sign, square):
    return sign * math.sqrt(square.numerator / square.denominator)


def _closed_form(sign, square):
    return f'{"+" if sign > 0 else "-"}sqrt({square.numerator}/{square.denominator})'


def max_terms(terms):
    counts = {}
    for t in terms:
        counts[t[2:4]] = counts.get(t[2:4], 0) + 1
    return max(counts.values())


def render_header():
    out = ['// GENERATED by tools/gen_sh_rotation_table.py from the Ivanic-Ruedenberg recurrence -- do not edit; tests/'
           'test_gaussian_transforms_cpu.py',
           '// regenerates it and compares.  X(c, m, n, i, j, p, q):  D^l[m][n] += c * D^1[i][j] * D^{l-1}[p][q], indices from 0, '
           'terms listed by',
           '// (m, n).  c is the double sqrt(a / b) of the closed form in the comment, as a hexadecimal literal (exact).',
           '#ifndef KAMD_SH_ROTATION_TABLE_H_', '#define KAMD_SH_ROTATION_TABLE_H_']
    for l in (2, 3):
        terms = band_terms(l)
        out.append(f'#define KAMD_SH_BAND{l}_NUM_TERMS {len(terms)}')
        out.append(f'#define KAMD_SH_BAND{l}_MAX_TERMS_PER_ELEMENT {max_terms(terms)}')
        out.append(f'#define KAMD_SH_BAND{l}_TERMS(X) \\')
        for k, (sign, square, m, n, i, j, p, q) in enumerate(terms):
            end = ' \\' if k + 1 < len(terms) else ''
            out.append(f'  X({coefficient(sign, square).hex()}, {m}, {n}, {i}, {j}, {p}, {q}) /* {_closed_form(sign, square)} */{end}')
    out.append('#endif  // KAMD_SH_ROTATION_TABLE_H_')
    return '\n'.join(out) + '\n'


def render_module():
    out = ['"""GENERATED by tools/gen_sh_rotation_table.py from the Ivanic-Ruedenberg recurrence -- do not edit; tests/'
           'test_gaussian_transforms_cpu.py',
           'regenerates it and compares.  A term (c, m, n, i, j, p, q):  D^l[m][n] += c * D^1[i][j] * D^{l-1}[p][q], indices from 0, '
           'listed by (m, n);',
           'c is the double sqrt(a / b) of the closed form in the comment."""', '_h = float.fromhex', '']
    for l in (2, 3):
        terms = band_terms(l)
        out.append(f'BAND{l}_MAX_TERMS_PER_ELEMENT = {max_terms(terms)}')
        out.append(f'BAND{l} = (')
        for sign, square, m, n, i, j, p, q in terms:
            out.append(f"    (_h('{coefficient(sign, square).hex()}'), {m}, {n}, {i}, {j}, {p}, {q}),  # {_closed_form(sign, square)}")
        out.append(')')
    out.append('BANDS = {2: BAND2, 3: BAND3}')
    return '\n'.join(out) + '\n'


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--check', action='store_true', help='compare with the committed files instead of writing them')
    args = ap.parse_args()
    stale = []
    for path, text in ((HEADER, render_header()), (MODULE, render_module())):
        if args.check:
            if not os.path.exists(path) or open(path).read() != text:
                stale.append(path)
        else:
            with open(path, 'w') as f:
                f.write(text)
            print('wrote', os.path.relpath(path, ROOT))
    if stale:
        print('stale:', *stale)
        return 1
    return 0


if __name__ == '__main__':
    sys.exit(main())
