"""Generates kaolin_amd/csrc/mcube_table.h: the 256-case triangle table of marching cubes, from rules alone.

    python tools/gen_mcube_table.py            writes the header
    python tools/gen_mcube_table.py --check    exits 1 when the committed header differs from the generated one

Cell geometry, in tensor-index terms (dim0, dim1, dim2):
    corners  0:(0,0,0) 1:(0,0,1) 2:(0,1,1) 3:(0,1,0) 4:(1,0,0) 5:(1,0,1) 6:(1,1,1) 7:(1,1,0)
    case     bit k is set iff value(corner k) < iso
    edges    0:(0,1) 1:(1,2) 2:(2,3) 3:(3,0) 4:(4,5) 5:(5,6) 6:(6,7) 7:(7,4) 8:(0,4) 9:(1,5) 10:(2,6) 11:(3,7);  an edge is
             crossed iff its two bits differ

Rules:
  1. Segments.  On each of the six cell faces the crossed edges are joined by segments: two crossings give one segment, four
     crossings (the ambiguous face) give two, each cutting off a corner whose bit is SET.  The rule reads the face's four corners
     only, so the two cells that share a face draw the same segments.
  2. Loops.  The segments chain into closed loops, oriented so that triangle normals point from the clear side (>= iso) to the set
     side (< iso): for a segment of direction d on the face of outward normal n, with s pointing to the set side of the segment
     within the face, (s x d) . n < 0.  A loop starts at its smallest edge id; loops are ordered by that id.
  3. Triangles.  A loop of n crossings gets n - 2 triangles.  No interior diagonal may join two crossings that lie on one cell
     face: such a diagonal lies IN that face, where the neighbouring cell may draw it too (a non-manifold edge).  The
     triangulations of a loop v[0..n) are enumerated depth first: the triangle on the side (v[lo], v[hi]) takes its apex
     v[k], k ascending from lo + 1, then the part lo..k, then the part k..hi; the first admissible one is taken, and its triangles
     are listed in that order (the triangle, the low part, the high part), each as (v[lo], v[k], v[hi]).

Every row holds its triangles as edge ids, three per triangle, ended by 255; at most 5 triangles occur.
"""
import os
import sys

CORNERS = ((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0), (1, 0, 0), (1, 0, 1), (1, 1, 1), (1, 1, 0))
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
END = 255
HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'kaolin_amd', 'csrc', 'mcube_table.h')


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _dot(a, b):
    return sum(x * y for x, y in zip(a, b))


def _sub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def _mid(e):
    a, b = EDGES[e]
    return tuple((x + y) / 2 for x, y in zip(CORNERS[a], CORNERS[b]))


def cell_faces():
    """(axis, side) -> (corner ids, edge ids) of the six faces of the cell."""
    faces = {}
    for axis in range(3):
        for side in range(2):
            cs = [c for c in range(8) if CORNERS[c][axis] == side]
            es = [e for e, (a, b) in enumerate(EDGES) if a in cs and b in cs]
            faces[axis, side] = (cs, es)
    return faces


FACES = cell_faces()
SAME_FACE = {(a, b) for _, es in FACES.values() for a in es for b in es if a != b}


def segments(case):
    """Directed segments (from edge, to edge) of one case: rules 1 and 2."""
    bit = [(case >> k) & 1 for k in range(8)]
    out = []
    for (axis, side), (cs, es) in FACES.items():
        crossed = [e for e in es if bit[EDGES[e][0]] != bit[EDGES[e][1]]]
        n = tuple((2 * side - 1) if d == axis else 0 for d in range(3))
        centre = tuple(sum(CORNERS[c][d] for c in cs) / 4 for d in range(3))
        pairs = []                                              # (edge, edge, a vector to the set side of the segment)
        if len(crossed) == 2:
            set_c = [c for c in cs if bit[c]]
            clear_c = [c for c in cs if not bit[c]]
            s = _sub(tuple(sum(CORNERS[c][d] for c in set_c) / len(set_c) for d in range(3)),
                     tuple(sum(CORNERS[c][d] for c in clear_c) / len(clear_c) for d in range(3)))
            pairs.append((crossed[0], crossed[1], s))
        elif len(crossed) == 4:
            for c in cs:
                if bit[c]:
                    a, b = [e for e in es if c in EDGES[e]]
                    pairs.append((a, b, _sub(CORNERS[c], centre)))
        else:
            assert not crossed
        for a, b, s in pairs:
            d = _sub(_mid(b), _mid(a))
            t = _dot(_cross(s, d), n)
            assert t != 0
            out.append((a, b) if t < 0 else (b, a))
    return out


def loops(case):
    nxt = {}
    for a, b in segments(case):
        assert a not in nxt
        nxt[a] = b
    assert sorted(nxt) == sorted(nxt.values())
    out, left = [], set(nxt)
    while left:
        e = first = min(left)
        loop = []
        while True:
            loop.append(e)
            left.remove(e)
            e = nxt[e]
            if e == first:
                break
        out.append(loop)
    return out


def triangulate(loop):
    """Rule 3: the first admissible triangulation, as a list of (a, b, c) edge ids; None when there is none."""
    n = len(loop)

    def ok(i, j):                                               # may v[i] - v[j] be a side of a triangle?
        if (j - i) % n in (1, n - 1):
            return True                                         # a side of the loop itself
        return (loop[i], loop[j]) not in SAME_FACE

    def part(lo, hi):
        if hi - lo < 2:
            return []
        for k in range(lo + 1, hi):
            if not (ok(lo, k) and ok(k, hi)):
                continue
            a = part(lo, k)
            if a is None:
                continue
            b = part(k, hi)
            if b is None:
                continue
            return [(loop[lo], loop[k], loop[hi])] + a + b
        return None

    return part(0, n - 1)


def table():
    rows = []
    for case in range(256):
        tris = []
        for loop in loops(case):
            assert 3 <= len(loop) <= 7
            t = triangulate(loop)
            assert t is not None and len(t) == len(loop) - 2
            tris += t
        assert len(tris) <= 5
        rows.append([e for t in tris for e in t])
    return rows


def header_text():
    rows = table()
    lines = ['// GENERATED by tools/gen_mcube_table.py -- do not edit; tests/test_mcube_cpu.py compares it with the generator.',
             '// Marching-cubes cases: bit k of the case is set iff value(corner k) < iso.  Row = triangles as cell edge ids, three per',
             '// triangle, ended by 255 (at most 5 triangles).  Corner and edge numbering, and the rules, are in the generator.',
             '#pragma once',
             '',
             '#define KAMD_MCUBE_ROW 16',
             '#ifndef KAMD_MCUBE_QUALIFIER  // (mcube.hip places the arrays in device memory)',
             '#define KAMD_MCUBE_QUALIFIER static const',
             '#endif',
             '',
             'KAMD_MCUBE_QUALIFIER unsigned char kamd_mcube_table[256 * KAMD_MCUBE_ROW] = {']
    for case, row in enumerate(rows):
        cells = row + [END] * (16 - len(row))
        lines.append('    ' + ', '.join(f'{v:3d}' for v in cells) + f',  // {case}')
    lines.append('};')
    lines.append('')
    lines.append('// triangles per case')
    lines.append('KAMD_MCUBE_QUALIFIER unsigned char kamd_mcube_num_triangles[256] = {')
    for i in range(0, 256, 32):
        lines.append('    ' + ', '.join(str(len(r) // 3) for r in rows[i:i + 32]) + ',')
    lines.append('};')
    return '\n'.join(lines) + '\n'


def main():
    text = header_text()
    if '--check' in sys.argv[1:]:
        with open(HEADER) as f:
            same = f.read() == text
        print('mcube_table.h is', 'up to date' if same else 'STALE')
        sys.exit(0 if same else 1)
    with open(HEADER, 'w') as f:
        f.write(text)
    print('wrote', os.path.normpath(HEADER))


if __name__ == '__main__':
    main()
