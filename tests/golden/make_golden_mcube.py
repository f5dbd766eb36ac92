"""Generates tests/golden/mcube_examples.json from the RECORDED cases of the reference's own TestMarchingCube
(tests/python/kaolin/ops/conversions/test_voxelgrid.py): per case the 2 x 2 x 2 uint8 grid and the vertices and faces the
reference's test expects of kaolin.ops.conversions.voxelgrids_to_trianglemeshes.  Data only: the three tensor literals of every
``test_voxelgrids_to_trianglemeshes_<n>`` method are read with ``ast.literal_eval``; nothing of the reference is executed (its
operator needs a CUDA device).

Run in the build container (where the reference tree is mounted):
    python tests/golden/make_golden_mcube.py
"""
import ast
import json
import os
import re

import _refload

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, 'mcube_examples.json')
SRC = os.path.join(_refload.REF, 'tests/python/kaolin/ops/conversions/test_voxelgrid.py')
NAMES = ('voxelgrid', 'expected_vertices', 'expected_faces')


def recorded_cases():
    with open(SRC) as f:
        tree = ast.parse(f.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == 'TestMarchingCube')
    cases = {}
    for fn in cls.body:
        m = isinstance(fn, ast.FunctionDef) and re.fullmatch(r'test_voxelgrids_to_trianglemeshes_(\d+)', fn.name)
        if not m:
            continue
        got = {}
        for st in fn.body:
            if isinstance(st, ast.Assign) and isinstance(st.targets[0], ast.Name) and st.targets[0].id in NAMES:
                call = st.value                                 # torch.tensor(<literal>, device=..., dtype=...)
                assert isinstance(call, ast.Call) and call.func.attr == 'tensor'
                got[st.targets[0].id] = ast.literal_eval(call.args[0])
        assert sorted(got) == sorted(NAMES), fn.name
        cases[int(m.group(1))] = got
    return [cases[k] for k in sorted(cases)]


def main():
    cases = recorded_cases()
    assert len(cases) == 14, len(cases)
    for c in cases:
        assert len(c['voxelgrid']) == 2 and all(len(r) == 2 and all(len(q) == 2 for q in r) for r in c['voxelgrid'])
        nv = len(c['expected_vertices'])
        assert all(len(v) == 3 for v in c['expected_vertices']) and all(len(f) == 3 for f in c['expected_faces'])
        assert all(0 <= i < nv for f in c['expected_faces'] for i in f)
        # every recorded coordinate is a multiple of 0.5: exact in float32 and in JSON
        assert all(float(x) * 2 == int(float(x) * 2) for v in c['expected_vertices'] for x in v)
    with open(OUT, 'w') as f:
        json.dump([{'voxelgrid': c['voxelgrid'], 'vertices': c['expected_vertices'], 'faces': c['expected_faces']} for c in cases],
                  f, separators=(',', ':'))
        f.write('\n')
    print('wrote', OUT, len(cases), 'cases', os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
