"""The FlexiCubes case tables as Python lists, read once from the generated header the HIP kernels compile
(csrc/flexicubes_table.h, written by tools/gen_flexicubes_table.py, which has the rules):

    DMC_TABLE[case][group]   the crossed cube edges of one dual vertex, ascending, padded with -1 to 7; 4 groups
    NUM_VD_TABLE[case]       the number of groups
    CHECK_TABLE[case]        (marked, normal x, y, z, replacement case) of the ambiguity rule
"""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..', '..', 'csrc', 'flexicubes_table.h')


def _load():
    with open(HEADER) as f:
        text = re.sub(r'//[^\n]*', '', f.read())
    bodies = re.findall(r'=\s*\{([^}]*)\}', text)
    if len(bodies) != 2:
        raise RuntimeError(f'{HEADER}: not the generated FlexiCubes tables')
    words = [int(w, 16) for w in re.findall(r'0x([0-9a-fA-F]+)', bodies[0])]
    marks = [int(m) for m in re.findall(r'\d+', bodies[1])]
    if len(words) != 256 or len(marks) != 256:
        raise RuntimeError(f'{HEADER}: not the generated FlexiCubes tables')
    dmc, num_vd, check = [], [], []
    for case in range(256):
        groups = [[e for e in range(12) if (words[case] >> (4 * e)) & 15 == g] for g in range(4)]
        dmc.append([(g + [-1] * 7)[:7] for g in groups])
        num_vd.append((words[case] >> 48) & 15)
        row = [0, 0, 0, 0, 0]
        if marks[case]:
            axis, side = (marks[case] - 1) >> 1, (marks[case] - 1) & 1
            row = [1, 0, 0, 0, 255 - case]
            row[1 + axis] = 1 if side else -1
        check.append(row)
    return dmc, num_vd, check


DMC_TABLE, NUM_VD_TABLE, CHECK_TABLE = _load()
