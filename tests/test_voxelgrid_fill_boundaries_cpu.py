"""ops.voxelgrid.fill at the word, brick, pass-batch and grid-stride edges of csrc/voxelgrid_fill.hip, without a GPU: the CPU path
(``_fill_torch``, the repeated-shift fixed point) against the breadth-first oracle of tests/voxelgrid_fill_cases.py on every case
of the suite, the oracle against SciPy's ``binary_fill_holes`` (the reference's own definition) where SciPy is installed, and
the properties that make the cases worth running: every random case has cavities to fill and outside voxels to reach, the built
ones are what test_voxelgrid_fill_boundaries_gpu.py says of them.  torch.equal everywhere."""
import numpy as np
import pytest
import torch

import voxelgrid_fill_cases as cases
from kaolin_amd.ops import voxelgrid as vg

# X = 1 or Y = 1 puts every voxel on a boundary face: such a grid has no cavity and nothing off the faces, whatever its volume
THIN = [name for name, (_, x, y, z) in cases.RANDOM_SHAPES.items() if min(x, y, z) <= 2]
CONDITIONED = [name for name, shape in cases.RANDOM_SHAPES.items()
               if int(np.prod(shape)) >= cases.MIN_VOLUME and name not in THIN]


@pytest.mark.parametrize('name', cases.NAMES)
def test_cpu_path_matches_oracle(name):
    grid = cases.case(name)
    out = vg.fill(torch.from_numpy(grid.copy()))                  # (the cached case is read-only)
    assert out.dtype == torch.bool and out.shape == grid.shape
    assert torch.equal(out, torch.from_numpy(cases.expected(name).copy()))


@pytest.mark.parametrize('name', CONDITIONED)
def test_random_cases_have_cavities_and_reached_voxels(name):
    """at least 50 cavity voxels (filled, not wall) and at least 50 outside voxels on no boundary face, in every batch item"""
    cavity, outside = cases.counts(cases.case(name), cases.expected(name))
    print(name, cases.case(name).shape, 'cavity', cavity, 'outside off the faces', outside)
    assert (cavity >= cases.MIN_COUNT).all() and (outside >= cases.MIN_COUNT).all()


def test_condition_covers_every_random_case_that_can_meet_it():
    """The random cases outside the condition are those below 1000 voxels and the grids one or two voxels thick, in which every
    voxel lies on a boundary face: their fill is their walls."""
    small = [name for name, shape in cases.RANDOM_SHAPES.items() if int(np.prod(shape)) < cases.MIN_VOLUME]
    assert sorted(set(small) | set(THIN) | set(CONDITIONED)) == sorted(cases.RANDOM_SHAPES)
    assert set(THIN) == {'z1', 'z2', 'xy1x1', 'xy1x40', 'xy40x1', 'xy2x2'}
    assert set(CONDITIONED) >= {f'z{z}' for z in cases.Z_SIZES if z >= 63} | {'batch', 'xy15x17', 'xy31x33', 'xy33x31'}
    for name in THIN:
        assert np.array_equal(cases.expected(name), cases.case(name)) and not cases.case(name).all()


@pytest.mark.parametrize('name', ['z513', 'xy31x33', 'batch'])
def test_oracle_matches_scipy(name):
    ndimage = pytest.importorskip('scipy.ndimage')
    six = ndimage.generate_binary_structure(3, 1)
    grid = cases.case(name)
    want = np.stack([ndimage.binary_fill_holes(item, structure=six) for item in grid])
    assert np.array_equal(cases.expected(name), want)


def test_oracle_on_a_grid_small_enough_to_read():
    """a 3 x 3 x 3 shell fills, the same shell with a hole in one face does not, and a value is a wall when it is not 0"""
    shell = np.ones((2, 3, 3, 3))
    shell[:, 1, 1, 1] = 0
    shell[1, 1, 1, 2] = 0
    shell[0, 0, 0, 0] = -0.5
    out = cases.fill_oracle(shell)
    assert out[0].all() and not out[1, 1, 1, 1] and not out[1, 1, 1, 2] and out[1].sum() == 25
    assert cases.fill_oracle(np.zeros((0, 3, 3, 3))).shape == (0, 3, 3, 3)


def test_carry_cases_are_what_they_claim():
    """a, b, c: the whole row is reached; d, e: the row above the wall voxel is a cavity; f: a cavity of 13 voxels over z = 256"""
    row = {name: ~cases.expected(name)[0, 1, 1] for name in cases.CARRY_NAMES}          # True = outside
    for name in cases.CARRY_NAMES:
        assert cases.expected(name).sum() == 9 * 513 - row[name].sum()                  # nothing outside but in the row
    assert row['carry_a'].all()
    assert row['carry_b'][:512].all() and not row['carry_b'][512]
    assert row['carry_c'][1:].all() and not row['carry_c'][0]
    assert row['carry_d'][:255].all() and not row['carry_d'][255:].any() and not cases.case('carry_d')[0, 1, 1, 256:512].any()
    assert row['carry_e'][:256].all() and not row['carry_e'][256:].any() and not cases.case('carry_e')[0, 1, 1, 257:512].any()
    assert not row['carry_f'].any() and (~cases.case('carry_f')).sum() == 13 and cases.expected('carry_f').all()


@pytest.mark.parametrize('name,axis,cut', [('corridor_z', 3, 256), ('corridor_x', 1, 16), ('corridor_y', 2, 16)])
def test_corridor_is_one_open_path_that_crosses_the_brick_33_times(name, axis, cut):
    """The flood reaches every corridor voxel (the fill is the input), the corridor has one voxel on a boundary face, and 33 of
    its rows hold both the voxel below the cut and the voxel above it."""
    grid, out = cases.case(name), cases.expected(name)
    assert np.array_equal(out, grid)
    empty = ~grid
    assert empty.sum() - cases.off_faces(empty).sum() == 1
    below, above = np.take(empty, cut - 1, axis=axis), np.take(empty, cut, axis=axis)
    assert (below & above).sum() == 33
    if name == 'corridor_z':
        assert empty.sum() == 451


def test_many_bricks_tail_items_have_a_cavity_and_a_reached_voxel():
    """4101 bricks, 36909 rows and 1.37 M unpack threads; among the five items past the 4096 workgroups of a pass at least one has a
    cavity and at least one an outside voxel on no boundary face (here: the odd ones both, the even ones the latter)"""
    grid = cases.case('many_bricks')
    assert grid.shape == cases.MANY_SHAPE and grid.shape[0] > 4096 and grid.shape[0] * 9 > 16384 and grid.size > 1048576
    cavity, outside = cases.counts(grid, cases.expected('many_bricks'))
    tail = list(cases.MANY_TAIL)
    print('tail items: cavity', cavity[tail], 'outside off the faces', outside[tail])
    assert (cavity[tail] > 0).any() and (outside[tail] > 0).any()
    assert (cavity[:4096] > 0).sum() > 1000 and (outside[:4096] > 0).sum() > 1000
