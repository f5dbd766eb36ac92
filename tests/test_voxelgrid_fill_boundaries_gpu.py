"""The HIP flood fill (csrc/voxelgrid_fill.hip) at the edges of its words, chunks, pack rounds, bricks, pass batches and
grid-stride loops: every comparison is torch.equal against the breadth-first oracle of tests/voxelgrid_fill_cases.py, which
test_voxelgrid_fill_boundaries_cpu.py pins to the CPU path and to SciPy and whose cases it shows to be what they claim.

Which test reaches which branch (from the shapes):
    bricks along Z, `below` / `above` carries          test_z_sizes[257 ... 513], test_carries_across_z_256, test_corridor_*
    second / third round of the pack kernel            test_z_sizes[257 ... 289] / test_z_sizes[513], test_carries_across_z_256
    last-voxel seed in a new word, dropped ballot half test_z_sizes[31 ... 65, 127 ... 129]
    unpack 16-wide / 4-wide / 1-wide                   test_z_sizes[32, 64, 128, 256, 288, 512] / [260] / the odd sizes
    unpack 4-wide / 1-wide for an unaligned output     test_unaligned_output_through_the_c_abi[4] / [1]
    halo at X or Y = 16, 32; X = 1, Y = 1              test_xy_sizes
    fourth host read (more than 2 + 4 + 8 passes)      test_corridor_across_z_takes_more_than_three_batches
    second brick of a workgroup, grid-stride loops     test_more_bricks_than_workgroups"""
import pytest
import torch

import voxelgrid_fill_cases as cases
from kaolin_amd import _C, _lib
from kaolin_amd.ops import voxelgrid as vg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# the kernel's constants (csrc/voxelgrid_fill.hip, csrc/common.h)
VF_BX = VF_BY = 16          # rows of a brick along X and Y
VF_WZ = 8                   # words of a brick along Z: 256 voxels
VF_POLL = 8                 # passes per batch after the batches of 2 and 4
BLOCK_CAP = 256 * 16        # KAMD_NUM_CU * 16 workgroups: a pass has more bricks than that -> a workgroup takes a second one
PACK_WAVES = BLOCK_CAP * 4  # rows the pack kernel takes at once (one per wavefront)
UNPACK_THREADS = BLOCK_CAP * 256

EDGE_CASES = ['z257', 'z513', 'xy31x33']
WALL = {torch.float16: 1, torch.float64: 0.4, torch.int64: -(2 ** 40), torch.uint8: 128}


def on_gpu(name):
    return torch.from_numpy(cases.case(name).copy()).to(DEV)


def want(name):
    return torch.from_numpy(cases.expected(name).copy())


def check(name, x=None):
    out = vg.fill(on_gpu(name) if x is None else x)
    assert out.dtype == torch.bool and out.shape == cases.case(name).shape
    assert torch.equal(out.cpu(), want(name)), int((out.cpu() != want(name)).sum())
    return out


@pytest.mark.parametrize('z', cases.Z_SIZES)
def test_z_sizes(z):
    """5 x 6 x Z random: W = 1 ... 17 words, one to nine chunks, one to three pack rounds, one to three bricks along Z, the three
    unpack widths"""
    check(f'z{z}')


@pytest.mark.parametrize('x,y', cases.XY_SIZES)
def test_xy_sizes(x, y):
    """X x Y x 33 random, X and Y at one row, below, at and past one and two bricks"""
    check(f'xy{x}x{y}')


def test_batch_at_brick_scale():
    """3 x 17 x 33 x 65: 2 x 3 bricks per item; every item is also the fill of that item alone"""
    out = check('batch')
    x = on_gpu('batch')
    for n in range(x.shape[0]):
        assert torch.equal(vg.fill(x[n:n + 1]), out[n:n + 1])


@pytest.mark.parametrize('name', cases.CARRY_NAMES)
def test_carries_across_z_256(name):
    """one empty row of 3 x 3 x 513 that is open below, above, at both ends or at neither, or cut at z = 255 / 256: whatever is
    reached is reached through the carry bits between the three bricks along Z"""
    check(name)


def test_corridor_across_z_takes_more_than_three_batches():
    """The corridor of 33 rows crosses z = 256 once per row, and the visits it needs, in order, are lower, upper, lower, ... brick of
    the same 16 rows of Y (nine visits for each of four pairs, then two in the last).  A launch visits a brick once, so a pass
    serves at most two visits of one pair, three where the front moves on to the next pair (lower, next lower, next upper): the
    38 visits take at least 4 passes in the first pair, then 1 + 3 for each pair after it, 17 passes that change something, and
    one more finds nothing to do -- more than the 2 + 4 + 8 passes of the first three batches, so the host reads a fourth time."""
    stats = {}
    out = _C.ops.voxelgrid_fill_cuda(on_gpu('corridor_z'), stats=stats)
    print('corridor_z', stats)
    assert torch.equal(out.cpu(), want('corridor_z'))
    assert stats['passes'] >= 17
    assert stats['polls'] >= 4 and stats['launched'] == 2 + 4 + VF_POLL * (stats['polls'] - 2)


@pytest.mark.parametrize('name', ['corridor_x', 'corridor_y'])
def test_corridor_across_a_brick_face(name):
    """the same corridor across x = 16 and across y = 16: every crossing goes through the LDS halo of the next brick"""
    check(name)


def test_more_bricks_than_workgroups():
    """4101 items of one brick each: the workgroups 0 ... 4 of a pass take a second brick (the items 4096 ... 4100, which have
    cavities and reached voxels: see the CPU suite), the pack kernel's wavefronts a third row, the unpack's threads a second
    byte"""
    n, x, y, z = cases.MANY_SHAPE
    assert n > BLOCK_CAP and 2 * PACK_WAVES < n * x * y and UNPACK_THREADS < n * x * y * z < 2 * UNPACK_THREADS
    check('many_bricks')


@pytest.mark.parametrize('strided', [False, True], ids=['contiguous', 'z_step_2'])
@pytest.mark.parametrize('dtype', list(WALL), ids=lambda d: str(d).split('.')[-1])
@pytest.mark.parametrize('name', EDGE_CASES)
def test_types_and_strides_at_the_edges(name, dtype, strided):
    x = (on_gpu(name).to(torch.float64) * WALL[dtype]).to(dtype)
    if strided:
        n, sx, sy, sz = x.shape
        padded = torch.full((n, sx + 2, sy + 3, 2 * sz + 1), 7, dtype=dtype, device=DEV)
        sliced = padded[:, 1:-1, 2:-1, 1::2]
        sliced.copy_(x)
        x = sliced
        assert not x.is_contiguous() and x.stride(3) == 2
    check(name, x)


@pytest.mark.parametrize('offset', [0, 4, 1])
def test_unaligned_output_through_the_c_abi(offset):
    """Z = 32 allows the 16-wide unpack; an output pointer 4 past a 16-byte boundary takes the 4-wide one, 1 past it the 1-wide one.
    The output lies inside a longer buffer of 0xAB, which must be untouched around it."""
    lib = _lib.load()
    grid = cases.case('z32')
    n, sx, sy, sz = grid.shape
    x = on_gpu('z32').to(torch.uint8)
    buffer = torch.full((grid.size + 16,), 0xAB, dtype=torch.uint8, device=DEV)
    assert buffer.data_ptr() % 16 == 0 and x.is_contiguous()
    ws = _lib.workspace(lib.kamd_voxelgrid_fill_workspace(n, sx, sy, sz), x.device)
    status = lib.kamd_voxelgrid_fill_u8(_lib.stream_ptr(x.device), n, sx, sy, sz, x.data_ptr(), *x.stride(),
                                        buffer.data_ptr() + offset, ws.data_ptr(), None)
    assert status == 0
    got = buffer.cpu()
    assert torch.equal(got[offset:offset + grid.size].view(grid.shape), want('z32').to(torch.uint8))
    assert (got[:offset] == 0xAB).all() and (got[offset + grid.size:] == 0xAB).all()
