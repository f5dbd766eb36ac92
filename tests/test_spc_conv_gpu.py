"""ops.spc.conv3d / conv_transpose3d through the HIP path (csrc/spc_conv.hip): the `check_*` helpers of tests/test_spc_conv_cpu.py on
CUDA tensors, at the smallest shapes at which each kernel can go wrong.  Everything is compared with the float64 brute force of
tests/spc_conv_bruteforce.py within `conv_bound` (any order of T products rounded once each; float32 and float64 accumulate in
their own precision on the HIP path, half goes through the torch formulation with float32 sums).  No out-of-range index, malformed
octree or pyramid that disagrees with its hierarchy is launched on the GPU."""
import numpy as np
import pytest
import torch

import spc_bruteforce as bf
from test_spc_conv_cpu import (SPARSE3, bad_arguments, check_all_misses, check_backward, check_chain, check_duplicate,
                               check_forward, check_modules, check_shortcut, check_spc_class, kal, kernel, make_case, t)

pytestmark = pytest.mark.gpu

ROWS_PER_TILE = 64      # output rows of a workgroup of the gather-GEMM (csrc/spc_conv.hip SC_ROWS)
COLS_PER_TILE = 64      # its output channels (SC_COLS); also the (in, out) tile of the weight gradient
CHANNEL_STEP = {torch.float32: 32, torch.float64: 16}     # channels staged per step (ScTile<T>::CK); the MFMA shape is 16x16x4
WGRAD_SLICES = 32       # row slices of the weight gradient (SC_SLICES); a slice is a multiple of CHANNEL_STEP rows
MAP_BLOCK = 256         # (offset, row) pairs per block of the map kernel (SC_MAP_BLOCK)
T = ROWS_PER_TILE
DTYPES = [torch.float32, torch.float64]
IDS = ['f32', 'f64']


def cube_with_cells(level, cells, seed):
    """a cube of `level` with exactly `cells` occupied cells: that many points at the deepest level"""
    rng = np.random.RandomState(seed)
    flat = np.zeros(8 ** level, dtype=bool)
    flat[rng.choice(8 ** level, cells, replace=False)] = True
    return flat.reshape((2 ** level,) * 3)


def both(case, dtype, bias=False):
    _, a = check_forward(case, 'cuda', dtype, bias=bias)
    _, _, b = check_backward(case, 'cuda', dtype)
    return max(a, b)


# ----------------------------------------------------------------------------------------------------------------- the row tile
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('rows', [1, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1])
def test_rows_around_the_tile(rows, dtype):
    """jump 0: the output rows of the forward and of the gradient by the input are the `rows` cells"""
    for transposed in (False, True):
        case = make_case([cube_with_cells(3, rows, rows)], 0, kernel(3, 1), transposed, cin=5, cout=7)
        assert case.bf.n_out == case.bf.n_in == rows
        both(case, dtype)


@pytest.mark.parametrize('rows', [MAP_BLOCK - 1, MAP_BLOCK, MAP_BLOCK + 1])
def test_rows_around_the_block_of_the_map_kernel(rows):
    for transposed in (False, True):
        both(make_case([cube_with_cells(4, rows, rows)], 0, kernel(2), transposed, cin=3, cout=2), torch.float32)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_rows_around_the_capacity_of_one_step_per_slice(dtype):
    """up to WGRAD_SLICES * CHANNEL_STEP rows every slice of the weight gradient is one step; one row more and a slice takes two"""
    full = WGRAD_SLICES * CHANNEL_STEP[dtype]
    for rows in (full - 1, full, full + 1):
        case = make_case([cube_with_cells(4, rows, rows)], 0, kernel(2), False, cin=3, cout=2)
        assert case.bf.n_in == rows
        check_backward(case, 'cuda', dtype)


# ------------------------------------------------------------------------------------------------------------------- the channels
CHANNELS = [(1, 1), (1, 7), (5, 1), (5, 7), (4, 16), (16, 16), (17, 33), (33, 17), (64, 64),       # around the MFMA shape and a step
            (COLS_PER_TILE + 1, 2), (2, COLS_PER_TILE + 1)]     # a second column tile of the gather, a second tile of the weight gradient


@pytest.fixture(scope='module')
def channel_cube():
    return [cube_with_cells(3, T + 9, 5)]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('cin,cout', CHANNELS)
def test_channel_padding(channel_cube, cin, cout, dtype):
    for transposed, jump in ((False, 0), (True, 1)):
        both(make_case(channel_cube, jump, kernel(2), transposed, cin=cin, cout=cout, seed=cin), dtype, bias=True)


# --------------------------------------------------------------------------------------------------------------------- the offsets
@pytest.mark.parametrize('size,offset,jump', [(1, 0, 1), (2, 0, 0), (3, 1, 0), (4, 1, 0), (5, 2, 0)])
def test_number_of_offsets(channel_cube, size, offset, jump):
    for transposed in (False, True):
        case = make_case(channel_cube, jump, kernel(size, offset), transposed, cin=5, cout=7)
        assert case.K == size ** 3
        both(case, torch.float32)


# ----------------------------------------------------------------------------------------------------------------------- the jumps
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('jump', [0, 1, 2, 3])
def test_jumps(jump, dtype):
    """jump 3 is the level: one output point per item for conv3d, one input point for the transpose; the 2^3 and 3^3 kernels of the
    transpose are smaller than the strides 4 and 8"""
    for transposed in (False, True):
        for size, offset in ((2, 0), (3, 1), (5, 2)):
            both(make_case(SPARSE3[:2], jump, kernel(size, offset), transposed, cin=3, cout=4), dtype)


def test_levels_below_the_deepest():
    """input at level 2 of a level-3 octree: the per-item offsets of an inner level"""
    both(make_case(SPARSE3, 1, kernel(3, 1), False, cin=3, cout=4, level=2), torch.float32)
    both(make_case(SPARSE3, 1, kernel(3, 1), True, cin=3, cout=4, level=1), torch.float32)


# ------------------------------------------------------------------------------------------------------------------------ the batch
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_batch_of_unequal_items(dtype):
    """1, about T and several T points at the input level: the per-item offsets into octrees, exsum, point_hierarchies, input and
    output"""
    cubes = [cube_with_cells(3, 1, 1), cube_with_cells(3, T + 3, 2), cube_with_cells(3, 4 * T + 5, 3)]
    for order in (cubes, cubes[::-1]):
        for transposed, jump in ((False, 0), (False, 1), (True, 0), (True, 1)):
            both(make_case(order, jump, kernel(3, 1), transposed, cin=5, cout=7), dtype)


def test_level_1_octree():
    for transposed in (False, True):
        for jump in (0, 1):
            both(make_case([bf.cube_of_points([[0, 0, 0], [1, 0, 1], [1, 1, 1]], 1)], jump, kernel(3, 1), transposed, cin=2, cout=3),
                 torch.float32)


def test_chain_to_level_14_gpu():
    check_chain('cuda')
    check_chain('cuda', torch.float64)


# ---------------------------------------------------------------------------------------------------------------------- tile skip
def test_tiles_without_and_with_one_neighbour():
    """64 cells at even coordinates have no neighbour but themselves, one more cell next to one of them gives exactly one row of a
    tile a neighbour for (1, 0, 0) and one for (-1, 0, 0): the skipped offsets and the offsets kept for a single row"""
    cube = np.zeros((8, 8, 8), dtype=bool)
    cube[::2, ::2, ::2] = True
    cube[5, 4, 4] = True
    for transposed in (False, True):
        case = make_case([cube], 0, kernel(3, 1), transposed, cin=5, cout=7)
        assert case.bf.n_out == T + 1
        hits = np.zeros((27, 2), dtype=int)
        for k, o, _ in case.bf.triples:
            hits[k, o // T] += 1
        assert (hits == 0).any() and (hits == 1).any() and hits[13].tolist() == [T, 1]
        both(case, torch.float32)
        both(case, torch.float64)


# ------------------------------------------------------------------------------------------------------------ the weight gradient
def test_weight_gradient_slices():
    """the full 8^3 octree: 512 rows, so 16 of the slices hold 32 rows each and 16 are empty.  Offset 0 hits in every row, (6, 6, 6)
    only in 8 rows at one end (one slice), (4, 4, 4) in one octant (two slices), (1, 0, 0) in half of every slice"""
    cube = np.ones((8, 8, 8), dtype=bool)
    vectors = [[0, 0, 0], [6, 6, 6], [4, 4, 4], [1, 0, 0]]
    for transposed in (False, True):
        case = make_case([cube], 0, vectors, transposed, cin=5, cout=7)
        per_k = np.bincount([k for k, _, _ in case.bf.triples], minlength=4)
        assert per_k.tolist() == [512, 8, 64, 448]
        for dtype in DTYPES:
            check_backward(case, 'cuda', dtype, which='weight')
            check_backward(case, 'cuda', dtype, which='input')
            check_backward(case, 'cuda', dtype)


def test_more_rows_than_one_step_per_slice():
    """4096 rows (the full 16^3 octree): 128 rows a slice, four steps of 32 (eight of 16 for double)"""
    case = make_case([np.ones((16, 16, 16), dtype=bool)], 0, [[0, 0, 0], [1, 1, 1], [-1, 0, 2]], False, cin=3, cout=2)
    for dtype in DTYPES:
        check_backward(case, 'cuda', dtype)


# ----------------------------------------------------------------------------------------------------- determinism, recycled memory
def run(case, dtype):
    x, w, _, g = case.tensors('cuda', dtype)
    x.requires_grad_(), w.requires_grad_()
    out, _ = case.op()(*case.structure('cuda'), x, w, t(case.kernel_vectors, 'cuda'), case.jump)
    out.backward(g)
    return out.detach(), x.grad, w.grad


@pytest.fixture(scope='module')
def bigger():
    return {tr: make_case([cube_with_cells(4, 5 * T + 7, 9)] * 2, 1 - int(tr), kernel(3, 1), tr, cin=17, cout=33) for tr in (False, True)}


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_results_are_bit_identical_from_run_to_run(bigger, dtype):
    for case in bigger.values():
        first, second = run(case, dtype), run(case, dtype)
        assert all(torch.equal(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_results_do_not_depend_on_recycled_memory(bigger, dtype):
    """every buffer of a call is torch.empty: with the allocator's free blocks full of NaN bits before each call the results stay
    within the bound and equal to the first call's"""
    for case in bigger.values():
        kept = None
        for _ in range(2):
            junk = [torch.full((n,), -1, dtype=torch.int32, device='cuda') for n in (1024, 16384, 131072, 1048576) for _ in range(4)]
            del junk
            out, _ = check_forward(case, 'cuda', dtype)
            grad_x, grad_w, _ = check_backward(case, 'cuda', dtype)
            kept = kept or (out, grad_x, grad_w)
            assert all(torch.equal(a, b) for a, b in zip(kept, (out, grad_x, grad_w)))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_hip_path_against_the_cpu_path(bigger, dtype):
    """both are within their bound of the brute force (checked by the helpers), so within the sum of the bounds of each other"""
    for case in bigger.values():
        for device in ('cuda', 'cpu'):
            check_forward(case, device, dtype, bias=True)
            check_backward(case, device, dtype)


def test_half_and_bfloat16_take_the_torch_formulation_on_the_gpu(bigger):
    for case in bigger.values():
        check_forward(case, 'cuda', torch.float16, bias=True)
        check_backward(case, 'cuda', torch.float16)
        check_forward(case, 'cuda', torch.bfloat16)


def test_only_the_gradient_asked_for():
    case = make_case(SPARSE3[:2], 1, kernel(2), False, cin=5, cout=7)
    check_backward(case, 'cuda', which='input')
    check_backward(case, 'cuda', which='weight')


# -------------------------------------------------------------------------------------------------------------- the contract's corners
def test_shortcut_gpu():
    check_shortcut('cuda')


def test_vectors_that_leave_the_grid_gpu():
    check_all_misses('cuda')
    check_all_misses('cuda', torch.float64)


def test_duplicate_vectors_gpu():
    check_duplicate('cuda')


def test_modules_gpu():
    check_modules('cuda')


def test_spc_class_gpu():
    s = check_spc_class('cuda')
    assert s.cuda() is s
    moved = s.cpu()
    assert moved is not s and moved.octrees.device.type == 'cpu' and moved.exsum.device.type == 'cpu'
    assert torch.equal(moved.point_hierarchies, s.point_hierarchies.cpu()) and moved.pyramids is s.pyramids
    assert kal().rep.Spc.make_dense(1).octrees.is_cuda


# ----------------------------------------------------------------------------------------------------------------------- the shims
def shim_arguments(case, backward):
    octrees, points, level, pyramids, exsum = case.structure('cuda')
    x, w, _, g = case.tensors('cuda', torch.float32)
    kv = t(case.kernel_vectors, 'cuda')
    if backward:
        return [octrees, points, case.bf.out_level, pyramids, exsum, x, g, w, kv, case.jump]
    return [octrees, points, level, pyramids, exsum, x, w, kv, case.jump]


def test_shims_against_the_public_interface_and_their_refusals():
    ops = kal()._C.ops.spc
    for transposed, name in ((False, 'Conv3d'), (True, 'ConvTranspose3d')):
        case = make_case(SPARSE3[:2], 1, kernel(2), transposed, cin=5, cout=7)
        forward, backward = getattr(ops, name + '_forward'), getattr(ops, name + '_backward')
        out, level = forward(*shim_arguments(case, False))
        want, _ = check_forward(case, 'cuda')
        assert level == case.bf.out_level and torch.equal(out, want)
        grads = backward(*shim_arguments(case, True))
        want_x, want_w, _ = check_backward(case, 'cuda')
        assert isinstance(grads, list) and torch.equal(grads[0], want_x) and torch.equal(grads[1], want_w)
        for shim, is_backward in ((forward, False), (backward, True)):
            good = shim_arguments(case, is_backward)
            for position in (0, 1, 4, 5, 6, 7) + ((8,) if is_backward else ()):
                args = list(good)
                args[position] = args[position].cpu()
                with pytest.raises(RuntimeError, match='CUDA'):
                    shim(*args)
            args = list(good)
            args[5] = args[5][:-1]
            with pytest.raises(ValueError, match='input must be of size'):
                shim(*args)
            args = list(good)
            args[-1] = -1
            with pytest.raises(ValueError, match='jump'):
                shim(*args)
            args = list(good)
            args[5] = args[5].half()
            with pytest.raises(ValueError, match='one dtype'):
                shim(*args)


def test_bad_arguments_are_refused_before_any_launch():
    for transposed in (False, True):
        case = make_case(SPARSE3[:2], 1, kernel(2), transposed, cin=3, cout=2)
        for what, args, word in bad_arguments(case, 'cuda'):
            with pytest.raises(ValueError, match=word):
                case.op()(*args)
                pytest.fail(what)


# --------------------------------------------------------------------------------------------------------------------- a real case
def test_layers_on_the_sphere_octree():
    """the level-6 octree of the geodesic sphere through Spc(...).to_dict(): Conv3d (jump 1) to level 5 and ConvTranspose3d (jump 1)
    back to level 6, each layer's forward and gradients against the brute force"""
    K = kal()
    from kaolin_amd.utils.testing import geodesic_sphere
    v, f = geodesic_sphere(8)
    octree = K.ops.conversions.unbatched_mesh_to_spc((v.float() * 1.2)[f].contiguous().cuda(), 6)[0]
    s = K.rep.Spc(octree, torch.tensor([octree.numel()], dtype=torch.int32))
    packed = (s.octrees.cpu().numpy(), s.lengths.numpy(), s.pyramids.numpy(), s.exsum.cpu().numpy(), s.point_hierarchies.cpu().numpy())
    assert s.max_level == 6 and int(s.num_points(6)) > 20 * T
    down = make_case(packed, 1, kernel(3, 1), False, cin=4, cout=8, seed=1)
    up = make_case(packed, 1, kernel(2), True, cin=8, cout=4, seed=2, level=5)
    torch.manual_seed(0)
    conv, deconv = K.ops.spc.Conv3d(4, 8, t(down.kernel_vectors, 'cuda'), jump=1).cuda(), \
        K.ops.spc.ConvTranspose3d(8, 4, t(up.kernel_vectors, 'cuda'), jump=1).cuda()
    with torch.no_grad():
        conv.weight.copy_(down.tensors('cuda', torch.float32)[1])
        deconv.weight.copy_(up.tensors('cuda', torch.float32)[1])
        conv.bias.zero_(), deconv.bias.zero_()
    x = down.tensors('cuda', torch.float32)[0]
    hidden, level = conv(**s.to_dict(), level=6, input=x)
    assert level == 5 and tuple(hidden.shape) == (int(s.num_points(5)), 8)
    out, level = deconv(**s.to_dict(), level=level, input=hidden)
    assert level == 6 and tuple(out.shape) == (int(s.num_points(6)), 4)
    out.sum().backward()
    assert conv.weight.grad is not None and deconv.weight.grad is not None and torch.isfinite(conv.weight.grad).all()
    want, _ = check_forward(down, 'cuda')
    assert torch.equal(hidden, want)
    shares = [check_backward(down, 'cuda')[2], check_forward(up, 'cuda')[1], check_backward(up, 'cuda')[2]]
    print('sphere: shares of the bound', shares)
