"""ops.spc.conv3d / conv_transpose3d, their layers and kaolin.rep.Spc on CPU tensors (the torch formulation), against the brute force
of tests/spc_conv_bruteforce.py -- and the brute force against torch's dense convolutions of the zero-filled grid, which is how the
reference's own test defines the operators.  Values and gradients are compared within `conv_bound`, derived from the arithmetic:
any order of T products rounded once each.  float32 and float64 accumulate in their own precision; half (and bfloat16) go through
the torch formulation, which accumulates in float32 and rounds the result once, so their sums take the float32 bound and their
final rounding the half unit.  The `check_*` helpers take a device: tests/test_spc_conv_gpu.py runs them through the HIP path."""
import itertools

import numpy as np
import pytest
import torch

import spc_bruteforce as bf
import spc_conv_bruteforce as cbf

NAME = {torch.float64: 'float64', torch.float32: 'float32', torch.float16: 'float16', torch.bfloat16: 'bfloat16'}


def kal():
    import kaolin_amd
    return kaolin_amd


def spc():
    return kal().ops.spc


def t(array, device, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(array), dtype=dtype).to(device)


def kernel(size, offset=0):
    """the size^3 kernel vectors starting at -offset, in the order the dense weights are laid out"""
    return np.array(list(itertools.product(range(-offset, size - offset), repeat=3)), dtype=np.int16)


def sparse_cube(shape, density, seed):
    """a random grid of `shape` inside the next power-of-two cube, as feature_grids_to_spc pads it"""
    rng = np.random.RandomState(seed)
    D = 1 << int(np.ceil(np.log2(max(shape))))
    cube = np.zeros((D, D, D), dtype=bool)
    cube[:shape[0], :shape[1], :shape[2]] = rng.rand(*shape) < density
    cube[tuple(rng.randint(0, s) for s in shape)] = True
    return cube


def hierarchies(points, pyramids):
    """per item of a packed batch an object with `level_points`, the points of every level: what the brute force reads"""
    items, first = [], 0
    for pyramid in np.asarray(pyramids):
        d = bf.Decoded()
        d.level_points = [np.asarray(points[first + pyramid[1, l]:first + pyramid[1, l + 1]]) for l in range(pyramid.shape[1] - 1)]
        first += int(pyramid[1, -1])
        items.append(d)
    return items


def chain(level, cell):
    """the packed batch of ONE octree with a single point per level, down to `cell` of `level`, written out by hand"""
    cell = np.asarray(cell, dtype=np.int64)
    points = np.stack([cell >> (level - l) for l in range(level + 1)]).astype(np.int16)
    child = [int(((points[l + 1, 0] & 1) << 2) | ((points[l + 1, 1] & 1) << 1) | (points[l + 1, 2] & 1)) for l in range(level)]
    pyramids = np.array([[[1] * (level + 1) + [0], list(range(level + 2))]], dtype=np.int32)
    return (np.array([1 << c for c in child], dtype=np.uint8), np.array([level], dtype=np.int32), pyramids,
            np.arange(1, level + 1, dtype=np.int32), points)


class ConvCase:
    """A batch of octrees, an operator and its arguments; the brute force's answers are computed once per dtype and kept."""

    def __init__(self, cubes, jump, kernel_vectors, transposed, cin, cout, seed=0, level=None):
        """cubes: a list of boolean 2^L cubes, or the packed batch itself: (octrees, lengths, pyramids, exsum, points) arrays"""
        octrees, lengths, pyramids, exsum, points = cubes if isinstance(cubes, tuple) else bf.decode_batch(cubes)[1:]
        self.decoded = hierarchies(points, pyramids)
        self.max_level = pyramids.shape[2] - 2
        self.octrees, self.lengths, self.pyramids, self.exsum, self.points = octrees, lengths, pyramids, exsum, points
        self.jump, self.transposed = jump, transposed
        self.level = level if level is not None else (self.max_level - jump if transposed else self.max_level)
        self.kernel_vectors = np.asarray(kernel_vectors, dtype=np.int16).reshape(-1, 3)
        self.K, self.cin, self.cout = len(self.kernel_vectors), cin, cout
        self.bf = cbf.triples(self.decoded, self.level, jump, self.kernel_vectors, transposed)
        rng = np.random.RandomState(seed)
        self.x = rng.uniform(-1, 1, (self.bf.n_in, cin))
        self.w = rng.uniform(-1, 1, (self.K, cin, cout))
        self.bias = rng.uniform(-1, 1, cout)
        self.g = rng.uniform(-1, 1, (self.bf.n_out, cout))
        self._kept = {}

    def structure(self, device):
        return (t(self.octrees, device), t(self.points, device), self.level, t(self.pyramids, 'cpu'), t(self.exsum, device))

    def tensors(self, device, dtype):
        """x, w, bias, g rounded to `dtype` (the brute force sees the rounded values)"""
        return tuple(t(a, device, torch.float64).to(dtype) for a in (self.x, self.w, self.bias, self.g))

    def want(self, dtype):
        if dtype not in self._kept:
            x, w, _, g = (a.double().numpy() for a in self.tensors('cpu', dtype))
            self._kept[dtype] = (cbf.forward(self.bf, x, w), cbf.grad_input(self.bf, g, w), cbf.grad_weight(self.bf, x, g, self.K))
        return self._kept[dtype]

    def op(self):
        return spc().conv_transpose3d if self.transposed else spc().conv3d


def make_case(cubes, jump, kernel_vectors, transposed, cin=2, cout=3, seed=0, level=None):
    return ConvCase(cubes, jump, kernel_vectors, transposed, cin, cout, seed, level)


def share_of_bound(got, want, bound):
    """the largest |got - want| / bound; where the bound is 0 (no product went into the element) the value must be exact"""
    got = got.detach().double().cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all()
    err = np.abs(got - want).astype(np.float64)
    assert (err[bound == 0] == 0).all(), 'an element without neighbours is not exactly 0'
    share = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
    print(f'share of the bound: {share:.3f}')
    assert share <= 1.0, share
    return share


def accumulates_in(device, dtype):
    """half and bfloat16 run the torch formulation on every device: float32 sums, one final rounding"""
    return 'float32' if dtype in (torch.float16, torch.bfloat16) else NAME[dtype]


def check_forward(case, device, dtype=torch.float32, bias=False, op=None):
    """the operator on `device` against the brute force within the bound -> (output, share of the bound used)"""
    x, w, b, _ = case.tensors(device, dtype)
    out, level = (op or case.op())(*case.structure(device), x, w, t(case.kernel_vectors, device), case.jump, b if bias else None)
    assert isinstance(level, int) and level == case.bf.out_level
    assert out.dtype == dtype and out.device.type == device and tuple(out.shape) == (case.bf.n_out, case.cout)
    want, abs_sum, count = case.want(dtype)[0]
    extra = 0.0
    if bias:        # one more term, added to the ROUNDED sum: the sum's own rounding stays in the bound
        extra = cbf.UNIT[NAME[dtype]] * np.abs(want)
        want, abs_sum, count = want + b.double().cpu().numpy(), abs_sum + np.abs(b.double().cpu().numpy()), count + 1
    bound = cbf.conv_bound(abs_sum, count, want, NAME[dtype], accumulates_in(device, dtype)) + extra
    return out, share_of_bound(out, want, bound)


def check_backward(case, device, dtype=torch.float32, which='both', op=None):
    """both gradients (or only `which`: 'input' / 'weight') for dL/dY = case.g -> (grad_input, grad_weight, share)"""
    x, w, _, g = case.tensors(device, dtype)
    x.requires_grad_(which in ('both', 'input'))
    w.requires_grad_(which in ('both', 'weight'))
    out, _ = (op or case.op())(*case.structure(device), x, w, t(case.kernel_vectors, device), case.jump)
    out.backward(g)
    _, want_x, want_w = case.want(dtype)
    share = 0.0
    if which in ('both', 'input'):
        assert x.grad.dtype == dtype and x.grad.shape == x.shape
        share = max(share, share_of_bound(x.grad, want_x[0], cbf.conv_bound(*want_x[1:], want_x[0], NAME[dtype],
                                                                             accumulates_in(device, dtype))))
    else:
        assert x.grad is None
    if which in ('both', 'weight'):
        assert w.grad.dtype == dtype and w.grad.shape == w.shape
        share = max(share, share_of_bound(w.grad, want_w[0], cbf.conv_bound(*want_w[1:], want_w[0], NAME[dtype],
                                                                             accumulates_in(device, dtype))))
    else:
        assert w.grad is None
    return x.grad, w.grad, share


# -------------------------------------------------------------------------------------------- the brute force is pinned to dense torch
def dense_of_rows(case, rows, level):
    """(B, C, D, D, D) float64: the rows of `level` scattered into the zero-filled grids"""
    D, B = 2 ** level, len(case.decoded)
    grid = np.zeros((B, rows.shape[1], D, D, D))
    first = 0
    for b, d in enumerate(case.decoded):
        pts = d.level_points[level].astype(np.int64)
        grid[b][:, pts[:, 0], pts[:, 1], pts[:, 2]] = rows[first:first + len(pts)].T
        first += len(pts)
    return grid


def dense_forward(case, size, offset):
    """torch's dense convolution of the zero-filled grid, read at the output level's points (its occupancy mask) -> rows"""
    F = torch.nn.functional
    s = 2 ** case.jump
    x = torch.from_numpy(dense_of_rows(case, case.x, case.level))
    w = torch.from_numpy(case.w)                                      # (K, in, out), k = the flattened (dx, dy, dz)
    if case.transposed:
        dense_w = w.permute(1, 2, 0).reshape(case.cin, case.cout, size, size, size)
        full = F.conv_transpose3d(x, dense_w, stride=s, output_padding=s - 1)
        E = 2 ** case.bf.out_level
        out = full[:, :, offset:offset + E, offset:offset + E, offset:offset + E]
    else:
        dense_w = w.permute(2, 1, 0).reshape(case.cout, case.cin, size, size, size)
        out = F.conv3d(F.pad(x, (offset, size - 1 - offset) * 3), dense_w, stride=s)
    assert out.shape[2:] == (2 ** case.bf.out_level,) * 3
    rows = []
    for b, d in enumerate(case.decoded):
        pts = d.level_points[case.bf.out_level].astype(np.int64)
        rows.append(out[b][:, pts[:, 0], pts[:, 1], pts[:, 2]].T.numpy())
    return np.concatenate(rows)


KERNELS = [(1, 0), (2, 0), (3, 0), (3, 1), (4, 0), (5, 2)]
SPARSE3 = [sparse_cube((5, 6, 7), 0.4, seed) for seed in (1, 2, 3)]
FULL = [np.ones((8, 8, 8), dtype=bool)]


# (K = 1 with jump 0 is the matmul shortcut, which has a test of its own; jump 3 = the level: one output point per item)
DENSE_CONFIGS = [(size, offset, jump) for size, offset in KERNELS for jump in (0, 1, 2, 3) if (size, jump) != (1, 0)]


@pytest.mark.parametrize('transposed', [False, True])
@pytest.mark.parametrize('size,offset,jump', DENSE_CONFIGS)
@pytest.mark.parametrize('cubes', [SPARSE3, SPARSE3[:1], FULL], ids=['batch3', 'batch1', 'full'])
def test_bruteforce_against_the_dense_convolution(cubes, size, offset, jump, transposed):
    case = make_case(cubes, jump, kernel(size, offset), transposed, seed=size + jump)
    want, abs_sum, count = cbf.forward(case.bf, case.x, case.w)
    dense = dense_forward(case, size, offset)
    # both are float64 sums of the same products (the dense one adds zeros): each within the bound of the exact value
    assert (np.abs(want - dense) <= 2 * cbf.conv_bound(abs_sum, count, want, 'float64')).all()
    if jump == 3 and not transposed:
        assert case.bf.n_out == len(cubes)


# ------------------------------------------------------------------------------------------------- the torch formulation
CPU_CASES = [(False, 0, (3, 1)), (False, 1, (2, 0)), (False, 2, (5, 2)), (False, 3, (4, 0)), (False, 1, (1, 0)),
             (True, 0, (3, 1)), (True, 1, (2, 0)), (True, 2, (5, 2)), (True, 3, (4, 0)), (True, 2, (1, 0)), (True, 2, (3, 0))]
_cases = {}


def cpu_case(transposed, jump, size_offset, batch=3):
    key = (transposed, jump, size_offset, batch)
    if key not in _cases:
        _cases[key] = make_case(SPARSE3[:batch], jump, kernel(*size_offset), transposed, cin=5, cout=7, seed=jump)
    return _cases[key]


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.float16], ids=['f32', 'f64', 'f16'])
@pytest.mark.parametrize('transposed,jump,size_offset', CPU_CASES)
def test_forward_cpu(transposed, jump, size_offset, dtype):
    case = cpu_case(transposed, jump, size_offset)
    check_forward(case, 'cpu', dtype)
    check_forward(case, 'cpu', dtype, bias=True)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64, torch.float16], ids=['f32', 'f64', 'f16'])
@pytest.mark.parametrize('transposed,jump,size_offset', CPU_CASES)
def test_backward_cpu(transposed, jump, size_offset, dtype):
    check_backward(cpu_case(transposed, jump, size_offset), 'cpu', dtype)


def test_forward_and_backward_cpu_single_item_and_bfloat16():
    check_forward(cpu_case(False, 1, (3, 1), batch=1), 'cpu', torch.float32, bias=True)
    check_backward(cpu_case(True, 1, (3, 1), batch=1), 'cpu', torch.float32)
    check_forward(cpu_case(False, 0, (3, 1)), 'cpu', torch.bfloat16)


def test_only_the_gradient_asked_for_cpu():
    case = cpu_case(False, 1, (2, 0))
    check_backward(case, 'cpu', which='input')
    check_backward(case, 'cpu', which='weight')


@pytest.mark.parametrize('transposed', [False, True])
@pytest.mark.parametrize('jump', [0, 1])
def test_gradcheck(transposed, jump):
    case = make_case([bf.random_cube(2, 7, density=0.4)], jump, kernel(2), transposed, cin=2, cout=3)
    x, w, b, _ = case.tensors('cpu', torch.float64)
    structure, kv = case.structure('cpu'), t(case.kernel_vectors, 'cpu')
    x.requires_grad_(), w.requires_grad_(), b.requires_grad_()
    assert torch.autograd.gradcheck(lambda x, w, b: case.op()(*structure, x, w, kv, jump, b)[0], (x, w, b))


# ------------------------------------------------------------------------------------------------------------ the contract's corners
def check_shortcut(device, dtype=torch.float32):
    """K = 1, jump = 0: input.mm(weight[0]) whatever the vector is, level unchanged"""
    for transposed in (False, True):
        case = make_case(SPARSE3[:2], 0, [[3, -2, 1]], transposed, cin=5, cout=7)
        x, w, b, _ = case.tensors(device, dtype)
        out, level = case.op()(*case.structure(device), x, w, t(case.kernel_vectors, device), 0, b)
        assert level == case.level and torch.equal(out, x.mm(w[0]) + b)


def check_all_misses(device, dtype=torch.float32):
    """a vector of +-2^level leaves the grid from every point: zero rows, a zero gradient for that k"""
    for transposed, jump in ((False, 0), (True, 0), (False, 1), (True, 1)):
        level = 3
        vectors = np.concatenate([kernel(2), [[2 ** level, 0, 0], [0, -2 ** level, 0]]]).astype(np.int16)
        case = make_case(SPARSE3[:2], jump, vectors, transposed, cin=3, cout=2)
        assert not any(k >= 8 for k, _, _ in case.bf.triples)
        _, grad_w, _ = check_backward(case, device, dtype)
        assert (grad_w[8:] == 0).all()
        only = make_case(SPARSE3[:2], jump, vectors[8:], transposed, cin=3, cout=2)
        out, _ = check_forward(only, device, dtype)
        assert (out == 0).all()
        out, _ = check_forward(only, device, dtype, bias=True)
        assert torch.equal(out, only.tensors(device, dtype)[2].expand_as(out))


def check_duplicate(device, dtype=torch.float32):
    """a vector listed twice contributes twice, each with its own weights"""
    for transposed in (False, True):
        vectors = np.concatenate([kernel(3, 1), kernel(3, 1)[13:15], kernel(3, 1)[:1]])
        case = make_case(SPARSE3[:2], 1, vectors, transposed, cin=3, cout=4)
        check_forward(case, device, dtype)
        check_backward(case, device, dtype)


def check_chain(device, dtype=torch.float32):
    """one point per level down to level 14, 3^3 kernel: only the centre offset has a neighbour, at 15-bit coordinates"""
    for transposed in (False, True):
        case = make_case(chain(14, [16383, 10922, 5461]), 0, kernel(3, 1), transposed, cin=3, cout=2)
        assert [(k, o, i) for k, o, i in case.bf.triples] == [(13, 0, 0)] and case.level == 14
        check_forward(case, device, dtype)
        check_backward(case, device, dtype)


def test_shortcut():
    check_shortcut('cpu')


def test_chain_to_level_14():
    check_chain('cpu')


def test_vectors_that_leave_the_grid():
    check_all_misses('cpu')


def test_duplicate_vectors():
    check_duplicate('cpu')


def check_modules(device):
    S = spc()
    torch.manual_seed(3)
    for cls, fn, transposed in ((S.Conv3d, S.conv3d, False), (S.ConvTranspose3d, S.conv_transpose3d, True)):
        case = make_case(SPARSE3[:2], 1, kernel(3, 1), transposed, cin=5, cout=7)
        kv = t(case.kernel_vectors, 'cpu')
        for with_bias in (True, False):
            layer = cls(5, 7, kv, jump=1, bias=with_bias).to(device)
            assert dict(layer.named_parameters()).keys() == ({'weight', 'bias'} if with_bias else {'weight'})
            assert tuple(layer.weight.shape) == (27, 5, 7) and layer.kernel_shape == (27, 5, 7)
            assert [n for n, _ in layer.named_buffers()] == ['kernel_vectors'] and torch.equal(layer.kernel_vectors.cpu(), kv)
            fan = 27 * (7 if transposed else 5)
            assert 0.5 / np.sqrt(fan) < layer.weight.detach().abs().max().item() <= 1 / np.sqrt(fan)
            assert with_bias == (layer.bias is not None) and (not with_bias or layer.bias.detach().abs().max().item() <= 1 / np.sqrt(fan))
            assert repr(layer) == f'{cls.__name__}(in=5, out=7, kernel_vector_size=27)'
            x = case.tensors(device, torch.float32)[0]
            out, level = layer(*case.structure(device), x)
            want, want_level = fn(*case.structure(device), x, layer.weight, layer.kernel_vectors, 1, layer.bias)
            assert level == want_level == case.bf.out_level and torch.equal(out, want)
            out.sum().backward()
            assert layer.weight.grad is not None and (not with_bias or layer.bias.grad is not None)
            with pytest.raises(TypeError, match=f'{cls.__name__} got an unexpected keyword argument colour'):
                layer(*case.structure(device), x, colour=1)
            layer(*case.structure(device), x, lengths=t(case.lengths, 'cpu'), max_level=case.max_level)     # members of Spc.KEYS pass


def test_modules():
    check_modules('cpu')


def test_unexpected_keywords():
    case = cpu_case(False, 1, (2, 0))
    x, w, _, _ = case.tensors('cpu', torch.float32)
    kv = t(case.kernel_vectors, 'cpu')
    for name in ('conv3d', 'conv_transpose3d'):
        with pytest.raises(TypeError, match=f'{name} got an unexpected keyword argument stride'):
            getattr(spc(), name)(*case.structure('cpu'), x, w, kv, 1, stride=2)
    out, _ = spc().conv3d(*case.structure('cpu'), x, w, kv, 1, lengths=t(case.lengths, 'cpu'), max_level=3)
    assert torch.equal(out, spc().conv3d(*case.structure('cpu'), x, w, kv, 1)[0])


def bad_arguments(case, device):
    """(what is wrong, positional arguments of the operator, a word of the message): every ValueError of the contract"""
    octrees, points, level, pyramids, exsum = case.structure(device)
    x, w, b, _ = case.tensors(device, torch.float32)
    kv = t(case.kernel_vectors, device)
    other = 'cpu' if device != 'cpu' else 'meta'
    good = [octrees, points, level, pyramids, exsum, x, w, kv, case.jump, b]

    def swap(**changes):
        names = ['octrees', 'points', 'level', 'pyramids', 'exsum', 'x', 'w', 'kv', 'jump', 'b']
        return [changes.get(n, v) for n, v in zip(names, good)]
    L = case.max_level
    out_of_range = dict(level=0, jump=1) if not case.transposed else dict(level=L, jump=1)
    return [
        ('level above the pyramid', swap(level=L + 1), 'level'), ('negative level', swap(level=-1), 'level'),
        ('negative jump', swap(jump=-1), 'jump'), ('target level outside', swap(**out_of_range), 'output level'),
        ('rows of input', swap(x=x[:-1]), 'input must be of size'), ('input not 2D', swap(x=x[None]), 'input must be of size'),
        ('in channels of weight', swap(w=w[:, :-1]), 'weight must be of size'), ('K of weight', swap(w=w[:-1]), 'weight must be of size'),
        ('weight not 3D', swap(w=w[0]), 'weight must be of size'),
        ('kernel_vectors int32', swap(kv=kv.int()), 'kernel_vectors must be short'),
        ('kernel_vectors (K, 2)', swap(kv=kv[:, :2]), 'kernel_vectors must be short'),
        *([('pyramids on the device', swap(pyramids=pyramids.to(device)), 'pyramids must be')] if device != 'cpu' else []),
        ('pyramids 2D', swap(pyramids=pyramids[0]), 'pyramids must be'),
        ('weight elsewhere', swap(w=w.to(other)), 'weight is on'), ('octrees elsewhere', swap(octrees=octrees.to(other)), 'octrees is on'),
        ('exsum elsewhere', swap(exsum=exsum.to(other)), 'exsum is on'), ('bias elsewhere', swap(b=b.to(other)), 'bias is on'),
        ('weight double', swap(w=w.double()), 'one dtype'), ('bias half', swap(b=b.half()), 'one dtype'),
        ('bias size', swap(b=b[:-1]), 'bias must be of size'),
        ('legacy exsum', swap(exsum=torch.cat([exsum.new_zeros(1), exsum])), 'current layout'),
        ('octree bytes', swap(octrees=octrees[:-1]), 'octrees must be'), ('points', swap(points=points[:-1]), 'point_hierarchies must be'),
    ]


def check_bad_arguments(device):
    for transposed in (False, True):
        case = make_case(SPARSE3[:2], 1, kernel(2), transposed, cin=3, cout=2)
        for what, args, word in bad_arguments(case, device):
            with pytest.raises(ValueError, match=word):
                case.op()(*args)
                pytest.fail(what)


def test_bad_arguments():
    check_bad_arguments('cpu')


def test_a_neighbour_table_of_2_to_the_31_entries_is_refused():
    """K * n_out < 2^31 is checked from the pyramid alone: nothing of that size is allocated"""
    check = kal()._C.ops.spc_conv_check
    n = 2 ** 20
    pyramids = torch.tensor([[[1, n, 0], [0, 1, 1 + n]]], dtype=torch.int32)
    meta = dict(device='meta')
    args = (torch.empty(1, dtype=torch.uint8, **meta), torch.empty((1 + n, 3), dtype=torch.int16, **meta), 1, pyramids,
            torch.empty(1, dtype=torch.int32, **meta), torch.empty((n, 1), **meta))
    check('conv3d', False, *args, torch.empty((2047, 1, 1), **meta), torch.empty((2047, 3), dtype=torch.int16, **meta), 0)
    with pytest.raises(ValueError, match='below 2\\^31'):
        check('conv3d', False, *args, torch.empty((2048, 1, 1), **meta), torch.empty((2048, 3), dtype=torch.int16, **meta), 0)


# ------------------------------------------------------------------------------------------------------------------- kaolin.rep.Spc
def check_spc_class(device):
    K, S, Spc = kal(), spc(), kal().rep.Spc
    assert Spc.KEYS == {'octrees', 'lengths', 'max_level', 'pyramids', 'exsum', 'point_hierarchies'}
    case = make_case(SPARSE3, 1, kernel(3, 1), False, cin=3, cout=2)
    octrees, lengths = t(case.octrees, device), t(case.lengths, 'cpu')
    s = Spc(octrees, lengths)
    assert s._max_level is None and s._pyramids is None and s._exsum is None and s._point_hierarchies is None     # lazily
    max_level, pyramids, exsum = S.scan_octrees(octrees, lengths)
    assert s.max_level == max_level == 3 and s._pyramids is not None and s._exsum is not None and s._point_hierarchies is None
    assert torch.equal(s.pyramids, pyramids) and torch.equal(s.exsum, exsum) and s.exsum.device.type == device
    assert torch.equal(s.point_hierarchies, S.generate_points(octrees, pyramids, exsum)) and s.batch_size == 3
    assert torch.equal(s.point_hierarchies.cpu(), t(case.points, 'cpu'))
    assert torch.equal(s.num_points(2), pyramids[:, 0, 2]) and s.num_points(0).tolist() == [1, 1, 1]
    assert set(s.to_dict()) == Spc.KEYS and set(s.to_dict(keys=['octrees', 'exsum'])) == {'octrees', 'exsum'}
    x, w, _, _ = case.tensors(device, torch.float32)
    kv = t(case.kernel_vectors, device)
    out, level = S.conv3d(**s.to_dict(), level=s.max_level, input=x, weight=w, kernel_vectors=kv, jump=1)
    want, _ = S.conv3d(*case.structure(device), x, w, kv, 1)
    assert level == 2 and torch.equal(out, want)
    dense = S.to_dense(**s.to_dict(), input=out, level=level)
    assert torch.equal(dense, S.to_dense(s.point_hierarchies, s.pyramids, out, level))
    given = Spc(octrees, lengths, max_level, pyramids, exsum, s.point_hierarchies, features=x)
    assert given.exsum is exsum and given.pyramids is pyramids and given.features is x
    assert s.to(device) is s
    listed = Spc.from_list(list(torch.split(octrees, case.lengths.tolist())))
    assert torch.equal(listed.octrees, octrees) and torch.equal(listed.lengths, lengths) and listed.lengths.dtype == torch.int32
    grids = torch.zeros((2, 3, 5, 6, 7), device=device)
    grids[0, :, 1, 2, 3] = torch.tensor([1.0, 2.0, 3.0], device=device)
    grids[1, 1, 4, 5, 6] = 4.0
    f = Spc.from_features(grids)
    o, l, feats = S.feature_grids_to_spc(grids)
    assert torch.equal(f.octrees, o) and torch.equal(f.lengths, l) and torch.equal(f.features, feats) and f.max_level == 3
    masked = Spc.from_features(grids, masks=torch.ones((2, 5, 6, 7), dtype=torch.bool, device=device))
    assert masked.num_points(3).tolist() == [210, 210]
    dense_spc = Spc.make_dense(2, device)
    assert dense_spc.octrees.tolist() == [255] * 9 and dense_spc.lengths.tolist() == [9] and dense_spc.max_level == 2
    assert dense_spc.num_points(2).tolist() == [64] and dense_spc.octrees.device.type == device
    return s


def test_spc_class():
    s = check_spc_class('cpu')
    assert s.cpu() is s


def test_spc_class_checks_its_arguments():
    Spc = kal().rep.Spc
    octrees, lengths = torch.tensor([255], dtype=torch.uint8), torch.tensor([1], dtype=torch.int32)
    pyramids = torch.tensor([[[1, 8, 0], [0, 1, 9]]], dtype=torch.int32)
    exsum = torch.tensor([8], dtype=torch.int32)
    Spc(octrees, lengths, 1, pyramids, exsum, torch.zeros((9, 3), dtype=torch.int16))
    for args, word in [((octrees.int(), lengths), 'octrees must be'), ((octrees[None], lengths), 'octrees must be'),
                       ((octrees, lengths.long()), 'lengths must be'), ((octrees, lengths, 1.0), 'max_level'),
                       ((octrees, lengths, 1, pyramids.long()), 'pyramids must be an IntTensor'),
                       ((octrees, lengths, 2, pyramids), 'pyramids must be of shape'),
                       ((octrees, lengths, 1, pyramids[0]), 'pyramids must be of shape'),
                       ((octrees, lengths, 1, pyramids, exsum.long()), 'exsum must be an IntTensor'),
                       ((octrees, lengths, 1, pyramids, exsum[None]), 'exsum must be a 1D'),
                       ((octrees, lengths, 1, pyramids, exsum, torch.zeros((9, 3))), 'point_hierarchies must be a ShortTensor'),
                       ((octrees, lengths, 1, pyramids, exsum, torch.zeros((9, 2), dtype=torch.int16)), 'point_hierarchies must be of shape'),
                       ((octrees, lengths, 1, pyramids, exsum, None, [1.0]), 'features must be')]:
        with pytest.raises(AssertionError, match=word):
            Spc(*args)
    with pytest.raises(ValueError, match='current layout'):
        Spc(octrees, lengths, exsum=torch.tensor([0, 8], dtype=torch.int32))
    import kaolin_amd
    kaolin = kaolin_amd.install_as_kaolin()
    import kaolin.rep
    assert kaolin.rep.Spc is Spc
