"""kaolin.ops.voxelgrid and kaolin.metrics.voxelgrid on CPU tensors against the reference's recorded outputs
(golden/voxelgrid_ops.npz).  Everything is boolean, integer or exactly representable: torch.equal everywhere, no tolerance
(``nan`` in iou compared as equal)."""
import builtins
import re

import pytest
import torch

import kaolin_amd as kal
from kaolin_amd.ops import voxelgrid as vg
from kaolin_amd.metrics import voxelgrid as vgm
from voxelgrid_golden import FILL_BINARY_CASES, error, grid, tensor


def raises_like(name):
    kind, text = error(name)
    return pytest.raises(getattr(builtins, kind), match=re.escape(text))


# ---- fill --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', FILL_BINARY_CASES)
@pytest.mark.parametrize('dtype', [torch.bool, torch.float32, torch.int64])
def test_fill_matches_reference(name, dtype):
    out = vg.fill(grid(f'fill_{name}_in').to(dtype))
    assert out.dtype == torch.bool and not out.requires_grad
    assert torch.equal(out, grid(f'fill_{name}_out'))


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32, torch.float64])
def test_fill_wall_is_nonzero(dtype):
    """0.4, -1 and nan are walls, -0.0 is empty, the enclosed 0 fills."""
    out = vg.fill(tensor('fill_values_in').to(dtype))
    assert torch.equal(out, grid('fill_values_out'))
    assert out[0, 1, 1, 1] and not out[0, 2, 0, 0]


def test_fill_non_contiguous_and_grad_input():
    x = grid('fill_shell_puncture_in').float()
    view = x.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1)
    assert not view.is_contiguous()
    assert torch.equal(vg.fill(view), grid('fill_shell_puncture_out'))
    out = vg.fill(grid('fill_doc_in').float().requires_grad_())
    assert not out.requires_grad and torch.equal(out, grid('fill_doc_out'))


@pytest.mark.parametrize('shape', [(3, 4, 5), (1, 1, 3, 4, 5)])
def test_fill_rank_error(shape):
    with pytest.raises(ValueError, match=re.escape(f'Expected voxelgrids to have 4 dimensions but got {len(shape)} dimensions.')):
        vg.fill(torch.zeros(shape))


def test_fill_empty_batch():
    assert vg.fill(torch.zeros(0, 3, 3, 3)).shape == (0, 3, 3, 3)


# ---- extract_surface -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['wide', 'thin'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bool, torch.float64])
def test_extract_surface(mode, dtype):
    out = vg.extract_surface(tensor('surface_in').to(dtype), mode)
    assert out.dtype == torch.bool
    assert torch.equal(out, grid(f'surface_{mode}'))


def test_extract_surface_default_is_wide():
    assert torch.equal(vg.extract_surface(tensor('surface_in')), grid('surface_wide'))


def test_extract_surface_errors():
    with raises_like('surface_mode'):
        vg.extract_surface(tensor('surface_in'), 'narrow')
    with raises_like('surface_ndim'):
        vg.extract_surface(tensor('surface_in')[0])


# ---- downsample ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,scale', [('int2', 2), ('list232', [2, 3, 2]), ('list461', [4, 6, 1]), ('tuple223', (2, 2, 3)),
                                       ('int1', 1)])
def test_downsample(tag, scale):
    out = vg.downsample(tensor('down_in'), scale)
    assert out.dtype == torch.float32
    assert torch.equal(out, tensor(f'down_{tag}'))


def test_downsample_bool_goes_through_float():
    out = vg.downsample(tensor('down_bool_in'), 2)
    assert out.dtype == torch.float32 and torch.equal(out, tensor('down_bool_int2'))
    assert vg.downsample(tensor('down_in').double(), 2).dtype == torch.float64


@pytest.mark.parametrize('name,make', [
    ('down_list_len', lambda x: vg.downsample(x, [2, 2])),
    ('down_ndim', lambda x: vg.downsample(x.unsqueeze(0), [2, 2, 2])),
    ('down_small', lambda x: vg.downsample(x, [2, 0, 2])),
    ('down_large', lambda x: vg.downsample(x, [2, 2, 7])),
    ('down_type', lambda x: vg.downsample(x, 2.5)),
    ('down_int_large', lambda x: vg.downsample(x, 7)),
])
def test_downsample_errors(name, make):
    with raises_like(name):
        make(tensor('down_in'))


def test_force_float():
    assert vg._force_float(torch.zeros(2, dtype=torch.bool)).dtype == torch.float32
    for dtype in (torch.float16, torch.float64, torch.int64, torch.uint8):
        assert vg._force_float(torch.zeros(2, dtype=dtype)).dtype == dtype


# ---- odms ----------------------------------------------------------------------------------------------------------------
def test_extract_odms():
    out = vg.extract_odms(tensor('odm_vox'))
    assert out.dtype == torch.long and torch.equal(out, tensor('odm_odms'))
    assert torch.equal(vg.extract_odms(tensor('odm_vox').float()), tensor('odm_odms_float'))


@pytest.mark.parametrize('votes', [1, 2, 7])
@pytest.mark.parametrize('src', ['exact', 'noisy'])
def test_project_odms(votes, src):
    odms = tensor('odm_odms' if src == 'exact' else 'odm_noisy')
    out = vg.project_odms(odms, votes=votes)
    assert out.dtype == torch.bool and torch.equal(out, grid(f'proj_{src}_v{votes}'))
    out = vg.project_odms(odms, voxelgrids=tensor('odm_vox'), votes=votes)
    assert out.dtype == torch.bool and torch.equal(out, grid(f'proj_{src}_v{votes}_vox'))


def test_project_odms_leaves_its_input_alone_and_defaults_to_one_vote():
    odms = tensor('odm_noisy').clone()
    out = vg.project_odms(odms)
    assert torch.equal(odms, tensor('odm_noisy')) and torch.equal(out, grid('proj_noisy_v1'))


def test_project_odms_errors():
    odms, vox = tensor('odm_odms'), tensor('odm_vox')
    with raises_like('proj_six'):
        vg.project_odms(odms[:, :5])
    with raises_like('proj_batch'):
        vg.project_odms(odms, voxelgrids=vox[:1])
    with raises_like('proj_dim'):
        vg.project_odms(odms, voxelgrids=torch.ones(2, 5, 4, 5))


# ---- iou -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [torch.float32, torch.bool])
def test_iou(dtype):
    out = vgm.iou(tensor('iou_pred').to(dtype), tensor('iou_gt').to(dtype))
    want = tensor('iou_out')
    assert out.dtype == torch.float32 and out.shape == (3,)
    assert torch.isnan(want[2]) and torch.isnan(out[2])          # the empty union
    assert torch.equal(out[:2], want[:2])


def test_iou_shape_error():
    with raises_like('iou_shape'):
        vgm.iou(tensor('iou_pred'), tensor('iou_gt')[:, :3])


# ---- wiring --------------------------------------------------------------------------------------------------------------
def test_public_names_and_install_as_kaolin():
    assert kal.ops.voxelgrid is vg and kal.metrics.voxelgrid is vgm
    for name in ('downsample', 'extract_surface', 'fill', 'extract_odms', 'project_odms', '_force_float'):
        assert callable(getattr(vg, name))
    kal.install_as_kaolin()
    import kaolin.ops.voxelgrid
    import kaolin.metrics.voxelgrid
    assert kaolin.ops.voxelgrid.fill is vg.fill and kaolin.metrics.voxelgrid.iou is vgm.iou


def test_fill_workspace_query_is_host_only():
    from kaolin_amd import _lib
    ws = _lib.load().kamd_voxelgrid_fill_workspace
    one = ws(1, 256, 256, 256)
    assert one >= 2 * 256 ** 3 // 8 and one < 2 * 256 ** 3 // 8 + 4096      # two bit grids and a few control words
    assert ws(8, 256, 256, 256) > 7 * one and ws(1, 70, 45, 37) >= 2 * 70 * 45 * 2 * 4     # rows padded to whole words
    assert ws(0, 4, 4, 4) == 0 and ws(1, 0, 4, 4) == 0
