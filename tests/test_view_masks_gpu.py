"""GPU: ``_C.average_view_masks`` (csrc/box_vote.hip) against the float32 expression of tests/test_view_masks.py, by exact
equality.  The expression is evaluated with torch ops on the host copy of the maps: additions and a division are IEEE
operations there, while a device tensor divided by a scalar is multiplied by its reciprocal, which is another number for V = 3."""
import pytest
import torch

from tests.test_view_masks import SHAPES, expression, maps_and_flips

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("v,d,m", SHAPES)
def test_kernel_equals_the_expression(v, d, m):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    maps, flips = maps_and_flips(v, d, m)
    got = _C.average_view_masks(maps.cuda(), flips)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (d, 1, m, m)
    assert torch.equal(got.cpu(), expression(maps, flips))
    assert torch.equal(got.cpu(), _C.average_view_masks(maps, flips))          # the host twin, same bits


@pytest.mark.parametrize("m", (14, 28))
def test_one_view_is_returned_bit_for_bit_and_a_mirrored_pair_is_its_map(m):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    one = torch.rand(1, 5, 1, m, m, generator=torch.Generator().manual_seed(m))
    one[0, 0, 0, 0, :4] = torch.tensor([0.0, 1.0, 1e-42, 3e-39])             # subnormals survive "/ 1"
    one = one.cuda()
    assert torch.equal(_C.average_view_masks(one, [False]), one[0])
    assert torch.equal(_C.average_view_masks(one, [True]), torch.flip(one[0], [-1]))
    pair = torch.stack([one[0], torch.flip(one[0], [-1])])
    assert torch.equal(_C.average_view_masks(pair, [False, True]), one[0])


def test_more_elements_than_one_grid_pass():
    """4096 workgroups of 256 threads cover 2^20 elements in one pass; 1400 maps of 28 x 28 take the grid-stride loop."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    maps = torch.rand(2, 1400, 1, 28, 28, generator=torch.Generator().manual_seed(3))
    assert maps[0].numel() > 4096 * 256
    got = _C.average_view_masks(maps.cuda(), [False, True])
    assert torch.equal(got.cpu(), expression(maps, [False, True]))
