"""CPU: ``_C.average_view_masks`` on host tensors (``libovis_cpu.so``) against the same float32 expression written with
torch ops -- ``torch.flip(..., [-1])`` for mirrored views, a left-to-right sum, then a division by V -- by exact equality."""
import itertools

import pytest
import torch

SHAPES = list(itertools.product((1, 2, 3), (0, 1, 5), (14, 28)))   # V, D, M


def maps_and_flips(v, d, m):
    g = torch.Generator().manual_seed(1000 * v + 10 * d + m)
    maps = torch.rand(v, d, 1, m, m, generator=g)
    flips = [bool((k + v) % 2) for k in range(v)]                  # V = 1: mirrored; V = 2: [False, True]; V = 3: [True, False, True]
    return maps, flips


def expression(maps, flips):
    """The mean as torch ops on HOST tensors; the divisor is a tensor, so the division is a division."""
    total = None
    for m, flip in zip(maps, flips):
        m = torch.flip(m, [-1]) if flip else m
        total = m if total is None else total + m
    return total / torch.tensor(float(len(flips)), dtype=torch.float32)


@pytest.mark.parametrize("v,d,m", SHAPES)
def test_host_twin_equals_the_expression(v, d, m):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    maps, flips = maps_and_flips(v, d, m)
    got = _C.average_view_masks(maps, flips)
    assert got.dtype == torch.float32 and tuple(got.shape) == (d, 1, m, m)
    assert torch.equal(got, expression(maps, flips))
    if d:
        assert not torch.equal(got, expression(maps, [not f for f in flips]))   # the flips matter


@pytest.mark.parametrize("m", (14, 28))
def test_one_view_is_returned_bit_for_bit_and_a_mirrored_pair_is_its_map(m):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    one = torch.rand(1, 5, 1, m, m, generator=torch.Generator().manual_seed(m))
    one[0, 0, 0, 0, :4] = torch.tensor([0.0, 1.0, 1e-42, 3e-39])             # zeros, ones and subnormals survive "/ 1"
    assert torch.equal(_C.average_view_masks(one, [False]), one[0])
    assert torch.equal(_C.average_view_masks(one, [True]), torch.flip(one[0], [-1]))
    pair = torch.stack([one[0], torch.flip(one[0], [-1])])                    # the same map, plain and pre-mirrored
    assert torch.equal(_C.average_view_masks(pair, [False, True]), one[0])


def test_argument_errors():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    maps = torch.zeros(2, 3, 1, 14, 14)
    with pytest.raises(RuntimeError, match="expected"):
        _C.average_view_masks(maps, [False])
    with pytest.raises(RuntimeError, match="expected"):
        _C.average_view_masks(maps[:, :, 0], [False, False])
    with pytest.raises(RuntimeError, match="expected"):
        _C.average_view_masks(maps.double(), [False, False])
    with pytest.raises(RuntimeError, match="expected"):
        _C.average_view_masks(torch.zeros(2, 3, 1, 14, 7), [False, False])
    with pytest.raises(RuntimeError, match="at most 64"):
        _C.average_view_masks(torch.zeros(65, 1, 1, 2, 2), [False] * 65)
