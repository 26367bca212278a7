"""GPU: the device run-length encoder of pasted masks (csrc/mask_rle.hip: ``_C.pasted_masks_runs`` / ``pasted_masks_rle``)
against ``_C.paste_masks`` on the same inputs, copied to the host and encoded by the NumPy restatement of pycocotools
(tests/coco_rle_reference.py) -- integers and bytes compared exactly.  The shapes are the smallest at which the encoder
can go wrong: every edge of the image, runs that merge across column boundaries, a box wider than two workgroups, far more
runs than lanes, counts of five characters and negative differences."""
import numpy as np
import pytest
import torch

from tests import coco_rle_reference as rle

pytestmark = pytest.mark.gpu


def _device_rles(probs, boxes, sizes, threshold=0.5):
    """-> per mask (counts list, string bytes) from the two device entry points."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    args = (torch.as_tensor(probs, dtype=torch.float32).cuda(), torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4).cuda(),
            torch.as_tensor(sizes, dtype=torch.int32).reshape(-1, 2).cuda())
    counts, run_offsets = _C.pasted_masks_runs(*args, threshold)
    data, char_offsets = _C.pasted_masks_rle(*args, threshold)
    p = args[0].shape[0]
    assert counts.dtype == torch.int32 and data.dtype == torch.uint8 and counts.is_cuda and data.is_cuda
    assert run_offsets.dtype == char_offsets.dtype == torch.int64 and run_offsets.shape == char_offsets.shape == (p + 1,)
    ro, co = run_offsets.tolist(), char_offsets.tolist()
    assert ro[0] == co[0] == 0 and ro[-1] == counts.numel() and co[-1] == data.numel()
    counts, data = counts.cpu().numpy(), data.cpu().numpy()
    return [(counts[ro[i]:ro[i + 1]].tolist(), bytes(data[co[i]:co[i + 1]])) for i in range(p)]


def _pasted(probs, boxes, sizes, threshold=0.5):
    """The oracle: one ``paste_masks`` call per mask at its own image size -> list of uint8 [h, w]."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    probs = torch.as_tensor(probs, dtype=torch.float32).cuda()
    boxes = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4).cuda()
    return [_C.paste_masks(probs[i:i + 1], boxes[i:i + 1], (int(h), int(w)), threshold)[0].cpu().numpy().astype(np.uint8)
            for i, (h, w) in enumerate(np.asarray(sizes).reshape(-1, 2))]


def _check(probs, boxes, sizes, threshold=0.5):
    """Both device outputs equal the encoded oracle; -> (the oracle's masks, the device counts)."""
    masks = _pasted(probs, boxes, sizes, threshold)
    got = _device_rles(probs, boxes, sizes, threshold)
    assert len(got) == len(masks)
    for i, (mask, (counts, text)) in enumerate(zip(masks, got)):
        want = rle.rle_encode(mask)
        assert counts == want, (i, mask.shape, counts[:8], want[:8], len(counts), len(want))
        assert text == rle.rle_to_string(want), (i, text[:40])
    return masks, [g[0] for g in got]


def _maps(p, m, seed):
    return np.random.RandomState(seed).rand(p, m, m).astype(np.float32)


def _checkerboard(m):
    y, x = np.mgrid[0:m, 0:m]
    return ((y + x) % 2).astype(np.float32)[None]


def _row_stripes(m):
    """Rows in alternating pairs of ones and zeros, constant along x: every column of the pasted mask has run ends."""
    return np.repeat(((np.arange(m) // 2) % 2 == 0).astype(np.float32)[:, None], m, 1)[None]


def test_one_pixel_image():
    masks, counts = _check(np.stack([np.ones((14, 14), np.float32), np.zeros((14, 14), np.float32)]),
                           [[-5, -5, 5, 5], [-5, -5, 5, 5]], [[1, 1], [1, 1]])
    assert masks[0].all() and not masks[1].any()
    assert counts == [[0, 1], [1]]


@pytest.mark.parametrize("m", [1, 14, 28])
@pytest.mark.parametrize("threshold", [0.5, 0.3])
def test_random_maps_inside_and_clipped_at_every_edge(m, threshold):
    h, w = 37, 53
    boxes = [[10.3, 8.2, 40.7, 30.1],                                            # inside
             [-12, 9, 20, 25], [35, 5, 70.5, 30], [12, -9.5, 40, 18], [8, 20, 44, 60],   # left, right, top, bottom
             [-6, -4, 60, 41], [30, 20, 52.2, 36.4], [0, 0, 52, 36]]               # all four; bottom right corner; the image's box
    masks, _ = _check(_maps(len(boxes), m, 10 + m), boxes, [[h, w]] * len(boxes), threshold)
    if m > 1:
        assert all(0 < k.sum() < h * w for k in masks)


def test_no_masks():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    empty = (torch.zeros(0, 14, 14).cuda(), torch.zeros(0, 4).cuda(), torch.zeros(0, 2, dtype=torch.int32).cuda())
    for fn, dtype in ((_C.pasted_masks_runs, torch.int32), (_C.pasted_masks_rle, torch.uint8)):
        out, offsets = fn(*empty)
        assert out.shape == (0,) and out.dtype == dtype and offsets.tolist() == [0]


def test_boxes_that_miss_the_image_and_a_degenerate_box():
    h, w = 30, 40
    boxes = [[-30, 5, -8, 20], [48, 5, 70, 20], [5, -30, 20, -8], [5, 40, 20, 60], [30, 5, 12, 20], [5, 22, 20, 9]]
    masks, counts = _check(np.ones((len(boxes), 14, 14), np.float32), boxes, [[h, w]] * len(boxes))
    assert not any(k.any() for k in masks) and counts == [[h * w]] * len(boxes)


def test_runs_merge_across_column_boundaries():
    h, w = 21, 19
    ones = np.ones((1, 14, 14), np.float32)
    striped = ones.copy()
    striped[0, 6] = 0                          # one interior row of zeros
    big = [[-w, -h, 2 * w, 2 * h]]             # the map's interior covers the whole image
    masks, counts = _check(np.concatenate([ones, striped]), big * 2, [[h, w]] * 2)
    assert masks[0].all() and counts[0] == [0, h * w]
    assert masks[1][0].all() and masks[1][-1].all() and not masks[1].all()
    assert len(counts[1]) == 2 * w + 2          # every column's zeros, the ones merging across every column boundary
    # touching the bottom but not the top; touching the right edge and the bottom with the last pixel set
    masks, counts = _check(np.repeat(ones, 2, 0), [[3, 6, w - 4, 3 * h], [w // 2, h // 2, 2 * w, 2 * h]], [[h, w]] * 2)
    assert masks[0][-1].any() and not masks[0][0].any()
    assert masks[1][-1, -1] and not masks[1][0].any() and len(counts[1]) % 2 == 0


def test_a_box_wider_than_two_workgroups():
    h, w = 5, 700
    masks, counts = _check(_row_stripes(14), [[20, -2, 680, 8]], [[h, w]])
    assert np.count_nonzero(masks[0].any(0) & ~masks[0].all(0)) > 512   # run ends in more than two rounds of columns
    assert len(counts[0]) > 700


def test_far_more_runs_than_lanes():
    masks, counts = _check(_checkerboard(28), [[0, 0, 63, 63]], [[64, 64]])
    assert len(counts[0]) > 4 * 256


def test_long_counts_and_negative_differences():
    h, w = 1200, 1100
    masks, counts = _check(_maps(1, 14, 3), [[1080, 50, 1098, 1190]], [[h, w]])
    c = counts[0]
    assert c[0] >= 1 << 20 and len(rle.rle_to_string(c[:1])) == 5
    assert min(c[i] - c[i - 2] for i in range(3, len(c))) < 0


def test_masks_of_three_image_sizes_in_one_call():
    sizes = [[37, 53], [48, 64], [50, 50]]
    rs = np.random.RandomState(5)
    order = rs.permutation(12) % 3
    per_mask = [sizes[k] for k in order]
    xy = rs.rand(12, 2) * 30 - 5
    boxes = np.concatenate([xy, xy + 5 + rs.rand(12, 2) * 40], 1)
    masks, _ = _check(_maps(12, 14, 6), boxes, per_mask)
    assert len({k.shape for k in masks}) == 3 and all(k.any() for k in masks)


def test_two_calls_give_the_same_bytes():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    args = (torch.from_numpy(np.concatenate([_maps(5, 28, 8), _checkerboard(28)])).cuda(),
            torch.tensor([[3, 4, 50, 40], [-9, 2, 30, 70], [0, 0, 63, 47], [20, 20, 90, 90], [1, 1, 5, 5], [0, 0, 63, 47]],
                         dtype=torch.float32).cuda(), torch.tensor([[48, 64]] * 6, dtype=torch.int32).cuda())
    a, b = _C.pasted_masks_rle(*args), _C.pasted_masks_rle(*args)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[0].numel() > 0
    a, b = _C.pasted_masks_runs(*args), _C.pasted_masks_runs(*args)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_refusals():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    dev = torch.device("cuda")
    many = (torch.zeros(65536, 1, 1, device=dev), torch.zeros(65536, 4, device=dev), torch.ones(65536, 2, dtype=torch.int32, device=dev))
    probs, boxes = torch.zeros(2, 14, 14, device=dev), torch.zeros(2, 4, device=dev)
    sizes = torch.tensor([[4, 5], [6, 7]], dtype=torch.int32, device=dev)
    for fn in (_C.pasted_masks_runs, _C.pasted_masks_rle):
        with pytest.raises(RuntimeError, match="OVIS_ERANGE"):
            fn(*many)
        with pytest.raises(RuntimeError, match="OVIS_ERANGE"):
            fn(torch.zeros(1, 121, 121, device=dev), boxes[:1], sizes[:1])
        for bad in ([[4, 0], [6, 7]], [[4, 5], [-1, 7]], [[4, 5], [65536, 65536]]):
            with pytest.raises(RuntimeError, match="height >= 1"):
                fn(probs, boxes, torch.tensor(bad, dtype=torch.int32, device=dev))
        with pytest.raises(RuntimeError):
            fn(probs, boxes, sizes.long())
        with pytest.raises(RuntimeError):
            fn(probs, boxes[:1], sizes)
        with pytest.raises(RuntimeError):
            fn(probs[:, :, :7], boxes, sizes)
        with pytest.raises(RuntimeError):
            fn(probs, boxes, sizes.cpu())
