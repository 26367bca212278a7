"""GPU: the prediction compositor kernel (csrc/render.hip, ``_C.render_instances``) against the NumPy restatement of
tests/render_reference.py (held to the reference's own functions by tests/test_render_reference.py) -- byte for byte --
and, for fill layers, against a composition over the masks ``_C.paste_masks`` makes.  The shapes are the smallest at
which the kernel takes each of its paths: a 64 x 16 tile per workgroup (ragged at 17 x 33, several tiles at 130 x 259),
rows whose byte offset is no multiple of 4, 64 layers per list round."""
import functools

import numpy as np
import pytest
import torch

from tests import render_reference as R

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (17, 33), (61, 97), (130, 259)]   # (H, W): W * 3 is no multiple of 16 (nor of 4, but for 1 x 1's single pixel)


def _maps(k, m, seed):
    return np.random.RandomState(seed).rand(k, m, m).astype(np.float32)


def _edge_boxes(h, w):
    W, H = float(w), float(h)
    return np.float32([
        [W * 0.2, H * 0.3, W * 0.7, H * 0.8],          # inside
        [-200.0, -100.0, -50.0, -60.0],                # wholly outside
        [-20.5, H * 0.1, W * 0.4, H * 0.5],            # over the left border
        [W * 0.1, -15.2, W * 0.6, H * 0.3],            # ... the top
        [W - 20.0, H * 0.2, W + 25.3, H * 0.6],        # ... the right
        [W * 0.1, H - 30.0, W * 0.5, H + 17.7],        # ... the bottom
        [W * 0.45, H * 0.1, W * 0.45 + 0.4, H * 0.9],  # narrower than one pixel
        [-5.0, -5.0, W + 5.0, H + 5.0],                # everything
    ])


def _device(image, maps, boxes, colors, kinds=None, params=None, alpha=0.5, outline_colors=None, outline_thickness=2):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    d = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    params = params if params is None or np.isscalar(params) else d(np.float32(params))
    got = _C.render_instances(d(image), d(maps), d(boxes), d(colors), d(kinds), params, alpha, d(outline_colors), outline_thickness)
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == image.shape
    return got.cpu().numpy()


def _over_paste_masks(image, maps, boxes, colors, threshold=0.5, alpha=0.5):
    """The fills composed on the host over the [K, H, W] masks of the existing one-launch paste kernel."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    h, w = image.shape[:2]
    masks = _C.paste_masks(torch.from_numpy(maps).cuda(), torch.from_numpy(boxes).cuda(), (h, w), threshold).cpu().numpy()
    out = image.copy()
    for mask, color in zip(masks, colors):
        out = R.fill(out, mask, color, alpha)
    return out


@functools.lru_cache(maxsize=None)
def _edge_case(h, w):
    rs = np.random.RandomState(100 * h + w)
    boxes = _edge_boxes(h, w)
    k = len(boxes)
    return (rs.randint(0, 256, (h, w, 3)).astype(np.uint8), _maps(k, 14, h + w), boxes,
            rs.randint(0, 256, (k, 3)).astype(np.float32), rs.randint(0, 256, (k, 3)).astype(np.uint8))


@pytest.mark.parametrize("h,w", SIZES)
def test_fills_at_every_border_equal_the_restatement_and_the_pasted_masks(h, w):
    image, maps, boxes, colors, outline = _edge_case(h, w)
    want = R.render(image, maps, boxes, colors)
    got = _device(image, maps, boxes, colors)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(got, _over_paste_masks(image, maps, boxes, colors))
    assert (h, w) == (1, 1) or not np.array_equal(got, image)
    want = R.render(image, maps, boxes, colors, params=0.3, alpha=0.25)
    assert np.array_equal(_device(image, maps, boxes, colors, params=0.3, alpha=0.25), want)
    assert np.array_equal(want, _over_paste_masks(image, maps, boxes, colors, 0.3, 0.25))


@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("thickness", [1, 2, 3])
def test_outlines_touching_every_border(h, w, thickness):
    image, maps, boxes, colors, outline = _edge_case(h, w)
    boxes = boxes.copy()
    boxes[0] = [0.0, 0.0, w - 1.0, h - 1.0]            # the bands of all four edges are clipped by the image
    boxes[1] = [w * 0.6, h * 0.7, w * 0.3, h * 0.2]    # corners in the other order
    want = R.render(image, maps, boxes, colors, outline_colors=outline, outline_thickness=thickness)
    assert np.array_equal(_device(image, maps, boxes, colors, outline_colors=outline, outline_thickness=thickness), want)
    # the outlines alone (no pixel of a zero map passes its threshold)
    alone = _device(image, np.zeros_like(maps), boxes, colors, outline_colors=outline, outline_thickness=thickness)
    assert np.array_equal(alone, R.render(image, np.zeros_like(maps), boxes, colors, outline_colors=outline, outline_thickness=thickness))
    assert not np.array_equal(alone, image)


def test_no_layer_copies_the_image():
    image = _edge_case(61, 97)[0]
    got = _device(image, np.zeros((0, 14, 14), np.float32), np.zeros((0, 4), np.float32), np.zeros((0, 3), np.float32))
    assert np.array_equal(got, image)
    got = _device(image, np.zeros((0, 14, 14), np.float32), np.zeros((0, 4), np.float32), np.zeros((0, 3), np.float32),
                  outline_colors=np.zeros((0, 3), np.uint8))
    assert np.array_equal(got, image)


@pytest.mark.parametrize("m", [14, 28, 56])
def test_map_resolutions(m):
    image, _, boxes, colors, _ = _edge_case(61, 97)
    maps = _maps(len(boxes), m, m)
    got = _device(image, maps, boxes, colors)
    assert np.array_equal(got, R.render(image, maps, boxes, colors))
    assert np.array_equal(got, _over_paste_masks(image, maps, boxes, colors))
    kinds, params = np.ones(len(boxes), np.int32), np.linspace(0.2, 3.0, len(boxes)).astype(np.float32)
    assert np.array_equal(_device(image, maps, boxes, colors, kinds, params), R.render(image, maps, boxes, colors, kinds, params))


def test_probability_exactly_at_the_threshold_is_not_filled():
    """A box whose integer pasted box is 16 x 16 for M = 14: the resize has scale 1, every pixel reads one cell of the
    padded map with weight exactly 1, so the pasted value IS the planted float."""
    image = np.full((40, 50, 3), 200, np.uint8)
    box = np.float32([[8.4375, 8.4375, 21.5625, 21.5625]])
    assert R.pasted_rect(box[0], 14) == (7, 7, 22, 22, 16, 16)
    thr = np.float32(0.5)
    maps = np.full((1, 14, 14), np.nextafter(thr, np.float32(0)), np.float32)
    maps[0, 3, 4] = thr                                  # pixel (7 + 1 + 3, 7 + 1 + 4)
    maps[0, 5, 6] = np.nextafter(thr, np.float32(1))
    colors = np.float32([[0, 100, 50]])
    got = _device(image, maps, box, colors)
    assert np.array_equal(got, R.render(image, maps, box, colors))
    changed = np.argwhere((got != image).any(2)).tolist()
    assert changed == [[7 + 1 + 5, 7 + 1 + 6]] and got[13, 14].tolist() == [100, 150, 125]
    assert np.array_equal(got, _over_paste_masks(image, maps, box, colors))


def test_layer_order_matters_and_is_kept():
    image, maps, boxes, colors, _ = _edge_case(61, 97)
    pick = [0, 7, 5]                                     # three layers stacked on the lower middle of the image
    other = [5, 0, 7]
    a = _device(image, maps[pick], boxes[pick], colors[pick])
    b = _device(image, maps[other], boxes[other], colors[other])
    assert not np.array_equal(a, b)
    assert np.array_equal(a, R.render(image, maps[pick], boxes[pick], colors[pick]))
    assert np.array_equal(b, R.render(image, maps[other], boxes[other], colors[other]))
    assert np.array_equal(a, _over_paste_masks(image, maps[pick], boxes[pick], colors[pick]))


def test_130_layers_on_one_tile_take_three_list_rounds():
    """Every layer covers the whole 17 x 33 image (one ragged tile): the ordered list is built and worked off in rounds of 64.
    Fill and heat layers interleaved, as the combined view stacks them."""
    k, h, w = 130, 17, 33
    rs = np.random.RandomState(5)
    image = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    maps = _maps(k, 14, 9)
    boxes = np.float32([-3.0, -2.0, w + 2.0, h + 1.0]) + rs.uniform(-1, 1, (k, 4)).astype(np.float32)
    colors = rs.randint(0, 256, (k, 3)).astype(np.float32)
    kinds = np.tile(np.int32([0, 1]), k // 2)
    params = np.where(kinds == 0, 0.5, rs.uniform(0.1, 0.6, k)).astype(np.float32)
    got = _device(image, maps, boxes, colors, kinds, params)
    assert np.array_equal(got, R.render(image, maps, boxes, colors, kinds, params))
    fills = np.zeros(k, np.int32)
    got = _device(image, maps, boxes, colors, fills, 0.5)
    assert np.array_equal(got, R.render(image, maps, boxes, colors, fills, 0.5))
    assert np.array_equal(got, _over_paste_masks(image, maps, boxes, colors))
    # a sparse list: only every 50th layer meets the image, the rounds in between are empty
    far = boxes.copy()
    far[np.arange(k) % 50 != 7] += 1000.0
    assert np.array_equal(_device(image, maps, far, colors, kinds, params), R.render(image, maps, far, colors, kinds, params))


def test_blends_that_end_in_one_half_are_truncated():
    image = np.zeros((20, 30, 3), np.uint8)
    image[:, :] = [101, 101, 254]
    box = np.float32([[2.0, 2.0, 25.0, 15.0]])
    maps = np.ones((1, 14, 14), np.float32)
    colors = np.float32([[100, 50, 255]])                 # 100.5, 75.5, 254.5
    got = _device(image, maps, box, colors)
    assert got[8, 12].tolist() == [100, 75, 254] and np.array_equal(got, R.render(image, maps, box, colors))
    rs = np.random.RandomState(8)
    image = rs.randint(0, 256, (20, 30, 3)).astype(np.uint8)
    colors = (rs.randint(0, 1021, (1, 3)) / 4.0).astype(np.float32)   # quarter steps, as the reference's palette * 255 has
    assert np.array_equal(_device(image, maps, box, colors), R.render(image, maps, box, colors))


def test_heat_clipped_to_one_and_exactly_zero():
    rs = np.random.RandomState(4)
    image = rs.randint(0, 256, (30, 40, 3)).astype(np.uint8)
    boxes = np.float32([[2.0, 2.0, 18.0, 26.0], [20.0, 3.0, 38.0, 27.0], [5.0, 5.0, 35.0, 25.0]])
    maps = np.stack([np.ones((14, 14), np.float32), np.zeros((14, 14), np.float32), _maps(1, 14, 2)[0]])
    colors = np.float32([[0, 0, 255], [255, 0, 0], [10, 200, 30]])
    kinds = np.ones(3, np.int32)
    params = np.float32([5.0, 5.0, -1.0])                 # m = 1 inside; m = 0 (zero map); m = 0 (negative product clipped)
    got = _device(image, maps, boxes, colors, kinds, params)
    assert np.array_equal(got, R.render(image, maps, boxes, colors, kinds, params))
    assert got[14, 10].tolist() == [0, 0, 255] and np.array_equal(got[:, 20:], image[:, 20:])
    params = np.float32([0.4, 0.9, 2.0])
    maps[1] = _maps(1, 14, 3)[0]
    got = _device(image, maps, boxes, colors, kinds, params)
    assert np.array_equal(got, R.render(image, maps, boxes, colors, kinds, params)) and not np.array_equal(got, image)


def test_interleaved_fill_and_heat_sequence():
    image, maps, boxes, scores, _ = R.golden_inputs("combined")
    k = len(boxes)
    twice = np.repeat(np.arange(k), 2)
    rs = np.random.RandomState(6)
    colors = rs.randint(0, 256, (2 * k, 3)).astype(np.float32)
    colors[1::2] = [0, 0, 255]
    params = np.full(2 * k, 0.5, np.float32)
    params[1::2] = [np.float32(0.2 / s) for s in scores.tolist()]
    m2 = maps[twice].copy()
    m2[1::2] = _maps(k, 14, 12) * 0.8
    kinds = np.tile(np.int32([0, 1]), k)
    outline = rs.randint(0, 256, (2 * k, 3)).astype(np.uint8)
    got = _device(image, m2, boxes[twice], colors, kinds, params, outline_colors=outline)
    assert np.array_equal(got, R.render(image, m2, boxes[twice], colors, kinds, params, outline_colors=outline))


def _raw(image_ptr, h, w, maps, boxes_ptr, k, m, kinds, params, colors, out_ptr, alpha=0.5):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    rc = _C._L.ovis_render_instances_u8(image_ptr, h, w, maps.data_ptr(), boxes_ptr, k, m, kinds.data_ptr(), params.data_ptr(),
                                        colors.data_ptr(), alpha, 0, 2, out_ptr, _C._stream())
    torch.cuda.synchronize()
    return rc


def test_nothing_outside_the_image_is_written_at_any_alignment():
    """image and out at odd byte offsets inside larger buffers (the byte-wise path of every lane) and at aligned ones: the
    guard bytes around out keep their value."""
    h, w = 17, 33
    image, maps, boxes, colors, _ = _edge_case(h, w)
    k, n = len(boxes), h * w * 3
    want = R.render(image, maps, boxes, colors)
    d_maps, d_boxes, d_colors = (torch.from_numpy(a).cuda() for a in (maps, boxes, colors))
    kinds, params = torch.zeros(k, dtype=torch.int32, device="cuda"), torch.full((k,), 0.5, device="cuda")
    for in_off, out_off in ((0, 0), (13, 0), (0, 13), (3, 6), (16, 32)):
        src = torch.zeros(n + 64, dtype=torch.uint8, device="cuda")
        src[in_off:in_off + n] = torch.from_numpy(image).cuda().reshape(-1)
        dst = torch.full((n + 96,), 0xA5, dtype=torch.uint8, device="cuda")
        assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
        rc = _raw(src.data_ptr() + in_off, h, w, d_maps, d_boxes.data_ptr(), k, 14, kinds, params, d_colors, dst.data_ptr() + out_off)
        assert rc == 0
        dst = dst.cpu().numpy()
        assert np.array_equal(dst[out_off:out_off + n].reshape(h, w, 3), want), (in_off, out_off)
        assert (dst[:out_off] == 0xA5).all() and (dst[out_off + n:] == 0xA5).all(), (in_off, out_off)


def test_bad_arguments_raise():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C, _lib
    h, w = 17, 33
    image, maps, boxes, colors, outline = _edge_case(h, w)
    k = len(boxes)
    for bad in (dict(alpha=1.5), dict(alpha=float("nan")), dict(outline_colors=outline, outline_thickness=0),
                dict(outline_colors=outline, outline_thickness=256)):
        with pytest.raises(RuntimeError, match="OVIS_E"):
            _device(image, maps, boxes, colors, **bad)
    with pytest.raises(RuntimeError, match="OVIS_ERANGE"):
        _device(image, np.zeros((1, 121, 121), np.float32), boxes[:1], colors[:1])
    with pytest.raises(RuntimeError):   # host and device tensors mixed
        _C.render_instances(torch.from_numpy(image), torch.from_numpy(maps).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(colors).cuda())
    d_image, d_maps, d_colors = (torch.from_numpy(a).cuda() for a in (image, maps, colors))
    d_boxes = torch.zeros(4 * k + 4, device="cuda")
    kinds, params = torch.zeros(k, dtype=torch.int32, device="cuda"), torch.full((k,), 0.5, device="cuda")
    out = torch.empty_like(d_image)
    args = (d_maps, d_boxes.data_ptr(), k, 14, kinds, params, d_colors)
    assert _raw(d_image.data_ptr(), h, w, *args, out.data_ptr()) == 0
    with pytest.raises(RuntimeError, match="OVIS_EINVAL"):          # out aliases image
        _lib.check(_raw(d_image.data_ptr(), h, w, *args, d_image.data_ptr()), "render_instances")
    with pytest.raises(RuntimeError, match="OVIS_EINVAL"):          # ... or overlaps it
        _lib.check(_raw(d_image.data_ptr(), h, w // 2, *args, d_image.data_ptr() + 8), "render_instances")
    with pytest.raises(RuntimeError, match="OVIS_ERANGE"):          # boxes not 16-byte aligned
        _lib.check(_raw(d_image.data_ptr(), h, w, d_maps, d_boxes.data_ptr() + 4, k, 14, kinds, params, d_colors, out.data_ptr()),
                   "render_instances")
    with pytest.raises(RuntimeError, match="OVIS_ERANGE"):
        _lib.check(_raw(d_image.data_ptr(), 65536, 1, *args, out.data_ptr()), "render_instances")
    with pytest.raises(RuntimeError, match="OVIS_EINVAL"):
        _lib.check(_raw(d_image.data_ptr(), 0, w, *args, out.data_ptr()), "render_instances")
