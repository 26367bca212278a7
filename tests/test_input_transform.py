"""CPU: the input transform (raw uint8 images -> the padded float batch) against the reference's own results, all by exact
equality.  tests/golden/input_transform.npz holds PIL's bilinear resizes and the reference classes' box / polygon geometry
(make_input_transform_golden.py); tests/input_transform_ref.py is a scalar NumPy restatement of the whole transform.  The
restatement is pinned to the fixture (and to PIL itself where it is installed), the host twin (libovis_cpu.so) to the
restatement; tests/test_input_transform_gpu.py pins the device kernels to the host twin."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

from tests import input_transform_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "input_transform.npz"))


def test_restatement_equals_the_fixture_and_pil():
    for i, (_, _, oh, ow) in enumerate(R.CASES):
        img = R.case_input(i)
        assert R.crc(img) == int(GOLD["crc"][i]), f"seeded input {i} drifted"
        got = R.pil_resize(img, oh, ow)
        assert got.shape == GOLD[f"pil_{i}"].shape and np.array_equal(got, GOLD[f"pil_{i}"]), R.CASES[i]


def test_restatement_equals_installed_pil():
    Image = pytest.importorskip("PIL.Image")
    for i, (_, _, oh, ow) in enumerate(R.CASES):
        img = R.case_input(i)
        assert np.array_equal(R.pil_resize(img, oh, ow), np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR)))


def _host(images, sizes, flips, mean, std, bgr, pad):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    data, desc = R.pack(images, sizes, flips)
    out = _C.transform_images(torch.from_numpy(data), torch.from_numpy(desc), mean, std, bgr, pad)
    assert not out.is_cuda and out.dtype == torch.float32
    return out.numpy()


@pytest.mark.parametrize("index", range(len(R.CASES)))
def test_host_twin_equals_restatement(index):
    _, _, oh, ow = R.CASES[index]
    img = R.case_input(index)
    for flip_h, flip_v, bgr, std in itertools.product((0, 1), (0, 1), (True, False), ((1.0, 1.0, 1.0), R.STD_COCO)):
        mean = R.MEAN if bgr else (0.485, 0.456, 0.406)
        want = R.transform([img], [(oh, ow)], [(flip_h, flip_v)], mean, std, bgr, (oh, ow))
        got = _host([img], [(oh, ow)], [(flip_h, flip_v)], mean, std, bgr, (oh, ow))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (flip_h, flip_v, bgr, std)


@pytest.mark.parametrize("divisible", [0, 32])
def test_host_twin_batch_of_three_pads_with_zeros(divisible):
    idx = (0, 1, 3)  # 80 x 106, 43 x 27, 33 x 133
    images, sizes = [R.case_input(i) for i in idx], [R.CASES[i][2:] for i in idx]
    flips = [(0, 0), (1, 0), (0, 1)]
    pad_h, pad_w = max(s[0] for s in sizes), max(s[1] for s in sizes)
    if divisible:
        pad_h, pad_w = -(-pad_h // divisible) * divisible, -(-pad_w // divisible) * divisible
        assert (pad_h, pad_w) == (96, 160)
    want = R.transform(images, sizes, flips, R.MEAN, R.STD_COCO, True, (pad_h, pad_w))
    got = _host(images, sizes, flips, R.MEAN, R.STD_COCO, True, (pad_h, pad_w))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    for b, (oh, ow) in enumerate(sizes):   # +0.0 exactly, not -0.0
        assert not got[b, :, oh:, :].view(np.uint32).any() and not got[b, :, :, ow:].view(np.uint32).any()


def test_host_twin_refuses_a_descriptor_outside_its_buffers():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    data = torch.zeros(5 * 4 * 3, dtype=torch.uint8)
    for bad in ([0, 5, 5, 4, 4, 0, 0], [0, 5, 4, 9, 4, 0, 0], [4, 5, 4, 4, 4, 0, 0], [0, 0, 4, 4, 4, 0, 0]):
        with pytest.raises(RuntimeError):
            _C.transform_images(data, torch.tensor([bad], dtype=torch.int32), R.MEAN, (1, 1, 1), True, (8, 8))


def test_get_size():
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import get_size

    assert get_size(640, 480, 800, 1333) == (800, 1066)
    assert get_size(640, 427, 800, 1333) == (800, 1199)
    assert get_size(500, 200, 800, 1333) == (533, 1332)   # the max-size branch: size = round(1333 * 200 / 500) = 533
    assert get_size(1066, 800, 800, 1333) == (800, 1066)  # already at the size: returned as it is


def _geometry(name):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        import make_input_transform_golden as G
    finally:
        sys.path.pop(0)
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList, PolygonMasks

    k = sorted(G.SIZE_CASES).index(name)
    size, new_size = G.SIZE_CASES[name]
    boxes, polys = G.geometry_inputs(size, 77 + k)
    t = BoxList(boxes, size)
    t.add_field("masks", PolygonMasks(polys, size))
    t.add_field("labels", torch.arange(5))
    t.add_field("is_det", "Yes")
    return t, new_size


@pytest.mark.parametrize("name", ["equal", "per_axis"])
def test_box_and_polygon_geometry_equals_the_reference(name):
    t, new_size = _geometry(name)
    ratios = [float(a) / float(b) for a, b in zip(new_size, t.size)]
    assert (ratios[0] == ratios[1]) == (name == "equal")
    r = t.resize(new_size)
    assert r.size == new_size and r.get_field("masks").size == new_size
    assert torch.equal(r.get_field("labels"), torch.arange(5)) and r.get_field("is_det") == "Yes"
    assert np.array_equal(r.bbox.numpy(), GOLD[f"box_{name}_resize"])
    assert np.array_equal(r.get_field("masks").coords.numpy(), GOLD[f"poly_{name}_resize"])
    for method in (0, 1):
        f = r.transpose(method)
        assert np.array_equal(f.bbox.numpy(), GOLD[f"box_{name}_flip{method}"])
        assert np.array_equal(f.get_field("masks").coords.numpy(), GOLD[f"poly_{name}_flip{method}"])
    with pytest.raises(NotImplementedError):
        r.transpose(2)


def test_fields_that_cannot_follow_raise():
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList

    t = BoxList(torch.tensor([[1.0, 2.0, 8.0, 9.0]]), (20, 10))
    t.add_field("masks", torch.zeros(1, 10, 20, dtype=torch.bool))   # dense masks are tied to the old pixel grid
    with pytest.raises(NotImplementedError):
        t.resize((40, 20))
    with pytest.raises(NotImplementedError):
        t.transpose(0)
    u = BoxList(torch.tensor([[1.0, 2.0, 8.0, 9.0]]), (20, 10))
    u.add_field("thing", object())
    with pytest.raises(NotImplementedError):
        u.resize((40, 20))


@pytest.mark.parametrize("method", [0, 1])
def test_flipped_polygon_mask_is_the_flipped_mask(method):
    """Rasterising the transposed polygons gives the transposed raster -- for polygons the two conventions agree on.  The
    reference flips coordinates about (W - 1) / 2 (``W - x - 1``, segmentation_mask.py:265-268) while its rasteriser
    (pycocotools: vertices scaled by 5 and rounded half up, a column k taken at 5 k + 2) treats pixel k as [k, k + 1): a
    vertical edge at x = a + 0.5 has columns >= a + 1 on its right both before and after the flip, an edge at an integer x
    moves by one pixel, and a sloped edge is redrawn.  So the statement is exact for axis-aligned polygons with
    half-integer vertices, which is what is asserted; one instance is made of two polygons."""
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import PolygonMasks

    polys = [[[3.5, 2.5, 20.5, 2.5, 20.5, 15.5, 3.5, 15.5]],
             [[1.5, 1.5, 9.5, 1.5, 9.5, 6.5, 1.5, 6.5], [12.5, 8.5, 28.5, 8.5, 28.5, 17.5, 12.5, 17.5]]]
    m = PolygonMasks(polys, (31, 19))
    plain = m.convert_to_binarymask()
    assert plain.shape == (2, 19, 31) and plain.any()
    flipped = m.transpose(method).convert_to_binarymask()
    assert torch.equal(flipped, plain.flip(2 if method == 0 else 1))


def test_config_keys_and_jitter():
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms

    cfg = get_defaults()
    assert cfg.INPUT.HORIZONTAL_FLIP_PROB_TRAIN == 0.5 and cfg.INPUT.VERTICAL_FLIP_PROB_TRAIN == 0.0
    assert (cfg.INPUT.BRIGHTNESS, cfg.INPUT.CONTRAST, cfg.INPUT.SATURATION, cfg.INPUT.HUE) == (0.0, 0.0, 0.0, 0.0)
    cfg.merge_from_list(["INPUT.HORIZONTAL_FLIP_PROB_TRAIN", 0.25, "INPUT.VERTICAL_FLIP_PROB_TRAIN", 0.5,
                         "DATALOADER.SIZE_DIVISIBILITY", 32])
    t = build_transforms(cfg, is_train=True)
    assert (t.flip_horizontal_prob, t.flip_vertical_prob, t.size_divisible) == (0.25, 0.5, 32)
    e = build_transforms(cfg, is_train=False)
    assert (e.flip_horizontal_prob, e.flip_vertical_prob) == (0.0, 0.0) and e.min_size == (cfg.INPUT.MIN_SIZE_TEST,)
    for key in ("BRIGHTNESS", "CONTRAST", "SATURATION", "HUE"):
        c = get_defaults()
        c.merge_from_list([f"INPUT.{key}", 0.1])
        with pytest.raises(NotImplementedError):
            build_transforms(c, is_train=True)
        build_transforms(c, is_train=False)   # build.py:15-23: no jitter at test time


def test_host_half_draws_like_the_reference_and_moves_the_targets():
    """The host half over the raw synthetic stream: sizes by get_size, the reference's draw order (size, hflip, vflip per
    image), targets resized then flipped, and the device half (here on host tensors) equal to the restatement."""
    import random

    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import make_raw_batch
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms, get_size

    cfg = get_defaults()
    cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", (96, 112), "INPUT.MAX_SIZE_TRAIN", 160, "INPUT.VERTICAL_FLIP_PROB_TRAIN", 0.5,
                         "DATALOADER.SIZE_DIVISIBILITY", 32])
    t = build_transforms(cfg, is_train=True)
    images, targets = make_raw_batch(3, seed=5, sizes=((48, 64), (61, 43), (50, 50)), num_gt=2)
    raw, moved = t.host(images, targets, rng=random.Random(4))  # seed 4 draws both sizes and every flip combination but none
    rng, sizes, flips = random.Random(4), [], []
    for img in images:
        sizes.append(get_size(img.shape[1], img.shape[0], rng.choice((96, 112)), 160))
        flips.append((rng.random() < 0.5, rng.random() < 0.5))
    assert raw["image_sizes"] == sizes and raw["desc"][:, 5:].tolist() == [[int(a), int(b)] for a, b in flips]
    assert any(a for a, _ in flips) and any(b for _, b in flips)
    assert raw["pad_hw"][0] % 32 == 0 and raw["pad_hw"][1] % 32 == 0
    for tgt, got, (oh, ow), (fh, fv) in zip(targets, moved, sizes, flips):
        want = tgt.resize((ow, oh))
        want = want.transpose(0) if fh else want
        want = want.transpose(1) if fv else want
        assert got.size == (ow, oh) and torch.equal(got.bbox, want.bbox)
        assert torch.equal(got.get_field("masks").coords, want.get_field("masks").coords)
    out = t.device(raw)
    want = R.transform([i.numpy() for i in images], sizes, flips, cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, cfg.INPUT.TO_BGR255,
                       raw["pad_hw"])
    assert out.image_sizes == sizes and np.array_equal(out.tensors.numpy().view(np.uint32), want.view(np.uint32))


def test_evaluation_stream_uses_the_test_sizes_and_never_flips():
    """``raw_test_batches`` under ``build_transforms(cfg, is_train=False)``: INPUT.MIN_SIZE_TEST / MAX_SIZE_TEST decide the
    sizes, the flip probabilities of the training keys are ignored, batches of ``ims_per_batch`` with a short last one."""
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import make_raw_batch, raw_test_batches
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms, get_size

    cfg = get_defaults()
    cfg.merge_from_list(["INPUT.MIN_SIZE_TEST", 96, "INPUT.MAX_SIZE_TEST", 120, "INPUT.MIN_SIZE_TRAIN", (48,),
                         "INPUT.HORIZONTAL_FLIP_PROB_TRAIN", 1.0, "INPUT.VERTICAL_FLIP_PROB_TRAIN", 1.0])
    t = build_transforms(cfg, is_train=False)
    batches = list(raw_test_batches(t, range(3), 2, "cpu"))
    assert [ids for _, _, ids in batches] == [[0, 1], [2]] and all(tg is None for _, tg, _ in batches)
    shapes = set()
    for images, _, ids in batches:
        raws = [make_raw_batch(1, seed=5000 + i)[0][0].numpy() for i in ids]
        sizes = [get_size(r.shape[1], r.shape[0], 96, 120) for r in raws]
        shapes.update(r.shape[:2] for r in raws)
        assert images.image_sizes == sizes and all(max(s) <= 120 for s in sizes)
        pad = (max(s[0] for s in sizes), max(s[1] for s in sizes))
        want = R.transform(raws, sizes, [(0, 0)] * len(raws), cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, cfg.INPUT.TO_BGR255, pad)
        assert np.array_equal(images.tensors.numpy().view(np.uint32), want.view(np.uint32))
    assert len(shapes) >= 2   # images of different raw sizes went through


def test_host_twin_answers_an_oversize_dimension_like_the_device():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms  # noqa: F401

    data, desc = torch.zeros(4 * 4 * 3, dtype=torch.uint8), torch.tensor([[0, 4, 4, 4, 4, 0, 0]], dtype=torch.int32)
    for pad in ((4, 16385), (16385, 4)):
        with pytest.raises(RuntimeError, match="OVIS_ERANGE"):
            _C.transform_images(data, desc, R.MEAN, (1, 1, 1), True, pad)
    with pytest.raises(RuntimeError, match="OVIS_ERANGE"):   # an image dimension, named before its bytes are looked for
        _C.transform_images(data, torch.tensor([[0, 16385, 4, 4, 4, 0, 0]], dtype=torch.int32), R.MEAN, (1, 1, 1), True, (4, 4))


def test_host_half_refuses_an_empty_batch():
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import InputTransform

    with pytest.raises(ValueError, match="empty batch"):
        InputTransform((800,), 1333, 0.5, 0.0, R.MEAN, (1, 1, 1), True).host([])
