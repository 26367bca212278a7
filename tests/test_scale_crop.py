"""CPU: scale jitter with a fixed-size crop above and below the kernels -- the draw rule of the host half against written-out
cases and a ``random.Random`` replay, off-means-off, the host twin of the window kernel against the NumPy restatement and
PIL, the targets' geometry against the reference's own crops (tests/golden/scale_crop.npz), and the command-line errors."""
import importlib.util
import os
import random

import numpy as np
import pytest
import torch

from tests import input_transform_ref as T
from tests import scale_crop_reference as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "scale_crop.npz")
FLIPS = [(False, False), (True, False), (False, True), (True, True)]


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"ovis_tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _transform(scale_jitter=None, crop_size=None, seed=0, flips=(0.5, 0.5), **kw):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import InputTransform

    return InputTransform((96, 112), 160, flips[0], flips[1], T.MEAN, T.STD_COCO, True, seed=seed, scale_jitter=scale_jitter,
                          crop_size=crop_size, **kw)


def _cfg(*extra):
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults

    cfg = get_defaults()
    cfg.merge_from_list(list(extra))
    return cfg


class Scripted:
    """A generator that hands out written-down values: ``uniform`` the scales, ``random`` the rest, in order."""

    def __init__(self, scales, randoms):
        self.scales, self.randoms, self.calls = list(scales), list(randoms), 0

    def uniform(self, lo, hi):
        s = self.scales.pop(0)
        assert lo <= s <= hi
        return s

    def random(self):
        self.calls += 1
        return self.randoms.pop(0)

    def choice(self, items):
        raise AssertionError("the size draw is replaced by the scale draw")


def _image(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


# ---- 1. the draw rule -------------------------------------------------------------------------------------------------------
# (in_h, in_w), canvas, s, (fy, fx) -> (out_h, out_w), (win_y, win_x, win_h, win_w), worked by hand:
#  a. s = 0.5 on 1024^2: r = min(512 / 480, 512 / 640) = 0.8 -> 384 x 512; both fit, the offsets are 0 whatever fy, fx
#  b. s = 2: r = min(2048 / 480, 2048 / 640) = 3.2 -> 1536 x 2048; win_y = round(0.5 * 512) = 256, win_x = round(0.25 * 1024)
#  c. 100 x 300 on 64 x 96 at 1.5: r = min(96 / 100, 144 / 300) = 0.48 -> 48 x 144; the height fits (win_y = 0, win_h = 48),
#     win_x = round(0.99 * 48) = round(47.52) = 48, win_w = min(96, 144 - 48) = 96
#  d. 1 x 1 at 0.001: r = 0.064, round(0.064) = 0 -> the floor: 1 x 1
#  e. 69 x 50 on 64 x 96 at 69 / 64: r = min(69 / 69, 103.5 / 50) = 1 -> 69 x 50; win_y = round(0.5 * 5) = round(2.5) = 2 (half to
#     even), win_h = 64; the width fits and is padded: win_w = 50
HAND = [((480, 640), (1024, 1024), 0.5, (0.9, 0.7), (384, 512), (0, 0, 384, 512)),
        ((480, 640), (1024, 1024), 2.0, (0.5, 0.25), (1536, 2048), (256, 256, 1024, 1024)),
        ((100, 300), (64, 96), 1.5, (0.3, 0.99), (48, 144), (0, 48, 48, 96)),
        ((1, 1), (64, 96), 0.001, (0.5, 0.5), (1, 1), (0, 0, 1, 1)),
        ((69, 50), (64, 96), 69 / 64, (0.5, 0.5), (69, 50), (2, 0, 64, 50))]


@pytest.mark.parametrize("case", HAND, ids="abcde")
def test_draw_rule_hand_computed(case):
    (h, w), canvas, s, (fy, fx), out_hw, window = case
    rng = Scripted([s], [0.9, 0.2, fy, fx])   # flips: 0.9 >= 0.5 no, 0.2 < 0.5 yes
    raw, _ = _transform((0.001, 2.0), canvas, size_divisible=32).host([_image(h, w)], rng=rng)
    assert raw["desc"].dtype == torch.int32 and tuple(raw["desc"].shape) == (1, 11)
    assert raw["desc"][0].tolist() == [0, h, w, *out_hw, 0, 1, *window]
    assert raw["image_sizes"] == [(window[2], window[3])]
    assert raw["pad_hw"] == tuple(-(-c // 32) * 32 for c in canvas) and raw["max_in_hw"] == (h, w)
    assert rng.calls == 4 and not rng.randoms
    assert sc.jittered_size(h, w, s, canvas) == out_hw and sc.window_of(fy, fx, out_hw, canvas) == window


def test_draw_rule_replayed_on_a_seeded_generator():
    """A seeded ``random.Random``: uniform for the scale IN PLACE OF the size choice, the two flips, then fy and fx -- for
    every image, whatever its size; no draw more, no draw less."""
    images = [_image(48, 64, 1), _image(61, 43, 2), _image(50, 50, 3), _image(1, 16, 4)]
    for seed in range(6):
        t = _transform((0.3, 2.5), (40, 56), flips=(0.5, 0.25))
        state = random.Random(seed)
        raw, _ = t.host(images, rng=state)
        r = random.Random(seed)
        for i, img in enumerate(images):
            oh, ow, fh, fv, window, drawn = sc.draws(r, img.shape[:2], (0.3, 2.5), (40, 56), (0.5, 0.25))
            assert drawn == 1 and raw["desc"][i].tolist()[1:] == [img.shape[0], img.shape[1], oh, ow, int(fh), int(fv), *window]
        assert state.getstate() == r.getstate()
        assert raw["pad_hw"] == (40, 56)


def _corner_target():
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList, PolygonMasks

    t = BoxList(torch.tensor([[28.0, 28.0, 31.0, 31.0]]), (32, 32))
    t.add_field("labels", torch.tensor([3]))
    t.add_field("masks", PolygonMasks([[[28, 28, 31, 28, 31, 31, 28, 31]]], (32, 32)))
    t.add_field("caption", "a corner")
    return t


def test_redraw_stops_at_the_first_surviving_box_and_after_eight():
    """32 x 32 at scale 2 of a 16 x 16 canvas stays 32 x 32; the only box sits in the bottom-right corner.  fy = fx = 0 shows
    the top-left quarter (no box left), 0.99 the bottom-right one."""
    t = _transform((2.0, 2.0), (16, 16), flips=(0.0, 0.0))
    rng = Scripted([2.0], [0.5, 0.5] + [0.0, 0.0] * 2 + [0.99, 0.99] + [0.0, 0.0])
    raw, targets = t.host([_image(32, 32)], [_corner_target()], rng=rng)
    assert raw["desc"][0].tolist() == [0, 32, 32, 32, 32, 0, 0, 16, 16, 16, 16]
    assert rng.calls == 2 + 2 * 3 and rng.randoms == [0.0, 0.0]          # the third window stands, nothing more is drawn
    assert targets[0].size == (16, 16) and targets[0].bbox.tolist() == [[12.0, 12.0, 15.0, 15.0]]
    assert targets[0].get_field("labels").tolist() == [3] and targets[0].get_field("caption") == "a corner"
    assert targets[0].get_field("masks").size == (16, 16)
    assert targets[0].get_field("masks").coords.tolist() == [12.0, 12.0, 15.0, 12.0, 15.0, 15.0, 12.0, 15.0]
    # nine windows without a box: the first and eight redraws; the ninth stands and the image arrives without targets
    rng = Scripted([2.0], [0.5, 0.5] + [0.0, 0.0] * 9 + [0.99, 0.99])
    raw, targets = t.host([_image(32, 32)], [_corner_target()], rng=rng)
    assert raw["desc"][0].tolist()[7:] == [0, 0, 16, 16] and rng.calls == 2 + 2 * 9 and rng.randoms == [0.99, 0.99]
    assert len(targets[0]) == 0 and targets[0].size == (16, 16) and len(targets[0].get_field("masks")) == 0
    # an image without a box, and a call without targets, draw one window
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList

    for tg in ([BoxList(torch.zeros((0, 4)), (32, 32))], None):
        rng = Scripted([2.0], [0.5, 0.5, 0.0, 0.0])
        t.host([_image(32, 32)], tg, rng=rng)
        assert rng.calls == 4
    # the restatement's loop agrees on both counts
    for misses, drawn in ((2, 3), (9, 9)):
        r = Scripted([2.0], [0.5, 0.5] + [0.0, 0.0] * misses + [0.99, 0.99] * 2)
        got = sc.draws(r, (32, 32), (2.0, 2.0), (16, 16), (0.0, 0.0),
                       survives=lambda out_hw, fh, fv, win: sc.crop_boxes([[28, 28, 31, 31]], win)[1].any())
        assert got[5] == drawn


# ---- 2. off means off -------------------------------------------------------------------------------------------------------
def test_without_the_switch_nothing_changes():
    from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import make_raw_batch
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import InputTransform, ViewTransform, build_transforms

    images, targets = make_raw_batch(3, seed=9, sizes=((48, 64), (61, 43), (50, 50)), num_gt=2)
    a, b = random.Random(11), random.Random(11)
    raw_new, t_new = _transform(None, None).host(images, targets, rng=a)
    plain = InputTransform((96, 112), 160, 0.5, 0.5, T.MEAN, T.STD_COCO, True)   # built without the new parameters
    raw_old, t_old = plain.host(images, targets, rng=b)
    assert tuple(raw_new["desc"].shape) == (3, 7) and sorted(raw_new) == ["data", "desc", "image_sizes", "max_in_hw", "pad_hw"]
    assert a.getstate() == b.getstate()
    assert torch.equal(raw_new["desc"], raw_old["desc"]) and raw_new["pad_hw"] == raw_old["pad_hw"]
    assert raw_new["image_sizes"] == raw_old["image_sizes"] and [t.size for t in t_new] == [t.size for t in t_old]
    assert torch.equal(_transform(None, None).device(raw_new).tensors, plain.device(raw_old).tensors)
    # evaluation transforms and the view transform never scale-jitter
    cfg = _cfg()
    t = build_transforms(cfg, is_train=True, scale_jitter=(0.5, 2.0), crop_size=(64, 96))
    assert t.scale_jitter == (0.5, 2.0) and t.crop_size == (64, 96)
    assert build_transforms(cfg, is_train=True, scale_jitter=(0.5, 2.0)).crop_size == (1024, 1024)
    assert build_transforms(cfg, is_train=True).scale_jitter is None
    assert build_transforms(cfg, is_train=False, scale_jitter=(0.5, 2.0), crop_size=(64, 96)).scale_jitter is None
    views = build_transforms(_cfg("TEST.BBOX_AUG.ENABLED", True), is_train=False, scale_jitter=(0.5, 2.0))
    assert type(views) is ViewTransform and tuple(views.host(images)[0]["desc"].shape[1:]) == (3, 7)
    with pytest.raises(ValueError, match="crop_size"):
        build_transforms(cfg, is_train=True, crop_size=(64, 96))
    with pytest.raises(ValueError, match="crop_size"):
        _transform(None, (64, 96))


# ---- 3. the host twin ---------------------------------------------------------------------------------------------------------
window_cases, INPUTS = sc.window_cases, sc.INPUTS


@pytest.fixture(scope="module")
def restated():
    """The restatement of every case, computed once and shared (tests/test_scale_crop_gpu.py computes its own copy)."""
    return [sc.window_transform(*case[:4], T.MEAN, T.STD_COCO, True, case[4]) for case in window_cases()]


def test_host_twin_equals_the_restatement(restated):
    from cvpr22_cross_modal_pseudo_labeling_amd import _cpu

    n = 0
    for case, want in zip(window_cases(), restated):
        data, desc = sc.pack(*case[:4])
        got = _cpu.transform_images_window(torch.from_numpy(data), torch.from_numpy(desc), T.MEAN, T.STD_COCO, True, case[4])
        assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32)), (desc.tolist(), case[4])
        n += 1
    assert n == len(INPUTS) * 5 * 5
    # RGB / 255 instead of BGR 0..255
    case = next(window_cases())
    data, desc = sc.pack(*case[:4])
    got = _cpu.transform_images_window(torch.from_numpy(data), torch.from_numpy(desc), (0.4, 0.5, 0.6), (0.2, 0.3, 0.25), False, case[4])
    want = sc.window_transform(*case[:4], (0.4, 0.5, 0.6), (0.2, 0.3, 0.25), False, case[4])
    assert np.array_equal(got.numpy().view(np.uint32), want.view(np.uint32))


def test_host_twin_equals_pil():
    """PIL itself: resize(BILINEAR), transpose, crop, then the normalisation."""
    try:
        from PIL import Image
    except ImportError:   # the restatement stands in (test_host_twin_equals_the_restatement)
        return
    from cvpr22_cross_modal_pseudo_labeling_amd import _cpu

    mean, std = np.asarray(T.MEAN, dtype=np.float32), np.asarray(T.STD_COCO, dtype=np.float32)
    for images, sizes, flips, wins, pad_hw in window_cases():
        data, desc = sc.pack(images, sizes, flips, wins)
        got = _cpu.transform_images_window(torch.from_numpy(data), torch.from_numpy(desc), T.MEAN, T.STD_COCO, True, pad_hw).numpy()
        for b, (img, (oh, ow), (fh, fv), (wy, wx, wh, ww)) in enumerate(zip(images, sizes, flips, wins)):
            pil = Image.fromarray(img, "RGB").resize((ow, oh), Image.BILINEAR)
            pil = pil.transpose(Image.FLIP_LEFT_RIGHT) if fh else pil
            pil = pil.transpose(Image.FLIP_TOP_BOTTOM) if fv else pil
            px = np.asarray(pil.crop((wx, wy, wx + ww, wy + wh)))
            want = ((px[:, :, ::-1].astype(np.float32) - mean) / std).transpose(2, 0, 1)
            assert np.array_equal(got[b, :, :wh, :ww], want), (desc[b].tolist(), pad_hw)
            assert not got[b, :, wh:].any() and not got[b, :, :, ww:].any()


def test_host_twin_refuses_what_the_device_turns_into_nan():
    from cvpr22_cross_modal_pseudo_labeling_amd import _cpu

    img = _image(5, 7)
    good = [0, 5, 7, 10, 14, 0, 0, 2, 3, 6, 8]
    for change, what in (({8: 7}, "past out_w"), ({7: 5}, "past out_h"), ({9: 0}, "empty"), ({7: -1}, "negative"),
                         ({0: 4}, "bytes past the buffer"), ({9: 9}, "taller than the canvas"), ({10: 13, 8: 0}, "wider than the canvas")):
        d = list(good)
        for k, v in change.items():
            d[k] = v
        with pytest.raises(RuntimeError, match="OVIS_EINVAL"):
            _cpu.transform_images_window(torch.from_numpy(img.reshape(-1)), torch.tensor([d], dtype=torch.int32), T.MEAN,
                                         T.STD_COCO, True, (8, 12))
    _cpu.transform_images_window(torch.from_numpy(img.reshape(-1)), torch.tensor([good], dtype=torch.int32), T.MEAN, T.STD_COCO,
                                 True, (8, 12))
    with pytest.raises(RuntimeError, match=r"\[B,11\]"):
        _cpu.transform_images_window(torch.from_numpy(img.reshape(-1)), torch.tensor([good[:7]], dtype=torch.int32), T.MEAN,
                                     T.STD_COCO, True, (8, 12))


def test_transform_end_to_end_on_host_tensors():
    """``InputTransform`` with scale jitter, both halves on the host: the canvas, the windows' sizes and the restatement's
    pixels; composed with the colour jitter the bytes are jittered first."""
    from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import make_raw_batch
    from tests import color_jitter_reference as J

    images, targets = make_raw_batch(3, seed=9, sizes=((48, 64), (61, 43), (50, 50)), num_gt=2)
    for jitter in (None, (0.4, 0.4, 0.4, 0.1)):
        t = _transform((0.5, 2.0), (64, 96), size_divisible=32, color_jitter=jitter)
        raw, out_targets = t.host(images, targets, rng=random.Random(21))
        got = t.device(raw)
        desc = raw["desc"].numpy()
        assert tuple(got.tensors.shape) == (3, 3, 64, 96) and got.image_sizes == [tuple(d[9:11]) for d in desc.tolist()]
        src = [np.asarray(i) for i in images]
        if jitter:
            src = [J.apply_chain(i, o, p) for i, o, p in zip(src, raw["jitter_ops"].numpy(), raw["jitter_params"].numpy())]
        want = sc.window_transform(src, [tuple(d[3:5]) for d in desc], [tuple(d[5:7]) for d in desc], [tuple(d[7:11]) for d in desc],
                                   T.MEAN, T.STD_COCO, True, (64, 96))
        assert np.array_equal(got.tensors.numpy().view(np.uint32), want.view(np.uint32))
        for tg, (h, w) in zip(out_targets, got.image_sizes):
            assert tg.size == (w, h) and tg.get_field("masks").size == (w, h) and len(tg.get_field("masks")) == len(tg)
            if len(tg):
                assert float(tg.bbox.min()) >= 0 and float(tg.bbox[:, 0::2].max()) <= w - 1 and float(tg.bbox[:, 1::2].max()) <= h - 1


# ---- 4. the targets' geometry against the reference's own crops ------------------------------------------------------------------
def test_target_geometry_equals_the_reference():
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList, PolygonMasks, RleMasks
    from tests import coco_rle_reference as rle_ref

    golden = np.load(GOLDEN)
    bitmaps = sc.golden_masks()
    for k, window in enumerate(sc.GOLDEN_WINDOWS):
        boxes = BoxList(torch.from_numpy(sc.GOLDEN_BOXES.copy()), sc.FRAME)
        boxes.add_field("index", torch.arange(len(sc.GOLDEN_BOXES)))
        boxes.add_field("caption", "carried")
        cropped = boxes.crop(window)
        assert np.array_equal(cropped.bbox.numpy(), golden[f"boxes_{k}"]) and tuple(cropped.size) == tuple(golden[f"box_size_{k}"])
        assert cropped.get_field("caption") == "carried" and torch.equal(cropped.get_field("index"), boxes.get_field("index"))
        assert torch.equal(boxes.bbox, torch.from_numpy(sc.GOLDEN_BOXES))   # a copy: the source is left as it is
        clipped = cropped.clip_to_image(remove_empty=True)
        assert clipped.get_field("index").tolist() == golden[f"kept_{k}"].tolist()
        assert np.array_equal(clipped.bbox.numpy(), golden[f"clipped_{k}"])
        assert 0 < len(clipped) < len(boxes)   # the one-pixel-wide box is empty in every window
        polys = PolygonMasks(sc.GOLDEN_POLYGONS, sc.FRAME).crop(window)
        assert tuple(polys.size) == tuple(golden[f"poly_size_{k}"]) and polys.coords.dtype == torch.float32
        for g, inst in enumerate(polys.instances()):
            for q, p in enumerate(inst):
                assert np.array_equal(p.numpy(), golden[f"poly_{k}_{g}_{q}"]), (k, g, q)
        # the recorded RLE window cuts the reference's pixels out of the dense canvas
        rle = RleMasks([rle_ref.rle_encode(m) for m in bitmaps], bitmaps.shape[1:]).crop(window)
        wx, wy, ww, wh = rle.window
        assert rle.size == (ww, wh) == tuple(golden[f"mask_size_{k}"]) and rle.frame_size == sc.FRAME
        assert (wx, wy, wx + ww, wy + wh) == sc.mask_window(window, *sc.FRAME)
        want = np.unpackbits(golden[f"mask_{k}"])[:3 * wh * ww].reshape(3, wh, ww).astype(bool)
        assert np.array_equal(bitmaps[:, wy:wy + wh, wx:wx + ww], want)
        for again in (lambda: rle.crop(window), lambda: rle.resize((20, 15)), lambda: rle.transpose(0), lambda: rle.transpose(1)):
            with pytest.raises(NotImplementedError, match="crop"):
                again()
    # the NumPy statement of crop + clip used by the draw-rule test is the same thing
    for k, (x0, y0, x1, y1) in enumerate(sc.GOLDEN_WINDOWS[:3]):
        b, keep = sc.crop_boxes(sc.GOLDEN_BOXES, (y0, x0, y1 - y0, x1 - x0))
        assert np.flatnonzero(keep).tolist() == golden[f"kept_{k}"].tolist() and np.array_equal(b[keep], golden[f"clipped_{k}"])


def test_fields_follow_through_their_own_crop_or_raise():
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList, PastedMasks

    t = BoxList(torch.tensor([[1.0, 1.0, 5.0, 5.0]]), (8, 8))
    t.add_field("masks", PastedMasks(torch.zeros(1, 4, 4), t.bbox, (8, 8)))
    with pytest.raises(NotImplementedError, match="has no crop"):
        t.crop((0, 0, 4, 4))
    t = BoxList(torch.tensor([[1.0, 1.0, 5.0, 5.0]]), (8, 8))
    t.add_field("masks", torch.zeros(1, 8, 8))
    with pytest.raises(NotImplementedError, match="dense mask tensor"):
        t.crop((0, 0, 4, 4))


# ---- 5. the command line ------------------------------------------------------------------------------------------------------
def test_train_net_flag_errors(capsys):
    train_net = _tool("train_net")
    for argv, text in ((["--scale-jitter", "0.5", "2.0"], "--scale-jitter"),
                       (["--raw-input", "--crop-size", "64", "96"], "--crop-size"),
                       (["--raw-input", "--scale-jitter", "0", "2.0"], "--scale-jitter"),
                       (["--raw-input", "--scale-jitter", "-0.5", "2.0"], "--scale-jitter"),
                       (["--raw-input", "--scale-jitter", "2.0", "1.0"], "--scale-jitter"),
                       (["--raw-input", "--scale-jitter", "0.5", "2.0", "--crop-size", "0", "96"], "--crop-size"),
                       (["--raw-input", "--scale-jitter", "0.5", "2.0", "--crop-size", "64", "-1"], "--crop-size"),
                       (["--raw-input", "--scale-jitter", "0.5", "2.0", "--crop-size", "8193", "64"], "--scale-jitter"),
                       (["--raw-input", "--scale-jitter", "0.5", "16.5"], "--scale-jitter")):
        with pytest.raises(SystemExit) as err:
            train_net.main(argv)
        message = capsys.readouterr().err
        assert err.value.code == 2 and text in message and "error:" in message, (argv, message)
    cfg = _cfg("MODEL.DEVICE", "cpu", "DATALOADER.NUM_WORKERS", 0)
    with pytest.raises(ValueError, match="scale_jitter"):
        train_net.make_data_source(cfg, 2, scale_jitter=(0.5, 2.0))
    with pytest.raises(ValueError, match="crop_size"):
        train_net.make_data_source(cfg, 2, raw_input=True, crop_size=(64, 96))
    # accepted: HI * side == 16384 exactly; the stream has the canvas' shape; composed with the colour jitter
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import check_scale_jitter

    assert check_scale_jitter((1, 16), (1024, 64)) == ((1.0, 16.0), (1024, 64))
    cfg = _cfg("MODEL.DEVICE", "cpu", "DATALOADER.NUM_WORKERS", 0, "INPUT.BRIGHTNESS", 0.3)
    loader, transform = train_net.make_data_source(cfg, 2, raw_input=True, color_jitter=True, scale_jitter=(0.1, 0.3), crop_size=(64, 96))
    raw, targets = next(iter(loader))
    assert tuple(raw["desc"].shape) == (2, 11) and "jitter_ops" in raw and tuple(raw["pad_hw"]) == (64, 96)
    assert tuple(transform.device(raw).tensors.shape) == (2, 3, 64, 96)
    assert [tuple(t.size) for t in targets] == [(w, h) for h, w in raw["image_sizes"]]
