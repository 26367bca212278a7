"""GPU: scale jitter with a fixed-size crop on the device.  ``_C.transform_images_window`` must equal, bit for bit, the same
window sliced out of ``_C.transform_images`` at the full resized size, and the host twin; ``_C.project_rle_masks`` through a
recorded window must equal the dense, literally sliced restatement (tests/scale_crop_reference.py); polygon targets behind
``PolygonMasks.crop`` must equal the host rasteriser's; and a training step of the tiny model runs from a jittered loader
batch, with polygon and with RLE ground truth, twice to the same bits."""
import copy

import numpy as np
import pytest
import torch

from tests import coco_rle_reference as rle_ref
from tests import input_transform_ref as T
from tests import rle_targets_reference as rt
from tests import scale_crop_reference as sc
from tests import tiny_coco, tiny_rle_coco

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _device_window(images, sizes, flips, wins, pad_hw, mean=T.MEAN, std=T.STD_COCO, to_bgr255=True):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    data, desc = sc.pack(images, sizes, flips, wins)
    max_in = (max(i.shape[0] for i in images), max(i.shape[1] for i in images))
    return _C.transform_images_window(torch.from_numpy(data).to(DEV), torch.from_numpy(desc).to(DEV), mean, std, to_bgr255, pad_hw, max_in)


def _sliced_from_the_full_transform(images, sizes, flips, wins, pad_hw, mean=T.MEAN, std=T.STD_COCO, to_bgr255=True):
    """Per image ``_C.transform_images`` on the device at exactly its full resized size, the window sliced out of it."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    out = torch.zeros((len(images), 3) + tuple(pad_hw), dtype=torch.float32, device=DEV)
    for b, (img, size, flip, (wy, wx, wh, ww)) in enumerate(zip(images, sizes, flips, wins)):
        data, desc = T.pack([img], [size], [flip])
        full = _C.transform_images(torch.from_numpy(data).to(DEV), torch.from_numpy(desc).to(DEV), mean, std, to_bgr255, size,
                                   img.shape[:2])
        out[b, :, :wh, :ww] = full[0, :, wy:wy + wh, wx:wx + ww]
    return out


def _host_twin(images, sizes, flips, wins, pad_hw, mean=T.MEAN, std=T.STD_COCO, to_bgr255=True):
    from cvpr22_cross_modal_pseudo_labeling_amd import _cpu

    data, desc = sc.pack(images, sizes, flips, wins)
    return _cpu.transform_images_window(torch.from_numpy(data), torch.from_numpy(desc), mean, std, to_bgr255, pad_hw)


# ---- 1. the window kernel ---------------------------------------------------------------------------------------------------
def test_window_kernel_over_the_grid():
    """The grid of tests/test_scale_crop.py: four inputs x five resizes (both skipped-pass paths) x four flips x four
    windows, padded and exact canvases."""
    n = 0
    for case in sc.window_cases():
        got = _device_window(*case)
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(case[0]), 3) + tuple(case[4])
        assert torch.equal(got, _sliced_from_the_full_transform(*case)), (case[1][0], case[2][0], case[3])
        assert np.array_equal(_bits(got), _bits(_host_twin(*case))), (case[1][0], case[2][0], case[3])
        n += 1
    assert n == 100


def test_window_kernel_on_a_mixed_batch_and_two_x_blocks():
    # three images of different sizes, flips and windows on one canvas; RGB / 255 normalisation
    images = [sc.image(33, 47, 1), sc.image(20, 31, 2), sc.image(64, 9, 3)]
    sizes, flips = [(76, 108), (9, 31), (64, 40)], [(True, False), (False, True), (True, True)]
    wins = [(11, 23, 40, 50), (0, 3, 9, 28), (24, 0, 40, 40)]
    for to_bgr255, mean, std in ((True, T.MEAN, T.STD_COCO), (False, (0.4, 0.5, 0.6), (0.2, 0.3, 0.25))):
        got = _device_window(images, sizes, flips, wins, (48, 64), mean, std, to_bgr255)
        assert torch.equal(got, _sliced_from_the_full_transform(images, sizes, flips, wins, (48, 64), mean, std, to_bgr255))
        assert np.array_equal(_bits(got), _bits(_host_twin(images, sizes, flips, wins, (48, 64), mean, std, to_bgr255)))
        want = sc.window_transform(images, sizes, flips, wins, mean, std, to_bgr255, (48, 64))
        assert np.array_equal(_bits(got), want.view(np.uint32))
    # pad_w = 300: two x-blocks of 256 lanes; 30 x 40 -> 360 x 480, of which a 200 x 300 window is made
    img = [sc.image(30, 40, 4)] * 2
    case = (img, [(360, 480)] * 2, [(True, True), (False, False)], [(77, 131, 200, 300), (160, 180, 200, 300)], (200, 300))
    got = _device_window(*case)
    assert torch.equal(got, _sliced_from_the_full_transform(*case))
    assert np.array_equal(_bits(got), _bits(_host_twin(*case)))


def test_an_invalid_descriptor_is_nan_and_its_neighbours_are_untouched():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    images = [sc.image(33, 47, 1), sc.image(20, 31, 2), sc.image(16, 9, 3)]
    sizes, flips = [(76, 108), (30, 31), (16, 40)], [(True, False), (False, True), (True, True)]
    wins = [(11, 23, 40, 50), (5, 3, 20, 28), (0, 8, 16, 32)]
    data, desc = sc.pack(images, sizes, flips, wins)
    data_dev, max_in = torch.from_numpy(data).to(DEV), (33, 47)

    def run(d):
        return _C.transform_images_window(data_dev, torch.from_numpy(np.ascontiguousarray(d)).to(DEV), T.MEAN, T.STD_COCO, True,
                                          (48, 64), max_in)

    good = run(desc)
    assert not torch.isnan(good).any()
    without = run(desc[[0, 2]])   # the same byte buffer, the middle image left out
    assert torch.equal(without, good[[0, 2]])
    for column, value in ((8, 31 - 28 + 1), (0, data.size - 3 * 20 * 31 + 1), (7, 30 - 20 + 1), (9, 49), (4, 16385)):
        bad = desc.copy()
        bad[1, column] = value   # a window past out_w; bytes past the buffer; a window past out_h; taller than the canvas; out_w > 16384
        got = run(bad)
        assert torch.isnan(got[1]).all(), (column, value)
        assert torch.equal(got[[0, 2]], without), (column, value)
    with pytest.raises(RuntimeError, match=r"\[B,11\]"):
        _C.transform_images_window(data_dev, torch.from_numpy(desc[:, :7].copy()).to(DEV), T.MEAN, T.STD_COCO, True, (48, 64), max_in)


def test_transform_device_half_equals_the_host_half_with_and_without_colour_jitter():
    """``InputTransform.device`` on device tensors against the same call on host tensors (pinned to the restatement by
    tests/test_scale_crop.py); with the colour jitter the 11-column descriptors feed ``_C.color_jitter`` their first seven."""
    import random

    from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import make_raw_batch
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import InputTransform

    images, targets = make_raw_batch(3, seed=9, sizes=((48, 64), (61, 43), (50, 50)), num_gt=2)
    for jitter in (None, (0.4, 0.4, 0.4, 0.1)):
        t = InputTransform((96, 112), 160, 0.5, 0.5, T.MEAN, T.STD_COCO, True, size_divisible=32, color_jitter=jitter,
                           scale_jitter=(0.5, 2.0), crop_size=(64, 96))
        raw, _ = t.host(images, targets, rng=random.Random(21))
        host = t.device(raw)
        dev = t.device({k: v.to(DEV) if torch.is_tensor(v) else v for k, v in raw.items()})
        assert dev.tensors.is_cuda and tuple(dev.tensors.shape) == (3, 3, 64, 96) and dev.image_sizes == host.image_sizes
        assert np.array_equal(_bits(dev.tensors), _bits(host.tensors))


# ---- 2. RLE targets through a window ------------------------------------------------------------------------------------------
G = 3
# (h0, w0) -> the resized frames (h1, w1): up and down
RLE_SHAPES = [((9, 13), [(20, 27), (7, 9)]), ((40, 64), [(100, 75), (21, 40)])]


def _rle_masks(bitmaps):
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import RleMasks

    items = [rle_ref.rle_to_string(rle_ref.rle_encode(m)).decode("ascii") if k % 2 == 0 else rle_ref.rle_encode(m)
             for k, m in enumerate(bitmaps)]
    return RleMasks(items, bitmaps.shape[1:])


def _rle_windows(h1, w1):
    """(win_y, win_x, win_h, win_w): interior at ODD offsets, flush with the far edges, the whole frame."""
    wh, ww = max(2, (2 * h1) // 3 - 1), max(2, (2 * w1) // 3 - 1)
    return [(1, 3 if w1 - ww > 3 else 1, wh, ww), (h1 - wh, w1 - ww, wh, ww), (0, 0, h1, w1)]


def _window_boxes(ww, wh, seed):
    """Boxes in the window's frame: the edge boxes and random ones of the un-windowed test, and boxes on .5 -- half to even
    sends 0.5 -> 0, 2.5 -> 2, 4.5 -> 4, so behind an odd offset rounding first and offsetting first disagree."""
    halves = np.asarray([[0.5, 0.5, 4.5, 2.5], [2.5, 0.5, ww - 1.5, wh - 1.5], [0.5, 2.5, 6.5, 4.5]], dtype=np.float32)
    return np.concatenate([halves, rt.edge_boxes(ww, wh), rt.random_boxes(8, ww, wh, seed)])


@pytest.fixture(scope="module")
def rle_sources():
    """{(h0, w0): (bool [G, h0, w0] bitmaps, their RleMasks decoded on the device)} -- decoded once."""
    out = {}
    for s, ((h0, w0), _) in enumerate(RLE_SHAPES):
        bitmaps = rt.salt_and_pepper(G, h0, w0, 60 + s)
        out[(h0, w0)] = (bitmaps, _rle_masks(bitmaps).to(DEV).decoded())
    return out


@pytest.mark.parametrize("M", [14, 28])
@pytest.mark.parametrize("shape", RLE_SHAPES, ids=["9x13", "40x64"])
def test_rle_targets_through_a_window(rle_sources, shape, M):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    (h0, w0), frames = shape
    bitmaps, decoded = rle_sources[(h0, w0)]
    some = 0
    for h1, w1 in frames:
        for flip_h, flip_v in rt.FLIPS:
            m = decoded.resize((w1, h1))
            m = m.transpose(0) if flip_h else m
            m = m.transpose(1) if flip_v else m
            for k, (wy, wx, wh, ww) in enumerate(_rle_windows(h1, w1)):
                boxes = _window_boxes(ww, wh, 7 + k)
                if k == 0:   # the case is what it claims to be: an odd offset behind a .5
                    assert wx % 2 == 1 and wy % 2 == 1
                    assert (np.rint(boxes[:3]) + np.float32(wx) != np.rint(boxes[:3] + np.float32(wx))).any()
                gt_index = np.arange(len(boxes)) % G
                cropped = m.crop((wx, wy, wx + ww, wy + wh))
                assert cropped.window == (wx, wy, ww, wh) and cropped.size == (ww, wh) and cropped.words is m.words
                boxes_dev, index_dev = torch.from_numpy(boxes).to(DEV), torch.from_numpy(gt_index).to(DEV)
                got = _C.project_rle_masks(cropped, index_dev, boxes_dev, M)
                want = sc.project_window(bitmaps, gt_index, boxes, (h1, w1), flip_h, flip_v, (wy, wx, wh, ww), M)
                assert got.shape == (len(boxes), M, M) and got.dtype == torch.float32
                differ = got.cpu().numpy() != want
                assert not differ.any(), ((h1, w1), flip_h, flip_v, (wy, wx, wh, ww), int(differ.sum()), np.argwhere(differ)[:5].tolist())
                some += int(want.any())
                if k == 2:   # the whole frame: the un-windowed entry, bit for bit
                    assert torch.equal(got, _C.project_rle_masks(m, index_dev, boxes_dev, M))
                # through the structure's own route, on an indexed subset
                sub = cropped[torch.tensor([True, False, True], device=DEV)]
                got = sub.project(torch.from_numpy(gt_index % 2).to(DEV), boxes_dev, M)
                want = sc.project_window(bitmaps[[0, 2]], gt_index % 2, boxes, (h1, w1), flip_h, flip_v, (wy, wx, wh, ww), M)
                assert np.array_equal(got.cpu().numpy(), want)
    assert some >= 12
    with pytest.raises(NotImplementedError, match="MODEL.DEVICE cpu"):
        cropped.project(torch.zeros(1, dtype=torch.int64), torch.zeros(1, 4), M)


def test_a_window_outside_the_frame_is_refused(rle_sources):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    _, decoded = rle_sources[(9, 13)]
    m = decoded.resize((27, 20)).crop((3, 1, 20, 15))
    boxes, index = torch.tensor([[0.0, 0.0, 5.0, 5.0]], device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)
    _C.project_rle_masks(m, index, boxes, 14)
    for window in ((3, 1, 25, 14), (3, 1, 17, 20), (-1, 1, 17, 14), (3, 1, 0, 14)):   # (win_x, win_y, win_w, win_h)
        with pytest.raises(RuntimeError):
            _C.project_rle_masks(m._with(window=window), index, boxes, 14)


# ---- 3. polygon targets behind the crop ---------------------------------------------------------------------------------------
def test_polygon_targets_behind_the_crop():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C, _cpu
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import PolygonMasks

    polys = PolygonMasks(sc.GOLDEN_POLYGONS, sc.FRAME)
    some = 0
    for size in ((100, 75), (27, 20)):
        for flip_h, flip_v in rt.FLIPS:
            m = polys.resize(size)
            m = m.transpose(0) if flip_h else m
            m = m.transpose(1) if flip_v else m
            for wy, wx, wh, ww in _rle_windows(size[1], size[0]):
                c = m.crop((wx, wy, wx + ww, wy + wh))
                assert c.size == (ww, wh)
                boxes = _window_boxes(ww, wh, 3)
                index = torch.from_numpy(np.arange(len(boxes)) % 3)
                for M in (14, 28):
                    want = _cpu.project_polygon_masks(c.coords, c.polygon_start, c.instance_start, index, torch.from_numpy(boxes), c.size, M)
                    got = c.project(index.to(DEV), torch.from_numpy(boxes).to(DEV), M)
                    assert got.is_cuda and torch.equal(got.cpu(), want), (size, flip_h, flip_v, (wy, wx, wh, ww), M)
                    some += int(want.any())
                # whole-image masks on the cropped canvas: the two rasterisers agree there too
                assert torch.equal(c.to(DEV).convert_to_binarymask().cpu(), c.convert_to_binarymask())
    assert some >= 24


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    paths = tiny_coco.write(tmp_path_factory.mktemp("tiny_scale_crop"))
    paths["instances_bitmap"] = tiny_rle_coco.write(paths)
    return paths


@pytest.fixture(scope="module")
def tiny():
    from tests.tiny_model import build_tiny

    model, e_vocab, _, _, _ = build_tiny("student_teacher_mask_rcnn_uncertainty")
    return model, e_vocab


@pytest.mark.parametrize("kind", ["polygons", "rle"])
def test_one_training_step_on_a_jittered_batch(paths, tiny, kind):
    """Loader -> prefetcher -> the windowed device transform -> one step of the tiny student-teacher model, with the sizes of
    tests/test_dataset_reader_gpu.py: a [B, 3, 64, 96] batch, every box inside its image, finite losses, and the same loss
    bits from a second run with the same seed."""
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import make_data_loader
    from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCOCapDetDataset
    from cvpr22_cross_modal_pseudo_labeling_amd.data.prefetch import DevicePrefetcher
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import comm, solver, trainer
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import PolygonMasks, RleMasks

    cfg = tiny_coco.small_cfg()
    dataset = COCOCapDetDataset(paths["instances_bitmap" if kind == "rle" else "instances"], paths["captions"], paths["img_dir"], True,
                                extra_args=cfg.DATASETS.DATASET_ARGS, vocab_file=paths["vocab"])
    model, e_vocab = tiny

    def run():
        transform = build_transforms(cfg, is_train=True, scale_jitter=(0.5, 2.0), crop_size=(64, 96))
        loader = make_data_loader(cfg, dataset, transform, True, 0, 1, num_workers=0, seed=6, max_iter=1)
        stream = DevicePrefetcher(loader, DEV, depth=2, transform=transform)
        try:
            ((images, targets),) = list(stream)
        finally:
            stream.close()
        net = copy.deepcopy(model).cuda()
        net.set_class_embeddings(dataset.class_emb_mtx.cuda())
        net.set_caption_vocab(e_vocab.cuda())
        net.train()
        opt = solver.make_optimizer(cfg, net)
        red = comm.BucketedGradReducer(net)
        torch.manual_seed(100)
        losses = {k: float(v.detach()) for k, v in trainer.train_step(net, opt, red, images, targets).items()}
        red.remove()
        return images, targets, losses

    images, targets, losses = run()
    assert tuple(images.tensors.shape) == (2, 3, 64, 96) and images.tensors.is_cuda and not torch.isnan(images.tensors).any()
    kinds = set()
    for b, (t, (h, w)) in enumerate(zip(targets, images.image_sizes)):
        assert t.size == (w, h) and h <= 64 and w <= 96 and len(t) >= 1
        assert float(t.bbox.min()) >= 0 and float(t.bbox[:, 0::2].max()) <= w - 1 and float(t.bbox[:, 1::2].max()) <= h - 1
        masks = t.get_field("masks")
        assert len(masks) == len(t) and tuple(masks.size) == (w, h) and isinstance(t.get_field("caption"), str)
        kinds.add(type(masks))
        if isinstance(masks, RleMasks):
            assert masks.window is not None and masks.words is not None
        assert not images.tensors[b, :, h:].any() and not images.tensors[b, :, :, w:].any()   # zero outside the window
    assert (RleMasks in kinds) if kind == "rle" else kinds == {PolygonMasks}
    print(f"losses on the jittered {kind} batch:", losses)
    assert "loss_mask" in losses and all(v == v and abs(v) < 1e6 for v in losses.values()), losses
    _, _, again = run()
    assert again == losses, (losses, again)
