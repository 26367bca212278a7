"""CPU: test-time augmentation (TEST.BBOX_AUG) -- the keys, the view plan made from one packing of the bytes, the views'
pixels, the host route of the view merge against a hand-computed case and against a fixture made by the reference's own
classes, and identity-only augmentation against plain inference."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import input_transform_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "bbox_aug.npz")


def _cfg(opts=()):
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults

    cfg = get_defaults()
    cfg.merge_from_list(list(opts))
    cfg.freeze()
    return cfg


AUG = ["TEST.BBOX_AUG.ENABLED", "True", "TEST.BBOX_AUG.H_FLIP", "True", "TEST.BBOX_AUG.SCALES", "(48, 96)",
       "TEST.BBOX_AUG.MAX_SIZE", "160", "TEST.BBOX_AUG.SCALE_H_FLIP", "True", "INPUT.MIN_SIZE_TEST", "64",
       "INPUT.MAX_SIZE_TEST", "90", "DATALOADER.SIZE_DIVISIBILITY", "32"]


# ---- keys ------------------------------------------------------------------------------------------------------------------------
def test_keys_defaults_and_override_list():
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.detector import check_supported

    aug = _cfg().TEST.BBOX_AUG
    assert dict(aug) == {"ENABLED": False, "H_FLIP": False, "SCALES": (), "MAX_SIZE": 4000, "SCALE_H_FLIP": False}
    cfg = _cfg(AUG)
    aug = cfg.TEST.BBOX_AUG
    assert (aug.ENABLED, aug.H_FLIP, aug.SCALES, aug.MAX_SIZE, aug.SCALE_H_FLIP) == (True, True, (48, 96), 160, True)
    check_supported(cfg)
    with pytest.raises(NotImplementedError, match="GT_BOX_EVAL"):
        check_supported(_cfg(AUG + ["MODEL.GT_BOX_EVAL", "True"]))
    check_supported(_cfg(["MODEL.GT_BOX_EVAL", "True"]))   # each alone is served


# ---- views ------------------------------------------------------------------------------------------------------------------------
def _raw_images():
    rs = np.random.RandomState(77)
    return [rs.randint(0, 256, (37, 53, 3)).astype(np.uint8), rs.randint(0, 256, (64, 41, 3)).astype(np.uint8)]


def test_view_plan_from_one_packing():
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import InputTransform, ViewTransform, build_transforms, get_size

    assert isinstance(build_transforms(_cfg(), is_train=False), InputTransform)        # off: today's transform
    assert isinstance(build_transforms(_cfg(AUG), is_train=True), InputTransform)      # training is never augmented here
    t = build_transforms(_cfg(AUG), is_train=False)
    assert isinstance(t, ViewTransform)
    want = [(64, 90, False), (64, 90, True), (48, 160, False), (48, 160, True), (96, 160, False), (96, 160, True)]
    assert t.plan == want                                                               # bbox_aug.py:26-51, in its order
    images = _raw_images()
    raw, targets = t.host(images)
    assert targets is None
    assert raw["data"].dtype == torch.uint8 and raw["data"].numel() == sum(i.size for i in images)   # packed ONCE
    assert torch.equal(raw["data"], torch.cat([torch.from_numpy(i).reshape(-1) for i in images]))
    desc = raw["desc"]
    assert desc.dtype == torch.int32 and tuple(desc.shape) == (6, 2, 7)
    assert raw["max_in_hw"] == (64, 53)
    for v, (min_size, max_size, flip) in enumerate(want):
        sizes = [get_size(53, 37, min_size, max_size), get_size(41, 64, min_size, max_size)]
        assert desc[v, :, 0].tolist() == [0, 37 * 53 * 3]                               # the same byte offsets in every view
        assert desc[v, :, 1:3].tolist() == [[37, 53], [64, 41]]
        assert desc[v, :, 3:5].tolist() == [list(s) for s in sizes]
        assert desc[v, :, 5].tolist() == [int(flip)] * 2 and desc[v, :, 6].tolist() == [0, 0]   # forced, never vertical
        assert [tuple(s) for s in raw["image_sizes"][v]] == sizes
        pad_h, pad_w = max(s[0] for s in sizes), max(s[1] for s in sizes)
        assert raw["pad_hw"][v] == (-(-pad_h // 32) * 32, -(-pad_w // 32) * 32)        # SIZE_DIVISIBILITY per view
    assert len({raw["pad_hw"][v] for v in range(6)}) > 1                                # ... and the views do differ
    with pytest.raises(ValueError):
        t.host(images, targets=[None, None])


def test_view_pixels_equal_single_calls_and_pil():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import ViewBatch, build_transforms

    cfg = _cfg(AUG)
    t = build_transforms(cfg, is_train=False)
    images = _raw_images()
    raw, _ = t.host(images)
    batch = t.device(raw)
    assert isinstance(batch, ViewBatch) and len(batch) == 6 and batch.flips == [False, True, False, True, False, True]
    assert isinstance(batch.to("cpu"), ViewBatch)
    mean, std = cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD
    for v, view in enumerate(batch.views):
        pad_hw = raw["pad_hw"][v]
        assert tuple(view.tensors.shape) == (2, 3) + pad_hw and view.tensors.dtype == torch.float32
        assert view.image_sizes == [tuple(s) for s in raw["image_sizes"][v]]
        for i, img in enumerate(images):
            oh, ow = raw["image_sizes"][v][i]
            single = torch.tensor([[0, img.shape[0], img.shape[1], oh, ow, int(batch.flips[v]), 0]], dtype=torch.int32)
            one = _C.transform_images(torch.from_numpy(img).reshape(-1), single, mean, std, cfg.INPUT.TO_BGR255, pad_hw)
            assert torch.equal(view.tensors[i], one[0]), (v, i)
    # one mirrored view against PIL itself: Resize -> RandomHorizontalFlip(1.0), then the reference's normalisation
    v = 3
    for i, img in enumerate(images):
        oh, ow = raw["image_sizes"][v][i]
        pil = np.asarray(Image.fromarray(img).resize((ow, oh), Image.BILINEAR).transpose(Image.FLIP_LEFT_RIGHT))
        want = R.transform([pil], [(oh, ow)], [(False, False)], mean, std, cfg.INPUT.TO_BGR255, raw["pad_hw"][v])
        assert np.array_equal(batch.views[v].tensors[i].numpy(), want[0]), i


# ---- the host route of the merge --------------------------------------------------------------------------------------------------
def _post(score_thresh=0.05, nms=0.5, per_img=100):
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.roi_heads import PostProcessor

    pp = PostProcessor(_cfg())
    pp.score_thresh, pp.nms, pp.detections_per_img = score_thresh, nms, per_img
    return pp


def test_host_merge_hand_computed():
    """Two views of one 40 x 30 image, 3 classes, threshold 0.5: view 1 is 20 x 10 and mirrored (ratios 2 and 3)."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    nan = float("nan")
    z = [0.0, 0.0, 1.0, 1.0]
    boxes = torch.tensor([
        # view 0                class 1               class 2
        [z, [4.0, 6, 20, 18], [1.0, 1, 5, 5]],       # class 2 scores exactly the threshold: dropped
        [z, [24.0, 10, 36, 28], [3.0, 3, 9, 9]],     # class 2 scores NaN: dropped
        [z, [0.0, 0, 2, 2], [10.0, 10, 30, 25]],
        # view 1 (mirrored, 20 wide): x -> (20 - x) - 1, then x * 2, y * 3
        [z, [9.0, 2, 17, 6], [0.0, 0, 1, 1]],        # class 1 maps onto view 0's first box, same score: NMS keeps view 0's
        [z, [0.0, 0, 1, 1], [4.0, 3, 14, 8]],        # class 2 -> [10, 9, 30, 24]: suppresses view 0's 0.6
    ])
    scores = torch.tensor([[0.0, 0.9, 0.5], [0.1, 0.8, nan], [0.1, 0.7, 0.6], [0.0, 0.9, 0.2], [0.0, 0.1, 0.95]])
    segments = [(0, 3, 0, 40, 0, 1.0, 1.0), (3, 2, 0, 20, 1, 40.0 / 20.0, 30.0 / 10.0)]
    cand_boxes, cand_scores, cand_group, offsets = _C.merge_view_detections(boxes, scores, segments, 3, 0.5)
    assert cand_group.dtype == torch.int32 and offsets.dtype == torch.int32
    assert offsets.tolist() == [0, 0, 4, 6]
    assert cand_group.tolist() == [1, 1, 1, 1, 2, 2]
    assert cand_scores.tolist() == [0.9, 0.8, 0.7, 0.9, 0.6, 0.95] or torch.equal(
        cand_scores, torch.tensor([0.9, 0.8, 0.7, 0.9, 0.6, 0.95]))
    assert cand_boxes.tolist() == [[4, 6, 20, 18], [24, 10, 36, 28], [0, 0, 2, 2], [4, 6, 20, 18], [10, 10, 30, 25],
                                   [10, 9, 30, 24]]
    pp = _post(0.5, 0.5, 100)
    (all_kept,) = pp.filter_merged((cand_boxes, cand_scores, cand_group, offsets), [(40, 30)], 3)
    assert all_kept.get_field("labels").tolist() == [1, 1, 1, 2] and all_kept.get_field("labels").dtype == torch.int64
    assert all_kept.bbox.tolist() == [[4, 6, 20, 18], [24, 10, 36, 28], [0, 0, 2, 2], [10, 9, 30, 24]]
    pp.detections_per_img = 2          # more survivors than DETECTIONS_PER_IMG: the two best, in list order
    (best,) = pp.filter_merged((cand_boxes, cand_scores, cand_group, offsets), [(40, 30)], 3)
    assert best.size == (40, 30)
    assert best.bbox.tolist() == [[4, 6, 20, 18], [10, 9, 30, 24]]
    assert torch.equal(best.get_field("scores"), torch.tensor([0.9, 0.95])) and best.get_field("labels").tolist() == [1, 2]
    # nothing above the threshold: empty outputs keep dtypes and shapes
    none = _C.merge_view_detections(boxes, scores, segments, 3, 2.0)
    assert tuple(none[0].shape) == (0, 4) and tuple(none[1].shape) == (0,) and none[2].dtype == torch.int32
    assert none[3].tolist() == [0, 0, 0, 0]
    (empty,) = pp.filter_merged(none, [(40, 30)], 3)
    assert tuple(empty.bbox.shape) == (0, 4) and empty.get_field("scores").dtype == torch.float32
    assert empty.get_field("labels").dtype == torch.int64 and len(empty) == 0


def test_host_merge_argument_errors():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    boxes, scores = torch.zeros(4, 3, 4), torch.zeros(4, 3)
    with pytest.raises(RuntimeError, match="rows"):
        _C.merge_view_detections(boxes, scores, [(2, 3, 0, 10, 0, 1.0, 1.0)], 3, 0.5)
    with pytest.raises(RuntimeError, match="images"):
        _C.merge_view_detections(boxes, scores, [(0, 2, 1, 10, 0, 1.0, 1.0)], 3, 0.5)
    with pytest.raises(RuntimeError, match="expected"):
        _C.merge_view_detections(boxes, scores, [(0, 2, 0, 10, 0, 1.0, 1.0)], 4, 0.5)
    with pytest.raises(RuntimeError, match="expected"):
        _C.merge_view_detections(boxes.reshape(4, 12), scores, [(0, 2, 0, 10, 0, 1.0, 1.0)], 3, 0.5)


def test_host_route_reproduces_the_reference_fixture():
    """tests/golden/bbox_aug.npz: BoxList.transpose / resize, the concatenation and PostProcessor.filter_results of the
    reference itself (tests/golden/make_bbox_aug_golden.py)."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    z = np.load(GOLDEN)
    c = int(z["num_classes"])
    sizes, flips = z["view_sizes"].tolist(), z["view_flips"].tolist()
    boxes = torch.cat([torch.from_numpy(z[f"boxes_{v}"]).reshape(-1, c, 4) for v in range(len(sizes))], 0)
    scores = torch.cat([torch.from_numpy(z[f"scores_{v}"]) for v in range(len(sizes))], 0)
    rows = z["boxes_0"].shape[0]
    (tw, th) = sizes[0]
    assert float(tw) / sizes[2][0] != float(th) / sizes[2][1]          # a ratio per axis
    segments = [(v * rows, rows, 0, w, int(flip), float(tw) / float(w), float(th) / float(h))
                for v, ((w, h), flip) in enumerate(zip(sizes, flips))]
    merged = _C.merge_view_detections(boxes, scores, segments, c, float(z["score_thresh"]))
    # the candidates are the reference's concatenated list, thresholded class by class
    ref_boxes = torch.from_numpy(z["merged_boxes"]).reshape(-1, c, 4)
    ref_scores = torch.from_numpy(z["merged_scores"]).reshape(-1, c)
    want_b, want_s = [], []
    for j in range(1, c):
        idx = (ref_scores[:, j] > float(z["score_thresh"])).nonzero().squeeze(1)
        want_b.append(ref_boxes[idx, j])
        want_s.append(ref_scores[idx, j])
    assert torch.equal(merged[0], torch.cat(want_b)) and torch.equal(merged[1], torch.cat(want_s))
    pp = _post(float(z["score_thresh"]), float(z["nms"]), int(z["detections_per_img"]))
    (got,) = pp.filter_merged(merged, [tuple(sizes[0])], c)
    assert len(got) == int(z["detections_per_img"])                    # the cut was taken
    assert torch.equal(got.bbox, torch.from_numpy(z["out_boxes"]))
    assert torch.equal(got.get_field("scores"), torch.from_numpy(z["out_scores"]))
    assert torch.equal(got.get_field("labels"), torch.from_numpy(z["out_labels"]))


# ---- the whole path on host tensors --------------------------------------------------------------------------------------------
def test_identity_only_augmentation_is_plain_inference():
    """ENABLED with no flip and no scales: a single view merged with itself is ordinary inference, bit for bit."""
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import ViewBatch
    from cvpr22_cross_modal_pseudo_labeling_amd.engine.bbox_aug import im_detect_bbox_aug
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import to_image_list
    from tests.tiny_model import build_tiny

    model, _, e_seen, images, _ = build_tiny("student_teacher_mask_rcnn_uncertainty")
    model.set_class_embeddings(e_seen)
    model.eval()
    with torch.no_grad():
        want = model(images)
    got = im_detect_bbox_aug(model, ViewBatch([to_image_list(images)], [False]))
    assert len(got) == len(want) == 2 and sum(len(w) for w in want) > 0
    for g, w in zip(got, want):
        assert g.size == w.size and torch.equal(g.bbox, w.bbox)
        assert sorted(g.fields()) == sorted(w.fields()) and "mask" in g.fields()
        for f in w.fields():
            assert g.get_field(f).dtype == w.get_field(f).dtype and torch.equal(g.get_field(f), w.get_field(f)), f
    with pytest.raises(RuntimeError, match="eval"):
        model.train()
        model.detect_unfiltered(images)


def test_ready_made_images_are_refused_under_augmentation():
    """A stream of already-transformed images (tools/test_net.py's) cannot be augmented: the key is never silently ignored."""
    from types import SimpleNamespace

    from cvpr22_cross_modal_pseudo_labeling_amd.engine.inference import compute_on_dataset

    class Detector(torch.nn.Module):
        def __init__(self, cfg):
            super().__init__()
            self.roi_heads = SimpleNamespace(cfg=cfg)

        def forward(self, images, targets=None):
            return []

    batches = [(torch.zeros(1, 3, 8, 8), None, [])]
    assert compute_on_dataset(Detector(_cfg()), batches, "cpu") == {}
    with pytest.raises(ValueError, match="infer_net.py"):
        compute_on_dataset(Detector(_cfg(AUG)), batches, "cpu")
