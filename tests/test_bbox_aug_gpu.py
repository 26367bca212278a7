"""GPU: the view-merge kernels against the host (BoxList) route, ``PostProcessor.filter_merged`` on the device against the
host loop, and test-time augmentation end to end on the tiny model and the tiny COCO dataset."""
import importlib.util
import math
import os

import pytest
import torch

from tests import tiny_coco

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs", "coco_cap_det", "student_teacher_mask_rcnn_uncertainty.yaml")
THRESH = 0.7

# name -> (rows per segment, image of every segment, classes, what is planted)
CASES = {
    "one_segment_c2": ([65], [0], 2, "random"),
    "two_views_c49": ([63, 64], [0, 0], 49, "random"),
    "two_images_six_segments_c66": ([257, 0, 65, 1, 64, 63], [0, 0, 0, 1, 1, 1], 66, "random"),
    "one_view_per_image_c130": ([64, 257], [0, 1], 130, "random"),
    "six_views_empty_in_the_middle_c49": ([1, 63, 0, 65, 257, 64], [0] * 6, 49, "random"),
    "lvis_vocabulary_c1204": ([65, 65], [0, 0], 1204, "random"),
    "none_above": ([257, 65, 64], [0, 0, 1], 66, "none"),
    "all_above": ([65, 64, 1], [0, 1, 1], 49, "all"),
    "seventy_images_two_launches": ([3] * 70, list(range(70)), 5, "random"),
}


def _case(name):
    rows, images, c, mode = CASES[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    r = sum(rows)
    scores = torch.rand(r, c, generator=g)
    if mode == "none":
        scores = scores * THRESH * 0.99
    elif mode == "all":
        scores = scores * 0.2 + 0.75
    else:  # the edges of the comparison, wherever a row exists
        scores[0, c - 1] = THRESH            # equal to the threshold: dropped
        scores[r - 1, 1] = float("nan")      # NaN: dropped
        scores[r // 2, 1] = float("inf")     # kept
    segments, row = [], 0
    for k, (n, image) in enumerate(zip(rows, images)):
        width = 101 + 2 * k                   # odd
        first = images.index(image) == k
        flip = k % 2 == 1 or (k == 0 and len(rows) == 1)
        ratio_w, ratio_h = (1.0, 1.0) if first or k % 3 == 1 else (101.0 / float(width), 67.0 / float(40 + k))
        segments.append((row, n, image, width, int(flip), ratio_w, ratio_h))
        row += n
    xy = torch.rand(r, c, 2, generator=g) * 60
    boxes = torch.cat([xy, xy + torch.rand(r, c, 2, generator=g) * 40], 2)
    return boxes, scores, segments, c, mode


_HOST = {}


def _host(name):
    """The host route's outputs of a case, computed once."""
    if name not in _HOST:
        from cvpr22_cross_modal_pseudo_labeling_amd import _C

        boxes, scores, segments, c, _ = _case(name)
        _HOST[name] = _C.merge_view_detections(boxes, scores, segments, c, THRESH)
    return _HOST[name]


def test_cases_admit_more_than_one_order():
    """CPU-side check of the inputs: every non-degenerate case has candidates in several classes and several segments, flips
    on and off, a ratio of exactly 1.0 and unequal ratios."""
    for name, (rows, images, c, mode) in CASES.items():
        boxes, scores, segments, c, mode = _case(name)
        cand_boxes, cand_scores, cand_group, offsets = _host(name)
        assert offsets.numel() == (max(images) + 1) * c + 1 and int(offsets[-1]) == cand_boxes.shape[0]
        if mode == "none":
            assert cand_boxes.shape[0] == 0
            continue
        with_candidates = sum(bool((scores[s[0]:s[0] + s[1], 1:] > THRESH).any()) for s in segments)
        assert with_candidates > 1 or len(rows) == 1, name
        assert (cand_group % c).unique().numel() > 1 or c == 2, name
        if mode == "all":
            assert cand_boxes.shape[0] == sum(rows) * (c - 1)
        else:
            assert 0 < cand_boxes.shape[0] < sum(rows) * (c - 1)
            assert not torch.isnan(cand_scores).any() and torch.isinf(cand_scores).any() and (cand_scores > THRESH).all()
    flips = {s[4] for n in CASES for s in _case(n)[2]}
    ratios = {(s[5] == 1.0, s[5] == s[6]) for n in CASES for s in _case(n)[2]}
    assert flips == {0, 1} and (True, True) in ratios and (False, False) in ratios


@pytest.mark.parametrize("name", list(CASES))
def test_merge_kernel_equals_host_route(name):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    boxes, scores, segments, c, _ = _case(name)
    got = _C.merge_view_detections(boxes.cuda(), scores.cuda(), segments, c, THRESH)
    want = _host(name)
    for g, w, what in zip(got, want, ("cand_boxes", "cand_scores", "cand_group", "offsets")):
        assert g.is_cuda and g.dtype == w.dtype and g.shape == w.shape, what
        assert torch.equal(g.cpu(), w), what
    again = _C.merge_view_detections(boxes.cuda(), scores.cuda(), segments, c, THRESH)   # placement is a function of the inputs
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_merge_wrapper_errors():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    boxes, scores = torch.zeros(8, 3, 4), torch.zeros(8, 3)
    seg = [(0, 8, 0, 11, 0, 1.0, 1.0)]
    with pytest.raises(RuntimeError, match="mixed"):
        _C.merge_view_detections(boxes.cuda(), scores, seg, 3, 0.5)
    with pytest.raises(RuntimeError, match="mixed"):
        _C.merge_view_detections(boxes, scores.cuda(), seg, 3, 0.5)
    with pytest.raises(RuntimeError, match="expected"):
        _C.merge_view_detections(boxes.cuda().reshape(8, 12), scores.cuda(), seg, 3, 0.5)
    with pytest.raises(RuntimeError, match="expected"):
        _C.merge_view_detections(boxes.cuda(), scores.cuda().reshape(12, 2), seg, 3, 0.5)
    with pytest.raises(RuntimeError, match="expected"):
        _C.merge_view_detections(boxes.cuda().double(), scores.cuda(), seg, 3, 0.5)
    with pytest.raises(RuntimeError, match="rows"):   # refused on the host, before any launch
        _C.merge_view_detections(boxes.cuda(), scores.cuda(), [(4, 5, 0, 11, 0, 1.0, 1.0)], 3, 0.5)
    with pytest.raises(RuntimeError, match="rows"):
        _C.merge_view_detections(boxes.cuda(), scores.cuda(), [(-1, 2, 0, 11, 0, 1.0, 1.0)], 3, 0.5)
    with pytest.raises(RuntimeError, match="images"):
        _C.merge_view_detections(boxes.cuda(), scores.cuda(), [(0, 4, 0, 11, 0, 1.0, 1.0), (4, 4, 2, 11, 0, 1.0, 1.0)], 3, 0.5)
    with pytest.raises(RuntimeError, match="views"):
        _C.merge_view_detections(boxes.cuda(), scores.cuda(), [(0, 0, 0, 11, 0, 1.0, 1.0)] * 65, 3, 0.5)
    # the library itself refuses records outside the tensors as well
    import ctypes
    ints = (ctypes.c_int32 * 5)(4, 5, 0, 11, 0)
    ratios = (ctypes.c_float * 2)(1.0, 1.0)
    counts = torch.zeros(3, dtype=torch.int32, device="cuda")
    assert _C._L.ovis_view_merge_count_f32(scores.cuda().data_ptr(), 8, 3, 1, ints, ratios, 1, 0.5, counts.data_ptr(), 3, None) == -1


# ---- filtering ------------------------------------------------------------------------------------------------------------------
def _post(per_img=100):
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.roi_heads import PostProcessor

    pp = PostProcessor(get_defaults())
    pp.detections_per_img = per_img
    return pp


def _same_detections(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.size == w.size and g.bbox.shape == w.bbox.shape and torch.equal(g.bbox.cpu(), w.bbox)
        assert torch.equal(g.get_field("scores").cpu(), w.get_field("scores"))
        assert g.get_field("labels").dtype == torch.int64 and torch.equal(g.get_field("labels").cpu(), w.get_field("labels"))


def _merged_views(scale, seed, n=120, nc=49, views=3, images=2):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    g = torch.Generator().manual_seed(seed)
    r = n * views * images
    xy = torch.rand(r, nc, 2, generator=g) * 300
    boxes = torch.cat([xy, xy + torch.rand(r, nc, 2, generator=g) * 150 + 10], 2)
    scores = torch.softmax(torch.randn(r, nc, generator=g) * scale, 1)
    segments = [(k * n, n, k // views, 501, k % 2, 1.0 if k % views == 0 else 0.75, 1.0 if k % views == 0 else 1.25)
                for k in range(views * images)]
    return _C.merge_view_detections(boxes, scores, segments, nc, 0.05), nc, [(501, 375)] * images


@pytest.mark.parametrize("scale,per_img", [(0.0, 100), (3.0, 100), (3.0, 7)])   # nothing above the threshold / many / over the cap
def test_filter_merged_device_equals_host(scale, per_img):
    merged, nc, sizes = _merged_views(scale, 5)
    pp = _post(per_img)
    want = pp.filter_merged(merged, sizes, nc)
    got = pp.filter_merged(tuple(t.cuda() for t in merged), sizes, nc)
    assert all(g.bbox.is_cuda for g in got)
    _same_detections(got, want)
    assert (scale == 0.0) == (sum(len(w) for w in want) == 0)
    if per_img == 7:
        assert all(len(w) >= 7 for w in want)
    if scale == 0.0:   # empty results keep dtypes and shapes
        assert all(tuple(g.bbox.shape) == (0, 4) and g.get_field("scores").dtype == torch.float32 for g in got)


def test_filter_merged_split_at_class_boundaries():
    merged, nc, sizes = _merged_views(3.0, 6)
    dev = tuple(t.cuda() for t in merged)
    k, runs = merged[0].shape[0], (merged[3][1:] - merged[3][:-1])
    limit = max(300, int(runs.max()))
    assert k > 3 * limit and int(runs.max()) <= limit           # several slices, every run fits
    pp = _post()
    whole = pp.filter_merged(dev, sizes, nc)
    split = pp.filter_merged(dev, sizes, nc, max_candidates=limit)
    _same_detections(split, [w.to("cpu") for w in whole])
    _same_detections(split, pp.filter_merged(merged, sizes, nc))
    # a slice TARGET below the largest run never raises: that run gets a slice of its own
    _same_detections(pp.filter_merged(dev, sizes, nc, slice_candidates=10), [w.to("cpu") for w in whole])
    _same_detections(pp.filter_merged(dev, sizes, nc, slice_candidates=10 * k), [w.to("cpu") for w in whole])
    run = int(runs.argmax())
    with pytest.raises(RuntimeError, match=f"class {run % nc} of image {run // nc} has {int(runs.max())} candidates"):
        pp.filter_merged(dev, sizes, nc, max_candidates=int(runs.max()) - 1)


# ---- the whole path -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    from tests.tiny_model import build_tiny

    model, _, e_seen, images, _ = build_tiny("student_teacher_mask_rcnn_uncertainty")
    model = model.cuda()
    model.set_class_embeddings(e_seen.cuda())
    model.eval()
    return model, images


def _same_boxlists(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.size == w.size and torch.equal(g.bbox, w.bbox) and sorted(g.fields()) == sorted(w.fields())
        for f in w.fields():
            assert g.get_field(f).dtype == w.get_field(f).dtype and torch.equal(g.get_field(f), w.get_field(f)), f


def test_identity_only_augmentation_is_plain_inference_on_the_device(tiny):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import ViewBatch
    from cvpr22_cross_modal_pseudo_labeling_amd.engine.bbox_aug import im_detect_bbox_aug
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import to_image_list

    model, images = tiny
    with torch.no_grad():
        want = model(images.cuda())
    got = im_detect_bbox_aug(model, ViewBatch([to_image_list(images.cuda())], [False]))
    assert sum(len(w) for w in want) > 0 and all("mask" in g.fields() for g in got)
    _same_boxlists(got, want)


def test_flip_and_scales_device_path_equals_host_route_of_the_same_views(tiny):
    """H_FLIP + two scales (shorter side <= 96): the device path against the SAME per-view model outputs pushed through the
    host route (merge, filter), then the mask head on the host route's boxes."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms
    from cvpr22_cross_modal_pseudo_labeling_amd.engine.bbox_aug import im_detect_bbox_aug, view_segments

    model, _ = tiny
    cfg = get_defaults()
    cfg.merge_from_list(["TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", True, "TEST.BBOX_AUG.SCALES", (64, 96),
                         "TEST.BBOX_AUG.MAX_SIZE", 160, "INPUT.MIN_SIZE_TEST", 80, "INPUT.MAX_SIZE_TEST", 128])
    transform = build_transforms(cfg, is_train=False)
    g = torch.Generator().manual_seed(3)
    raw, _ = transform.host([torch.randint(0, 256, (61, 83, 3), dtype=torch.uint8, generator=g),
                             torch.randint(0, 256, (90, 57, 3), dtype=torch.uint8, generator=g)])
    raw = {k: v.cuda() if torch.is_tensor(v) else v for k, v in raw.items()}
    batch = transform.device(raw)
    assert len(batch) == 4 and batch.flips == [False, True, False, False]
    got = im_detect_bbox_aug(model, batch)
    # the same views, by hand
    per_view = [model.detect_unfiltered(images)[1] for images in batch.views]
    nc = model.roi_heads["box"].predictor.num_classes
    boxes, scores, segments = view_segments(per_view, batch.flips, nc)
    assert len(segments) == 8 and [s[2] for s in segments] == [0] * 4 + [1] * 4
    post = model.roi_heads_student["box"].post_processor
    merged = _C.merge_view_detections(boxes.cpu(), scores.cpu(), segments, nc, post.score_thresh)
    assert len({int(s) for s in (merged[2] % nc)}) > 1                 # several classes survive the threshold
    want = post.filter_merged(merged, [d.size for d in per_view[0]], nc)
    assert sum(len(w) for w in want) > 0
    for g_, w in zip(got, want):
        assert g_.size == w.size and torch.equal(g_.bbox.cpu(), w.bbox)
        assert torch.equal(g_.get_field("scores").cpu(), w.get_field("scores"))
        assert torch.equal(g_.get_field("labels").cpu(), w.get_field("labels"))
    features = model.detect_unfiltered(batch.views[0])[0]
    masks = model.segment(features, [w.to("cuda") for w in want])
    for g_, m in zip(got, masks):
        assert torch.equal(g_.get_field("mask"), m.get_field("mask"))


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"ovis_tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_run_datasets_with_augmentation_saves_masks_and_scores(tmp_path):
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.data.catalog import DatasetCatalog
    from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import calibrate_stem_bn, make_batch, make_embeddings
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.detector import build_detection_model

    paths = tiny_coco.write(tmp_path / "data")
    name = "coco_zeroshot_val"
    cfg = get_defaults()
    cfg.merge_from_file(YAML)
    cfg.merge_from_list(["DATALOADER.NUM_WORKERS", 0, "INPUT.MIN_SIZE_TEST", 80, "INPUT.MAX_SIZE_TEST", 128, "TEST.IMS_PER_BATCH", 2,
                         "MODEL.RPN.PRE_NMS_TOP_N_TEST", 200, "MODEL.RPN.POST_NMS_TOP_N_TEST", 40, "DATASETS.TEST", (name,),
                         "TEST.BBOX_AUG.ENABLED", True, "TEST.BBOX_AUG.H_FLIP", True, "TEST.BBOX_AUG.SCALES", (64, 96),
                         "TEST.BBOX_AUG.MAX_SIZE", 160, "TEST.BBOX_AUG.SCALE_H_FLIP", True, "OUTPUT_DIR", str(tmp_path / "out")])
    cfg.freeze()
    torch.manual_seed(11)
    device = torch.device("cuda", 0)
    model = build_detection_model(cfg).to(device)
    calibrate_stem_bn(model, make_batch(1, device=device, seed=7)[0])
    model.set_class_embeddings(make_embeddings(cfg.MODEL.ROI_BOX_HEAD.EMB_DIM, device=device)[1])
    tool = _tool("infer_net")
    results = tool.run_datasets(cfg, model, DatasetCatalog(paths["catalog"], paths["root"]), device, evaluate=True)
    out = os.path.join(str(tmp_path / "out"), "inference", name)
    saved = torch.load(os.path.join(out, "predictions.pth"), weights_only=False)
    assert len(saved) == len(results[name]) == len(tiny_coco.IDS_WITH_VALID_ANNOTATION)
    for det in saved:
        assert {"scores", "labels", "mask"} <= set(det.fields()) and det.get_field("mask").shape[0] == len(det)
    import json
    with open(os.path.join(out, "coco_results.json")) as f:
        scored = json.load(f)
    assert sorted(scored) == ["bbox", "segm"]
    for iou_type in scored:
        assert all(math.isfinite(v) for v in scored[iou_type].values()) and "AP" in scored[iou_type]
