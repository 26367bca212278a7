"""Multi-scale / flip testing (TEST.BBOX_AUG): maskrcnn_benchmark/engine/bbox_aug.py:11-69.

The reference runs the whole detector per view, maps every view's detections back per view and per image
(``BoxList.transpose`` / ``BoxList.resize``), concatenates them and filters the concatenation with the box
post-processor's per-class loop.  Here the views of a batch come from one upload (data/transforms.py::ViewTransform), the
detector's unfiltered pass runs per view, and ONE ``_C.merge_view_detections`` writes the flipped-back, rescaled,
thresholded, class-major candidate list of the whole batch, which ``PostProcessor.filter_merged`` hands to the grouped NMS
as it is.  Detections are in the first view's frame and size, as in the reference.

Deviation: the reference returns boxes only under augmentation; with MODEL.MASK_ON the merged boxes get
their masks here from the mask head on the FIRST (un-augmented) view's features, so mask scoring and pictures keep working.

Two options, both off by default and neither in the reference (with both off nothing below differs from before):
``vote_thresh`` -- box voting (Detectron's ``box_voting``, scoring method ID): behind the grouped NMS and the
DETECTIONS_PER_IMG cut every kept detection's box becomes the score-weighted mean of the candidates of its own (image,
class) run that overlap it by IoU >= vote_thresh (``_C.vote_boxes``); scores, labels, number and order stay.
``average_masks`` -- every view's features are kept, the final detections are mapped into every view's frame (``resize``,
then the flip: the inverse order of the merge), the mask head runs per view and ``mask`` becomes the mean of the views'
maps (``_C.average_view_masks``, mirrored views' columns reversed).  Only ``mask`` is averaged: every other field the mask
head writes (the uncertainty maps) stays the first view's.

A third option lives in the post-processor itself (``PostProcessor.soft_nms``, tools/infer_net.py --soft-nms): with it set,
``filter_merged`` decays the merged candidates' scores with ``_C.soft_nms`` (one call over the whole list) where it runs the
grouped NMS otherwise; the kept indices it hands to the vote are candidate indices either way, and the vote keeps weighing
with the candidates' ORIGINAL scores.
"""
import torch

from .. import _C
from ..modeling.structures import BoxList

# ``filter_merged`` cuts the candidate list into slices of about this many candidates, at (image, class) boundaries, one
# grouped NMS each.  A call tests every pair of its candidates whatever their groups (K^2 / 2 IoU tests) and its sequential
# reduce has its pipelined form up to 12288 candidates (csrc/nms.hip: kFastBlocks), so one call over a batch's ~50 000
# candidates costs more than the per-image calls it replaces; 8192 was the fastest of 2048 ... 131072 at 2 images x 6 views
# x 1000 proposals x 66 classes (profiles/ab_view_merge.txt).
NMS_SLICE_CANDIDATES = 8192


def view_segments(detections_per_view, flips, num_classes):
    """The segment records of ``_C.merge_view_detections`` for ``detections_per_view[v][i]`` (view v, image i; bbox
    [n * C, 4], ``scores`` [n * C]), rows laid out image-major then view order -> (boxes [R, C, 4], scores [R, C], segments).
    ``ratio_*`` = float(first view's size) / float(view's size), what ``BoxList.resize`` computes (bbox_aug.py:20-24); a
    mirrored view is flipped back first, in its own width (bbox_aug.py:106-107)."""
    boxes, scores, segments, row = [], [], [], 0
    num_images = len(detections_per_view[0])
    for i in range(num_images):
        target_w, target_h = detections_per_view[0][i].size
        for view, flip in zip(detections_per_view, flips):
            det = view[i]
            w, h = det.size
            n = len(det) // num_classes
            boxes.append(det.bbox.reshape(n, num_classes, 4))
            scores.append(det.get_field("scores").reshape(n, num_classes))
            segments.append((row, n, i, w, int(flip), float(target_w) / float(w), float(target_h) / float(h)))
            row += n
    return torch.cat(boxes, 0), torch.cat(scores, 0), segments


def _unwrap(model):
    return model.module if hasattr(model, "module") and not hasattr(model, "detect_unfiltered") else model


def model_cfg(model):
    """The configuration a detector's heads were built from (None for a module without such heads)."""
    return getattr(getattr(_unwrap(model), "roi_heads", None), "cfg", None)


def evaluating_post_processor(model):
    """The box post-processor that filters a detector's evaluation pass, single view or merged views: the student's when the
    model has one (its ``soft_nms`` attribute is what tools/infer_net.py --soft-nms sets)."""
    model = _unwrap(model)
    heads = model.roi_heads_student if hasattr(model, "roi_heads_student") else model.roi_heads
    return heads["box"].post_processor


def check_options(cfg, vote_thresh=None, average_masks=False):
    """The two options against the configuration; raises ValueError with what is wrong (tools/infer_net.py says the same)."""
    if vote_thresh is not None and not 0.0 < float(vote_thresh) <= 1.0:
        raise ValueError(f"box voting: the IoU threshold must lie in (0, 1], got {vote_thresh}")
    if average_masks and not cfg.MODEL.MASK_ON:
        raise ValueError("view-averaged masks need MODEL.MASK_ON True: there is no mask head to average")


def _with_boxes(boxlist, bbox):
    """``boxlist`` with other coordinates: same size, same fields."""
    out = BoxList(bbox, boxlist.size)
    for name in boxlist.fields():
        out.add_field(name, boxlist.get_field(name))
    return out


def _average_masks(model, features, results, per_view, flips):
    """``results`` with ``mask`` = the mean over the views of the mask head's maps.  View 0 runs on the detections as they
    are, so every other field it writes is view 0's; view v on the detections in v's frame and size."""
    out = model.segment(features[0], results)
    maps = [torch.cat([r.get_field("mask") for r in out], 0)]
    for v in range(1, len(features)):
        boxes = []
        for r, det in zip(results, per_view[v]):
            b = r.resize(det.size)
            boxes.append(b.transpose(0) if flips[v] else b)
        maps.append(torch.cat([r.get_field("mask") for r in model.segment(features[v], boxes)], 0))
    mean = _C.average_view_masks(torch.stack(maps, 0), flips)
    for r, m in zip(out, mean.split([len(r) for r in out], 0)):
        r.add_field("mask", m)
    return out


@torch.no_grad()
def im_detect_bbox_aug(model, view_batch, cfg=None, vote_thresh=None, average_masks=False):
    """``view_batch``: data.transforms.ViewBatch on the model's device -> one BoxList per image (``scores``, ``labels``,
    and ``mask`` when MODEL.MASK_ON), in the first view's frame.  ``cfg``: the model's configuration (default: the one
    its heads were built from).  ``vote_thresh`` (None: off; a float in (0, 1]): box voting over the merged candidates;
    ``average_masks``: ``mask`` is the mean over every view's mask-head pass instead of the first view's (module docstring)."""
    model = _unwrap(model)
    heads = model.roi_heads_student if hasattr(model, "roi_heads_student") else model.roi_heads
    box_head, cfg = heads["box"], (heads.cfg if cfg is None else cfg)
    check_options(cfg, vote_thresh, average_masks)
    features, per_view = [], []
    for images in view_batch.views:
        view_features, detections = model.detect_unfiltered(images)
        if not features or average_masks:
            features.append(view_features)  # without average_masks the masks come from the un-augmented view alone
        per_view.append(detections)
    sizes = [det.size for det in per_view[0]]
    num_classes = model.roi_heads["box"].predictor.num_classes   # bbox_aug.py:66, the classifier's matrix
    boxes, scores, segments = view_segments(per_view, view_batch.flips, num_classes)
    post = box_head.post_processor
    merged = _C.merge_view_detections(boxes, scores, segments, num_classes, post.score_thresh)
    if vote_thresh is None:
        results = post.filter_merged(merged, sizes, num_classes, slice_candidates=NMS_SLICE_CANDIDATES)
    else:
        results, kept = post.filter_merged(merged, sizes, num_classes, slice_candidates=NMS_SLICE_CANDIDATES, return_kept=True)
        cand_boxes, cand_scores, cand_group, offsets = merged
        voted = _C.vote_boxes(cand_boxes, cand_scores, offsets, cand_group, torch.cat(kept, 0), float(vote_thresh))
        voted = voted.split([len(r) for r in results], 0)
        results = [_with_boxes(r, b) for r, b in zip(results, voted)]
    if cfg.MODEL.MASK_ON:
        if average_masks:
            results = _average_masks(model, features, results, per_view, view_batch.flips)
        else:
            results = model.segment(features[0], results)
    return results
