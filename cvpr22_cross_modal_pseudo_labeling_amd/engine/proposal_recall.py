"""Box-proposal recall -- the ``box_proposal`` task that opens the reference's evaluation table
(maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py: ``do_coco_evaluation`` :29-38, ``evaluate_box_proposals``
:199-312): AR@100, ARs@100, ARm@100, ARl@100, AR@1000, ... of a prediction list, plus AR@<limit>_split_<split> -- how many
of a split's ground truths the class-agnostic proposals cover, which for an open-vocabulary detector says whether the RPN,
trained on the seen classes, proposes the unseen ones at all.

The matching is class-agnostic, one-to-one and globally greedy -- a different one from ``COCOeval.evaluateImg`` -- and runs
on the DEVICE (csrc/proposal_recall.hip through ``_C.proposal_gt_overlaps``): one launch per chunk of images covers every
image, area range and limit and returns, per ground truth, the IoU of the round that consumed it.  The reference runs it
as a Python loop of ``torch.max`` calls per image, once per (area, limit).  What is left for the HOST is the reference's own
float32 arithmetic over a few numbers per ground truth: the count of overlaps at or above each of the ten thresholds,
divided by the number of positives, and their mean.

Semantics beyond the reference's: a value is -1.0 when there is no positive (the reference would divide by zero); the sort
by ``score_field`` is stable; an annotation without ``iscrowd`` is not a crowd.  The reference's four extra area bins
(96-128, ...) and other thresholds are not computed.  There is no host-only scoring.
"""
from collections import OrderedDict

import numpy as np
import torch

from .. import _C
from .coco_eval import _scoring_device, detection_boxes

LIMITS = (100, 1000)                  # coco_eval.py:32
AREA_SUFFIXES = ("", "s", "m", "l")   # coco_eval.py:31
# coco_eval.py:218-222: all, small, medium, large -- the upper bound is 1e5 ** 2, not COCOeval's 1e10 (the same in fp32)
AREA_RANGES = ((0 ** 2, 1e5 ** 2), (0 ** 2, 32 ** 2), (32 ** 2, 96 ** 2), (96 ** 2, 1e5 ** 2))
CHUNK_IMAGES = 512  # images per launch: a few KB each


def _thresholds():
    return torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)  # coco_eval.py:297-299


def _rows(dataset, predictions, score_field):
    """Per image with a non-crowd annotation (coco_eval.py:233-256): (proposals fp32 [P, 4] xyxy at the file's size, best
    ``score_field`` first; ground-truth boxes fp32 [G, 4] xyxy; their areas fp32 [G]; their category ids)."""
    rows = []
    for idx, pred in enumerate(predictions):
        info = dataset.get_img_info(idx)
        anns = [a for a in dataset.coco.anns(dataset.id_to_img_map[idx]) if a.get("iscrowd", 0) == 0]
        if not anns:
            continue
        boxes = detection_boxes(pred, int(info["width"]), int(info["height"]))[0].float().reshape(-1, 4)
        if len(pred):
            if not pred.has_field(score_field):
                raise ValueError(f"evaluate_box_proposals: the predictions have no '{score_field}' field")
            order = torch.sort(pred.get_field(score_field).detach().cpu(), descending=True, stable=True)[1]
            boxes = boxes[order]
        gt = torch.as_tensor([a["bbox"] for a in anns], dtype=torch.float32).reshape(-1, 4)
        x, y, w, h = gt.unbind(1)  # BoxList.convert("xyxy") of an xywh box (bounding_box.py:60-66)
        gt = torch.stack((x, y, x + (w - 1).clamp(min=0), y + (h - 1).clamp(min=0)), 1)
        areas = torch.as_tensor([a["area"] for a in anns], dtype=torch.float32)
        rows.append((boxes, gt, areas, [a["category_id"] for a in anns]))
    return rows


def gt_overlaps(rows, device, limits=LIMITS, area_ranges=AREA_RANGES, chunk_images=CHUNK_IMAGES):
    """fp32 [A, L, G total] on the host: ``_C.proposal_gt_overlaps`` over ``rows`` (what ``_rows`` makes; only the
    proposals, the ground-truth boxes and the areas of a row are read), a chunk of images a launch."""
    ranges = torch.tensor(area_ranges, dtype=torch.float32).reshape(-1, 2).to(device)
    parts = []
    for first in range(0, len(rows), chunk_images):
        chunk = rows[first:first + chunk_images]
        table, p, g = [], 0, 0
        for row in chunk:
            table.append([p, len(row[0]), g, len(row[1])])
            p += len(row[0])
            g += len(row[1])
        out = _C.proposal_gt_overlaps(torch.cat([r[0] for r in chunk]).to(device), torch.cat([r[1] for r in chunk]).to(device),
                                      torch.cat([r[2] for r in chunk]).to(device), table, ranges, list(limits))
        parts.append(out.cpu())
    return torch.cat(parts, 2) if parts else torch.zeros((len(area_ranges), len(limits), 0), dtype=torch.float32)


def average_recall(values):
    """coco_eval.py:294-305 for per-ground-truth ``values`` (fp32: >= 0 a positive's recorded overlap, -1 not a positive):
    the mean over the thresholds of count(overlap >= t) / num_pos, in fp32 as the reference computes it; -1.0 when there is
    no positive."""
    overlaps = values[values >= 0]
    num_pos = overlaps.numel()
    if num_pos == 0:
        return -1.0
    thresholds = _thresholds()
    recalls = torch.zeros_like(thresholds)
    for i, t in enumerate(thresholds):
        recalls[i] = (overlaps >= t).float().sum() / float(num_pos)
    return recalls.mean().item()


def evaluate_box_proposals(dataset, predictions, device="cuda", score_field="objectness", limits=LIMITS):
    """OrderedDict AR@100, ARs@100, ARm@100, ARl@100, AR@1000, ... (for ``limits``, in the reference's order), then
    AR@<limit>_split_<split> for every key of ``dataset.class_splits`` and every limit.  ``predictions``: BoxLists in
    dataset-index order with a ``score_field`` (``objectness`` for RPN proposals; ``scores`` scores detections as proposals,
    which is what the reference's table shows: its post-processor copies ``scores`` into ``objectness``).

    Per image, as the reference does: the prediction is resized to the file's size and sorted by ``score_field``; the ground
    truth is the ``iscrowd == 0`` annotations' ``bbox`` and ``area``; an image without ground truth contributes nothing, one
    with ground truth and no proposal only positives.  Only the first ``limit`` proposals take part; an area range keeps the
    ground truths with lo <= area <= hi.  The split keys use the "all"-range matching -- one greedy pass over all ground
    truths -- and restrict numerator and denominator to the ground truths of the split's categories.  A value is -1.0 when
    there is no positive, where the reference would divide by zero.  A box that is reversed after the resize (x2 - x1 + 1 <= 0
    or y2 - y1 + 1 <= 0, where the reference's IoU loses its meaning) is a ValueError of ``_C.proposal_gt_overlaps``; a box
    narrower than a pixel (x2 < x1 by less than 1) is scored as the reference scores it.  ``device``: the HIP device that
    matches."""
    device = _scoring_device(device, "evaluate_box_proposals")
    if len(predictions) > len(dataset):
        raise ValueError(f"evaluate_box_proposals: {len(predictions)} predictions for a dataset of {len(dataset)} images")
    rows = _rows(dataset, predictions, score_field)
    with torch.cuda.device(device):
        table = gt_overlaps(rows, device, limits)
    cats = np.asarray([c for r in rows for c in r[3]], dtype=np.int64)
    results = OrderedDict()
    for l, limit in enumerate(limits):
        for a, suffix in enumerate(AREA_SUFFIXES):
            results["AR{}@{:d}".format(suffix, limit)] = average_recall(table[a, l])
    for split, ids in dataset.class_splits.items():
        members = torch.from_numpy(np.isin(cats, list(ids)))
        for l, limit in enumerate(limits):
            results["AR@{:d}_split_{}".format(limit, split)] = average_recall(table[0, l][members])
    return results
