"""TEST-ONLY: a NumPy restatement of Boundary IoU / Boundary AP (Cheng et al., CVPR 2021) as include/ovis_hip.h states the
rule, independent of the kernel's formulation: the erosion is LITERALLY ``d`` iterations of a 3x3 minimum over a
zero-padded array (``mask_to_boundary``'s one-pixel zero border and ``cv2.erode(iterations=d)``), not a windowed AND of a
bit stream; the IoUs are ratios of Python integers.  Matching, accumulate and summarise are those of
tests/coco_eval_reference.py, by import.  It imports nothing from the product.

``boundary-iou-api`` and ``cv2`` are absent from this build's environment, so no fixture recorded from them is possible;
tests/test_boundary_reference.py holds this restatement to hand-derived cases and to the closed form of the erosion.
"""
import math

import numpy as np

from tests import coco_eval_reference as ref

DILATION_RATIO = 0.02


def dilation(height, width, ratio=DILATION_RATIO):
    return max(1, int(round(ratio * math.sqrt(height * height + width * width))))


def erode(mask, d):
    """``d`` iterations of: pad with one ring of zeros, take the minimum of every 3x3 neighbourhood."""
    m = np.asarray(mask, dtype=bool)
    h, w = m.shape
    for _ in range(d):
        p = np.zeros((h + 2, w + 2), dtype=bool)
        p[1:-1, 1:-1] = m
        out = np.ones((h, w), dtype=bool)
        for dy in range(3):
            for dx in range(3):
                out &= p[dy:dy + h, dx:dx + w]
        m = out
    return m


def erode_closed_form(mask, d):
    """Pixel (y, x) survives iff the (2d + 1)^2 square around it lies inside the image and is all set -- scalar loops."""
    m = np.asarray(mask, dtype=bool)
    h, w = m.shape
    out = np.zeros((h, w), dtype=bool)
    for y in range(d, h - d):
        for x in range(d, w - d):
            out[y, x] = m[y - d:y + d + 1, x - d:x + d + 1].all()
    return out


def boundary(mask, d):
    m = np.asarray(mask, dtype=bool)
    return m & ~erode(m, d)


def pack(masks):
    """bool [N, H, W] -> int64 [N, ceil(H * W / 64)]: pixel p = y * W + x is bit p % 64 of word p / 64, the tail zero."""
    masks = np.asarray(masks, dtype=bool)
    n, pixels = masks.shape[0], masks.shape[1] * masks.shape[2]
    nwords = (pixels + 63) // 64
    padded = np.zeros((n, nwords * 64), dtype=np.uint8)
    padded[:, :pixels] = masks.reshape(n, pixels)
    return np.packbits(padded, axis=1, bitorder="little").view("<i8").reshape(n, nwords)


def _ratio(inter, mine, other, crowd):
    union = mine if crowd else mine + other - inter
    return np.float64(0) if union == 0 else np.float64(inter) / np.float64(union)


def min_iou(d, g, crowd, dilation_d):
    """min(mask IoU, boundary IoU) of two masks of one image, both ratios from Python integers."""
    d, g = np.asarray(d, dtype=bool), np.asarray(g, dtype=bool)
    bd, bg = boundary(d, dilation_d), boundary(g, dilation_d)
    mask_iou = _ratio(int((d & g).sum()), int(d.sum()), int(g.sum()), crowd)
    boundary_iou = _ratio(int((bd & bg).sum()), int(bd.sum()), int(bg.sum()), crowd)
    return min(mask_iou, boundary_iou)


def match_tables(images, ratio=DILATION_RATIO):
    """tests/coco_eval_reference.py::match_tables for Boundary AP: the same problems, orders and areas (the MASK areas),
    the IoU replaced by ``min_iou`` with the image's own dilation.  ``images``: the segm input of that module."""
    category, det_start, gt_start, scores, dtm, dtig, gtig = [], [0], [0], [], [], [], []
    for image in images:
        for c in sorted({d["category"] for d in image["dets"]} | {g["category"] for g in image["gts"]}):
            dets = [d for d in image["dets"] if d["category"] == c]
            dets = [dets[i] for i in np.argsort([-d["score"] for d in dets], kind="mergesort")][:ref.MAX_DETS[-1]]
            gts = [g for g in image["gts"] if g["category"] == c]
            ious = [[min_iou(d["mask"], g["mask"], g["iscrowd"], dilation(*np.asarray(d["mask"]).shape, ratio)) for g in gts]
                    for d in dets]
            det_areas = [float(np.asarray(d["mask"], dtype=bool).sum()) for d in dets]
            m, di, gi = ref.match_problem(ious, det_areas, [g["area"] for g in gts], [g["iscrowd"] for g in gts])
            category.append(c)
            det_start.append(det_start[-1] + len(dets))
            gt_start.append(gt_start[-1] + len(gts))
            scores += [d["score"] for d in dets]
            dtm.append(m)
            dtig.append(di)
            gtig.append(gi)
    num_a, num_t = len(ref.AREA_RANGES), len(ref.IOU_THRESHOLDS)
    return {"category": np.asarray(category, dtype=np.int64), "det_start": np.asarray(det_start), "gt_start": np.asarray(gt_start),
            "scores": np.asarray(scores, dtype=np.float64),
            "dt_match": np.concatenate(dtm + [np.zeros((num_a, num_t, 0), np.int32)], axis=2),
            "dt_ignore": np.concatenate(dtig + [np.zeros((num_a, num_t, 0), bool)], axis=2),
            "gt_ignore": np.concatenate(gtig + [np.zeros((num_a, 0), bool)], axis=1)}


def evaluate(images, category_names, class_splits, ratio=DILATION_RATIO):
    tables = match_tables(images, ratio)
    return ref.summarize(ref.accumulate(tables, len(category_names)), category_names, class_splits)
