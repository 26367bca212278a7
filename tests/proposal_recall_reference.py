"""TEST-ONLY: a NumPy float32 restatement of the reference's box-proposal recall, ``evaluate_box_proposals``
(maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py:199-312) over ``boxlist_iou``
(structures/boxlist_ops.py:53-89), written from those lines with explicit loops: the greedy rounds one by one, ``np.argmax``
for ``torch.max``'s first occurrence.  Everything is float32, every operation in the reference's order; NumPy's elementwise
float32 arithmetic is IEEE, one rounding per operation, as torch's is.

Unlike the reference, which returns the recorded overlaps in ROUND order, ``gt_overlaps`` returns them PER GROUND TRUTH
(what the device kernel returns): the IoU of the round that consumed it, 0 for one inside the area range that no round
consumed, -1 for one outside.  The count of the values >= 0 is the reference's ``num_pos``; sorted, those of the images that
have a proposal are its ``gt_overlaps`` (an image without proposals adds to ``num_pos`` only, coco_eval.py:261-267: its
ground truths are zeros here, which no threshold counts)."""
from collections import OrderedDict

import numpy as np

F = np.float32
ONE = F(1)
AREA_RANGES = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]]  # coco_eval.py:218-222
AREA_SUFFIXES = ("", "s", "m", "l")  # coco_eval.py:31
LIMITS = (100, 1000)                 # coco_eval.py:32
# torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32) (coco_eval.py:297-299): start + i * step in fp64, then rounded
THRESHOLDS = (0.5 + np.arange(10, dtype=np.float64) * 0.05).astype(F)


def box_iou(p, g):
    """boxlist_iou of one pair of xyxy boxes, scalar float32 (boxlist_ops.py:75-88, TO_REMOVE = 1)."""
    p, g = [F(v) for v in p], [F(v) for v in g]
    area1 = (p[2] - p[0] + ONE) * (p[3] - p[1] + ONE)
    area2 = (g[2] - g[0] + ONE) * (g[3] - g[1] + ONE)
    w = min(p[2], g[2]) - max(p[0], g[0]) + ONE
    h = min(p[3], g[3]) - max(p[1], g[1]) + ONE
    w, h = max(w, F(0)), max(h, F(0))
    inter = w * h
    return inter / (area1 + area2 - inter)


def iou_matrix(props, gts):
    """float32 [P, G]: ``box_iou`` of every pair; a loop over the ground truths, the same float32 operations elementwise
    over the proposals."""
    props, gts = np.asarray(props, dtype=F).reshape(-1, 4), np.asarray(gts, dtype=F).reshape(-1, 4)
    out = np.zeros((len(props), len(gts)), dtype=F)
    area1 = (props[:, 2] - props[:, 0] + ONE) * (props[:, 3] - props[:, 1] + ONE)
    for j, g in enumerate(gts):
        area2 = (g[2] - g[0] + ONE) * (g[3] - g[1] + ONE)
        w = np.maximum(np.minimum(props[:, 2], g[2]) - np.maximum(props[:, 0], g[0]) + ONE, F(0))
        h = np.maximum(np.minimum(props[:, 3], g[3]) - np.maximum(props[:, 1], g[1]) + ONE, F(0))
        inter = w * h
        out[:, j] = inter / (area1 + area2 - inter)
    assert out.dtype == F
    return out


def gt_overlaps(props, gts, gt_areas, area_range, limit, iou=None):
    """float32 [G] for one image, one area range and one limit (coco_eval.py:258-290).  ``props`` best first.  ``iou``: the
    image's full ``iou_matrix`` when the caller already has it."""
    props, gts = np.asarray(props, dtype=F).reshape(-1, 4), np.asarray(gts, dtype=F).reshape(-1, 4)
    gt_areas = np.asarray(gt_areas, dtype=F)
    lo, hi = F(area_range[0]), F(area_range[1])
    out = np.zeros(len(gts), dtype=F)
    valid = []
    for j in range(len(gts)):
        if gt_areas[j] >= lo and gt_areas[j] <= hi:
            valid.append(j)
        else:
            out[j] = -1
    num_props = min(len(props), limit)
    if not valid or num_props == 0:
        return out
    full = iou_matrix(props, gts) if iou is None else iou
    overlaps = full[:num_props][:, valid].copy()
    for _ in range(min(num_props, len(valid))):
        max_overlaps = np.zeros(len(valid), dtype=F)
        argmax_overlaps = np.zeros(len(valid), dtype=np.int64)
        for c in range(len(valid)):
            argmax_overlaps[c] = np.argmax(overlaps[:, c])  # first occurrence
            max_overlaps[c] = overlaps[argmax_overlaps[c], c]
        gt_ind = int(np.argmax(max_overlaps))
        assert max_overlaps[gt_ind] >= 0
        box_ind = int(argmax_overlaps[gt_ind])
        out[valid[gt_ind]] = overlaps[box_ind, gt_ind]
        overlaps[box_ind, :] = -1
        overlaps[:, gt_ind] = -1
    return out


def overlaps_table(images, area_ranges=AREA_RANGES, limits=LIMITS):
    """float32 [A, L, G total] over ``images``: dicts of ``props`` [P, 4], ``gt_boxes`` [G, 4], ``gt_areas`` [G] -- the
    layout of the device kernel's output for the images' ground truths concatenated."""
    total = sum(len(im["gt_boxes"]) for im in images)
    out = np.zeros((len(area_ranges), len(limits), total), dtype=F)
    base = 0
    for im in images:
        g = len(im["gt_boxes"])
        iou = iou_matrix(im["props"], im["gt_boxes"])
        for a, rng in enumerate(area_ranges):
            for l, limit in enumerate(limits):
                out[a, l, base:base + g] = gt_overlaps(im["props"], im["gt_boxes"], im["gt_areas"], rng, limit, iou)
        base += g
    return out


def average_recall(values):
    """(AR float, num_pos, the sorted overlaps) of per-ground-truth values (coco_eval.py:294-305): the entries >= 0 are the
    positives.  -1.0 when there is none (the reference would divide by zero)."""
    values = np.asarray(values, dtype=F)
    overlaps = np.sort(values[values >= 0])
    num_pos = len(overlaps)
    if num_pos == 0:
        return -1.0, 0, overlaps
    recalls = np.zeros(len(THRESHOLDS), dtype=F)
    for i, t in enumerate(THRESHOLDS):
        recalls[i] = F(np.count_nonzero(overlaps >= t)) / F(num_pos)
    total = F(0)
    for r in recalls:
        total = total + r
    return float(total / F(len(recalls))), num_pos, overlaps


def image_row(boxes, size, scores, width, height, anns):
    """One image of ``overlaps_table`` as coco_eval.py:233-256 makes it, or None when it has no non-crowd annotation: the
    prediction's ``boxes`` (at ``size`` = (width, height) of the transformed image) resized to the file's ``width`` x
    ``height`` (bounding_box.py:91-127: one ratio when both axes agree, else one per axis; a float32 multiply either way),
    sorted by ``scores`` descending (stably); the non-crowd annotations' boxes as xyxy with x2 = x + max(w - 1, 0)
    (bounding_box.py:60-66) and their ``area``.  ``gt_cats``: the annotations' category ids."""
    anns = [a for a in anns if a.get("iscrowd", 0) == 0]
    if not anns:
        return None
    boxes = np.asarray(boxes, dtype=F).reshape(-1, 4)
    rw, rh = float(width) / float(size[0]), float(height) / float(size[1])
    boxes = boxes * np.asarray([rw, rh, rw, rh], dtype=np.float64).astype(F)
    order = np.argsort(-np.asarray(scores), kind="stable")
    gt = np.asarray([a["bbox"] for a in anns], dtype=F).reshape(-1, 4)
    gt_xyxy = np.stack([gt[:, 0], gt[:, 1], gt[:, 0] + np.maximum(gt[:, 2] - ONE, F(0)),
                        gt[:, 1] + np.maximum(gt[:, 3] - ONE, F(0))], axis=1)
    return {"props": boxes[order], "gt_boxes": gt_xyxy, "gt_areas": np.asarray([a["area"] for a in anns], dtype=F),
            "gt_cats": [a["category_id"] for a in anns]}


def fixture_rows(fixture):
    """``image_row`` of every image of tests/golden/proposal_recall.npz (the loaded archive)."""
    rows = []
    for k in range(len(fixture["file_wh"])):
        p0, p1 = fixture["prop_start"][k:k + 2]
        a0, a1 = fixture["ann_start"][k:k + 2]
        anns = [{"bbox": fixture["ann_bbox"][i].tolist(), "area": float(fixture["ann_area"][i]),
                 "iscrowd": int(fixture["ann_iscrowd"][i]), "category_id": int(fixture["ann_category"][i])} for i in range(a0, a1)]
        row = image_row(fixture["boxes"][p0:p1], tuple(fixture["pred_wh"][k].tolist()), fixture["objectness"][p0:p1],
                        int(fixture["file_wh"][k][0]), int(fixture["file_wh"][k][1]), anns)
        if row is not None:
            rows.append(row)
    return rows


def dataset_rows(dataset, predictions, score_field="objectness"):
    """``image_row`` of every image of a dataset object (data/datasets.py) and its prediction list."""
    rows = []
    for idx, pred in enumerate(predictions):
        info = dataset.get_img_info(idx)
        row = image_row(pred.bbox.detach().cpu().numpy(), pred.size, pred.get_field(score_field).detach().cpu().numpy(),
                        info["width"], info["height"], dataset.coco.anns(dataset.id_to_img_map[idx]))
        if row is not None:
            rows.append(row)
    return rows


def evaluate(rows, limits=LIMITS, splits=None):
    """OrderedDict AR@100, ARs@100, ..., ARl@1000 (coco_eval.py:31-38), then AR@<limit>_split_<split> for ``splits`` =
    {split: [category ids]}: the "all"-range matching, numerator and denominator over the split's ground truths."""
    table = overlaps_table(rows, AREA_RANGES, limits)
    cats = np.asarray([c for r in rows for c in r["gt_cats"]], dtype=np.int64)
    out = OrderedDict()
    for l, limit in enumerate(limits):
        for a, suffix in enumerate(AREA_SUFFIXES):
            out[f"AR{suffix}@{limit:d}"] = average_recall(table[a, l])[0]
    for split, ids in (splits or {}).items():
        for l, limit in enumerate(limits):
            out[f"AR@{limit:d}_split_{split}"] = average_recall(table[0, l][np.isin(cats, list(ids))])[0]
    return out
