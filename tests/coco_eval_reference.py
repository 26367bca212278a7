"""TEST-ONLY: a scalar Python / NumPy restatement of COCO box / mask AP scoring -- pycocotools' ``COCOeval`` (``computeIoU``,
``evaluateImg``, ``accumulate``, ``summarize``) as the reference calls it in
maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py:315-333, plus the per-class / per-split AP50 of
``COCOResults.update`` (:364-404).  Plain loops over detections, ground truths and thresholds; mask IoU from dense boolean
``&`` sums, not packed bits.  It imports nothing from the product.

No fixture recorded from the reference is possible: the reference delegates scoring to ``pycocotools``, which is absent
from this build's environment and from the reference tree, so this restatement -- held to hand-derived literals by
tests/test_coco_eval_reference.py -- is the independent statement the device code is compared with.

Inputs are plain Python: ``images`` is a list, in image-id order, of ``{"dets": [...], "gts": [...]}``; a detection is
``{"category": index, "score": float, "bbox": [x, y, w, h]}`` or, for segm, ``{"category", "score", "mask": bool [H, W]}``, in
prediction order; a ground truth ``{"category", "bbox" or "mask", "area", "iscrowd"}`` in annotation order.
"""
from collections import OrderedDict

import numpy as np

IOU_THRESHOLDS = np.linspace(.5, .95, 10)
RECALL_THRESHOLDS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RANGES = [(0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10)]


def box_iou(d, g, crowd):
    dx, dy, dw, dh = (np.float64(v) for v in d)
    gx, gy, gw, gh = (np.float64(v) for v in g)
    iw = max(min(dx + dw, gx + gw) - max(dx, gx), np.float64(0))
    ih = max(min(dy + dh, gy + gh) - max(dy, gy), np.float64(0))
    i = iw * ih
    u = dw * dh if crowd else dw * dh + gw * gh - i
    return np.float64(0) if u == 0 else i / u


def mask_iou(d, g, crowd):
    d, g = np.asarray(d, dtype=bool), np.asarray(g, dtype=bool)
    i = int((d & g).sum())
    u = int(d.sum()) if crowd else int(d.sum()) + int(g.sum()) - i
    return np.float64(0) if u == 0 else np.float64(i) / np.float64(u)


def match_problem(ious, det_areas, gt_areas, gt_crowd):
    """evaluateImg for one (image, category): ious [D][G] of the detections in score order against the ground truths in
    annotation order -> (dt_match [A][T][D]: index of the matched ground truth in annotation order or -1, dt_ignore,
    gt_ignore [A][G])."""
    num_d, num_g = len(det_areas), len(gt_areas)
    dt_match = np.full((len(AREA_RANGES), len(IOU_THRESHOLDS), num_d), -1, dtype=np.int32)
    dt_ignore = np.zeros((len(AREA_RANGES), len(IOU_THRESHOLDS), num_d), dtype=bool)
    gt_ignore = np.zeros((len(AREA_RANGES), num_g), dtype=bool)
    for a, (lo, hi) in enumerate(AREA_RANGES):
        ignore = [bool(gt_crowd[g]) or gt_areas[g] < lo or gt_areas[g] > hi for g in range(num_g)]
        gt_ignore[a] = ignore
        order = [g for g in range(num_g) if not ignore[g]] + [g for g in range(num_g) if ignore[g]]  # stable
        for t, thr in enumerate(IOU_THRESHOLDS):
            taken = [False] * num_g
            for d in range(num_d):
                best, m = min(thr, 1 - 1e-10), -1
                for g in order:
                    if taken[g] and not gt_crowd[g]:
                        continue
                    if m > -1 and not ignore[m] and ignore[g]:
                        break
                    if ious[d][g] < best:
                        continue
                    best, m = ious[d][g], g
                if m == -1:
                    dt_ignore[a, t, d] = det_areas[d] < lo or det_areas[d] > hi
                    continue
                taken[m] = True
                dt_match[a, t, d] = m
                dt_ignore[a, t, d] = ignore[m]
    return dt_match, dt_ignore, gt_ignore


def match_tables(images, iou_type):
    """The match tables of every (image, category) problem with a detection or a ground truth, in image order: ``category``
    [P], ``det_start`` / ``gt_start`` [P + 1], ``scores`` [D], ``dt_match`` / ``dt_ignore`` [A, T, D], ``gt_ignore`` [A, G]."""
    key = "bbox" if iou_type == "bbox" else "mask"
    iou = box_iou if iou_type == "bbox" else mask_iou
    category, det_start, gt_start, scores, dtm, dtig, gtig = [], [0], [0], [], [], [], []
    for image in images:
        for c in sorted({d["category"] for d in image["dets"]} | {g["category"] for g in image["gts"]}):
            dets = [d for d in image["dets"] if d["category"] == c]
            dets = [dets[i] for i in np.argsort([-d["score"] for d in dets], kind="mergesort")][:MAX_DETS[-1]]
            gts = [g for g in image["gts"] if g["category"] == c]
            ious = [[iou(d[key], g[key], g["iscrowd"]) for g in gts] for d in dets]
            if iou_type == "bbox":
                det_areas = [np.float64(d["bbox"][2]) * np.float64(d["bbox"][3]) for d in dets]
            else:
                det_areas = [float(np.asarray(d["mask"], dtype=bool).sum()) for d in dets]
            m, di, gi = match_problem(ious, det_areas, [g["area"] for g in gts], [g["iscrowd"] for g in gts])
            category.append(c)
            det_start.append(det_start[-1] + len(dets))
            gt_start.append(gt_start[-1] + len(gts))
            scores += [d["score"] for d in dets]
            dtm.append(m)
            dtig.append(di)
            gtig.append(gi)
    num_a, num_t = len(AREA_RANGES), len(IOU_THRESHOLDS)
    return {"category": np.asarray(category, dtype=np.int64), "det_start": np.asarray(det_start), "gt_start": np.asarray(gt_start),
            "scores": np.asarray(scores, dtype=np.float64),
            "dt_match": np.concatenate(dtm + [np.zeros((num_a, num_t, 0), np.int32)], axis=2),
            "dt_ignore": np.concatenate(dtig + [np.zeros((num_a, num_t, 0), bool)], axis=2),
            "gt_ignore": np.concatenate(gtig + [np.zeros((num_a, 0), bool)], axis=1)}


def accumulate(tables, num_categories):
    """precision [T, R, K, A, M], -1 where a (category, area) has no image entry or no non-ignored ground truth."""
    precision = -np.ones((len(IOU_THRESHOLDS), len(RECALL_THRESHOLDS), num_categories, len(AREA_RANGES), len(MAX_DETS)))
    for k in range(num_categories):
        problems = [p for p in range(len(tables["category"])) if tables["category"][p] == k]
        if not problems:
            continue
        for a in range(len(AREA_RANGES)):
            for m, max_det in enumerate(MAX_DETS):
                scores, matched, ignored, npig = [], [], [], 0
                for p in problems:
                    rows = list(range(tables["det_start"][p], tables["det_start"][p + 1]))[:max_det]
                    scores += [tables["scores"][r] for r in rows]
                    matched.append(tables["dt_match"][a][:, rows] >= 0)
                    ignored.append(tables["dt_ignore"][a][:, rows])
                    npig += sum(1 for g in range(tables["gt_start"][p], tables["gt_start"][p + 1]) if not tables["gt_ignore"][a][g])
                if npig == 0:
                    continue
                order = np.argsort(-np.asarray(scores, dtype=np.float64), kind="mergesort")
                matched, ignored = np.concatenate(matched, axis=1)[:, order], np.concatenate(ignored, axis=1)[:, order]
                for t in range(len(IOU_THRESHOLDS)):
                    tp, fp, pr, rc = 0.0, 0.0, [], []
                    for d in range(len(order)):
                        if not ignored[t, d]:
                            tp += 1.0 if matched[t, d] else 0.0
                            fp += 0.0 if matched[t, d] else 1.0
                        rc.append(tp / npig)
                        pr.append(tp / (fp + tp + np.spacing(1)))
                    for i in range(len(pr) - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    q = np.zeros(len(RECALL_THRESHOLDS))
                    for r, i in enumerate(np.searchsorted(rc, RECALL_THRESHOLDS, side="left")):
                        if i < len(pr):
                            q[r] = pr[i]
                    precision[t, :, k, a, m] = q
    return precision


def _mean(values):
    values = values[values > -1]
    return float(np.mean(values)) if values.size else -1.0


def summarize(precision, category_names, class_splits):
    m = MAX_DETS.index(100)
    t50, t75 = int(np.where(IOU_THRESHOLDS == .5)[0][0]), int(np.where(IOU_THRESHOLDS == .75)[0][0])
    out = OrderedDict()
    out["AP"] = _mean(precision[:, :, :, 0, m])
    out["AP50"] = _mean(precision[t50, :, :, 0, m])
    out["AP75"] = _mean(precision[t75, :, :, 0, m])
    out["APs"], out["APm"], out["APl"] = (_mean(precision[:, :, :, a, m]) for a in (1, 2, 3))
    for k, name in enumerate(category_names):
        out[f"AP50_class_{name}"] = _mean(precision[t50, :, k, 0, m])
    for split, cats in class_splits.items():
        out[f"AP50_split_{split}"] = _mean(precision[t50][:, list(cats)][:, :, 0, m])
    return out


def evaluate(images, iou_type, category_names, class_splits):
    tables = match_tables(images, iou_type)
    return summarize(accumulate(tables, len(category_names)), category_names, class_splits)
