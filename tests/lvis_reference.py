"""TEST-ONLY: a scalar Python / NumPy restatement of LVIS-style federated scoring -- rules 1 to 10 of include/ovis_hip.h
("LVIS-style federated AP") -- written per (image, category), area range and threshold, the way the rule text reads: plain
loops over dicts.  It imports nothing from the product; the box and mask IoU are restated here, only the boundary band comes
from tests/boundary_reference.py (itself a restatement).

No fixture recorded from ``lvis-api`` is possible: it is absent from this build's environment, so this restatement -- held
to hand-computed cases by tests/test_lvis_reference.py -- is the independent statement the device code is compared with.
Neither has been compared with lvis-api's own output.

Inputs are plain Python.  ``data`` is the annotation file as a dict: ``categories`` [{"id", "name", "frequency"}], ``images``
[{"id", "neg_category_ids", "not_exhaustive_category_ids"}], ``annotations`` [{"image_id", "category_id", "bbox", optional
"area", optional "ignore", for segm / boundary "mask": bool [H, W]}] in file order.  ``dets`` is a list, in file / prediction
order, of {"image_id", "category_id", "score", "bbox" [x, y, w, h] or "mask": bool [H, W]}.
"""
from collections import OrderedDict

import numpy as np

from tests import boundary_reference as bref

IOU_THRESHOLDS = np.linspace(.5, .95, 10)
RECALL_THRESHOLDS = np.linspace(0, 1, 101)
AREA_RANGES = [(0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10)]
MAX_DETS = 300
FREQUENCIES = ("r", "c", "f")


# ---- rule 1 ---------------------------------------------------------------------------------------------------------------------
def check(data):
    for image in sorted(data["images"], key=lambda im: im["id"]):
        for key in ("neg_category_ids", "not_exhaustive_category_ids"):
            if key not in image:
                raise ValueError(f"image {image['id']} has no '{key}'")
    for cat in sorted(data["categories"], key=lambda c: c["id"]):
        if cat.get("frequency") not in FREQUENCIES:
            raise ValueError(f"category {cat['id']} has no 'frequency'")


# ---- rule 6 ---------------------------------------------------------------------------------------------------------------------
def box_iou(d, g):
    dx, dy, dw, dh = (np.float64(v) for v in d)
    gx, gy, gw, gh = (np.float64(v) for v in g)
    iw = max(min(dx + dw, gx + gw) - max(dx, gx), np.float64(0))
    ih = max(min(dy + dh, gy + gh) - max(dy, gy), np.float64(0))
    i = iw * ih
    u = dw * dh + gw * gh - i
    return np.float64(0) if u == 0 else i / u


def mask_iou(d, g):
    d, g = np.asarray(d, dtype=bool), np.asarray(g, dtype=bool)
    i = int((d & g).sum())
    u = int(d.sum()) + int(g.sum()) - i
    return np.float64(0) if u == 0 else np.float64(i) / np.float64(u)


def boundary_min_iou(d, g, ratio=bref.DILATION_RATIO):
    d, g = np.asarray(d, dtype=bool), np.asarray(g, dtype=bool)
    depth = bref.dilation(d.shape[0], d.shape[1], ratio)
    return min(mask_iou(d, g), mask_iou(bref.boundary(d, depth), bref.boundary(g, depth)))


def pair_iou(det, gt, iou_type):
    if iou_type == "bbox":
        return box_iou(det["bbox"], gt["bbox"])
    return mask_iou(det["mask"], gt["mask"]) if iou_type == "segm" else boundary_min_iou(det["mask"], gt["mask"])


def det_area(det, iou_type):
    if iou_type == "bbox":
        return np.float64(det["bbox"][2]) * np.float64(det["bbox"][3])
    return float(np.asarray(det["mask"], dtype=bool).sum())


def gt_area(ann):
    return ann["area"] if "area" in ann else ann["bbox"][2] * ann["bbox"][3]


# ---- rules 3 and 4 --------------------------------------------------------------------------------------------------------------
def kept_detections(data, dets, max_dets=MAX_DETS):
    """{image id: the detections of that image that are judged, by descending score (stable)}."""
    kept = {}
    for image in data["images"]:
        mine = [d for d in dets if d["image_id"] == image["id"]]
        order = sorted(range(len(mine)), key=lambda k: -mine[k]["score"])   # sorted() is stable: ties keep file order
        if max_dets >= 0:
            order = order[:max_dets]                                          # the cap acts before anything else
        positives = {a["category_id"] for a in data["annotations"] if a["image_id"] == image["id"]}
        looked_for = positives | set(image["neg_category_ids"])
        kept[image["id"]] = [mine[k] for k in order if mine[k]["category_id"] in looked_for]
    return kept


# ---- rules 7 and 8 --------------------------------------------------------------------------------------------------------------
def match_problem(ious, det_areas, gt_areas, gt_ignore_in, not_exhaustive):
    """One (image, category): ious [D][G] of the detections in score order against the ground truths in annotation order ->
    (dt_match [A][T][D]: the matched ground truth's position or -1, dt_ignore [A][T][D], gt_ignore [A][G])."""
    num_d, num_g = len(det_areas), len(gt_areas)
    dt_match = np.full((len(AREA_RANGES), len(IOU_THRESHOLDS), num_d), -1, dtype=np.int32)
    dt_ignore = np.zeros((len(AREA_RANGES), len(IOU_THRESHOLDS), num_d), dtype=bool)
    gt_ignore = np.zeros((len(AREA_RANGES), num_g), dtype=bool)
    for a, (lo, hi) in enumerate(AREA_RANGES):
        ignore = [bool(gt_ignore_in[g]) or gt_areas[g] < lo or gt_areas[g] > hi for g in range(num_g)]
        gt_ignore[a] = ignore
        wanted = [g for g in range(num_g) if not ignore[g]]
        others = [g for g in range(num_g) if ignore[g]]
        for t, thr in enumerate(IOU_THRESHOLDS):
            floor = min(thr, 1 - 1e-10)
            taken = set()
            for d in range(num_d):
                choice = -1
                for group in (wanted, others):      # failing a non-ignored match, the same among the ignored ones
                    for g in group:
                        if g in taken or ious[d][g] < floor:
                            continue
                        if choice == -1 or ious[d][g] >= ious[d][choice]:   # an equal IoU goes to the later one
                            choice = g
                    if choice != -1:
                        break
                if choice == -1:
                    dt_ignore[a, t, d] = det_areas[d] < lo or det_areas[d] > hi or bool(not_exhaustive)
                    continue
                taken.add(choice)                   # never matched again, ignored or not
                dt_match[a, t, d] = choice
                dt_ignore[a, t, d] = ignore[choice]
    return dt_match, dt_ignore, gt_ignore


# ---- rule 5: the tables of every problem ------------------------------------------------------------------------------------------
def match_tables(data, dets, iou_type, max_dets=MAX_DETS):
    """``category`` [P] (index into the sorted category ids), ``det_start`` / ``gt_start`` [P + 1], ``scores`` [D],
    ``dt_match`` / ``dt_ignore`` [A, T, D], ``gt_ignore`` [A, G], plus ``not_exhaustive`` [P]: problems in image-id order."""
    check(data)
    cat_ids = sorted(c["id"] for c in data["categories"])
    kept = kept_detections(data, dets, max_dets)
    category, det_start, gt_start, scores, dtm, dtig, gtig, flags = [], [0], [0], [], [], [], [], []
    for image in sorted(data["images"], key=lambda im: im["id"]):
        anns = [a for a in data["annotations"] if a["image_id"] == image["id"]]
        for c in sorted({d["category_id"] for d in kept[image["id"]]} | {a["category_id"] for a in anns}):
            mine = [d for d in kept[image["id"]] if d["category_id"] == c]      # still by descending score, stably
            gts = [a for a in anns if a["category_id"] == c]
            ious = [[pair_iou(d, g, iou_type) for g in gts] for d in mine]
            flag = c in image["not_exhaustive_category_ids"]
            m, di, gi = match_problem(ious, [det_area(d, iou_type) for d in mine], [gt_area(g) for g in gts],
                                      [g.get("ignore", 0) for g in gts], flag)
            category.append(cat_ids.index(c))
            det_start.append(det_start[-1] + len(mine))
            gt_start.append(gt_start[-1] + len(gts))
            scores += [d["score"] for d in mine]
            dtm.append(m)
            dtig.append(di)
            gtig.append(gi)
            flags.append(flag)
    num_a, num_t = len(AREA_RANGES), len(IOU_THRESHOLDS)
    return {"category": np.asarray(category, dtype=np.int64), "det_start": np.asarray(det_start), "gt_start": np.asarray(gt_start),
            "scores": np.asarray(scores, dtype=np.float64), "not_exhaustive": np.asarray(flags, dtype=bool),
            "dt_match": np.concatenate(dtm + [np.zeros((num_a, num_t, 0), np.int32)], axis=2),
            "dt_ignore": np.concatenate(dtig + [np.zeros((num_a, num_t, 0), bool)], axis=2),
            "gt_ignore": np.concatenate(gtig + [np.zeros((num_a, 0), bool)], axis=1)}


# ---- rule 9 ---------------------------------------------------------------------------------------------------------------------
def accumulate(tables, num_categories):
    """-> (precision [T, R, K, A], recall [T, K, A]); -1 where a (category, area) has no non-ignored ground truth."""
    precision = -np.ones((len(IOU_THRESHOLDS), len(RECALL_THRESHOLDS), num_categories, len(AREA_RANGES)))
    recall = -np.ones((len(IOU_THRESHOLDS), num_categories, len(AREA_RANGES)))
    for k in range(num_categories):
        problems = [p for p in range(len(tables["category"])) if tables["category"][p] == k]
        for a in range(len(AREA_RANGES)):
            rows, num_gt = [], 0
            for p in problems:                       # image-id order
                rows += list(range(tables["det_start"][p], tables["det_start"][p + 1]))
                num_gt += sum(1 for g in range(tables["gt_start"][p], tables["gt_start"][p + 1]) if not tables["gt_ignore"][a][g])
            if num_gt == 0:
                continue
            rows = sorted(rows, key=lambda r: -tables["scores"][r])   # stable: equal scores keep image-id order
            for t in range(len(IOU_THRESHOLDS)):
                tp, fp, pr, rc = 0.0, 0.0, [], []
                for r in rows:
                    if tables["dt_ignore"][a][t][r]:
                        continue
                    if tables["dt_match"][a][t][r] >= 0:
                        tp += 1.0
                    else:
                        fp += 1.0
                    rc.append(tp / num_gt)
                    pr.append(tp / (tp + fp + np.spacing(1)))
                for i in range(len(pr) - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                q = np.zeros(len(RECALL_THRESHOLDS))
                for r, i in enumerate(np.searchsorted(rc, RECALL_THRESHOLDS, side="left")):
                    if i < len(pr):
                        q[r] = pr[i]
                precision[t, :, k, a] = q
                recall[t, k, a] = rc[-1] if rc else 0.0
    return precision, recall


# ---- rule 10 --------------------------------------------------------------------------------------------------------------------
def _mean(values):
    values = np.asarray(values)
    values = values[values > -1]
    return float(np.mean(values)) if values.size else -1.0


def summarize(precision, category_names, frequencies, class_splits, recall=None):
    t50, t75 = int(np.where(IOU_THRESHOLDS == .5)[0][0]), int(np.where(IOU_THRESHOLDS == .75)[0][0])
    out = OrderedDict()
    out["AP"] = _mean(precision[:, :, :, 0])
    out["AP50"] = _mean(precision[t50, :, :, 0])
    out["AP75"] = _mean(precision[t75, :, :, 0])
    out["APs"], out["APm"], out["APl"] = (_mean(precision[:, :, :, a]) for a in (1, 2, 3))
    for f in FREQUENCIES:
        out[f"AP{f}"] = _mean([precision[:, :, k, 0] for k in range(len(frequencies)) if frequencies[k] == f])
    for k, name in enumerate(category_names):
        out[f"AP50_class_{name}"] = _mean(precision[t50, :, k, 0])
    for split, cats in class_splits.items():
        out[f"AP50_split_{split}"] = _mean([precision[t50, :, k, 0] for k in cats])
    if recall is not None:
        for name, a in (("AR@300", 0), ("ARs@300", 1), ("ARm@300", 2), ("ARl@300", 3)):
            out[name] = _mean(recall[:, :, a])
        for split, cats in class_splits.items():
            out[f"AR@300_split_{split}"] = _mean([recall[:, k, 0] for k in cats])
    return out


def evaluate(data, dets, iou_type, class_splits=None, recall=False, max_dets=MAX_DETS):
    """``class_splits``: {split: [category indices]}."""
    cats = sorted(data["categories"], key=lambda c: c["id"])
    tables = match_tables(data, dets, iou_type, max_dets)
    precision, rec = accumulate(tables, len(cats))
    return summarize(precision, [c["name"] for c in cats], [c["frequency"] for c in cats], class_splits or {},
                     rec if recall else None)
