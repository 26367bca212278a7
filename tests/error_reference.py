"""TEST-ONLY: a plain-Python restatement of the error analysis of include/ovis_hip.h ("Error analysis": TIDE's decomposition
of AP50 into Cls, Loc, Both, Dupe, Bkg and Miss) -- image-level IoU, the base matching at (area all, IoU 0.5), types, missed
ground truths, the eight fixes and AP50, all from scratch in loops over detections and ground truths.  It imports nothing
from the product and not tests/coco_eval_reference.py either; tests/test_error_reference.py holds it to hand-computed cases
and to that restatement's AP50.

Inputs are those of tests/coco_eval_reference.py: ``images`` is a list, in image-id order, of ``{"dets": [...], "gts": [...]}``;
a detection is ``{"category": index, "score": float, "bbox": [x, y, w, h]}`` or, for segm, ``{"category", "score", "mask": bool
[H, W]}``, in prediction order; a ground truth ``{"category", "bbox" or "mask", "area", "iscrowd"}`` in annotation order.
"""
from collections import OrderedDict

import numpy as np

TYPES = ("none", "Cls", "Loc", "Both", "Dupe", "Bkg")  # the codes of err_type
MAIN = ("Cls", "Loc", "Both", "Dupe", "Bkg", "Miss")
RECALL_THRESHOLDS = np.linspace(0, 1, 101)
MAX_DETS = 100


def box_iou(d, g, crowd=False):
    dx, dy, dw, dh = (float(v) for v in d)
    gx, gy, gw, gh = (float(v) for v in g)
    iw = max(min(dx + dw, gx + gw) - max(dx, gx), 0.0)
    ih = max(min(dy + dh, gy + gh) - max(dy, gy), 0.0)
    inter = iw * ih
    union = dw * dh if crowd else dw * dh + gw * gh - inter
    return 0.0 if union == 0 else inter / union


def mask_iou(d, g, crowd=False):
    d, g = np.asarray(d, dtype=bool), np.asarray(g, dtype=bool)
    inter = int((d & g).sum())
    union = int(d.sum()) if crowd else int(d.sum()) + int(g.sum()) - inter
    return 0.0 if union == 0 else float(inter) / float(union)


def classify(ious, det_cat, det_match, det_ignore, gt_cat, gt_crowd, t_f=0.5, t_b=0.1):
    """TYPES and MISSED for one image.  ious [D][G]: every detection against every ground truth (only the entries against
    non-crowd ground truths are read); det_match [D]: the row of the ground truth the base matched, or -1; det_ignore [D].
    -> (type codes [D], targets [D]: a ground-truth row or -1, missed flags [G])."""
    types, targets = [], []
    for d in range(len(det_cat)):
        if det_match[d] >= 0 or det_ignore[d]:
            types.append(0)
            targets.append(-1)
            continue
        s, gs, o, go = 0.0, -1, 0.0, -1
        for g in range(len(gt_cat)):
            if gt_crowd[g]:
                continue
            v = ious[d][g]
            if gt_cat[g] == det_cat[d]:
                if gs < 0 or v >= s:   # an equal IoU goes to the later row
                    s, gs = v, g
            elif go < 0 or v >= o:
                o, go = v, g
        if t_b <= s < t_f:
            kind, target = "Loc", gs
        elif o >= t_f:
            kind, target = "Cls", go
        elif s >= t_f:
            kind, target = "Dupe", gs
        elif max(s, o) <= t_b:
            kind, target = "Bkg", -1
        else:
            kind, target = "Both", -1
        types.append(TYPES.index(kind))
        targets.append(target)
    missed = []
    for g in range(len(gt_cat)):
        held = bool(gt_crowd[g])
        for d in range(len(det_cat)):
            if det_match[d] == g or (types[d] in (TYPES.index("Cls"), TYPES.index("Loc")) and targets[d] == g):
                held = True
        missed.append(not held)
    return types, targets, missed


def base_match(ious, gt_crowd, thr=0.5):
    """COCOeval.evaluateImg at area "all" and one threshold for one (image, category): ious [D][G] (crowd form against
    crowds), detections in score order -> (match [D]: a ground-truth index or -1, ignore [D])."""
    num_g = len(gt_crowd)
    order = [g for g in range(num_g) if not gt_crowd[g]] + [g for g in range(num_g) if gt_crowd[g]]
    taken, match, ignore = [False] * num_g, [], []
    for row in ious:
        best, m = min(thr, 1 - 1e-10), -1
        for g in order:
            if taken[g] and not gt_crowd[g]:
                continue
            if m > -1 and not gt_crowd[m] and gt_crowd[g]:
                break
            if row[g] < best:
                continue
            best, m = row[g], g
        match.append(m)
        ignore.append(bool(gt_crowd[m]) if m > -1 else False)
        if m > -1:
            taken[m] = True
    return match, ignore


def rows(images, iou_type, t_f=0.5, t_b=0.1):
    """The flat detection and ground-truth rows of the whole input, in the scorer's order -- images in order; inside an image
    the detections by (category, descending score, stably), at most 100 per category, the ground truths by category, stably
    -- with the base matching and the error types.  -> dict of lists: det_cat, det_score, det_image, det_match (global
    ground-truth row or -1), det_ignore, err_type, err_gt (global row or -1); gt_cat, gt_crowd, gt_image, gt_missed."""
    key = "bbox" if iou_type == "bbox" else "mask"
    iou = box_iou if iou_type == "bbox" else mask_iou
    out = {k: [] for k in ("det_cat", "det_score", "det_image", "det_match", "det_ignore", "err_type", "err_gt", "gt_cat",
                           "gt_crowd", "gt_image", "gt_missed")}
    for index, image in enumerate(images):
        cats = sorted({d["category"] for d in image["dets"]} | {g["category"] for g in image["gts"]})
        dets, gts = [], []
        for c in cats:
            of_c = [d for d in image["dets"] if d["category"] == c]
            dets += [of_c[i] for i in np.argsort([-d["score"] for d in of_c], kind="mergesort")][:MAX_DETS]
            gts += [g for g in image["gts"] if g["category"] == c]
        match, ignore = [-1] * len(dets), [False] * len(dets)
        for c in cats:
            d_rows = [i for i, d in enumerate(dets) if d["category"] == c]
            g_rows = [j for j, g in enumerate(gts) if g["category"] == c]
            m, ig = base_match([[iou(dets[i][key], gts[j][key], gts[j]["iscrowd"]) for j in g_rows] for i in d_rows],
                               [gts[j]["iscrowd"] for j in g_rows])
            for i, mm, ii in zip(d_rows, m, ig):
                match[i], ignore[i] = (g_rows[mm] if mm > -1 else -1), ii
        ious = [[iou(d[key], g[key]) for g in gts] for d in dets]
        types, targets, missed = classify(ious, [d["category"] for d in dets], match, ignore, [g["category"] for g in gts],
                                          [g["iscrowd"] for g in gts], t_f, t_b)
        base = len(out["gt_cat"])
        out["det_cat"] += [d["category"] for d in dets]
        out["det_score"] += [float(d["score"]) for d in dets]
        out["det_image"] += [index] * len(dets)
        out["det_match"] += [m + base if m > -1 else -1 for m in match]
        out["det_ignore"] += ignore
        out["err_type"] += types
        out["err_gt"] += [t + base if t > -1 else -1 for t in targets]
        out["gt_cat"] += [g["category"] for g in gts]
        out["gt_crowd"] += [bool(g["iscrowd"]) for g in gts]
        out["gt_image"] += [index] * len(gts)
        out["gt_missed"] += missed
    return out


def ap50_columns(entries, num_gt):
    """entries: [(category, score, row, is true positive)] of the detections that count; num_gt [K]: the ground truths left
    per category -> precision [R, K] at the 101 recall samples, -1 for a category without ground truth."""
    columns = -np.ones((len(RECALL_THRESHOLDS), len(num_gt)))
    for k in range(len(num_gt)):
        if num_gt[k] <= 0:
            continue
        mine = sorted([e for e in entries if e[0] == k], key=lambda e: (-e[1], e[2]))
        tp, fp, pr, rc = 0.0, 0.0, [], []
        for _, _, _, hit in mine:
            tp += 1.0 if hit else 0.0
            fp += 0.0 if hit else 1.0
            rc.append(tp / num_gt[k])
            pr.append(tp / (fp + tp + np.spacing(1)))
        for i in range(len(pr) - 1, 0, -1):
            if pr[i] > pr[i - 1]:
                pr[i - 1] = pr[i]
        for r, thr in enumerate(RECALL_THRESHOLDS):
            i = 0
            while i < len(rc) and rc[i] < thr:
                i += 1
            columns[r, k] = pr[i] if i < len(pr) else 0.0
    return columns


def _mean(values):
    values = values[values > -1]
    return float(np.mean(values)) if values.size else -1.0


def analyze(images, iou_type, num_categories, class_splits, t_f=0.5, t_b=0.1):
    """The whole analysis -> OrderedDict with the keys of ``engine.error_analysis.analyze_tables``."""
    r = rows(images, iou_type, t_f, t_b)
    num_d, num_g = len(r["det_cat"]), len(r["gt_cat"])
    taken = [False] * num_g
    for d in range(num_d):
        if r["det_match"][d] > -1:
            taken[r["det_match"][d]] = True

    def table(fix):
        """(entries, ground truths per category) after ``fix`` (None: the base)."""
        num_gt = [0] * num_categories
        for g in range(num_g):
            if r["gt_crowd"][g] or (fix == "Miss" and r["gt_missed"][g]) or (fix == "FalseNeg" and not taken[g]):
                continue
            num_gt[r["gt_cat"][g]] += 1
        claimed, winners = set(), {}
        if fix in ("Loc", "Cls"):   # the highest score claims a free target, ties to the earlier row
            fixed = [d for d in range(num_d) if TYPES[r["err_type"][d]] == fix]
            for d in sorted(fixed, key=lambda d: (-r["det_score"][d], d)):
                g = r["err_gt"][d]
                if g > -1 and not taken[g] and g not in claimed:
                    claimed.add(g)
                    winners[d] = g
        entries = []
        for d in range(num_d):
            if r["det_ignore"][d]:
                continue   # neither a true nor a false positive
            hit, cat, kind = r["det_match"][d] > -1, r["det_cat"][d], TYPES[r["err_type"][d]]
            if fix in ("Dupe", "Bkg", "Both") and kind == fix:
                continue
            if fix == "FalsePos" and not hit:
                continue
            if fix in ("Loc", "Cls") and kind == fix:
                if d not in winners:
                    continue
                hit = True
                if fix == "Cls":
                    cat = r["gt_cat"][winners[d]]
            entries.append((cat, r["det_score"][d], d, hit))
        return entries, num_gt

    def means(fix):
        columns = ap50_columns(*table(fix))
        return [_mean(columns)] + [_mean(columns[:, list(cats)]) for cats in class_splits.values()]

    base = means(None)
    res = OrderedDict(AP50=base[0])
    for split, value in zip(class_splits, base[1:]):
        res[f"AP50_split_{split}"] = value
    for fix in MAIN + ("FalsePos", "FalseNeg"):
        after = means(fix)
        gains = [-1.0 if a == -1 or b == -1 else a - b for a, b in zip(after, base)]
        res[f"dAP50_{fix}"] = gains[0]
        if fix in MAIN:
            for split, gain in zip(class_splits, gains[1:]):
                res[f"dAP50_{fix}_split_{split}"] = gain
    groups = OrderedDict([("all", list(range(num_categories)))] + [(s, list(c)) for s, c in class_splits.items()])
    res["counts"] = OrderedDict()
    for group, cats in groups.items():
        res["counts"][group] = OrderedDict((name, sum(1 for d in range(num_d) if TYPES[r["err_type"][d]] == name and r["det_cat"][d] in cats))
                                           for name in MAIN[:-1])
        res["counts"][group]["Miss"] = sum(1 for g in range(num_g) if r["gt_missed"][g] and r["gt_cat"][g] in cats)
    res["cls_confusion_by_split"] = OrderedDict(
        (gs, OrderedDict((ds, sum(1 for d in range(num_d) if TYPES[r["err_type"][d]] == "Cls"
                                  and r["gt_cat"][r["err_gt"][d]] in class_splits[gs] and r["det_cat"][d] in class_splits[ds])) for ds in class_splits))
        for gs in class_splits)
    return res
