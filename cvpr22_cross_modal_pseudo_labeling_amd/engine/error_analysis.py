"""Why an AP50 is low: the error decomposition of TIDE (Bolya et al., "TIDE: A General Toolbox for Identifying Object
Detection Errors", ECCV 2020) on the scorer's own match tables.  Every false positive of the matching at (area all, IoU 0.5)
is one of Cls, Loc, Both, Dupe, Bkg, every unmatched ground truth that is no target of a Loc or Cls error is Miss, and
``dAP50_<T>`` is what AP50 would gain if the errors of type T alone were fixed.  tidecv is not a dependency: the rules are
restated in include/ovis_hip.h ("Error analysis"), the numbers follow THAT text and have not been compared with tidecv's
output.  COCO rules only, bbox and segm only.

* on the DEVICE, inside ``coco_eval.score_chunk(error_thresholds=(t_f, t_b))``: one more IoU call over a table with one row
  per image -- every detection of an image against every ground truth of it, other categories included, from the box rows or
  the packed mask words the chunk already holds; nothing is pasted, rasterised, decoded or packed again -- and
  ``_C.error_types`` (csrc/error_types.hip), which types every detection and flags the missed ground truths.  Three more
  flat arrays come back beside the match tables.
* on the HOST, here, in NumPy over those flat arrays: the eight fixes and the AP50 of every fixed table (``analyze_tables``),
  O(detections) each, as ``coco_tables.accumulate`` is -- whose ``_sampled_precision`` makes every precision column, so the base
  AP50 is ``evaluate_coco``'s own, bit for bit, overall and per split.

In a category the order of equal scores is the order of the detection rows (image id, category index, descending score); a
detection the Cls fix moves keeps its row, and the 100 per (image, category) are not re-applied to the category it moves to.
"""
from collections import OrderedDict

import numpy as np
import torch

from . import coco_eval
from .. import _C
from .coco_tables import RECALL_THRESHOLDS, _mean, _sampled_precision

ERROR_TYPES = _C.ERROR_TYPES[1:]  # Cls, Loc, Both, Dupe, Bkg: err_type 1 .. 5
MAIN_TYPES = ERROR_TYPES + ("Miss",)
SPECIAL_FIXES = ("FalsePos", "FalseNeg")
FG_THRESHOLD, BG_THRESHOLD = 0.5, 0.1


def _precision_columns(det_cat, scores, tp, fp, alive, npig):
    """fp64 [1, R, K]: the precision of every category at the 101 recall samples (area all, IoU 0.5) -- -1 where ``npig[k]``
    (the category's non-ignored ground truths) is 0 -- from the detections ``alive`` keeps: ``tp`` / ``fp`` bool [D] (an
    ignored detection is neither), merged per category by descending score, stably in row order."""
    columns = -np.ones((1, len(RECALL_THRESHOLDS), len(npig)))
    rows = np.flatnonzero(alive)
    rows = rows[np.lexsort((-scores[rows], det_cat[rows]))]  # stable: equal scores of a category stay in row order
    cuts = np.searchsorted(det_cat[rows], np.arange(len(npig) + 1))
    for k in np.flatnonzero(npig > 0):
        sel = rows[cuts[k]:cuts[k + 1]]
        columns[0, :, k] = _sampled_precision(np.cumsum(tp[sel]).astype(np.float64), np.cumsum(fp[sel]).astype(np.float64),
                                              npig[k])
    return columns


def _claims(fixed, target, scores, free):
    """Of the detection rows ``fixed`` (ascending), those that become true positives of their ``target`` ground truth: the
    target is ``free`` and the row has the highest score among the fixed rows of that target, ties to the earlier row."""
    fixed = fixed[target[fixed] >= 0]
    order = fixed[np.lexsort((fixed, -scores[fixed], target[fixed]))]
    first = np.ones(len(order), dtype=bool)
    first[1:] = target[order[1:]] != target[order[:-1]]
    return order[first & free[target[order]]]


def analyze_tables(tables, num_categories, class_splits):
    """The analysis of one iou type from match tables scored with ``error_thresholds`` (the structure: engine/coco_tables.py)
    -> OrderedDict: ``AP50`` and ``AP50_split_<split>`` (the base), ``dAP50_<T>`` for Cls, Loc, Both, Dupe, Bkg, Miss, FalsePos,
    FalseNeg, ``dAP50_<T>_split_<split>`` for the first six, ``counts`` {"all" or split: {T: errors}} (by the detection's
    category; Miss by the ground truth's) and ``cls_confusion_by_split`` {split of the target ground truth: {split of the
    detection: Cls errors}}.  ``class_splits``: {split: [category indices]}."""
    if "err_type" not in tables:
        if len(tables["det_start"]) > 1 or tables["det_start"][-1] or tables["gt_start"][-1]:
            raise ValueError("analyze_tables: match tables without err_type: score them with error_thresholds=(t_f, t_b)")
        tables = dict(tables, err_type=np.zeros(0, np.uint8), err_gt=np.zeros(0, np.int32), gt_missed=np.zeros(0, np.uint8))
    cat = np.asarray(tables["category"], dtype=np.int64)
    det_start, gt_start = np.asarray(tables["det_start"], dtype=np.int64), np.asarray(tables["gt_start"], dtype=np.int64)
    scores = np.asarray(tables["scores"], dtype=np.float64)
    det_cat, gt_cat = np.repeat(cat, np.diff(det_start)), np.repeat(cat, np.diff(gt_start))
    local = np.asarray(tables["dt_match"])[0, 0].astype(np.int64)
    matched, ignored = local >= 0, np.asarray(tables["dt_ignore"], dtype=bool)[0, 0]
    crowd = np.asarray(tables["gt_ignore"], dtype=bool)[0]  # area "all": a ground truth is ignored iff it is a crowd
    det_gt = np.where(matched, local + np.repeat(gt_start[:-1], np.diff(det_start)), -1)  # the matched ground truth's row
    err_type, err_gt = np.asarray(tables["err_type"]), np.asarray(tables["err_gt"], dtype=np.int64)
    missed = np.asarray(tables["gt_missed"], dtype=bool)
    tp, fp = matched & ~ignored, ~matched & ~ignored
    taken = np.zeros(len(gt_cat), dtype=bool)
    taken[det_gt[matched]] = True
    npig = np.bincount(gt_cat[~crowd], minlength=num_categories)
    alive = np.ones(len(det_cat), dtype=bool)

    def fixed_columns(name):
        if name in ("Dupe", "Bkg", "Both"):
            return _precision_columns(det_cat, scores, tp, fp, alive & (err_type != _C.ERROR_TYPES.index(name)), npig)
        if name in ("Loc", "Cls"):
            fixed = np.flatnonzero(err_type == _C.ERROR_TYPES.index(name))
            won = _claims(fixed, err_gt, scores, ~taken)
            keep, new_tp, new_cat = alive.copy(), tp.copy(), det_cat.copy()
            keep[fixed] = False
            keep[won], new_tp[won] = True, True
            if name == "Cls":
                new_cat[won] = gt_cat[err_gt[won]]
            return _precision_columns(new_cat, scores, new_tp, fp & ~new_tp, keep, npig)
        if name == "Miss":
            return _precision_columns(det_cat, scores, tp, fp, alive, npig - np.bincount(gt_cat[missed], minlength=num_categories))
        if name == "FalsePos":
            return _precision_columns(det_cat, scores, tp, fp, alive & ~fp, npig)
        return _precision_columns(det_cat, scores, tp, fp, alive, np.bincount(gt_cat[taken & ~crowd], minlength=num_categories))

    def means(columns):
        return [_mean(columns)] + [_mean(columns[:, :, list(cats)]) for cats in class_splits.values()]

    base = means(_precision_columns(det_cat, scores, tp, fp, alive, npig))
    res = OrderedDict(AP50=base[0])
    for split, value in zip(class_splits, base[1:]):
        res[f"AP50_split_{split}"] = value
    for name in MAIN_TYPES + SPECIAL_FIXES:
        after = means(fixed_columns(name))
        gains = [-1.0 if a == -1 or b == -1 else a - b for a, b in zip(after, base)]
        res[f"dAP50_{name}"] = gains[0]
        if name in MAIN_TYPES:
            for split, gain in zip(class_splits, gains[1:]):
                res[f"dAP50_{name}_split_{split}"] = gain

    members = OrderedDict([("all", np.ones(num_categories, dtype=bool))])
    for split, cats in class_splits.items():
        members[split] = np.zeros(num_categories, dtype=bool)
        members[split][list(cats)] = True
    res["counts"] = OrderedDict(
        (group, OrderedDict([(name, int(np.count_nonzero((err_type == code + 1) & inside[det_cat])))
                             for code, name in enumerate(ERROR_TYPES)] + [("Miss", int(np.count_nonzero(missed & inside[gt_cat])))]))
        for group, inside in members.items())
    cls = np.flatnonzero(err_type == _C.ERROR_TYPES.index("Cls"))
    res["cls_confusion_by_split"] = OrderedDict(
        (gt_split, OrderedDict((det_split, int(np.count_nonzero(members[gt_split][gt_cat[err_gt[cls]]] & members[det_split][det_cat[cls]])))
                               for det_split in class_splits))
        for gt_split in class_splits)
    return res


def analyze_scored(dataset, tables_by_type, cat_ids):
    """``analyze_tables`` of every bbox / segm entry of {iou_type: tables}, with the dataset's class splits."""
    cat_index = {c: i for i, c in enumerate(cat_ids)}
    splits = OrderedDict((split, [cat_index[c] for c in ids]) for split, ids in dataset.class_splits.items())
    return OrderedDict((t, analyze_tables(tables, len(cat_ids), splits)) for t, tables in tables_by_type.items()
                       if t in ("bbox", "segm"))


def _check(iou_types, fg_threshold, bg_threshold, who):
    for t in iou_types:
        if t not in ("bbox", "segm"):
            raise ValueError(f"{who}: iou_type '{t}' is not analysed (bbox, segm)")
    if not 0.0 <= bg_threshold <= fg_threshold <= 1.0:
        raise ValueError(f"{who}: thresholds 0 <= bg_threshold <= fg_threshold <= 1 expected, got {bg_threshold}, {fg_threshold}")
    return float(fg_threshold), float(bg_threshold)


def _analyze(who, match_tables, dataset, detections, iou_types, device, fg_threshold, bg_threshold, max_images):
    """What ``analyze_errors`` and ``analyze_errors_results`` share.  ``match_tables``: ``coco_eval``'s entry for their kind of
    detections; ``detections``: {iou_type: what it scores} -- a requested iou_type it does not have is checked and skipped."""
    device = coco_eval._scoring_device(device, who)
    thresholds = _check(iou_types, fg_threshold, bg_threshold, who)
    ground_truth = coco_eval._ground_truth(dataset)
    with torch.cuda.device(device):
        scored = OrderedDict((t, match_tables(dataset, detections[t], t, device, ground_truth=ground_truth,
                                              max_images=max_images, error_thresholds=thresholds)[0])
                             for t in iou_types if t in detections)
    return analyze_scored(dataset, scored, ground_truth[0])


def analyze_errors(dataset, predictions, iou_types=("bbox", "segm"), device="cuda", fg_threshold=FG_THRESHOLD,
                   bg_threshold=BG_THRESHOLD, max_images=None):
    """{iou_type: ``analyze_tables``' numbers} for ``predictions`` (what ``evaluate_coco`` takes): the base ``AP50`` and
    ``AP50_split_<split>`` are ``evaluate_coco``'s, bit for bit.  ``fg_threshold`` / ``bg_threshold``: t_f and t_b of the rules
    in include/ovis_hip.h; ``max_images``: the most images of a chunk (``match_tables``).  Scores on the HIP device."""
    return _analyze("analyze_errors", coco_eval.match_tables, dataset, dict.fromkeys(iou_types, predictions), iou_types, device,
                    fg_threshold, bg_threshold, max_images)


def analyze_errors_results(dataset, results, iou_types=("bbox", "segm"), device="cuda", fg_threshold=FG_THRESHOLD,
                           bg_threshold=BG_THRESHOLD, max_images=None):
    """``analyze_errors`` for detections from COCO results files: ``results`` is {iou_type: a path or the parsed list}
    (``coco_eval.load_coco_results``); an iou_type it does not have is skipped."""
    return _analyze("analyze_errors_results", coco_eval.results_match_tables, dataset, results, iou_types, device,
                    fg_threshold, bg_threshold, max_images)


def task_tables(analysis):
    """{"errors_<iou_type>": the analysis' numbers without the nested counts}: what ``coco_eval.format_results`` prints as
    the ``errors_bbox`` / ``errors_segm`` tasks behind the scoring tables."""
    return OrderedDict((f"errors_{t}", OrderedDict((k, v) for k, v in numbers.items() if not isinstance(v, dict)))
                       for t, numbers in analysis.items())
