"""COCO box / mask AP and the seen / unseen AP50 of a prediction list -- the dataset-specific ``evaluate`` the reference
runs after ``inference`` (maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py: ``prepare_for_coco_detection``
:71-105, ``prepare_for_coco_segmentation`` :108-162, ``evaluate_predictions_on_coco`` :315-333, ``COCOResults`` :336-414).

The reference hands JSON results to pycocotools' ``COCOeval``; pycocotools is not a dependency here, its rules are restated:

* on the DEVICE (csrc/coco_eval.hip through ``_C``), a chunk of images at a time: the detections' masks are pasted at
  image size (``_C.paste_masks``) and the polygon ground truth rasterised (``_C.polygons_to_masks``) per image size,
  packed to bit words, and then three launches cover the whole chunk -- box IoU or mask IoU of every (image, category)
  problem, and ``COCOeval.evaluateImg``'s matching for every problem, area range and IoU threshold.  Only the match tables
  come back: 4 x 10 x (an int32 and a flag) per detection.
* on the HOST, in NumPy fp64: ``COCOeval.accumulate`` and ``summarize`` (``accumulate`` / ``summarize`` below), term by
  term -- O(detections), not hot.

Chunks are sized by device memory: an image costs (detections + ground truths) x height x width x 9 / 8 bytes (the pasted
byte masks and their packed words; box scoring costs nothing worth counting), and a chunk takes images in id order until
a quarter of the memory free at the start is used, or ``MAX_CHUNK_IMAGES``, or until its detections, its ground truths or
its polygons would exceed ``MAX_CALL_MASKS`` -- the most one ``paste_masks`` / ``polygons_to_masks`` call takes, so the
per-size calls of a chunk stay inside their callees' limits even when every image has the same size.

Detections also come from COCO RESULTS FILES (``evaluate_coco_results``: the ``bbox.json`` / ``segm.json`` of
engine/coco_results.py, of the reference or of any other tool): ``load_coco_results`` is pycocotools' ``loadRes`` plus the
per-category cap, and a ``segm`` row carries its RLE instead of a map and a box.  RLE masks -- those detections and RLE
ground truth alike -- never become byte masks: ``_C.coco_rle_words`` (csrc/coco_rle_decode.hip) decodes all of an image-size
group in one call straight to the packed words, and reports a malformed encoding as a status that is raised here.

Semantics beyond pycocotools' own: images and categories are all those of the annotation file, sorted by id; an image
without a prediction counts with zero detections; every annotation is ground truth, crowds included (``ignore =
iscrowd``); a ground truth's ``area`` is the annotation's ``area`` when present, else its box's w * h; an IoU whose union
is 0 is 0 (pycocotools yields NaN for two zero-area boxes; clipped detections have w, h >= 1).

RECALL.  ``recall=True`` adds ``COCOeval.summarize``'s six AR numbers and AR100_split_<split> (``accumulate_recall`` /
``summarize_recall``): host arithmetic over the SAME match tables, no further device work -- the matching walks a problem's
detections in score order, so the first k columns of the maxDets = 100 tables are the maxDets = k matching, which is how
pycocotools itself slices them.  The ``box_proposal`` task of the reference's table is a different, class-agnostic matching
with a kernel of its own: engine/proposal_recall.py.  Keypoints are not scored.

BOUNDARY AP.  A third ``iou_type``, ``"boundary"`` (Cheng et al., "Boundary IoU", CVPR 2021): segm's matching on min(mask IoU,
boundary IoU), where a mask's boundary is what d = max(1, round(0.02 x diagonal)) iterations of a 3x3 erosion take away.
boundary-iou-api is not a dependency either; the rule is restated in include/ovis_hip.h and the numbers follow THAT text --
they have not been compared with boundary-iou-api's output.  It works on the words segm already has: per image size one
``_C.coco_boundary_words`` call for the detections and one for the ground truths (csrc/coco_boundary.hip), then
``_C.coco_boundary_iou`` fills the IoU buffer the matching reads; a chunk plans 11 / 8 byte per pixel and mask instead of
9 / 8 (the boundary words and the erosion's scratch).  Asked for together, segm and boundary share one paste / rasterise /
decode / pack per chunk, and segm's tables are those of a run without boundary, bit for bit.

LVIS.  ``rules="lvis"`` (default ``"coco"``: nothing changes) scores an annotation file that is only FEDERATEDLY annotated -- its
images carry ``neg_category_ids`` and ``not_exhaustive_category_ids``, its categories ``frequency`` -- by the ten rules restated in
include/ovis_hip.h (lvis-api is not a dependency; the numbers follow THAT text and have not been compared with lvis-api's own
output): the image's 300 best detections over all categories instead of 100 per category, detections of categories nobody
looked for in the image dropped (``_kept_rows``), ``ignore`` keys instead of crowds, a matching that never re-matches a ground
truth and ignores the unmatched detections of not-exhaustive categories (``_C.lvis_match``, csrc/lvis_eval.hip), no maxDets
dimension (``accumulate_lvis``) and APr / APc / APf beside the COCO keys (``summarize_lvis``).  Every iou_type takes the
keyword, boundary included; everything image-sized is shared with COCO scoring.

ERROR ANALYSIS.  ``error_thresholds=(t_f, t_b)`` (default None: nothing changes) on ``score_chunk``, ``match_tables``,
``results_match_tables``, ``evaluate_coco`` and ``evaluate_coco_results`` adds, for bbox and segm under ``rules="coco"``, one IoU
call on a table with one row per image and ``_C.error_types`` (csrc/error_types.hip); the tables then carry ``err_type``,
``err_gt``, ``gt_missed`` and the rows' images, which engine/error_analysis.py turns into dAP50 per error type.

SHARDED.  ``evaluate_coco_sharded`` is ``evaluate_coco`` for a caller that holds one rank's {dataset index: BoxList} instead of
the gathered list (a training run's periodic evaluation, engine/evaluation.py): an image's matching does not depend on any
other image, so every rank scores the images it predicted on its own device and only the match tables go to rank 0, where
``merge_shard_tables`` puts the whole-image blocks into image-id order -- the tables ``match_tables`` gives, array for array.
"""
import contextlib
import json
import math
import os
from collections import OrderedDict

import numpy as np
import torch
import torch.distributed as dist

from . import comm
from .. import _C
from ..modeling.structures import BoxList, PolygonMasks

IOU_THRESHOLDS = np.linspace(.5, .95, 10)
RECALL_THRESHOLDS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RANGES = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], dtype=np.float64)  # all, s, m, l
METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl")
MAX_CHUNK_IMAGES = 4096
MAX_CALL_MASKS = 65535  # what one paste_masks / polygons_to_masks call takes: masks, instances or polygons
# the masks of one pasted_masks_rle call of the results export (engine/coco_results.py): inside MAX_CALL_MASKS, and small
# enough that a chunk's maps (25 MB at M = 28) and runs (a few hundred int32 per mask) are no burden on the device
MAX_EXPORT_MASKS = 8192
IOU_TYPES = ("bbox", "segm", "boundary")
MASK_IOU_TYPES = ("segm", "boundary")  # scored from the packed mask words: one pass over a chunk serves both
BOUNDARY_DILATION_RATIO = 0.02
RULES = ("coco", "lvis")  # lvis: LVIS-style federated scoring, the ten rules of include/ovis_hip.h
LVIS_MAX_DETS = 300  # per image, over all categories together (rule 3)
LVIS_METRICS = METRICS + ("APr", "APc", "APf")
LVIS_FREQUENCIES = ("r", "c", "f")
LVIS_RECALL_METRICS = ("AR@300", "ARs@300", "ARm@300", "ARl@300")


def _check_rules(rules, who):
    if rules not in RULES:
        raise ValueError(f"{who}: rules '{rules}' is not supported ({', '.join(RULES)})")


def _check_iou_type(iou_type, who):
    if iou_type not in IOU_TYPES:
        raise ValueError(f"{who}: iou_type '{iou_type}' is not supported ({', '.join(IOU_TYPES)})")


def boundary_dilation(height, width, ratio=BOUNDARY_DILATION_RATIO):
    """The erosion depth d of Boundary IoU for a ``height`` x ``width`` image, rule 1 of include/ovis_hip.h: ``ratio`` of
    the diagonal, rounded half to even (Python 3's ``round``), at least 1.  Host arithmetic; the device gets the integer."""
    return max(1, int(round(ratio * math.sqrt(height * height + width * width))))


def _jobs(iou_types):
    """The scoring passes ``iou_types`` take, in order of first appearance: each a name, or -- when both are asked for --
    the tuple ("segm", "boundary"), which one pass over the chunks' mask words serves."""
    both = all(t in iou_types for t in MASK_IOU_TYPES)
    jobs = []
    for t in iou_types:
        job = MASK_IOU_TYPES if both and t in MASK_IOU_TYPES else t
        if job not in jobs:
            jobs.append(job)
    return jobs


# ---- host: COCOeval.accumulate / summarize --------------------------------------------------------------------------------
def accumulate(tables, num_categories):
    """``COCOeval.accumulate`` -> precision fp64 [T, R, K, A, M] (-1: no image entry or no non-ignored ground truth).

    ``tables``: the match tables of every problem -- (image, category) with a detection or a ground truth -- in image-id
    order, as plain NumPy arrays: ``category`` int [P] (index into the sorted category ids), ``det_start`` int [P + 1] and
    ``gt_start`` int [P + 1] (row ranges), ``scores`` f64 [D] (descending and at most 100 inside a problem), ``dt_match``
    int [A, T, D] (>= 0: matched), ``dt_ignore`` bool [A, T, D], ``gt_ignore`` bool [A, G]."""
    cat = np.asarray(tables["category"], dtype=np.int64)
    det_start, gt_start = np.asarray(tables["det_start"], dtype=np.int64), np.asarray(tables["gt_start"], dtype=np.int64)
    scores_all = np.asarray(tables["scores"], dtype=np.float64)
    matched_all, dt_ignore_all = np.asarray(tables["dt_match"]) >= 0, np.asarray(tables["dt_ignore"], dtype=bool)
    gt_ignore_all = np.asarray(tables["gt_ignore"], dtype=bool)
    det_problem = np.repeat(np.arange(len(cat)), np.diff(det_start))
    det_rank = np.arange(len(det_problem)) - det_start[:-1][det_problem]
    det_cat, gt_cat = cat[det_problem], np.repeat(cat, np.diff(gt_start))
    num_t, num_r, num_a, num_m = len(IOU_THRESHOLDS), len(RECALL_THRESHOLDS), len(AREA_RANGES), len(MAX_DETS)
    precision = -np.ones((num_t, num_r, num_categories, num_a, num_m))
    for k in range(num_categories):
        if not np.any(cat == k):
            continue
        dets_k, gts_k = np.nonzero(det_cat == k)[0], gt_cat == k
        for a in range(num_a):
            npig = np.count_nonzero(~gt_ignore_all[a][gts_k])
            if npig == 0:
                continue
            for m, max_det in enumerate(MAX_DETS):
                sel = dets_k[det_rank[dets_k] < max_det]
                # a stable sort: equal scores stay in image order
                sel = sel[np.argsort(-scores_all[sel], kind="mergesort")]
                dtm, dt_ig = matched_all[a][:, sel], dt_ignore_all[a][:, sel]
                tp_sum = np.cumsum(np.logical_and(dtm, np.logical_not(dt_ig)), axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig)), axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    precision[t, :, k, a, m] = _sampled_precision(tp, fp, npig)
    return precision


def _sampled_precision(tp, fp, npig):
    """The precision at the 101 recall thresholds, from the running tp / fp sums (fp64 [n]) of one category, area range and
    IoU threshold over its score-ordered non-ignored detections and its ``npig`` non-ignored ground truths."""
    nd = len(tp)
    rc = tp / npig
    pr = tp / (fp + tp + np.spacing(1))
    q = np.zeros((len(RECALL_THRESHOLDS),))
    if nd:  # the right-to-left envelope: pr[i - 1] = max(pr[i - 1], pr[i])
        pr = np.maximum.accumulate(pr[::-1])[::-1]
    inds = np.searchsorted(rc, RECALL_THRESHOLDS, side="left")
    ok = inds < nd  # a recall point past the last detection keeps precision 0
    q[ok] = pr[inds[ok]]
    return q


def _mean(s):
    s = s[s > -1]
    return float(np.mean(s)) if s.size else -1.0


def summarize(precision, category_names, class_splits, class_order=None):
    """``COCOeval.summarize``'s six AP numbers and ``COCOResults.update``'s per-class / per-split AP50 (coco_eval.py:364-404)
    -> OrderedDict.  category_names: the name of every category index; class_splits: {split: [category indices]};
    class_order: the category indices in the order their ``AP50_class_`` keys appear (None: index order)."""
    m100 = MAX_DETS.index(100)
    t50, t75 = np.where(.5 == IOU_THRESHOLDS)[0], np.where(.75 == IOU_THRESHOLDS)[0]
    res = OrderedDict()
    res["AP"] = _mean(precision[:, :, :, 0, m100])
    res["AP50"] = _mean(precision[t50][:, :, :, 0, m100])
    res["AP75"] = _mean(precision[t75][:, :, :, 0, m100])
    for name, a in (("APs", 1), ("APm", 2), ("APl", 3)):
        res[name] = _mean(precision[:, :, :, a, m100])
    s = precision[t50][:, :, :, 0, m100]  # [1, R, K]
    for k in range(len(category_names)) if class_order is None else class_order:
        res[f"AP50_class_{category_names[k]}"] = _mean(s[:, :, [k]])
    for split, cats in class_splits.items():
        res[f"AP50_split_{split}"] = _mean(s[:, :, list(cats)])
    return res


RECALL_METRICS = ("AR1", "AR10", "AR100", "ARs", "ARm", "ARl")


def accumulate_recall(tables, num_categories):
    """The ``recall`` array of ``COCOeval.accumulate`` -> fp64 [T, K, A, M] from the match tables ``accumulate`` takes: -1
    where the category has no problem or no non-ignored ground truth in the area range, 0 where it has no detection, else
    tp / npig after the last of the first ``maxDet`` detections of every image.  ``match_kernel`` walks a problem's
    detections in score order, each choosing among what the earlier ones left, so the first k columns of the maxDets = 100
    tables ARE the maxDets = k matching -- pycocotools slices ``dtMatches[:, 0:maxDet]`` in the same way."""
    cat = np.asarray(tables["category"], dtype=np.int64)
    det_start, gt_start = np.asarray(tables["det_start"], dtype=np.int64), np.asarray(tables["gt_start"], dtype=np.int64)
    matched_all, dt_ignore_all = np.asarray(tables["dt_match"]) >= 0, np.asarray(tables["dt_ignore"], dtype=bool)
    gt_ignore_all = np.asarray(tables["gt_ignore"], dtype=bool)
    det_problem = np.repeat(np.arange(len(cat)), np.diff(det_start))
    det_rank = np.arange(len(det_problem)) - det_start[:-1][det_problem]
    det_cat, gt_cat = cat[det_problem], np.repeat(cat, np.diff(gt_start))
    num_t, num_a, num_m = len(IOU_THRESHOLDS), len(AREA_RANGES), len(MAX_DETS)
    recall = -np.ones((num_t, num_categories, num_a, num_m))
    for k in range(num_categories):
        if not np.any(cat == k):
            continue
        dets_k, gts_k = np.nonzero(det_cat == k)[0], gt_cat == k
        for a in range(num_a):
            npig = np.count_nonzero(~gt_ignore_all[a][gts_k])
            if npig == 0:
                continue
            for m, max_det in enumerate(MAX_DETS):
                sel = dets_k[det_rank[dets_k] < max_det]
                # the last entry of a running sum: the order of the detections does not matter
                tps = np.logical_and(matched_all[a][:, sel], np.logical_not(dt_ignore_all[a][:, sel]))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                for t, tp in enumerate(tp_sum):
                    recall[t, k, a, m] = (tp / npig)[-1] if len(tp) else 0
    return recall


def summarize_recall(recall, category_names, class_splits):
    """``COCOeval.summarize``'s six AR numbers -- AR1, AR10, AR100 (all areas), ARs, ARm, ARl (maxDets = 100), each the
    mean of the entries > -1 -- and AR100_split_<split> over the categories of every split -> OrderedDict."""
    m100 = MAX_DETS.index(100)
    res = OrderedDict()
    for name, m in (("AR1", MAX_DETS.index(1)), ("AR10", MAX_DETS.index(10)), ("AR100", m100)):
        res[name] = _mean(recall[:, :, 0, m])
    for name, a in (("ARs", 1), ("ARm", 2), ("ARl", 3)):
        res[name] = _mean(recall[:, :, a, m100])
    if len(category_names) != recall.shape[1]:
        raise ValueError(f"summarize_recall: {len(category_names)} category names for a recall array of {recall.shape[1]}")
    for split, cats in class_splits.items():
        res[f"AR100_split_{split}"] = _mean(recall[:, list(cats), 0, m100])
    return res


def accumulate_lvis(tables, num_categories):
    """Rule 9 of include/ovis_hip.h -> (precision fp64 [T, R, K, A], recall fp64 [T, K, A]) from the match tables of
    ``rules="lvis"`` (the structure ``accumulate`` takes; a problem holds every detection that survived the image's cap and
    the federated filter -- there is no maxDets dimension).  -1: the (category, area) has no non-ignored ground truth."""
    cat = np.asarray(tables["category"], dtype=np.int64)
    det_start, gt_start = np.asarray(tables["det_start"], dtype=np.int64), np.asarray(tables["gt_start"], dtype=np.int64)
    scores_all = np.asarray(tables["scores"], dtype=np.float64)
    matched_all, dt_ignore_all = np.asarray(tables["dt_match"]) >= 0, np.asarray(tables["dt_ignore"], dtype=bool)
    gt_ignore_all = np.asarray(tables["gt_ignore"], dtype=bool)
    det_cat, gt_cat = np.repeat(cat, np.diff(det_start)), np.repeat(cat, np.diff(gt_start))
    num_t, num_r, num_a = len(IOU_THRESHOLDS), len(RECALL_THRESHOLDS), len(AREA_RANGES)
    precision, recall = -np.ones((num_t, num_r, num_categories, num_a)), -np.ones((num_t, num_categories, num_a))
    for k in range(num_categories):
        sel, gts_k = np.nonzero(det_cat == k)[0], gt_cat == k
        if not gts_k.any():
            continue
        sel = sel[np.argsort(-scores_all[sel], kind="mergesort")]  # a stable sort: equal scores stay in image order
        for a in range(num_a):
            npig = np.count_nonzero(~gt_ignore_all[a][gts_k])
            if npig == 0:
                continue
            dtm, dt_ig = matched_all[a][:, sel], dt_ignore_all[a][:, sel]
            tp_sum = np.cumsum(np.logical_and(dtm, np.logical_not(dt_ig)), axis=1).astype(dtype=np.float64)
            fp_sum = np.cumsum(np.logical_and(np.logical_not(dtm), np.logical_not(dt_ig)), axis=1).astype(dtype=np.float64)
            for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                precision[t, :, k, a] = _sampled_precision(tp, fp, npig)
                recall[t, k, a] = (tp / npig)[-1] if len(tp) else 0
    return precision, recall


def summarize_lvis(precision, category_names, class_splits, frequencies, class_order=None, recall=None):
    """Rule 10 of include/ovis_hip.h -> OrderedDict: AP, AP50, AP75, APs, APm, APl, then APr, APc, APf (area "all" over the
    categories whose ``frequencies`` entry is r, c, f), AP50_class_<name> (``class_order`` as in ``summarize``) and
    AP50_split_<split>; ``recall`` (``accumulate_lvis``' second array): followed by AR@300, ARs@300, ARm@300, ARl@300 and
    AR@300_split_<split>.  The 300 of the keys is the cap the numbers are usually made with (``LVIS_MAX_DETS``)."""
    if len(category_names) != precision.shape[2] or len(frequencies) != precision.shape[2]:
        raise ValueError(f"summarize_lvis: {len(category_names)} names and {len(frequencies)} frequencies for a precision "
                         f"array of {precision.shape[2]} categories")
    t50, t75 = np.where(.5 == IOU_THRESHOLDS)[0], np.where(.75 == IOU_THRESHOLDS)[0]
    res = OrderedDict()
    res["AP"] = _mean(precision[:, :, :, 0])
    res["AP50"] = _mean(precision[t50][:, :, :, 0])
    res["AP75"] = _mean(precision[t75][:, :, :, 0])
    for name, a in (("APs", 1), ("APm", 2), ("APl", 3)):
        res[name] = _mean(precision[:, :, :, a])
    for f in LVIS_FREQUENCIES:
        res[f"AP{f}"] = _mean(precision[:, :, np.asarray([k for k, v in enumerate(frequencies) if v == f], dtype=np.int64), 0])
    s = precision[t50][:, :, :, 0]  # [1, R, K]
    for k in range(len(category_names)) if class_order is None else class_order:
        res[f"AP50_class_{category_names[k]}"] = _mean(s[:, :, [k]])
    for split, cats in class_splits.items():
        res[f"AP50_split_{split}"] = _mean(s[:, :, list(cats)])
    if recall is not None:
        for name, a in zip(LVIS_RECALL_METRICS, range(len(AREA_RANGES))):
            res[name] = _mean(recall[:, :, a])
        for split, cats in class_splits.items():
            res[f"AR@300_split_{split}"] = _mean(recall[:, list(cats), 0])
    return res


def format_results(results):
    """The reference's ``Task: ... / names / values`` table (``COCOResults.__repr__``, coco_eval.py:406-414)."""
    out = "\n"
    for task, metrics in results.items():
        out += "Task: {}\n".format(task)
        out += ", ".join(metrics.keys()) + "\n"
        out += ", ".join("{:.4f}".format(v) for v in metrics.values()) + "\n"
    return out


# ---- host: ground truth and detections as rows ----------------------------------------------------------------------------
def rle_decode(rle, height, width):
    """uint8 [height, width] of a COCO RLE ``{"counts", "size"}``: column-major runs, zeros first; ``counts`` an
    uncompressed list or pycocotools' compressed string (``rleFrString``).  The host statement of the format: scoring
    itself decodes on the device (``_C.coco_rle_words``), the tests hold that decoder and the export's strings to this."""
    counts = rle["counts"]
    if list(rle.get("size", [height, width])) != [height, width]:
        raise ValueError(f"RLE of size {rle.get('size')} on an image of {height} x {width}")
    if isinstance(counts, (str, bytes)):
        s = counts.encode("ascii") if isinstance(counts, str) else counts
        runs, p = [], 0
        while p < len(s):
            x, k, more = 0, 0, True
            while more:
                c = s[p] - 48
                x |= (c & 0x1f) << (5 * k)
                more = bool(c & 0x20)
                p += 1
                k += 1
                if not more and (c & 0x10):
                    x |= -1 << (5 * k)
            if len(runs) > 2:
                x += runs[-2]
            runs.append(x)
        counts = runs
    counts = np.asarray(counts, dtype=np.int64)
    if counts.ndim != 1 or (counts < 0).any() or int(counts.sum()) != height * width:
        raise ValueError(f"RLE runs do not add up to {height} x {width} pixels")
    flat = np.repeat(np.arange(len(counts)) % 2, counts).astype(np.uint8)
    return np.ascontiguousarray(flat.reshape(width, height).T)


def category_frequencies(dataset):
    """The ``frequency`` (r, c or f) of every category of the annotation file, in sorted-id order (rule 1 of LVIS-style
    scoring, include/ovis_hip.h).  ValueError naming the first category without one."""
    coco = dataset.coco
    out = []
    for c in coco.cat_ids():
        f = coco.cats[c].get("frequency")
        if f not in LVIS_FREQUENCIES:
            raise ValueError(f"rules='lvis': category {c} ({coco.cats[c].get('name')}) has no 'frequency' in "
                             f"{LVIS_FREQUENCIES} (got {f!r}); the annotation file is not federatedly annotated")
        out.append(f)
    return out


def _ground_truth(dataset, rules="coco"):
    """-> (category ids sorted, per image of the file in id order a record of its annotations sorted by category index,
    stably: annotation order inside a category).  ``rules="lvis"`` (rules 1 and 2 of include/ovis_hip.h): every record also
    holds ``neg`` and ``not_exhaustive`` (int64 arrays of category indices, sorted) and ``ignore`` (the annotations'
    ``ignore`` keys), its ``crowd`` is all zero (``iscrowd`` is not read), and an image without either list or a category
    without ``frequency`` is a ValueError that names it."""
    _check_rules(rules, "evaluate_coco")
    coco = dataset.coco
    cat_ids = coco.cat_ids()
    cat_index = {c: i for i, c in enumerate(cat_ids)}
    lvis = rules == "lvis"
    images = []
    for img_id in sorted(coco.imgs):
        info = coco.imgs[img_id]
        anns = [a for a in coco.anns(img_id) if a["category_id"] in cat_index]
        anns = sorted(anns, key=lambda a: cat_index[a["category_id"]])  # stable
        boxes = np.asarray([a["bbox"] for a in anns], dtype=np.float64).reshape(-1, 4)
        images.append({
            "id": img_id, "width": int(info["width"]), "height": int(info["height"]), "anns": anns, "boxes": boxes,
            "cats": np.asarray([cat_index[a["category_id"]] for a in anns], dtype=np.int64),
            "areas": np.asarray([a["area"] if "area" in a else a["bbox"][2] * a["bbox"][3] for a in anns], dtype=np.float64),
            "crowd": np.asarray([1 if a.get("iscrowd", 0) and not lvis else 0 for a in anns], dtype=np.uint8),
            "polygons": sum(len(a["segmentation"]) for a in anns if isinstance(a.get("segmentation"), list))})
        if lvis:
            for key in ("neg_category_ids", "not_exhaustive_category_ids"):
                if not isinstance(info.get(key), (list, tuple)):
                    raise ValueError(f"rules='lvis': image {img_id} has no '{key}' list; the annotation file is not "
                                     "federatedly annotated")
            images[-1].update(
                neg=np.unique([cat_index[c] for c in info["neg_category_ids"] if c in cat_index]).astype(np.int64),
                not_exhaustive=np.unique([cat_index[c] for c in info["not_exhaustive_category_ids"]
                                          if c in cat_index]).astype(np.int64),
                ignore=np.asarray([1 if a.get("ignore", 0) else 0 for a in anns], dtype=np.uint8))
    if lvis:
        category_frequencies(dataset)  # raises on the first category without a frequency
    return cat_ids, images


def detection_boxes(pred, width, height):
    """(xyxy, xywh) float32 [K, 4] on the host: the prediction's boxes resized to the file's ``width`` x ``height``, and the
    reference's ``BoxList.convert("xywh")`` of them, w = x2 - x1 + 1 (coco_eval.py:82-83)."""
    xyxy = BoxList(pred.bbox.detach().cpu(), pred.size).resize((width, height)).bbox
    x1, y1, x2, y2 = xyxy.unbind(1)
    return xyxy, torch.stack((x1, y1, x2 - x1 + 1, y2 - y1 + 1), 1)


def mask_maps(pred):
    """The prediction's ``mask`` field, which must hold the mask head's [K, 1, M, M] probability maps."""
    if not pred.has_field("mask"):
        raise ValueError("evaluate_coco: segm scoring needs the predictions' 'mask' field (MODEL.MASK_ON)")
    maps = pred.get_field("mask")
    if not torch.is_tensor(maps) or not maps.is_floating_point() or maps.dim() != 4 or maps.shape[1] != 1 \
            or maps.shape[2] != maps.shape[3] or maps.shape[0] != len(pred):
        raise ValueError(
            f"evaluate_coco: field 'mask' must hold the mask head's [K, 1, M, M] probability maps, got "
            f"{getattr(maps, 'dtype', type(maps).__name__)} {tuple(getattr(maps, 'shape', ()))}; masks that are already "
            "pasted into the image (MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS True) cannot be scored -- run inference with "
            "MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS False")
    return maps


def _kept_rows(cats, scores, image, rules, lvis_max_dets):
    """The detections of one image that are scored, as indices into ``cats`` / ``scores`` sorted by (category index,
    descending score), stably: ties keep the input order.  coco: at most 100 per category.  lvis (rules 3 to 5 of
    include/ovis_hip.h): the ``lvis_max_dets`` best of the image over all categories together (negative: all), and of those
    the ones whose category is a negative of the image or has a ground truth in it."""
    if rules != "lvis":
        order = np.lexsort((-scores, cats))
        rank = np.arange(len(order)) - np.searchsorted(cats[order], cats[order], side="left")
        return order[rank < MAX_DETS[-1]]
    order = np.argsort(-scores, kind="mergesort")
    if lvis_max_dets >= 0:
        order = order[:lvis_max_dets]
    order = order[np.isin(cats[order], np.union1d(image["neg"], image["cats"]))]
    return order[np.lexsort((-scores[order], cats[order]))]  # equal scores stay in the order the first sort left them in


def _detections(pred, image, label_to_cat, with_masks, rules="coco", lvis_max_dets=LVIS_MAX_DETS):
    """One image's prediction as rows sorted by (category index, descending score), stably, at most 100 per category
    (coco_eval.py:71-105 / :108-162 and the ``dt[0:maxDets[-1]]`` of COCOeval.computeIoU); ``rules="lvis"``: the image's
    cap and the federated filter instead (``_kept_rows``)."""
    empty = {"cats": np.zeros(0, np.int64), "scores": np.zeros(0), "xywh": np.zeros((0, 4)), "xyxy": None, "maps": None}
    if pred is None or len(pred) == 0:
        return empty
    xyxy, xywh = detection_boxes(pred, image["width"], image["height"])
    scores = pred.get_field("scores").detach().cpu().double().numpy()
    cats = np.asarray([label_to_cat[int(l)] for l in pred.get_field("labels").tolist()], dtype=np.int64)
    order = _kept_rows(cats, scores, image, rules, lvis_max_dets)  # stable: ties keep prediction order
    out = {"cats": cats[order], "scores": scores[order], "xywh": xywh.double().numpy()[order], "xyxy": None, "maps": None}
    if with_masks:
        maps = mask_maps(pred)
        index = torch.from_numpy(order)
        out["maps"], out["xyxy"] = maps.detach().cpu()[index, 0].float(), xyxy[index]
    return out


def load_coco_results(dataset, results, iou_type, rules="coco", lvis_max_dets=LVIS_MAX_DETS, images=None):
    """The detections of a COCO results file as per-image rows, for the images of ``_ground_truth(dataset)`` in its order
    (pycocotools' ``loadRes`` and the ``dt[0:maxDets[-1]]`` of COCOeval): ``results`` is a path or the parsed list of
    {"image_id", "category_id", "score", "bbox" (xywh) or "segmentation" ({"size": [h, w], "counts": str or list})}.  Rows
    are what ``_detections`` makes: sorted by (category index, descending score), stably in file order, at most 100 per
    category and image.  bbox: ``xywh`` as written (the area is w * h).  segm: ``rle`` holds the rows' segmentation dicts in
    place of ``maps`` / ``xyxy`` (the area comes from the decoder); ``entry`` is every row's index in the file.  Entries of
    a category the annotation file does not have are dropped (COCOeval never evaluates them).  ValueError, naming the
    entry: an image_id the file does not have, a polygon segmentation, a ``size`` that is not the image's, a missing key.
    ``rules="lvis"``: the image's cap of ``lvis_max_dets`` and the federated filter take the place of the 100 per category
    (``_kept_rows``); ``images``: the records of ``_ground_truth(dataset, "lvis")`` when the caller already has them."""
    _check_iou_type(iou_type, "load_coco_results")
    _check_rules(rules, "load_coco_results")
    if rules == "lvis" and images is None:
        images = _ground_truth(dataset, rules)[1]  # boundary: the rows of segm, it scores the same segm.json
    if isinstance(results, (str, bytes, os.PathLike)):
        with open(results) as f:
            results = json.load(f)
    if not isinstance(results, (list, tuple)):
        raise ValueError(f"load_coco_results: a results file is a JSON list of detections, got {type(results).__name__}")
    coco = dataset.coco
    cat_index = {c: i for i, c in enumerate(coco.cat_ids())}
    field = "bbox" if iou_type == "bbox" else "segmentation"
    per_image = {}
    for index, entry in enumerate(results):
        where = f"load_coco_results: entry {index}"
        if not isinstance(entry, dict) or "image_id" not in entry:
            raise ValueError(f"{where} has no 'image_id'")
        where += f" (image_id {entry['image_id']})"
        if entry["image_id"] not in coco.imgs:
            raise ValueError(f"{where}: the annotation file has no such image")
        for key in ("category_id", "score", field):
            if key not in entry:
                raise ValueError(f"{where} has no '{key}'")
        if entry["category_id"] not in cat_index:
            continue
        if iou_type == "bbox":
            if len(entry["bbox"]) != 4:
                raise ValueError(f"{where}: 'bbox' is not [x, y, w, h]")
        else:
            seg, info = entry["segmentation"], coco.imgs[entry["image_id"]]
            if isinstance(seg, (list, tuple)):
                raise ValueError(f"{where}: polygon segmentations in results are not supported (RLE only)")
            if not isinstance(seg, dict) or "counts" not in seg or "size" not in seg:
                raise ValueError(f"{where}: 'segmentation' is not an RLE {{'size', 'counts'}}")
            if list(seg["size"]) != [int(info["height"]), int(info["width"])]:
                raise ValueError(f"{where}: RLE of size {seg['size']} on an image of {info['height']} x {info['width']}")
        per_image.setdefault(entry["image_id"], []).append(index)
    rows = []
    for position, img_id in enumerate(sorted(coco.imgs)):
        members = per_image.get(img_id, [])
        scores = np.asarray([results[k]["score"] for k in members], dtype=np.float64)
        cats = np.asarray([cat_index[results[k]["category_id"]] for k in members], dtype=np.int64)
        # stable: ties keep file order
        order = _kept_rows(cats, scores, images[position] if rules == "lvis" else None, rules, lvis_max_dets)
        members = [members[k] for k in order]
        row = {"cats": cats[order], "scores": scores[order], "xywh": np.zeros((len(members), 4)), "xyxy": None, "maps": None,
               "entry": np.asarray(members, dtype=np.int64)}
        if iou_type == "bbox":
            row["xywh"] = np.asarray([results[k]["bbox"] for k in members], dtype=np.float64).reshape(-1, 4)
        else:
            row["rle"] = [results[k]["segmentation"] for k in members]
        rows.append(row)
    return rows


def _chunks(images, dets, with_masks, budget, max_images=None, boundary=False, errors=False):
    """Lists of consecutive image indices: a chunk closes before the image that would take it over ``budget`` bytes of
    masks, over ``max_images`` (None: MAX_CHUNK_IMAGES) or -- for segm -- over MAX_CALL_MASKS detections, ground truths or
    polygons.  An image that breaks a limit alone still gets its own chunk.  ``boundary``: a mask costs 11 / 8 byte per
    pixel instead of 9 / 8 -- its boundary words (10 / 8), and as much again for ``_C.coco_boundary_words``' scratch.
    ``errors`` (error analysis, engine/error_analysis.py): the image-level IoU block of an image, 8 bytes per (detection,
    ground truth) pair over ALL its categories, is planned on top, for box scoring too."""
    max_images = MAX_CHUNK_IMAGES if max_images is None else max_images
    chunk, used = [], np.zeros(4, dtype=np.int64)
    limits = np.asarray([budget, MAX_CALL_MASKS, MAX_CALL_MASKS, MAX_CALL_MASKS], dtype=np.float64)
    for i, (image, det) in enumerate(zip(images, dets)):
        n_det, n_gt = len(det["cats"]), len(image["cats"])
        cost = np.asarray([(n_det + n_gt) * image["height"] * image["width"] * (11 if boundary else 9) // 8, n_det, n_gt,
                           image["polygons"]], dtype=np.int64) * (1 if with_masks else 0)
        if errors:
            cost[0] += n_det * n_gt * 8
        if chunk and (np.any(used + cost > limits) or len(chunk) >= max_images):
            yield chunk
            chunk, used = [], np.zeros(4, dtype=np.int64)
        chunk.append(i)
        used = used + cost
    if chunk:
        yield chunk


@contextlib.contextmanager
def _stage(timer, name):
    """Device events around a stage when ``timer`` (a dict name -> list of (start, end)) is given."""
    if timer is None:
        yield
        return
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    yield
    end.record()
    timer.setdefault(name, []).append((start, end))


def _decode_rle(segmentations, names, height, width, device):
    """(words int64 [n, ceil(height * width / 64)], areas int64 [n]) of n COCO RLEs of one image size, decoded on the device
    in one ``_C.coco_rle_words`` call.  ``names[k]`` says what mask k is, for the ValueError a malformed one raises."""
    sizes = torch.tensor([[height, width]], dtype=torch.int32).expand(len(segmentations), 2).contiguous().to(device)
    words, _, areas, status = _C.coco_rle_words([s["counts"] for s in segmentations], sizes)
    status = status.cpu().numpy()
    if status.any():
        k = int(np.flatnonzero(status)[0])
        raise ValueError(f"{names[k]}: malformed RLE for an image of {height} x {width}: "
                         f"{_C.COCO_RLE_STATUS.get(int(status[k]), int(status[k]))}")
    return words.view(len(segmentations), -1), areas


def _pack_group(group_rows, masks, words_parts, areas_out, base, rle=None):
    """Packs one image-size group's masks; -> the word offset behind it.  ``rle``: (rows of ``masks``, their words, their
    areas) of the group's RLE masks, which take the place of what those (empty) rows of ``masks`` pack to."""
    words, areas = _C.coco_pack_masks(masks)
    if rle is not None:
        words[rle[0]], areas[rle[0]] = rle[1], rle[2]
    words_parts.append(words.reshape(-1))
    areas_out[group_rows] = areas
    return base + words.numel()


def _boundary_group(words_parts, bwords_parts, bareas_out, group_rows, height, width, ratio, timer):
    """The boundary words and areas (``_C.coco_boundary_words``) of the image-size group whose mask words were appended to
    ``words_parts`` last."""
    nwords = (height * width + 63) // 64
    with _stage(timer, "boundary"):
        bwords, bareas = _C.coco_boundary_words(words_parts[-1].view(-1, nwords), height, width,
                                                boundary_dilation(height, width, ratio))
    bwords_parts.append(bwords.reshape(-1))
    bareas_out[group_rows] = bareas


def _image_problems(images, dets, det_image_base, gt_image_base, image_words, device):
    """The chunk's image-level table (error analysis): ``CocoProblems`` with one row per image -- all its detection rows
    against all its ground-truth rows; ``image_words``: image -> (first det word, first gt word, words per mask), or None
    for boxes."""
    rows, off = [], 0
    for i, (image, det) in enumerate(zip(images, dets)):
        nd, ng = len(det["cats"]), len(image["cats"])
        rows.append([det_image_base[i], nd, gt_image_base[i], ng, off] + list(image_words[i] if image_words else (0, 0, 0)))
        off += nd * ng
    return _C.CocoProblems(np.asarray(rows, dtype=np.int64).reshape(-1, 8), device)


def score_chunk(images, dets, iou_type, device, timer=None, boundary_dilation_ratio=BOUNDARY_DILATION_RATIO, rules="coco",
                error_thresholds=None):
    """The match tables of one chunk of images (the NumPy form ``accumulate`` takes): a constant number of launches --
    box or mask IoU and the matching -- plus, for segm, the paste, rasterise and pack calls of every image size; detections
    that carry ``rle`` (``load_coco_results``) and RLE ground truth take one ``_C.coco_rle_words`` call per image size
    instead -- a malformed encoding raises a ValueError that names the entry or the annotation.

    boundary (Boundary AP: the rule is in include/ovis_hip.h) works on the words segm makes: one
    ``_C.coco_boundary_words`` call per image size and side, then ``_C.coco_boundary_iou`` writes min(mask IoU, boundary
    IoU) where segm has the mask IoU, and the same matching follows -- with the MASK areas.  ``iou_type`` may be the tuple
    ("segm", "boundary"): the words are made once, both IoU buffers are matched, and {name: tables} comes back.

    ``rules="lvis"`` (``images`` / ``dets`` from ``_ground_truth`` / ``_detections`` under the same rules): the IoU entries
    get all-zero crowd flags, and ``_C.lvis_match`` takes the place of ``_C.coco_match`` -- with the annotations' ignore
    flags and one not-exhaustive flag per problem (rules 7 and 8 of include/ovis_hip.h).

    ``error_thresholds=(t_f, t_b)`` (default None: nothing changes, not a key, not a launch): the error analysis of
    include/ovis_hip.h for bbox and segm.  One more IoU call on a table with ONE ROW PER IMAGE fills the image-level buffer
    -- every detection of an image against every ground truth of it, from the box rows or the mask words that are already
    there -- and ``_C.error_types`` reads it beside the base matching ``dt_match[0, 0]``.  Their tables gain ``err_type`` uint8
    [D], ``err_gt`` int32 [D] (the chunk's ground-truth row or -1), ``gt_missed`` uint8 [G], ``det_image`` / ``gt_image`` (the
    row's image, counted inside the chunk) and ``num_images``.  boundary's tables are not analysed."""
    if error_thresholds is not None and rules != "coco":
        raise ValueError("evaluate_coco: the error analysis follows COCO's rules only (rules='coco')")
    types = (iou_type,) if isinstance(iou_type, str) else tuple(iou_type)
    with_masks, boundary = types[0] != "bbox", "boundary" in types
    rows, det_base, gt_base, iou_off = [], 0, 0, 0
    det_image_base, gt_image_base = [], []
    for i, (image, det) in enumerate(zip(images, dets)):
        det_image_base.append(det_base)
        gt_image_base.append(gt_base)
        for c in np.union1d(det["cats"], image["cats"]).tolist():
            d0, d1 = np.searchsorted(det["cats"], [c, c + 1])
            g0, g1 = np.searchsorted(image["cats"], [c, c + 1])
            rows.append([det_base + d0, d1 - d0, gt_base + g0, g1 - g0, iou_off, 0, 0, 0, c, i])
            iou_off += (d1 - d0) * (g1 - g0)
        det_base += len(det["cats"])
        gt_base += len(image["cats"])
    table = np.asarray(rows, dtype=np.int64).reshape(-1, 10)
    num_dets, num_gts = det_base, gt_base
    crowd = torch.from_numpy(np.concatenate([im["crowd"] for im in images] + [np.zeros(0, np.uint8)])).to(device)
    if rules == "lvis":  # crowd is all zero here: no IoU takes the crowd form
        gt_ignore_in = torch.from_numpy(np.concatenate([im["ignore"] for im in images] + [np.zeros(0, np.uint8)])).to(device)
        open_flags = np.asarray([c in images[i]["not_exhaustive"] for c, i in zip(table[:, 8], table[:, 9])], dtype=np.uint8)
        not_exhaustive = torch.from_numpy(open_flags.reshape(-1)).to(device)
    gt_areas = torch.from_numpy(np.concatenate([im["areas"] for im in images] + [np.zeros(0)])).to(device)
    scores = np.concatenate([d["scores"] for d in dets] + [np.zeros(0)])
    if not with_masks:
        det_xywh = torch.from_numpy(np.concatenate([d["xywh"] for d in dets] + [np.zeros((0, 4))])).to(device)
        gt_xywh = torch.from_numpy(np.concatenate([im["boxes"] for im in images] + [np.zeros((0, 4))])).to(device)
        problems = _C.CocoProblems(table[:, :8], device)
        with _stage(timer, "iou"):
            iou = _C.coco_box_iou(det_xywh, gt_xywh, crowd, problems)
            det_areas = det_xywh[:, 2] * det_xywh[:, 3]
        if error_thresholds is not None:
            image_problems = _image_problems(images, dets, det_image_base, gt_image_base, None, device)
            with _stage(timer, "image_iou"):
                image_iou = _C.coco_box_iou(det_xywh, gt_xywh, crowd, image_problems)
    else:
        groups = {}
        for i, image in enumerate(images):
            groups.setdefault((image["height"], image["width"]), []).append(i)
        det_words, gt_words, det_word_base, gt_word_base = [], [], 0, 0
        det_areas_i = torch.zeros(num_dets, dtype=torch.int64, device=device)
        gt_areas_i = torch.zeros(num_gts, dtype=torch.int64, device=device)
        det_bwords, gt_bwords = [], []  # boundary: the boundary words, laid out as the mask words
        det_bareas_i, gt_bareas_i = torch.zeros_like(det_areas_i), torch.zeros_like(gt_areas_i)
        image_words = {}  # image -> (first det word, first gt word, words per mask)
        for (height, width), members in groups.items():
            nwords = (height * width + 63) // 64
            det_rows = np.concatenate([np.arange(len(dets[i]["cats"])) + det_image_base[i] for i in members])
            gt_rows = np.concatenate([np.arange(len(images[i]["cats"])) + gt_image_base[i] for i in members])
            d_off, g_off = det_word_base, gt_word_base
            for i in members:
                image_words[i] = (d_off, g_off, nwords)
                d_off += len(dets[i]["cats"]) * nwords
                g_off += len(images[i]["cats"]) * nwords
            with_dets = [i for i in members if len(dets[i]["cats"])]
            if len(det_rows) and dets[with_dets[0]].get("rle") is not None:  # a results file: straight to the words
                names = [f"results entry {k} (image_id {images[i]['id']})" for i in with_dets for k in dets[i]["entry"]]
                with _stage(timer, "decode"):
                    words, areas = _decode_rle([s for i in with_dets for s in dets[i]["rle"]], names, height, width, device)
                det_words.append(words.reshape(-1))
                det_areas_i[torch.from_numpy(det_rows).to(device)] = areas
                det_word_base += words.numel()
            elif len(det_rows):
                maps = torch.cat([dets[i]["maps"] for i in members if len(dets[i]["cats"])]).to(device)
                boxes = torch.cat([dets[i]["xyxy"] for i in members if len(dets[i]["cats"])]).to(device)
                with _stage(timer, "paste"):
                    pasted = _C.paste_masks(maps, boxes, (height, width))
                with _stage(timer, "pack"):
                    det_word_base = _pack_group(torch.from_numpy(det_rows).to(device), pasted, det_words,
                                                det_areas_i, det_word_base)
                del pasted
            if boundary and len(det_rows):
                _boundary_group(det_words, det_bwords, det_bareas_i, torch.from_numpy(det_rows).to(device), height, width,
                                boundary_dilation_ratio, timer)
            if len(gt_rows):
                anns = [a for i in members for a in images[i]["anns"]]
                for a in anns:
                    if "segmentation" not in a:
                        raise ValueError(f"evaluate_coco: annotation {a.get('id')} has no 'segmentation' (segm scoring)")
                polygons = PolygonMasks([[] if isinstance(a["segmentation"], dict) else a["segmentation"] for a in anns],
                                        (width, height)).to(device)
                with _stage(timer, "rasterise"):
                    masks = polygons.convert_to_binarymask()
                rle_rows = [r for r, a in enumerate(anns) if isinstance(a["segmentation"], dict)]
                rle = None
                if rle_rows:  # decoded on the device to the words their (empty) rows of `masks` give way to
                    for r in rle_rows:
                        seg = anns[r]["segmentation"]
                        if list(seg.get("size", [height, width])) != [height, width]:
                            raise ValueError(f"RLE of size {seg.get('size')} on an image of {height} x {width}")
                    with _stage(timer, "decode"):
                        rle = (torch.tensor(rle_rows, device=device),) + _decode_rle(
                            [anns[r]["segmentation"] for r in rle_rows], [f"annotation {anns[r].get('id')}" for r in rle_rows],
                            height, width, device)
                with _stage(timer, "pack"):
                    gt_word_base = _pack_group(torch.from_numpy(gt_rows).to(device), masks, gt_words, gt_areas_i,
                                               gt_word_base, rle)
                del masks
                if boundary:
                    _boundary_group(gt_words, gt_bwords, gt_bareas_i, torch.from_numpy(gt_rows).to(device), height, width,
                                    boundary_dilation_ratio, timer)
        if len(table):  # the word columns of every problem, from its image's share of the word buffers
            img = table[:, 9]
            first = np.asarray([image_words[i] for i in range(len(images))], dtype=np.int64).reshape(-1, 3)
            table[:, 7] = first[img, 2]
            table[:, 5] = first[img, 0] + (table[:, 0] - np.asarray(det_image_base)[img]) * table[:, 7]
            table[:, 6] = first[img, 1] + (table[:, 2] - np.asarray(gt_image_base)[img]) * table[:, 7]
        problems = _C.CocoProblems(table[:, :8], device)
        empty = torch.zeros(0, dtype=torch.int64, device=device)
        det_words, gt_words = torch.cat(det_words) if det_words else empty, torch.cat(gt_words) if gt_words else empty
        if "segm" in types:
            with _stage(timer, "iou"):
                iou = _C.coco_mask_iou(det_words, det_areas_i, gt_words, gt_areas_i, crowd, problems)
            if error_thresholds is not None:  # the same words once more, addressed image by image
                image_problems = _image_problems(images, dets, det_image_base, gt_image_base, image_words, device)
                with _stage(timer, "image_iou"):
                    image_iou = _C.coco_mask_iou(det_words, det_areas_i, gt_words, gt_areas_i, crowd, image_problems)
        if boundary:
            with _stage(timer, "boundary_iou"):
                boundary_iou = _C.coco_boundary_iou(det_words, torch.cat(det_bwords) if det_bwords else empty, det_areas_i,
                                                    det_bareas_i, gt_words, torch.cat(gt_bwords) if gt_bwords else empty,
                                                    gt_areas_i, gt_bareas_i, crowd, problems)
        det_areas = det_areas_i.double()  # boundary too: the area ranges stay those of the masks
    thresholds = torch.from_numpy(IOU_THRESHOLDS).to(device)
    area_ranges = torch.from_numpy(AREA_RANGES).to(device)
    tables = {}
    if error_thresholds is not None:
        det_cat = torch.from_numpy(np.concatenate([d["cats"] for d in dets] + [np.zeros(0, np.int64)]).astype(np.int32)).to(device)
        gt_cat = torch.from_numpy(np.concatenate([im["cats"] for im in images] + [np.zeros(0, np.int64)]).astype(np.int32)).to(device)
        det_gt_base = torch.from_numpy(np.repeat(table[:, 2], table[:, 1]).astype(np.int32)).to(device)
        det_image = np.repeat(np.arange(len(images)), [len(d["cats"]) for d in dets])
        gt_image = np.repeat(np.arange(len(images)), [len(im["cats"]) for im in images])
    for name in types:
        with _stage(timer, "match"):
            if rules == "lvis":
                dt_match, dt_ignore, gt_ignore = _C.lvis_match(boundary_iou if name == "boundary" else iou, problems,
                                                               det_areas, gt_areas, gt_ignore_in, not_exhaustive,
                                                               area_ranges, thresholds)
            else:
                dt_match, dt_ignore, gt_ignore = _C.coco_match(boundary_iou if name == "boundary" else iou, problems,
                                                               det_areas, gt_areas, crowd, area_ranges, thresholds)
        tables[name] = {"category": table[:, 8].copy(), "det_start": np.concatenate([table[:, 0], [num_dets]]),
                        "gt_start": np.concatenate([table[:, 2], [num_gts]]), "scores": scores,
                        "dt_match": dt_match.cpu().numpy(), "dt_ignore": dt_ignore.cpu().numpy(),
                        "gt_ignore": gt_ignore.cpu().numpy()}
        if error_thresholds is not None and name != "boundary":
            with _stage(timer, "error_types"):
                base = dt_match[0, 0]  # the ground truth's index inside its problem -> its row in the chunk
                err_type, err_gt, gt_missed = _C.error_types(
                    image_iou, image_problems, det_cat, torch.where(base >= 0, base + det_gt_base, base),
                    dt_ignore[0, 0].view(torch.uint8), gt_cat, crowd, *error_thresholds)
            tables[name].update(err_type=err_type.cpu().numpy(), err_gt=err_gt.cpu().numpy(), gt_missed=gt_missed.cpu().numpy(),
                                det_image=det_image, gt_image=gt_image, num_images=len(images))
    return tables[iou_type] if isinstance(iou_type, str) else tables


def concatenate_tables(parts):
    """The match tables of consecutive chunks as one."""
    det_off, gt_off, det_start, gt_start = 0, 0, [], []
    for p in parts:
        det_start.append(p["det_start"][:-1] + det_off)
        gt_start.append(p["gt_start"][:-1] + gt_off)
        det_off += p["det_start"][-1]
        gt_off += p["gt_start"][-1]
    num_a, num_t = len(AREA_RANGES), len(IOU_THRESHOLDS)
    errors = {}
    if parts and all("err_type" in p for p in parts):  # the error analysis' arrays travel with the tables they belong to
        gt_offs = np.cumsum([0] + [p["gt_start"][-1] for p in parts])
        image_offs = np.cumsum([0] + [p["num_images"] for p in parts])
        errors = {"err_type": np.concatenate([p["err_type"] for p in parts]),
                  "err_gt": np.concatenate([np.where(p["err_gt"] >= 0, p["err_gt"] + off, -1).astype(np.int32)
                                            for p, off in zip(parts, gt_offs)]),
                  "gt_missed": np.concatenate([p["gt_missed"] for p in parts]),
                  "det_image": np.concatenate([p["det_image"] + off for p, off in zip(parts, image_offs)]),
                  "gt_image": np.concatenate([p["gt_image"] + off for p, off in zip(parts, image_offs)]),
                  "num_images": int(image_offs[-1])}
    return {"category": np.concatenate([p["category"] for p in parts] + [np.zeros(0, np.int64)]),
            "det_start": np.concatenate(det_start + [np.asarray([det_off], dtype=np.int64)]),
            "gt_start": np.concatenate(gt_start + [np.asarray([gt_off], dtype=np.int64)]),
            "scores": np.concatenate([p["scores"] for p in parts] + [np.zeros(0)]),
            "dt_match": np.concatenate([p["dt_match"] for p in parts] + [np.zeros((num_a, num_t, 0), np.int32)], axis=2),
            "dt_ignore": np.concatenate([p["dt_ignore"] for p in parts] + [np.zeros((num_a, num_t, 0), bool)], axis=2),
            "gt_ignore": np.concatenate([p["gt_ignore"] for p in parts] + [np.zeros((num_a, 0), bool)], axis=1), **errors}


def _job_types(iou_type, who):
    """The names of one scoring pass: ``iou_type`` itself, or the members of the tuple ("segm", "boundary")."""
    types = (iou_type,) if isinstance(iou_type, str) else tuple(iou_type)
    for t in types:
        _check_iou_type(t, who)
    if len(types) != 1 and types != MASK_IOU_TYPES:
        raise ValueError(f"{who}: one pass scores one iou_type or {MASK_IOU_TYPES}, not {types}")
    return types


def match_tables(dataset, predictions, iou_type, device, budget=None, timer=None, max_images=None, ground_truth=None,
                 boundary_dilation_ratio=BOUNDARY_DILATION_RATIO, rules="coco", lvis_max_dets=LVIS_MAX_DETS,
                 error_thresholds=None):
    """-> (the match tables of every (image, category) problem of the annotation file, in image-id order; the sorted
    category ids).  ``budget``: the bytes of device memory a chunk may plan with (None: a quarter of what is free);
    ``max_images``: the most images of a chunk (None: MAX_CHUNK_IMAGES); ``ground_truth``: ``_ground_truth(dataset, rules)``
    when the caller already has it.  ``iou_type``: bbox, segm, boundary, or the tuple ("segm", "boundary") -- then the first
    item is {name: tables}, both from one set of mask words per chunk.  ``rules="lvis"``: LVIS-style federated scoring
    (include/ovis_hip.h), at most ``lvis_max_dets`` detections per image.  ``error_thresholds=(t_f, t_b)``: the tables of
    bbox and segm also carry the error analysis' arrays (``score_chunk``)."""
    types = _job_types(iou_type, "evaluate_coco")
    _check_rules(rules, "evaluate_coco")
    if len(predictions) > len(dataset):
        raise ValueError(f"evaluate_coco: {len(predictions)} predictions for a dataset of {len(dataset)} images")
    device = torch.device(device)
    cat_ids, images = ground_truth if ground_truth is not None else _ground_truth(dataset, rules)
    cat_index = {c: i for i, c in enumerate(cat_ids)}
    label_to_cat = {label: cat_index[json_id] for label, json_id in dataset.contiguous_category_id_to_json_id.items()}
    by_image = {dataset.id_to_img_map[idx]: pred for idx, pred in enumerate(predictions)}
    dets = [_detections(by_image.get(image["id"]), image, label_to_cat, types[0] != "bbox", rules, lvis_max_dets)
            for image in images]
    return _score_rows(images, dets, iou_type, device, budget, timer, max_images, boundary_dilation_ratio, rules,
                       error_thresholds), cat_ids


def _score_rows(images, dets, iou_type, device, budget, timer, max_images, boundary_dilation_ratio=BOUNDARY_DILATION_RATIO,
                rules="coco", error_thresholds=None):
    """The match tables of the images' ground truth and detection rows, chunk by chunk ({name: tables} for a tuple)."""
    if budget is None:
        budget = torch.cuda.mem_get_info(device)[0] // 4
    types = (iou_type,) if isinstance(iou_type, str) else tuple(iou_type)
    extra = {} if rules == "coco" else {"rules": rules}
    if error_thresholds is not None:
        extra["error_thresholds"] = tuple(float(t) for t in error_thresholds)
    parts = [score_chunk([images[i] for i in chunk], [dets[i] for i in chunk], iou_type, device, timer, boundary_dilation_ratio,
                         **extra)
             for chunk in _chunks(images, dets, types[0] != "bbox", budget, max_images, "boundary" in types,
                                  error_thresholds is not None)]
    if isinstance(iou_type, str):
        return concatenate_tables(parts)
    return {name: concatenate_tables([part[name] for part in parts]) for name in types}


def results_match_tables(dataset, results, iou_type, device, budget=None, timer=None, max_images=None, ground_truth=None,
                         boundary_dilation_ratio=BOUNDARY_DILATION_RATIO, rules="coco", lvis_max_dets=LVIS_MAX_DETS,
                         error_thresholds=None):
    """``match_tables`` for the detections of a results file (``results``: what ``load_coco_results`` takes)."""
    types = _job_types(iou_type, "evaluate_coco_results")
    _check_rules(rules, "evaluate_coco_results")
    device = torch.device(device)
    cat_ids, images = ground_truth if ground_truth is not None else _ground_truth(dataset, rules)
    dets = load_coco_results(dataset, results, types[0], rules, lvis_max_dets, images)
    return _score_rows(images, dets, iou_type, device, budget, timer, max_images, boundary_dilation_ratio, rules,
                       error_thresholds), cat_ids


def _scoring_device(device, who):
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{who}: scoring runs on the HIP device (IoU and matching have no host implementation)")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def _summaries(dataset, iou_types, device, tables_of, recall=False, ground_truth=None, rules="coco", tables_out=None):
    """{iou_type: ``summarize`` of ``accumulate`` of ``tables_of(iou_type, ground truth)``} with the dataset's names,
    splits and class order; ``recall``: followed by ``summarize_recall`` of ``accumulate_recall`` of the same tables.
    When segm and boundary are both asked for, ``tables_of`` is called ONCE for the two, with the tuple ("segm",
    "boundary"), and returns {name: tables} (``_jobs``).  ``rules="lvis"``: ``summarize_lvis`` of ``accumulate_lvis``."""
    results, scored = OrderedDict(), {}
    ground_truth = ground_truth if ground_truth is not None else _ground_truth(dataset, rules)
    frequencies = category_frequencies(dataset) if rules == "lvis" else None
    cat_ids = ground_truth[0]
    cat_index = {c: i for i, c in enumerate(cat_ids)}
    splits = OrderedDict((split, [cat_index[c] for c in ids]) for split, ids in dataset.class_splits.items())
    class_order = [cat_index[c] for c in dataset.categories if c in cat_index]
    with torch.cuda.device(device):
        for job in _jobs(iou_types):
            tables, _ = tables_of(job, ground_truth)
            scored.update({job: tables} if isinstance(job, str) else tables)
        if tables_out is not None:  # the caller goes on with the match tables themselves (engine/error_analysis.py)
            tables_out.update(scored, cat_ids=cat_ids)
        for iou_type in iou_types:
            tables = scored[iou_type]
            if rules == "lvis":
                precision, recalls = accumulate_lvis(tables, len(cat_ids))
                results[iou_type] = summarize_lvis(precision, [dataset.categories[c] for c in cat_ids], splits, frequencies,
                                                   class_order, recalls if recall else None)
                continue
            results[iou_type] = summarize(accumulate(tables, len(cat_ids)), [dataset.categories[c] for c in cat_ids], splits,
                                          class_order)
            if recall:
                results[iou_type].update(summarize_recall(accumulate_recall(tables, len(cat_ids)),
                                                          [dataset.categories[c] for c in cat_ids], splits))
    return results


def evaluate_coco(dataset, predictions, iou_types=("bbox", "segm"), device="cuda", recall=False,
                  boundary_dilation_ratio=BOUNDARY_DILATION_RATIO, rules="coco", lvis_max_dets=LVIS_MAX_DETS,
                  error_thresholds=None, tables_out=None):
    """{iou_type: OrderedDict of AP, AP50, AP75, APs, APm, APl, AP50_class_<name> per category (in the order of
    ``dataset.categories``, as ``COCOResults.update`` iterates) and AP50_split_<split> per key of ``dataset.class_splits``}
    for ``predictions``: the list ``inference()`` returns or ``torch.load`` gives from ``predictions.pth`` (BoxLists in
    dataset-index order, fields ``scores``, ``labels`` and -- for segm -- ``mask`` [K, 1, M, M]).  ``recall``: followed by
    AR1, AR10, AR100, ARs, ARm, ARl and AR100_split_<split> (``summarize_recall``).  ``device``: the HIP device that scores;
    there is no host-only scoring.

    ``"boundary"`` among ``iou_types`` is Boundary AP (Cheng et al., CVPR 2021): segm's keys from a matching on min(mask
    IoU, boundary IoU), the boundary band ``boundary_dilation_ratio`` of the image diagonal deep -- the rule is written
    out in include/ovis_hip.h.  Beside segm it costs no second paste / rasterise / pack, and leaves segm's numbers alone.

    ``rules="lvis"``: LVIS-style federated scoring of an annotation file whose images carry ``neg_category_ids`` and
    ``not_exhaustive_category_ids`` and whose categories carry ``frequency`` -- the ten rules of include/ovis_hip.h, for
    every iou_type, boundary included: at most ``lvis_max_dets`` detections per image over all categories (negative: no
    cap), detections of categories nobody looked for in the image are not judged, and the keys are AP ... APl, APr, APc,
    APf, AP50_class_<name>, AP50_split_<split>, with ``recall`` AR@300, ARs@300, ARm@300, ARl@300, AR@300_split_<split>.
    The rules are restated, not imported: the numbers have not been compared with lvis-api's output.

    ``error_thresholds=(t_f, t_b)`` with ``tables_out={}`` (``rules="coco"`` only): the same pass also types the errors
    (``score_chunk``), and ``tables_out`` receives {iou_type: match tables} and ``cat_ids`` for
    ``engine.error_analysis.analyze_scored``; the returned numbers are those of a call without the two, bit for bit."""
    device = _scoring_device(device, "evaluate_coco")
    for iou_type in iou_types:
        _check_iou_type(iou_type, "evaluate_coco")
    _check_rules(rules, "evaluate_coco")
    if error_thresholds is not None:
        if rules != "coco":
            raise ValueError("evaluate_coco: the error analysis follows COCO's rules only (rules='coco')")
        return _summaries(dataset, iou_types, device,
                          lambda iou_type, gt: match_tables(dataset, predictions, iou_type, device, ground_truth=gt,
                                                            boundary_dilation_ratio=boundary_dilation_ratio,
                                                            error_thresholds=error_thresholds), recall, tables_out=tables_out)
    if rules == "coco":
        return _summaries(dataset, iou_types, device,
                          lambda iou_type, gt: match_tables(dataset, predictions, iou_type, device, ground_truth=gt,
                                                            boundary_dilation_ratio=boundary_dilation_ratio), recall)
    return _summaries(dataset, iou_types, device,
                      lambda iou_type, gt: match_tables(dataset, predictions, iou_type, device, ground_truth=gt,
                                                        boundary_dilation_ratio=boundary_dilation_ratio, rules=rules,
                                                        lvis_max_dets=lvis_max_dets), recall, rules=rules)


def evaluate_coco_results(dataset, results, iou_types=("bbox", "segm"), device="cuda", recall=False,
                          boundary_dilation_ratio=BOUNDARY_DILATION_RATIO, rules="coco", lvis_max_dets=LVIS_MAX_DETS,
                          error_thresholds=None, tables_out=None):
    """``evaluate_coco``'s numbers, in the same structure, for detections that come from COCO results files: ``results`` is
    {iou_type: a path or the parsed list} (``load_coco_results``); an iou_type it does not have is skipped -- but boundary
    reads the ``"boundary"`` entry when there is one and else the ``"segm"`` one: it scores the same ``segm.json``.  Whatever
    wrote the files -- ``export_coco_results``, the reference, another tool -- nothing but the annotation file is needed
    beside them.  ``recall``, ``boundary_dilation_ratio``, ``rules``, ``lvis_max_dets``, ``error_thresholds`` / ``tables_out`` (one
    file for segm and boundary): as in ``evaluate_coco``.  ``device``:
    the HIP device that decodes the masks and scores; there is no host-only scoring."""
    device = _scoring_device(device, "evaluate_coco_results")
    _check_rules(rules, "evaluate_coco_results")
    for iou_type in results:
        _check_iou_type(iou_type, "evaluate_coco_results")
    files = dict(results)
    if "boundary" not in files and "segm" in files:
        files["boundary"] = files["segm"]
    iou_types = [t for t in iou_types if t in files]
    errors = {}
    if error_thresholds is not None:
        if rules != "coco":
            raise ValueError("evaluate_coco_results: the error analysis follows COCO's rules only (rules='coco')")
        if "boundary" in files and files["boundary"] is not files["segm"]:
            raise ValueError("evaluate_coco_results: the error analysis scores segm and boundary from one results file")
        errors = {"error_thresholds": error_thresholds}
    if all(t in iou_types for t in MASK_IOU_TYPES) and files["boundary"] is not files["segm"]:  # two files: two passes
        return OrderedDict((t, evaluate_coco_results(dataset, {t: files[t]}, (t,), device, recall, boundary_dilation_ratio,
                                                     rules, lvis_max_dets)[t])
                           for t in iou_types)

    def tables_of(job, gt):
        return results_match_tables(dataset, files[job if isinstance(job, str) else job[0]], job, device, ground_truth=gt,
                                    boundary_dilation_ratio=boundary_dilation_ratio, rules=rules, lvis_max_dets=lvis_max_dets,
                                    **errors)
    return _summaries(dataset, iou_types, device, tables_of, recall, rules=rules, tables_out=tables_out)


# ---- every rank scores what it predicted: only match tables travel --------------------------------------------------------
def shard_owners(index_lists):
    """{dataset index: the rank that scores it} for ``index_lists[rank]`` = the dataset indices rank ``rank`` predicted: the
    LOWEST rank that holds an index owns it (the test sampler's last slice may wrap around to index 0, so an image can sit
    on two ranks).  A function of the exchanged lists alone: every rank evaluates it to the same answer."""
    owner = {}
    for rank, indices in enumerate(index_lists):
        for idx in indices:
            owner.setdefault(int(idx), rank)
    return owner


def merge_shard_tables(parts):
    """The match tables of several shards as the one table ``match_tables`` gives for all their images.  ``parts[rank]``:
    the tables of that rank's images plus ``image`` int [P], the image id of every problem; the problems of an image are
    consecutive (a whole-image block), the blocks of a part in any order.  Blocks are put into image-id order and
    concatenated; of an image that several parts hold, the lowest rank's block is kept (``shard_owners``' rule).  An image
    scores the same whatever else is scored beside it, so this is array for array the unsharded result -- and with it the
    tie order of ``accumulate``, whose stable sort leaves equal scores in image order.  Host only, NumPy only."""
    blocks = {}
    for part in parts:
        image = np.asarray(part["image"], dtype=np.int64)
        if len(image) != len(part["category"]):
            raise ValueError(f"merge_shard_tables: {len(image)} image ids for {len(part['category'])} problems")
        if not len(image):
            continue
        cuts = np.flatnonzero(np.diff(image)) + 1
        seen = set()
        for p0, p1 in zip(np.concatenate([[0], cuts]).tolist(), np.concatenate([cuts, [len(image)]]).tolist()):
            img_id = int(image[p0])
            if img_id in seen:
                raise ValueError(f"merge_shard_tables: the problems of image {img_id} are not one block")
            seen.add(img_id)
            blocks.setdefault(img_id, (part, p0, p1))  # parts come in rank order: the first holder is the lowest rank
    ordered = []
    for img_id in sorted(blocks):
        part, p0, p1 = blocks[img_id]
        d0, d1, g0, g1 = part["det_start"][p0], part["det_start"][p1], part["gt_start"][p0], part["gt_start"][p1]
        ordered.append({"category": part["category"][p0:p1], "det_start": part["det_start"][p0:p1 + 1] - d0,
                        "gt_start": part["gt_start"][p0:p1 + 1] - g0, "scores": part["scores"][d0:d1],
                        "dt_match": part["dt_match"][:, :, d0:d1], "dt_ignore": part["dt_ignore"][:, :, d0:d1],
                        "gt_ignore": part["gt_ignore"][:, g0:g1]})
    return concatenate_tables(ordered)


def evaluate_coco_sharded(dataset, local_predictions, iou_types=("bbox", "segm"), device="cuda", recall=False,
                          boundary_dilation_ratio=BOUNDARY_DILATION_RATIO, rules="coco", lvis_max_dets=LVIS_MAX_DETS):
    """``evaluate_coco``'s numbers without gathering the predictions: ``local_predictions`` is THIS rank's {dataset index:
    BoxList} (what ``engine.inference.compute_on_dataset`` returns), every rank calls this, rank 0 gets the OrderedDict and
    the others None.  The ranks exchange their index lists; ``shard_owners`` says who scores an image that sits on two of
    them, and the images of the annotation file that nobody predicted (those ``COCODataset`` drops are still scored) go
    to rank 0 with zero detections.  Every rank then makes the detection rows of its images and scores them against their
    ground truth on its own device (``_detections``, ``_score_rows``), and its match tables -- about 208 B per detection, not
    the M x M maps -- go to rank 0 with the image id of every problem, where ``merge_shard_tables`` puts them into the order
    ``match_tables`` has.  One process: the same code with one shard.  ``rules``, ``lvis_max_dets``: as in ``evaluate_coco``
    -- cap, federated filter and matching are per image, so nothing else changes."""
    device = _scoring_device(device, "evaluate_coco_sharded")
    _check_rules(rules, "evaluate_coco_sharded")
    for iou_type in iou_types:
        _check_iou_type(iou_type, "evaluate_coco_sharded")
    world, rank = comm.get_world_size(), comm.get_rank()
    index_lists = [sorted(int(i) for i in local_predictions)]
    if index_lists[0] and not 0 <= index_lists[0][0] <= index_lists[0][-1] < len(dataset):
        raise ValueError(f"evaluate_coco_sharded: prediction indices {index_lists[0][0]} .. {index_lists[0][-1]} for a dataset "
                         f"of {len(dataset)} images")
    if world > 1:
        mine, index_lists = index_lists[0], [None] * world
        dist.all_gather_object(index_lists, mine)
    owner_of_image = {dataset.id_to_img_map[idx]: r for idx, r in shard_owners(index_lists).items()}
    ground_truth = _ground_truth(dataset, rules)
    cat_ids, images = ground_truth
    cat_index = {c: i for i, c in enumerate(cat_ids)}
    label_to_cat = {label: cat_index[json_id] for label, json_id in dataset.contiguous_category_id_to_json_id.items()}
    images = [image for image in images if owner_of_image.get(image["id"], 0) == rank]  # in image-id order
    by_image = {dataset.id_to_img_map[idx]: local_predictions[idx] for idx in index_lists[rank]}
    merged = {}
    with torch.cuda.device(device):
        for job in _jobs(iou_types):  # segm and boundary together: one pass over the mask words, two tables
            dets = [_detections(by_image.get(image["id"]), image, label_to_cat, job != "bbox", rules, lvis_max_dets)
                    for image in images]
            scored = _score_rows(images, dets, job, device, None, None, None, boundary_dilation_ratio, rules)
            problems = np.asarray([len(np.union1d(det["cats"], image["cats"])) for image, det in zip(images, dets)],
                                  dtype=np.int64)
            for iou_type, tables in ({job: scored} if isinstance(job, str) else scored).items():
                tables["image"] = np.repeat(np.asarray([image["id"] for image in images], dtype=np.int64), problems)
                parts = [tables]
                if world > 1:
                    parts = [None] * world
                    dist.all_gather_object(parts, tables)
                if rank == 0:
                    merged[iou_type] = merge_shard_tables(parts)
    if rank != 0:
        return None
    return _summaries(dataset, iou_types, device,
                      lambda job, gt: (merged[job] if isinstance(job, str) else {t: merged[t] for t in job}, cat_ids), recall,
                      ground_truth, rules)


def annotation_dataset(ann_file):
    """The dataset object scoring needs, from the annotation file alone: no images, no configuration.  The ``split`` keys
    of its categories, when present, give the AP50_split_<split> rows."""
    from ..data.datasets import COCODataset

    dataset = COCODataset(ann_file, "", False)
    for item in dataset.coco.dataset["categories"]:
        if "split" in item:
            dataset.class_splits.setdefault(item["split"], []).append(item["id"])
    return dataset
