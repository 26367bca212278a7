"""The host half of COCO / LVIS-style scoring (engine/coco_eval.py): ``COCOeval.accumulate`` and ``summarize`` restated term
by term in NumPy fp64 over the match tables the device makes, and the joining of such tables -- O(detections), not hot.
NumPy only: nothing here loads the HIP library or touches a device.

MATCH TABLES.  What ``coco_eval.score_chunk`` / ``match_tables`` make and everything here takes -- the one description of the
structure: a dict of plain NumPy arrays over the P problems of a set of images, a problem being an (image, category) pair with
a detection or a ground truth, in image-id order and, inside an image, in category-index order; D detection rows and G
ground-truth rows, those of a problem consecutive; A = 4 area ranges, T = 10 IoU thresholds:

  ``category``   int [P]        the problem's index into the sorted category ids
  ``det_start``  int [P + 1]    the problem's detection rows are det_start[p] : det_start[p + 1]
  ``gt_start``   int [P + 1]    its ground-truth rows, likewise
  ``scores``     f64 [D]        descending inside a problem (coco: at most 100 per problem; lvis: what the image's cap and the
                                federated filter left)
  ``dt_match``   int32 [A, T, D]  the matched ground truth's index INSIDE ITS PROBLEM, or -1
  ``dt_ignore``  bool [A, T, D];  ``gt_ignore``  bool [A, G]

Scored with ``error_thresholds`` (bbox and segm under COCO's rules; engine/error_analysis.py reads them), the tables also hold

  ``err_type``   uint8 [D]      0 or the code of Cls, Loc, Both, Dupe, Bkg (``_C.ERROR_TYPES``)
  ``err_gt``     int32 [D]      the ground-truth ROW the error points at, or -1
  ``gt_missed``  uint8 [G];  ``det_image`` int [D], ``gt_image`` int [G]: the row's image, counted from 0;  ``num_images`` int

and a shard's tables on their way to rank 0 (``merge_shard_tables``) carry ``image`` int [P], the image id of every problem.
"""
from collections import OrderedDict

import numpy as np

IOU_THRESHOLDS = np.linspace(.5, .95, 10)
RECALL_THRESHOLDS = np.linspace(0, 1, 101)
MAX_DETS = (1, 10, 100)
AREA_RANGES = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], dtype=np.float64)  # all, s, m, l
METRICS = ("AP", "AP50", "AP75", "APs", "APm", "APl")
RECALL_METRICS = ("AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
LVIS_METRICS = METRICS + ("APr", "APc", "APf")
LVIS_FREQUENCIES = ("r", "c", "f")
LVIS_RECALL_METRICS = ("AR@300", "ARs@300", "ARm@300", "ARl@300")


# ---- COCOeval.accumulate ----------------------------------------------------------------------------------------------------
def _accumulated(tables, num_categories, caps, with_precision=True):
    """The one walk of ``COCOeval.accumulate`` over the match tables -> (precision fp64 [T, R, K, A, M] or None, recall fp64
    [T, K, A, M]), M = len(caps): every category with a ground-truth row x every cap on a detection's rank inside its problem
    (None: no cap) x every area range with non-ignored ground truths, from the running tp / fp sums over the category's
    detections inside the cap, merged by descending score.  -1: the (category, area range) has no non-ignored ground truth;
    recall is the last entry of tp / npig, 0 without a detection."""
    cat = np.asarray(tables["category"], dtype=np.int64)
    det_start, gt_start = np.asarray(tables["det_start"], dtype=np.int64), np.asarray(tables["gt_start"], dtype=np.int64)
    scores_all = np.asarray(tables["scores"], dtype=np.float64)
    matched_all, dt_ignore_all = np.asarray(tables["dt_match"]) >= 0, np.asarray(tables["dt_ignore"], dtype=bool)
    gt_ignore_all = np.asarray(tables["gt_ignore"], dtype=bool)
    det_problem = np.repeat(np.arange(len(cat)), np.diff(det_start))
    det_rank = np.arange(len(det_problem)) - det_start[:-1][det_problem]
    det_cat, gt_cat = cat[det_problem], np.repeat(cat, np.diff(gt_start))
    num_t, num_r, num_a = len(IOU_THRESHOLDS), len(RECALL_THRESHOLDS), len(AREA_RANGES)
    precision = -np.ones((num_t, num_r, num_categories, num_a, len(caps))) if with_precision else None
    recall = -np.ones((num_t, num_categories, num_a, len(caps)))
    for k in range(num_categories):
        gts_k = gt_cat == k
        if not gts_k.any():  # no ground truth: npig is 0 in every area range
            continue
        dets_k = np.nonzero(det_cat == k)[0]
        npigs = [np.count_nonzero(~gt_ignore_all[a][gts_k]) for a in range(num_a)]
        for m, cap in enumerate(caps):
            sel = dets_k if cap is None else dets_k[det_rank[dets_k] < cap]
            sel = sel[np.argsort(-scores_all[sel], kind="mergesort")]  # a stable sort: equal scores stay in image order
            for a, npig in enumerate(npigs):
                if npig == 0:
                    continue
                dtm, counted = matched_all[a][:, sel], np.logical_not(dt_ignore_all[a][:, sel])
                tp_sum = np.cumsum(np.logical_and(dtm, counted), axis=1).astype(dtype=np.float64)
                recall[:, k, a, m] = tp_sum[:, -1] / npig if len(sel) else 0
                if with_precision:
                    fp_sum = np.cumsum(np.logical_and(np.logical_not(dtm), counted), axis=1).astype(dtype=np.float64)
                    for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                        precision[t, :, k, a, m] = _sampled_precision(tp, fp, npig)
    return precision, recall


def accumulate(tables, num_categories):
    """``COCOeval.accumulate`` -> precision fp64 [T, R, K, A, M] (-1: no image entry or no non-ignored ground truth) from
    the match tables of every problem (this module's docstring)."""
    return _accumulated(tables, num_categories, MAX_DETS)[0]


def accumulate_recall(tables, num_categories):
    """The ``recall`` array of ``COCOeval.accumulate`` -> fp64 [T, K, A, M] from the same tables: -1 as in ``accumulate``, 0
    where the category has no detection, else tp / npig after the last of the first ``maxDet`` detections of every image (the
    first k columns of the maxDets = 100 matching ARE the maxDets = k matching: engine/coco_eval.py, RECALL)."""
    return _accumulated(tables, num_categories, MAX_DETS, with_precision=False)[1]


def accumulate_lvis(tables, num_categories):
    """Rule 9 of include/ovis_hip.h -> (precision fp64 [T, R, K, A], recall fp64 [T, K, A]) from the match tables of
    ``rules="lvis"``: no maxDets dimension.  -1: the (category, area) has no non-ignored ground truth."""
    precision, recall = _accumulated(tables, num_categories, (None,))
    return precision[..., 0], recall[..., 0]


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


# ---- COCOeval.summarize -----------------------------------------------------------------------------------------------------
def _summarize(precision, category_names, class_splits, class_order, frequencies=None):
    """The AP rows of precision fp64 [T, R, K, A]: the six of ``COCOeval.summarize``, with ``frequencies`` APr / APc / APf,
    then AP50_class_<name> and AP50_split_<split>."""
    t50, t75 = np.where(.5 == IOU_THRESHOLDS)[0], np.where(.75 == IOU_THRESHOLDS)[0]
    res = OrderedDict()
    res["AP"] = _mean(precision[:, :, :, 0])
    res["AP50"] = _mean(precision[t50][:, :, :, 0])
    res["AP75"] = _mean(precision[t75][:, :, :, 0])
    for name, a in (("APs", 1), ("APm", 2), ("APl", 3)):
        res[name] = _mean(precision[:, :, :, a])
    for f in LVIS_FREQUENCIES if frequencies is not None else ():
        res[f"AP{f}"] = _mean(precision[:, :, np.asarray([k for k, v in enumerate(frequencies) if v == f], dtype=np.int64), 0])
    s = precision[t50][:, :, :, 0]  # [1, R, K]
    for k in range(len(category_names)) if class_order is None else class_order:
        res[f"AP50_class_{category_names[k]}"] = _mean(s[:, :, [k]])
    for split, cats in class_splits.items():
        res[f"AP50_split_{split}"] = _mean(s[:, :, list(cats)])
    return res


def summarize(precision, category_names, class_splits, class_order=None):
    """``COCOeval.summarize``'s six AP numbers and ``COCOResults.update``'s per-class / per-split AP50 (coco_eval.py:364-404)
    -> OrderedDict.  category_names: the name of every category index; class_splits: {split: [category indices]};
    class_order: the category indices in the order their ``AP50_class_`` keys appear (None: index order)."""
    return _summarize(precision[..., MAX_DETS.index(100)], category_names, class_splits, class_order)


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


def summarize_lvis(precision, category_names, class_splits, frequencies, class_order=None, recall=None):
    """Rule 10 of include/ovis_hip.h -> OrderedDict: AP, AP50, AP75, APs, APm, APl, then APr, APc, APf (area "all" over the
    categories whose ``frequencies`` entry is r, c, f), AP50_class_<name> (``class_order`` as in ``summarize``) and
    AP50_split_<split>; ``recall`` (``accumulate_lvis``' second array): followed by AR@300, ARs@300, ARm@300, ARl@300 and
    AR@300_split_<split>.  The 300 of the keys is the cap the numbers are usually made with."""
    if len(category_names) != precision.shape[2] or len(frequencies) != precision.shape[2]:
        raise ValueError(f"summarize_lvis: {len(category_names)} names and {len(frequencies)} frequencies for a precision "
                         f"array of {precision.shape[2]} categories")
    res = _summarize(precision, category_names, class_splits, class_order, frequencies)
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


# ---- joining tables: consecutive chunks, and the shards of a run where every rank scores what it predicted ---------------
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
