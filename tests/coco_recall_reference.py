"""TEST-ONLY: a scalar restatement of the RECALL half of pycocotools' ``COCOeval.accumulate`` and of the six AR lines of
``COCOeval.summarize``, over the match tables of tests/coco_eval_reference.py (its ``match_tables`` restates
``evaluateImg``).  Plain loops over problems, detections and thresholds; fp64 as pycocotools.

accumulate: for a category with an image entry and npig > 0 non-ignored ground truths in the area range, the detections of
every image are cut to the first maxDet (``dtMatches[:, 0:maxDet]``), tp counts the matched, non-ignored ones, and
``recall[t, k, a, m] = tp / npig`` after the last detection (``rc[-1]``), 0 when there is none; -1 otherwise.
summarize: ``_summarize(0, ...)`` takes ``recall[:, :, aind, mind]`` and averages the entries > -1."""
from collections import OrderedDict

import numpy as np

from tests.coco_eval_reference import AREA_RANGES, IOU_THRESHOLDS, MAX_DETS


def accumulate_recall(tables, num_categories):
    """recall fp64 [T, K, A, M]."""
    recall = -np.ones((len(IOU_THRESHOLDS), num_categories, len(AREA_RANGES), len(MAX_DETS)))
    for k in range(num_categories):
        problems = [p for p in range(len(tables["category"])) if tables["category"][p] == k]
        if not problems:
            continue
        for a in range(len(AREA_RANGES)):
            npig = 0
            for p in problems:
                for g in range(tables["gt_start"][p], tables["gt_start"][p + 1]):
                    npig += 0 if tables["gt_ignore"][a][g] else 1
            if npig == 0:
                continue
            for m, max_det in enumerate(MAX_DETS):
                for t in range(len(IOU_THRESHOLDS)):
                    tp, nd = 0.0, 0
                    for p in problems:
                        for d in range(tables["det_start"][p], min(tables["det_start"][p + 1], tables["det_start"][p] + max_det)):
                            nd += 1
                            if tables["dt_match"][a][t, d] >= 0 and not tables["dt_ignore"][a][t, d]:
                                tp += 1.0
                    recall[t, k, a, m] = tp / npig if nd else 0.0
    return recall


def _mean(values):
    values = np.asarray(values, dtype=np.float64)
    values = values[values > -1]
    return float(np.mean(values)) if values.size else -1.0


def summarize_recall(recall, category_names, class_splits):
    """AR1, AR10, AR100, ARs, ARm, ARl (stats[6:12] of COCOeval.summarize) and AR100_split_<split>."""
    m1, m10, m100 = (MAX_DETS.index(v) for v in (1, 10, 100))
    out = OrderedDict()
    out["AR1"], out["AR10"], out["AR100"] = (_mean(recall[:, :, 0, m]) for m in (m1, m10, m100))
    out["ARs"], out["ARm"], out["ARl"] = (_mean(recall[:, :, a, m100]) for a in (1, 2, 3))
    for split, cats in class_splits.items():
        out[f"AR100_split_{split}"] = _mean(recall[:, list(cats), 0, m100])
    return out
