"""TEST-ONLY: a six-image federatedly annotated (LVIS-style) dataset and a set of detections for it -- the smallest that has
every case LVIS-style scoring (include/ovis_hip.h, rules 1 to 10) must handle.  Only the annotation file is written: scoring
reads no pixels.

  id   w x h    annotations                                                     negatives     not exhaustive
   3   64 x 48  two overlapping of 2, one of 9, one of 5 with ``ignore: 1``      11, 14        9
   8   53 x 37  one of 5, one of 20 (two polygons)                               2, 23         --
  10   50 x 50  none                                                            2, 31         5
  15   60 x 40  RLE: a blob of 23, a box of 11 with ``iscrowd: 1`` (not read)    5             23
  21   45 x 33  one of 14 (no ``area`` key), two of 31 (one ``ignore: 1``)       9, 20         31
  30   64 x 48  one of 2 (area 1400: medium), one of 31                         5, 14, 23     2

Categories, in FILE order (not sorted): 8 ids over the frequencies f / c / r and the splits seen / unseen.  The detections
hold, per rule: strays of categories nobody looked for (dropped), hits on negatives (false positives), unmatched detections of
not-exhaustive categories (ignored), a second detection on an ``ignore`` ground truth and on the ``iscrowd`` one (false
positives, where COCO's crowd rule would ignore them), equal scores in two images (image-id order decides)."""
import json

import numpy as np

IMAGES = [(15, 60, 40), (3, 64, 48), (30, 64, 48), (8, 53, 37), (21, 45, 33), (10, 50, 50)]   # FILE order: (id, width, height)
SORTED_IDS = [3, 8, 10, 15, 21, 30]
CATEGORIES = [(20, "rare_seen", "r", "seen"), (2, "freq_seen", "f", "seen"), (9, "rare_unseen", "r", "unseen"),
              (5, "common_seen", "c", "seen"), (31, "common/seen two", "c", "seen"), (11, "freq_seen_b", "f", "seen"),
              (14, "common_unseen", "c", "unseen"), (23, "freq_unseen", "f", "unseen")]
FEDERATED = {3: ([11, 14], [9]), 8: ([2, 23], []), 10: ([2, 31], [5]), 15: ([5], [23]), 21: ([9, 20], [31]),
             30: ([5, 14, 23], [2])}   # image id -> (neg_category_ids, not_exhaustive_category_ids)


def _rect(x, y, w, h):
    return [[x, y, x + w, y, x + w, y + h, x, y + h]]


def blob():
    """The bitmap of image 15's ground truth of category 23: an ellipse, bool [40, 60]."""
    y, x = np.mgrid[0:40, 0:60]
    return ((x - 22) / 13.0) ** 2 + ((y - 18) / 10.0) ** 2 <= 1.0


def box_bitmap():
    mask = np.zeros((40, 60), dtype=bool)
    mask[1:31, 1:51] = True
    return mask


def rle_of(mask):
    """The uncompressed COCO RLE of a bool [H, W] bitmap: column-major runs, zeros first."""
    flat = np.asarray(mask, dtype=np.uint8).T.reshape(-1)
    cuts = np.flatnonzero(np.diff(flat)) + 1
    runs = np.diff(np.concatenate([[0], cuts, [len(flat)]])).tolist()
    return {"size": [int(mask.shape[0]), int(mask.shape[1])], "counts": ([0] if flat[0] else []) + runs}


def _bitmap_box(mask):
    ys, xs = np.nonzero(mask)
    return [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]


# FILE order: (annotation id, image, category, xywh box, segmentation, extra keys); ``area`` is w * h unless given here
ANNOTATIONS = [
    (4, 3, 5, [0, 30, 12, 12], _rect(0, 30, 12, 12), {"ignore": 1}),
    (1, 3, 2, [10, 10, 30, 20], _rect(10, 10, 30, 20), {}),
    (6, 8, 20, [30.5, 10, 12, 20], [[30.5, 10, 42, 10, 36, 18], [31, 20, 42, 20, 42, 29, 31, 29]], {}),
    (2, 3, 2, [12, 12, 30, 20], _rect(12, 12, 30, 20), {}),
    (3, 3, 9, [40, 5, 20, 12], _rect(40, 5, 20, 12), {}),
    (5, 8, 5, [5, 6, 20, 15], _rect(5, 6, 20, 15), {}),
    (7, 15, 23, _bitmap_box(blob()), rle_of(blob()), {"area": float(blob().sum())}),
    (8, 15, 11, [1, 1, 50, 30], rle_of(box_bitmap()), {"iscrowd": 1}),
    (9, 21, 14, [2, 3, 10, 10], _rect(2, 3, 10, 10), {"area": None}),     # None: the key is left out
    (10, 21, 31, [20, 5, 20, 20], _rect(20, 5, 20, 20), {}),
    (11, 21, 31, [22, 7, 16, 16], _rect(22, 7, 16, 16), {"ignore": 1}),
    (12, 30, 2, [5, 5, 40, 35], _rect(5, 5, 40, 35), {}),
    (13, 30, 31, [50, 30, 10, 10], _rect(50, 30, 10, 10), {})]

DETECTIONS = {   # image id -> [(json category id, score, xyxy at the FILE's scale)] in prediction order
    3: [(2, .9, [10, 10, 39, 29]), (2, .8, [12, 12, 41, 31]), (2, .7, [11, 11, 40, 30]), (9, .6, [0, 0, 5, 5]),
        (9, .5, [40, 5, 59, 16]), (11, .85, [20, 20, 40, 40]), (20, .95, [1, 1, 30, 30]), (5, .75, [0, 30, 11, 41]),
        (5, .65, [0, 30, 11, 41])],
    8: [(5, .9, [5, 6, 24, 20]), (20, .8, [30, 10, 41, 29]), (2, .7, [0, 0, 10, 10]), (31, .9, [0, 0, 10, 10])],
    10: [(2, .5, [5, 5, 30, 40]), (5, .9, [5, 5, 20, 20]), (31, .3, [10, 10, 20, 20])],
    15: [(23, .9, [9, 8, 35, 28]), (23, .4, [40, 30, 55, 38]), (11, .95, [1, 1, 50, 30]), (11, .5, [1, 1, 50, 30]),
         (5, .2, [3, 3, 10, 10])],
    21: [(14, .9, [2, 3, 11, 12]), (31, .5, [20, 5, 39, 24]), (31, .45, [22, 7, 37, 22]), (31, .42, [0, 0, 8, 8]),
         (9, .3, [5, 5, 15, 15])],
    30: [(2, .6, [5, 5, 44, 39]), (31, .5, [0, 0, 9, 9]), (31, .35, [50, 30, 59, 39]), (14, .8, [10, 10, 20, 20])],
}


def dataset_dict(degenerate=False):
    """The annotation file as a dict.  ``degenerate``: every image's negatives are ALL the categories absent from it,
    nothing is not-exhaustive, and no annotation has an ``ignore`` or ``iscrowd`` key -- the file on which LVIS-style and
    COCO scoring must agree."""
    anns = []
    for ann_id, image, cat, box, seg, extra in ANNOTATIONS:
        ann = {"id": ann_id, "image_id": image, "category_id": cat, "bbox": box, "segmentation": seg,
               "area": float(box[2] * box[3])}
        ann.update(extra)
        if ann["area"] is None:
            del ann["area"]
        if degenerate:
            ann.pop("ignore", None)
            ann.pop("iscrowd", None)
        anns.append(ann)
    images = []
    for image_id, w, h in IMAGES:
        neg, open_ = FEDERATED[image_id]
        if degenerate:
            present = {a["category_id"] for a in anns if a["image_id"] == image_id}
            neg, open_ = [c for c, _, _, _ in CATEGORIES if c not in present], []
        images.append({"id": image_id, "file_name": f"{image_id}.png", "width": w, "height": h, "neg_category_ids": list(neg),
                       "not_exhaustive_category_ids": list(open_)})
    cats = [{"id": c, "name": name, "frequency": f, "split": split} for c, name, f, split in CATEGORIES]
    return {"images": images, "categories": cats, "annotations": anns}


def write(path, data=None):
    with open(str(path), "w") as f:
        json.dump(dataset_dict() if data is None else data, f)
    return str(path)
