"""Writes tests/golden/scorer_tables.npz and tests/golden/scorer_calls.json: the scorer's match tables (engine/coco_eval.py)
and the ``_C`` calls of a chunk, recorded on the device at the commit BEFORE the scorer was restructured
(python tests/golden/make_scorer_golden.py), so that tests/test_scorer_golden_gpu.py holds every later tree to that commit and
not to itself.  Only the public keyword signatures are used: ``match_tables`` and ``results_match_tables``.

The case: 4 images of two sizes (64 x 48 and 60 x 40: Boundary IoU dilations 2 and 1, and a 60 x 40 mask ends in a partial
64-bit word), 4 categories over two splits and three frequencies, a crowd, an ``ignore`` key, an RLE ground truth, an image
without a detection, a category with detections and no ground truth (9), equal scores inside a category, and the
``neg_category_ids`` / ``not_exhaustive_category_ids`` / ``frequency`` keys, so one file scores under both rule sets.  The
detections come as predictions (maps at twice the file's image sizes) and as results files (xywh boxes; RLE bitmaps).

Every configuration of ``CONFIGS`` runs once as one chunk and once with ``max_images=1``; of the one-chunk run the sequence of
``_C`` function names is kept too -- "same launches, same order" as a list of the project's own Python names."""
import contextlib
import json
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

TABLES_FILE, CALLS_FILE = os.path.join(HERE, "scorer_tables.npz"), os.path.join(HERE, "scorer_calls.json")
M, SCALE = 14, 2
IMAGES = [(15, 60, 40), (3, 64, 48), (30, 64, 48), (10, 60, 40)]  # FILE order: (id, width, height)
CATEGORIES = [(5, "common_seen", "c", "seen"), (2, "freq_seen", "f", "seen"), (9, "rare_unseen", "r", "unseen"),
              (23, "freq_unseen", "f", "unseen")]
FEDERATED = {3: ([9], [5]), 15: ([5], [23]), 30: ([2, 9], []), 10: ([23], [])}  # image -> (negatives, not exhaustive)
# the _C entries engine/coco_eval.py reaches, directly or through PolygonMasks.convert_to_binarymask
C_ENTRIES = ("CocoProblems", "paste_masks", "polygons_to_masks", "coco_pack_masks", "coco_rle_words", "coco_boundary_words",
             "coco_box_iou", "coco_mask_iou", "coco_boundary_iou", "coco_match", "lvis_match", "error_types")
ERRORS = {"error_thresholds": (0.5, 0.1)}
LVIS = {"rules": "lvis", "lvis_max_dets": 5}
BOTH = ("segm", "boundary")
# (name, "predictions" or "results", iou_type, keywords)
CONFIGS = [(f"{source}_{'+'.join((t,) if isinstance(t, str) else t)}{tag}", source, t, kw)
           for source in ("predictions", "results")
           for tag, kw, types in (("", {}, ("bbox", "segm", BOTH)), ("_lvis", LVIS, ("bbox", BOTH)),
                                  ("_errors", ERRORS, ("bbox", "segm")))
           for t in types]


def _rect(x, y, w, h):
    return [[x, y, x + w, y, x + w, y + h, x, y + h]]


def rle_of(mask):
    """The uncompressed COCO RLE of a bool [H, W] bitmap: column-major runs, zeros first."""
    flat = np.asarray(mask, dtype=np.uint8).T.reshape(-1)
    cuts = np.flatnonzero(np.diff(flat)) + 1
    runs = np.diff(np.concatenate([[0], cuts, [len(flat)]])).tolist()
    return {"size": [int(mask.shape[0]), int(mask.shape[1])], "counts": ([0] if flat[0] else []) + runs}


def _ellipse(height, width, cx, cy, rx, ry):
    y, x = np.mgrid[0:height, 0:width]
    return ((x - cx) / rx) ** 2 + ((y - cy) / ry) ** 2 <= 1.0


# FILE order: (annotation id, image, category, xywh box, segmentation, extra keys)
ANNOTATIONS = [
    (4, 3, 5, [0, 30, 12, 12], _rect(0, 30, 12, 12), {"iscrowd": 1}),
    (1, 3, 2, [10, 10, 30, 20], _rect(10, 10, 30, 20), {}),
    (2, 3, 2, [12, 12, 30, 20], _rect(12, 12, 30, 20), {}),
    (7, 15, 23, [9.0, 8.0, 27.0, 21.0], rle_of(_ellipse(40, 60, 22, 18, 13.0, 10.0)), {"area": 400.0}),
    (8, 15, 2, [30.5, 10, 12, 20], [[30.5, 10, 42, 10, 36, 18], [31, 20, 42, 20, 42, 29, 31, 29]], {"ignore": 1}),
    (12, 30, 5, [5, 5, 40, 35], _rect(5, 5, 40, 35), {}),
    (13, 30, 23, [50, 30, 10, 10], _rect(50, 30, 10, 10), {}),
    (14, 10, 2, [20, 5, 20, 20], _rect(20, 5, 20, 20), {})]

DETECTIONS = {  # image id -> [(json category id, score, xyxy at the FILE's scale)] in prediction order
    3: [(2, .9, [10, 10, 39, 29]), (2, .9, [12, 12, 41, 31]), (2, .7, [11, 11, 40, 30]), (5, .8, [0, 30, 11, 41]),
        (5, .6, [0, 30, 11, 41]), (9, .5, [40, 5, 59, 16]), (23, .4, [1, 1, 30, 30])],
    15: [(23, .9, [9, 8, 35, 28]), (23, .4, [40, 30, 55, 38]), (2, .6, [30, 10, 41, 29]), (5, .3, [3, 3, 10, 10])],
    30: [(5, .8, [6, 6, 44, 39]), (23, .5, [50, 30, 59, 39]), (9, .5, [10, 10, 20, 20]), (2, .45, [5, 5, 44, 39]),
         (5, .8, [30, 2, 60, 20])],
}


def dataset_dict():
    anns = []
    for ann_id, image, cat, box, seg, extra in ANNOTATIONS:
        anns.append(dict({"id": ann_id, "image_id": image, "category_id": cat, "bbox": box, "segmentation": seg,
                          "area": float(box[2] * box[3])}, **extra))
    images = [{"id": i, "file_name": f"{i}.png", "width": w, "height": h, "neg_category_ids": list(FEDERATED[i][0]),
               "not_exhaustive_category_ids": list(FEDERATED[i][1])} for i, w, h in IMAGES]
    cats = [{"id": c, "name": name, "frequency": f, "split": split} for c, name, f, split in CATEGORIES]
    return {"images": images, "categories": cats, "annotations": anns}


def make_case(folder):
    """-> (dataset, predictions in dataset-index order, {"bbox": results list, "segm": results list})."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList
    path = os.path.join(str(folder), "scorer_case.json")
    with open(path, "w") as f:
        json.dump(dataset_dict(), f)
    dataset = coco_eval.annotation_dataset(path)
    assert dataset.ids == sorted(i for i, _, _ in IMAGES) and list(dataset.class_splits) == ["seen", "unseen"]
    g = torch.Generator().manual_seed(11)
    predictions, results = [], {"bbox": [], "segm": []}
    for image_id in dataset.ids:
        info, dets = dataset.coco.imgs[image_id], DETECTIONS.get(image_id, [])
        pred = BoxList(torch.tensor([d[2] for d in dets], dtype=torch.float32).reshape(-1, 4) * SCALE,
                       (info["width"] * SCALE, info["height"] * SCALE))
        pred.add_field("scores", torch.tensor([d[1] for d in dets], dtype=torch.float32))
        pred.add_field("labels", torch.tensor([dataset.json_category_id_to_contiguous_id[d[0]] for d in dets], dtype=torch.int64))
        maps = torch.rand(len(dets), 1, M, M, generator=g)
        maps[:, :, 2:M - 2, 2:M - 2] = 0.9
        maps[0::2] = 0.9  # every other one crisp: the pasted mask is the box
        pred.add_field("mask", maps)
        predictions.append(pred)
        for k, (cat, score, (x1, y1, x2, y2)) in enumerate(dets):
            w, h = x2 - x1 + 1, y2 - y1 + 1
            mask = np.zeros((info["height"], info["width"]), dtype=bool)
            mask[y1:y2 + 1, x1:x2 + 1] = True
            if k % 2:  # every other one round
                mask &= _ellipse(info["height"], info["width"], x1 + w / 2.0, y1 + h / 2.0, w / 2.0, h / 2.0)
            results["bbox"].append({"image_id": image_id, "category_id": cat, "score": score, "bbox": [x1, y1, w, h]})
            results["segm"].append({"image_id": image_id, "category_id": cat, "score": score, "segmentation": rle_of(mask)})
    return dataset, predictions, results


@contextlib.contextmanager
def recorded_calls(calls):
    """Appends the name of every ``C_ENTRIES`` call to ``calls`` while inside."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    real = {entry: getattr(_C, entry) for entry in C_ENTRIES}

    class Problems(real["CocoProblems"]):
        def __init__(self, *a, **k):
            calls.append("CocoProblems")
            super().__init__(*a, **k)

    def wrapper(entry):
        def counted(*a, **k):
            calls.append(entry)
            return real[entry](*a, **k)
        return counted
    try:
        for entry in C_ENTRIES:
            setattr(_C, entry, Problems if entry == "CocoProblems" else wrapper(entry))
        yield
    finally:
        for entry, fn in real.items():
            setattr(_C, entry, fn)


def score_all(device="cuda"):
    """-> ({"<config>/<one or per_image>/<iou type>/<array>": array}, {config: the _C calls of its one-chunk run})."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    arrays, calls = {}, {}
    with tempfile.TemporaryDirectory() as folder:
        dataset, predictions, results = make_case(folder)
        for name, source, iou_type, keywords in CONFIGS:
            for chunking, max_images in (("one", None), ("per_image", 1)):
                seen = []
                with recorded_calls(seen):
                    if source == "predictions":
                        tables, _ = coco_eval.match_tables(dataset, predictions, iou_type, device, max_images=max_images, **keywords)
                    else:
                        tables, _ = coco_eval.results_match_tables(dataset, results["bbox" if iou_type == "bbox" else "segm"],
                                                                   iou_type, device, max_images=max_images, **keywords)
                if chunking == "one":
                    calls[name] = seen
                for task, table in ({iou_type: tables} if isinstance(iou_type, str) else tables).items():
                    for key, value in table.items():
                        arrays[f"{name}/{chunking}/{task}/{key}"] = np.asarray(value)
    return arrays, calls


if __name__ == "__main__":
    arrays, calls = score_all()
    np.savez_compressed(TABLES_FILE, **arrays)
    with open(CALLS_FILE, "w") as f:
        json.dump(calls, f, indent=0, sort_keys=True)
    print(f"{len(arrays)} arrays of {len(CONFIGS)} configurations -> {TABLES_FILE} ({os.path.getsize(TABLES_FILE)} bytes), {CALLS_FILE}")
    for name in sorted(calls):
        print(name, len(calls[name]), "calls;", "detections", arrays[f"{name}/one/{name.split('_')[1].split('+')[0]}/scores"].shape[0])
