"""COCO box / mask AP and the seen / unseen AP50 of a prediction list -- the dataset-specific ``evaluate`` the reference
runs after ``inference`` (maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py: ``prepare_for_coco_detection``
:71-105, ``prepare_for_coco_segmentation`` :108-162, ``evaluate_predictions_on_coco`` :315-333, ``COCOResults`` :336-414).

The reference hands JSON results to pycocotools' ``COCOeval``; pycocotools is not a dependency here, its rules are restated:

* on the DEVICE (csrc/coco_eval.hip through ``_C``), a chunk of images at a time: the detections' masks are pasted at
  image size (``_C.paste_masks``) and the polygon ground truth rasterised (``_C.polygons_to_masks``) per image size,
  packed to bit words, and then three launches cover the whole chunk -- box IoU or mask IoU of every (image, category)
  problem, and ``COCOeval.evaluateImg``'s matching for every problem, area range and IoU threshold.  Only the match tables
  come back: 4 x 10 x (an int32 and a flag) per detection.
* on the HOST, in NumPy fp64: ``COCOeval.accumulate`` and ``summarize`` (``accumulate`` / ``summarize`` of
  engine/coco_tables.py, which describes the match tables and needs no device; its names are importable from here), term
  by term -- O(detections), not hot.  A public entry turns its scoring keywords into one ``ScoringOptions``, which everything
  below takes; a chunk is scored in five stages (``_chunk_tables``).

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

ERROR ANALYSIS.  ``error_thresholds=(t_f, t_b)`` (default None: nothing changes) adds, for bbox and segm under ``rules="coco"``,
one IoU call on a table with one row per image and ``_C.error_types`` (csrc/error_types.hip); the tables then carry the error
arrays, which engine/error_analysis.py turns into dAP50 per error type.

SHARDED.  ``evaluate_coco_sharded`` is ``evaluate_coco`` for a caller that holds one rank's {dataset index: BoxList} (a training
run's periodic evaluation, engine/evaluation.py): every rank scores what it predicted and only the match tables travel.
"""
import contextlib
import dataclasses
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
from .coco_tables import (AREA_RANGES, IOU_THRESHOLDS, LVIS_FREQUENCIES, LVIS_METRICS, LVIS_RECALL_METRICS,  # noqa: F401
                          MAX_DETS, METRICS, RECALL_METRICS, RECALL_THRESHOLDS, _accumulated, _mean, _sampled_precision,
                          accumulate, accumulate_lvis, accumulate_recall, concatenate_tables, format_results,
                          merge_shard_tables, shard_owners, summarize, summarize_lvis, summarize_recall)

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


@dataclasses.dataclass(frozen=True)
class ScoringOptions:
    """What the caller chose about HOW to score, made once by the public entry that was called (``_options``) and handed
    down as it is -- to the helpers, and to the public entries below it through their ``options`` keyword: a new scoring option
    is a field here, its one use, and a keyword of the public entries that offer it -- not a parameter of every layer."""
    rules: str = "coco"
    lvis_max_dets: int = LVIS_MAX_DETS  # lvis: the image's cap over all categories (negative: none)
    boundary_dilation_ratio: float = BOUNDARY_DILATION_RATIO
    error_thresholds: tuple = None  # (t_f, t_b): also type the errors (engine/error_analysis.py)


def _options(who, rules="coco", lvis_max_dets=LVIS_MAX_DETS, boundary_dilation_ratio=BOUNDARY_DILATION_RATIO,
             error_thresholds=None, options=None):
    """The entry ``who``'s scoring keywords, checked, as a ``ScoringOptions`` -- or ``options``, the record an entry above made."""
    if options is not None:
        return options
    if rules not in RULES:
        raise ValueError(f"{who}: rules '{rules}' is not supported ({', '.join(RULES)})")
    if error_thresholds is not None:
        if rules != "coco":
            raise ValueError(f"{who}: the error analysis follows COCO's rules only (rules='coco')")
        error_thresholds = tuple(float(t) for t in error_thresholds)
    return ScoringOptions(rules, lvis_max_dets, boundary_dilation_ratio, error_thresholds)


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


def _passes(iou_types):
    """``_jobs`` with every pass as the tuple of its names."""
    return [job if job == MASK_IOU_TYPES else (job,) for job in _jobs(iou_types)]


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


def _ground_truth(dataset, options=ScoringOptions()):
    """-> (category ids sorted, per image of the file in id order a record of its annotations sorted by category index,
    stably: annotation order inside a category).  ``options.rules == "lvis"`` (rules 1 and 2 of include/ovis_hip.h): every
    record also holds ``neg`` and ``not_exhaustive`` (int64 arrays of category indices, sorted) and ``ignore`` (the
    annotations' ``ignore`` keys), its ``crowd`` is all zero (``iscrowd`` is not read), and an image without either list or a
    category without ``frequency`` is a ValueError that names it."""
    coco = dataset.coco
    cat_ids = coco.cat_ids()
    cat_index = {c: i for i, c in enumerate(cat_ids)}
    lvis = options.rules == "lvis"
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


def _kept_rows(cats, scores, image, options):
    """The detections of one image that are scored, as indices into ``cats`` / ``scores`` sorted by (category index,
    descending score), stably: ties keep the input order.  coco: at most 100 per category.  lvis (rules 3 to 5 of
    include/ovis_hip.h): the ``options.lvis_max_dets`` best of the image over all categories together (negative: all), and of
    those the ones whose category is a negative of the image or has a ground truth in it."""
    if options.rules != "lvis":
        order = np.lexsort((-scores, cats))
        rank = np.arange(len(order)) - np.searchsorted(cats[order], cats[order], side="left")
        return order[rank < MAX_DETS[-1]]
    order = np.argsort(-scores, kind="mergesort")
    if options.lvis_max_dets >= 0:
        order = order[:options.lvis_max_dets]
    order = order[np.isin(cats[order], np.union1d(image["neg"], image["cats"]))]
    return order[np.lexsort((-scores[order], cats[order]))]  # equal scores stay in the order the first sort left them in


def _detection_rows(dataset, by_image, ground_truth, with_masks, options=ScoringOptions()):
    """The detection rows of {image id: prediction} for the image records of ``ground_truth`` = (category ids, records) --
    whoever holds predictions, all of them or a shard's, makes its rows here.  Per image: sorted by (category index, descending
    score), stably, at most 100 per category (coco_eval.py:71-105 / :108-162 and the ``dt[0:maxDets[-1]]`` of
    COCOeval.computeIoU); lvis: the image's cap and the federated filter instead (``_kept_rows``)."""
    cat_ids, images = ground_truth
    cat_index = {c: i for i, c in enumerate(cat_ids)}
    label_to_cat = {label: cat_index[json_id] for label, json_id in dataset.contiguous_category_id_to_json_id.items()}
    rows = []
    for image in images:
        pred = by_image.get(image["id"])
        if pred is None or len(pred) == 0:
            rows.append({"cats": np.zeros(0, np.int64), "scores": np.zeros(0), "xywh": np.zeros((0, 4)), "xyxy": None,
                         "maps": None})
            continue
        xyxy, xywh = detection_boxes(pred, image["width"], image["height"])
        scores = pred.get_field("scores").detach().cpu().double().numpy()
        cats = np.asarray([label_to_cat[int(l)] for l in pred.get_field("labels").tolist()], dtype=np.int64)
        order = _kept_rows(cats, scores, image, options)  # stable: ties keep prediction order
        rows.append({"cats": cats[order], "scores": scores[order], "xywh": xywh.double().numpy()[order], "xyxy": None,
                     "maps": None})
        if with_masks:
            index = torch.from_numpy(order)
            rows[-1]["maps"], rows[-1]["xyxy"] = mask_maps(pred).detach().cpu()[index, 0].float(), xyxy[index]
    return rows


def load_coco_results(dataset, results, iou_type, rules="coco", lvis_max_dets=LVIS_MAX_DETS, images=None, options=None):
    """The detections of a COCO results file as per-image rows, for the images of ``_ground_truth(dataset)`` in its order
    (pycocotools' ``loadRes`` and the ``dt[0:maxDets[-1]]`` of COCOeval): ``results`` is a path or the parsed list of
    {"image_id", "category_id", "score", "bbox" (xywh) or "segmentation" ({"size": [h, w], "counts": str or list})}.  Rows
    are what ``_detection_rows`` makes: sorted by (category index, descending score), stably in file order, at most 100 per
    category and image.  bbox: ``xywh`` as written (the area is w * h).  segm: ``rle`` holds the rows' segmentation dicts in
    place of ``maps`` / ``xyxy`` (the area comes from the decoder); ``entry`` is every row's index in the file.  Entries of
    a category the annotation file does not have are dropped (COCOeval never evaluates them).  ValueError, naming the
    entry: an image_id the file does not have, a polygon segmentation, a ``size`` that is not the image's, a missing key.
    ``rules="lvis"``: ``_kept_rows``' cap and filter instead; ``images``: ``_ground_truth``'s records when the caller has them."""
    _check_iou_type(iou_type, "load_coco_results")
    options = _options("load_coco_results", rules, lvis_max_dets, options=options)
    if options.rules == "lvis" and images is None:
        images = _ground_truth(dataset, options)[1]  # boundary: the rows of segm, it scores the same segm.json
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
        order = _kept_rows(cats, scores, images[position] if options.rules == "lvis" else None, options)
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


class _MaskSide:
    """The packed masks of one side of a chunk, its detections or its ground truths (they differ only in where a group's
    words come from: ``_detection_group``, ``_ground_truth_group``), filled one image-size group at a time and joined once.
    ``base``: the words so far, which is where the next group's first mask starts; ``boundary_ratio``: None, or the dilation
    ratio its boundary words are made with."""

    def __init__(self, num_rows, device, timer, boundary_ratio):
        self.device, self.timer, self.boundary_ratio, self.base = device, timer, boundary_ratio, 0
        self.parts, self.boundary_parts = [], []  # the boundary words lie as the mask words do
        self.areas = torch.zeros(num_rows, dtype=torch.int64, device=device)
        self.boundary_areas = torch.zeros_like(self.areas)

    def add(self, rows, words, areas):
        """``words`` int64 [n, words per mask] and ``areas`` int64 [n] of the chunk's rows ``rows`` (int64 [n], on the device)."""
        self.rows = rows
        self.parts.append(words.reshape(-1))
        self.areas[rows] = areas
        self.base += words.numel()

    def pack(self, rows, masks, rle=None):
        """``add`` of what the byte ``masks`` pack to, the words of ``rle`` = (rows of ``masks``, words, areas) substituted."""
        with _stage(self.timer, "pack"):
            rows = torch.from_numpy(rows).to(self.device)  # ahead of the launch: the copy waits for what is queued before it
            words, areas = _C.coco_pack_masks(masks)
            if rle is not None:
                words[rle[0]], areas[rle[0]] = rle[1], rle[2]
            self.add(rows, words, areas)

    def boundary(self, height, width):
        """The boundary words and areas (``_C.coco_boundary_words``) of the group added last, where they are asked for."""
        if self.boundary_ratio is None:
            return
        nwords = (height * width + 63) // 64
        with _stage(self.timer, "boundary"):
            bwords, bareas = _C.coco_boundary_words(self.parts[-1].view(-1, nwords), height, width,
                                                    boundary_dilation(height, width, self.boundary_ratio))
        self.boundary_parts.append(bwords.reshape(-1))
        self.boundary_areas[self.rows] = bareas

    def words(self, boundary=False):
        """The mask (or boundary) words of all groups as one flat buffer."""
        parts = self.boundary_parts if boundary else self.parts
        return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64, device=self.device)


def _detection_group(side, rows, members, images, dets, height, width):
    """The detections of the images ``members`` (one image size; chunk rows ``rows``, host int64) into ``side``: the RLEs of a
    results file decode straight to the words, the maps of predictions are pasted and packed."""
    with_dets = [i for i in members if len(dets[i]["cats"])]
    if dets[with_dets[0]].get("rle") is not None:
        names = [f"results entry {k} (image_id {images[i]['id']})" for i in with_dets for k in dets[i]["entry"]]
        with _stage(side.timer, "decode"):
            words, areas = _decode_rle([s for i in with_dets for s in dets[i]["rle"]], names, height, width, side.device)
        side.add(torch.from_numpy(rows).to(side.device), words, areas)
        return
    maps = torch.cat([dets[i]["maps"] for i in with_dets]).to(side.device)
    boxes = torch.cat([dets[i]["xyxy"] for i in with_dets]).to(side.device)
    with _stage(side.timer, "paste"):
        pasted = _C.paste_masks(maps, boxes, (height, width))
    side.pack(rows, pasted)


def _ground_truth_group(side, rows, members, images, height, width):
    """The ground truths of the images ``members`` into ``side``: polygons are rasterised and packed; RLE annotations are
    decoded on the device to the words their (empty) rows of the rasterised masks give way to."""
    anns = [a for i in members for a in images[i]["anns"]]
    for a in anns:
        if "segmentation" not in a:
            raise ValueError(f"evaluate_coco: annotation {a.get('id')} has no 'segmentation' (segm scoring)")
    polygons = PolygonMasks([[] if isinstance(a["segmentation"], dict) else a["segmentation"] for a in anns],
                            (width, height)).to(side.device)
    with _stage(side.timer, "rasterise"):
        masks = polygons.convert_to_binarymask()
    rle_rows = [r for r, a in enumerate(anns) if isinstance(a["segmentation"], dict)]
    rle = None
    if rle_rows:
        for r in rle_rows:
            seg = anns[r]["segmentation"]
            if list(seg.get("size", [height, width])) != [height, width]:
                raise ValueError(f"RLE of size {seg.get('size')} on an image of {height} x {width}")
        with _stage(side.timer, "decode"):
            rle = (torch.tensor(rle_rows, device=side.device),) + _decode_rle(
                [anns[r]["segmentation"] for r in rle_rows], [f"annotation {anns[r].get('id')}" for r in rle_rows],
                height, width, side.device)
    side.pack(rows, masks, rle)


def _problem_table(images, dets):
    """Stage 1 -> (table int64 [P, 10]: the 8 columns of ``_C.CocoProblems``, the word columns still 0, then the problem's
    category index and its image inside the chunk; the first detection row of every image; its first ground-truth row)."""
    rows, det_base, gt_base, iou_off, det_image_base, gt_image_base = [], 0, 0, 0, [], []
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
    return np.asarray(rows, dtype=np.int64).reshape(-1, 10), det_image_base, gt_image_base


def _mask_sides(images, dets, table, det_image_base, gt_image_base, boundary_ratio, device, timer):
    """Stage 2 for masks, one image size at a time -> (the detections' ``_MaskSide``, the ground truths', image -> (first det
    word, first gt word, words per mask)), and the word columns of ``table`` filled in.  ``boundary_ratio``: as ``_MaskSide``."""
    groups = {}
    for i, image in enumerate(images):
        groups.setdefault((image["height"], image["width"]), []).append(i)
    det_side = _MaskSide(sum(len(d["cats"]) for d in dets), device, timer, boundary_ratio)
    gt_side = _MaskSide(sum(len(im["cats"]) for im in images), device, timer, boundary_ratio)
    image_words = {}
    for (height, width), members in groups.items():
        nwords = (height * width + 63) // 64
        det_rows = np.concatenate([np.arange(len(dets[i]["cats"])) + det_image_base[i] for i in members])
        gt_rows = np.concatenate([np.arange(len(images[i]["cats"])) + gt_image_base[i] for i in members])
        d_off, g_off = det_side.base, gt_side.base
        for i in members:
            image_words[i] = (d_off, g_off, nwords)
            d_off += len(dets[i]["cats"]) * nwords
            g_off += len(images[i]["cats"]) * nwords
        if len(det_rows):
            _detection_group(det_side, det_rows, members, images, dets, height, width)
            det_side.boundary(height, width)
        if len(gt_rows):
            _ground_truth_group(gt_side, gt_rows, members, images, height, width)
            gt_side.boundary(height, width)
    if len(table):  # the word columns of every problem, from its image's share of the word buffers
        img = table[:, 9]
        first = np.asarray([image_words[i] for i in range(len(images))], dtype=np.int64).reshape(-1, 3)
        table[:, 7] = first[img, 2]
        table[:, 5] = first[img, 0] + (table[:, 0] - np.asarray(det_image_base)[img]) * table[:, 7]
        table[:, 6] = first[img, 1] + (table[:, 2] - np.asarray(gt_image_base)[img]) * table[:, 7]
    return det_side, gt_side, image_words


def _image_problems(images, dets, det_image_base, gt_image_base, image_words, device):
    """The chunk's image-level table (error analysis): ``CocoProblems`` with one row per image -- all its detection rows
    against all its ground-truth rows; ``image_words``: what ``_mask_sides`` returns, or None for boxes."""
    rows, off = [], 0
    for i, (image, det) in enumerate(zip(images, dets)):
        nd, ng = len(det["cats"]), len(image["cats"])
        rows.append([det_image_base[i], nd, gt_image_base[i], ng, off] + list(image_words[i] if image_words else (0, 0, 0)))
        off += nd * ng
    return _C.CocoProblems(np.asarray(rows, dtype=np.int64).reshape(-1, 8), device)


def _chunk_tables(images, dets, types, device, timer, options):
    """{name: match tables} of one chunk for the names ``types`` of one pass, in five stages: the problem table; the box
    rows or the mask words of the two sides; the IoU buffers -- per problem, image-level for the error analysis, boundary;
    the matching per name; the error arrays."""
    with_masks, boundary, errors = types[0] != "bbox", "boundary" in types, options.error_thresholds is not None
    table, det_image_base, gt_image_base = _problem_table(images, dets)  # stage 1
    crowd = torch.from_numpy(np.concatenate([im["crowd"] for im in images] + [np.zeros(0, np.uint8)])).to(device)
    if options.rules == "lvis":  # crowd is all zero here: no IoU takes the crowd form
        gt_ignore_in = torch.from_numpy(np.concatenate([im["ignore"] for im in images] + [np.zeros(0, np.uint8)])).to(device)
        open_flags = np.asarray([c in images[i]["not_exhaustive"] for c, i in zip(table[:, 8], table[:, 9])], dtype=np.uint8)
        not_exhaustive = torch.from_numpy(open_flags.reshape(-1)).to(device)
    gt_areas = torch.from_numpy(np.concatenate([im["areas"] for im in images] + [np.zeros(0)])).to(device)
    scores = np.concatenate([d["scores"] for d in dets] + [np.zeros(0)])
    iou = {}  # name -> the flat IoU buffer its matching reads
    if not with_masks:  # stages 2 and 3 for boxes: the rows, then the IoU of every problem and of every image
        det_xywh = torch.from_numpy(np.concatenate([d["xywh"] for d in dets] + [np.zeros((0, 4))])).to(device)
        gt_xywh = torch.from_numpy(np.concatenate([im["boxes"] for im in images] + [np.zeros((0, 4))])).to(device)
        problems = _C.CocoProblems(table[:, :8], device)
        with _stage(timer, "iou"):
            iou["bbox"] = _C.coco_box_iou(det_xywh, gt_xywh, crowd, problems)
            det_areas = det_xywh[:, 2] * det_xywh[:, 3]
        if errors:
            image_problems = _image_problems(images, dets, det_image_base, gt_image_base, None, device)
            with _stage(timer, "image_iou"):
                image_iou = _C.coco_box_iou(det_xywh, gt_xywh, crowd, image_problems)
    else:  # stages 2 and 3 for masks
        det_side, gt_side, image_words = _mask_sides(images, dets, table, det_image_base, gt_image_base,
                                                     options.boundary_dilation_ratio if boundary else None, device, timer)
        problems = _C.CocoProblems(table[:, :8], device)
        det_words, gt_words = det_side.words(), gt_side.words()
        if "segm" in types:
            with _stage(timer, "iou"):
                iou["segm"] = _C.coco_mask_iou(det_words, det_side.areas, gt_words, gt_side.areas, crowd, problems)
            if errors:  # the same words once more, addressed image by image
                image_problems = _image_problems(images, dets, det_image_base, gt_image_base, image_words, device)
                with _stage(timer, "image_iou"):
                    image_iou = _C.coco_mask_iou(det_words, det_side.areas, gt_words, gt_side.areas, crowd, image_problems)
        if boundary:
            with _stage(timer, "boundary_iou"):
                iou["boundary"] = _C.coco_boundary_iou(det_words, det_side.words(boundary=True), det_side.areas,
                                                       det_side.boundary_areas, gt_words, gt_side.words(boundary=True),
                                                       gt_side.areas, gt_side.boundary_areas, crowd, problems)
        det_areas = det_side.areas.double()  # boundary too: the area ranges stay those of the masks
    thresholds = torch.from_numpy(IOU_THRESHOLDS).to(device)
    area_ranges = torch.from_numpy(AREA_RANGES).to(device)
    if errors:
        det_cat = torch.from_numpy(np.concatenate([d["cats"] for d in dets] + [np.zeros(0, np.int64)]).astype(np.int32)).to(device)
        gt_cat = torch.from_numpy(np.concatenate([im["cats"] for im in images] + [np.zeros(0, np.int64)]).astype(np.int32)).to(device)
        det_gt_base = torch.from_numpy(np.repeat(table[:, 2], table[:, 1]).astype(np.int32)).to(device)
        det_image = np.repeat(np.arange(len(images)), [len(d["cats"]) for d in dets])
        gt_image = np.repeat(np.arange(len(images)), [len(im["cats"]) for im in images])
    tables = {}
    for name in types:  # stages 4 and 5
        with _stage(timer, "match"):
            if options.rules == "lvis":
                dt_match, dt_ignore, gt_ignore = _C.lvis_match(iou[name], problems, det_areas, gt_areas, gt_ignore_in,
                                                               not_exhaustive, area_ranges, thresholds)
            else:
                dt_match, dt_ignore, gt_ignore = _C.coco_match(iou[name], problems, det_areas, gt_areas, crowd, area_ranges,
                                                               thresholds)
        tables[name] = {"category": table[:, 8].copy(), "det_start": np.concatenate([table[:, 0], [len(scores)]]),
                        "gt_start": np.concatenate([table[:, 2], [gt_areas.numel()]]), "scores": scores,
                        "dt_match": dt_match.cpu().numpy(), "dt_ignore": dt_ignore.cpu().numpy(),
                        "gt_ignore": gt_ignore.cpu().numpy()}
        if errors and name != "boundary":
            with _stage(timer, "error_types"):
                base = dt_match[0, 0]  # the ground truth's index inside its problem -> its row in the chunk
                err_type, err_gt, gt_missed = _C.error_types(
                    image_iou, image_problems, det_cat, torch.where(base >= 0, base + det_gt_base, base),
                    dt_ignore[0, 0].view(torch.uint8), gt_cat, crowd, *options.error_thresholds)
            tables[name].update(err_type=err_type.cpu().numpy(), err_gt=err_gt.cpu().numpy(), gt_missed=gt_missed.cpu().numpy(),
                                det_image=det_image, gt_image=gt_image, num_images=len(images))
    return tables


def _as_asked(tables, iou_type):
    """{name: tables} as the public entries return it: the tables themselves when ``iou_type`` is a name."""
    return tables[iou_type] if isinstance(iou_type, str) else tables


def score_chunk(images, dets, iou_type, device, timer=None, boundary_dilation_ratio=BOUNDARY_DILATION_RATIO, rules="coco",
                error_thresholds=None, options=None):
    """The match tables of one chunk of images (the structure: engine/coco_tables.py; the stages: ``_chunk_tables``): a
    constant number of launches -- box or mask IoU and the matching -- plus, for masks, the paste / rasterise / decode / pack
    calls of every image size, and what boundary, ``rules="lvis"`` and ``error_thresholds=(t_f, t_b)`` add to them (the
    module's docstring; default: not a key, not a launch).  ``images`` / ``dets``: of ``_ground_truth`` and ``_detection_rows`` or
    ``load_coco_results`` under the same rules; a malformed RLE raises a ValueError that names the entry or the annotation.
    ``iou_type`` may be the tuple ("segm", "boundary"): the words are made once, both IoU buffers are matched -- with the MASK
    areas -- and {name: tables} comes back.  The error analysis counts the rows' images inside the chunk and leaves
    boundary's tables alone."""
    options = _options("evaluate_coco", rules, LVIS_MAX_DETS, boundary_dilation_ratio, error_thresholds, options)
    return _as_asked(_chunk_tables(images, dets, _job_types(iou_type, "evaluate_coco"), device, timer, options), iou_type)


def _job_types(iou_type, who):
    """The names of one scoring pass: ``iou_type`` itself, or the members of the tuple ("segm", "boundary")."""
    types = (iou_type,) if isinstance(iou_type, str) else tuple(iou_type)
    for t in types:
        _check_iou_type(t, who)
    if len(types) != 1 and types != MASK_IOU_TYPES:
        raise ValueError(f"{who}: one pass scores one iou_type or {MASK_IOU_TYPES}, not {types}")
    return types


def _score_rows(images, dets, types, device, options=ScoringOptions(), budget=None, timer=None, max_images=None):
    """{name: match tables} of the images' ground truth and detection rows for the names ``types`` of one pass, chunk by
    chunk.  ``budget``: the bytes of device memory a chunk may plan with (None: a quarter of what is free)."""
    budget = torch.cuda.mem_get_info(device)[0] // 4 if budget is None else budget
    # through the public name, which is where a caller counts or replaces the chunks
    parts = [score_chunk([images[i] for i in chunk], [dets[i] for i in chunk], types, device, timer, options=options)
             for chunk in _chunks(images, dets, types[0] != "bbox", budget, max_images, "boundary" in types,
                                  options.error_thresholds is not None)]
    return {name: concatenate_tables([part[name] for part in parts]) for name in types}


def match_tables(dataset, predictions, iou_type, device, budget=None, timer=None, max_images=None, ground_truth=None,
                 boundary_dilation_ratio=BOUNDARY_DILATION_RATIO, rules="coco", lvis_max_dets=LVIS_MAX_DETS,
                 error_thresholds=None, options=None):
    """-> (the match tables of every (image, category) problem of the annotation file, in image-id order; the sorted
    category ids).  ``budget``: the bytes of device memory a chunk may plan with (None: a quarter of what is free);
    ``max_images``: the most images of a chunk (None: MAX_CHUNK_IMAGES); ``ground_truth``: ``_ground_truth`` under the same
    rules when the caller already has it.  ``iou_type``: bbox, segm, boundary, or the tuple ("segm", "boundary") -- then the
    first item is {name: tables}, both from one set of mask words per chunk.  ``rules``, ``lvis_max_dets``,
    ``error_thresholds``: as in ``evaluate_coco``; with the last, the tables of bbox and segm carry the error arrays."""
    types = _job_types(iou_type, "evaluate_coco")
    options = _options("evaluate_coco", rules, lvis_max_dets, boundary_dilation_ratio, error_thresholds, options)
    if len(predictions) > len(dataset):
        raise ValueError(f"evaluate_coco: {len(predictions)} predictions for a dataset of {len(dataset)} images")
    ground_truth = ground_truth if ground_truth is not None else _ground_truth(dataset, options)
    by_image = {dataset.id_to_img_map[idx]: pred for idx, pred in enumerate(predictions)}
    dets = _detection_rows(dataset, by_image, ground_truth, types[0] != "bbox", options)
    tables = _score_rows(ground_truth[1], dets, types, torch.device(device), options, budget, timer, max_images)
    return _as_asked(tables, iou_type), ground_truth[0]


def results_match_tables(dataset, results, iou_type, device, budget=None, timer=None, max_images=None, ground_truth=None,
                         boundary_dilation_ratio=BOUNDARY_DILATION_RATIO, rules="coco", lvis_max_dets=LVIS_MAX_DETS,
                         error_thresholds=None, options=None):
    """``match_tables`` for the detections of a results file (``results``: what ``load_coco_results`` takes)."""
    types = _job_types(iou_type, "evaluate_coco_results")
    options = _options("evaluate_coco_results", rules, lvis_max_dets, boundary_dilation_ratio, error_thresholds, options)
    cat_ids, images = ground_truth if ground_truth is not None else _ground_truth(dataset, options)
    dets = load_coco_results(dataset, results, types[0], images=images, options=options)
    tables = _score_rows(images, dets, types, torch.device(device), options, budget, timer, max_images)
    return _as_asked(tables, iou_type), cat_ids


def _scoring_device(device, who):
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{who}: scoring runs on the HIP device (IoU and matching have no host implementation)")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def _summaries(dataset, iou_types, device, tables_of, options, recall=False, ground_truth=None, tables_out=None):
    """{iou_type: ``summarize`` of ``accumulate`` of its match tables} with the dataset's names, splits and class order;
    ``recall``: followed by ``summarize_recall`` of the same walk's recall; lvis: ``summarize_lvis`` of ``accumulate_lvis``.
    ``tables_of(names, ground truth)`` -> ({name: tables}, category ids) is called once per pass of ``_passes``."""
    results, scored = OrderedDict(), {}
    ground_truth = ground_truth if ground_truth is not None else _ground_truth(dataset, options)
    frequencies = category_frequencies(dataset) if options.rules == "lvis" else None
    cat_ids = ground_truth[0]
    cat_index = {c: i for i, c in enumerate(cat_ids)}
    names = [dataset.categories[c] for c in cat_ids]
    splits = OrderedDict((split, [cat_index[c] for c in ids]) for split, ids in dataset.class_splits.items())
    class_order = [cat_index[c] for c in dataset.categories if c in cat_index]
    with torch.cuda.device(device):
        for types in _passes(iou_types):
            scored.update(tables_of(types, ground_truth)[0])
        if tables_out is not None:  # the caller goes on with the match tables themselves (engine/error_analysis.py)
            tables_out.update(scored, cat_ids=cat_ids)
        for iou_type in iou_types:
            if options.rules == "lvis":
                precision, recalls = accumulate_lvis(scored[iou_type], len(cat_ids))
                results[iou_type] = summarize_lvis(precision, names, splits, frequencies, class_order, recalls if recall else None)
                continue
            precision, recalls = _accumulated(scored[iou_type], len(cat_ids), MAX_DETS)
            results[iou_type] = summarize(precision, names, splits, class_order)
            if recall:
                results[iou_type].update(summarize_recall(recalls, names, splits))
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

    ``"boundary"`` among ``iou_types`` (Boundary AP, ``boundary_dilation_ratio`` of the image diagonal deep) and
    ``rules="lvis"`` (LVIS-style federated scoring, at most ``lvis_max_dets`` detections per image over all categories,
    negative: no cap; the keys are AP ... APl, APr, APc, APf, AP50_class_<name>, AP50_split_<split>, with ``recall`` AR@300,
    ARs@300, ARm@300, ARl@300, AR@300_split_<split>): the module's docstring and include/ovis_hip.h.

    ``error_thresholds=(t_f, t_b)`` with ``tables_out={}`` (``rules="coco"`` only): the same pass also types the errors
    (``score_chunk``), and ``tables_out`` receives {iou_type: match tables} and ``cat_ids`` for
    ``engine.error_analysis.analyze_scored``; the returned numbers are those of a call without the two, bit for bit."""
    device = _scoring_device(device, "evaluate_coco")
    for iou_type in iou_types:
        _check_iou_type(iou_type, "evaluate_coco")
    options = _options("evaluate_coco", rules, lvis_max_dets, boundary_dilation_ratio, error_thresholds)
    return _summaries(dataset, iou_types, device,
                      lambda types, gt: match_tables(dataset, predictions, types, device, ground_truth=gt, options=options),
                      options, recall, tables_out=tables_out if error_thresholds is not None else None)


def evaluate_coco_results(dataset, results, iou_types=("bbox", "segm"), device="cuda", recall=False,
                          boundary_dilation_ratio=BOUNDARY_DILATION_RATIO, rules="coco", lvis_max_dets=LVIS_MAX_DETS,
                          error_thresholds=None, tables_out=None):
    """``evaluate_coco``'s numbers, in the same structure, for detections that come from COCO results files: ``results`` is
    {iou_type: a path or the parsed list} (``load_coco_results``); an iou_type it does not have is skipped -- but boundary
    reads the ``"boundary"`` entry when there is one and else the ``"segm"`` one: it scores the same ``segm.json``.  Whatever
    wrote the files -- ``export_coco_results``, the reference, another tool -- nothing but the annotation file is needed
    beside them.  ``recall``, ``boundary_dilation_ratio``, ``rules``, ``lvis_max_dets``, ``error_thresholds`` / ``tables_out`` (one
    file for segm and boundary): as in ``evaluate_coco``.  ``device``: the HIP device that decodes the masks and scores."""
    device = _scoring_device(device, "evaluate_coco_results")
    options = _options("evaluate_coco_results", rules, lvis_max_dets, boundary_dilation_ratio, error_thresholds)
    for iou_type in results:
        _check_iou_type(iou_type, "evaluate_coco_results")
    files = dict(results)
    if "boundary" not in files and "segm" in files:
        files["boundary"] = files["segm"]
    iou_types = [t for t in iou_types if t in files]
    if error_thresholds is not None and "boundary" in files and files["boundary"] is not files["segm"]:
        raise ValueError("evaluate_coco_results: the error analysis scores segm and boundary from one results file")
    if all(t in iou_types for t in MASK_IOU_TYPES) and files["boundary"] is not files["segm"]:  # two files: two passes
        return OrderedDict((t, evaluate_coco_results(dataset, {t: files[t]}, (t,), device, recall, boundary_dilation_ratio,
                                                     rules, lvis_max_dets)[t])
                           for t in iou_types)
    return _summaries(dataset, iou_types, device,
                      lambda types, gt: results_match_tables(dataset, files[types[0]], types, device, ground_truth=gt,
                                                             options=options),
                      options, recall, tables_out=tables_out)


# ---- every rank scores what it predicted: only match tables travel --------------------------------------------------------
def evaluate_coco_sharded(dataset, local_predictions, iou_types=("bbox", "segm"), device="cuda", recall=False,
                          boundary_dilation_ratio=BOUNDARY_DILATION_RATIO, rules="coco", lvis_max_dets=LVIS_MAX_DETS):
    """``evaluate_coco``'s numbers without gathering the predictions: ``local_predictions`` is THIS rank's {dataset index:
    BoxList} (what ``engine.inference.compute_on_dataset`` returns), every rank calls this, rank 0 gets the OrderedDict and
    the others None.  The ranks exchange their index lists; ``shard_owners`` says who scores an image that sits on two of
    them, and the images of the annotation file that nobody predicted (those ``COCODataset`` drops are still scored) go
    to rank 0 with zero detections.  Every rank then makes the detection rows of its images and scores them against their
    ground truth on its own device (``_detection_rows``, ``_score_rows``), and its match tables -- about 208 B per detection,
    not the M x M maps -- go to rank 0 with the image id of every problem, where ``merge_shard_tables`` puts them into the
    order ``match_tables`` has.  One process: the same code with one shard.  ``rules``, ``lvis_max_dets``: per image too."""
    device = _scoring_device(device, "evaluate_coco_sharded")
    options = _options("evaluate_coco_sharded", rules, lvis_max_dets, boundary_dilation_ratio)
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
    ground_truth = _ground_truth(dataset, options)
    cat_ids = ground_truth[0]
    images = [image for image in ground_truth[1] if owner_of_image.get(image["id"], 0) == rank]  # in image-id order
    by_image = {dataset.id_to_img_map[idx]: local_predictions[idx] for idx in index_lists[rank]}
    merged = {}
    with torch.cuda.device(device):
        for types in _passes(iou_types):  # segm and boundary together: one pass over the mask words, two tables
            dets = _detection_rows(dataset, by_image, (cat_ids, images), types[0] != "bbox", options)
            problems = np.asarray([len(np.union1d(det["cats"], image["cats"])) for image, det in zip(images, dets)],
                                  dtype=np.int64)
            for iou_type, tables in _score_rows(images, dets, types, device, options).items():
                tables["image"] = np.repeat(np.asarray([image["id"] for image in images], dtype=np.int64), problems)
                parts = [tables]
                if world > 1:
                    parts = [None] * world
                    dist.all_gather_object(parts, tables)
                if rank == 0:
                    merged[iou_type] = merge_shard_tables(parts)
    if rank != 0:
        return None
    return _summaries(dataset, iou_types, device, lambda types, gt: ({t: merged[t] for t in types}, cat_ids), options, recall,
                      ground_truth)


def annotation_dataset(ann_file):
    """The dataset object scoring needs, from the annotation file alone: no images, no configuration.  The ``split`` keys
    of its categories, when present, give the AP50_split_<split> rows."""
    from ..data.datasets import COCODataset

    dataset = COCODataset(ann_file, "", False)
    for item in dataset.coco.dataset["categories"]:
        if "split" in item:
            dataset.class_splits.setdefault(item["split"], []).append(item["id"])
    return dataset
