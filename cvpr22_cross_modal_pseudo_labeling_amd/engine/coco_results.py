"""The detections of a test set as COCO results files -- the ``bbox.json`` / ``segm.json`` the reference leaves in
``OUTPUT_DIR/inference/<name>/`` (maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py: ``do_coco_evaluation``
:40-61 over ``prepare_for_coco_detection`` :71-105 and ``prepare_for_coco_segmentation`` :108-162): what evaluation
servers, pycocotools and every downstream tool read.

``bbox`` is host arithmetic on the boxes.  For ``segm`` the reference pastes every mask into an H x W canvas, copies it
to the host and runs pycocotools' ``encode`` on it; here the run lengths and the compressed ``counts`` strings are made on
the device straight from the mask head's maps and the boxes (``_C.pasted_masks_rle``, csrc/mask_rle.hip), a chunk of
images per call, and only the strings come back.  A decoded string equals ``_C.paste_masks`` of that detection at the
original image size, bit for bit.

Unlike the scorer (engine/coco_eval.py) the export keeps EVERY detection, in dataset-index order and prediction order:
no cap of 100 per category, no sorting.
"""
import json
import os

import torch

from .. import _C
from . import coco_eval

IOU_TYPES = ("bbox", "segm")


def _records(dataset, predictions):
    """Per non-empty prediction, in dataset-index order: (prediction, file id, width, height, json category ids, scores)."""
    if len(predictions) > len(dataset):
        raise ValueError(f"export_coco_results: {len(predictions)} predictions for a dataset of {len(dataset)} images")
    for idx, pred in enumerate(predictions):
        if len(pred) == 0:
            continue
        info = dataset.get_img_info(idx)
        cats = [dataset.contiguous_category_id_to_json_id[l] for l in pred.get_field("labels").tolist()]
        yield pred, dataset.id_to_img_map[idx], int(info["width"]), int(info["height"]), cats, pred.get_field("scores").tolist()


def bbox_results(dataset, predictions):
    """``prepare_for_coco_detection``: one {"image_id", "category_id", "bbox" (xywh at the file's size), "score"} per detection."""
    out = []
    for pred, image_id, width, height, cats, scores in _records(dataset, predictions):
        _, xywh = coco_eval.detection_boxes(pred, width, height)
        out.extend({"image_id": image_id, "category_id": cats[k], "bbox": box, "score": scores[k]}
                   for k, box in enumerate(xywh.tolist()))
    return out


def _mask_pieces(records, max_masks):
    """(maps [k, M, M], boxes [k, 4], sizes int32 [k, 2]) of at most ``max_masks`` masks each, in order: the images' masks
    as they come, an image with more than ``max_masks`` cut."""
    for pred, _, width, height, _, _ in records:
        maps = coco_eval.mask_maps(pred).detach()[:, 0].float()
        boxes, _ = coco_eval.detection_boxes(pred, width, height)
        sizes = torch.tensor([[height, width]], dtype=torch.int32).expand(len(pred), 2)
        for k in range(0, len(pred), max_masks):
            yield maps[k:k + max_masks], boxes[k:k + max_masks], sizes[k:k + max_masks]


def _mask_chunks(records, max_masks):
    """The pieces gathered into chunks of at most ``max_masks`` masks of one map resolution: lists of pieces."""
    chunk, used = [], 0
    for piece in _mask_pieces(records, max_masks):
        if chunk and (used + len(piece[0]) > max_masks or piece[0].shape[1] != chunk[0][0].shape[1]):
            yield chunk
            chunk, used = [], 0
        chunk.append(piece)
        used += len(piece[0])
    if chunk:
        yield chunk


def segm_results(dataset, predictions, device):
    """``prepare_for_coco_segmentation``: one {"image_id", "category_id", "segmentation": {"size": [h, w], "counts": str},
    "score"} per detection; the masks are the Masker's (threshold 0.5, padding 1) at the file's image size.  One
    ``_C.pasted_masks_rle`` call per chunk of at most ``coco_eval.MAX_EXPORT_MASKS`` masks."""
    records = list(_records(dataset, predictions))
    max_masks = min(int(coco_eval.MAX_EXPORT_MASKS), coco_eval.MAX_CALL_MASKS)
    if max_masks < 1:
        raise ValueError("export_coco_results: coco_eval.MAX_EXPORT_MASKS must be at least 1")
    counts = []
    for chunk in _mask_chunks(records, max_masks):
        maps, boxes, sizes = (torch.cat([piece[i] for piece in chunk]).to(device) for i in range(3))
        data, offsets = _C.pasted_masks_rle(maps, boxes, sizes, 0.5)
        text, offsets = data.cpu().numpy().tobytes(), offsets.tolist()
        counts.extend(text[a:b].decode("ascii") for a, b in zip(offsets[:-1], offsets[1:]))
    out, at = [], 0
    for _, image_id, width, height, cats, scores in records:
        for k in range(len(cats)):
            out.append({"image_id": image_id, "category_id": cats[k],
                        "segmentation": {"size": [height, width], "counts": counts[at + k]}, "score": scores[k]})
        at += len(cats)
    return out


def export_coco_results(dataset, predictions, folder, iou_types=IOU_TYPES, device="cuda"):
    """Writes ``folder``/<iou_type>.json (the reference's names) for ``predictions`` -- the list ``inference()`` returns or
    ``torch.load`` gives from ``predictions.pth`` (BoxLists in dataset-index order, fields ``scores``, ``labels`` and, for
    segm, ``mask`` [K, 1, M, M]) -- -> {iou_type: path}.  ``device``: the HIP device that encodes the masks; ``bbox`` alone
    needs none.  No predictions: ``[]``."""
    for iou_type in iou_types:
        if iou_type not in IOU_TYPES:
            raise ValueError(f"export_coco_results: iou_type '{iou_type}' is not supported (bbox, segm)")
    device = torch.device(device)
    if "segm" in iou_types and device.type != "cuda":
        raise ValueError("export_coco_results: segm results are encoded on the HIP device (the mask run-length encoder has "
                         "no host implementation)")
    os.makedirs(folder, exist_ok=True)
    paths = {}
    for iou_type in iou_types:
        results = bbox_results(dataset, predictions) if iou_type == "bbox" else segm_results(dataset, predictions, device)
        paths[iou_type] = os.path.join(folder, iou_type + ".json")
        with open(paths[iou_type], "w") as f:
            json.dump(results, f)
    return paths
