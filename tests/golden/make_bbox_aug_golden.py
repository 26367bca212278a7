"""Writes tests/golden/bbox_aug.npz: the merge of test-time-augmentation views as the REFERENCE computes it, recorded where
the reference is available (python tests/golden/make_bbox_aug_golden.py; oracle/_ref/ref_C.so built first).

Seeded inputs -- 3 views (identity; the same size mirrored; a larger view with unequal width / height ratios, mirrored) of
one image, 40 rows each, 9 classes -- go through the reference's own classes (tests/golden/ref_import.py, its ``_C.nms``
bound to the reference's CPU kernel): ``BoxList.transpose(0)`` for the mirrored views (engine/bbox_aug.py:106-107),
``BoxList.resize(first view's size)`` (bbox_aug.py:20-24), the concatenation of bbox_aug.py:53-60 and
``PostProcessor.filter_results`` (box_head/inference.py:121-163).  Inputs and outputs are stored; only data is written.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402

NUM_CLASSES, ROWS = 9, 40
VIEWS = [((61, 47), False), ((61, 47), True), ((97, 71), True)]   # ((width, height), mirrored): 61/97 != 47/71
SCORE_THRESH, NMS, DETECTIONS_PER_IMG = 0.05, 0.5, 25


def make_inputs():
    g = torch.Generator().manual_seed(20240607)
    boxes, scores = [], []
    centers = torch.rand(ROWS, NUM_CLASSES, 2, generator=g)          # shared by the views: the same objects seen thrice
    extents = torch.rand(ROWS, NUM_CLASSES, 2, generator=g) * 0.3 + 0.05
    for (w, h), mirrored in VIEWS:
        wh = torch.tensor([float(w), float(h)])
        c = centers + (torch.rand(ROWS, NUM_CLASSES, 2, generator=g) - 0.5) * 0.04
        lo, hi = (c - extents / 2).clamp(0, 1) * (wh - 1), (c + extents / 2).clamp(0, 1) * (wh - 1)
        b = torch.cat([lo, hi], -1)
        if mirrored:  # what the detector sees in the mirrored picture
            b = torch.stack([w - b[..., 2] - 1, b[..., 1], w - b[..., 0] - 1, b[..., 3]], -1)
        boxes.append(b.reshape(ROWS, NUM_CLASSES * 4).contiguous())
        s = torch.softmax(torch.randn(ROWS, NUM_CLASSES, generator=g) * 2.5, -1)
        scores.append(s)
    return boxes, scores


def main():
    ref_import.install()
    from maskrcnn_benchmark.modeling.roi_heads.box_head.inference import PostProcessor
    from maskrcnn_benchmark.structures.bounding_box import BoxList

    boxes, scores = make_inputs()
    views = []
    for (size, mirrored), b, s in zip(VIEWS, boxes, scores):
        boxlist = BoxList(b.reshape(-1, 4), size, mode="xyxy")
        boxlist.add_field("scores", s.reshape(-1))
        if mirrored:
            boxlist = boxlist.transpose(0)
        views.append(boxlist if not views else boxlist.resize(views[0].size))
    merged = BoxList(torch.cat([v.bbox for v in views]), views[0].size, views[0].mode)   # bbox_aug.py:55-59
    merged.add_field("scores", torch.cat([v.get_field("scores") for v in views]))
    post = PostProcessor(SCORE_THRESH, NMS, DETECTIONS_PER_IMG)
    result = post.filter_results(merged, NUM_CLASSES)
    assert 0 < len(result) <= ROWS * NUM_CLASSES
    out = {"num_classes": np.int64(NUM_CLASSES), "score_thresh": np.float64(SCORE_THRESH), "nms": np.float64(NMS),
           "detections_per_img": np.int64(DETECTIONS_PER_IMG),
           "view_sizes": np.asarray([v[0] for v in VIEWS], dtype=np.int64), "view_flips": np.asarray([v[1] for v in VIEWS]),
           "merged_boxes": merged.bbox.numpy(), "merged_scores": merged.get_field("scores").numpy(),
           "out_boxes": result.bbox.numpy(), "out_scores": result.get_field("scores").numpy(),
           "out_labels": result.get_field("labels").numpy()}
    for v, (b, s) in enumerate(zip(boxes, scores)):
        out[f"boxes_{v}"], out[f"scores_{v}"] = b.numpy(), s.numpy()
    path = os.path.join(HERE, "bbox_aug.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", len(result), "detections, labels", sorted(set(result.get_field("labels").tolist())))


if __name__ == "__main__":
    main()
