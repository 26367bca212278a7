"""Time of COCO scoring (engine/coco_eval.py) for one chunk of synthetic images, split by stage:

    python tools/bench_coco_eval.py [--images 32] [--height 480] [--width 640] [--detections 100] [--ground-truths 20]
        [--boundary] [--repeats 1]

Seeded, no model: every image gets ``--detections`` random boxes with 28 x 28 mask maps over 10 categories and
``--ground-truths`` random hexagons.  The whole set is scored as ONE chunk, once to warm up (code objects, allocator) and
once under device events around the paste, rasterise, pack, IoU and match calls; the host accumulate / summarise is timed
with the wall clock.  Prints one JSON line per IoU type.  ``--boundary`` adds a third pass, segm and Boundary AP scored
TOGETHER from one set of mask words (``iou_type`` "segm+boundary": what ``--boundary-ap`` costs on top is that line minus the
segm line; its stages ``boundary`` -- the erosion -- and ``boundary_iou`` are new, the others are segm's).  ``--repeats N``
times every pass N times and prints each: the spread is the noise a difference has to clear.
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCODataset  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList  # noqa: E402

CATEGORIES = 10
MAP = 28


def make_case(folder, images, height, width, detections, ground_truths, seed=0):
    rs = np.random.RandomState(seed)
    anns = []
    for i in range(images):
        for _ in range(ground_truths):
            cx, cy = rs.uniform(40, width - 40), rs.uniform(40, height - 40)
            rx, ry = rs.uniform(10, 120), rs.uniform(10, 120)
            poly = []
            for k in range(6):
                poly += [float(np.clip(cx + rx * math.cos(k * math.pi / 3), 0, width)),
                         float(np.clip(cy + ry * math.sin(k * math.pi / 3), 0, height))]
            x0, y0, x1, y1 = min(poly[0::2]), min(poly[1::2]), max(poly[0::2]), max(poly[1::2])
            anns.append({"id": len(anns) + 1, "image_id": i, "category_id": int(rs.randint(1, CATEGORIES + 1)), "iscrowd": 0,
                         "bbox": [x0, y0, x1 - x0, y1 - y0], "area": (x1 - x0) * (y1 - y0) * .65, "segmentation": [poly]})
    path = os.path.join(folder, "instances.json")
    with open(path, "w") as f:
        json.dump({"images": [{"id": i, "file_name": f"{i}.png", "width": width, "height": height} for i in range(images)],
                   "categories": [{"id": c, "name": f"class{c}"} for c in range(1, CATEGORIES + 1)], "annotations": anns}, f)
    dataset = COCODataset(path, folder, False)
    g = torch.Generator().manual_seed(seed)
    predictions = []
    for _ in range(images):
        xy = torch.rand(detections, 2, generator=g) * torch.tensor([width - 60.0, height - 60.0])
        wh = torch.rand(detections, 2, generator=g) * 200 + 16
        pred = BoxList(torch.cat((xy, torch.minimum(xy + wh, torch.tensor([width - 1.0, height - 1.0]))), 1), (width, height))
        pred.add_field("scores", torch.rand(detections, generator=g))
        pred.add_field("labels", torch.randint(1, CATEGORIES + 1, (detections,), generator=g))
        pred.add_field("mask", torch.rand(detections, 1, MAP, MAP, generator=g))
        predictions.append(pred)
    return dataset, predictions


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--images", type=int, default=32)
    parser.add_argument("--height", type=int, default=480)
    parser.add_argument("--width", type=int, default=640)
    parser.add_argument("--detections", type=int, default=100)
    parser.add_argument("--ground-truths", type=int, default=20)
    parser.add_argument("--boundary", action="store_true", help="also time segm and Boundary AP scored together")
    parser.add_argument("--repeats", type=int, default=1, help="timed runs per pass, each printed")
    args = parser.parse_args()
    device = torch.device("cuda", torch.cuda.current_device())
    with tempfile.TemporaryDirectory() as folder:
        dataset, predictions = make_case(folder, args.images, args.height, args.width, args.detections, args.ground_truths)
    budget = 1 << 62   # one chunk
    passes = ["bbox", "segm"] + ([("segm", "boundary")] if args.boundary else [])
    for iou_type in passes:
        coco_eval.match_tables(dataset, predictions, iou_type, device, budget)   # warm-up
    for _ in range(args.repeats):   # the passes alternate, so a drift of the machine meets all of them
        for iou_type in passes:
            torch.cuda.synchronize()
            timer = {}
            t0 = time.perf_counter()
            tables, cat_ids = coco_eval.match_tables(dataset, predictions, iou_type, device, budget, timer)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            tables = {iou_type: tables} if isinstance(iou_type, str) else tables
            results = {name: coco_eval.summarize(coco_eval.accumulate(t, len(cat_ids)), [str(c) for c in cat_ids], {})
                       for name, t in tables.items()}
            t2 = time.perf_counter()
            stages = {name: round(sum(s.elapsed_time(e) for s, e in events), 3) for name, events in timer.items()}
            first = next(iter(tables.values()))
            line = {"iou_type": "+".join(tables), "images": args.images, "size": [args.height, args.width],
                    "detections": int(first["det_start"][-1]), "ground_truths": int(first["gt_start"][-1]),
                    "problems": len(first["category"]), "device_ms": stages, "device_ms_total": round(sum(stages.values()), 3),
                    "chunk_wall_ms": round((t1 - t0) * 1e3, 2), "host_accumulate_ms": round((t2 - t1) * 1e3, 2)}
            line.update({"AP" if isinstance(iou_type, str) else f"AP_{name}": r["AP"] for name, r in results.items()})
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
