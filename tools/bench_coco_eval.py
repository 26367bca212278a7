"""Time of COCO scoring (engine/coco_eval.py) for one chunk of synthetic images, split by stage:

    python tools/bench_coco_eval.py [--images 32] [--height 480] [--width 640] [--detections 100] [--ground-truths 20]
        [--boundary] [--repeats 1] [--lvis] [--errors]

Seeded, no model: every image gets ``--detections`` random boxes with 28 x 28 mask maps over 10 categories and
``--ground-truths`` random hexagons.  The whole set is scored as ONE chunk, once to warm up (code objects, allocator) and
once under device events around the paste, rasterise, pack, IoU and match calls; the host accumulate / summarise is timed
with the wall clock.  Prints one JSON line per IoU type.  ``--boundary`` adds a third pass, segm and Boundary AP scored
TOGETHER from one set of mask words (``iou_type`` "segm+boundary": what ``--boundary-ap`` costs on top is that line minus the
segm line; its stages ``boundary`` -- the erosion -- and ``boundary_iou`` are new, the others are segm's).  ``--repeats N``
times every pass N times and prints each: the spread is the noise a difference has to clear.

``--lvis`` scores an LVIS-shaped chunk under ``rules="lvis"`` instead (``make_lvis_case``: 1203 categories with frequencies, per
image 300 detections over about 150 of them, about 12 ground truths in about 6 categories, about 20 negative categories among
those the detector fired on, two not-exhaustive ones), with the same stage lines, and then times the MATCHING alone on the
chunk's own problem table: ``_C.lvis_match`` against ``_C.coco_match`` with all-zero flags -- the tables of the two must be
identical, which is asserted -- and both again on the sub-table of the problems WITHOUT ground truth, where ``lvis_match``
reads no IoU and shuffles nothing.  ``--repeats`` runs of 50 launches each of the C entries into outputs allocated once, device events around the 50; one JSON line
(``"match"``) with every run's time per launch in microseconds.

``--errors`` (not with ``--lvis``) times bbox and segm a second time with the error analysis (engine/error_analysis.py) in the
same alternation: those lines say ``"errors": true``, carry two more stages -- ``image_iou``, the IoU of every detection of an
image against every ground truth of it, and ``error_types``, the typing and missed-ground-truth kernels with the few tensor ops
that hand them the base matching -- and ``host_analysis_ms``, the fixes and their AP50s on the host.  What the analysis costs
is such a line minus the line without it.  A last line, ``"error_types"``, times the C entry alone -- its two kernels into
outputs allocated once, 50 calls per run -- on the inputs of the bbox pass.
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
from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval, error_analysis  # noqa: E402
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


LVIS_CATEGORIES = 1203


def make_lvis_case(folder, images, height, width, detections=300, fired=150, ground_truths=12, positives=6, negatives=20,
                   seed=0):
    """An LVIS-shaped chunk: per image ``detections`` boxes over ``fired`` of the 1203 categories, ``ground_truths`` hexagons in
    ``positives`` of those categories, ``negatives`` more of them verified absent, two of the positives not exhaustive."""
    rs = np.random.RandomState(seed)
    g = torch.Generator().manual_seed(seed)
    anns, infos, predictions = [], [], []
    for i in range(images):
        cats = rs.choice(np.arange(1, LVIS_CATEGORIES + 1), size=fired, replace=False)
        pos, neg = cats[:positives], cats[positives:positives + negatives]
        for k in range(ground_truths):
            cx, cy = rs.uniform(40, width - 40), rs.uniform(40, height - 40)
            rx, ry = rs.uniform(10, 120), rs.uniform(10, 120)
            poly = []
            for v in range(6):
                poly += [float(np.clip(cx + rx * math.cos(v * math.pi / 3), 0, width)),
                         float(np.clip(cy + ry * math.sin(v * math.pi / 3), 0, height))]
            x0, y0, x1, y1 = min(poly[0::2]), min(poly[1::2]), max(poly[0::2]), max(poly[1::2])
            anns.append({"id": len(anns) + 1, "image_id": i, "category_id": int(pos[k % positives]),
                         "bbox": [x0, y0, x1 - x0, y1 - y0], "area": (x1 - x0) * (y1 - y0) * .65, "segmentation": [poly]})
        infos.append({"id": i, "file_name": f"{i}.png", "width": width, "height": height,
                      "neg_category_ids": [int(c) for c in neg], "not_exhaustive_category_ids": [int(c) for c in pos[:2]]})
        xy = torch.rand(detections, 2, generator=g) * torch.tensor([width - 60.0, height - 60.0])
        wh = torch.rand(detections, 2, generator=g) * 200 + 16
        pred = BoxList(torch.cat((xy, torch.minimum(xy + wh, torch.tensor([width - 1.0, height - 1.0]))), 1), (width, height))
        pred.add_field("scores", torch.rand(detections, generator=g))
        pred.add_field("labels", torch.from_numpy(cats[torch.randint(0, fired, (detections,), generator=g).numpy()]))
        pred.add_field("mask", torch.rand(detections, 1, MAP, MAP, generator=g))
        predictions.append(pred)
    path = os.path.join(folder, "lvis_instances.json")
    with open(path, "w") as f:
        json.dump({"images": infos, "annotations": anns,
                   "categories": [{"id": c, "name": f"class{c}", "frequency": "rcf"[c % 3]} for c in range(1, LVIS_CATEGORIES + 1)]}, f)
    return COCODataset(path, folder, False), predictions   # labels = json ids: the ids are 1 .. 1203, contiguous


def time_matching(dataset, predictions, device, budget, repeats, launches=50):
    """``_C.lvis_match`` against ``_C.coco_match`` on the problem table the chunk's segm pass makes, flags all zero, and on its
    sub-table of the problems without ground truth -> the ``"match"`` line."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    seen = {}
    real = _C.lvis_match

    def capture(*args):
        seen["args"] = args
        return real(*args)
    _C.lvis_match = capture
    try:
        coco_eval.match_tables(dataset, predictions, "segm", device, budget, rules="lvis")
    finally:
        _C.lvis_match = real
    iou, problems, det_areas, gt_areas, gt_ignore_in, flags, area_ranges, thresholds = seen["args"]
    zero_gt, zero_flags = torch.zeros_like(gt_ignore_in), torch.zeros_like(flags)
    empty = problems.host[problems.host[:, 3] == 0]
    sub = _C.CocoProblems(empty, device)
    sub_flags = torch.zeros(len(sub), dtype=torch.uint8, device=device)
    for a, b in zip(_C.lvis_match(iou, problems, det_areas, gt_areas, zero_gt, zero_flags, area_ranges, thresholds),
                    _C.coco_match(iou, problems, det_areas, gt_areas, zero_gt, area_ranges, thresholds)):
        assert torch.equal(a, b), "lvis_match and coco_match differ on a table with all-zero flags"
    for a, b in zip(_C.lvis_match(iou, sub, det_areas, gt_areas, zero_gt, sub_flags, area_ranges, thresholds),
                    _C.coco_match(iou, sub, det_areas, gt_areas, zero_gt, area_ranges, thresholds)):
        assert torch.equal(a, b), "lvis_match and coco_match differ on the problems without ground truth"
    # the C entries themselves, into outputs allocated once: a call is one launch and nothing else
    num_a, num_t, d, g = area_ranges.shape[0], thresholds.numel(), det_areas.numel(), gt_areas.numel()
    dt_match = torch.empty((num_a, num_t, d), dtype=torch.int32, device=device)
    dt_ignore = torch.empty((num_a, num_t, d), dtype=torch.uint8, device=device)
    gt_ignore = torch.empty((num_a, g), dtype=torch.uint8, device=device)

    def entry(name, table, *flag_args):
        def call():
            rc = getattr(_C._L, name)(iou.data_ptr(), table.dev.data_ptr(), len(table), table.max_gts, det_areas.data_ptr(),
                                      gt_areas.data_ptr(), *[f.data_ptr() for f in flag_args], area_ranges.data_ptr(), num_a,
                                      thresholds.data_ptr(), num_t, d, g, dt_match.data_ptr(), dt_ignore.data_ptr(),
                                      gt_ignore.data_ptr(), _C._stream())
            assert rc == 0, (name, rc)
        return call
    cases = {"lvis_match": entry("ovis_lvis_match", problems, zero_gt, zero_flags),
             "coco_match": entry("ovis_coco_match", problems, zero_gt),
             "lvis_match_flags": entry("ovis_lvis_match", problems, gt_ignore_in, flags),
             "lvis_match_no_gt": entry("ovis_lvis_match", sub, zero_gt, sub_flags),
             "coco_match_no_gt": entry("ovis_coco_match", sub, zero_gt)}
    times = {name: [] for name in cases}
    for _ in range(repeats):   # the entries alternate, so a drift of the machine meets all of them
        for name, call in cases.items():
            call()
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            start.record()
            for _ in range(launches):
                call()
            end.record()
            torch.cuda.synchronize()
            times[name].append(round(start.elapsed_time(end) / launches * 1e3, 2))
    return {"match": "per launch in us", "problems": len(problems), "problems_without_gt": len(sub),
            "detections": int(det_areas.numel()), "ground_truths": int(gt_areas.numel()), "pairs": int(iou.numel()),
            "launches_per_run": launches, "us": times, "identical_tables": True}


def time_typing(dataset, predictions, device, budget, repeats, launches=50):
    """``ovis_error_types`` alone on the inputs the chunk's bbox pass hands it: the C entry (its two kernels) into outputs
    allocated once, ``repeats`` runs of ``launches`` calls, device events around them -> the ``"error_types"`` line, per call in
    microseconds.  The ``error_types`` STAGE of the lines above also holds the tensor ops that make the entry's inputs."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    seen = {}
    real = _C.error_types

    def capture(*args):
        seen["args"] = args
        return real(*args)
    _C.error_types = capture
    try:
        coco_eval.match_tables(dataset, predictions, "bbox", device, budget,
                               error_thresholds=(error_analysis.FG_THRESHOLD, error_analysis.BG_THRESHOLD))
    finally:
        _C.error_types = real
    iou, images, det_cat, det_match, det_ignore, gt_cat, crowd, t_f, t_b = seen["args"]
    det_match, det_ignore = det_match.contiguous(), det_ignore.contiguous()
    d, g = det_cat.numel(), gt_cat.numel()
    err_type = torch.empty(d, dtype=torch.uint8, device=device)
    err_gt = torch.empty(d, dtype=torch.int32, device=device)
    gt_missed = torch.empty(g, dtype=torch.uint8, device=device)

    def call():
        rc = _C._L.ovis_error_types(iou.data_ptr(), images.dev.data_ptr(), len(images), int(images.host[:, 1].max()), images.max_gts,
                                    det_cat.data_ptr(), det_match.data_ptr(), det_ignore.data_ptr(), gt_cat.data_ptr(),
                                    crowd.data_ptr(), t_f, t_b, d, g, err_type.data_ptr(), err_gt.data_ptr(), gt_missed.data_ptr(),
                                    _C._stream())
        assert rc == 0, rc
    times = []
    for _ in range(repeats):
        call()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(launches):
            call()
        end.record()
        torch.cuda.synchronize()
        times.append(round(start.elapsed_time(end) / launches * 1e3, 2))
    for a, b in zip(real(*seen["args"]), (err_type, err_gt, gt_missed)):
        assert torch.equal(a, b), "the timed entry and _C.error_types differ"
    return {"error_types": "per call (two kernels) in us", "images": len(images), "detections": d, "ground_truths": g,
            "pairs": int(iou.numel()), "launches_per_run": launches, "us": times}


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--images", type=int, default=32)
    parser.add_argument("--height", type=int, default=480)
    parser.add_argument("--width", type=int, default=640)
    parser.add_argument("--detections", type=int, default=100)
    parser.add_argument("--ground-truths", type=int, default=20)
    parser.add_argument("--boundary", action="store_true", help="also time segm and Boundary AP scored together")
    parser.add_argument("--repeats", type=int, default=1, help="timed runs per pass, each printed")
    parser.add_argument("--lvis", action="store_true",
                        help="an LVIS-shaped chunk (300 detections per image over 150 of 1203 categories, 12 ground truths, 20 "
                             "negatives) under rules='lvis', and lvis_match against coco_match on its problem table")
    parser.add_argument("--errors", action="store_true",
                        help="also time bbox and segm with the error analysis: stages image_iou and error_types, and the "
                             "host's fixes")
    args = parser.parse_args()
    if args.errors and args.lvis:
        parser.error("--errors follows COCO's rules: it does not go with --lvis")
    device = torch.device("cuda", torch.cuda.current_device())
    with tempfile.TemporaryDirectory() as folder:
        if args.lvis:
            dataset, predictions = make_lvis_case(folder, args.images, args.height, args.width)
        else:
            dataset, predictions = make_case(folder, args.images, args.height, args.width, args.detections, args.ground_truths)
    rules = {"rules": "lvis"} if args.lvis else {}
    frequencies = coco_eval.category_frequencies(dataset) if args.lvis else None
    budget = 1 << 62   # one chunk
    passes = [("bbox", {}), ("segm", {})] + ([(("segm", "boundary"), {})] if args.boundary else [])
    if args.errors:
        thresholds = {"error_thresholds": (error_analysis.FG_THRESHOLD, error_analysis.BG_THRESHOLD)}
        passes += [("bbox", thresholds), ("segm", thresholds)]
    for iou_type, errors in passes:
        coco_eval.match_tables(dataset, predictions, iou_type, device, budget, **rules, **errors)   # warm-up
    for _ in range(args.repeats):   # the passes alternate, so a drift of the machine meets all of them
        for iou_type, errors in passes:
            torch.cuda.synchronize()
            timer = {}
            t0 = time.perf_counter()
            tables, cat_ids = coco_eval.match_tables(dataset, predictions, iou_type, device, budget, timer, **rules, **errors)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            tables = {iou_type: tables} if isinstance(iou_type, str) else tables
            if args.lvis:
                results = {name: coco_eval.summarize_lvis(coco_eval.accumulate_lvis(t, len(cat_ids))[0], [str(c) for c in cat_ids],
                                                          {}, frequencies) for name, t in tables.items()}
            else:
                results = {name: coco_eval.summarize(coco_eval.accumulate(t, len(cat_ids)), [str(c) for c in cat_ids], {})
                           for name, t in tables.items()}
            t2 = time.perf_counter()
            stages = {name: round(sum(s.elapsed_time(e) for s, e in events), 3) for name, events in timer.items()}
            first = next(iter(tables.values()))
            line = {"rules": "lvis" if args.lvis else "coco", "iou_type": "+".join(tables), "images": args.images, "size": [args.height, args.width],
                    "detections": int(first["det_start"][-1]), "ground_truths": int(first["gt_start"][-1]),
                    "problems": len(first["category"]), "device_ms": stages, "device_ms_total": round(sum(stages.values()), 3),
                    "chunk_wall_ms": round((t1 - t0) * 1e3, 2), "host_accumulate_ms": round((t2 - t1) * 1e3, 2)}
            line.update({"AP" if isinstance(iou_type, str) else f"AP_{name}": r["AP"] for name, r in results.items()})
            if errors:
                analysis = error_analysis.analyze_tables(tables[iou_type], len(cat_ids), {})
                line.update(errors=True, host_analysis_ms=round((time.perf_counter() - t2) * 1e3, 2), counts=analysis["counts"]["all"],
                            dAP50={k[6:]: round(v, 4) for k, v in analysis.items() if k.startswith("dAP50_")})
            print(json.dumps(line), flush=True)
    if args.errors:
        print(json.dumps(time_typing(dataset, predictions, device, budget, max(args.repeats, 1))), flush=True)
    if args.lvis:
        print(json.dumps(time_matching(dataset, predictions, device, budget, max(args.repeats, 1))), flush=True)


if __name__ == "__main__":
    main()
