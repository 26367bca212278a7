"""Times the REFERENCE's box-proposal recall -- its Python loop of ``torch.max`` calls, ``evaluate_box_proposals``
(maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py:199-312) -- on the host, on the inputs of
tools/bench_proposal_recall.py, where the reference is available:

    python tests/golden/time_reference_proposal_recall.py [--images 32] [--proposals 1000] [--ground-truths 20]

The eight (limit, area) calls of ``do_coco_evaluation`` (coco_eval.py:31-38), once to warm up and three times under the
wall clock.  Prints one JSON line; writes nothing.  The figure stands beside the device kernel's in DESIGN section 4; the
two come from different hardware and are not a speed-up."""
import argparse
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_proposal_recall_golden as golden  # noqa: E402
from tools.bench_proposal_recall import HEIGHT, WIDTH, make_rows  # noqa: E402


class _Dataset:
    def __init__(self, rows):
        self.id_to_img_map = {k: k for k in range(len(rows))}
        self.coco = golden._Coco({k: [{"bbox": [float(b[0]), float(b[1]), float(b[2] - b[0] + 1), float(b[3] - b[1] + 1)],
                                       "area": float(a), "iscrowd": 0} for b, a in zip(gts, areas)]
                                  for k, (_, gts, areas) in enumerate(rows)})

    def get_img_info(self, index):
        return {"width": WIDTH, "height": HEIGHT}


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--images", type=int, default=32)
    parser.add_argument("--proposals", type=int, default=1000)
    parser.add_argument("--ground-truths", type=int, default=20)
    args = parser.parse_args()
    ref = golden.load_reference()
    from maskrcnn_benchmark.structures.bounding_box import BoxList

    rows = make_rows(args.images, args.proposals, args.ground_truths)
    dataset = _Dataset(rows)
    predictions = []
    for boxes, _, _ in rows:
        pred = BoxList(torch.from_numpy(boxes), (WIDTH, HEIGHT), mode="xyxy")
        pred.add_field("objectness", torch.arange(len(boxes), 0, -1, dtype=torch.float32))   # already best first
        predictions.append(pred)

    def table():
        return {(limit, area): ref.evaluate_box_proposals(predictions, dataset, area=area, limit=limit)["ar"].item()
                for limit in golden.LIMITS for area in golden.AREAS}

    table()
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        ars = table()
        times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({"images": args.images, "proposals": args.proposals, "ground_truths": args.ground_truths,
                      "threads": torch.get_num_threads(), "reference_loop_ms": [round(t, 1) for t in times],
                      "AR@1000": ars[(1000, "all")]}))


if __name__ == "__main__":
    main()
