"""Time of the box-proposal recall matching (csrc/proposal_recall.hip) for one chunk of synthetic images:

    python tools/bench_proposal_recall.py [--images 32] [--proposals 1000] [--ground-truths 20] [--repeats 20]

Seeded, no model: every image of 480 x 640 gets ``--ground-truths`` boxes of mixed sizes and ``--proposals`` proposals, four in
five of them jittered ground truths.  One ``_C.proposal_gt_overlaps`` call covers the chunk -- every image, the four area
ranges and the two limits of the reference's table -- once to warm up (code object, allocator); then the entry point alone
is launched ``--repeats`` times back to back under one pair of device events (kernel time per launch; the median of five such
rounds is reported), and once more the wall clock goes around the whole of ``engine.proposal_recall.gt_overlaps``
(concatenate, upload, host checks, launch, read back).  Prints one JSON line.  ``make_rows`` is also what tests/golden/time_reference_proposal_recall.py
feeds to the reference's own Python loop on the host.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDTH, HEIGHT = 640, 480


def make_rows(images, proposals, ground_truths, seed=0):
    """-> per image (proposals fp32 [P, 4] xyxy best first, ground-truth boxes fp32 [G, 4] xyxy, areas fp32 [G])."""
    rs = np.random.RandomState(seed)
    rows = []
    for _ in range(images):
        side = np.asarray([12.0, 28.0, 50.0, 90.0, 140.0, 220.0])[np.arange(ground_truths) % 6] * (0.8 + 0.4 * rs.rand(ground_truths))
        wh = side[:, None] * (0.7 + 0.6 * rs.rand(ground_truths, 2))
        xy = rs.rand(ground_truths, 2) * (np.asarray([WIDTH, HEIGHT]) - wh - 1).clip(min=1)
        gts = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        areas = (wh[:, 0] * wh[:, 1] * (0.6 + 0.4 * rs.rand(ground_truths))).astype(np.float32)
        pick = rs.randint(max(ground_truths, 1), size=proposals)
        near = gts[pick] + rs.randn(proposals, 4) * 0.1 * np.tile(wh[pick], 2) if ground_truths else np.zeros((proposals, 4))
        far_xy = rs.rand(proposals, 2) * np.asarray([WIDTH - 60.0, HEIGHT - 60.0])
        far = np.concatenate([far_xy, far_xy + rs.rand(proposals, 2) * 200 + 8], 1)
        boxes = np.where((rs.rand(proposals) < 0.8)[:, None] & (ground_truths > 0), near, far)
        boxes = np.stack([np.minimum(boxes[:, 0], boxes[:, 2]), np.minimum(boxes[:, 1], boxes[:, 3]),
                          np.maximum(boxes[:, 0], boxes[:, 2]), np.maximum(boxes[:, 1], boxes[:, 3])], 1)
        boxes = boxes.clip(min=0, max=[WIDTH - 1, HEIGHT - 1, WIDTH - 1, HEIGHT - 1]).astype(np.float32)
        rows.append((boxes, gts, areas))
    return rows


def main():
    import torch

    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import proposal_recall

    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--images", type=int, default=32)
    parser.add_argument("--proposals", type=int, default=1000)
    parser.add_argument("--ground-truths", type=int, default=20)
    parser.add_argument("--repeats", type=int, default=20)
    args = parser.parse_args()
    device = torch.device("cuda", torch.cuda.current_device())
    rows = [tuple(torch.from_numpy(t) for t in r) for r in make_rows(args.images, args.proposals, args.ground_truths)]
    table = [[i * args.proposals, args.proposals, i * args.ground_truths, args.ground_truths] for i in range(args.images)]
    props, gts, areas = (torch.cat([r[k] for r in rows]).to(device) for k in range(3))
    ranges = torch.tensor(proposal_recall.AREA_RANGES, dtype=torch.float32).to(device)
    limits = list(proposal_recall.LIMITS)
    out = _C.proposal_gt_overlaps(props, gts, areas, table, ranges, limits)   # warm-up
    torch.cuda.synchronize()
    table_dev = torch.tensor(table, dtype=torch.int64).to(device)
    limits_dev = torch.tensor(limits, dtype=torch.int32).to(device)
    raw = torch.empty_like(out)
    stream = torch.cuda.current_stream().cuda_stream
    rounds = []
    for _ in range(5):  # the entry point alone, back to back: what the events bracket is kernel time
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(args.repeats):
            rc = _C._L.ovis_proposal_gt_overlaps(props.data_ptr(), gts.data_ptr(), areas.data_ptr(), table_dev.data_ptr(),
                                                 args.images, args.ground_truths, ranges.data_ptr(), ranges.shape[0],
                                                 limits_dev.data_ptr(), len(limits), max(limits), gts.shape[0], raw.data_ptr(), stream)
            assert rc == 0, rc
        end.record()
        torch.cuda.synchronize()
        rounds.append(start.elapsed_time(end) / args.repeats)
    assert torch.equal(raw, out)
    t0 = time.perf_counter()
    whole = proposal_recall.gt_overlaps(rows, device)
    t1 = time.perf_counter()
    assert torch.equal(whole, out.cpu())
    print(json.dumps({"images": args.images, "proposals": args.proposals, "ground_truths": args.ground_truths,
                      "units": args.images * len(proposal_recall.AREA_RANGES) * len(limits),
                      "kernel_ms_median": round(float(np.median(rounds)), 4), "kernel_ms_rounds": [round(r, 4) for r in rounds],
                      "chunk_wall_ms": round((t1 - t0) * 1e3, 3), "AR@1000": proposal_recall.average_recall(whole[0, 1])}))


if __name__ == "__main__":
    main()
