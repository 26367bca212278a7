"""Time of COCO RLE strings -> packed bit words for the masks of a results file, two routes in one process:

    python tools/bench_rle_decode.py [--masks 2000] [--height 480] [--width 640] [--rounds 3] [--iters 10]

  device   ``_C.coco_rle_words`` (csrc/coco_rle_decode.hip): one call for all strings -- join, upload, count / runs /
           words launches, the host reads in between
  host     what there was before it: ``coco_eval.rle_decode`` per mask in a Python loop, one upload, ``_C.coco_pack_masks``

Seeded, no model: the strings are the export's own (``_C.pasted_masks_rle``) for random boxes with 28 x 28 maps.  Each
route is warmed once, then the routes alternate ``--rounds`` times; a route's time is the wall clock around calls that end
in a device synchronise (the host route is timed once a round, the device route ``--iters`` times).  The outputs of the
two routes are compared (words and areas, ``torch.equal``).  A second shape -- noise masks, about half as many runs as
pixels -- times the device route alone at the other end of the binary search's depth.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from cvpr22_cross_modal_pseudo_labeling_amd import _C  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval  # noqa: E402

MAP = 28


def export_strings(masks, height, width, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    xy = torch.rand(masks, 2, generator=g) * torch.tensor([width - 60.0, height - 60.0])
    wh = torch.rand(masks, 2, generator=g) * 200 + 16
    boxes = torch.cat((xy, torch.minimum(xy + wh, torch.tensor([width - 1.0, height - 1.0]))), 1)
    maps = torch.rand(masks, MAP, MAP, generator=g)
    sizes = torch.tensor([[height, width]], dtype=torch.int32).expand(masks, 2).contiguous()
    data, offsets = _C.pasted_masks_rle(maps.to(device), boxes.to(device), sizes.to(device))
    text, offsets = data.cpu().numpy().tobytes(), offsets.tolist()
    return [text[a:b].decode("ascii") for a, b in zip(offsets[:-1], offsets[1:])], sizes.to(device)


def device_route(strings, sizes):
    words, _, areas, status = _C.coco_rle_words(strings, sizes)
    assert not bool(status.any())   # a host read, as the scorer does
    return words, areas


def host_route(strings, height, width, device):
    masks = np.stack([coco_eval.rle_decode({"counts": s, "size": [height, width]}, height, width) for s in strings])
    words, areas = _C.coco_pack_masks(torch.from_numpy(masks).to(device))
    return words.reshape(-1), areas


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters, out


def main():
    parser = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    parser.add_argument("--masks", type=int, default=2000)
    parser.add_argument("--height", type=int, default=480)
    parser.add_argument("--width", type=int, default=640)
    parser.add_argument("--rounds", type=int, default=3)
    parser.add_argument("--iters", type=int, default=10)
    parser.add_argument("--noise-masks", type=int, default=64)
    args = parser.parse_args()
    device = torch.device("cuda", torch.cuda.current_device())
    strings, sizes = export_strings(args.masks, args.height, args.width, device)
    dev_out = device_route(strings, sizes)      # warm-up of both routes, and the comparison
    host_out = host_route(strings, args.height, args.width, device)
    equal = torch.equal(dev_out[0], host_out[0]) and torch.equal(dev_out[1], host_out[1])
    dev_ms, host_ms = [], []
    for _ in range(args.rounds):
        dev_ms.append(round(timed(lambda: device_route(strings, sizes), args.iters)[0], 3))
        host_ms.append(round(timed(lambda: host_route(strings, args.height, args.width, device), 1)[0], 1))
    rs = np.random.RandomState(1)
    pixels = args.height * args.width
    variants = [torch.from_numpy(np.diff(np.concatenate([[0], np.sort(rs.choice(np.arange(1, pixels), pixels // 2, replace=False)),
                                                         [pixels]])).astype(np.int32)) for _ in range(2)]
    noise, noise_sizes = [variants[k % 2] for k in range(args.noise_masks)], sizes[:args.noise_masks].contiguous()
    device_route(noise, noise_sizes)   # warm-up
    noise_ms = timed(lambda: device_route(noise, noise_sizes), args.iters)[0]
    print(json.dumps({"masks": args.masks, "size": [args.height, args.width],
                      "characters_per_mask": round(sum(map(len, strings)) / args.masks, 1), "outputs_equal": equal,
                      "device_ms": sorted(dev_ms)[len(dev_ms) // 2], "device_rounds_ms": dev_ms,
                      "host_ms": sorted(host_ms)[len(host_ms) // 2], "host_rounds_ms": host_ms,
                      "noise": {"masks": args.noise_masks, "runs_per_mask": int(variants[0].numel()),
                                "device_ms": round(noise_ms, 3)}}))


if __name__ == "__main__":
    main()
