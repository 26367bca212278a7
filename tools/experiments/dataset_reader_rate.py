"""What the dataset reader delivers on the host, on its own: images/s of JPEG decode + target building + the host half of the
input transform (data/datasets.py, data/build.py), per loader worker and with several workers, over a throw-away dataset
of smooth JPEG images at the common COCO sizes with seven polygon instances each.  No GPU is touched.
    python tools/experiments/dataset_reader_rate.py [--images 96] [--workers 1 4 8 16] [--out FILE]"""
import argparse
import json
import os
import platform
import sys
import tempfile
import time

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.data.build import make_data_loader  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCODataset  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import RAW_SIZES  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms  # noqa: E402


def write_dataset(root, count):
    rs = np.random.RandomState(0)
    images, anns = [], []
    for i in range(count):
        h, w = RAW_SIZES[i % len(RAW_SIZES)]
        small = rs.randint(0, 256, (h // 16 + 1, w // 16 + 1, 3)).astype(np.uint8)  # smooth content: JPEG sizes like photographs'
        Image.fromarray(small).resize((w, h), Image.BICUBIC).save(os.path.join(root, f"{i}.jpg"), quality=90)
        images.append({"id": i, "file_name": f"{i}.jpg", "width": w, "height": h})
        for k in range(7):
            bw, bh = rs.randint(24, w // 2), rs.randint(24, h // 2)
            x, y = rs.randint(0, w - bw), rs.randint(0, h - bh)
            poly = [x, y, x + bw, y, x + bw, y + bh // 2, x + bw // 2, y + bh, x, y + bh, x + 2, y + bh // 2]
            anns.append({"id": len(anns), "image_id": i, "category_id": 1 + k % 3, "bbox": [x, y, bw, bh], "iscrowd": 0,
                         "segmentation": [[float(v) for v in poly]]})
    ann_file = os.path.join(root, "instances.json")
    with open(ann_file, "w") as f:
        json.dump({"images": images, "annotations": anns, "categories": [{"id": c, "name": f"c{c}"} for c in (1, 2, 3)]}, f)
    return ann_file


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=96)
    ap.add_argument("--workers", type=int, nargs="+", default=[1, 4, 8, 16])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    cfg = get_defaults()
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", 2])
    cfg.freeze()
    transform = build_transforms(cfg, is_train=True)
    lines = [f"dataset reader throughput: JPEG decode + targets + host half of the input transform, {args.images} images of "
             f"{' / '.join(f'{h}x{w}' for h, w in RAW_SIZES)} (h x w), 7 polygon instances each, 2 images per batch",
             f"machine: {platform.processor() or platform.machine()}, {len(os.sched_getaffinity(0))} CPUs in the affinity mask"
             f"{' (' + os.environ['OMP_NUM_THREADS'] + ' allowed: OMP_NUM_THREADS)' if 'OMP_NUM_THREADS' in os.environ else ''}, "
             f"python {platform.python_version()}, PIL {Image.__version__}"]
    with tempfile.TemporaryDirectory() as root:
        dataset = COCODataset(write_dataset(root, args.images), root, True)
        passes = 3
        for workers in args.workers:
            loader = make_data_loader(cfg, dataset, transform, True, 0, 1, num_workers=workers, max_iter=passes * args.images // 2)
            it = iter(loader)
            for _ in range(max(2 * workers, 4)):  # workers started, first batches through
                next(it)
            t0, n = time.perf_counter(), 0
            for raw, _ in it:
                n += len(raw["image_sizes"])
            dt = time.perf_counter() - t0
            lines.append(f"workers {workers:2d}: {n / dt:8.1f} images/s  ({n / dt / workers:6.1f} per worker)")
    lines.append("the training step consumes ~60 images/s per GPU (student-teacher step, 2 images in ~33 ms)")
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
