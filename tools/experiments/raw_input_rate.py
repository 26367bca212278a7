"""What the raw input path (loader workers decide and pack uint8 images, the device resizes / flips / normalises / pads:
data/transforms.py) delivers against the float32 path (SyntheticBatches: ready-made 3 x 800 x 1333 float batches), each on its
own: batches/s through DataLoader + DevicePrefetcher, bytes staged per step, and -- where PIL is installed -- what the
reference's per-image pipeline (PIL bilinear resize, flip, ToTensor, BGR255, mean/std) costs on one host core.
    python tools/experiments/raw_input_rate.py [images_per_batch] [workers] [batches]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.data.prefetch import DevicePrefetcher  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import RawSyntheticBatches, SyntheticBatches, make_raw_batch  # noqa: E402
from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import build_transforms, get_size  # noqa: E402

ims = int(sys.argv[1]) if len(sys.argv) > 1 else 2
workers = int(sys.argv[2]) if len(sys.argv) > 2 else 4
count = int(sys.argv[3]) if len(sys.argv) > 3 else 40


def staged_bytes(obj):
    if torch.is_tensor(obj):
        return obj.numel() * obj.element_size()
    if isinstance(obj, dict):
        return sum(staged_bytes(v) for v in obj.values())
    if isinstance(obj, (list, tuple)):
        return sum(staged_bytes(v) for v in obj)
    if hasattr(obj, "bbox"):
        return staged_bytes(obj.bbox) + staged_bytes(obj.extra_fields)
    if hasattr(obj, "polygon_start"):
        return staged_bytes([obj.coords, obj.polygon_start, obj.instance_start])
    return 0


def rate(source, transform, label):
    loader = torch.utils.data.DataLoader(source, batch_size=None, num_workers=workers, prefetch_factor=2, persistent_workers=True)
    nbytes = staged_bytes(next(iter(source)))
    data = DevicePrefetcher(loader, "cuda", depth=2, transform=transform)
    for _ in range(8):
        next(data)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(count):
        next(data)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / count
    data.close()
    del loader
    print(f"{label}: {dt * 1e3:.1f} ms per {ims}-image batch = {1 / dt:.1f} batches/s, {nbytes / 1e6:.2f} MB staged per step")
    return dt


cfg = get_defaults()
transform = build_transforms(cfg, is_train=True)
t_f32 = rate(SyntheticBatches(ims, seed0=1234, rank=0), None, "float32 path (SyntheticBatches)")
t_raw = rate(RawSyntheticBatches(ims, transform, seed0=1234, rank=0), transform, "raw path (uint8 + device transform)")
print(f"raw over float32: {t_f32 / t_raw:.2f}x the batches/s")

# the device half alone, and the host half alone in this process
raw, _ = transform.host(*make_raw_batch(ims, seed=1))
dev = {k: v.cuda() if torch.is_tensor(v) else v for k, v in raw.items()}
for _ in range(20):
    transform.device(dev)
a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
a.record()
for _ in range(50):
    transform.device(dev)
b.record()
torch.cuda.synchronize()
print(f"device half alone: {a.elapsed_time(b) / 50:.3f} ms per {ims}-image batch")
t0 = time.perf_counter()
for i in range(10):
    transform.host(*make_raw_batch(ims, seed=i))
print(f"make_raw_batch + host half in one process: {(time.perf_counter() - t0) / 10 * 1e3:.1f} ms per batch")

try:
    from PIL import Image
except ImportError:
    print("PIL is not installed: no host-pipeline comparison")
else:
    torch.set_num_threads(1)
    images, _ = make_raw_batch(4, seed=2)
    mean = torch.tensor(cfg.INPUT.PIXEL_MEAN).view(3, 1, 1)
    t0 = time.perf_counter()
    reps = 5
    for _ in range(reps):
        for img in images:
            pil = Image.fromarray(img.numpy())
            oh, ow = get_size(img.shape[1], img.shape[0], cfg.INPUT.MIN_SIZE_TRAIN[0], cfg.INPUT.MAX_SIZE_TRAIN)
            pil = pil.resize((ow, oh), Image.BILINEAR).transpose(Image.FLIP_LEFT_RIGHT)
            t = torch.from_numpy(np.asarray(pil).copy()).permute(2, 0, 1).float().div(255)  # ToTensor
            t = (t[[2, 1, 0]] * 255 - mean) / 1.0
    per = (time.perf_counter() - t0) / (reps * len(images))
    print(f"PIL pipeline on one core (resize, flip, ToTensor, BGR255, mean/std): {per * 1e3:.1f} ms per image = {1 / per:.0f} images/s "
          f"per core")
