"""TEST-ONLY: a scalar NumPy restatement of the reference's input transform, written from PIL's algorithm
(libImaging/Resample.c: precompute_coeffs / normalize_coeffs_8bpc / ImagingResampleHorizontal_8bpc / ...Vertical_8bpc) and
mb/data/transforms/transforms.py:27-120 + mb/structures/image_list.py:29-70, independent of the package's C++ / HIP code:
python floats are IEEE doubles and are combined in PIL's order, the 8-bit arithmetic is exact integers, the normalisation is
numpy float32 (one IEEE operation per step).  Also the fixture's cases and their seeded inputs."""
import zlib

import numpy as np

PRECISION_BITS = 32 - 8 - 2

# (in_h, in_w, out_h, out_w): upscale on both axes; non-integer downscale (seven taps); vertical pass only; horizontal pass
# only; wide support; a single output pixel; identity (no pass)
CASES = [(48, 64, 80, 106), (97, 61, 43, 27), (120, 90, 37, 90), (33, 50, 33, 133), (300, 200, 64, 43), (7, 5, 1, 1),
         (30, 40, 30, 40)]
STD_COCO = (57.375, 57.12, 58.395)
MEAN = (102.9801, 115.9465, 122.7717)


def case_input(index):
    """The seeded uint8 [in_h, in_w, 3] input of CASES[index] (numpy's legacy RandomState: a frozen stream)."""
    in_h, in_w = CASES[index][:2]
    return np.random.RandomState(9000 + index).randint(0, 256, (in_h, in_w, 3)).astype(np.uint8)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def _triangle(x):
    if x < 0.0:
        x = -x
    return 1.0 - x if x < 1.0 else 0.0


def axis_coefficients(in_size, out_size):
    """Per output position: (first input position, the taps' integer weights)."""
    scale = float(np.float32(in_size) - np.float32(0)) / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = 0.0 + (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)       # int(): truncation toward zero, C's (int)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [_triangle((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((xmin, [int(0.5 + v * (1 << PRECISION_BITS)) for v in w]))
    return out


def resample_axis(img, out_size, axis):
    """One 8-bit pass of uint8 [h, w, 3] along ``axis`` (0 = vertical, 1 = horizontal)."""
    img = np.moveaxis(img, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + img.shape[1:], dtype=np.uint8)
    for xx, (xmin, k) in enumerate(axis_coefficients(img.shape[0], out_size)):
        acc = np.full(img.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for i, kv in enumerate(k):
            acc += img[xmin + i] * kv
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis)


def pil_resize(img, out_h, out_w):
    """PIL ``Image.resize((out_w, out_h), BILINEAR)`` of an RGB uint8 image: horizontal pass, then vertical, each only when
    its size changes."""
    if out_w != img.shape[1]:
        img = resample_axis(img, out_w, 1)
    if out_h != img.shape[0]:
        img = resample_axis(img, out_h, 0)
    return img


def transform(images, out_sizes, flips, mean, std, to_bgr255, pad_hw):
    """float32 [B, 3, pad_h, pad_w]: Resize, flips, ToTensor, Normalize, zero padding."""
    out = np.zeros((len(images), 3) + tuple(pad_hw), dtype=np.float32)
    mean, std = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    for b, (img, (oh, ow), (flip_h, flip_v)) in enumerate(zip(images, out_sizes, flips)):
        r = pil_resize(img, oh, ow)
        if flip_h:
            r = r[:, ::-1]
        if flip_v:
            r = r[::-1]
        if to_bgr255:
            v = r[:, :, ::-1].astype(np.float32)
        else:
            v = r.astype(np.float32) / np.float32(255)
        v = (v - mean) / std
        assert v.dtype == np.float32
        out[b, :, :oh, :ow] = v.transpose(2, 0, 1)
    return out


def pack(images, out_sizes, flips):
    """The byte buffer and the [B, 7] int32 descriptors of ``_C.transform_images``."""
    desc, off = [], 0
    for img, (oh, ow), (fh, fv) in zip(images, out_sizes, flips):
        desc.append([off, img.shape[0], img.shape[1], oh, ow, int(fh), int(fv)])
        off += img.size
    return np.concatenate([np.ascontiguousarray(i).reshape(-1) for i in images]), np.asarray(desc, dtype=np.int32)
