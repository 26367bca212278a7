"""TEST-ONLY: a dense NumPy restatement of the chain ``_C.project_rle_masks`` evaluates (csrc/rle_targets.hip): the bitmap
ground truth of an image resized to the training size, flipped, cropped to each positive's box and resized to M x M --
BinaryMaskList.resize / .transpose / .crop / .resize of the reference (structures/segmentation_mask.py:113-158) under the
EXACT form of "bilinear resample, truncate to uint8": a pixel is 1 iff every tap with a non-zero weight is set.

Per axis n_in -> n_out, in fp32 (NumPy does not contract):  scale = n_in / n_out;  src = max((d + 0.5) * scale - 0.5, 0);
i0 = min(floor(src), n_in - 1);  i1 = min(i0 + 1, n_in - 1);  lam = src - floor(src).  Every canvas is built here -- the
kernel builds none -- so the two share nothing but the formulas.
"""
import numpy as np

F32 = np.float32


def axis_taps(n_in, n_out):
    """(i0 int64 [n_out], i1 int64 [n_out], lam float32 [n_out]) of one axis."""
    d = np.arange(n_out, dtype=F32)
    scale = F32(n_in) / F32(n_out)
    src = np.maximum((d + F32(0.5)) * scale - F32(0.5), F32(0))
    assert src.dtype == F32
    fl = np.floor(src)
    lam = src - fl
    i0 = np.minimum(fl, F32(n_in - 1))
    i1 = np.minimum(i0 + F32(1), F32(n_in - 1))
    return i0.astype(np.int64), i1.astype(np.int64), lam


def _taps(mask, out_h, out_w):
    y0, y1, ly = axis_taps(mask.shape[-2], out_h)
    x0, x1, lx = axis_taps(mask.shape[-1], out_w)
    v00, v01 = mask[..., y0[:, None], x0[None, :]], mask[..., y0[:, None], x1[None, :]]
    v10, v11 = mask[..., y1[:, None], x0[None, :]], mask[..., y1[:, None], x1[None, :]]
    return (v00, v01, v10, v11), ly[:, None], lx[None, :]


def resize_rule(mask, out_h, out_w):
    """bool [..., out_h, out_w] of a bool [..., h, w] mask: every tap with a non-zero weight is set."""
    (v00, v01, v10, v11), ly, lx = _taps(np.asarray(mask, dtype=bool), out_h, out_w)
    zy, zx = ly == 0, lx == 0
    return v00 & (zx | v01) & (zy | v10) & (zx | zy | v11)


def resize_exact(mask, out_h, out_w):
    """float64 [..., out_h, out_w]: the interpolated value with the restatement's own fp32 lams, the sum in fp64."""
    (v00, v01, v10, v11), ly, lx = _taps(np.asarray(mask, dtype=np.float64), out_h, out_w)
    ly, lx = ly.astype(np.float64), lx.astype(np.float64)
    return (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11)


def crop_window(box, width, height):
    """(xmin, ymin, xmax, ymax) ints of BinaryMaskList.crop on a (width, height) mask: round half to even in fp32, the
    clamps, at least one pixel."""
    b = np.rint(np.asarray(box, dtype=F32))
    xmin, ymin = min(max(b[0], 0), width - 1), min(max(b[1], 0), height - 1)
    xmax, ymax = max(min(max(b[2], 0), width), xmin + 1), max(min(max(b[3], 0), height), ymin + 1)
    return int(xmin), int(ymin), int(xmax), int(ymax)


def resized_flipped(masks, size_hw, flip_h, flip_v):
    """bool [G, h1, w1]: stage 1 of the chain, the rule h0 x w0 -> h1 x w1 and the flips."""
    r = resize_rule(masks, size_hw[0], size_hw[1])
    if flip_v:
        r = r[..., ::-1, :]
    if flip_h:
        r = r[..., :, ::-1]
    return r


def crop_resize(frame_masks, gt_index, boxes, resolution):
    """float32 [P, M, M]: stage 2 -- crop the [G, h1, w1] masks to each box and resize by the rule."""
    h1, w1 = frame_masks.shape[-2:]
    out = np.zeros((len(boxes), resolution, resolution), dtype=F32)
    for p, (g, box) in enumerate(zip(gt_index, boxes)):
        xmin, ymin, xmax, ymax = crop_window(box, w1, h1)
        out[p] = resize_rule(frame_masks[int(g), ymin:ymax, xmin:xmax], resolution, resolution)
    return out


def project(masks, gt_index, boxes, size_hw, flip_h, flip_v, resolution):
    """The whole chain: masks bool [G, h0, w0] -> float32 [P, M, M]."""
    return crop_resize(resized_flipped(masks, size_hw, flip_h, flip_v), gt_index, boxes, resolution)


# the shapes and boxes the tests share
SHAPES = [((37, 50), (21, 40)), ((48, 64), (100, 75)), ((40, 56), (40, 56)), ((61, 45), (122, 90))]
BIG_SHAPE = ((480, 640), (800, 1067))
FLIPS = [(False, False), (True, False), (False, True), (True, True)]


def salt_and_pepper(g, h, w, seed):
    return np.random.default_rng(seed).random((g, h, w)) > 0.35


def edge_boxes(width, height):
    """The eight edge boxes of tests/test_targets_gpu.py (outside the image, degenerate, .5 ties, the whole image) in a
    (width, height) frame, then crops of 14, 28 and 42 pixels (clamped by the frame) so that lam == 0."""
    W, H = float(width), float(height)
    boxes = [[-5.0, -3.0, 10.5, 7.5], [W - 3.0, H - 2.0, W + 9.0, H + 4.0], [10.5, 10.5, 10.6, 10.7], [0.5, 1.5, 2.5, 3.5],
             [0.0, 0.0, W - 1.0, H - 1.0], [30.0, 40.0, 30.0, 40.0], [2.5, 3.5, 100.5, 7.5], [50.2, 60.8, 51.1, 199.9]]
    for k, (x0, y0) in zip((14, 28, 42), ((1.0, 2.0), (3.0, 0.0), (0.0, 1.0))):
        boxes.append([x0 + 0.2, y0 - 0.3, x0 + k - 0.4, y0 + k + 0.3])
        boxes.append([x0, y0, x0 + k, y0 + 14.0])
    return np.asarray(boxes, dtype=F32)


def random_boxes(n, width, height, seed):
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2)) * np.array([max(width - 12, 1), max(height - 12, 1)])
    wh = rng.random((n, 2)) * np.array([width * 0.6, height * 0.6]) + 6
    return np.concatenate([xy, np.minimum(xy + wh, [width - 1, height - 1])], 1).astype(F32)


GOLDEN_RESOLUTION, GOLDEN_BOXES = 14, 24


def golden_cases():
    """The cases of tests/golden/rle_targets.npz: (k, (h0, w0), (h1, w1), flip_h, flip_v, seed of the source bitmap, seed
    of the boxes)."""
    k = 0
    for s, (src, dst) in enumerate(SHAPES + [BIG_SHAPE]):
        for flip_h, flip_v in FLIPS:
            yield k, src, dst, flip_h, flip_v, 100 + s, 1000 + k
            k += 1
