"""TEST-ONLY: an independent NumPy / plain-Python restatement of scale jitter with a fixed-size crop, built on the two
restatements that already exist (tests/input_transform_ref.py, tests/rle_targets_reference.py) and sharing nothing with the
package's C++ / HIP / Python code:

  * the window transform = ``input_transform_ref.transform`` at the FULL resized size, then a literal slice and a zero pad;
  * the draw rule of include/ovis_hip.h in plain Python on a ``random.Random``;
  * mask targets through a literally sliced dense canvas.

Also the cases of tests/golden/scale_crop.npz (the reference's own BoxList.crop / PolygonInstance.crop / BinaryMaskList.crop).
"""
import numpy as np

from tests import input_transform_ref as T
from tests import rle_targets_reference as rt

MAX_REDRAWS = 8


# ---- pixels ---------------------------------------------------------------------------------------------------------------
def window_transform(images, out_sizes, flips, windows, mean, std, to_bgr255, pad_hw):
    """float32 [B, 3, pad_h, pad_w]: every image resized to its full (out_h, out_w), flipped and normalised by
    ``T.transform`` on a canvas of its own, then ``[win_y : win_y + win_h, win_x : win_x + win_w]`` copied to the corner of a
    zero canvas.  windows: (win_y, win_x, win_h, win_w) in the frame of the resized, flipped image."""
    out = np.zeros((len(images), 3) + tuple(pad_hw), dtype=np.float32)
    for b, (img, size, flip, (wy, wx, wh, ww)) in enumerate(zip(images, out_sizes, flips, windows)):
        full = T.transform([img], [size], [flip], mean, std, to_bgr255, size)[0]
        assert 0 <= wy and 0 <= wx and wy + wh <= size[0] and wx + ww <= size[1]
        out[b, :, :wh, :ww] = full[:, wy:wy + wh, wx:wx + ww]
    return out


def pack(images, out_sizes, flips, windows):
    """The byte buffer and the [B, 11] int32 descriptors of ``_C.transform_images_window``."""
    data, desc = T.pack(images, out_sizes, flips)
    return data, np.concatenate([desc, np.asarray(windows, dtype=np.int32).reshape(len(images), 4)], axis=1)


# ---- the draw rule --------------------------------------------------------------------------------------------------------
def jittered_size(in_h, in_w, s, crop_hw):
    r = min(crop_hw[0] * s / in_h, crop_hw[1] * s / in_w)
    return max(1, round(in_h * r)), max(1, round(in_w * r))


def window_of(fy, fx, out_hw, crop_hw):
    win_y = round(fy * max(out_hw[0] - crop_hw[0], 0))
    win_x = round(fx * max(out_hw[1] - crop_hw[1], 0))
    return win_y, win_x, min(crop_hw[0], out_hw[0] - win_y), min(crop_hw[1], out_hw[1] - win_x)


def draws(rng, in_hw, scale_range, crop_hw, flip_probs, survives=None):
    """One image: -> (out_h, out_w, flip_h, flip_v, window, number of windows drawn).  ``survives(out_hw, flip_h, flip_v,
    window)`` says whether a ground-truth box is left (None: the image has no box, nothing is redrawn)."""
    s = rng.uniform(*scale_range)
    out_hw = jittered_size(in_hw[0], in_hw[1], s, crop_hw)
    flip_h = rng.random() < flip_probs[0]
    flip_v = rng.random() < flip_probs[1]
    drawn = 0
    while True:
        fy = rng.random()
        fx = rng.random()
        window = window_of(fy, fx, out_hw, crop_hw)
        drawn += 1
        if survives is None or drawn == 1 + MAX_REDRAWS or survives(out_hw, flip_h, flip_v, window):
            return out_hw[0], out_hw[1], flip_h, flip_v, window, drawn


# ---- the window grid both the host twin and the device kernel are held to --------------------------------------------------------
INPUTS = [(5, 7), (33, 47), (16, 1), (1, 16)]
FLIPS = [(False, False), (True, False), (False, True), (True, True)]


def image(h, w, seed=0):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def out_sizes(h, w):
    """Up on both axes, down on both, the vertical pass only (out_w == in_w), the horizontal only, neither."""
    return [(round(h * 2.3), round(w * 2.3)), (max(1, h // 2), max(1, (2 * w) // 3)), (2 * h + 1, w), (h, 3 * w - 1), (h, w)]


def windows(oh, ow):
    """At offset 0, interior, flush with the far edge, the whole image: (win_y, win_x, win_h, win_w)."""
    ch, cw = max(1, (oh + 1) // 2), max(1, (2 * ow) // 3)
    return [(0, 0, ch, cw), ((oh - ch) // 2, (ow - cw) // 2, ch, cw), (oh - ch, ow - cw, ch, cw), (0, 0, oh, ow)]


def window_cases():
    """(images, out sizes, flips, windows, pad_hw): per input, resize and flip combination one batch of the four windows on
    a canvas larger than every window (padding), and the whole image once more on a canvas of exactly its size."""
    for k, (h, w) in enumerate(INPUTS):
        img = image(h, w, 50 + k)
        for oh, ow in out_sizes(h, w):
            for flip in FLIPS:
                yield [img] * 4, [(oh, ow)] * 4, [flip] * 4, windows(oh, ow), (oh + 3, ow + 5)
            yield [img], [(oh, ow)], [FLIPS[3]], [(0, 0, oh, ow)], (oh, ow)


# ---- boxes ----------------------------------------------------------------------------------------------------------------
def crop_boxes(boxes, window):
    """float32 [N, 4] and the keep mask of crop + clip_to_image(remove_empty=True): window = (win_y, win_x, win_h, win_w)."""
    wy, wx, wh, ww = window
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4).copy()
    b[:, 0::2] = np.clip(b[:, 0::2] - np.float32(wx), np.float32(0), np.float32(ww))
    b[:, 1::2] = np.clip(b[:, 1::2] - np.float32(wy), np.float32(0), np.float32(wh))
    b[:, 0::2] = np.clip(b[:, 0::2], np.float32(0), np.float32(ww - 1))
    b[:, 1::2] = np.clip(b[:, 1::2], np.float32(0), np.float32(wh - 1))
    return b, (b[:, 3] > b[:, 1]) & (b[:, 2] > b[:, 0])


# ---- masks ----------------------------------------------------------------------------------------------------------------
def mask_window(box, width, height):
    """(xmin, ymin, xmax, ymax) ints of BinaryMaskList.crop on a (width, height) mask for a python-number box."""
    xmin, ymin, xmax, ymax = [round(float(v)) for v in box]
    xmin, ymin = min(max(xmin, 0), width - 1), min(max(ymin, 0), height - 1)
    xmax, ymax = max(min(max(xmax, 0), width), xmin + 1), max(min(max(ymax, 0), height), ymin + 1)
    return xmin, ymin, xmax, ymax


def project_window(masks, gt_index, boxes, size_hw, flip_h, flip_v, window, resolution):
    """float32 [P, M, M]: masks bool [G, h0, w0] resized to ``size_hw`` and flipped (the dense canvas), SLICED to
    ``window`` = (win_y, win_x, win_h, win_w), then cropped to each box -- given in the window's frame -- and resized."""
    wy, wx, wh, ww = window
    canvas = rt.resized_flipped(masks, size_hw, flip_h, flip_v)
    return rt.crop_resize(np.ascontiguousarray(canvas[:, wy:wy + wh, wx:wx + ww]), gt_index, boxes, resolution)


# ---- the cases of tests/golden/scale_crop.npz -------------------------------------------------------------------------------
FRAME = (40, 30)   # (width, height)
# xyxy boxes in the frame: inside every window; straddling the left, top, right and bottom edge of the interior window; wholly
# outside it; touching the frame's last pixel; one pixel wide; the whole frame; fractional, landing on .5
GOLDEN_BOXES = np.asarray([[8, 7, 20, 18], [2, 8, 12, 15], [10, 1, 18, 9], [22, 10, 35, 16], [12, 20, 20, 28],
                           [31, 25, 38, 29], [0, 0, 3, 2], [30, 20, 39, 29], [15, 12, 15, 20], [0, 0, 39, 29],
                           [6.5, 5.5, 24.5, 22.5], [4.25, 3.75, 5.0, 4.0]], dtype=np.float32)
# (xmin, ymin, xmax, ymax): interior; flush with the far edges; the frame; larger than the frame; larger and shifted
GOLDEN_WINDOWS = [(5, 4, 30, 24), (20, 10, 40, 30), (0, 0, 40, 30), (0, 0, 50, 36), (-3, -2, 50, 36)]
# per instance a list of polygons (flat x, y pairs) in the frame
GOLDEN_POLYGONS = [[[8, 7, 20, 7, 20, 18, 8, 18]], [[2, 8, 12, 8, 7.5, 15.25]], [[30, 20, 39, 20, 39, 29, 30, 29], [1, 1, 4, 1, 4, 3]]]


def golden_masks():
    """bool [3, 30, 40]: the seeded bitmaps BinaryMaskList.crop is recorded on."""
    return rt.salt_and_pepper(3, FRAME[1], FRAME[0], 77)
