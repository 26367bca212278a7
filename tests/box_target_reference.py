"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of the reference's box-target and proposal arithmetic.

No torch, nothing from the package and nothing from oracle/: this module exists to pin them (tests/test_box_target_reference.py)
and to judge the HIP kernels at their edges (tests/test_box_targets_edges_gpu.py).  Every function names the lines of
maskrcnn_benchmark/ it restates.

Two kinds of numbers, kept apart on purpose:

* DECISIONS are restated in ``np.float32``, operation by operation, in the order of ``boxlist_iou`` / ``devIoU``: the IoU
  itself, argmax with the first maximum winning, ``< low``, ``< high``, ``== best_per_gt``, ``> thr`` / ``>= thr`` and the
  size test against ``min_size``.  They are IEEE ``+ - * / max min`` (the library is built with contraction off and its
  division is correctly rounded), so a kernel has to agree bit for bit.  An fp64 IoU would decide ties differently.
* VALUES (``BoxCoder.encode`` deltas, ``BoxCoder.decode`` boxes, the smooth-L1 loss and gradient) are computed in fp64 from
  the fp32 inputs; the tests bound a kernel's distance from them.

The last section holds the edge inputs both test modules share, so the CPU pins run on exactly what the GPU tests run on.
"""
import math

import numpy as np

F32 = np.float32
_ONE, _ZERO, _HALF = F32(1), F32(0), F32(0.5)
EPS = 2.0 ** -24  # one fp32 rounding, relative (half an ulp)


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------ decisions, float32
def area_f32(b):
    """structures/bounding_box.py:226-230 (BoxList.area, xyxy): (x2 - x1 + 1) * (y2 - y1 + 1)."""
    b = _f32(b)
    return (b[:, 2] - b[:, 0] + _ONE) * (b[:, 3] - b[:, 1] + _ONE)


def iou_f32(gt, boxes):
    """structures/boxlist_ops.py:75-89 (boxlist_iou) -> [G, P] float32.  csrc/cuda/nms.cu:13-21 (devIoU) is the same
    expression: max / min of the corners, ``right - left + 1`` clamped at 0, ``inter / (Sa + Sb - inter)``."""
    gt, boxes = _f32(gt), _f32(boxes)
    area1, area2 = area_f32(gt), area_f32(boxes)
    lt = np.maximum(gt[:, None, :2], boxes[None, :, :2])
    rb = np.minimum(gt[:, None, 2:], boxes[None, :, 2:])
    wh = np.maximum(rb - lt + _ONE, _ZERO)
    inter = wh[:, :, 0] * wh[:, :, 1]
    iou = inter / (area1[:, None] + area2[None, :] - inter)
    assert iou.dtype == np.float32
    return iou


BELOW_LOW_THRESHOLD, BETWEEN_THRESHOLDS = -1, -2


def matcher(iou, high, low, allow_low_quality):
    """modeling/matcher.py:64-81 and set_low_quality_matches_ (:83-112): per column the first argmax; -1 below ``low``, -2
    between the thresholds; with low-quality matches every column that EQUALS a row's maximum anywhere gets its argmax
    back.  The thresholds are compared as float32, like a float32 tensor against a Python scalar."""
    assert iou.dtype == np.float32 and iou.ndim == 2 and iou.size > 0
    high, low = F32(high), F32(low)
    vals = iou.max(axis=0)
    all_matches = iou.argmax(axis=0).astype(np.int64)  # the first maximum wins
    matches = all_matches.copy()
    matches[vals < low] = BELOW_LOW_THRESHOLD
    matches[(vals >= low) & (vals < high)] = BETWEEN_THRESHOLDS
    if allow_low_quality:
        best_per_gt = iou.max(axis=1)
        tied = (iou == best_per_gt[:, None]).any(axis=0)
        matches[tied] = all_matches[tied]
    return matches


def ties_per_gt(iou):
    """How many columns equal each row's maximum (the pairs of matcher.py:94-96), and that maximum."""
    best = iou.max(axis=1)
    return (iou == best[:, None]).sum(axis=1), best


def small_box_keep_f32(boxes, min_size):
    """structures/boxlist_ops.py:43-47 (remove_small_boxes) on xyxy boxes: bounding_box.py:66-70 forms
    ``w = x2 - x1 + 1`` and the test is ``(ws >= min_size) & (hs >= min_size)``, in float32."""
    b = _f32(boxes)
    m = F32(min_size)
    return ((b[..., 2] - b[..., 0] + _ONE) >= m) & ((b[..., 3] - b[..., 1] + _ONE) >= m)


def greedy_nms_f32(boxes, alive, thr, ge=False):
    """csrc/cuda/nms.cu:59-62 and :112-123 on boxes that are already in descending score order: walk the boxes, keep one
    that no kept box suppressed, suppress every later box whose devIoU with it is ``> thr`` (``>= thr`` with ``ge``).
    ``alive`` (bool [K] or None) marks the boxes that take part at all (the others were removed in front of the NMS,
    rpn/inference.py:115-116).  -> kept indices, ascending."""
    b = _f32(boxes)
    k = b.shape[0]
    removed = np.zeros(k, dtype=bool) if alive is None else ~np.asarray(alive, dtype=bool)
    area = area_f32(b)
    thr = F32(thr)
    keep = []
    for i in range(k):
        if removed[i]:
            continue
        keep.append(i)
        if i + 1 == k:
            break
        r = b[i + 1:]
        w = np.maximum(np.minimum(b[i, 2], r[:, 2]) - np.maximum(b[i, 0], r[:, 0]) + _ONE, _ZERO)
        h = np.maximum(np.minimum(b[i, 3], r[:, 3]) - np.maximum(b[i, 1], r[:, 1]) + _ONE, _ZERO)
        inter = w * h
        iou = inter / (area[i] + area[i + 1:] - inter)
        assert iou.dtype == np.float32
        removed[i + 1:] |= (iou >= thr) if ge else (iou > thr)
    return np.asarray(keep, dtype=np.int64)


# ------------------------------------------------------------------ values, float64
def encode(reference_boxes, proposals, weights):
    """modeling/box_coder.py:32-50 (BoxCoder.encode) in fp64 from the fp32 boxes."""
    r = _f32(reference_boxes).astype(np.float64)
    p = _f32(proposals).astype(np.float64)
    ex_w, ex_h = p[:, 2] - p[:, 0] + 1, p[:, 3] - p[:, 1] + 1
    ex_cx, ex_cy = p[:, 0] + 0.5 * ex_w, p[:, 1] + 0.5 * ex_h
    gt_w, gt_h = r[:, 2] - r[:, 0] + 1, r[:, 3] - r[:, 1] + 1
    gt_cx, gt_cy = r[:, 0] + 0.5 * gt_w, r[:, 1] + 0.5 * gt_h
    wx, wy, ww, wh = (float(F32(v)) for v in weights)
    return np.stack((wx * (gt_cx - ex_cx) / ex_w, wy * (gt_cy - ex_cy) / ex_h, ww * np.log(gt_w / ex_w),
                     wh * np.log(gt_h / ex_h)), axis=1)


def decode(rel_codes, boxes, weights, xform_clip=math.log(1000.0 / 16)):
    """modeling/box_coder.py:62-95 (BoxCoder.decode) in fp64: rel_codes [R, 4K], boxes [R, 4] -> [R, 4K].  The clip of
    dw / dh is the float32 value a float32 tensor is clamped to."""
    c = _f32(rel_codes).astype(np.float64)
    b = _f32(boxes).astype(np.float64)
    widths, heights = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
    ctr_x, ctr_y = b[:, 0] + 0.5 * widths, b[:, 1] + 0.5 * heights
    wx, wy, ww, wh = (float(F32(v)) for v in weights)
    clip = float(F32(xform_clip))
    dx, dy = c[:, 0::4] / wx, c[:, 1::4] / wy
    dw, dh = np.minimum(c[:, 2::4] / ww, clip), np.minimum(c[:, 3::4] / wh, clip)
    pcx, pcy = dx * widths[:, None] + ctr_x[:, None], dy * heights[:, None] + ctr_y[:, None]
    pw, ph = np.exp(dw) * widths[:, None], np.exp(dh) * heights[:, None]
    out = np.zeros_like(c)
    out[:, 0::4] = pcx - 0.5 * pw
    out[:, 1::4] = pcy - 0.5 * ph
    out[:, 2::4] = pcx + 0.5 * pw - 1
    out[:, 3::4] = pcy + 0.5 * ph - 1
    return out


def rpn_targets(gt, anchors, visible, high, low, allow_lq, weights):
    """modeling/rpn/loss.py:42-89 (match_targets_to_anchors + prepare_targets with generate_rpn_labels, :134-137):
    labels ``matched >= 0``, then in this order background (-1 -> 0), not visible -> -1, between the thresholds -> -1
    (:68-79); regression targets are the encode of ``gt[matched.clamp(min=0)]`` (:52, :82-84).
    -> (labels int64 [A], fp64 targets [A, 4])."""
    gt, anchors = _f32(gt), _f32(anchors)
    matched = matcher(iou_f32(gt, anchors), high, low, allow_lq)
    labels = (matched >= 0).astype(np.int64)
    labels[matched == BELOW_LOW_THRESHOLD] = 0
    labels[~np.asarray(visible, dtype=bool)] = -1
    labels[matched == BETWEEN_THRESHOLDS] = -1
    return labels, encode(gt[np.maximum(matched, 0)], anchors, weights)


def match_encode(gt, gt_labels, props, high, low, weights, between_keeps_label):
    """modeling/roi_heads/box_head/loss.py:46-77 (between_keeps_label False: below -> label 0, between -> label -1) and
    mask_head/loss.py:60-77 (True: only below -> 0, so a between-thresholds proposal keeps the label of the ground truth
    its clamped index points at, which is ground truth 0): Matcher without low-quality matches, ``matched.clamp(min=0)``,
    labels, and the encode against the clamped match (box_head/loss.py:79-82).
    -> (matched index int64 [P], labels int64 [P], fp64 targets [P, 4] or None without weights)."""
    gt, props = _f32(gt), _f32(props)
    matched = matcher(iou_f32(gt, props), high, low, False)
    idx = np.maximum(matched, 0)
    labels = np.asarray(gt_labels, dtype=np.int64)[idx].copy()
    labels[matched == BELOW_LOW_THRESHOLD] = 0
    if not between_keeps_label:
        labels[matched == BETWEEN_THRESHOLDS] = -1
    return idx, labels, (None if weights is None else encode(gt[idx], props, weights))


def anchors_of(topk_idx, cell_anchors, feat_w, stride):
    """modeling/rpn/anchor_generator.py:73-93 (grid_anchors: shifts ``arange(0, W * stride, stride)``, meshgrid (y, x),
    ``shifts.view(-1, 1, 4) + base.view(1, -1, 4)``) read at flat indices in the (y, x, a) order of
    rpn/inference.py:87-102 -> float32 [..., 4]."""
    idx = np.asarray(topk_idx, dtype=np.int64)
    cell = _f32(cell_anchors)
    a_n = cell.shape[0]
    a, pos = idx % a_n, idx // a_n
    y, x = pos // feat_w, pos % feat_w
    sx, sy = (x * int(stride)).astype(np.float32), (y * int(stride)).astype(np.float32)
    return np.stack((sx, sy, sx, sy), axis=-1) + cell[a]


# roundings on the longest path of csrc/rpn.hip:39-48 to one output coordinate -- x2 through the centre:
#   widths = (ax2 - ax1) + 1 : 2      dx = c0 / wx : 1      dx * widths : 1      ... + ctr_x : 1
#   pcx + 0.5 * pw : 1 (0.5 * pw is exact)      ... - 1 : 1                                                   = 7
# (through the width it is 6: widths 2, c2 / ww 1, expf(dw) * widths 1, the same last two) -- plus expf itself, 2 ulp =
# 4 * 2^-24.  Fixed from the code before anything was measured.
DECODE_ROUNDINGS = 7 + 4


def rpn_decode(box_regression, topk_idx, cell_anchors, image_wh, weights, xform_clip, stride):
    """modeling/rpn/inference.py:90-114: gather of the top-k candidates' deltas (permute_and_flatten: channel a * 4 + c
    at (y, x)) and anchors, BoxCoder.decode, clip_to_image (structures/bounding_box.py:214-219, clamp to
    [0, w - 1] x [0, h - 1]) in fp64.  box_regression [N, 4A, H, W] float32 (any strides), topk_idx [N, K].
    -> (boxes fp64 [N, K, 4], bound [N, K, 4]): ``DECODE_ROUNDINGS * 2^-24 * (|ctr| + |d| * size + e^dw * size + 1)`` of
    the element's axis; 0 where the unclipped value lies further than that outside the image, because the clamp then
    returns the border itself, which is exact."""
    reg = np.asarray(box_regression)
    assert reg.dtype == np.float32
    n, c4, h, w = reg.shape
    idx = np.asarray(topk_idx, dtype=np.int64)
    a_n = c4 // 4
    anchors = anchors_of(idx, cell_anchors, w, stride).astype(np.float64)          # [N, K, 4]
    a, pos = idx % a_n, idx // a_n
    y, x = pos // w, pos % w
    img = np.arange(n)[:, None]
    codes = np.stack([reg[img, a * 4 + c, y, x] for c in range(4)], axis=-1).astype(np.float64)
    wts = np.array([float(F32(v)) for v in weights])
    clip = float(F32(xform_clip))
    size = anchors[..., 2:] - anchors[..., :2] + 1                                  # widths, heights
    ctr = anchors[..., :2] + 0.5 * size
    d = codes[..., :2] / wts[:2]
    dwh = np.minimum(codes[..., 2:] / wts[2:], clip)
    pc = d * size + ctr
    pwh = np.exp(dwh) * size
    raw = np.concatenate((pc - 0.5 * pwh, pc + 0.5 * pwh - 1), axis=-1)
    hi = (np.asarray(image_wh, dtype=np.float64) - 1)[:, None, :]                   # [N, 1, 2]
    hi = np.concatenate((hi, hi), axis=-1)
    mag = np.abs(ctr) + np.abs(d) * size + pwh + 1
    bound = DECODE_ROUNDINGS * EPS * np.concatenate((mag, mag), axis=-1)
    bound = np.where((raw - bound > hi) | (raw + bound < 0), 0.0, bound)
    return np.clip(raw, 0.0, hi), bound


def small_box_verdict(boxes64, bound, min_size):
    """What the float32 size test (small_box_keep_f32) must answer for ANY float32 box within ``bound`` of ``boxes64``:
    rounding is monotone, so the float32 size of the narrowest / widest such box brackets the kernel's.  -> (keep, decided):
    ``decided`` is False where the two ends disagree, i.e. the fp64 size is within the bound of ``min_size``."""
    m = F32(min_size)

    def size32(lo, hi):
        return (hi.astype(np.float32) - lo.astype(np.float32)) + _ONE

    x1, y1, x2, y2 = (boxes64[..., i] for i in range(4))
    b1, c1, b2, c2 = (bound[..., i] for i in range(4))
    keep_narrow = (size32(x1 + b1, x2 - b2) >= m) & (size32(y1 + c1, y2 - c2) >= m)
    keep_wide = (size32(x1 - b1, x2 + b2) >= m) & (size32(y1 - c1, y2 + c2) >= m)
    return keep_wide, keep_narrow == keep_wide


def small_box_keep_f64(boxes64, min_size):
    """The same size test on the fp64 boxes: the verdict for a planted box, which is never excluded -- its size is either
    exact (clamped to integer borders) or far from every ``min_size`` but 0, where fp64 keeps every box."""
    b = np.asarray(boxes64, dtype=np.float64)
    return ((b[..., 2] - b[..., 0] + 1) >= float(min_size)) & ((b[..., 3] - b[..., 1] + 1) >= float(min_size))


def smooth_l1_picked(box_regression, targets, positives, labels, column0, beta, denominator):
    """modeling/roi_heads/box_head/loss.py:147-170 with layers/smooth_l1_loss.py:11-16 (size_average=False) in fp64:
    over the positives, columns ``4 * labels[p] + c`` (or ``column0 + c``) of box_regression against targets[p, c];
    ``n < beta`` -> 0.5 n^2 / beta, else n - 0.5 beta; everything divided by ``denominator``.  ``beta`` is the float32 the
    kernel receives.  -> (loss, gradient fp64 [R, C], sum of the (non-negative) terms before the division)."""
    reg = np.asarray(box_regression)
    tgt = np.asarray(targets)
    assert reg.dtype == np.float32 and tgt.dtype == np.float32
    pos = np.asarray(positives, dtype=np.int64)
    beta = float(F32(beta))
    col0 = np.full(pos.shape, int(column0), dtype=np.int64) if labels is None else 4 * np.asarray(labels, dtype=np.int64)[pos]
    cols = col0[:, None] + np.arange(4)[None, :]
    d = reg[pos[:, None], cols].astype(np.float64) - tgt[pos].astype(np.float64)
    n = np.abs(d)
    quad = n < beta
    terms = np.where(quad, 0.5 * n * n / beta, n - 0.5 * beta)
    grad = np.zeros(reg.shape, dtype=np.float64)
    grad[pos[:, None], cols] = np.where(quad, d / beta, np.sign(d)) / float(denominator)
    total = float(terms.sum())
    return total / float(denominator), grad, total


def smooth_l1_loss_bound(num_pos, total):
    """Bound on |float32 loss - fp64 loss| * denominator: the additions on the longest chain of csrc/boxes.hip:94-113 --
    ceil(4P / 1024) per lane, 6 wave steps, 16 partials and 2 more -- each within 2^-24 of a partial sum <= the total."""
    return (math.ceil(4 * num_pos / 1024) + 24) * EPS * total


# ------------------------------------------------------------------ the shared edge inputs
STRIDE = 16
CELL_ANCHORS = np.array([[-8, -8, 23, 23], [-24, -8, 39, 23], [-8, -24, 23, 39]], dtype=np.float32)


def grid_anchors(h, w):
    """Every anchor of an h x w map, position-major ((y, x) row-major) then cell: integer coordinates."""
    return anchors_of(np.arange(h * w * CELL_ANCHORS.shape[0]), CELL_ANCHORS, w, STRIDE)


def inside(anchors, image_w, image_h):
    """anchor_generator.py:101-106 with straddle_thresh 0."""
    a = _f32(anchors)
    return (a[:, 0] >= 0) & (a[:, 1] >= 0) & (a[:, 2] < image_w) & (a[:, 3] < image_h)


T1_MAP = (9, 12)
T1_THRESHOLDS = (0.7, 0.3)
# coincides with an anchor | two-way tie at 0.6 | tiny, four-way tie at 1/64 | touched by no anchor | duplicate of the first
T1_GT = np.array([[40, 40, 71, 71], [48, 40, 79, 71], [100, 60, 103, 63], [500, 500, 520, 520], [40, 40, 71, 71]], dtype=np.float32)

T2_THRESHOLDS = (0.5, 0.25)
T2_ANCHORS = np.array([[0, 0, 9, 9], [100, 0, 109, 9], [200, 0, 209, 9]], dtype=np.float32)
T2_GT = np.array([[0, 0, 9, 4], [100, 0, 104, 4], [200, 0, 204, 3]], dtype=np.float32)   # IoU exactly 0.5, 0.25, 0.2
T2_IOU = (0.5, 0.25, 0.2)


def rpn_match_cases():
    """-> list of (name, gt, anchors, visible, high, low, allow_lq, weights): T1 (ties), T2 (thresholds), T3 (sizes)."""
    unit, box_w = (1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)
    cases = []
    h, w = T1_MAP
    anc = grid_anchors(h, w)
    vis = inside(anc, STRIDE * w, STRIDE * h)
    for name, gt, lq in (("T1-lq", T1_GT, True), ("T1-plain", T1_GT, False), ("T1-first3-lq", T1_GT[:3], True)):
        cases.append((name, gt, anc, vis, *T1_THRESHOLDS, lq, unit))
    # one anchor ([56, 40, 87, 71]) at IoU 0.6 with two DIFFERENT ground truths, and an untouched third: the labels cannot
    # tell which ground truth an anchor was restored to, the targets can (the first maximum wins)
    two = np.array([[48, 40, 79, 71], [64, 40, 95, 71], [500, 500, 520, 520]], dtype=np.float32)
    cases.append(("T1-two-gt-tie-lq", two, anc, vis, *T1_THRESHOLDS, True, unit))
    for lq in (True, False):
        cases.append((f"T2-lq{int(lq)}", T2_GT, T2_ANCHORS, np.ones(3, dtype=bool), *T2_THRESHOLDS, lq, unit))
    # T3: visibility is data to the kernel; every third anchor is invisible and still counts towards a ground truth's best
    rng = np.random.default_rng(20)
    big = grid_anchors(74, 75)                       # 16650 anchors: pass 1's 64-block stride loop takes a second trip
    for a_n, g_n, jitter, wts in ((1, 1, False, unit), (255, 1, True, box_w), (257, 40, False, box_w), (257, 40, True, unit),
                                  (16650, 1, False, unit), (16650, 40, True, box_w), (16650, 40, False, unit)):
        anc = big[:a_n] if a_n < 1000 else big
        span = anc[:, 2:].max(axis=0)
        xy = rng.integers(-8, np.maximum(span - 20, 1), size=(g_n, 2)).astype(np.float32)
        wh = rng.integers(6, 90, size=(g_n, 2)).astype(np.float32)
        gt = np.concatenate((xy, xy + wh), axis=1)
        if jitter:
            gt = (gt + rng.uniform(-0.5, 0.5, size=gt.shape)).astype(np.float32)
        if g_n > 1 or not jitter:
            gt[-1] = anc[-1]                         # the last anchor's own box: its best is found only in the last trip
        else:
            gt[-1] = anc[-1] + rng.uniform(-0.5, 0.5, size=4).astype(np.float32)   # a lone fractional box next to it
        vis = np.arange(a_n) % 3 != 1
        for lq in (True, False):
            cases.append((f"T3-A{a_n}-G{g_n}-{'frac' if jitter else 'int'}-lq{int(lq)}", gt, anc, vis, 0.7, 0.3, lq, wts))
    return cases


def match_encode_cases():
    """-> list of (name, gt, gt_labels, proposals, high, low, weights)."""
    rng = np.random.default_rng(21)
    box_w = (10.0, 10.0, 5.0, 5.0)
    cases = [("T2", T2_GT, np.array([7, 3, 5]), T2_ANCHORS, *T2_THRESHOLDS, box_w)]
    # two identical ground truths (index of the first) and proposals that overlap nothing (index 0, label 0)
    gt = np.array([[300, 300, 340, 350], [20, 20, 80, 90], [20, 20, 80, 90]], dtype=np.float32)
    props = np.array([[20, 20, 80, 90], [22, 18, 81, 88], [600, 600, 640, 640], [-50, -50, -10, -10], [300, 300, 340, 350]],
                     dtype=np.float32)
    cases.append(("dup-none", gt, np.array([4, 9, 11]), props, 0.5, 0.3, box_w))
    for g_n, p_n in ((1, 1), (1, 257), (3, 255), (300, 1), (300, 257)):
        xy = rng.integers(0, 400, size=(g_n, 2)).astype(np.float32)
        gt = np.concatenate((xy, xy + rng.integers(8, 120, size=(g_n, 2))), axis=1).astype(np.float32)
        src = gt[rng.integers(0, g_n, size=p_n)]
        props = (src + rng.normal(0, 6, size=(p_n, 4))).astype(np.float32)
        props[:, 2:] = np.maximum(props[:, 2:], props[:, :2] + 2)
        props[p_n // 2] = gt[-1]                     # one exact copy of a ground truth
        if p_n > 4:
            props[1] = [900, 900, 930, 930]          # overlaps nothing
        cases.append((f"G{g_n}-P{p_n}", gt, rng.integers(1, 49, size=g_n), props, 0.5, 0.3, box_w))
    return cases


DECODE_IMAGES_WH = np.array([[192, 144], [185, 134], [64, 48]], dtype=np.float32)   # the last is smaller than the grid
DECODE_MIN_SIZES = (0, 1, 16, 48, 64)  # 48 and 64: the sides of the smallest image, met with equality by a box clamped to it
XFORM_CLIP = math.log(1000.0 / 16)


def decode_case(weights, layout, k):
    """Input of the rpn_decode tests: 3 images on a 9 x 12 map with 3 anchors per cell, deltas ``randn * 0.5`` plus planted
    ones (below), the top-k list with the planted candidates in it (all 324 candidates, permuted, for k = 324).
    layout "nchw": a contiguous [N, 4A, H, W]; "nhwc_view": the NCHW view of channels [A, 5A) of an NHWC [N, H, W, 5A + 1].
    -> (box_regression view, topk_idx [N, k], image_wh [N, 2], planted [N, k]: planted case number or -1, base array the
    view lives in)."""
    n, a, h, w = 3, CELL_ANCHORS.shape[0], 9, 12
    rng = np.random.default_rng(22)
    d = (rng.standard_normal((n, h, w, a, 4)) * 0.5).astype(np.float32)
    clip = F32(XFORM_CLIP)
    plant = [((4, 6, 0), (0, 0, 10, 10)),                    # 0: beyond the clip, clamped to both borders: the image's size
             ((2, 3, 1), (0.25, -0.25, clip, 0)),            # 1: dw exactly xform_clip
             ((5, 2, 2), (0, 0, -20, -20)),                  # 2: a box that collapses onto the anchor's centre
             ((3, 5, 0), (50, 0, 0, 0)),                     # 3: the whole box onto the right border: width exactly 1
             ((6, 8, 0), (-50, -50, 0, 0)),                  # 4: ... onto the top-left corner: 1 x 1
             ((0, 0, 0), (0, 0, 10, 10)),                    # 5: beyond the clip at the corner anchor
             ((1, 1, 1), (0, 0, np.nextafter(clip, F32(0)), np.nextafter(clip, F32(9)))),   # 6: one ulp either side of the clip
             ((8, 11, 2), (0, 50, 0, 0))]                    # 7: onto the bottom border: height exactly 1
    ids = []
    for (y, x, c), delta in plant:
        d[:, y, x, c] = np.asarray(delta, dtype=np.float32)
        ids.append((y * w + x) * a + c)
    codes = (d * np.asarray(weights, dtype=np.float32)).astype(np.float32)               # [N, H, W, A, 4]
    if layout == "nchw":
        base = np.ascontiguousarray(codes.reshape(n, h, w, 4 * a).transpose(0, 3, 1, 2))
        reg = base
    else:
        base = rng.standard_normal((n, h, w, 5 * a + 1)).astype(np.float32)
        base[..., a:5 * a] = codes.reshape(n, h, w, 4 * a)
        reg = base[..., a:5 * a].transpose(0, 3, 1, 2)
    idx = np.empty((n, k), dtype=np.int64)
    planted = np.full((n, k), -1, dtype=np.int64)
    for i in range(n):
        rest = [j for j in rng.permutation(h * w * a) if j not in ids]
        order = np.array((ids + rest)[:k])
        number = np.array((list(range(len(ids))) + [-1] * len(rest))[:k])
        shuffle = rng.permutation(k)
        idx[i], planted[i] = order[shuffle], number[shuffle]
    return reg, idx, DECODE_IMAGES_WH.copy(), planted, base
