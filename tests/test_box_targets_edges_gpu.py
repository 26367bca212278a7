"""GPU: the RPN target and proposal kernels (csrc/targets.hip, rpn.hip, nms.hip, boxes.hip) against the NumPy restatement of
the reference (tests/box_target_reference.py, pinned by tests/test_box_target_reference.py) at the edges where a kernel
mislabels silently: exact IoU ties, IoUs exactly on a threshold, ground truths nothing touches, sizes around the block,
tile and stride-loop boundaries, deltas beyond the clip, boxes clamped to one pixel or to the whole image, sizes that meet
``min_size`` with equality.  Integer outputs (labels, indices, flags, kept lists, counts) are compared exactly -- the
decisions are IEEE float32 arithmetic the kernel has to reproduce bit for bit; values are bounded against fp64.

Largest measured error-to-bound ratios on an MI355X (printed by every test; run with ``-s``):
  rpn_match_encode targets   0.08   of 1e-6 * max(1, max|ref|)                  (T3-A16650-G40-frac-lq1)
  match_encode targets       0.07   of the same bound                           (G1-P257)
  rpn_decode boxes           0.14   of DECODE_ROUNDINGS * 2^-24 * magnitude     (every layout and weight set, K 257 / 324)
  smooth_l1_picked loss      0.08   of (ceil(4P / 1024) + 24) * 2^-24 * sum     (P 1, beta 1, class-agnostic)
DECODE_ROUNDINGS is 11: seven roundings plus expf's 2 ulp = 4 * 2^-24; read as 7 + 2 the decode ratio would be 0.17.
"""
import numpy as np
import pytest
import torch

from tests import box_target_reference as R

pytestmark = pytest.mark.gpu

UNIT, BOX_W = (1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)


def C(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _targets_ratio(got, ref):
    """The project's bound for encoded deltas (tests/test_targets_gpu.py:40): max error over 1e-6 * max(1, max|ref|)."""
    return float(np.abs(got.cpu().numpy().astype(np.float64) - ref).max()) / (1e-6 * max(1.0, float(np.abs(ref).max())))


# ------------------------------------------------------------------ rpn_match_encode
@pytest.mark.parametrize("case", R.rpn_match_cases(), ids=lambda c: c[0])
def test_rpn_match_encode_edges(case):
    """T1 exact ties (coinciding anchor, two-way tie between the thresholds, four-way tie below ``low``, a ground truth no
    anchor touches -- every anchor ties its best of 0 and is restored, the reference's quirk -- and a duplicate), T2 IoUs
    exactly on ``high`` / ``low``, T3 sizes 1 / 255 / 257 / 16650 (two trips of pass 1's stride loop; the last anchor's own
    box is a ground truth) x 1 / 40 ground truths, integer and fractional, a third of the anchors invisible."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    name, gt, anchors, visible, high, low, lq, weights = case
    want_lab, want_tgt = R.rpn_targets(gt, anchors, visible, high, low, lq, weights)
    lab, tgt = _C.rpn_match_encode(C(gt), C(anchors), C(visible), high, low, lq, weights)
    assert lab.dtype == torch.int64 and tgt.shape == (anchors.shape[0], 4)
    wrong = np.nonzero(lab.cpu().numpy() != want_lab)[0]
    assert wrong.size == 0, (wrong[:8], lab.cpu().numpy()[wrong[:8]], want_lab[wrong[:8]])
    ratio = _targets_ratio(tgt, want_tgt)
    print(f"rpn_match_encode {name}: labels -1/0/1 = {np.bincount(want_lab + 1, minlength=3).tolist()}, targets error / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_rpn_match_encode_t2_labels_by_hand():
    """IoU == high is a match, IoU == low is 'between' (ignored), 0.2 is background; with low-quality matches each is its
    ground truth's best and becomes positive."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    high, low = R.T2_THRESHOLDS
    vis = C(np.ones(3, dtype=bool))
    assert _C.rpn_match_encode(C(R.T2_GT), C(R.T2_ANCHORS), vis, high, low, False, UNIT)[0].tolist() == [1, -1, 0]
    assert _C.rpn_match_encode(C(R.T2_GT), C(R.T2_ANCHORS), vis, high, low, True, UNIT)[0].tolist() == [1, 1, 1]


# ------------------------------------------------------------------ match_encode
@pytest.mark.parametrize("case", R.match_encode_cases(), ids=lambda c: c[0])
def test_match_encode_edges(case):
    """G 1 / 3 / 300 x P 1 / 255 / 257, the T2 boxes as proposals, two identical ground truths, proposals that overlap
    nothing; both ``between_keeps_label`` modes; ``weights=None`` returns no targets."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    name, gt, gt_labels, props, high, low, weights = case
    for keep in (False, True):
        want_idx, want_lab, want_tgt = R.match_encode(gt, gt_labels, props, high, low, weights, keep)
        idx, lab, tgt = _C.match_encode(C(gt), C(gt_labels), C(props), high, low, weights, between_keeps_label=keep)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(lab.cpu().numpy(), want_lab)
        ratio = _targets_ratio(tgt, want_tgt)
        print(f"match_encode {name} keep={keep}: targets error / bound = {ratio:.3f}")
        assert ratio <= 1.0
    idx2, lab2, none = _C.match_encode(C(gt), C(gt_labels), C(props), high, low)
    assert none is None and np.array_equal(idx2.cpu().numpy(), want_idx)
    assert np.array_equal(lab2.cpu().numpy(), R.match_encode(gt, gt_labels, props, high, low, None, False)[1])


def test_match_encode_planted_by_hand():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    cases = {c[0]: c for c in R.match_encode_cases()}
    _, gt, labels, props, high, low, w = cases["T2"]
    idx, lab, _ = _C.match_encode(C(gt), C(labels), C(props), high, low, w)
    assert idx.tolist() == [0, 0, 0] and lab.tolist() == [7, -1, 0]           # == high matches; == low is between
    _, lab, _ = _C.match_encode(C(gt), C(labels), C(props), high, low, w, between_keeps_label=True)
    assert lab.tolist() == [7, 7, 0]                                          # mask head: the label of ground truth 0
    _, gt, labels, props, high, low, w = cases["dup-none"]
    idx, lab, tgt = _C.match_encode(C(gt), C(labels), C(props), high, low, w)
    assert idx.tolist() == [1, 1, 0, 0, 0] and lab.tolist() == [9, 9, 0, 0, 4]  # the first of two identical ground truths
    assert tgt[0].tolist() == [0.0, 0.0, 0.0, 0.0]
    want = R.encode(gt[[0, 0]], props[2:4], w)                                # overlap nothing: deltas against ground truth 0
    assert np.abs(tgt[2:4].cpu().numpy() - want).max() <= 1e-6 * np.abs(want).max()


# ------------------------------------------------------------------ rpn_decode
@pytest.mark.parametrize("k", [1, 257, 324])
@pytest.mark.parametrize("layout", ["nchw", "nhwc_view"])
@pytest.mark.parametrize("weights", [UNIT, BOX_W], ids=["w1", "w10-5"])
def test_rpn_decode_edges(weights, layout, k):
    """Three images -- (192, 144), (185, 134) and (64, 48), the last smaller than the 9 x 12 grid so that clipping decides
    most boxes -- both layouts and weight sets, K 1 / 257 / all 324 permuted, the planted deltas of
    box_target_reference.decode_case, min_size 0 / 1 / 16 and the two sides of the smallest image.  Boxes within the
    reference's per-element bound of fp64; the drop flag is the float32 size test on the kernel's own boxes and the
    reference's verdict wherever the bound leaves one."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    reg, idx, image_wh, planted, base = R.decode_case(weights, layout, k)
    a = R.CELL_ANCHORS.shape[0]
    reg_dev = C(base) if layout == "nchw" else C(base)[..., a:5 * a].permute(0, 3, 1, 2)
    assert reg_dev.shape == reg.shape and (layout == "nchw") == reg_dev.is_contiguous()
    want, bound = R.rpn_decode(reg, idx, R.CELL_ANCHORS, image_wh, weights, R.XFORM_CLIP, R.STRIDE)
    is_planted = planted >= 0
    worst = 0.0
    for min_size in R.DECODE_MIN_SIZES:
        boxes, drop = _C.rpn_decode(reg_dev, C(idx), C(R.CELL_ANCHORS), C(image_wh), weights, R.XFORM_CLIP, min_size, R.STRIDE)
        got = boxes.cpu().numpy()
        err = np.abs(got.astype(np.float64) - want)
        assert bool((err[bound == 0] == 0).all())                         # clamped well outside the image: the border itself
        ratio = float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0
        worst = max(worst, ratio)
        assert ratio <= 1.0, ratio
        flag = drop.cpu().numpy()
        assert set(np.unique(flag)) <= {0, -1}
        assert np.array_equal(flag == 0, R.small_box_keep_f32(got, min_size))
        keep, decided = R.small_box_verdict(want, bound, min_size)
        keep = np.where(is_planted, R.small_box_keep_f64(want, min_size), keep)   # a planted box is judged outright
        excluded = ~(decided | is_planted)
        assert np.array_equal((flag == 0)[~excluded], keep[~excluded])
        assert not (excluded & is_planted).any()                          # no planted case is excluded ...
        assert excluded.sum() <= 0.01 * max(1, (~is_planted).sum())       # ... and at most 1 % of the random ones
    for i in range(3):  # the planted boxes are what they claim
        w_img, h_img = image_wh[i]
        size = {int(p): (got[i, j, 2] - got[i, j, 0] + 1, got[i, j, 3] - got[i, j, 1] + 1) for j, p in enumerate(planted[i]) if p >= 0}
        if k > 1:
            assert size[0] == (w_img, h_img) and size[3][0] == 1 and size[4] == (1, 1) and size[7][1] == 1
        else:
            assert len(size) <= 1
    print(f"rpn_decode {layout} weights={weights} K={k}: boxes error / bound = {worst:.3f} (c = {R.DECODE_ROUNDINGS}), "
          f"exact borders {int((bound == 0).sum())} of {bound.size}")


# ------------------------------------------------------------------ nms_presorted_batched
def _random_boxes(rng, n, k, extent, side=120):
    xy = rng.uniform(0, 1, size=(n, k, 2)) * np.asarray(extent)
    wh = rng.uniform(0, 1, size=(n, k, 2)) * side + 4
    return np.concatenate((xy, xy + wh), axis=2).astype(np.float32)


def _check_nms(boxes, drop, thr, ge, below, reference=None):
    """Runs the kernel and compares every image with the greedy reference on the non-dropped boxes: the list, the zero fill
    behind it, both counts, and that the ``below`` survivors are a prefix.  -> per-image kept lists."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    n, k = boxes.shape[:2]
    keep, counts = _C.nms_presorted_batched(C(boxes), None if drop is None else C(drop), thr, below=below, ge_mode=ge)
    keep, counts = keep.cpu().numpy(), counts.cpu().numpy()
    assert keep.shape == (n, k) and counts.shape == (n, 2)
    out = []
    for i in range(n):
        want = reference[i] if reference is not None else R.greedy_nms_f32(boxes[i], None if drop is None else drop[i] >= 0, thr, ge)
        c, cb = int(counts[i, 0]), int(counts[i, 1])
        assert c == want.size, (i, c, want.size)
        assert np.array_equal(keep[i, :c], want)
        assert not keep[i, c:].any()
        assert cb == int((want < below).sum()) and bool((keep[i, :cb] < below).all()) and bool((keep[i, cb:c] >= below).all())
        out.append(want)
    return out


@pytest.mark.parametrize("k", [1, 63, 64, 65, 129])
def test_nms_presorted_batched_small_sizes(k):
    """K around the 64-box tile, four images with their own boxes: one with every candidate dropped (counts [0, 0], keep all
    zero), one with none dropped, two with a random third; ``below`` 0, 1, 64, 65, K and past K; ``drop=None``; both
    comparison modes."""
    rng = np.random.default_rng(100 + k)
    boxes = _random_boxes(rng, 4, k, (300.0, 200.0))
    drop = -(rng.uniform(size=(4, k)) < 0.33).astype(np.int32)
    drop[0] = -1
    drop[1] = 0
    refs = {ge: [R.greedy_nms_f32(boxes[i], drop[i] >= 0, 0.6, ge) for i in range(4)] for ge in (False, True)}
    assert refs[False][0].size == 0 and (k < 63 or 2 < refs[False][1].size < k)
    for below in (0, 1, 64, 65, k, k + 7):
        for ge in (False, True):
            _check_nms(boxes, drop, 0.6, ge, below, refs[ge])
    plain = _check_nms(boxes, None, 0.6, False, 0)
    assert all(p.size >= 1 for p in plain)


def test_nms_ge_mode_decides_exact_threshold_pairs():
    """Pairs with IoU exactly 0.5 at threshold 0.5 -- inside one 64-tile (ranks 12 and 40) and across tiles (ranks 10 and
    70) -- are kept by ``>`` and dropped by ``>=``; exact duplicates (ranks 5 / 100 and 80 / 90) are dropped by both."""
    k = 129
    boxes = np.stack([np.array([40 * i, 0, 40 * i + 9, 9], dtype=np.float32) for i in range(k)])
    boxes[70] = [400, 0, 409, 4]
    boxes[40] = [480, 0, 489, 4]
    boxes[100] = boxes[5]
    boxes[90] = boxes[80]
    assert R.iou_f32(boxes[[10]], boxes[[70]])[0, 0] == np.float32(0.5) == R.iou_f32(boxes[[12]], boxes[[40]])[0, 0]
    second = boxes[::-1].copy()                       # image 1: the same boxes in the opposite order (the half box first)
    both = np.stack([boxes, second])
    for drop in (None, np.zeros((2, k), dtype=np.int32)):
        gt_mode = _check_nms(both, drop, 0.5, False, 64)
        ge_mode = _check_nms(both, drop, 0.5, True, 64)
        assert sorted(set(range(k)) - set(gt_mode[0].tolist())) == [90, 100]
        assert sorted(set(range(k)) - set(ge_mode[0].tolist())) == [40, 70, 90, 100]
        assert sorted(set(range(k)) - set(ge_mode[1].tolist())) == sorted(k - 1 - r for r in (10, 12, 5, 80))
    # a dropped higher-ranked partner suppresses nothing
    drop = np.zeros((2, k), dtype=np.int32)
    drop[0, [10, 5]] = -1
    kept = _check_nms(both, drop, 0.5, True, 64)[0].tolist()
    assert 70 in kept and 100 in kept and 10 not in kept and 5 not in kept and 40 not in kept


def test_nms_presorted_batched_general_reduce_kernel():
    """K = 12289 is 193 tiles, one more than the pipelined reduce serves: the general reduce kernel with an image offset,
    drop flags and both counts."""
    rng = np.random.default_rng(7)
    n, k = 2, 12289
    boxes = _random_boxes(rng, n, k, (900.0, 600.0), 250)
    drop = -(rng.uniform(size=(n, k)) < 0.2).astype(np.int32)
    kept = _check_nms(boxes, drop, 0.6, False, 6000)
    assert all(300 < w.size < k // 2 for w in kept) and not np.array_equal(kept[0], kept[1])
    assert all(0 < (w < 6000).sum() < w.size for w in kept)


# ------------------------------------------------------------------ smooth_l1_picked
@pytest.mark.parametrize("per_class", [False, True], ids=["agnostic", "per-class"])
@pytest.mark.parametrize("beta", [1.0, 1.0 / 9], ids=["beta1", "beta1/9"])
@pytest.mark.parametrize("num_pos", [1, 256, 257, 700])
def test_smooth_l1_picked_edges(num_pos, beta, per_class):
    """1 / 256 / 257 / 700 positives (the 1024-lane loop takes one full trip at 256 and a partial second one above), both
    betas, class-agnostic (column0 4) and per-class columns including the last class, ``box_regression`` a column-slice
    view; planted d = +beta and -beta (linear branch, gradient +-1 / denominator) and d = 0 (gradient 0)."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    rng = np.random.default_rng(1000 + num_pos)
    rows, classes, denominator = 1024, (5 if per_class else 2), 700.0
    wide = (rng.standard_normal((rows, 4 * classes + 24)) * 0.6).astype(np.float32)
    tgt = (rng.standard_normal((rows, 4)) * 0.6).astype(np.float32)
    pos = np.sort(rng.permutation(rows)[:num_pos])
    labels = rng.integers(1, classes, size=rows)
    labels[pos[0]] = classes - 1                                           # the last class's columns
    reg = wide[:, 8:8 + 4 * classes]                                       # a view: row stride 4 * classes + 24
    col0 = 4 * labels[pos[0]] if per_class else 4
    b32 = np.float32(beta)
    p = pos[0]
    tgt[p, :3] = [0.0, 0.0, 0.375]
    reg[p, col0:col0 + 3] = [b32, -b32, 0.375]                             # d = +beta, -beta, 0
    want_loss, want_grad, total = R.smooth_l1_picked(reg, tgt, pos, labels if per_class else None, 4, beta, denominator)
    reg_dev = C(wide)[:, 8:8 + 4 * classes]
    assert not reg_dev.is_contiguous()
    args = (reg_dev, C(tgt), C(pos), C(labels) if per_class else None, 4, beta, denominator)
    loss, grad = _C.smooth_l1_picked_fwd_bwd(*args)
    bound = R.smooth_l1_loss_bound(num_pos, total) / denominator
    ratio = abs(float(loss) - want_loss) / bound
    print(f"smooth_l1_picked P={num_pos} beta={beta:.4f} per_class={per_class}: loss error / bound = {ratio:.3f}")
    assert ratio <= 1.0
    g = grad.cpu().numpy()
    assert g.shape == reg.shape
    assert np.allclose(g, want_grad, rtol=1e-6, atol=1e-9)
    assert g[p, col0] > 0 and g[p, col0 + 1] == -g[p, col0] and g[p, col0 + 2] == 0.0
    assert abs(g[p, col0] * denominator - 1.0) <= 1e-6                      # the linear branch's +-1 / denominator
    others = np.ones(rows, dtype=bool)
    others[pos] = False
    assert not g[others].any() and np.count_nonzero(g) <= 4 * num_pos
    loss2, none = _C.smooth_l1_picked_fwd_bwd(*args, need_grad=False)
    assert none is None and float(loss2) == float(loss)
