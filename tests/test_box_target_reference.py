"""CPU: pins tests/box_target_reference.py before any kernel is measured against it -- to the reference-made fixture
(tests/golden/heads.npz), to the package's host tensor-op forms on every edge input the GPU tests use
(tests/test_box_targets_edges_gpu.py), and to what the planted cases claim to be."""
import os

import numpy as np
import pytest
import torch

from tests import box_target_reference as R


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "heads.npz"))


def _close(got, want, rel=1e-6):
    """|got - want| <= rel * max(1, |want|), element-wise."""
    want = np.asarray(want, dtype=np.float64)
    return bool((np.abs(np.asarray(got, dtype=np.float64) - want) <= rel * np.maximum(1.0, np.abs(want))).all())


# ------------------------------------------------------------------ against the reference-made fixture
def test_rpn_targets_match_reference_fixture(z):
    """rpn/loss.py:56-89 as the reference ran it (tests/golden/make_golden.py): labels exact, targets to 1e-6."""
    from tests.test_components import _rpn_loss_case

    _, anchors, _, _, targets = _rpn_loss_case(z)
    for i in range(2):
        lab, tgt = R.rpn_targets(targets[i].bbox.numpy(), anchors[i].bbox.numpy(), anchors[i].get_field("visibility").numpy(),
                                 0.7, 0.3, True, (1.0, 1.0, 1.0, 1.0))
        assert np.array_equal(lab.astype(np.float32), z[f"rpnloss_labels{i}"])
        assert _close(tgt, z[f"rpnloss_targets{i}"])
        assert set(np.unique(lab)) == {-1, 0, 1}


def test_coder_and_matcher_match_reference_fixture(z):
    w = (10.0, 10.0, 5.0, 5.0)
    # coder_enc is float32 work on boxes at ~300 px: its own rounding (the centre difference cancels, then x 10 / width)
    # reaches 2.1e-6 of max(1, |value|) on 3 of the 120 elements -- the float32 tensor-op form reproduces the fixture bit
    # for bit, so that is the fixture's error, not the restatement's.  Bounded the way the project bounds encoded deltas
    # (tests/test_targets_gpu.py:40), by the largest value: measured 0.046 of the bound.
    enc = R.encode(z["coder_ref"], z["coder_prop"], w)
    assert float(np.abs(enc - z["coder_enc"]).max()) <= 1e-6 * max(1.0, float(np.abs(z["coder_enc"]).max()))
    assert _close(R.decode(z["coder_codes"], z["coder_prop"], w), z["coder_dec"])
    assert float(z["coder_codes"][0, 2]) / 5.0 > np.log(1000.0 / 16)  # the fixture does reach the clip
    iou = R.iou_f32(z["coder_ref"][:7], z["coder_prop"])
    assert _close(iou, z["iou"])  # the reference's fixture came from another machine's float32 division
    assert np.array_equal(R.matcher(z["iou"], 0.5, 0.5, False), z["match_plain"])
    assert np.array_equal(R.matcher(z["iou"], 0.7, 0.3, True), z["match_rpn"])
    # grid anchors in the (y, x, a) order against the reference's AnchorGenerator output
    h, w_ = 9, 12
    got = R.anchors_of(np.arange(h * w_ * 15), z["cell_anchors"], w_, 16)
    assert np.array_equal(got, z["anchors_img1"])
    assert np.array_equal(R.inside(got, w_ * 16 - 7, h * 16 - 10), z["anchors_vis1"])


def test_smooth_l1_matches_reference_fixture(z):
    a, b = z["sl1_a"], z["sl1_b"]
    pos = np.arange(a.shape[0])
    loss, _, total = R.smooth_l1_picked(a, b, pos, None, 0, 1.0, 1.0)
    assert loss == total and abs(loss - float(z["sl1_beta1_sum"])) <= 1e-6 * float(z["sl1_beta1_sum"])
    loss9, _, _ = R.smooth_l1_picked(a, b, pos, None, 0, 1.0 / 9, a.size)
    assert abs(loss9 - float(z["sl1_beta9_mean"])) <= 1e-6 * float(z["sl1_beta9_mean"])


# ------------------------------------------------------------------ against the package's host tensor-op forms
def _tensor_op_rpn_labels(gt, anchors, visible, high, low, lq, weights):
    """RPNLossComputation._call_tensor_ops' labels and regression targets, captured at the sampler."""
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.box_coder import BoxCoder
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.matcher import Matcher
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.rpn import RPNLossComputation
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList

    seen = []

    def sampler(labels):  # nothing sampled: the two losses are not what is looked at here
        seen.extend(labels)
        return [torch.zeros_like(l, dtype=torch.bool) for l in labels], [torch.zeros_like(l, dtype=torch.bool) for l in labels]

    loss = RPNLossComputation(Matcher(high, low, allow_low_quality_matches=lq), sampler, BoxCoder(weights))
    anc = BoxList(T(anchors), (4096, 4096))
    anc.add_field("visibility", T(visible))
    a = anchors.shape[0]
    loss._call_tensor_ops([anc], torch.zeros(1, 1, 1, a), torch.zeros(1, 4, 1, a), [BoxList(T(gt), (4096, 4096))])
    assert len(seen) == 1
    return seen[0].numpy()


@pytest.mark.parametrize("case", R.rpn_match_cases(), ids=lambda c: c[0])
def test_rpn_targets_equal_tensor_ops(case):
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.box_coder import BoxCoder
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.matcher import Matcher
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import box_iou

    _, gt, anchors, visible, high, low, lq, weights = case
    iou = R.iou_f32(gt, anchors)
    iou_t = box_iou(T(gt), T(anchors))
    assert np.array_equal(iou.view(np.int32), iou_t.numpy().view(np.int32))  # bit for bit
    matched = R.matcher(iou, high, low, lq)
    matched_t = Matcher(high, low, allow_low_quality_matches=lq)(iou_t)
    assert np.array_equal(matched, matched_t.numpy())
    lab, tgt = R.rpn_targets(gt, anchors, visible, high, low, lq, weights)
    assert np.array_equal(lab.astype(np.float32), _tensor_op_rpn_labels(gt, anchors, visible, high, low, lq, weights))
    tgt_t = BoxCoder(weights).encode(T(gt)[matched_t.clamp(min=0)], T(anchors)).numpy()
    assert float(np.abs(tgt_t - tgt).max()) <= 1e-6 * max(1.0, float(np.abs(tgt).max()))  # the project's bound for the deltas


@pytest.mark.parametrize("case", R.match_encode_cases(), ids=lambda c: c[0])
def test_match_encode_equals_tensor_ops(case):
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.box_coder import BoxCoder
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.matcher import Matcher
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import box_iou

    _, gt, gt_labels, props, high, low, weights = case
    matched = Matcher(high, low)(box_iou(T(gt), T(props)))
    idx_t = matched.clamp(min=0)
    for keep in (False, True):
        idx, lab, tgt = R.match_encode(gt, gt_labels, props, high, low, weights, keep)
        lab_t = T(gt_labels)[idx_t].clone()
        lab_t[matched == Matcher.BELOW_LOW_THRESHOLD] = 0
        if not keep:
            lab_t[matched == Matcher.BETWEEN_THRESHOLDS] = -1
        assert np.array_equal(idx, idx_t.numpy()) and np.array_equal(lab, lab_t.numpy())
        tgt_t = BoxCoder(weights).encode(T(gt)[idx_t], T(props)).numpy()
        assert float(np.abs(tgt_t - tgt).max()) <= 1e-6 * max(1.0, float(np.abs(tgt).max()))
    assert R.match_encode(gt, gt_labels, props, high, low, None, False)[2] is None


@pytest.mark.parametrize("weights", [(1.0, 1.0, 1.0, 1.0), (10.0, 10.0, 5.0, 5.0)])
def test_rpn_decode_equals_tensor_ops(weights):
    """The gather order, the anchors, the decode and the clip against permute_and_flatten + _decode_tensor_ops + clamp on
    the edge input of the GPU test, for a contiguous NCHW tensor and the NCHW view of an NHWC one."""
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.box_coder import BoxCoder
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.rpn import permute_and_flatten

    for layout in ("nchw", "nhwc_view"):
        reg, idx, image_wh, planted, _ = R.decode_case(weights, layout, 324)
        n, c4, h, w = reg.shape
        ref, bound = R.rpn_decode(reg, idx, R.CELL_ANCHORS, image_wh, weights, R.XFORM_CLIP, R.STRIDE)
        anchors = T(R.grid_anchors(h, w))
        flat = permute_and_flatten(T(reg), n, c4 // 4, 4, h, w)
        for i in range(n):
            sel = T(idx[i])
            got = BoxCoder(weights)._decode_tensor_ops(flat[i][sel], anchors[sel])
            got[:, 0::2].clamp_(min=0, max=float(image_wh[i, 0]) - 1)
            got[:, 1::2].clamp_(min=0, max=float(image_wh[i, 1]) - 1)
            err = np.abs(got.numpy().astype(np.float64) - ref[i])
            assert bool((err <= bound[i]).all()), float((err / np.maximum(bound[i], 1e-300)).max())
            for min_size in R.DECODE_MIN_SIZES:
                keep, decided = R.small_box_verdict(ref[i], bound[i], min_size)
                flag = R.small_box_keep_f32(got.numpy(), min_size)
                assert np.array_equal(flag[decided], keep[decided])
                mine = planted[i] >= 0                                    # planted boxes: the fp64 verdict, never excluded
                assert np.array_equal(flag[mine], R.small_box_keep_f64(ref[i], min_size)[mine])
                assert (~decided[~mine]).sum() <= 0.01 * (~mine).sum()


# ------------------------------------------------------------------ the planted cases are what they claim
def test_t1_ties_are_what_they_claim():
    h, w = R.T1_MAP
    anchors = R.grid_anchors(h, w)
    assert anchors.shape == (324, 4) and np.array_equal(anchors, np.rint(anchors))
    visible = R.inside(anchors, R.STRIDE * w, R.STRIDE * h)
    iou = R.iou_f32(R.T1_GT, anchors)
    ties, best = R.ties_per_gt(iou)
    assert ties.tolist() == [1, 2, 4, 324, 1]
    assert best.tolist() == [1.0, float(np.float32(0.6)), 1.0 / 64, 0.0, 1.0]
    assert int((anchors == R.T1_GT[0]).all(axis=1).sum()) == 1           # coincides with one anchor
    assert 0.3 < best[1] < 0.7 and best[2] < 0.3                          # between the thresholds; far below low
    high, low = R.T1_THRESHOLDS

    def counts(gt, lq):
        lab, _ = R.rpn_targets(gt, anchors, visible, high, low, lq, (1.0, 1.0, 1.0, 1.0))
        return [int((lab == v).sum()) for v in (1, -1, 0)]

    assert counts(R.T1_GT, True) == [176, 148, 0]     # the untouched ground truth restores EVERY anchor to its argmax
    assert counts(R.T1_GT, False) == [1, 162, 161]
    assert counts(R.T1_GT[:3], True) == [6, 161, 157]
    # the duplicate never wins: the first index does
    m = R.matcher(iou, high, low, True)
    assert 0 in m and 4 not in m
    # of the two anchors of the 0.6 tie one is ground truth 0's own anchor; the other is between the thresholds and is
    # restored to ground truth 1 only by the low-quality rule
    tie = np.nonzero(iou[1] == best[1])[0]
    assert R.matcher(iou, high, low, False)[tie].tolist() == [0, R.BETWEEN_THRESHOLDS] and m[tie].tolist() == [0, 1]


def test_t2_ious_sit_exactly_on_the_thresholds():
    iou = R.iou_f32(R.T2_GT, R.T2_ANCHORS)
    assert iou.diagonal().tolist() == [float(np.float32(v)) for v in R.T2_IOU]
    assert float((iou - np.diag(iou.diagonal())).max()) == 0.0           # far-apart clusters
    high, low = R.T2_THRESHOLDS
    assert iou[0, 0] == np.float32(high) and iou[1, 1] == np.float32(low) and iou[2, 2] < np.float32(low)
    assert R.matcher(iou, high, low, False).tolist() == [0, R.BETWEEN_THRESHOLDS, R.BELOW_LOW_THRESHOLD]
    assert R.matcher(iou, high, low, True).tolist() == [0, 1, 2]


def test_t3_reaches_the_second_trip_and_hides_a_third():
    big = [c for c in R.rpn_match_cases() if c[0].startswith("T3-A16650")]
    assert len(big) == 6
    for _, gt, anchors, visible, *_ in big:
        assert anchors.shape[0] == 16650 > 64 * 256                       # 64 blocks of 256 lanes walk it in two trips
        assert np.array_equal(gt[-1], anchors[-1])
        iou = R.iou_f32(gt[-1:], anchors)[0]
        assert iou[-1] == 1.0 and float(iou[: 64 * 256].max()) < 1.0      # the best lies in the second trip only
        assert 0.3 < 1.0 - visible.mean() < 0.36
    assert {c[1].shape[0] for c in R.rpn_match_cases() if c[0].startswith("T3")} == {1, 40}
    assert {c[2].shape[0] for c in R.rpn_match_cases() if c[0].startswith("T3")} == {1, 255, 257, 16650}


def test_greedy_nms_on_hand_cases():
    a, b = [0, 0, 9, 9], [0, 0, 9, 4]                                      # IoU exactly 0.5
    far = [100, 100, 120, 120]
    boxes = np.array([a, b, far, a], dtype=np.float32)
    assert R.iou_f32(boxes[:1], boxes[1:2])[0, 0] == np.float32(0.5)
    assert R.greedy_nms_f32(boxes, None, 0.5).tolist() == [0, 1, 2]       # '>' keeps the 0.5 pair, drops the duplicate
    assert R.greedy_nms_f32(boxes, None, 0.5, ge=True).tolist() == [0, 2]
    assert R.greedy_nms_f32(boxes, np.array([False, True, True, True]), 0.5, ge=True).tolist() == [1, 2]  # b kills the later a
    assert R.greedy_nms_f32(boxes, np.zeros(4, dtype=bool), 0.5).size == 0
    assert R.greedy_nms_f32(boxes[:1], None, 0.5).tolist() == [0]


def test_greedy_nms_equals_the_oracle(oracle_mod):
    g = torch.Generator().manual_seed(9)
    k = 400
    xy = torch.rand(k, 2, generator=g) * torch.tensor([300.0, 200.0])
    boxes = torch.cat([xy, xy + torch.rand(k, 2, generator=g) * 120 + 4], 1)
    scores = torch.sort(torch.rand(k, generator=g), descending=True).values
    want = oracle_mod.nms(boxes, scores, 0.6)
    got = R.greedy_nms_f32(boxes.numpy(), None, 0.6)
    assert 20 < got.size < k and np.array_equal(got, want.numpy())
