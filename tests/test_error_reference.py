"""CPU: tests/error_reference.py -- the plain-Python restatement of the error analysis of include/ovis_hip.h -- held to cases
computed by hand, and its base AP50 to tests/coco_eval_reference.py's on the same input.  The fractions are those of the
precision samples; a precision of "1" is 1 / (1 + spacing(1)), so they hold to 1e-12, not to the bit."""
from fractions import Fraction as F

import numpy as np
import pytest

from tests import coco_eval_reference as cref
from tests import error_reference as eref

A, B, C = 0, 1, 2
SPLITS = {"seen": [A], "unseen": [B]}


def det(cat, box, score):
    return {"category": cat, "bbox": box, "score": score}


def gt(cat, box, crowd=0):
    return {"category": cat, "bbox": box, "area": box[2] * box[3], "iscrowd": crowd}


def table_case():
    """The issue's first case: one 100 x 100 image, categories A and B."""
    g_a1, g_b1, g_a2 = [10, 10, 40, 40], [60, 60, 30, 30], [10, 60, 20, 20]
    return [{"gts": [gt(A, g_a1), gt(B, g_b1), gt(A, g_a2)],
             "dets": [det(A, g_a1, .9), det(A, g_a1, .8), det(A, g_b1, .7), det(B, [60, 60, 30, 10], .6), det(B, [0, 0, 5, 5], .5),
                      det(B, [10, 10, 40, 12], .4)]}]


def close(got, want):
    return got == pytest.approx(float(want), abs=1e-12)


def test_the_table_case_types_targets_and_missed():
    r = eref.rows(table_case(), "bbox")
    # rows: category A first (gA1, gA2 | the three A detections), then B (gB1 | the three B detections)
    assert r["gt_cat"] == [A, A, B] and r["det_cat"] == [A, A, A, B, B, B] and r["det_score"] == [.9, .8, .7, .6, .5, .4]
    assert r["det_match"] == [0, -1, -1, -1, -1, -1] and r["det_ignore"] == [False] * 6
    assert [eref.TYPES[t] for t in r["err_type"]] == ["none", "Dupe", "Cls", "Loc", "Bkg", "Both"]
    assert r["err_gt"] == [-1, 0, 2, 2, -1, -1]
    assert r["gt_missed"] == [False, True, False]      # gA1 is matched, gA2 is Miss, gB1 is a target
    assert eref.box_iou([60, 60, 30, 10], [60, 60, 30, 30]) == 300 / 900 and eref.box_iou([10, 10, 40, 12], [10, 10, 40, 40]) == 0.3


def test_the_table_case_daps_are_the_fractions_written_out():
    res = eref.analyze(table_case(), "bbox", 2, SPLITS)
    # base: A = [tp, fp, fp] over 2 ground truths -> precision 1 up to recall .5: 51 / 101; B = [fp, fp, fp] -> 0
    assert close(res["AP50"], F(51, 202)) and close(res["AP50_split_seen"], F(51, 101)) and res["AP50_split_unseen"] == 0.0
    assert close(res["dAP50_Cls"], F(1, 2))        # .7 moves to B and takes gB1: B = [tp, fp, fp, fp] -> 1
    assert close(res["dAP50_Loc"], F(1, 2))        # .6 takes gB1: B -> 1
    assert res["dAP50_Dupe"] == 0.0 and res["dAP50_Bkg"] == 0.0 and res["dAP50_Both"] == 0.0   # behind the only tp / all fp
    assert close(res["dAP50_Miss"], F(25, 101))    # without gA2 A = 1: (1 - 51 / 101) / 2
    assert res["dAP50_FalsePos"] == 0.0
    assert close(res["dAP50_FalseNeg"], F(151, 202))   # gA2 and gB1 leave: B drops out, A = 1
    assert close(res["dAP50_Cls_split_unseen"], 1) and res["dAP50_Cls_split_seen"] == 0.0
    assert close(res["dAP50_Miss_split_seen"], F(50, 101)) and res["dAP50_Miss_split_unseen"] == 0.0
    assert res["counts"]["all"] == {"Cls": 1, "Loc": 1, "Both": 1, "Dupe": 1, "Bkg": 1, "Miss": 1}
    assert res["counts"]["seen"] == {"Cls": 1, "Loc": 0, "Both": 0, "Dupe": 1, "Bkg": 0, "Miss": 1}
    assert res["counts"]["unseen"] == {"Cls": 0, "Loc": 1, "Both": 1, "Dupe": 0, "Bkg": 1, "Miss": 0}
    assert res["cls_confusion_by_split"] == {"seen": {"seen": 0, "unseen": 0}, "unseen": {"seen": 1, "unseen": 0}}


def test_two_fixed_detections_claim_one_target():
    """Both Loc errors aim at g1; .9 takes it and .8 is DELETED -- kept as a false positive it would sit between the two
    true positives and cost precision."""
    g1, g2 = [0, 0, 10, 10], [50, 50, 10, 10]
    images = [{"gts": [gt(A, g1), gt(A, g2)], "dets": [det(A, [0, 0, 10, 30], .9), det(A, [0, 0, 10, 25], .8), det(A, g2, .7)]}]
    r = eref.rows(images, "bbox")
    assert [eref.TYPES[t] for t in r["err_type"]] == ["Loc", "Loc", "none"] and r["err_gt"] == [0, 0, -1]
    res = eref.analyze(images, "bbox", 1, {})
    assert close(res["AP50"], F(17, 101))          # [fp, fp, tp] over 2: precision 1 / 3 up to recall .5
    assert close(res["dAP50_Loc"], 1 - F(17, 101))  # [tp, tp]: 1.  With .8 kept: (51 + 50 * 2 / 3) / 101
    # equal scores: the earlier row claims
    images[0]["dets"][1]["score"] = .9
    assert close(eref.analyze(images, "bbox", 1, {})["dAP50_Loc"], 1 - F(17, 101))


def test_a_loc_target_the_base_already_matched_deletes_the_detection():
    g = [0, 0, 10, 10]
    images = [{"gts": [gt(A, g)], "dets": [det(A, [0, 0, 10, 30], .95), det(A, g, .9)]}]
    r = eref.rows(images, "bbox")
    assert [eref.TYPES[t] for t in r["err_type"]] == ["Loc", "none"] and r["err_gt"] == [0, -1] and r["gt_missed"] == [False]
    res = eref.analyze(images, "bbox", 1, {})
    assert close(res["AP50"], F(1, 2)) and close(res["dAP50_Loc"], F(1, 2))   # [fp, tp] -> [tp]


def test_a_crowd_is_no_error_and_never_missed():
    crowd, g = [0, 0, 50, 50], [60, 60, 20, 20]
    images = [{"gts": [gt(A, crowd, 1), gt(B, g)],
               "dets": [det(A, [0, 0, 10, 10], .9), det(A, [5, 5, 10, 10], .8), det(B, g, .7), det(B, [0, 0, 50, 50], .6)]}]
    r = eref.rows(images, "bbox")
    assert r["det_match"] == [0, 0, 1, -1] and r["det_ignore"] == [True, True, False, False]   # a crowd is matched again
    # the B detection on the crowd: the crowd takes no part, so "other" is empty -> Bkg, not Cls
    assert [eref.TYPES[t] for t in r["err_type"]] == ["none", "none", "none", "Bkg"] and r["gt_missed"] == [False, False]
    res = eref.analyze(images, "bbox", 2, SPLITS)
    assert close(res["AP50"], 1) and res["AP50_split_seen"] == -1.0 and res["dAP50_Miss_split_seen"] == -1.0
    assert res["counts"]["all"] == {"Cls": 0, "Loc": 0, "Both": 0, "Dupe": 0, "Bkg": 1, "Miss": 0}


def test_a_fix_that_empties_a_category():
    g = [0, 0, 10, 10]
    images = [{"gts": [gt(A, g), gt(B, [50, 50, 10, 10])], "dets": [det(A, g, .9)]}]
    res = eref.analyze(images, "bbox", 2, SPLITS)
    assert close(res["AP50"], F(1, 2)) and close(res["dAP50_Miss"], F(1, 2)) and close(res["dAP50_FalseNeg"], F(1, 2))
    assert res["AP50_split_unseen"] == 0.0 and res["dAP50_Miss_split_unseen"] == -1.0   # no category remains in the split
    assert res["counts"]["unseen"]["Miss"] == 1


def test_without_ground_truth_every_dap_is_minus_one():
    images = [{"gts": [], "dets": [det(A, [0, 0, 10, 10], .9)]}, {"gts": [], "dets": []}]
    res = eref.analyze(images, "bbox", 2, SPLITS)
    assert res["AP50"] == -1.0 and all(v == -1.0 for k, v in res.items() if k.startswith("dAP50_"))
    assert res["counts"]["all"]["Bkg"] == 1 and res["counts"]["all"]["Miss"] == 0


def test_thresholds_exactly_met():
    """IoU exactly t_f: Dupe as "same" (never Loc), Cls as "other".  IoU exactly t_b: Loc as "same", Bkg as "other"."""
    half, tenth = [0, 0, 10, 20], [0, 0, 10, 100]
    assert eref.box_iou([0, 0, 10, 10], half) == 0.5 and eref.box_iou([0, 0, 10, 10], tenth) == 0.1

    def kinds(gts, dets, match):
        ious = [[eref.box_iou(d["bbox"], g["bbox"]) for g in gts] for d in dets]
        t, targets, _ = eref.classify(ious, [d["category"] for d in dets], match, [False] * len(dets), [g["category"] for g in gts],
                                      [g["iscrowd"] for g in gts])
        return [eref.TYPES[k] for k in t], targets
    d = det(A, [0, 0, 10, 10], .5)
    assert kinds([gt(A, half)], [d], [-1]) == (["Dupe"], [0])
    assert kinds([gt(B, half)], [d], [-1]) == (["Cls"], [0])
    assert kinds([gt(A, tenth)], [d], [-1]) == (["Loc"], [0])
    assert kinds([gt(B, tenth)], [d], [-1]) == (["Bkg"], [-1])
    assert kinds([gt(B, half), gt(B, half)], [d], [-1]) == (["Cls"], [1])   # an equal IoU goes to the later row


def _random_images(seed, crowds):
    rs = np.random.RandomState(seed)
    images = []
    for _ in range(5):
        gts = [gt(int(rs.randint(3)), [float(v) for v in np.r_[rs.randint(0, 60, 2), rs.randint(8, 40, 2)]],
                  int(crowds and rs.rand() < .2)) for _ in range(rs.randint(0, 7))]
        dets = []
        for _ in range(rs.randint(0, 12)):
            if gts and rs.rand() < .7:   # near a ground truth, of its class or not
                g = gts[rs.randint(len(gts))]
                box = [g["bbox"][0] + float(rs.randint(-6, 7)), g["bbox"][1] + float(rs.randint(-6, 7)),
                       max(1.0, g["bbox"][2] + float(rs.randint(-8, 9))), max(1.0, g["bbox"][3] + float(rs.randint(-8, 9)))]
                cat = g["category"] if rs.rand() < .7 else int(rs.randint(3))
            else:
                box, cat = [float(v) for v in np.r_[rs.randint(0, 60, 2), rs.randint(8, 40, 2)]], int(rs.randint(3))
            dets.append(det(cat, box, float(rs.choice([.9, .8, .7, .6, .5, .4, .3]))))
        images.append({"gts": gts, "dets": dets})
    return images


@pytest.mark.parametrize("crowds", [False, True])
def test_base_ap50_is_the_coco_restatements(crowds):
    images = _random_images(11, crowds)
    splits = {"seen": [A, C], "unseen": [B]}
    res = eref.analyze(images, "bbox", 3, splits)
    want = cref.evaluate(images, "bbox", ["a", "b", "c"], splits)
    assert res["AP50"] == want["AP50"] and 0 < res["AP50"] < 1
    for split in splits:
        assert res[f"AP50_split_{split}"] == want[f"AP50_split_{split}"]
    assert sum(res["counts"]["all"].values()) > 5
    # deleting every false positive or every unmatched ground truth never lowers AP50
    assert res["dAP50_FalsePos"] >= 0 and res["dAP50_FalseNeg"] >= 0
