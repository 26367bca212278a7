"""CPU: tests/lvis_reference.py -- the restatement of LVIS-style federated scoring (rules 1 to 10 of include/ovis_hip.h) the
device code is compared with -- against hand-computed cases, each built so that ONE rule decides the number.

The arithmetic the literals rest on: a lone true positive has precision P1 = 1 / (1 + spacing(1)) at all 101 recall points;
"a false positive, then a true positive" has tp = [0, 1], fp = [1, 1], precision [0, 1 / 2] -> [1 / 2, 1 / 2] after the
envelope, so 1 / 2 at all 101 points (1 / (2 + spacing(1)) rounds to 1 / 2 exactly); a category with a ground truth and no
detection has 0 everywhere; a category without ground truth is -1 and does not enter a mean."""
import numpy as np
import pytest

from tests import lvis_reference as lref

P1 = 1 / (1 + np.spacing(1))
BOX = [0, 0, 10, 10]
FAR = [50, 50, 10, 10]


def _is(got, want):
    """Equal up to the rounding of a mean of at most 3 x 10 x 101 fp64 values in [0, 1]: 3030 x 2^-53 < 1e-12."""
    return abs(got - want) <= 1e-12


def _data(images, anns, frequencies=("f", "c", "r")):
    """Categories 1, 2, 3 with the given frequencies; ``images``: {id: (neg ids, not-exhaustive ids)}; ``anns``: [(image id,
    category id, xywh, extra keys)] in file order."""
    return {"categories": [{"id": k + 1, "name": f"c{k + 1}", "frequency": f} for k, f in enumerate(frequencies)],
            "images": [{"id": i, "neg_category_ids": list(neg), "not_exhaustive_category_ids": list(open_)}
                       for i, (neg, open_) in images.items()],
            "annotations": [dict({"image_id": i, "category_id": c, "bbox": box, "area": box[2] * box[3]}, **extra)
                            for i, c, box, extra in anns]}


def _det(image_id, category_id, score, box):
    return {"image_id": image_id, "category_id": category_id, "score": score, "bbox": box}


def test_a_detection_of_a_category_nobody_looked_for_is_dropped():
    anns = [(1, 1, BOX, {}), (2, 2, BOX, {})]
    dets = [_det(1, 1, .9, BOX), _det(2, 2, .5, BOX)]
    stray = _det(1, 2, .95, FAR)          # category 2 in image 1: neither a ground truth nor a negative
    data = _data({1: ([], []), 2: ([], [])}, anns)
    without, with_ = lref.evaluate(data, dets, "bbox"), lref.evaluate(data, dets + [stray], "bbox")
    assert with_ == without and _is(with_["AP"], P1) and _is(with_["AP50_class_c2"], P1)
    tables = lref.match_tables(data, dets + [stray], "bbox")
    assert tables["category"].tolist() == [0, 1] and tables["scores"].tolist() == [.9, .5]
    # the same detection counts once image 1 lists category 2 as verified absent: a false positive ahead of the true one
    negative = lref.evaluate(_data({1: ([2], []), 2: ([], [])}, anns), dets + [stray], "bbox")
    assert _is(negative["AP50_class_c2"], .5) and _is(negative["AP50_class_c1"], P1) and _is(negative["AP"], (P1 + .5) / 2)


def test_an_unmatched_detection_of_a_not_exhaustive_category_leaves_precision_untouched():
    anns = [(1, 1, BOX, {})]
    dets = [_det(1, 1, .9, FAR), _det(1, 1, .8, BOX)]   # unmatched, then the true positive
    exhaustive = lref.evaluate(_data({1: ([], [])}, anns), dets, "bbox")
    open_ = lref.evaluate(_data({1: ([], [1])}, anns), dets, "bbox")
    assert _is(exhaustive["AP"], .5) and _is(open_["AP"], P1)
    tables = lref.match_tables(_data({1: ([], [1])}, anns), dets, "bbox")
    assert tables["not_exhaustive"].tolist() == [True]
    assert tables["dt_match"][0, 0].tolist() == [-1, 0] and tables["dt_ignore"][0, 0].tolist() == [True, False]


def test_the_cap_of_300_acts_before_anything_else():
    anns = [(1, 1, BOX, {}), (1, 2, FAR, {})]
    dets = [_det(1, 1, .001, BOX)] + [_det(1, 2, .9 - k / 1000, [100, 100, 5, 5]) for k in range(300)]
    data = _data({1: ([], [])}, anns)
    capped = lref.evaluate(data, dets, "bbox")
    assert _is(capped["AP50_class_c1"], 0.0)                        # the 301st by score: its category keeps no detection
    assert lref.match_tables(data, dets, "bbox")["det_start"].tolist() == [0, 0, 300]   # no cap of 100 per category
    assert _is(lref.evaluate(data, dets, "bbox", max_dets=-1)["AP50_class_c1"], P1)
    assert _is(lref.evaluate(data, dets, "bbox", max_dets=301)["AP50_class_c1"], P1)
    assert _is(lref.evaluate(data, dets[:300], "bbox")["AP50_class_c1"], P1)             # 300 in all: nothing is cut


def test_a_matched_ignored_ground_truth_is_not_matched_again():
    anns = [(1, 1, BOX, {"ignore": 1}), (1, 1, [100, 100, 10, 10], {})]
    dets = [_det(1, 1, .9, BOX), _det(1, 1, .8, BOX), _det(1, 1, .7, [100, 100, 10, 10])]
    data = _data({1: ([], [])}, anns)
    tables = lref.match_tables(data, dets, "bbox")
    for t in range(10):
        assert tables["dt_match"][0, t].tolist() == [0, -1, 1] and tables["dt_ignore"][0, t].tolist() == [True, False, False]
    assert tables["gt_ignore"][0].tolist() == [True, False]
    # ignored, false positive, true positive -> 1 / 2.  Under COCO's crowd rule the second would be matched to the crowd
    # again and ignored too: P1
    assert _is(lref.evaluate(data, dets, "bbox")["AP"], .5)


def test_an_equal_iou_goes_to_the_later_ground_truth():
    anns = [(1, 1, BOX, {}), (1, 1, BOX, {}), (1, 1, FAR, {})]
    tables = lref.match_tables(_data({1: ([], [])}, anns), [_det(1, 1, .9, BOX), _det(1, 1, .8, BOX)], "bbox")
    assert tables["dt_match"][0, 0].tolist() == [1, 0]          # then the earlier one: the later is taken


def test_an_iou_equal_to_the_threshold_matches():
    anns = [(1, 1, BOX, {})]
    tables = lref.match_tables(_data({1: ([], [])}, anns), [_det(1, 1, .9, [0, 0, 10, 5])], "bbox")   # 50 / 100
    assert lref.box_iou([0, 0, 10, 5], BOX) == .5
    assert tables["dt_match"][0, :, 0].tolist() == [0] + [-1] * 9
    res = lref.evaluate(_data({1: ([], [])}, anns), [_det(1, 1, .9, [0, 0, 10, 5])], "bbox")
    assert _is(res["AP50"], P1) and _is(res["AP75"], 0.0) and _is(res["AP"], P1 / 10)


def test_apr_apc_apf_and_an_empty_frequency_group():
    anns = [(1, 1, BOX, {}), (1, 2, BOX, {}), (1, 3, BOX, {})]
    dets = [_det(1, 1, .9, BOX), _det(1, 2, .9, FAR), _det(1, 2, .8, BOX)]    # f: a hit; c: a miss, then a hit; r: nothing
    res = lref.evaluate(_data({1: ([], [])}, anns), dets, "bbox", {"seen": [0, 1], "unseen": [2]}, recall=True)
    assert _is(res["APf"], P1) and _is(res["APc"], .5) and _is(res["APr"], 0.0) and _is(res["AP"], (P1 + .5 + 0) / 3)
    assert list(res)[:9] == ["AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf"]
    assert _is(res["AP50_split_seen"], (P1 + .5) / 2) and _is(res["AP50_split_unseen"], 0.0)
    assert _is(res["APs"], res["AP"]) and _is(res["APm"], -1) and _is(res["APl"], -1)      # area 100: small
    assert _is(res["AR@300"], 2 / 3) and _is(res["ARs@300"], 2 / 3) and _is(res["ARm@300"], -1)
    assert _is(res["AR@300_split_seen"], 1.0) and _is(res["AR@300_split_unseen"], 0.0)
    none_rare = lref.evaluate(_data({1: ([], [])}, anns, ("f", "c", "c")), dets, "bbox")
    assert _is(none_rare["APr"], -1) and _is(none_rare["APc"], .25) and _is(none_rare["APf"], P1)


def test_equal_scores_across_images_keep_image_id_order():
    anns = [(5, 1, BOX, {}), (2, 1, BOX, {})]                   # the file lists image 5 first
    miss_first = lref.evaluate(_data({5: ([], []), 2: ([], [])}, anns), [_det(5, 1, .5, BOX), _det(2, 1, .5, FAR)], "bbox")
    hit_first = lref.evaluate(_data({5: ([], []), 2: ([], [])}, anns), [_det(5, 1, .5, FAR), _det(2, 1, .5, BOX)], "bbox")
    # image 2 comes first.  miss, hit: tp = [0, 1], fp = [1, 1], recall [0, 1 / 2], precision 1 / 2 up to recall 1 / 2 --
    # 51 of the 101 points.  hit, miss: precision P1 at the same 51 points
    assert _is(miss_first["AP"], 51 * .5 / 101) and _is(hit_first["AP"], 51 * P1 / 101)
    assert hit_first["AP"] > miss_first["AP"]


def test_missing_keys_raise_naming_the_item():
    data = _data({1: ([], []), 2: ([], [])}, [(1, 1, BOX, {})])
    del data["images"][1]["neg_category_ids"]
    with pytest.raises(ValueError, match="image 2"):
        lref.evaluate(data, [], "bbox")
    data = _data({1: ([], [])}, [(1, 1, BOX, {})])
    del data["categories"][2]["frequency"]
    with pytest.raises(ValueError, match="category 3"):
        lref.evaluate(data, [], "bbox")
