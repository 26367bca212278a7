"""GPU: COCO AR end to end on the tiny dataset (tests/tiny_coco.py).  ``evaluate_coco(..., recall=True)`` appends the AR keys
behind unchanged AP keys and equals the scalar restatement (tests/coco_recall_reference.py) of the restated matching
(tests/coco_eval_reference.py) within 1e-9 -- fp64 means of at most 10 x 4 values <= 1; ``tools/score_results.py --recall``
gives the same numbers for the same detections written as a results file."""
import json

import pytest

from tests import coco_eval_reference as ref
from tests import coco_recall_reference as rec
from tests.test_coco_eval_gpu import SCALE, TINY_DETECTIONS, _restatement_images, _tiny, _tool

pytestmark = pytest.mark.gpu

DEV = "cuda"
AR_KEYS = ["AR1", "AR10", "AR100", "ARs", "ARm", "ARl", "AR100_split_seen", "AR100_split_unseen"]


def test_evaluate_coco_recall_equals_the_restatement_and_score_results_agrees(tmp_path_factory, tmp_path):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval

    dataset, predictions = _tiny(tmp_path_factory)
    plain = coco_eval.evaluate_coco(dataset, predictions, ("bbox", "segm"), DEV)
    got = coco_eval.evaluate_coco(dataset, predictions, ("bbox", "segm"), DEV, recall=True)
    for iou_type in ("bbox", "segm"):   # the default output is untouched, the AR keys follow it
        assert list(got[iou_type]) == list(plain[iou_type]) + AR_KEYS and not [k for k in plain[iou_type] if k.startswith("AR")]
        assert all(got[iou_type][k] == v for k, v in plain[iou_type].items())
    cat_ids = sorted(dataset.coco.cats)
    names = [dataset.categories[c] for c in cat_ids]
    splits = {s: [cat_ids.index(c) for c in ids] for s, ids in dataset.class_splits.items()}
    tables = ref.match_tables(_restatement_images(dataset, predictions), "bbox")
    want = rec.summarize_recall(rec.accumulate_recall(tables, len(names)), names, splits)
    assert list(want) == AR_KEYS
    for k in AR_KEYS:
        assert abs(got["bbox"][k] - want[k]) <= 1e-9, (k, got["bbox"][k], want[k])
    assert 0 < want["AR1"] <= want["AR10"] <= want["AR100"] < 1 and want["AR100_split_unseen"] > 0   # not degenerate
    assert all(v == -1 or 0 <= v <= 1 for v in got["segm"].values()) and got["segm"]["AR100"] > 0

    # the same detections as a bbox results file, scored by the tool
    entries = [{"image_id": image_id, "category_id": c, "score": s, "bbox": [b[0], b[1], b[2] - b[0] + 1, b[3] - b[1] + 1]}
               for image_id, dets in TINY_DETECTIONS.items() for c, s, b in dets]
    assert SCALE == 2   # the predictions are these boxes doubled in a doubled frame: resized back they are these numbers
    with open(tmp_path / "bbox.json", "w") as f:
        json.dump(entries, f)
    tool = _tool("score_results")
    ann_file = dataset.coco.ann_file
    without = tool.main(["--ann-file", ann_file, "--bbox", str(tmp_path / "bbox.json")])
    scored = tool.main(["--ann-file", ann_file, "--bbox", str(tmp_path / "bbox.json"), "--recall", "--output", str(tmp_path / "s.json")])
    assert list(scored) == ["bbox"] and list(scored["bbox"]) == list(without["bbox"]) + AR_KEYS
    assert not [k for k in without["bbox"] if k.startswith("AR")]
    for k in AR_KEYS:
        assert abs(scored["bbox"][k] - want[k]) <= 1e-9, k
    with open(tmp_path / "s.json") as f:
        assert json.load(f) == json.loads(json.dumps(scored))
