"""GPU: the error analysis end to end (engine/error_analysis.py, csrc/error_types.hip) on the seven-image dataset of
tests/tiny_coco.py -- four categories in a seen and an unseen split, a crowd, an RLE ground truth, five image sizes -- with
detections planted to make every error type, against the plain-Python restatement tests/error_reference.py: key by key and
exactly, since both make every precision sample by the same arithmetic from the same match tables."""
import json
import logging
import os

import numpy as np
import pytest
import torch

from tests import error_reference as eref
from tests import tiny_coco
from tests.test_coco_eval_gpu import _host_masks, _restatement_images

pytestmark = pytest.mark.gpu

DEV = "cuda"
M = 14
SCALE = 2   # the predictions live at twice the file's image sizes
TYPES = ("bbox", "segm")
DETECTIONS = {   # image id -> [(json category id, score, xyxy at the FILE's scale)]; categories 17, 3, 8 are seen, 44 unseen
    7: [(8, .9, [10, 10, 39, 29]), (8, .8, [11, 10, 39, 29]), (17, .7, [10, 10, 39, 29]), (44, .75, [10, 11, 39, 29]),
        (8, .6, [10, 10, 39, 16]), (3, .5, [50, 40, 60, 46]), (17, .3, [45, 2, 60, 9])],
    12: [(8, .85, [2, 3, 11, 6]), (3, .6, [2, 3, 11, 12])],
    20: [(3, .9, [5, 5, 30, 40])],
    55: [(44, .85, [40, 35, 59, 64]), (17, .4, [38, 30, 49, 49])],
    90: [(44, .95, [1, 1, 50, 30]), (44, .5, [1, 1, 50, 30]), (8, .3, [1, 1, 50, 30]), (44, .5, [2, 1, 50, 12])],
    101: [(17, .9, [30, 10, 42, 29]), (3, .8, [5, 6, 24, 20]), (3, .85, [30, 20, 50, 35]), (8, .2, [31, 11, 41, 28])],
}   # image 31 gets an empty prediction: its only ground truth is Miss


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCODataset
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList
    folder = tmp_path_factory.mktemp("error_analysis")
    paths = tiny_coco.write(folder / "data")
    dataset = COCODataset(paths["instances"], paths["img_dir"], False, {"LOAD_EMBEDDINGS": True, "EMB_KEY": "Tiny", "EMB_DIM": 4})
    assert dataset.class_splits == {"seen": [17, 3, 8], "unseen": [44]}
    g = torch.Generator().manual_seed(3)
    predictions = []
    for image_id in dataset.ids:
        info = dataset.coco.imgs[image_id]
        dets = DETECTIONS.get(image_id, [])
        pred = BoxList(torch.tensor([d[2] for d in dets], dtype=torch.float32).reshape(-1, 4) * SCALE,
                       (info["width"] * SCALE, info["height"] * SCALE))
        pred.add_field("scores", torch.tensor([d[1] for d in dets], dtype=torch.float32))
        pred.add_field("labels", torch.tensor([dataset.json_category_id_to_contiguous_id[d[0]] for d in dets], dtype=torch.int64))
        pred.add_field("mask", 0.6 + 0.4 * torch.rand(len(dets), 1, M, M, generator=g))   # nearly the whole box
        predictions.append(pred)
    masks = _host_masks(dataset, predictions)
    below, above = _host_masks(dataset, predictions, 0.5 - 2e-6)[0], _host_masks(dataset, predictions, 0.5 + 2e-6)[0]
    for image_id in below:   # no host-pasted pixel within 2e-6 of the threshold: the device paste gives the same masks
        for lo, hi in zip(below[image_id], above[image_id]):
            assert np.array_equal(lo, hi), image_id
    cat_ids = sorted(dataset.coco.cats)
    splits = {s: [cat_ids.index(c) for c in ids] for s, ids in dataset.class_splits.items()}
    want = {t: eref.analyze(_restatement_images(dataset, predictions, masks if t == "segm" else None), t, len(cat_ids), splits)
            for t in TYPES}
    return {"dataset": dataset, "predictions": predictions, "want": want, "folder": folder, "paths": paths}


def _same(got, want, where):
    assert list(got) == list(want), where
    for key in want:
        assert got[key] == want[key], (where, key, got[key], want[key])


def test_analyze_errors_equals_the_restatement(case):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval, error_analysis
    dataset, predictions, want = case["dataset"], case["predictions"], case["want"]
    got = error_analysis.analyze_errors(dataset, predictions, TYPES, DEV)
    assert list(got) == list(TYPES)
    for t in TYPES:
        _same(got[t], want[t], t)
    keys = ["AP50", "AP50_split_seen", "AP50_split_unseen"]
    for name in ("Cls", "Loc", "Both", "Dupe", "Bkg", "Miss"):
        keys += [f"dAP50_{name}", f"dAP50_{name}_split_seen", f"dAP50_{name}_split_unseen"]
    assert list(got["bbox"]) == keys + ["dAP50_FalsePos", "dAP50_FalseNeg", "counts", "cls_confusion_by_split"]
    # the case is what it claims to be: every type occurs, fixes gain, an unseen object was called seen and the reverse
    bbox = got["bbox"]
    assert all(bbox["counts"]["all"][name] > 0 for name in ("Cls", "Loc", "Both", "Dupe", "Bkg", "Miss")), bbox["counts"]
    assert bbox["counts"]["all"] == {"Cls": 5, "Loc": 3, "Both": 2, "Dupe": 2, "Bkg": 2, "Miss": 2}
    assert bbox["cls_confusion_by_split"] == {"seen": {"seen": 3, "unseen": 1}, "unseen": {"seen": 1, "unseen": 0}}
    assert 0 < bbox["AP50"] < 1 and bbox["dAP50_Cls"] > 0 and bbox["dAP50_Miss"] > 0 and bbox["dAP50_FalseNeg"] > 0
    assert sum(got["segm"]["counts"]["all"].values()) > 8
    # the base is evaluate_coco's AP50, bit for bit, overall and per split
    scores = coco_eval.evaluate_coco(dataset, predictions, TYPES, DEV)
    for t in TYPES:
        for key in ("AP50", "AP50_split_seen", "AP50_split_unseen"):
            assert got[t][key] == scores[t][key], (t, key)


def test_several_chunks_give_the_result_of_one(case, monkeypatch):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval, error_analysis
    sizes, real = [], coco_eval.score_chunk
    monkeypatch.setattr(coco_eval, "score_chunk", lambda images, *a, **k: sizes.append(len(images)) or real(images, *a, **k))
    got = error_analysis.analyze_errors(case["dataset"], case["predictions"], TYPES, DEV, max_images=1)
    assert sizes == [1] * 14
    for t in TYPES:
        _same(got[t], case["want"][t], t)
    whole, _ = coco_eval.match_tables(case["dataset"], case["predictions"], "bbox", DEV, error_thresholds=(.5, .1))
    parts, _ = coco_eval.match_tables(case["dataset"], case["predictions"], "bbox", DEV, error_thresholds=(.5, .1), max_images=2)
    assert sorted(whole) == sorted(parts)
    for key in whole:   # err_gt and the image rows are offset chunk by chunk
        assert np.array_equal(whole[key], parts[key]), key
    assert whole["num_images"] == 7 and whole["det_image"].max() == 6 and (whole["err_gt"] >= 0).sum() == 10


def test_results_files_give_the_same_analysis(case):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_results, error_analysis
    from tests.test_error_options import _tool
    files = coco_results.export_coco_results(case["dataset"], case["predictions"], str(case["folder"]), TYPES, DEV)
    got = error_analysis.analyze_errors_results(case["dataset"], files, TYPES, DEV)
    for t in TYPES:
        _same(got[t], case["want"][t], t)
    assert list(error_analysis.analyze_errors_results(case["dataset"], {"bbox": files["bbox"]}, TYPES, DEV)) == ["bbox"]
    # the tool: the tasks behind the scoring tables, the numbers in --output under the same names
    out = str(case["folder"] / "scores.json")
    tool = _tool("score_results")
    plain = tool.main(["--ann-file", case["paths"]["instances"], "--results-dir", str(case["folder"])])
    scored = tool.main(["--ann-file", case["paths"]["instances"], "--results-dir", str(case["folder"]), "--error-analysis",
                        "--boundary-ap", "--output", out])
    assert list(scored) == ["bbox", "segm", "boundary", "errors_bbox", "errors_segm"]
    for t in TYPES:
        assert scored[t] == plain[t]
    with open(out) as f:
        written = json.load(f)
    for t in TYPES:
        assert written[f"errors_{t}"] == json.loads(json.dumps(case["want"][t])), t


def test_the_flag_off_changes_no_table_and_no_key(case, monkeypatch):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    dataset, predictions = case["dataset"], case["predictions"]
    today = ["category", "det_start", "dt_ignore", "dt_match", "gt_ignore", "gt_start", "scores"]
    added = ["det_image", "err_gt", "err_type", "gt_image", "gt_missed", "num_images"]
    for iou_type in ("bbox", ("segm", "boundary")):
        on, _ = coco_eval.match_tables(dataset, predictions, iou_type, DEV, error_thresholds=(.5, .1))

        def boom(*a, **k):
            raise AssertionError("the error analysis ran without being asked for")
        with monkeypatch.context() as m:
            m.setattr(_C, "error_types", boom)
            m.setattr(coco_eval, "_image_problems", boom)
            off, _ = coco_eval.match_tables(dataset, predictions, iou_type, DEV)
        for name, tables in ({"bbox": off} if iou_type == "bbox" else off).items():
            with_errors = on if iou_type == "bbox" else on[name]
            assert sorted(tables) == today, name
            assert sorted(with_errors) == sorted(today + (added if name != "boundary" else [])), name   # boundary: not analysed
            for key in today:
                assert tables[key].dtype == with_errors[key].dtype and np.array_equal(tables[key], with_errors[key]), (name, key)
    with pytest.raises(ValueError, match="COCO's rules"):
        coco_eval.evaluate_coco(dataset, predictions, ("bbox",), DEV, rules="lvis", error_thresholds=(.5, .1))


def test_the_writer_adds_error_analysis_json_and_leaves_coco_results_alone(case, tmp_path, caplog):
    """What ``--evaluate --error-analysis`` does behind the gather (engine/evaluation.py::save_evaluation)."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import evaluation
    logger = logging.getLogger("ovis.test_errors")
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    plain.mkdir()
    flagged.mkdir()
    types = ("bbox", "segm", "boundary")
    a = evaluation.save_evaluation(case["dataset"], case["predictions"], str(plain), types, torch.device(DEV), logger, True)
    with caplog.at_level(logging.INFO, logger="ovis.test_errors"):
        b = evaluation.save_evaluation(case["dataset"], case["predictions"], str(flagged), types, torch.device(DEV), logger, True,
                                       errors=True)
    assert os.listdir(str(plain)) == ["coco_results.json"] and sorted(os.listdir(str(flagged))) == ["coco_results.json", "error_analysis.json"]
    assert (plain / "coco_results.json").read_bytes() == (flagged / "coco_results.json").read_bytes()
    assert list(a) == list(b) == ["box_proposal", "bbox", "segm", "boundary"]
    with open(str(flagged / "error_analysis.json")) as f:
        written = json.load(f)
    assert list(written) == ["bbox", "segm"]   # boundary is scored as before and not analysed
    for t in TYPES:
        assert written[t] == json.loads(json.dumps(case["want"][t])), t
    assert "Task: errors_bbox" in caplog.text and "Task: errors_segm" in caplog.text and "dAP50_Cls_split_unseen" in caplog.text
