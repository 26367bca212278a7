"""CPU: the host side of scoring COCO results files -- ``coco_eval.load_coco_results`` (pycocotools' ``loadRes`` and the cap of
100 per category and image) on the seven-image dataset of tests/tiny_coco.py, the command-line errors of
``tools/score_results.py``, and the decoder's prototypes and status codes as the binding reads them from the header."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

from tests import tiny_coco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RLE_B = {"size": [48, 64], "counts": [0, 10, 3062]}   # image 7 is 64 x 48


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    paths = tiny_coco.write(tmp_path_factory.mktemp("score_results"))
    return coco_eval.annotation_dataset(paths["instances"]), paths


def _box(image_id, category_id, score, bbox=(1, 2, 3, 4)):
    return {"image_id": image_id, "category_id": category_id, "score": score, "bbox": list(bbox)}


def test_annotation_dataset_needs_nothing_but_the_file(dataset):
    ds, _ = dataset
    assert ds.ids == tiny_coco.SORTED_IDS and ds.class_splits == {"seen": [17, 3, 8], "unseen": [44]}
    assert list(ds.categories.values()) == [name for _, name, _ in tiny_coco.CATEGORIES]


def test_rows_are_sorted_by_category_index_then_score_stably_in_file_order(dataset, tmp_path):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    ds, _ = dataset
    # sorted category ids 3, 8, 17, 44 -> indices 0..3.  Entries of image 7 interleaved with image 101's; two equal scores
    results = [_box(7, 17, .5, (0, 0, 1, 1)), _box(101, 3, .25), _box(7, 3, .5, (0, 0, 2, 2)), _box(7, 3, .75, (0, 0, 3, 3)),
               _box(7, 999, .9), _box(7, 3, .5, (0, 0, 4, 4)), _box(101, 44, 1.0, (9.5, 8.25, 7, 6)), _box(7, 8, .125, (0, 0, 5, 5))]
    rows = coco_eval.load_coco_results(ds, results, "bbox")
    assert len(rows) == 7   # one per image of the file, in id order
    by_id = dict(zip(tiny_coco.SORTED_IDS, rows))
    r = by_id[7]
    assert r["cats"].tolist() == [0, 0, 0, 1, 2] and r["scores"].tolist() == [.75, .5, .5, .125, .5]
    assert r["xywh"][:, 2].tolist() == [3, 2, 4, 5, 1] and r["entry"].tolist() == [3, 2, 5, 7, 0]   # category 999 is dropped
    assert r["xywh"].dtype == np.float64 and r["scores"].dtype == np.float64 and r["maps"] is None and r["xyxy"] is None
    assert by_id[101]["cats"].tolist() == [0, 3] and by_id[101]["xywh"][1].tolist() == [9.5, 8.25, 7, 6]
    for image_id in (12, 20, 31, 55, 90):
        assert len(by_id[image_id]["cats"]) == 0 and by_id[image_id]["xywh"].shape == (0, 4)
    path = tmp_path / "bbox.json"
    path.write_text(json.dumps(results))
    again = coco_eval.load_coco_results(ds, str(path), "bbox")   # a path reads the same
    for a, b in zip(rows, again):
        assert all(np.array_equal(a[k], b[k]) for k in ("cats", "scores", "xywh", "entry"))
    assert all(len(r["cats"]) == 0 for r in coco_eval.load_coco_results(ds, [], "bbox"))


def test_at_most_100_per_category_and_image_by_stable_score_order(dataset):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    ds, _ = dataset
    scores = [(k * 37 % 60) / 64 for k in range(120)]   # many ties
    results = [_box(7, 3, s, (k, 0, 1, 1)) for k, s in enumerate(scores)] + [_box(7, 8, .5), _box(12, 3, .5)]
    row = dict(zip(tiny_coco.SORTED_IDS, coco_eval.load_coco_results(ds, results, "bbox")))[7]
    want = np.argsort(-np.asarray(scores), kind="mergesort")[:100]
    assert row["cats"].tolist() == [0] * 100 + [1] and row["entry"].tolist() == want.tolist() + [120]
    assert row["xywh"][:100, 0].tolist() == want.tolist()


def test_segm_rows_carry_the_rle(dataset):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    ds, _ = dataset
    text = {"size": [48, 64], "counts": "0:PP3"}
    results = [{"image_id": 7, "category_id": 3, "score": .5, "segmentation": RLE_B},
               {"image_id": 7, "category_id": 3, "score": .75, "segmentation": text, "bbox": [0, 0, 1, 10]}]
    row = dict(zip(tiny_coco.SORTED_IDS, coco_eval.load_coco_results(ds, results, "segm")))[7]
    assert row["rle"] == [text, RLE_B] and row["entry"].tolist() == [1, 0] and row["maps"] is None and row["xyxy"] is None


@pytest.mark.parametrize("iou_type,entry,words", [
    ("bbox", _box(8, 3, .5), ["entry 1", "image_id 8"]),                                  # pycocotools asserts this
    ("bbox", {"image_id": 7, "category_id": 3, "bbox": [0, 0, 1, 1]}, ["entry 1", "image_id 7", "'score'"]),
    ("bbox", {"image_id": 7, "category_id": 3, "score": .5}, ["entry 1", "image_id 7", "'bbox'"]),
    ("segm", _box(7, 3, .5), ["entry 1", "image_id 7", "'segmentation'"]),
    ("segm", {"image_id": 7, "category_id": 3, "score": .5, "segmentation": [[0, 0, 5, 0, 5, 5]]}, ["entry 1", "image_id 7", "polygon"]),
    ("segm", {"image_id": 7, "category_id": 3, "score": .5, "segmentation": {"size": [64, 48], "counts": [3072]}},
     ["entry 1", "image_id 7", "48 x 64"]),
    ("segm", {"image_id": 7, "category_id": 3, "score": .5, "segmentation": {"counts": [3072]}}, ["entry 1", "image_id 7"]),
])
def test_errors_name_the_entry(dataset, iou_type, entry, words):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    ds, _ = dataset
    good = _box(101, 3, .5) if iou_type == "bbox" else {"image_id": 7, "category_id": 3, "score": .5, "segmentation": RLE_B}
    with pytest.raises(ValueError) as e:
        coco_eval.load_coco_results(ds, [good, entry], iou_type)
    assert all(w in str(e.value) for w in words), str(e.value)
    with pytest.raises(ValueError):
        coco_eval.load_coco_results(ds, {"annotations": []}, iou_type)   # not a results list
    with pytest.raises(ValueError):
        coco_eval.load_coco_results(ds, [good], "keypoints")


def test_evaluate_coco_results_refuses_the_host_in_evaluate_coco_s_words(dataset):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    ds, _ = dataset
    with pytest.raises(ValueError) as a:
        coco_eval.evaluate_coco_results(ds, {"bbox": []}, ("bbox",), "cpu")
    with pytest.raises(ValueError) as b:
        coco_eval.evaluate_coco(None, [], ("bbox",), "cpu")
    assert str(a.value).split(":", 1)[1] == str(b.value).split(":", 1)[1]


def test_score_results_command_line_errors(dataset, tmp_path, capsys):
    _, paths = dataset
    spec = importlib.util.spec_from_file_location("ovis_tool_score_results", os.path.join(ROOT, "tools", "score_results.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    (tmp_path / "empty").mkdir()
    (tmp_path / "full").mkdir()
    (tmp_path / "full" / "bbox.json").write_text("[]")
    for argv, word in (
            (["--ann-file", paths["instances"]], "no results file"),
            (["--ann-file", paths["instances"], "--results-dir", str(tmp_path / "empty")], "no results file"),
            (["--ann-file", paths["instances"], "--bbox", str(tmp_path / "none.json")], "does not exist"),
            (["--ann-file", str(tmp_path / "none.json"), "--results-dir", str(tmp_path / "full")], "does not exist"),
            (["--ann-file", paths["instances"], "--results-dir", str(tmp_path / "full"), "--device", "cpu"], "HIP device"),
            (["--results-dir", str(tmp_path / "full")], "--ann-file")):
        with pytest.raises(SystemExit) as e:
            tool.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv


def test_the_binding_reads_the_decoder_from_the_header():
    from cvpr22_cross_modal_pseudo_labeling_amd import _lib
    i, l, vp = C.c_int, C.c_long, C.c_void_p
    s = _lib.SIGNATURES
    assert s["ovis_coco_rle_count"] == (i, [vp, vp, i, vp, vp])
    assert s["ovis_coco_rle_runs"] == (i, [vp, vp, vp, i, vp, vp, vp])
    assert s["ovis_coco_runs_to_words"] == (i, [vp, vp, vp, vp, i, l, vp, vp, vp, vp, vp])
    codes = {k: v for k, v in _lib.CONSTANTS.items() if k.startswith("OVIS_COCO_RLE_")}
    assert codes == {"OVIS_COCO_RLE_OK": 0, "OVIS_COCO_RLE_BAD_CHAR": 1, "OVIS_COCO_RLE_UNTERMINATED": 2,
                     "OVIS_COCO_RLE_OVERFLOW": 3, "OVIS_COCO_RLE_NEGATIVE_RUN": 4, "OVIS_COCO_RLE_BAD_SUM": 5,
                     "OVIS_COCO_RLE_BAD_SIZE": 6}
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    assert sorted(_C.COCO_RLE_STATUS) == [1, 2, 3, 4, 5, 6]   # every non-zero code has its words
