"""CPU: the scalar restatement of COCO scoring (tests/coco_eval_reference.py) and the product's host accumulate / summarise
(engine/coco_eval.py), fed with the restatement's match tables, against hand-derived literals.  One 100 x 100 image, bbox
scoring.  Literals compare within 1e-9 (the means run over at most 101 * 10 * N values <= 1: fp64 summation-order error is
below 1e-11); the two precision arrays compare exactly."""
import numpy as np
import pytest

from tests import coco_eval_reference as ref

GT = {"category": 0, "bbox": [10, 10, 20, 20], "area": 400.0, "iscrowd": 0}
NAMES = ["a", "b", "c"]
SPLITS = {"seen": [0, 2], "unseen": [1]}


def _det(bbox, score, category=0):
    return {"category": category, "bbox": bbox, "score": score}


def _both(images, names=("a",), splits=None):
    """The restatement's and the product's summaries of the restatement's match tables; the precision arrays are equal."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval

    splits = splits or {}
    tables = ref.match_tables(images, "bbox")
    want = ref.accumulate(tables, len(names))
    got = coco_eval.accumulate(tables, len(names))
    assert got.shape == want.shape == (10, 101, len(names), 4, 3) and np.array_equal(got, want)
    a, b = ref.summarize(want, list(names), splits), coco_eval.summarize(got, list(names), splits)
    assert list(a) == list(b)
    return a, b


def _check(results, want):
    for res in results:
        for k, v in want.items():
            assert abs(res[k] - v) <= 1e-9, (k, res[k], v)


def test_constants_are_pycocotools_defaults():
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval

    assert np.array_equal(coco_eval.IOU_THRESHOLDS, ref.IOU_THRESHOLDS) and len(ref.IOU_THRESHOLDS) == 10
    assert ref.IOU_THRESHOLDS[0] == .5 and ref.IOU_THRESHOLDS[5] == .75 and abs(ref.IOU_THRESHOLDS[-1] - .95) < 1e-15
    assert np.array_equal(coco_eval.RECALL_THRESHOLDS, ref.RECALL_THRESHOLDS) and len(ref.RECALL_THRESHOLDS) == 101
    assert np.array_equal(coco_eval.AREA_RANGES, np.asarray(ref.AREA_RANGES)) and coco_eval.MAX_DETS == ref.MAX_DETS == (1, 10, 100)


def test_a_identical_detection():
    res = _both([{"dets": [_det([10, 10, 20, 20], .9)], "gts": [GT]}])
    _check(res, {"AP": 1, "AP50": 1, "AP75": 1, "APs": 1, "APm": -1, "APl": -1, "AP50_class_a": 1})


def test_b_higher_scoring_false_positive_first():
    images = [{"dets": [_det([10, 10, 20, 20], .8), _det([50, 50, 20, 20], .9)], "gts": [GT]}]
    res = _both(images)
    half = 1 / (2 + np.spacing(1))
    assert abs(half - .5) < 1e-15
    _check(res, {"AP": .5, "AP50": .5, "AP75": .5, "APs": .5, "APm": -1, "APl": -1})
    tables = ref.match_tables(images, "bbox")
    assert tables["scores"].tolist() == [.9, .8] and tables["dt_match"][0, :, 0].tolist() == [-1] * 10 \
        and tables["dt_match"][0, :, 1].tolist() == [0] * 10
    assert np.all(ref.accumulate(tables, 1)[:, :, 0, 0, 2] == half)


def test_c_iou_0625():
    # xyxy [10, 10, 29, 21.5] is xywh [10, 10, 20, 12.5]: i = 250, u = 250 + 400 - 250
    assert ref.box_iou([10, 10, 20, 12.5], GT["bbox"], 0) == .625
    res = _both([{"dets": [_det([10, 10, 20, 12.5], .9)], "gts": [GT]}])
    _check(res, {"AP": .3, "AP50": 1, "AP75": 0})


def test_d_only_a_crowd():
    crowd = {"category": 0, "bbox": [0, 0, 100, 100], "area": 10000.0, "iscrowd": 1}
    images = [{"dets": [_det([10, 10, 20, 20], .9)], "gts": [crowd]}]
    assert ref.box_iou([10, 10, 20, 20], crowd["bbox"], 1) == 1.0
    tables = ref.match_tables(images, "bbox")
    assert tables["dt_match"][:, :, 0].tolist() == [[0] * 10] * 4 and tables["dt_ignore"].all() and tables["gt_ignore"].all()
    res = _both(images)
    for r in res:
        assert all(v == -1 for v in r.values()), r


def test_e_two_categories_two_splits_and_one_without_ground_truth():
    images = [{"dets": [_det([10, 10, 20, 20], .9, 0)], "gts": [GT, dict(GT, category=1, bbox=[60, 60, 30, 30], area=900.0)]}]
    res = _both(images, NAMES, SPLITS)
    _check(res, {"AP": .5, "AP50": .5, "AP50_class_a": 1, "AP50_class_b": 0, "AP50_class_c": -1, "AP50_split_seen": 1,
                 "AP50_split_unseen": 0})
    for r in res:
        assert list(r) == ["AP", "AP50", "AP75", "APs", "APm", "APl", "AP50_class_a", "AP50_class_b", "AP50_class_c",
                           "AP50_split_seen", "AP50_split_unseen"]


def test_format_results_is_the_reference_table():
    from collections import OrderedDict

    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval

    text = coco_eval.format_results(OrderedDict(bbox=OrderedDict([("AP", .5), ("AP50", -1)])))
    assert text == "\nTask: bbox\nAP, AP50\n0.5000, -1.0000\n"


def test_rle_decode_uncompressed_and_compressed():
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval

    m = coco_eval.rle_decode({"counts": [0, 10, 3062], "size": [48, 64]}, 48, 64)
    assert m.shape == (48, 64) and m.dtype == np.uint8 and int(m.sum()) == 10 and m[:10, 0].all()   # column-major
    # runs 2, 3, 4, 3 as pycocotools' string: one character each, chr(48 + x) for 0 <= x < 16; the fourth and later runs
    # are stored as differences to the run two before (3 - 3 = 0)
    assert np.array_equal(coco_eval.rle_decode({"counts": "2340", "size": [3, 4]}, 3, 4),
                          coco_eval.rle_decode({"counts": [2, 3, 4, 3], "size": [3, 4]}, 3, 4))
    with pytest.raises(ValueError):
        coco_eval.rle_decode({"counts": [1, 2], "size": [3, 4]}, 3, 4)


def test_infer_net_evaluate_is_a_command_line_error_without_output_dir_or_device(tmp_path, capsys):
    import importlib.util
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("ovis_tool_infer_net", os.path.join(root, "tools", "infer_net.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    argv = ["--dataset-catalog", str(tmp_path / "none.json"), "--evaluate"]
    for opts, word in ((["MODEL.DEVICE", "cpu", "OUTPUT_DIR", ""], "set OUTPUT_DIR"), (["MODEL.DEVICE", "cpu", "OUTPUT_DIR", str(tmp_path)], "set MODEL.DEVICE cuda")):
        with pytest.raises(SystemExit) as e:
            tool.main(argv + opts)
        assert e.value.code == 2 and word in capsys.readouterr().err


def test_evaluate_coco_refuses_the_host():
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval

    with pytest.raises(ValueError):
        coco_eval.evaluate_coco(None, [], ("bbox",), "cpu")


def test_chunks_stay_inside_what_one_paste_or_rasterise_call_takes():
    """1000 images of one size with 100 detections and 20 single-polygon ground truths each, an unlimited byte budget: no
    chunk holds more than 65535 detections (one ``paste_masks`` call per image size), ground truths or polygons; every
    image is in exactly one chunk, in order."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval

    assert coco_eval.MAX_CALL_MASKS == 65535
    image = {"cats": np.zeros(20, np.int64), "height": 480, "width": 640, "polygons": 20}
    det = {"cats": np.zeros(100, np.int64)}
    chunks = list(coco_eval._chunks([image] * 1000, [det] * 1000, True, 1 << 62))
    assert [len(c) for c in chunks] == [655, 345] and sum(chunks, []) == list(range(1000))
    many_polygons = dict(image, polygons=40000)
    assert [len(c) for c in coco_eval._chunks([many_polygons] * 3, [det] * 3, True, 1 << 62)] == [1, 1, 1]
    assert [len(c) for c in coco_eval._chunks([image] * 1000, [det] * 1000, False, 0)] == [1000]    # boxes cost nothing
    assert [len(c) for c in coco_eval._chunks([image] * 5, [det] * 5, False, 0, max_images=2)] == [2, 2, 1]
    per_image = 120 * 480 * 640 * 9 // 8
    assert [len(c) for c in coco_eval._chunks([image] * 5, [det] * 5, True, 2 * per_image)] == [2, 2, 1]
    assert [len(c) for c in coco_eval._chunks([image] * 3, [det] * 3, True, 0)] == [1, 1, 1]        # never an empty chunk
