"""CPU: the COCO results export (engine/coco_results.py, ``tools/infer_net.py --export-results``) on host tensors, and the
NumPy restatement of pycocotools' encoder (tests/coco_rle_reference.py) that the device encoder's tests use as expected
values -- held here to ``coco_eval.rle_decode``, which was written independently for the scorer, and to known strings."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import coco_rle_reference as rle
from tests import tiny_coco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement of rleEncode / rleToString -----------------------------------------------------------------------------
def _thin_mask_near_the_end():
    """1200 x 1100: nothing before column 1000 (a leading run of 1.2e6 >= 2^20: five characters), then runs of unequal
    lengths (46 ones, then 5 ones: 5 - 46 < 0 in the string's differences)."""
    m = np.zeros((1200, 1100), np.uint8)
    m[5:51, 1000] = 1
    m[5:10, 1001] = 1
    m[700:1200, 1099] = 1   # up to the image's last pixel
    return m


def _masks(h, w):
    rs = np.random.RandomState(h * 1000 + w)
    out = {"empty": np.zeros((h, w), np.uint8), "full": np.ones((h, w), np.uint8),
           "random": (rs.rand(h, w) < 0.4).astype(np.uint8), "rect": np.zeros((h, w), np.uint8),
           "first_pixel": np.zeros((h, w), np.uint8)}
    out["rect"][h // 3:h // 3 + max(1, h // 2), w // 4:w // 4 + max(1, w // 2)] = 1
    out["first_pixel"][0, 0] = 1
    out["first_pixel"][h - 1, w - 1] = 1
    return out


@pytest.mark.parametrize("h,w", [(1, 1), (3, 4), (33, 17), (1200, 1100)])
def test_restatement_round_trips_through_rle_decode(h, w):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval

    masks = _masks(h, w)
    if (h, w) == (1200, 1100):
        masks["thin"] = _thin_mask_near_the_end()
    for name, mask in masks.items():
        counts = rle.rle_encode(mask)
        assert sum(counts) == h * w and all(c >= 0 for c in counts) and all(c > 0 for c in counts[1:]), name
        assert (counts[0] == 0) == bool(mask[0, 0]), name
        text = rle.rle_to_string(counts)
        assert np.array_equal(coco_eval.rle_decode({"counts": counts, "size": [h, w]}, h, w), mask), name
        assert np.array_equal(coco_eval.rle_decode({"counts": text.decode("ascii"), "size": [h, w]}, h, w), mask), name
        assert rle.encode(mask) == {"size": [h, w], "counts": text.decode("ascii")}
    assert rle.rle_encode(masks["empty"]) == [h * w] and rle.rle_encode(masks["full"]) == [0, h * w]


def test_restatement_gives_the_known_strings():
    assert rle.rle_to_string([2, 3, 4, 3]) == b"2340"         # the string tests/test_coco_eval_reference.py decodes
    assert rle.rle_to_string([0, 10, 3062]) == b"0:fo2"       # the RLE ground truth of tests/tiny_coco.py
    counts = rle.rle_encode(_thin_mask_near_the_end())
    assert counts[0] == 1000 * 1200 + 5 >= 1 << 20 and len(rle.rle_to_string(counts[:1])) == 5
    assert min(counts[i] - counts[i - 2] for i in range(3, len(counts))) < 0
    flat = np.zeros(12, np.uint8)   # column-major
    flat[2:5] = flat[9:12] = 1
    assert rle.rle_encode(flat.reshape(4, 3).T) == [2, 3, 4, 3]


# ---- bbox.json on host tensors --------------------------------------------------------------------------------------------------
DETECTIONS = {   # image id -> (prediction size as a multiple of the file's (w, h), [(json category id, score, xyxy at that size)])
    7: ((2, 2), [(8, .9, [20, 20, 78.5, 58]), (3, .8, [0, 0, 6, 24]), (17, .6, [10.25, 10, 60, 60])]),
    12: ((3, 2), [(8, .75, [6, 6, 33, 24]), (17, .5, [61, 10.5, 120.25, 50])]),   # one ratio per axis
    20: ((1, 1), [(3, .9, [5, 5, 30, 40])]),
    55: ((2, 2), [(44, .5 + k / 1000, [k % 50, k % 45, 50 + k % 50, 52 + k % 45]) for k in range(130)]),  # > 100 of one category
    101: ((1, 1), [(17, .9, [30, 10, 42, 29]), (3, .85, [30, 20, 50, 35])]),
}   # images 31 and 90 get empty predictions


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCODataset
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList

    paths = tiny_coco.write(tmp_path_factory.mktemp("tiny_coco_results"))
    dataset = COCODataset(paths["instances"], paths["img_dir"], False, {"LOAD_EMBEDDINGS": True, "EMB_KEY": "Tiny", "EMB_DIM": 4})
    assert dataset.ids == tiny_coco.SORTED_IDS
    predictions = []
    for image_id in dataset.ids:
        info = dataset.coco.imgs[image_id]
        (kw, kh), dets = DETECTIONS.get(image_id, ((1, 1), []))
        pred = BoxList(torch.tensor([d[2] for d in dets], dtype=torch.float32).reshape(-1, 4), (info["width"] * kw, info["height"] * kh))
        pred.add_field("scores", torch.tensor([d[1] for d in dets], dtype=torch.float32))
        pred.add_field("labels", torch.tensor([dataset.json_category_id_to_contiguous_id[d[0]] for d in dets], dtype=torch.int64))
        predictions.append(pred)
    return dataset, predictions


def test_bbox_export_on_host_tensors(tiny, tmp_path):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_results

    dataset, predictions = tiny
    paths = coco_results.export_coco_results(dataset, predictions, str(tmp_path / "out"), ("bbox",), "cpu")
    assert paths == {"bbox": str(tmp_path / "out" / "bbox.json")}
    with open(paths["bbox"]) as f:
        got = json.load(f)
    want = []
    for image_id in tiny_coco.SORTED_IDS:          # dataset-index order; images without detections contribute nothing
        (kw, kh), dets = DETECTIONS.get(image_id, ((1, 1), []))
        for cat, score, box in dets:               # prediction order, all of them
            # BoxList.resize then convert("xywh") in float32: x * float32(ratio), w = x2 - x1 + 1
            rx, ry = np.float32(1.0 / kw), np.float32(1.0 / kh)
            x1, y1, x2, y2 = (np.float32(v) * r for v, r in zip(box, (rx, ry, rx, ry)))
            xywh = [x1, y1, x2 - x1 + np.float32(1), y2 - y1 + np.float32(1)]
            assert all(v.dtype == np.float32 for v in xywh)
            want.append({"image_id": image_id, "category_id": cat, "bbox": [float(v) for v in xywh], "score": float(np.float32(score))})
    assert len(got) == len(want) == sum(len(d[1]) for d in DETECTIONS.values())
    assert got == want
    assert sum(1 for r in got if r["image_id"] == 55 and r["category_id"] == 44) == 130   # no cap of 100 per category
    assert {r["image_id"] for r in got} == set(DETECTIONS) and {r["category_id"] for r in got} <= {17, 3, 44, 8}
    # the same numbers the scorer's rows are made of (one conversion, shared)
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    idx = tiny_coco.SORTED_IDS.index(12)
    _, xywh = coco_eval.detection_boxes(predictions[idx], 45, 33)
    assert [r["bbox"] for r in got if r["image_id"] == 12] == xywh.tolist()


def test_no_predictions_write_an_empty_list(tiny, tmp_path):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_results

    dataset, predictions = tiny
    paths = coco_results.export_coco_results(dataset, [], str(tmp_path), ("bbox",), "cpu")
    with open(paths["bbox"]) as f:
        assert json.load(f) == []
    empty = predictions[3:4]   # image 31's empty prediction alone
    assert len(empty) == 1 and len(empty[0]) == 0
    with open(coco_results.export_coco_results(dataset, empty, str(tmp_path), ("bbox",), "cpu")["bbox"]) as f:
        assert json.load(f) == []


def test_segm_needs_the_device_and_unpasted_maps(tiny, tmp_path):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_results

    dataset, predictions = tiny
    with pytest.raises(ValueError, match="HIP device"):
        coco_results.export_coco_results(dataset, predictions, str(tmp_path), ("bbox", "segm"), "cpu")
    with pytest.raises(ValueError, match="iou_type"):
        coco_results.export_coco_results(dataset, predictions, str(tmp_path), ("keypoints",), "cpu")
    pasted = []
    for pred in predictions:   # masks already at image size: the scorer's message, before anything reaches a device
        p = pred.copy_with_fields(["scores", "labels"])
        p.add_field("mask", torch.zeros(len(p), 1, pred.size[1], pred.size[0]))
        pasted.append(p)
    with pytest.raises(ValueError, match="already pasted into the image"):
        coco_results.export_coco_results(dataset, pasted, str(tmp_path), ("segm",), "cuda")
    with pytest.raises(ValueError, match="'mask' field"):
        coco_results.export_coco_results(dataset, predictions, str(tmp_path), ("segm",), "cuda")


def test_device_encoder_refuses_host_tensors():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    probs, boxes, sizes = torch.zeros(2, 14, 14), torch.zeros(2, 4), torch.ones(2, 2, dtype=torch.int32)
    for fn in (_C.pasted_masks_runs, _C.pasted_masks_rle):
        with pytest.raises(RuntimeError, match="no host implementation"):
            fn(probs, boxes, sizes)


def test_infer_net_export_results_is_a_command_line_error_without_output_dir_or_device(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("ovis_tool_infer_net", os.path.join(ROOT, "tools", "infer_net.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    argv = ["--dataset-catalog", str(tmp_path / "none.json"), "--export-results"]
    for opts, words in ((["MODEL.DEVICE", "cpu", "OUTPUT_DIR", ""], ("set OUTPUT_DIR", "bbox.json", "segm.json")),
                        (["MODEL.DEVICE", "cpu", "MODEL.MASK_ON", "True", "OUTPUT_DIR", str(tmp_path)], ("set MODEL.DEVICE cuda",))):
        with pytest.raises(SystemExit) as e:
            tool.main(argv + opts)
        err = capsys.readouterr().err
        assert e.value.code == 2 and all(w in err for w in words), err
