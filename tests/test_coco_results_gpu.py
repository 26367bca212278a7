"""GPU: ``tools/infer_net.py --export-results`` / ``engine.coco_results.export_coco_results`` over the seven-image dataset of
tests/tiny_coco.py with the tiny model's detections: every ``segm.json`` entry decodes (``coco_eval.rle_decode``, the
scorer's independent decoder) to ``_C.paste_masks`` of that detection at the ORIGINAL image size, ``bbox.json`` lists the
same detections, and the chunk bound does not change a byte."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import tiny_coco

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs/coco_cap_det/student_teacher_mask_rcnn_uncertainty.yaml")
NAME = "coco_zeroshot_val"
OPTS = ["DATALOADER.NUM_WORKERS", "0", "INPUT.MIN_SIZE_TEST", "80", "INPUT.MAX_SIZE_TEST", "128", "TEST.IMS_PER_BATCH", "2",
        "MODEL.RPN.PRE_NMS_TOP_N_TEST", "200", "MODEL.RPN.POST_NMS_TOP_N_TEST", "40", "DATASETS.TEST", f"('{NAME}',)"]


def _load(folder):
    out = []
    for iou_type in ("bbox", "segm"):
        with open(os.path.join(folder, iou_type + ".json")) as f:
            out.append(json.load(f))
    return out


@pytest.fixture(scope="module")
def exported(tmp_path_factory):
    """One run of the tool: (dataset, saved predictions, the folder with predictions.pth, bbox.json and segm.json)."""
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import build_dataset
    from cvpr22_cross_modal_pseudo_labeling_amd.data.catalog import DatasetCatalog

    tmp = tmp_path_factory.mktemp("coco_results")
    paths = tiny_coco.write(tmp / "data")
    spec = importlib.util.spec_from_file_location("ovis_tool_infer_net", os.path.join(ROOT, "tools", "infer_net.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    torch.manual_seed(11)
    tool.main(["--config-file", YAML, "--dataset-catalog", paths["catalog"], "--data-dir", paths["root"], "--export-results"]
              + OPTS + ["OUTPUT_DIR", str(tmp / "out")])
    folder = str(tmp / "out" / "inference" / NAME)
    cfg = get_defaults()
    cfg.merge_from_file(YAML)
    cfg.merge_from_list(OPTS)
    dataset = build_dataset(cfg, NAME, DatasetCatalog(paths["catalog"], paths["root"]))
    predictions = torch.load(os.path.join(folder, "predictions.pth"), weights_only=False)
    return dataset, predictions, folder


def test_the_tool_leaves_both_files_beside_the_predictions(exported):
    dataset, predictions, folder = exported
    assert sorted(f for f in os.listdir(folder) if f.endswith((".json", ".pth"))) == ["bbox.json", "predictions.pth", "segm.json"]
    bbox, segm = _load(folder)
    total = sum(len(p) for p in predictions)
    assert total > 0 and len(bbox) == len(segm) == total
    for b, s in zip(bbox, segm):   # the same detections, entry by entry
        assert (b["image_id"], b["category_id"], b["score"]) == (s["image_id"], s["category_id"], s["score"])
        assert sorted(b) == ["bbox", "category_id", "image_id", "score"]
        assert sorted(s) == ["category_id", "image_id", "score", "segmentation"] and sorted(s["segmentation"]) == ["counts", "size"]
        assert isinstance(s["segmentation"]["counts"], str)


def test_every_segm_entry_decodes_to_the_pasted_mask(exported):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval

    dataset, predictions, folder = exported
    bbox, segm = _load(folder)
    at, set_pixels = 0, 0
    for idx, pred in enumerate(predictions):
        if len(pred) == 0:
            continue
        info = dataset.get_img_info(idx)
        h, w = info["height"], info["width"]
        xyxy, xywh = coco_eval.detection_boxes(pred, w, h)
        want = _C.paste_masks(pred.get_field("mask")[:, 0].float().cuda(), xyxy.cuda(), (h, w)).cpu().numpy()
        labels, scores = pred.get_field("labels").tolist(), pred.get_field("scores").tolist()
        for k in range(len(pred)):
            b, s = bbox[at + k], segm[at + k]
            assert b["image_id"] == dataset.id_to_img_map[idx] == s["image_id"]
            assert b["category_id"] == dataset.contiguous_category_id_to_json_id[labels[k]] and b["score"] == scores[k]
            assert b["bbox"] == xywh[k].tolist()
            assert s["segmentation"]["size"] == [h, w]
            got = coco_eval.rle_decode(s["segmentation"], h, w)
            assert np.array_equal(got, want[k].astype(np.uint8)), (idx, k)
            set_pixels += int(got.sum())
        at += len(pred)
    assert at == len(segm) and set_pixels > 0


def test_the_chunk_bound_does_not_change_the_files(exported, tmp_path, monkeypatch):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval, coco_results

    dataset, predictions, folder = exported
    calls = []
    real = _C.pasted_masks_rle
    monkeypatch.setattr(_C, "pasted_masks_rle", lambda *a, **k: calls.append(a[0].shape[0]) or real(*a, **k))
    paths = coco_results.export_coco_results(dataset, predictions, str(tmp_path / "default"), ("bbox", "segm"), "cuda")
    assert paths == {t: str(tmp_path / "default" / f"{t}.json") for t in ("bbox", "segm")}
    total = sum(len(p) for p in predictions)
    assert calls == [total]                       # one call for the whole set under the default bound
    del calls[:]
    monkeypatch.setattr(coco_eval, "MAX_EXPORT_MASKS", 1)
    coco_results.export_coco_results(dataset, predictions, str(tmp_path / "one"), ("bbox", "segm"), "cuda")
    assert calls == [1] * total
    for name in ("bbox.json", "segm.json"):
        files = [open(os.path.join(d, name), "rb").read() for d in (folder, str(tmp_path / "default"), str(tmp_path / "one"))]
        assert files[0] == files[1] == files[2], name
