"""GPU: Boundary AP end to end (engine/coco_eval.py, ``iou_type`` "boundary") on the seven-image datasets of
tests/tiny_coco.py (polygon ground truth and an RLE crowd) and tests/tiny_rle_coco.py (bitmap RLE ground truth): every number
and the device match tables against tests/boundary_reference.py on host-made masks; segm beside boundary bit-equal to segm
alone; the predictions route against the results-files route; sharded against unsharded; the recall keys; a detection set on
which boundary and segm differ; and ``tools/train_net.py --evaluate --boundary-ap`` leaving the training bit-identical."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import boundary_reference as bref
from tests import coco_eval_reference as ref
from tests import tiny_coco, tiny_rle_coco
from tests.test_coco_eval_gpu import M, SCALE, TABLE_KEYS, TINY_DETECTIONS, _restatement_images

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"ovis_tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _dataset(instances, img_dir):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCODataset
    dataset = COCODataset(instances, img_dir, False, {"LOAD_EMBEDDINGS": True, "EMB_KEY": "Tiny", "EMB_DIM": 4})
    assert dataset.ids == tiny_coco.SORTED_IDS
    return dataset


def _predictions(dataset, maps):
    """The detections of tests/test_coco_eval_gpu.py at twice the file's sizes.  ``maps``: "crisp" -- every map is 0.9
    throughout, the pasted mask is the box, a thick blob whose IoU is carried by its interior; "ragged" -- 0.9 inside and
    seeded noise on the two outer rings of cells, a thick blob with a rough outline; "noise" -- seeded noise throughout."""
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList
    g = torch.Generator().manual_seed(3)
    predictions = []
    for image_id in dataset.ids:
        info, dets = dataset.coco.imgs[image_id], TINY_DETECTIONS.get(image_id, [])
        pred = BoxList(torch.tensor([d[2] for d in dets], dtype=torch.float32).reshape(-1, 4) * SCALE,
                       (info["width"] * SCALE, info["height"] * SCALE))
        pred.add_field("scores", torch.tensor([d[1] for d in dets], dtype=torch.float32))
        pred.add_field("labels", torch.tensor([dataset.json_category_id_to_contiguous_id[d[0]] for d in dets], dtype=torch.int64))
        noise = torch.rand(len(dets), 1, M, M, generator=g)
        if maps != "noise":
            inner = slice(None) if maps == "crisp" else slice(2, M - 2)
            noise[:, :, inner, inner] = 0.9
        pred.add_field("mask", noise)
        predictions.append(pred)
    return predictions


def _host_masks(dataset, predictions, threshold=0.5):
    """({image id: detection masks}, {image id: ground-truth masks}) made on the HOST: ``paste_mask_in_image``, the host
    polygon rasteriser, the bitmaps tests/tiny_rle_coco.py encoded, and the run list of tiny_coco's crowd."""
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.roi_heads import paste_mask_in_image
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import PolygonMasks
    bitmaps = tiny_rle_coco.bitmaps()
    det_masks, gt_masks = {}, {}
    for idx, pred in enumerate(predictions):
        image_id = dataset.id_to_img_map[idx]
        info = dataset.coco.imgs[image_id]
        h, w = info["height"], info["width"]
        boxes = pred.bbox * torch.tensor([w / pred.size[0], h / pred.size[1]] * 2, dtype=torch.float32)
        det_masks[image_id] = [paste_mask_in_image(m[0], b, h, w, threshold, 1).numpy().astype(bool)
                               for m, b in zip(pred.get_field("mask"), boxes)]
        gt_masks[image_id] = []
        for a in dataset.coco.anns(image_id):
            seg = a["segmentation"]
            if isinstance(seg, dict) and isinstance(seg["counts"], list) and a["iscrowd"]:
                runs = np.asarray(seg["counts"])
                gt_masks[image_id].append(np.repeat(np.arange(len(runs)) % 2, runs).reshape(w, h).T.astype(bool))
            elif isinstance(seg, dict):
                gt_masks[image_id].append(bitmaps[a["id"]])
            else:
                gt_masks[image_id].append(PolygonMasks([seg], (w, h)).convert_to_binarymask()[0].numpy().astype(bool))
    return det_masks, gt_masks


def _no_pixel_at_the_threshold(dataset, predictions):
    """No host-pasted pixel within 2e-6 of the threshold: the device paste must give the same masks."""
    below, above = _host_masks(dataset, predictions, 0.5 - 2e-6)[0], _host_masks(dataset, predictions, 0.5 + 2e-6)[0]
    return all(np.array_equal(lo, hi) for i in below for lo, hi in zip(below[i], above[i]))


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """{name: (dataset, predictions, reference segm tables, reference boundary tables, category names in id order,
    splits)} -- the references are made once and shared."""
    paths = tiny_coco.write(tmp_path_factory.mktemp("tiny_boundary_ap"))
    bitmap_file = tiny_rle_coco.write(paths)
    out = {"paths": paths, "bitmap_file": bitmap_file}
    for name, instances, maps in (("polygon", paths["instances"], "ragged"), ("bitmap", bitmap_file, "ragged"),
                                  ("noise", paths["instances"], "noise"), ("crisp", paths["instances"], "crisp")):
        dataset = _dataset(instances, paths["img_dir"])
        predictions = _predictions(dataset, maps)
        assert _no_pixel_at_the_threshold(dataset, predictions), name
        images = _restatement_images(dataset, predictions, _host_masks(dataset, predictions))
        cat_ids = sorted(dataset.coco.cats)
        names = [dataset.categories[c] for c in cat_ids]
        splits = {s: [cat_ids.index(c) for c in ids] for s, ids in dataset.class_splits.items()}
        out[name] = (dataset, predictions, ref.match_tables(images, "segm"), bref.match_tables(images), names, splits)
    return out


def test_dilations_of_the_tiny_images_are_one_and_two():
    assert sorted({bref.dilation(h, w) for _, _, w, h, _ in tiny_coco.IMAGES}) == [1, 2]


@pytest.mark.parametrize("name", ["polygon", "bitmap", "noise", "crisp"])
def test_boundary_task_equals_the_restatement_and_segm_is_untouched(cases, name):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    dataset, predictions, segm_tables, boundary_tables, names, splits = cases[name]
    got = coco_eval.evaluate_coco(dataset, predictions, ("segm", "boundary"), DEV)
    assert list(got) == ["segm", "boundary"] and list(got["boundary"]) == list(got["segm"])
    for task, tables in (("segm", segm_tables), ("boundary", boundary_tables)):
        want = ref.summarize(ref.accumulate(tables, len(names)), names, splits)
        assert sorted(got[task]) == sorted(want)
        for k in want:
            print(name, task, k, got[task][k], want[k])
            assert abs(got[task][k] - want[k]) <= 1e-9, (task, k, got[task][k], want[k])
    # objects of a few dozen pixels with d = 1 or 2: a rough outline matches nothing by its boundary, only the crisp boxes do
    assert 0 < got["segm"]["AP"] < 1 and got["boundary"]["AP"] <= got["segm"]["AP"]
    if name == "crisp":
        assert 0 < got["boundary"]["AP"] < got["segm"]["AP"]   # the case is not degenerate
    # the device match tables: alone, and both from one pass over the chunks
    alone, cat_ids = coco_eval.match_tables(dataset, predictions, "boundary", DEV)
    both, _ = coco_eval.match_tables(dataset, predictions, ("segm", "boundary"), DEV)
    segm_alone, _ = coco_eval.match_tables(dataset, predictions, "segm", DEV)
    assert cat_ids == sorted(dataset.coco.cats) and sorted(both) == ["boundary", "segm"]
    for key in TABLE_KEYS:
        assert np.array_equal(alone[key], boundary_tables[key]), key
        assert np.array_equal(both["boundary"][key], boundary_tables[key]), key
        assert np.array_equal(both["segm"][key], segm_tables[key]) and np.array_equal(segm_alone[key], segm_tables[key]), key
        assert both["segm"][key].dtype == segm_alone[key].dtype and both["segm"][key].tobytes() == segm_alone[key].tobytes()
    # segm's numbers are those of a call without boundary, bit for bit, and boundary alone is boundary beside segm
    assert list(coco_eval.evaluate_coco(dataset, predictions, ("segm",), DEV)["segm"].items()) == list(got["segm"].items())
    assert list(coco_eval.evaluate_coco(dataset, predictions, ("boundary",), DEV)["boundary"].items()) == \
        list(got["boundary"].items())
    # chunked: a byte budget of one 64 x 48 image with six masks; an image always fits a chunk of its own
    chunked, _ = coco_eval.match_tables(dataset, predictions, ("segm", "boundary"), DEV, budget=6 * 64 * 48 * 11 // 8)
    for key in TABLE_KEYS:
        assert np.array_equal(chunked["boundary"][key], boundary_tables[key]), key
        assert np.array_equal(chunked["segm"][key], segm_tables[key]), key


def test_masks_are_made_once_for_segm_and_boundary(cases, monkeypatch):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    dataset, predictions = cases["polygon"][:2]
    calls = {}
    for entry in ("paste_masks", "polygons_to_masks", "coco_pack_masks", "coco_rle_words", "coco_boundary_words",
                  "coco_mask_iou", "coco_boundary_iou", "coco_match"):
        def counted(*a, _real=getattr(_C, entry), _entry=entry, **k):
            calls[_entry] = calls.get(_entry, 0) + 1
            return _real(*a, **k)
        monkeypatch.setattr(_C, entry, counted)
    coco_eval.evaluate_coco(dataset, predictions, ("segm",), DEV)
    segm_only = dict(calls)
    calls.clear()
    coco_eval.evaluate_coco(dataset, predictions, ("bbox", "segm", "boundary"), DEV)
    for entry in ("paste_masks", "polygons_to_masks", "coco_pack_masks", "coco_rle_words", "coco_mask_iou"):
        assert calls.get(entry, 0) == segm_only.get(entry, 0), entry   # nothing is pasted, rasterised, decoded or packed twice
    assert segm_only["paste_masks"] > 0 and "coco_boundary_words" not in segm_only
    assert calls["coco_boundary_words"] == segm_only["coco_pack_masks"]   # one call per image size and side
    assert calls["coco_boundary_iou"] == 1 and calls["coco_match"] == 3   # bbox, segm, boundary


def test_boundary_differs_from_segm_on_crisp_boxes(cases):
    """Full boxes around the ground truth: thick masks whose mask IoU passes thresholds their boundary IoU does not."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    dataset, predictions, segm_tables, boundary_tables, names, splits = cases["crisp"]
    assert not np.array_equal(segm_tables["dt_match"], boundary_tables["dt_match"])   # on the reference already
    got = coco_eval.evaluate_coco(dataset, predictions, ("segm", "boundary"), DEV)
    differing = [k for k in got["segm"] if got["segm"][k] != got["boundary"][k]]
    print(differing, got)
    assert "AP" in differing and got["boundary"]["AP"] < got["segm"]["AP"]
    # the area ranges stay those of the MASKS: what is ignored is the same, only what is matched changes
    assert np.array_equal(segm_tables["gt_ignore"], boundary_tables["gt_ignore"])


def test_predictions_route_equals_results_files_route(cases, tmp_path):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval, coco_results
    dataset, predictions = cases["bitmap"][:2]
    want = coco_eval.evaluate_coco(dataset, predictions, ("bbox", "segm", "boundary"), DEV, recall=True)
    files = coco_results.export_coco_results(dataset, predictions, str(tmp_path), ("bbox", "segm"), DEV)
    got = coco_eval.evaluate_coco_results(dataset, files, ("bbox", "segm", "boundary"), DEV, recall=True)
    assert list(got) == ["bbox", "segm", "boundary"]
    for task in want:
        assert list(got[task].items()) == list(want[task].items()), task
    for key in coco_eval.RECALL_METRICS + ("AR100_split_seen", "AR100_split_unseen"):
        assert key in got["boundary"] and list(got["boundary"]) == list(got["segm"])
    assert got["boundary"]["AR100"] <= got["segm"]["AR100"]
    # a "boundary" entry of its own is read instead of the segm one; without any mask file the task is skipped
    with open(files["segm"]) as f:
        segm = json.load(f)
    own = coco_eval.evaluate_coco_results(dataset, {"segm": [], "boundary": segm}, ("segm", "boundary"), DEV)
    assert own["segm"]["AP"] == 0 and list(own["boundary"].items()) == \
        [(k, v) for k, v in want["boundary"].items() if not k.startswith("AR")]
    assert list(coco_eval.evaluate_coco_results(dataset, {"bbox": files["bbox"]}, ("bbox", "segm", "boundary"), DEV)) == ["bbox"]
    # the tool: the table and the JSON gain the task behind segm, and nothing else changes
    out = str(tmp_path / "scores.json")
    scored = _tool("score_results").main(["--ann-file", cases["bitmap_file"], "--results-dir", str(tmp_path), "--boundary-ap",
                                          "--recall", "--output", out])
    assert list(scored) == ["bbox", "segm", "boundary"]
    with open(out) as f:
        written = json.load(f)
    for task in want:
        assert written[task] == dict(want[task]), task


def test_sharded_equals_unsharded(cases):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    dataset, predictions = cases["polygon"][:2]
    want = coco_eval.evaluate_coco(dataset, predictions, ("bbox", "segm", "boundary"), DEV, recall=True)
    local = dict(enumerate(predictions))
    got = coco_eval.evaluate_coco_sharded(dataset, local, ("bbox", "segm", "boundary"), DEV, recall=True)
    assert list(got) == ["bbox", "segm", "boundary"]
    for task in want:
        assert list(got[task].items()) == list(want[task].items()), task
    alone = coco_eval.evaluate_coco_sharded(dataset, local, ("boundary",), DEV)
    assert list(alone) == ["boundary"] and all(alone["boundary"][k] == want["boundary"][k] for k in alone["boundary"])
    # two shards' tables, merged as rank 0 merges them, are the unsharded tables
    cat_ids, images = coco_eval._ground_truth(dataset)
    by_image = {dataset.id_to_img_map[i]: p for i, p in local.items()}
    parts = {"segm": [], "boundary": []}
    for shard in (images[4:], images[:4]):
        dets = coco_eval._detection_rows(dataset, by_image, (cat_ids, shard), True)
        scored = coco_eval._score_rows(shard, dets, ("segm", "boundary"), torch.device(DEV, 0))
        problems = [len(np.union1d(d["cats"], im["cats"])) for im, d in zip(shard, dets)]
        for task in parts:
            scored[task]["image"] = np.repeat(np.asarray([im["id"] for im in shard], dtype=np.int64), problems)
            parts[task].append(scored[task])
    whole, _ = coco_eval.match_tables(dataset, predictions, ("segm", "boundary"), DEV)
    for task in parts:
        merged = coco_eval.merge_shard_tables(parts[task])
        for key in TABLE_KEYS:
            assert np.array_equal(merged[key], whole[task][key]), (task, key)


def test_the_dilation_ratio_is_a_keyword(cases):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    dataset, predictions, _, _, names, splits = cases["crisp"]
    images = _restatement_images(dataset, predictions, _host_masks(dataset, predictions))
    want = bref.evaluate(images, names, splits, ratio=0.1)   # d = 8 on the 64 x 48 image: deeper than most masks are wide
    got = coco_eval.evaluate_coco(dataset, predictions, ("boundary",), DEV, boundary_dilation_ratio=0.1)["boundary"]
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-9, (k, got[k], want[k])
    default = coco_eval.evaluate_coco(dataset, predictions, ("boundary",), DEV)["boundary"]
    assert dict(default) != dict(got)


# ---- a training run that scores Boundary AP is the plain training run -----------------------------------------------------------
TRAINING = ["DATALOADER.NUM_WORKERS", 0, "SOLVER.CHECKPOINT_PERIOD", 2, "SOLVER.TEST_PERIOD", 1, "SOLVER.LOG_PERIOD", 1,
            "SOLVER.BASE_LR", 0.005, "SOLVER.WARMUP_ITERS", 0, "DATASETS.TEST", ("coco_zeroshot_val",)]


def _same(a, b):
    if torch.is_tensor(a):
        return torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_train_net_boundary_ap_leaves_the_training_bit_identical(tmp_path):
    """Two iterations of the teacher configuration, scored behind each (TEST_PERIOD 1) and at the end: the histories and the
    final checkpoints of a plain run and of a ``--evaluate --boundary-ap`` run are equal bit for bit, and every
    ``coco_results*.json`` has the boundary task behind segm."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    paths = tiny_coco.write(tmp_path / "data")
    tool = _tool("train_net")
    runs = {}
    for name, kwargs in (("plain", {}), ("scored", {"evaluate": True, "boundary_ap": True})):
        out = str(tmp_path / name)
        cfg = tiny_coco.small_cfg("zeroshot_mask", extra=TRAINING + ["OUTPUT_DIR", out])
        torch.manual_seed(1234)
        history = tool.train(cfg, 0, False, 2, 2, save_checkpoints=True, dataset_catalog=paths["catalog"], data_dir=paths["root"],
                             seed=5, **kwargs)
        torch.cuda.synchronize()
        runs[name] = (history, torch.load(os.path.join(out, "model_final.pth"), map_location="cpu", weights_only=False), out)
    assert len(runs["plain"][0]) >= 1 and _same(runs["scored"][0], runs["plain"][0])
    assert _same(runs["scored"][1], runs["plain"][1])
    folder = os.path.join(runs["scored"][2], "inference", "coco_zeroshot_val")
    assert sorted(os.listdir(folder)) == ["coco_results.json", "coco_results_0000001.json", "coco_results_0000002.json",
                                          "predictions.pth"]
    for name in ("coco_results.json", "coco_results_0000001.json", "coco_results_0000002.json"):
        with open(os.path.join(folder, name)) as f:
            results = json.load(f)
        assert list(results) == ["bbox", "segm", "boundary"] and list(results["boundary"]) == list(results["segm"])
        assert list(results["segm"])[:6] == list(coco_eval.METRICS)
        for k, v in results["boundary"].items():
            assert v == -1 or 0 <= v <= 1, (name, k, v)
    with open(os.path.join(folder, "coco_results.json")) as f, open(os.path.join(folder, "coco_results_0000002.json")) as g:
        assert json.load(f) == json.load(g)   # the final test scores iteration 2's weights, by the gathered route
    with pytest.raises(ValueError):
        tool.train(tiny_coco.small_cfg("zeroshot_mask", extra=TRAINING + ["OUTPUT_DIR", str(tmp_path / "x")]), 0, False, 2, 2,
                   dataset_catalog=paths["catalog"], data_dir=paths["root"], boundary_ap=True)   # without evaluate
