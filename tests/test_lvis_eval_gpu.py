"""GPU: LVIS-style federated scoring end to end (engine/coco_eval.py ``rules="lvis"``, csrc/lvis_eval.hip) on the six-image
dataset of tests/tiny_lvis.py -- polygon and RLE ground truth, an image without annotations, 8 categories over three
frequencies and two splits: every number and the device match tables of bbox, segm and boundary against
tests/lvis_reference.py on host-made masks; the results-files route; the degenerate file on which LVIS-style and COCO
scoring agree; the errors of a file that is not federatedly annotated; ``rules="coco"`` untouched; sharded against
unsharded."""
import copy
import importlib.util
import json
import logging
import os

import numpy as np
import pytest
import torch

from tests import lvis_reference as lref
from tests import tiny_lvis

pytestmark = pytest.mark.gpu

DEV = "cuda"
M = 14
SCALE = 2   # the predictions live at twice the file's image sizes
TYPES = ("bbox", "segm", "boundary")
TABLE_KEYS = ("category", "det_start", "gt_start", "scores", "dt_match", "dt_ignore", "gt_ignore")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"ovis_tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _dataset(path):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    dataset = coco_eval.annotation_dataset(path)
    assert dataset.ids == tiny_lvis.SORTED_IDS
    assert dataset.class_splits == {"seen": [20, 2, 5, 31, 11], "unseen": [9, 14, 23]}
    return dataset


def _predictions(dataset):
    """tiny_lvis.DETECTIONS at twice the file's sizes; the maps are 0.9 inside and seeded noise on the two outer rings of
    cells -- thick blobs with a rough outline -- or, for every other detection, 0.9 throughout."""
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList
    g = torch.Generator().manual_seed(5)
    predictions = []
    for image_id in dataset.ids:
        info, dets = dataset.coco.imgs[image_id], tiny_lvis.DETECTIONS.get(image_id, [])
        pred = BoxList(torch.tensor([d[2] for d in dets], dtype=torch.float32).reshape(-1, 4) * SCALE,
                       (info["width"] * SCALE, info["height"] * SCALE))
        pred.add_field("scores", torch.tensor([d[1] for d in dets], dtype=torch.float32))
        pred.add_field("labels", torch.tensor([dataset.json_category_id_to_contiguous_id[d[0]] for d in dets], dtype=torch.int64))
        maps = torch.rand(len(dets), 1, M, M, generator=g)
        maps[:, :, 2:M - 2, 2:M - 2] = 0.9
        maps[0::2] = 0.9   # every other one crisp: the pasted mask is the box, which a boundary can match
        pred.add_field("mask", maps)
        predictions.append(pred)
    return predictions


def _host_masks(dataset, predictions, threshold=0.5):
    """({image id: detection masks}, {annotation id: ground-truth mask}) made on the HOST: ``paste_mask_in_image``, the host
    polygon rasteriser and the bitmaps tests/tiny_lvis.py encoded."""
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.roi_heads import paste_mask_in_image
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import PolygonMasks
    bitmaps = {7: tiny_lvis.blob(), 8: tiny_lvis.box_bitmap()}
    det_masks, gt_masks = {}, {}
    for idx, pred in enumerate(predictions):
        image_id = dataset.id_to_img_map[idx]
        info = dataset.coco.imgs[image_id]
        h, w = info["height"], info["width"]
        boxes = pred.bbox * torch.tensor([w / pred.size[0], h / pred.size[1]] * 2, dtype=torch.float32)
        det_masks[image_id] = [paste_mask_in_image(m[0], b, h, w, threshold, 1).numpy().astype(bool)
                               for m, b in zip(pred.get_field("mask"), boxes)]
        for a in dataset.coco.anns(image_id):
            seg = a["segmentation"]
            gt_masks[a["id"]] = bitmaps[a["id"]] if isinstance(seg, dict) else \
                PolygonMasks([seg], (w, h)).convert_to_binarymask()[0].numpy().astype(bool)
    return det_masks, gt_masks


def _reference_input(dataset, predictions, data):
    """(the annotation dict with a ``mask`` per annotation, the detections as the restatement takes them: the float32 xywh
    of the prepared boxes at the file's image size, widened, and the host-pasted mask)."""
    det_masks, gt_masks = _host_masks(dataset, predictions)
    below, above = _host_masks(dataset, predictions, 0.5 - 2e-6)[0], _host_masks(dataset, predictions, 0.5 + 2e-6)[0]
    for image_id in below:   # no host-pasted pixel within 2e-6 of the threshold: the device paste must give the same masks
        for lo, hi in zip(below[image_id], above[image_id]):
            assert np.array_equal(lo, hi), image_id
    data = copy.deepcopy(data)
    for a in data["annotations"]:
        a["mask"] = gt_masks[a["id"]]
    dets = []
    for idx, p in enumerate(predictions):
        image_id = dataset.id_to_img_map[idx]
        info = dataset.coco.imgs[image_id]
        box = p.bbox * torch.tensor([info["width"] / p.size[0], info["height"] / p.size[1]] * 2, dtype=torch.float32)
        xywh = torch.stack((box[:, 0], box[:, 1], box[:, 2] - box[:, 0] + 1, box[:, 3] - box[:, 1] + 1), 1).double().tolist()
        for k in range(len(p)):
            dets.append({"image_id": image_id, "category_id": dataset.contiguous_category_id_to_json_id[int(p.get_field("labels")[k])],
                         "score": float(p.get_field("scores")[k].double()), "bbox": xywh[k], "mask": det_masks[image_id][k]})
    return data, dets


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The dataset, the predictions and the restatement's tables and numbers of every task -- made once and shared."""
    folder = tmp_path_factory.mktemp("tiny_lvis")
    path = tiny_lvis.write(folder / "lvis.json")
    dataset = _dataset(path)
    predictions = _predictions(dataset)
    data, dets = _reference_input(dataset, predictions, tiny_lvis.dataset_dict())
    cat_ids = sorted(dataset.coco.cats)
    names = [dataset.categories[c] for c in cat_ids]
    frequencies = [dataset.coco.cats[c]["frequency"] for c in cat_ids]
    splits = {s: [cat_ids.index(c) for c in ids] for s, ids in dataset.class_splits.items()}
    out = {"dataset": dataset, "predictions": predictions, "data": data, "dets": dets, "names": names, "splits": splits,
           "frequencies": frequencies, "folder": folder, "path": path, "tables": {}, "want": {}, "want_recall": {}}
    for task in TYPES:
        tables = lref.match_tables(data, dets, task)
        precision, recall = lref.accumulate(tables, len(names))
        out["tables"][task] = tables
        out["want"][task] = lref.summarize(precision, names, frequencies, splits)
        out["want_recall"][task] = lref.summarize(precision, names, frequencies, splits, recall)
    return out


def _assert_summary(got, want, where):
    assert sorted(got) == sorted(want), where
    for k in want:
        print(where, k, got[k], want[k])
        assert abs(got[k] - want[k]) <= 1e-9, (where, k, got[k], want[k])


def test_evaluate_lvis_equals_the_restatement(case):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    dataset, predictions = case["dataset"], case["predictions"]
    in_file_order = [name for _, name, _, _ in tiny_lvis.CATEGORIES]   # AP50_class_ keys iterate dataset.categories
    assert in_file_order != case["names"] and list(dataset.categories.values()) == in_file_order
    ap_keys = list(coco_eval.LVIS_METRICS) + [f"AP50_class_{n}" for n in in_file_order] + ["AP50_split_seen", "AP50_split_unseen"]
    ar_keys = list(coco_eval.LVIS_RECALL_METRICS) + ["AR@300_split_seen", "AR@300_split_unseen"]
    assert coco_eval.LVIS_METRICS == ("AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf")
    got = coco_eval.evaluate_coco(dataset, predictions, TYPES, DEV, rules="lvis")
    with_recall = coco_eval.evaluate_coco(dataset, predictions, TYPES, DEV, recall=True, rules="lvis")
    assert list(got) == list(TYPES) and list(with_recall) == list(TYPES)
    for task in TYPES:
        assert list(got[task]) == ap_keys and list(with_recall[task]) == ap_keys + ar_keys
        _assert_summary(got[task], case["want"][task], task)
        _assert_summary(with_recall[task], case["want_recall"][task], task + " with recall")
        tables, cat_ids = coco_eval.match_tables(dataset, predictions, task, DEV, rules="lvis")
        assert cat_ids == sorted(dataset.coco.cats)
        for key in TABLE_KEYS:
            assert np.array_equal(tables[key], case["tables"][task][key]), (task, key)
        want = case["want"][task]
        assert 0 < want["AP"] < 1 and want["APr"] > -1 and want["APc"] > -1 and want["APf"] > -1   # the case is not degenerate
        assert want["APl"] == -1 and want["APm"] > -1
    # one pass over the mask words serves segm and boundary, and chunks of one image give the same tables
    both, _ = coco_eval.match_tables(dataset, predictions, ("segm", "boundary"), DEV, rules="lvis", max_images=1)
    for task in ("segm", "boundary"):
        for key in TABLE_KEYS:
            assert np.array_equal(both[task][key], case["tables"][task][key]), (task, key)
    # what the rules did to the 30 detections: the three strays are gone, 27 are judged
    bbox = case["tables"]["bbox"]
    assert len(bbox["scores"]) == 27 and sum(len(d) for d in tiny_lvis.DETECTIONS.values()) == 30
    assert bbox["not_exhaustive"].sum() > 0 and bbox["dt_ignore"][0, 0].sum() >= 4 and (bbox["gt_ignore"][0].sum() == 2)


def test_the_cap_is_a_keyword(case):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    dataset, predictions = case["dataset"], case["predictions"]
    capped, _ = coco_eval.match_tables(dataset, predictions, "bbox", DEV, rules="lvis", lvis_max_dets=4)
    want = lref.match_tables(case["data"], case["dets"], "bbox", max_dets=4)
    for key in TABLE_KEYS:
        assert np.array_equal(capped[key], want[key]), key
    assert len(want["scores"]) < len(case["tables"]["bbox"]["scores"])   # image 3's cap of 4 falls on its stray too
    got = coco_eval.evaluate_coco(dataset, predictions, ("bbox",), DEV, rules="lvis", lvis_max_dets=4)["bbox"]
    precision, _ = lref.accumulate(want, len(case["names"]))
    _assert_summary(got, lref.summarize(precision, case["names"], case["frequencies"], case["splits"]), "cap 4")
    uncapped, _ = coco_eval.match_tables(dataset, predictions, "bbox", DEV, rules="lvis", lvis_max_dets=-1)
    for key in TABLE_KEYS:
        assert np.array_equal(uncapped[key], case["tables"]["bbox"][key]), key


def test_results_files_give_the_numbers_of_the_predictions(case):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval, coco_results
    dataset, predictions = case["dataset"], case["predictions"]
    want = coco_eval.evaluate_coco(dataset, predictions, TYPES, DEV, recall=True, rules="lvis")
    files = coco_results.export_coco_results(dataset, predictions, str(case["folder"]), ("bbox", "segm"), DEV)
    got = coco_eval.evaluate_coco_results(dataset, files, TYPES, DEV, recall=True, rules="lvis")
    assert list(got) == list(TYPES)
    for task in TYPES:
        assert list(got[task].items()) == list(want[task].items()), task
    # the tool: --lvis beside --boundary-ap and --recall, the numbers in the JSON it writes
    out = str(case["folder"] / "scores.json")
    scored = _tool("score_results").main(["--ann-file", case["path"], "--results-dir", str(case["folder"]), "--lvis",
                                          "--boundary-ap", "--recall", "--output", out])
    assert list(scored) == list(TYPES)
    with open(out) as f:
        written = json.load(f)
    for task in TYPES:
        assert written[task] == dict(want[task]), task
    capped = coco_eval.evaluate_coco_results(dataset, {"bbox": files["bbox"]}, ("bbox",), DEV, rules="lvis", lvis_max_dets=4)
    assert list(capped["bbox"].items()) == \
        list(coco_eval.evaluate_coco(dataset, predictions, ("bbox",), DEV, rules="lvis", lvis_max_dets=4)["bbox"].items())


def test_lvis_numbers_are_saved_as_lvis_results(case, tmp_path):
    """What ``--evaluate --lvis`` does behind the gather (engine/evaluation.py::save_evaluation): the table is logged, the
    numbers go to lvis_results.json and no coco_results.json appears."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval, evaluation
    logger = logging.getLogger("ovis.test_lvis")
    got = evaluation.save_evaluation(case["dataset"], case["predictions"], str(tmp_path), TYPES, torch.device(DEV), logger, lvis=True)
    assert os.listdir(str(tmp_path)) == ["lvis_results.json"]
    with open(str(tmp_path / "lvis_results.json")) as f:
        written = json.load(f)
    want = coco_eval.evaluate_coco(case["dataset"], case["predictions"], TYPES, DEV, rules="lvis")
    assert list(written) == list(TYPES)
    for task in TYPES:
        assert written[task] == dict(want[task]) == dict(got[task]), task
    assert "APr" in coco_eval.format_results(got)
    evaluation.save_evaluation(case["dataset"], case["predictions"], str(tmp_path), ("bbox",), torch.device(DEV), logger)
    assert sorted(os.listdir(str(tmp_path))) == ["coco_results.json", "lvis_results.json"]


def test_degenerate_file_scores_as_coco(case):
    """Every image's negatives are all the categories absent from it, nothing is not-exhaustive, no crowds, no ignore keys,
    at most 100 detections per category and 300 per image: no rule of the ten can tell the file from a COCO one."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    dataset = _dataset(tiny_lvis.write(case["folder"] / "degenerate.json", tiny_lvis.dataset_dict(degenerate=True)))
    lvis = coco_eval.evaluate_coco(dataset, case["predictions"], TYPES, DEV, rules="lvis")
    coco = coco_eval.evaluate_coco(dataset, case["predictions"], TYPES, DEV, rules="coco")
    for task in TYPES:
        for key in coco_eval.METRICS:
            print(task, key, lvis[task][key], coco[task][key])
            assert lvis[task][key] == coco[task][key], (task, key)
        for key in coco[task]:   # and the project's per-class and per-split keys with them
            assert lvis[task][key] == coco[task][key], (task, key)
    # on the federated file the two differ: the rules do something
    federated = coco_eval.evaluate_coco(case["dataset"], case["predictions"], ("bbox",), DEV, rules="lvis")["bbox"]
    assert federated["AP"] != coco_eval.evaluate_coco(case["dataset"], case["predictions"], ("bbox",), DEV)["bbox"]["AP"]


def test_a_file_that_is_not_federated_raises_naming_the_item(case):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    for key, where in (("neg_category_ids", "image 8"), ("not_exhaustive_category_ids", "image 8")):
        data = tiny_lvis.dataset_dict()
        for image in data["images"]:
            if image["id"] in (8, 21):
                del image[key]
        dataset = _dataset(tiny_lvis.write(case["folder"] / "missing.json", data))
        with pytest.raises(ValueError, match=f"{where} .*{key}"):
            coco_eval.evaluate_coco(dataset, case["predictions"], ("bbox",), DEV, rules="lvis")
        with pytest.raises(ValueError, match=where):
            coco_eval.evaluate_coco_sharded(dataset, dict(enumerate(case["predictions"])), ("bbox",), DEV, rules="lvis")
        assert "AP" in coco_eval.evaluate_coco(dataset, case["predictions"], ("bbox",), DEV)["bbox"]   # COCO rules do not read it
    data = tiny_lvis.dataset_dict()
    for cat in data["categories"]:
        if cat["id"] in (9, 23):
            del cat["frequency"]
    dataset = _dataset(tiny_lvis.write(case["folder"] / "missing.json", data))
    with pytest.raises(ValueError, match="category 9 .*frequency"):
        coco_eval.evaluate_coco(dataset, case["predictions"], ("bbox",), DEV, rules="lvis")
    with pytest.raises(ValueError, match="category 9"):
        coco_eval.evaluate_coco_results(dataset, {"bbox": []}, ("bbox",), DEV, rules="lvis")
    with pytest.raises(ValueError, match="rules"):
        coco_eval.evaluate_coco(case["dataset"], case["predictions"], ("bbox",), DEV, rules="federated")


def test_coco_rules_are_what_a_call_without_the_keyword_gives(case):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    dataset, predictions = case["dataset"], case["predictions"]
    plain = coco_eval.evaluate_coco(dataset, predictions, TYPES, DEV, recall=True)
    named = coco_eval.evaluate_coco(dataset, predictions, TYPES, DEV, recall=True, rules="coco")
    assert list(plain) == list(named) == list(TYPES)
    for task in TYPES:
        assert list(plain[task].items()) == list(named[task].items()), task
        assert list(plain[task])[:6] == list(coco_eval.METRICS) and "APr" not in plain[task] and "AR100" in plain[task]
    a, _ = coco_eval.match_tables(dataset, predictions, "segm", DEV)
    b, _ = coco_eval.match_tables(dataset, predictions, "segm", DEV, rules="coco")
    for key in TABLE_KEYS:
        assert a[key].dtype == b[key].dtype and a[key].tobytes() == b[key].tobytes(), key


def test_sharded_equals_unsharded(case):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    dataset, predictions = case["dataset"], case["predictions"]
    want = coco_eval.evaluate_coco(dataset, predictions, TYPES, DEV, recall=True, rules="lvis")
    local = dict(enumerate(predictions))
    got = coco_eval.evaluate_coco_sharded(dataset, local, TYPES, DEV, recall=True, rules="lvis")
    assert list(got) == list(TYPES)
    for task in TYPES:
        assert list(got[task].items()) == list(want[task].items()), task
    # the images split over two owner lists: the tables, merged as rank 0 merges them, are the unsharded tables
    options = coco_eval.ScoringOptions(rules="lvis")
    cat_ids, images = coco_eval._ground_truth(dataset, options)
    by_image = {dataset.id_to_img_map[i]: p for i, p in local.items()}
    for tasks in (("bbox",), ("segm", "boundary")):
        parts = {task: [] for task in tasks}
        for shard in (images[4:], images[:4]):
            dets = coco_eval._detection_rows(dataset, by_image, (cat_ids, shard), tasks[0] != "bbox", options)
            scored = coco_eval._score_rows(shard, dets, tasks, torch.device(DEV, 0), options)
            problems = [len(np.union1d(d["cats"], im["cats"])) for im, d in zip(shard, dets)]
            for task in tasks:
                scored[task]["image"] = np.repeat(np.asarray([im["id"] for im in shard], dtype=np.int64), problems)
                parts[task].append(scored[task])
        for task in tasks:
            merged = coco_eval.merge_shard_tables(parts[task])
            whole, _ = coco_eval.match_tables(dataset, predictions, task, DEV, rules="lvis")
            for key in TABLE_KEYS:
                assert np.array_equal(merged[key], whole[key]) and np.array_equal(merged[key], case["tables"][task][key]), (task, key)
            precision, recall = coco_eval.accumulate_lvis(merged, len(cat_ids))
            again = coco_eval.summarize_lvis(precision, case["names"], case["splits"], case["frequencies"], None, recall)
            for k, v in again.items():
                assert v == want[task][k], (task, k)
