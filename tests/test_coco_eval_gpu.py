"""GPU: COCO scoring on the device (csrc/coco_eval.hip, engine/coco_eval.py) against the scalar restatement of
tests/coco_eval_reference.py and dense NumPy: box IoU and packed-mask IoU exactly, the matching's positions and ignore flags
exactly on planted segments, every number of ``evaluate_coco`` on the tiny dataset within 1e-9, and
``tools/infer_net.py --evaluate``."""
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import coco_eval_reference as ref
from tests import tiny_coco

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs/coco_cap_det/student_teacher_mask_rcnn_uncertainty.yaml")
DEV = "cuda"
TABLE_KEYS = ("category", "det_start", "gt_start", "scores", "dt_match", "dt_ignore", "gt_ignore")


# ---- box IoU ----------------------------------------------------------------------------------------------------------------
def test_box_iou_is_the_fp64_formula():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    dets = np.array([[10, 10, 20, 20],                # identical to ground truth 0
                     [100, 100, 5, 5],                # disjoint from all
                     [30, 10, 10, 20],                # touches ground truth 0's right edge: iw = 0
                     [12, 12, 4, 4],                  # inside the crowd
                     [50, 50, 0, 0],                  # zero area, on the zero-area ground truth 3: union 0 -> 0
                     [10.25, 11.5, 19.75, 7.125]], dtype=np.float64)
    gts = np.array([[10, 10, 20, 20], [0, 0, 64, 48], [200, 200, 10, 10], [50, 50, 0, 0], [9.5, 10.75, 21.3, 18.9]],
                   dtype=np.float64)
    crowd = np.array([0, 1, 0, 0, 0], dtype=np.uint8)
    d, g = dets[:, None, :], gts[None, :, :]
    iw = np.maximum(np.minimum(d[..., 0] + d[..., 2], g[..., 0] + g[..., 2]) - np.maximum(d[..., 0], g[..., 0]), 0)
    ih = np.maximum(np.minimum(d[..., 1] + d[..., 3], g[..., 1] + g[..., 3]) - np.maximum(d[..., 1], g[..., 1]), 0)
    i = iw * ih
    u = np.where(crowd[None, :] != 0, d[..., 2] * d[..., 3], d[..., 2] * d[..., 3] + g[..., 2] * g[..., 3] - i)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(u == 0, 0.0, i / u)
    assert want[0, 0] == 1.0 and want[1].max() == 0 and want[2, 0] == 0 and want[3, 1] == 1.0 and want[4, 3] == 0 and u[4, 3] == 0
    assert 0 < want[5, 4] < 1 and 0 < want[5, 0] < 1
    for a in range(6):
        for b in range(5):
            assert ref.box_iou(dets[a], gts[b], crowd[b]) == want[a, b]
    got = _C.coco_box_iou(torch.from_numpy(dets).to(DEV), torch.from_numpy(gts).to(DEV), torch.from_numpy(crowd).to(DEV))
    assert got.dtype == torch.float64 and got.shape == (6, 5) and torch.equal(got.cpu(), torch.from_numpy(want))
    with pytest.raises(RuntimeError):
        _C.coco_box_iou(torch.from_numpy(dets), torch.from_numpy(gts), torch.from_numpy(crowd))


# ---- packing and mask IoU -----------------------------------------------------------------------------------------------------
def _masks(h, w, seed):
    rs = np.random.RandomState(seed)
    last = np.zeros((h, w), dtype=bool)
    last[-1, -1] = True
    return np.stack([np.zeros((h, w), dtype=bool), np.ones((h, w), dtype=bool), last, rs.rand(h, w) < .5, rs.rand(h, w) < .1,
                     rs.rand(h, w) < .9])


@pytest.mark.parametrize("h,w", [(37, 53), (64, 64)])   # 37 * 53 = 30 * 64 + 41: a ragged tail word
def test_pack_masks_and_mask_iou_equal_dense_numpy(h, w, monkeypatch):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    dets, gts = _masks(h, w, 1), _masks(h, w, 2)[[3, 1, 0, 2, 4]]
    crowd = np.array([0, 0, 0, 0, 1], dtype=np.uint8)
    nwords = (h * w + 63) // 64
    packed = {}
    for name, masks, as_bool in (("d", dets, True), ("g", gts, False)):   # bool as paste_masks, uint8 as polygons_to_masks
        t = torch.from_numpy(masks if as_bool else masks.astype(np.uint8)).to(DEV)
        words, areas = _C.coco_pack_masks(t)
        assert words.shape == (len(masks), nwords) and words.dtype == torch.int64 and areas.dtype == torch.int64
        assert areas.cpu().tolist() == masks.reshape(len(masks), -1).sum(1).tolist()
        padded = np.zeros((len(masks), nwords * 64), dtype=np.uint8)
        padded[:, :h * w] = masks.reshape(len(masks), -1)
        want_words = np.packbits(padded, axis=1, bitorder="little").view("<i8")   # pixel p = bit p % 64 of word p / 64
        assert np.array_equal(words.cpu().numpy(), want_words)
        packed[name] = (words, areas)
    want = np.array([[ref.mask_iou(d, g, c) for g, c in zip(gts, crowd)] for d in dets])
    assert want[1, 1] == 1.0 and want[0].max() == 0 and want[2, 3] == 1.0 and want[3, 4] == (dets[3] & gts[4]).sum() / dets[3].sum()
    got = _C.coco_mask_iou(*packed["d"], *packed["g"], torch.from_numpy(crowd).to(DEV))
    assert got.dtype == torch.float64 and torch.equal(got.cpu(), torch.from_numpy(want))

    def boom(*a):
        raise AssertionError("launched on an empty input")
    for entry in ("ovis_coco_pack_masks_u64", "ovis_coco_mask_iou_f64", "ovis_coco_box_iou_f64"):
        monkeypatch.setattr(_C._L, entry, boom)
    dw, da = packed["d"]
    gw, ga = packed["g"]
    assert _C.coco_mask_iou(dw[:0], da[:0], gw, ga, torch.from_numpy(crowd).to(DEV)).shape == (0, 5)
    assert _C.coco_mask_iou(dw, da, gw[:0], ga[:0], torch.zeros(0, dtype=torch.uint8, device=DEV)).shape == (6, 0)
    words, areas = _C.coco_pack_masks(torch.zeros((0, h, w), dtype=torch.bool, device=DEV))
    assert words.shape == (0, nwords) and areas.shape == (0,)
    assert _C.coco_box_iou(torch.zeros((0, 4), dtype=torch.float64, device=DEV), torch.zeros((3, 4), dtype=torch.float64, device=DEV),
                           torch.zeros(3, dtype=torch.uint8, device=DEV)).shape == (0, 3)


# ---- matching on planted segments ---------------------------------------------------------------------------------------------
def _planted():
    """{image id: (detections [(category id, score, xywh)] in prediction order, ground truths [(category id, xywh, area,
    iscrowd)] in annotation order)}; 200 x 200 images, categories 1, 2, 3."""
    grid = [[12 * (k % 10), 12 * (k // 10), 10, 10] for k in range(70)]
    grid[69] = grid[5]     # equal IoU in lanes' first and second slot: the later one (69) wins
    grid[64] = grid[3]
    many = [(2, 1 - k / 128, [100, 100 + (k % 50), 4, 4]) for k in range(102)] + [(2, .125, [0, 0, 10, 10])]
    return {
        1: ([(1, .9, [0, 0, 10, 5]), (1, .8, [100, 0, 10, 7.5]), (1, .7, [50, 50, 10, 10]),
             (2, .9, [0, 0, 20, 12.5]),
             (3, .9, [100, 100, 10, 10]), (3, .8, [120, 120, 10, 10]), (3, .7, [100, 100, 10, 10])],
            [(1, [0, 0, 10, 10], 100, 0), (1, [100, 0, 10, 10], 100, 0),       # IoU exactly .5 and .75
             (1, [50, 50, 10, 10], 100, 0), (1, [50, 50, 10, 10], 100, 0),     # equal IoU: the later wins
             (2, [0, 0, 20, 12.5], 250, 1), (2, [0, 0, 20, 20], 400, 0),       # ignored IoU 1 before non-ignored IoU .625
             (3, [100, 100, 50, 50], 2500, 1)]),                               # three detections on one crowd
        2: ([(1, .9, [0, 0, 20, 20]), (1, .8, [0, 0, 20, 20]),
             (2, .9, [0, 0, 32, 32]), (2, .8, [50, 50, 96, 96]),
             (3, .9, [150, 150, 40, 40])],
            [(1, [0, 0, 20, 20], 400, 0),                                      # ignored in medium / large, matched once
             (2, [0, 0, 32, 32], 1024, 0), (2, [50, 50, 96, 96], 9216, 0),      # on both sides of 32^2 and 96^2
             (3, [0, 0, 10, 10], 100, 0)]),                                    # unmatched detection of area 1600
        3: ([(1, .5, [0, 0, 10, 8.75]), (1, .5, [0, 0, 10, 10])] + many           # equal scores; 103 of category 2
            + [(3, .9, grid[k]) for k in (0, 5, 5, 3, 3, 63, 64, 65, 69, 68)],
            [(1, [0, 0, 10, 10], 100, 0), (2, [0, 0, 10, 10], 100, 0)]
            + [(3, grid[k], 100, 1 if k == 64 else 0) for k in range(70)]),    # 70 ground truths, one a crowd
        4: ([(1, .9, [5, 5, 10, 10])], [(2, [5, 5, 10, 10], 100, 0)]),         # detections without ground truth and the reverse
    }


def _planted_dataset(tmp_path):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCODataset
    planted = _planted()
    anns, k = [], 0
    for image_id, (_, gts) in planted.items():
        for cat, box, area, crowd in gts:
            k += 1
            anns.append({"id": k, "image_id": image_id, "category_id": cat, "bbox": box, "area": area, "iscrowd": crowd})
    path = str(tmp_path / "planted.json")
    with open(path, "w") as f:
        json.dump({"images": [{"id": i, "file_name": f"{i}.png", "width": 200, "height": 200} for i in planted],
                   "categories": [{"id": c, "name": f"c{c}"} for c in (1, 2, 3)], "annotations": anns}, f)
    return COCODataset(path, str(tmp_path), False)


def _planted_predictions(dataset):
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList
    preds = []
    for image_id in dataset.ids:
        dets = _planted()[image_id][0]
        xywh = torch.tensor([d[2] for d in dets], dtype=torch.float32)
        pred = BoxList(torch.cat((xywh[:, :2], xywh[:, :2] + xywh[:, 2:] - 1), 1), (200, 200))
        pred.add_field("scores", torch.tensor([d[1] for d in dets], dtype=torch.float32))
        pred.add_field("labels", torch.tensor([dataset.json_category_id_to_contiguous_id[d[0]] for d in dets]))
        preds.append(pred)
    return preds


def _restatement_images(dataset, predictions, masks=None):
    """The restatement's input: the prepared detections (the float32 xywh of coco_eval.py:82-85 at the file's image size,
    widened) and every annotation; category = index into the sorted category ids.  masks: (per image detection masks,
    per image ground-truth masks) for segm."""
    cats = {c: i for i, c in enumerate(sorted(dataset.coco.cats))}
    by_id = {dataset.id_to_img_map[i]: (i, p) for i, p in enumerate(predictions)}
    images = []
    for image_id in sorted(dataset.coco.imgs):
        info = dataset.coco.imgs[image_id]
        dets = []
        if image_id in by_id:
            idx, p = by_id[image_id]
            box = p.bbox * torch.tensor([info["width"] / p.size[0], info["height"] / p.size[1]] * 2, dtype=torch.float32)
            xywh = torch.stack((box[:, 0], box[:, 1], box[:, 2] - box[:, 0] + 1, box[:, 3] - box[:, 1] + 1), 1).double().tolist()
            for k in range(len(p)):
                det = {"category": cats[dataset.contiguous_category_id_to_json_id[int(p.get_field("labels")[k])]],
                       "score": float(p.get_field("scores")[k].double()), "bbox": xywh[k]}
                if masks is not None:
                    det["mask"] = masks[0][image_id][k]
                dets.append(det)
        gts = []
        for k, a in enumerate(dataset.coco.anns(image_id)):
            gt = {"category": cats[a["category_id"]], "bbox": a["bbox"], "area": a["area"], "iscrowd": a["iscrowd"]}
            if masks is not None:
                gt["mask"] = masks[1][image_id][k]
            gts.append(gt)
        images.append({"dets": dets, "gts": gts})
    return images


def _count_chunks(monkeypatch):
    """-> a list that receives the number of images of every chunk ``score_chunk`` is called with from now on."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    sizes, real = [], coco_eval.score_chunk
    monkeypatch.setattr(coco_eval, "score_chunk", lambda images, *a, **k: sizes.append(len(images)) or real(images, *a, **k))
    return sizes


def test_matching_equals_the_restatement_on_planted_segments(tmp_path, monkeypatch):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    dataset = _planted_dataset(tmp_path)
    predictions = _planted_predictions(dataset)
    want = ref.match_tables(_restatement_images(dataset, predictions), "bbox")
    # the planted cases are what they claim to be (problems: image 1 c1 c2 c3, image 2 c1 c2 c3, image 3 c1 c2 c3, image 4 c1 c2)
    assert want["category"].tolist() == [0, 1, 2] * 3 + [0, 1]
    ds, m = want["det_start"].tolist(), want["dt_match"][0]
    assert m[:, 0].tolist() == [0] + [-1] * 9 and m[:, 1].tolist() == [1] * 6 + [-1] * 4 and m[:, 2].tolist() == [3] * 10
    assert m[:, ds[1]].tolist() == [1, 1, 1] + [0] * 7 and want["dt_ignore"][0][:, ds[1]].tolist() == [False] * 3 + [True] * 7
    assert (m[:, ds[2]:ds[3]] == 0).all() and want["dt_ignore"][0][:, ds[2]:ds[3]].all()
    assert want["dt_match"][2][:, ds[3]:ds[4]].tolist() == [[0, -1]] * 10 and want["dt_ignore"][2][:, ds[3]:ds[4]].all()
    gs = want["gt_start"].tolist()
    assert want["gt_ignore"][:, gs[4]:gs[5]].tolist() == [[False, False], [False, True], [False, False], [True, False]]
    assert want["dt_ignore"][:, 0, ds[5]].tolist() == [False, True, False, True] and (want["dt_match"][:, :, ds[5]] == -1).all()
    assert m[:, ds[6]:ds[7]].tolist() == [[0, -1]] * 8 + [[-1, 0]] * 2              # [0, 0, 10, 8.75] (IoU .875) was predicted first
    assert ds[8] - ds[7] == 100 and (m[:, ds[7]:ds[8]] == -1).all()                # the overlapping one was number 103
    assert gs[9] - gs[8] == 70 and m[0, ds[8]:ds[9]].tolist() == [0, 69, 5, 3, 64, 63, 64, 65, -1, 68]
    assert ds[10] - ds[9] == 1 and gs[10] == gs[9] and ds[11] == ds[10] and gs[11] - gs[10] == 1

    got, cat_ids = coco_eval.match_tables(dataset, predictions, "bbox", DEV)
    assert cat_ids == [1, 2, 3]
    for key in TABLE_KEYS:
        assert np.array_equal(got[key], want[key]), key
    # the same problems in chunks of one image: the tables do not depend on the chunking.  Image 4 alone is a chunk with a
    # detection and a ground truth but no pair of them: its IoU buffer is empty
    sizes = _count_chunks(monkeypatch)
    again, _ = coco_eval.match_tables(dataset, predictions, "bbox", DEV, max_images=1)
    assert sizes == [1, 1, 1, 1]
    for key in TABLE_KEYS:
        assert np.array_equal(again[key], want[key]), key
    del sizes[:]
    again, _ = coco_eval.match_tables(dataset, predictions, "bbox", DEV, max_images=3)
    assert sizes == [3, 1]
    for key in TABLE_KEYS:
        assert np.array_equal(again[key], want[key]), key


# ---- end to end on the tiny dataset -------------------------------------------------------------------------------------------
M = 14
SEED = 3
SCALE = 2   # the predictions live at twice the file's image sizes
TINY_DETECTIONS = {   # image id -> [(json category id, score, xyxy at the FILE's scale)]
    7: [(8, .9, [10, 10, 39, 29]), (3, .8, [0, 0, 3, 12]), (8, .7, [12, 8, 45, 33]), (17, .6, [5, 5, 30, 30])],
    12: [(8, .75, [2, 3, 11, 12]), (17, .5, [20, 5, 40, 25])],
    20: [(3, .9, [5, 5, 30, 40])],                                   # an image without annotations
    55: [(44, .85, [40, 35, 59, 64]), (44, .4, [38, 30, 49, 49])],     # the box that leaves the image
    90: [(44, .95, [1, 1, 50, 30]), (44, .5, [1, 1, 50, 30]), (3, .3, [10, 10, 30, 30])],
    101: [(17, .9, [30, 10, 42, 29]), (3, .8, [5, 6, 24, 20]), (3, .85, [30, 20, 50, 35]), (17, .2, [31, 11, 41, 28])],
}   # image 31 gets an empty prediction


def _tiny(tmp_path_factory):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCODataset
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList
    paths = tiny_coco.write(tmp_path_factory.mktemp("tiny_coco_eval"))
    dataset = COCODataset(paths["instances"], paths["img_dir"], False, {"LOAD_EMBEDDINGS": True, "EMB_KEY": "Tiny", "EMB_DIM": 4})
    assert dataset.ids == tiny_coco.SORTED_IDS and dataset.class_splits == {"seen": [17, 3, 8], "unseen": [44]}
    g = torch.Generator().manual_seed(SEED)
    predictions = []
    for image_id in dataset.ids:
        info = dataset.coco.imgs[image_id]
        dets = TINY_DETECTIONS.get(image_id, [])
        pred = BoxList(torch.tensor([d[2] for d in dets], dtype=torch.float32).reshape(-1, 4) * SCALE,
                       (info["width"] * SCALE, info["height"] * SCALE))
        pred.add_field("scores", torch.tensor([d[1] for d in dets], dtype=torch.float32))
        pred.add_field("labels", torch.tensor([dataset.json_category_id_to_contiguous_id[d[0]] for d in dets], dtype=torch.int64))
        pred.add_field("mask", torch.rand(len(dets), 1, M, M, generator=g))
        predictions.append(pred)
    return dataset, predictions


@pytest.fixture(scope="module")
def tiny(tmp_path_factory):
    return _tiny(tmp_path_factory)


def _host_masks(dataset, predictions, threshold=0.5):
    """({image id: detection masks}, {image id: ground-truth masks}) made on the HOST: ``paste_mask_in_image`` and
    ``_cpu.polygons_to_masks``; an RLE ground truth is decoded here."""
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.roi_heads import paste_mask_in_image
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import PolygonMasks
    det_masks, gt_masks = {}, {}
    for idx, pred in enumerate(predictions):
        image_id = dataset.id_to_img_map[idx]
        info = dataset.coco.imgs[image_id]
        h, w = info["height"], info["width"]
        boxes = pred.bbox * torch.tensor([w / pred.size[0], h / pred.size[1]] * 2, dtype=torch.float32)
        det_masks[image_id] = [paste_mask_in_image(m[0], b, h, w, threshold, 1).numpy() for m, b in zip(pred.get_field("mask"), boxes)]
        gt_masks[image_id] = []
        for a in dataset.coco.anns(image_id):
            seg = a["segmentation"]
            if isinstance(seg, dict):
                runs = np.asarray(seg["counts"])
                gt_masks[image_id].append(np.repeat(np.arange(len(runs)) % 2, runs).reshape(w, h).T.astype(bool))
            else:
                gt_masks[image_id].append(PolygonMasks([seg], (w, h)).convert_to_binarymask()[0].numpy().astype(bool))
    return det_masks, gt_masks


def test_evaluate_coco_equals_the_restatement_on_the_tiny_dataset(tiny, monkeypatch):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    dataset, predictions = tiny
    masks = _host_masks(dataset, predictions)
    below, above = _host_masks(dataset, predictions, 0.5 - 2e-6)[0], _host_masks(dataset, predictions, 0.5 + 2e-6)[0]
    for image_id in below:   # no host-pasted pixel within 2e-6 of the threshold: the device paste must give the same masks
        for lo, hi in zip(below[image_id], above[image_id]):
            assert np.array_equal(lo, hi), image_id
    assert masks[1][7][1].sum() == 10 and masks[1][7][1][:10, 0].all()     # the RLE crowd of image 7
    assert sum(int(m.sum()) for m in masks[0][55]) > 0
    cat_ids = sorted(dataset.coco.cats)
    names = [dataset.categories[c] for c in cat_ids]
    in_file_order = [name for _, name, _ in tiny_coco.CATEGORIES]   # COCOResults.update iterates dataset.categories
    assert in_file_order != names and list(dataset.categories.values()) == in_file_order
    splits = {s: [cat_ids.index(c) for c in ids] for s, ids in dataset.class_splits.items()}
    got = coco_eval.evaluate_coco(dataset, predictions, ("bbox", "segm"), DEV)
    assert list(got) == ["bbox", "segm"]
    for iou_type in ("bbox", "segm"):
        images = _restatement_images(dataset, predictions, masks if iou_type == "segm" else None)
        tables = ref.match_tables(images, iou_type)
        want = ref.summarize(ref.accumulate(tables, len(names)), names, splits)
        assert list(got[iou_type]) == list(coco_eval.METRICS) + [f"AP50_class_{n}" for n in in_file_order] \
            + ["AP50_split_seen", "AP50_split_unseen"] and sorted(got[iou_type]) == sorted(want)
        for k in want:
            assert abs(got[iou_type][k] - want[k]) <= 1e-9, (iou_type, k, got[iou_type][k], want[k])
        device_tables, _ = coco_eval.match_tables(dataset, predictions, iou_type, DEV)
        for key in TABLE_KEYS:
            assert np.array_equal(device_tables[key], tables[key]), (iou_type, key)
        assert 0 < want["AP"] < 1 and want["AP50_split_unseen"] > 0   # the case is not degenerate
    # segm in several chunks, each with its own paste / rasterise / pack calls: a byte budget of one 64 x 48 image with
    # six masks, then a limit of four masks per call; an image always fits a chunk of its own
    segm = ref.match_tables(_restatement_images(dataset, predictions, masks), "segm")
    sizes = _count_chunks(monkeypatch)
    chunked, _ = coco_eval.match_tables(dataset, predictions, "segm", DEV, budget=6 * 64 * 48 * 9 // 8)
    assert len(sizes) > 2 and sum(sizes) == 7 and max(sizes) > 1
    for key in TABLE_KEYS:
        assert np.array_equal(chunked[key], segm[key]), key
    del sizes[:]
    monkeypatch.setattr(coco_eval, "MAX_CALL_MASKS", 4)
    chunked, _ = coco_eval.match_tables(dataset, predictions, "segm", DEV)
    assert len(sizes) > 2 and sum(sizes) == 7 and max(sizes) > 1
    for key in TABLE_KEYS:
        assert np.array_equal(chunked[key], segm[key]), key
    with pytest.raises(ValueError):   # masks already at image size cannot be scored
        bad = predictions[0].copy_with_fields(["scores", "labels"])
        bad.add_field("mask", torch.zeros(len(bad), 1, 48 * SCALE, 64 * SCALE))
        coco_eval.evaluate_coco(dataset, [bad] + predictions[1:], ("segm",), DEV)


# ---- command line ---------------------------------------------------------------------------------------------------------------
def _tool(name):
    spec = importlib.util.spec_from_file_location(f"ovis_tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_infer_net_evaluate_writes_coco_results(tmp_path):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    paths = tiny_coco.write(tmp_path / "data")
    name = "coco_zeroshot_val"
    argv = ["--config-file", YAML, "--dataset-catalog", paths["catalog"], "--data-dir", paths["root"]]
    opts = ["DATALOADER.NUM_WORKERS", "0", "INPUT.MIN_SIZE_TEST", "80", "INPUT.MAX_SIZE_TEST", "128", "TEST.IMS_PER_BATCH", "2",
            "MODEL.RPN.PRE_NMS_TOP_N_TEST", "200", "MODEL.RPN.POST_NMS_TOP_N_TEST", "40", "DATASETS.TEST", f"('{name}',)"]
    plain, scored = str(tmp_path / "plain"), str(tmp_path / "scored")
    tool = _tool("infer_net")
    torch.manual_seed(11)
    tool.main(argv + opts + ["OUTPUT_DIR", plain])
    torch.manual_seed(11)
    tool.main(argv + ["--evaluate"] + opts + ["OUTPUT_DIR", scored])
    assert not os.path.exists(os.path.join(plain, "inference", name, "coco_results.json"))
    a = torch.load(os.path.join(plain, "inference", name, "predictions.pth"), weights_only=False)
    b = torch.load(os.path.join(scored, "inference", name, "predictions.pth"), weights_only=False)
    assert len(a) == len(b) == len(tiny_coco.IDS_WITH_VALID_ANNOTATION)
    for x, y in zip(a, b):   # --evaluate changes nothing that is saved
        assert x.size == y.size and torch.equal(x.bbox, y.bbox) and sorted(x.fields()) == sorted(y.fields())
        for f in x.fields():
            assert torch.equal(x.get_field(f), y.get_field(f)), f
    with open(os.path.join(scored, "inference", name, "coco_results.json")) as f:
        results = json.load(f)
    names = [n for _, n, _ in sorted(tiny_coco.CATEGORIES)]
    keys = list(coco_eval.METRICS) + [f"AP50_class_{n}" for n in names] + ["AP50_split_seen", "AP50_split_unseen"]
    assert sorted(results) == ["bbox", "segm"]
    for iou_type in ("bbox", "segm"):
        assert sorted(results[iou_type]) == sorted(keys)
        for k, v in results[iou_type].items():
            assert v == -1 or 0 <= v <= 1, (iou_type, k, v)
