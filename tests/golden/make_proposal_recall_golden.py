"""Writes tests/golden/proposal_recall.npz: box-proposal recall as the REFERENCE computes it, recorded where the reference
is available (python tests/golden/make_proposal_recall_golden.py).

A seeded six-image scene goes through the reference's own ``evaluate_box_proposals``
(maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py:199-312, loaded as a file) with its own ``BoxList`` and
``boxlist_iou``, for the 2 limits x 4 area ranges of ``do_coco_evaluation`` (coco_eval.py:31-38).  Stand-ins, each only as
wide as the import statements need: empty ``cv2`` / ``pycocotools`` / ``tqdm`` modules, a ``maskrcnn_benchmark.layers`` with
an unused ``nms`` name (boxlist_ops.py:6), a ``Masker`` name (coco_eval.py:9), and a dataset object with ``coco.getAnnIds`` /
``coco.loadAnns``, ``id_to_img_map`` and ``get_img_info``.  Inputs and outputs are stored; only data is written.

The scene (asserted below before anything is written): image 0 has about 1000 proposals, image 1 only a crowd annotation,
image 2 ground truth and no proposal, image 3 more ground truths than proposals, image 4 predictions at a size whose two
ratios to the file's differ, image 5 is ordinary; crowd annotations are present; all objectness values are distinct; the
proposals are mostly jittered ground truths, with the good ones spread over the whole ranking."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import ref_import  # noqa: E402

SEED = 20240911
AREAS = ("all", "small", "medium", "large")
LIMITS = (100, 1000)
# (file width, file height, prediction width, prediction height, ground truths, crowds, proposals)
IMAGES = [(640, 480, 640, 480, 24, 2, 1000), (320, 240, 320, 240, 0, 1, 30), (300, 200, 300, 200, 6, 0, 0),
          (400, 300, 400, 300, 12, 1, 5), (500, 375, 803, 600, 9, 0, 60), (640, 427, 640, 427, 30, 1, 200)]
CATEGORIES = (1, 2, 3, 4)


def make_scene():
    """-> per image (boxes fp32 [P, 4] at the prediction's size, objectness fp32 [P], annotations)."""
    rs = np.random.RandomState(SEED)
    total = sum(im[6] for im in IMAGES)
    ranks = rs.permutation(total)  # one ranking over the whole scene: every objectness is distinct
    scene, used = [], 0
    for width, height, pw, ph, num_gt, num_crowd, num_props in IMAGES:
        anns = []
        for k in range(num_gt + num_crowd):
            side = [10.0, 24.0, 60.0, 80.0, 130.0, 200.0][k % 6] * (0.8 + 0.4 * rs.rand())
            w, h = side * (0.7 + 0.6 * rs.rand()), side * (0.7 + 0.6 * rs.rand())
            w, h = min(w, width - 2.0), min(h, height - 2.0)
            x, y = rs.rand() * (width - w - 1), rs.rand() * (height - h - 1)
            box = [round(float(v), 2) for v in (x, y, w, h)]
            anns.append({"bbox": box, "area": round(box[2] * box[3] * (0.55 + 0.4 * rs.rand()), 3),
                         "iscrowd": 1 if k >= num_gt else 0, "category_id": int(CATEGORIES[k % len(CATEGORIES)])})
        if num_gt >= 9:  # areas exactly on the two inner bounds: inside both adjoining ranges (coco_eval.py:258)
            anns[0]["area"], anns[1]["area"] = float(32 ** 2), float(96 ** 2)
        boxes = np.zeros((num_props, 4), dtype=np.float32)
        sx, sy = pw / width, ph / height
        for p in range(num_props):
            if num_gt and rs.rand() < 0.8:  # a jittered ground truth
                x, y, w, h = anns[rs.randint(num_gt)]["bbox"]
                j = rs.randn(4) * 0.09
                x1, y1 = x + j[0] * w, y + j[1] * h
                x2, y2 = x + w - 1 + j[2] * w, y + h - 1 + j[3] * h
            else:
                x1, y1 = rs.rand() * width * 0.8, rs.rand() * height * 0.8
                x2, y2 = x1 + rs.rand() * width * 0.3, y1 + rs.rand() * height * 0.3
            x1, x2 = np.clip(sorted((x1, x2)), 0, width - 1)
            y1, y2 = np.clip(sorted((y1, y2)), 0, height - 1)
            boxes[p] = [x1 * sx, y1 * sy, x2 * sx, y2 * sy]
        objectness = ((ranks[used:used + num_props] + 1) / float(total + 1)).astype(np.float32)
        used += num_props
        scene.append((boxes, objectness, anns))
    return scene


class _Coco:
    def __init__(self, anns_of):
        self.by_id = {}
        self.ids_of = {}
        for image_id, anns in anns_of.items():
            for a in anns:
                ann_id = len(self.by_id) + 1
                self.by_id[ann_id] = a
                self.ids_of.setdefault(image_id, []).append(ann_id)

    def getAnnIds(self, imgIds):
        return list(self.ids_of.get(imgIds, []))

    def loadAnns(self, ids):
        return [self.by_id[i] for i in ids]


class _Dataset:
    def __init__(self, scene):
        self.id_to_img_map = {k: 100 + 7 * k for k in range(len(scene))}
        self.coco = _Coco({self.id_to_img_map[k]: anns for k, (_, _, anns) in enumerate(scene)})

    def get_img_info(self, index):
        return {"width": IMAGES[index][0], "height": IMAGES[index][1]}


def load_reference():
    """The reference's coco_eval.py as a module, behind the stand-ins of this file's docstring."""
    for name in ("cv2", "pycocotools", "tqdm"):
        if name not in sys.modules:
            ref_import._empty(name, tqdm=lambda x, *a, **k: x)
    sys.path.insert(0, ref_import.REF)
    import maskrcnn_benchmark  # noqa: F401

    ref_import._empty("maskrcnn_benchmark.layers", nms=None)
    mb = os.path.join(ref_import.REF, "maskrcnn_benchmark")
    for name, path in (("maskrcnn_benchmark.modeling", "modeling"), ("maskrcnn_benchmark.modeling.roi_heads", "modeling/roi_heads"),
                       ("maskrcnn_benchmark.modeling.roi_heads.mask_head", "modeling/roi_heads/mask_head")):
        ref_import._namespace_pkg(name, os.path.join(mb, path))
    ref_import._empty("maskrcnn_benchmark.modeling.roi_heads.mask_head.inference", Masker=types.SimpleNamespace)
    return ref_import.load_file_as("ref_coco_eval", "maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py")


def main():
    ref = load_reference()
    from maskrcnn_benchmark.structures.bounding_box import BoxList

    scene = make_scene()
    dataset = _Dataset(scene)
    predictions = []
    for (boxes, objectness, _), im in zip(scene, IMAGES):
        pred = BoxList(torch.from_numpy(boxes).reshape(-1, 4), (im[2], im[3]), mode="xyxy")
        pred.add_field("objectness", torch.from_numpy(objectness))
        predictions.append(pred)

    every = np.concatenate([s[1] for s in scene])
    assert len(np.unique(every)) == len(every), "objectness values must be distinct"
    assert len(scene) == 6 and len(scene[0][0]) >= 1000
    non_crowd = [[a for a in s[2] if a["iscrowd"] == 0] for s in scene]
    assert not non_crowd[1] and len(scene[1][0]) > 0, "an image without ground truth"
    assert non_crowd[2] and len(scene[2][0]) == 0, "an image with ground truth and no proposal"
    assert len(non_crowd[3]) > len(scene[3][0]) > 0, "more ground truths than proposals"
    assert IMAGES[4][0] / IMAGES[4][2] != IMAGES[4][1] / IMAGES[4][3] and (IMAGES[4][0], IMAGES[4][1]) != (IMAGES[4][2], IMAGES[4][3])
    assert any(a["iscrowd"] == 1 for s in scene for a in s[2]), "crowd annotations"
    for s in scene:
        assert np.all(s[0][:, 2] >= s[0][:, 0]) and np.all(s[0][:, 3] >= s[0][:, 1])

    out = {"limits": np.asarray(LIMITS, dtype=np.int64), "areas": np.asarray(AREAS),
           "file_wh": np.asarray([[im[0], im[1]] for im in IMAGES], dtype=np.int64),
           "pred_wh": np.asarray([[im[2], im[3]] for im in IMAGES], dtype=np.int64),
           "prop_start": np.cumsum([0] + [len(s[0]) for s in scene]).astype(np.int64),
           "ann_start": np.cumsum([0] + [len(s[2]) for s in scene]).astype(np.int64),
           "boxes": np.concatenate([s[0] for s in scene]).astype(np.float32), "objectness": every.astype(np.float32),
           "ann_bbox": np.asarray([a["bbox"] for s in scene for a in s[2]], dtype=np.float64).reshape(-1, 4),
           "ann_area": np.asarray([a["area"] for s in scene for a in s[2]], dtype=np.float64),
           "ann_iscrowd": np.asarray([a["iscrowd"] for s in scene for a in s[2]], dtype=np.int64),
           "ann_category": np.asarray([a["category_id"] for s in scene for a in s[2]], dtype=np.int64)}
    ars = {}
    for limit in LIMITS:
        for area in AREAS:
            stats = ref.evaluate_box_proposals(predictions, dataset, area=area, limit=limit)
            assert stats["gt_overlaps"].dtype == torch.float32
            out[f"gt_overlaps_{area}_{limit}"] = stats["gt_overlaps"].numpy()
            out[f"num_pos_{area}_{limit}"] = np.asarray(stats["num_pos"], dtype=np.int64)
            out[f"ar_{area}_{limit}"] = np.asarray(stats["ar"].item(), dtype=np.float64)
            ars[(area, limit)] = stats["ar"].item()
            assert stats["num_pos"] >= 5, (area, limit, stats["num_pos"])
            print(f"limit {limit:4d} {area:6s}: AR {stats['ar'].item():.4f}  num_pos {stats['num_pos']}")
    assert 0.3 < ars[("all", 1000)] < 0.8, ars
    assert ars[("all", 100)] != ars[("all", 1000)], ars
    np.savez_compressed(os.path.join(HERE, "proposal_recall.npz"), **out)
    print("wrote", os.path.join(HERE, "proposal_recall.npz"))


if __name__ == "__main__":
    main()
