"""CPU: RLE (bitmap) ground truth through the reader, the host half of the input transform and the pseudo-label tool --
``RleMasks`` (modeling/structures.py) is built in the loader worker from the annotation's ``counts`` and carries the
resize, the flips and the instance selection as bookkeeping; nothing is decoded on the host."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import coco_rle_reference as rle_ref
from tests import tiny_coco, tiny_rle_coco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    paths = tiny_coco.write(tmp_path_factory.mktemp("tiny_rle_coco"))
    paths["instances_bitmap"] = tiny_rle_coco.write(paths)
    return paths


@pytest.fixture(scope="module")
def det(paths):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCODataset

    return COCODataset(paths["instances_bitmap"], paths["img_dir"], True)


def test_reader_yields_rle_masks_and_drops_crowds(paths, det):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCOCapDetDataset
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import PolygonMasks, RleMasks

    assert det.ids == [7, 12, 55, 90, 101]
    masks = tiny_rle_coco.bitmaps()
    t = det[0][1]  # image 7: annotation 3 (compressed) + the crowd annotation 4, which is dropped
    m = t.get_field("masks")
    assert isinstance(m, RleMasks) and len(m) == 1 and m.ann_ids == [3] and m.image_id == 7
    assert m.size == (64, 48) and m.source_hw == (48, 64) and not m.flip_h and not m.flip_v
    text = rle_ref.rle_to_string(rle_ref.rle_encode(masks[3]))
    assert bytes(m.chars.tolist()) == text and m.char_offsets.tolist() == [0, len(text)]
    assert m.run_offsets.tolist() == [0, len(rle_ref.rle_encode(masks[3]))]   # the values of the string, counted on the host
    assert m.sizes.tolist() == [[48, 64]] and m.sizes.dtype == torch.int32 and m.instance.tolist() == [0]
    t = det[1][1]  # image 12: annotation 7 (compressed), annotation 8 (a list; its box is empty once clipped) is indexed away
    m = t.get_field("masks")
    assert isinstance(m, RleMasks) and len(t) == 1 and len(m) == 1 and m.instance.tolist() == [0] and m.num_items == 2
    assert m.ann_ids == [7, 8] and m.char_offsets.tolist()[0] == 0 and m.char_offsets[1] == m.char_offsets[2]
    runs8 = rle_ref.rle_encode(masks[8])
    assert m.runs[m.run_offsets[1]:m.run_offsets[2]].tolist() == runs8 and m.runs.dtype == torch.int32
    t = det[3][1]  # image 90: annotation 9 (compressed)
    assert isinstance(t.get_field("masks"), RleMasks) and t.get_field("masks").source_hw == (40, 60)
    assert isinstance(det[4][1].get_field("masks"), PolygonMasks)  # image 101 keeps its polygons: kinds differ per image
    cap = COCOCapDetDataset(paths["instances_bitmap"], paths["captions"], paths["img_dir"], False, vocab_file=paths["vocab"])
    m = cap[1][1].get_field("masks")   # image 12 again: this dataset keeps the emptied box, and its (empty) mask
    assert isinstance(m, RleMasks) and len(m) == 2 and m.instance.tolist() == [0, 1]


def test_mixed_kinds_and_wrong_size_raise_naming_the_image(paths):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCODataset

    def mix(data):   # image 101: annotation 2 keeps its polygons, annotation 1 becomes RLE
        for a in data["annotations"]:
            if a["id"] == 1:
                a["segmentation"] = rle_ref.encode(np.ones((37, 53), dtype=bool))

    mixed = COCODataset(tiny_rle_coco.write(paths, "instances_mixed", mix), paths["img_dir"], True)
    with pytest.raises(ValueError, match=r"image 101\b.*annotation 2\b.*polygons"):
        mixed[4]
    assert mixed[0][1].has_field("masks")   # the other images of the file still load

    def transposed(data):   # annotation 9 with (width, height) for its size
        for a in data["annotations"]:
            if a["id"] == 9:
                a["segmentation"] = dict(a["segmentation"], size=[60, 40])

    wrong = COCODataset(tiny_rle_coco.write(paths, "instances_wrong_size", transposed), paths["img_dir"], True)
    with pytest.raises(ValueError, match=r"image 90\b.*annotation 9\b.*RLE.*\[60, 40\].*\[40, 60\]"):
        wrong[3]
    # the file tiny_coco itself writes: the RLE of another image's size on image 90
    with pytest.raises(ValueError, match=r"image 90\b.*RLE"):
        COCODataset(paths["instances_rle"], paths["img_dir"], True)[3]


def test_bookkeeping_resize_transpose_getitem():
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList, RleMasks

    masks = [np.random.default_rng(k).random((37, 50)) > 0.5 for k in range(4)]
    items = [rle_ref.rle_to_string(rle_ref.rle_encode(m)) if k % 2 else rle_ref.rle_encode(m) for k, m in enumerate(masks)]
    m = RleMasks(items, (37, 50), image_id=5, ann_ids=[11, 12, 13, 14])
    assert len(m) == 4 and m.size == (50, 37) and m.words is None and m.words_per_mask == (37 * 50 + 63) // 64
    assert m.names()[2] == "image 5: annotation 13"
    assert m.run_offsets.tolist() == np.cumsum([0] + [len(rle_ref.rle_encode(x)) for x in masks]).tolist()
    r = m.resize((40, 21))
    assert r.size == (40, 21) and m.size == (50, 37) and r.source_hw == (37, 50) and r.chars is m.chars
    assert r.resize((40, 21)).size == (40, 21)   # the same size again is no second resize
    with pytest.raises(NotImplementedError, match="second resize"):
        r.resize((80, 42))
    f = r.transpose(0)
    assert (f.flip_h, f.flip_v) == (True, False) and (r.flip_h, r.flip_v) == (False, False)
    f = f.transpose(1).transpose(0)
    assert (f.flip_h, f.flip_v) == (False, True) and f.size == (40, 21)
    with pytest.raises(NotImplementedError):
        m.transpose(2)
    with pytest.raises(NotImplementedError):
        m.transpose(0).resize((40, 21))   # the kernel's chain is resize, then flips
    # indexing: an int, a slice, an index tensor, a bool tensor -- the instance index only
    assert f[2].instance.tolist() == [2] and f[-1].instance.tolist() == [3] and f[1:3].instance.tolist() == [1, 2]
    assert f[torch.tensor([3, 0, 3])].instance.tolist() == [3, 0, 3]
    picked = f[torch.tensor([False, True, False, True])]
    assert picked.instance.tolist() == [1, 3] and len(picked) == 2 and picked.num_items == 4
    assert picked[torch.tensor([1])].instance.tolist() == [3] and picked.chars is m.chars and picked.flip_v
    assert len(f[torch.zeros(4, dtype=torch.bool)]) == 0
    # a BoxList takes its masks along
    b = BoxList(torch.tensor([[0., 0., 9., 9.]] * 4), (50, 37))
    b.add_field("masks", m)
    b.add_field("labels", torch.arange(4))
    sub = b[torch.tensor([True, False, True, False])].resize((100, 74)).transpose(0)
    sm = sub.get_field("masks")
    assert sm.instance.tolist() == [0, 2] and sm.size == (100, 74) and sm.flip_h and sub.get_field("labels").tolist() == [0, 2]
    assert all(t.device.type == "cpu" for t in sm.device_tensors()) and len(sm.device_tensors()) == 6
    with pytest.raises(NotImplementedError, match="MODEL.DEVICE cpu"):
        sm.decoded()
    with pytest.raises(ValueError, match="neither a string nor a sequence of integers"):
        RleMasks([[0.5, 2.0]], (1, 2))


def test_mask_loss_on_the_cpu_says_rle_is_not_supported():
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.roi_heads import MaskRCNNLossComputation
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList, RleMasks

    gt = BoxList(torch.tensor([[2., 2., 20., 20.]]), (50, 37))
    gt.add_field("labels", torch.tensor([1]))
    gt.add_field("masks", RleMasks([[0, 37 * 50]], (37, 50)))
    prop = BoxList(torch.tensor([[2., 2., 20., 21.]]), (50, 37))
    with pytest.raises(NotImplementedError, match="RLE ground-truth masks under MODEL.DEVICE cpu"):
        MaskRCNNLossComputation(get_defaults()).prepare_targets([prop], [gt])


def test_host_transform_and_collate_carry_the_masks(paths, det):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import TrainCollator
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import InputTransform
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import PolygonMasks, RleMasks

    tr = InputTransform((64, 96), 128, 1.0, 1.0, [0.0] * 3, [1.0] * 3, True, size_divisible=32)
    items = [det[0], det[3], det[4]]   # images 7, 90 (RLE) and 101 (polygons)
    raw, targets = tr.host([i[0] for i in items], [i[1] for i in items], rng=random.Random(3))
    for (_, before, _), after, (oh, ow) in zip(items, targets, raw["image_sizes"]):
        assert after.size == (ow, oh)
        m, m0 = after.get_field("masks"), before.get_field("masks")
        assert type(m) is type(m0) and m.size == (ow, oh)
        if isinstance(m, RleMasks):
            assert m.flip_h and m.flip_v and m.source_hw == m0.source_hw and m.chars is m0.chars and m.words is None
            assert not m0.flip_h and m0.size == before.size
    assert isinstance(targets[2].get_field("masks"), PolygonMasks)
    # the loader's collate function: RleMasks pass through it
    raw, targets = TrainCollator(tr, seed=1)([det[0] + (0,), det[3] + (0,)])
    assert all(isinstance(t.get_field("masks"), RleMasks) for t in targets) and raw["loader"]["indices"] == [0, 3]


def _results(paths):
    """bbox.json / segm.json of an export over the tiny dataset: four detections in one order."""
    rs = np.random.default_rng(0)
    rows = [(7, 3, 0.9, [10.0, 10.0, 30.0, 20.0]), (7, 8, 0.3, [1.0, 2.0, 5.0, 6.0]), (90, 44, 0.75, [1.5, 1.0, 50.0, 30.25]),
            (12, 17, 0.8, [2.0, 3.0, 10.0, 10.0])]
    size = {i: (h, w) for i, _, w, h, _ in tiny_coco.IMAGES}
    bbox = [{"image_id": i, "category_id": c, "bbox": b, "score": s} for i, c, s, b in rows]
    segm = [{"image_id": i, "category_id": c, "score": s, "segmentation": rle_ref.encode(rs.random(size[i]) > 0.5)}
            for i, c, s, _ in rows]
    out = os.path.join(paths["root"], "results")
    os.makedirs(out, exist_ok=True)
    for name, rows_ in (("bbox", bbox), ("segm", segm)):
        with open(os.path.join(out, name + ".json"), "w") as f:
            json.dump(rows_, f)
    return out, bbox, segm


def test_results_to_annotations_round_trip(paths, tmp_path):
    from cvpr22_cross_modal_pseudo_labeling_amd.data.datasets import COCODataset
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import RleMasks

    results_dir, bbox, segm = _results(paths)
    out = str(tmp_path / "pseudo.json")
    tool = os.path.join(ROOT, "tools", "results_to_annotations.py")
    r = subprocess.run([sys.executable, tool, "--ann-file", paths["instances"], "--results-dir", results_dir,
                        "--score-threshold", "0.75", "--output", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "3 of 4 detections kept" in r.stdout
    data, source = json.load(open(out)), json.load(open(paths["instances"]))
    assert data["images"] == source["images"] and data["categories"] == source["categories"]   # embeddings and splits included
    assert [a["id"] for a in data["annotations"]] == [1, 2, 3]
    a = data["annotations"][1]
    assert a == {"id": 2, "image_id": 90, "category_id": 44, "bbox": [1.5, 1.0, 50.0, 30.25], "segmentation": segm[2]["segmentation"],
                 "area": 50.0 * 30.25, "iscrowd": 0, "score": 0.75}
    d = COCODataset(out, paths["img_dir"], True)
    assert d.ids == [7, 12, 90]
    per_image = {d.ids[k]: d[k][1] for k in range(len(d))}
    assert [len(per_image[i]) for i in (7, 12, 90)] == [1, 1, 1]
    assert per_image[90].bbox.tolist() == [[1.5, 1.0, 50.5, 30.25]] and per_image[7].bbox.tolist() == [[10.0, 10.0, 39.0, 29.0]]
    m = per_image[90].get_field("masks")
    assert isinstance(m, RleMasks) and bytes(m.chars.tolist()).decode("ascii") == segm[2]["segmentation"]["counts"]
    # entries that are not one export: the tool names the index
    segm[2]["score"] = 0.5
    with open(os.path.join(results_dir, "segm.json"), "w") as f:
        json.dump(segm, f)
    r = subprocess.run([sys.executable, tool, "--ann-file", paths["instances"], "--results-dir", results_dir,
                        "--score-threshold", "0.75", "--output", out], capture_output=True, text=True)
    assert r.returncode != 0 and "entry 2" in r.stderr and "score" in r.stderr
