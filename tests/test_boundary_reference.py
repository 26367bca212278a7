"""CPU: the Boundary AP restatement of tests/boundary_reference.py held to literals -- the dilation table of
include/ovis_hip.h, the iterative erosion against its closed form, hand-counted boundary rings -- and the host side of the
feature: ``boundary`` as an iou_type, and ``--boundary-ap`` on the three tools with its command-line errors."""
import importlib.util
import os

import numpy as np
import pytest

from tests import boundary_reference as bref
from tests import tiny_coco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"ovis_tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dilation_is_the_rounded_fiftieth_of_the_diagonal():
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    table = {(15, 20): 1, (45, 60): 2, (75, 100): 2, (70, 129): 3, (480, 640): 16, (800, 1333): 31, (1, 1): 1}
    for (h, w), d in table.items():
        assert bref.dilation(h, w) == d, (h, w)
        assert coco_eval.boundary_dilation(h, w) == d and coco_eval.boundary_dilation(w, h) == d, (h, w)
    # 75 x 100: 0.02 * 125 = 2.5 rounds half to EVEN
    assert bref.dilation(75, 100) == 2 and bref.dilation(105, 140) == 4 and coco_eval.boundary_dilation(105, 140) == 4
    assert coco_eval.boundary_dilation(480, 640, 0.01) == 8 and coco_eval.BOUNDARY_DILATION_RATIO == 0.02


@pytest.mark.parametrize("h,w,d,seed", [(9, 9, 1, 0), (12, 17, 2, 1), (20, 13, 3, 2), (7, 30, 1, 3), (5, 5, 2, 4), (4, 9, 2, 5),
                                        (1, 1, 1, 6)])
def test_iterated_3x3_erosion_is_the_closed_form(h, w, d, seed):
    rs = np.random.RandomState(seed)
    nearly_full = np.ones((h, w), dtype=bool)
    nearly_full.reshape(-1)[rs.choice(h * w, min(3, h * w), replace=False)] = False
    for mask in (rs.rand(h, w) < .5, rs.rand(h, w) < .9, nearly_full, np.ones((h, w), dtype=bool), np.zeros((h, w), dtype=bool)):
        assert np.array_equal(bref.erode(mask, d), bref.erode_closed_form(mask, d))


def test_hand_counted_boundaries():
    full = np.ones((9, 9), dtype=bool)
    ring = bref.boundary(full, 1)   # the image border counts as 0: the outer ring of the image
    assert ring.sum() == 32 and not ring[1:-1, 1:-1].any() and ring[0].all() and ring[:, 0].all()
    square = np.zeros((15, 20), dtype=bool)
    square[4:9, 6:11] = True
    b = bref.boundary(square, bref.dilation(15, 20))
    assert bref.dilation(15, 20) == 1 and b.sum() == 16 and not b[5:8, 7:10].any() and b[4, 6:11].all() and b[4:9, 10].all()
    clipped = np.zeros((15, 20), dtype=bool)   # a 6 x 5 block in the image's top left corner
    clipped[:6, :5] = True
    b = bref.boundary(clipped, 1)
    assert b[0, :5].all() and b[:6, 0].all() and b[5, :5].all() and b[:6, 4].all() and not b[1:5, 1:4].any()
    assert b.sum() == 6 * 5 - 4 * 3
    single = np.zeros((15, 20), dtype=bool)
    single[7, 3] = True
    assert np.array_equal(bref.boundary(single, 1), single) and np.array_equal(bref.boundary(single, 5), single)
    # deeper than the mask is wide: nothing survives, the boundary is the mask
    assert np.array_equal(bref.boundary(square, 3), square)
    assert bref.boundary(square, 2).sum() == 24   # only the centre pixel survives two iterations


def test_packing_and_min_iou():
    masks = np.zeros((2, 5, 30), dtype=bool)   # 150 pixels: 3 words, 42 bits of tail
    masks[0, 0, 0] = masks[0, 2, 4] = masks[0, 4, 29] = True
    masks[1] = True
    words = bref.pack(masks).view(np.uint64)
    # pixels 0, 2 * 30 + 4 = 64 and 4 * 30 + 29 = 149 = 2 * 64 + 21
    assert words.shape == (2, 3) and words[0].tolist() == [1, 1, 1 << 21]
    assert words[1].tolist() == [2 ** 64 - 1, 2 ** 64 - 1, 2 ** 22 - 1]
    # a thick 11 x 11 square against itself moved by one pixel: the boundary IoU is the smaller one
    a, b = np.zeros((15, 20), dtype=bool), np.zeros((15, 20), dtype=bool)
    a[2:13, 2:13] = True
    b[2:13, 3:14] = True
    assert bref.min_iou(a, a, 0, 1) == 1.0
    inter, union = 11 * 10, 11 * 12
    ring_inter, ring_union = 2 * 10 + 0, 2 * 40 - 2 * 10   # the rings share their top and bottom rows; the sides miss
    assert ring_inter / ring_union < inter / union
    assert bref.min_iou(a, b, 0, 1) == np.float64(ring_inter) / np.float64(ring_union)
    # one-pixel-wide structures are all boundary: the two IoUs coincide, and a crowd divides by the detection alone
    line, cross = np.zeros((15, 20), dtype=bool), np.zeros((15, 20), dtype=bool)
    line[7, 2:12] = True
    cross[7, 5:18] = True
    assert bref.min_iou(line, cross, 0, 1) == np.float64(7) / np.float64(16)
    assert bref.min_iou(line, cross, 1, 1) == np.float64(7) / np.float64(10)
    empty = np.zeros((15, 20), dtype=bool)
    assert bref.min_iou(empty, a, 0, 1) == 0 and bref.min_iou(empty, a, 1, 1) == 0 and bref.min_iou(a, empty, 0, 1) == 0
    # the mask IoU is the smaller one: a filled 7 x 7 square against its own one-pixel ring, which is the boundary of both
    ring = a & False
    ring[4:11, 4:11] = True
    filled = ring.copy()
    ring[5:10, 5:10] = False
    assert bref.min_iou(filled, ring, 0, 1) == np.float64(24) / np.float64(49)
    assert np.array_equal(bref.boundary(filled, 1), ring)


def test_boundary_is_an_iou_type_and_the_host_is_refused_as_for_segm(tmp_path):
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    assert coco_eval.IOU_TYPES == ("bbox", "segm", "boundary")
    with pytest.raises(ValueError) as host:
        coco_eval.evaluate_coco(None, [], ("boundary",), device="cpu")
    assert "scoring runs on the HIP device" in str(host.value) and "not supported" not in str(host.value)
    with pytest.raises(ValueError) as host:
        coco_eval.evaluate_coco_results(None, {"segm": []}, ("segm", "boundary"), "cpu")
    assert "scoring runs on the HIP device" in str(host.value)
    with pytest.raises(ValueError) as host:
        coco_eval.evaluate_coco_sharded(None, {}, ("boundary",), "cpu")
    assert "scoring runs on the HIP device" in str(host.value)
    dataset = coco_eval.annotation_dataset(tiny_coco.write(tmp_path)["instances"])
    for call in (lambda: coco_eval.match_tables(dataset, [], "keypoints", "cuda"),
                 lambda: coco_eval.results_match_tables(dataset, [], "keypoints", "cuda"),
                 lambda: coco_eval.load_coco_results(dataset, [], "keypoints")):
        with pytest.raises(ValueError) as unknown:
            call()
        assert "'keypoints' is not supported (bbox, segm, boundary)" in str(unknown.value)
    rle = {"size": [48, 64], "counts": [0, 10, 3062]}
    results = [{"image_id": 7, "category_id": 3, "score": .5, "segmentation": rle}]
    a, b = coco_eval.load_coco_results(dataset, results, "segm"), coco_eval.load_coco_results(dataset, results, "boundary")
    assert [r["rle"] for r in a] == [r["rle"] for r in b] and a[0]["rle"] == [rle]   # the same segm.json, the same rows
    assert coco_eval._jobs(("bbox", "segm", "boundary")) == ["bbox", ("segm", "boundary")]
    assert coco_eval._jobs(("boundary", "bbox")) == ["boundary", "bbox"] and coco_eval._jobs(("bbox", "segm")) == ["bbox", "segm"]


def test_a_chunk_plans_the_boundary_words_and_the_scratch():
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    image = {"height": 480, "width": 640, "cats": np.zeros(3, np.int64), "polygons": 3}
    det = {"cats": np.zeros(5, np.int64)}
    segm, both = 8 * 480 * 640 * 9 // 8, 8 * 480 * 640 * 11 // 8
    assert [len(c) for c in coco_eval._chunks([image] * 4, [det] * 4, True, 2 * segm)] == [2, 2]
    assert [len(c) for c in coco_eval._chunks([image] * 4, [det] * 4, True, 2 * segm, boundary=True)] == [1, 1, 1, 1]
    assert [len(c) for c in coco_eval._chunks([image] * 4, [det] * 4, True, 2 * both, boundary=True)] == [2, 2]


def test_boundary_ap_on_the_command_lines(tmp_path, capsys):
    catalog = ["--dataset-catalog", str(tmp_path / "none.json")]
    on = ["MODEL.DEVICE", "cuda", "OUTPUT_DIR", str(tmp_path), "MODEL.MASK_ON", "True"]
    off = ["MODEL.DEVICE", "cuda", "OUTPUT_DIR", str(tmp_path), "MODEL.MASK_ON", "False"]
    for tool in ("infer_net", "train_net"):
        for argv, word in ((["--boundary-ap"] + catalog + on, "--boundary-ap adds the boundary task to what --evaluate scores"),
                           (["--boundary-ap", "--evaluate"] + catalog + off, "--boundary-ap scores the mask head's masks: set "
                                                                             "MODEL.MASK_ON True")):
            with pytest.raises(SystemExit) as e:
                _tool(tool).main(argv)
            assert e.value.code == 2 and word in capsys.readouterr().err, (tool, argv)
    paths = tiny_coco.write(tmp_path / "data")
    (tmp_path / "boxes").mkdir()
    (tmp_path / "boxes" / "bbox.json").write_text("[]")
    (tmp_path / "masks").mkdir()
    (tmp_path / "masks" / "segm.json").write_text("[]")
    score = _tool("score_results")
    for argv, word in ((["--ann-file", paths["instances"], "--results-dir", str(tmp_path / "boxes"), "--boundary-ap"],
                        "--boundary-ap scores the masks of a segm results file"),
                       (["--ann-file", paths["instances"], "--bbox", str(tmp_path / "boxes" / "bbox.json"), "--boundary-ap"],
                        "--boundary-ap scores the masks of a segm results file"),
                       # with a segm file the flag parses: the next error is the device's, not the flag's
                       (["--ann-file", paths["instances"], "--results-dir", str(tmp_path / "masks"), "--boundary-ap", "--device",
                         "cpu"], "HIP device")):
        with pytest.raises(SystemExit) as e:
            score.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, argv


def test_scored_iou_types_put_boundary_behind_segm():
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import evaluation
    cfg = get_defaults()
    cfg.merge_from_list(["MODEL.MASK_ON", "True"])
    assert evaluation.scored_iou_types(cfg) == ("bbox", "segm")
    assert evaluation.scored_iou_types(cfg, True) == ("bbox", "segm", "boundary")
    cfg.merge_from_list(["MODEL.MASK_ON", "False"])
    assert evaluation.scored_iou_types(cfg) == ("bbox",)
    with pytest.raises(ValueError):
        evaluation.scored_iou_types(cfg, True)


def test_the_binding_reads_the_boundary_entries_from_the_header():
    import ctypes as C

    from cvpr22_cross_modal_pseudo_labeling_amd import _lib
    i, l, vp = C.c_int, C.c_long, C.c_void_p
    assert _lib.SIGNATURES["ovis_coco_boundary_words_u64"] == (i, [vp, i, i, i, i, vp, vp, vp, vp])
    assert _lib.SIGNATURES["ovis_coco_boundary_iou_f64"] == (i, [vp] * 10 + [i, l, vp, vp])
    text = open(os.path.join(ROOT, "include", "ovis_hip.h")).read()
    for phrase in ("min(mask_iou, boundary_iou)", "m & ~eroded(m)", "800x1333: 31", "half to even", "0x7fffffef"):
        assert phrase in text, phrase
