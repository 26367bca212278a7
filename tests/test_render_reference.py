"""CPU: the prediction compositor's arithmetic.  tests/render_reference.py (a NumPy restatement) is held to what the
REFERENCE's own ``overlay_filled_mask`` / ``overlay_uncertainty_mask`` / ``Masker`` / ``compute_colors_for_labels`` produced
(tests/golden/render.npz, written by tests/golden/make_render_golden.py); the host route of ``_C.render_instances``
(``libovis_cpu.so``) is held to the restatement, byte for byte; then ``engine.visualize`` and ``tools/infer_net.py
--visualize`` on top.  The device kernel meets the same restatement in tests/test_render_gpu.py."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from cvpr22_cross_modal_pseudo_labeling_amd.engine import visualize
from tests import render_reference as R
from tests import tiny_coco

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YAML = os.path.join(ROOT, "configs/coco_cap_det/student_teacher_mask_rcnn_uncertainty.yaml")
HEAT_BGR = np.float32([0, 0, 255])


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "render.npz"))
    assert g["crc"].tolist() == [R.golden_crc(n) for n in sorted(R.GOLDEN_CASES)], "the seeded inputs drifted"
    return g


def _gains(scores):
    return np.float32([np.float32(0.2 / s) for s in scores.tolist()])


def _restated(name, golden):
    """(the reference's picture, the restatement's, the layer arguments) of one fixture case."""
    image, maps, boxes, scores, _ = R.golden_inputs(name)
    k = len(boxes)
    want = golden[name] ^ image
    if name.startswith("fill"):
        args = dict(maps=maps, boxes=boxes, colors=golden[name + "_colors"], kinds=np.zeros(k, np.int32), params=np.full(k, 0.5, np.float32))
    elif name.startswith("heat"):
        args = dict(maps=maps, boxes=boxes, colors=np.tile(HEAT_BGR, (k, 1)), kinds=np.ones(k, np.int32), params=_gains(scores))
    else:
        twice = np.repeat(np.arange(k), 2)
        colors = golden[name + "_colors"][twice].copy()
        colors[1::2] = HEAT_BGR
        params = np.full(2 * k, 0.5, np.float32)
        params[1::2] = _gains(scores)
        args = dict(maps=maps[twice], boxes=boxes[twice], colors=colors, kinds=np.tile(np.int32([0, 1]), k), params=params)
    return image, want, R.render(image, **args), args


@pytest.mark.parametrize("name", ["fill_a", "fill_b"])
def test_restated_fill_equals_the_reference(golden, name):
    image, want, got, _ = _restated(name, golden)
    assert not np.array_equal(want, image) and np.array_equal(got, want)


@pytest.mark.parametrize("name", ["heat_a", "heat_b", "combined"])
def test_restated_heat_is_within_one_grey_level_of_the_reference(golden, name):
    """torch's CPU bilinear kernel and the float32 expression of csrc/pasted_value.h differ in the last bit at a few
    percent of the pixels; that moves a truncation at ~2e-5 of them, by one: every byte within 1 grey level, and at most
    0.1 % of the PIXELS (a pixel differs when any of its channels does) differing."""
    image, want, got, _ = _restated(name, golden)
    diff = np.abs(got.astype(np.int16) - want.astype(np.int16))
    pixels = int((diff != 0).any(2).sum())
    print(name, "max difference", int(diff.max()), "differing pixels", pixels, "of", diff.shape[0] * diff.shape[1])
    assert not np.array_equal(want, image)
    assert diff.max() <= 1 and pixels <= 1e-3 * diff.shape[0] * diff.shape[1], (int(diff.max()), pixels)


def test_colors_for_labels_is_the_reference_formula(golden):
    got = visualize.colors_for_labels(torch.from_numpy(golden["labels"]))
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), golden["label_colors"])


def _host(image, outline_colors=None, alpha=0.5, outline_thickness=2, **a):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    t = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in a.items()}
    oc = None if outline_colors is None else torch.from_numpy(outline_colors)
    return _C.render_instances(torch.from_numpy(image), t["maps"], t["boxes"], t["colors"], t["kinds"], t["params"], alpha, oc,
                               outline_thickness).numpy()


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CASES))
def test_host_route_equals_the_restatement(golden, name):
    image, _, restated, args = _restated(name, golden)
    assert np.array_equal(_host(image, **args), restated)
    k = len(args["boxes"])
    outline = np.random.RandomState(3).randint(0, 256, (k, 3)).astype(np.uint8)
    for t in (1, 2, 3):
        want = R.render(image, outline_colors=outline, outline_thickness=t, **args)
        assert not np.array_equal(want, restated)
        assert np.array_equal(_host(image, outline_colors=outline, outline_thickness=t, **args), want), t


def test_host_route_defaults_empty_and_bad_arguments():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    image, maps, boxes, _, _ = R.golden_inputs("fill_b")
    colors = np.float32([[255, 0, 0], [0, 255, 0], [1, 2, 3]])
    t_img, t_maps, t_boxes, t_colors = (torch.from_numpy(v) for v in (image, maps, boxes, colors))
    assert np.array_equal(_C.render_instances(t_img, t_maps, t_boxes, t_colors).numpy(), R.render(image, maps, boxes, colors))
    assert np.array_equal(_C.render_instances(t_img, t_maps, t_boxes, t_colors, params=0.3, alpha=0.25).numpy(),
                          R.render(image, maps, boxes, colors, params=0.3, alpha=0.25))
    assert torch.equal(_C.render_instances(t_img, t_maps[:0], t_boxes[:0], t_colors[:0]), t_img)   # K = 0 copies the image
    skipped = _C.render_instances(t_img, t_maps, t_boxes, t_colors, kinds=torch.tensor([0, 7, 0], dtype=torch.int32)).numpy()
    assert np.array_equal(skipped, R.render(image, maps[[0, 2]], boxes[[0, 2]], colors[[0, 2]]))  # an unknown kind is skipped
    for bad in (dict(alpha=1.5), dict(alpha=-0.1), dict(outline_colors=torch.zeros(3, 3, dtype=torch.uint8), outline_thickness=0),
                dict(outline_colors=torch.zeros(3, 3, dtype=torch.uint8), outline_thickness=256)):
        with pytest.raises(RuntimeError, match="OVIS_EINVAL" if "alpha" in bad or bad["outline_thickness"] == 0 else "OVIS_ERANGE"):
            _C.render_instances(t_img, t_maps, t_boxes, t_colors, **bad)
    with pytest.raises(RuntimeError, match="OVIS_ERANGE"):
        _C.render_instances(t_img, torch.zeros(1, 121, 121), t_boxes[:1], t_colors[:1])
    # a fill never leaves its integer pasted box, whatever the sign of the threshold
    inside = R.pasted_values(maps[0], boxes[0], *image.shape[:2])[1]
    got = _C.render_instances(t_img, t_maps[:1], t_boxes[:1], t_colors[:1], params=-1.0).numpy()
    assert (got != image).any(2)[inside].all() and np.array_equal(got[~inside], image[~inside])
    for wrong in ((t_img.float(), t_maps, t_boxes, t_colors), (t_img, t_maps, t_boxes[:2], t_colors), (t_img, t_maps, t_boxes, t_colors[:, :2])):
        with pytest.raises(RuntimeError):
            _C.render_instances(*wrong)


def _boxlist(name, size=None):
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList
    image, maps, boxes, scores, labels = R.golden_inputs(name)
    h, w = image.shape[:2]
    b = BoxList(torch.from_numpy(boxes), (w, h))
    b.add_field("scores", torch.from_numpy(scores))
    b.add_field("labels", torch.from_numpy(labels))
    b.add_field("mask", torch.from_numpy(maps)[:, None])
    return image, b


def test_select_top_predictions_keeps_above_threshold_best_first():
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList
    b = BoxList(torch.arange(20, dtype=torch.float32).reshape(5, 4), (40, 30))
    b.add_field("scores", torch.tensor([0.5, 0.9, 0.2, 0.7, 0.51]))
    b.add_field("labels", torch.tensor([1, 2, 3, 4, 5]))
    top = visualize.select_top_predictions(b, 0.5)
    assert top.get_field("labels").tolist() == [2, 4, 5] and top.get_field("scores").tolist() == pytest.approx([0.9, 0.7, 0.51])
    assert torch.equal(top.bbox, b.bbox[[1, 3, 4]])
    assert len(visualize.select_top_predictions(b, 0.95)) == 0


def test_render_predictions_is_outlines_then_fills_in_score_order():
    image, b = _boxlist("fill_a")
    _, maps, boxes, scores, labels = R.golden_inputs("fill_a")
    half = b.resize((b.size[0] // 2 + 3, b.size[1] * 2))           # predictions live at the transformed size
    got = visualize.render_predictions(image, half, threshold=0.4, unseen_labels=[int(labels[1])])
    keep = [i for i in np.argsort(-scores, kind="stable") if scores[i] > 0.4]
    assert 2 <= len(keep)
    back = half.resize(b.size).bbox.numpy()[keep]
    colors = visualize.colors_for_labels(torch.from_numpy(labels[keep])).numpy()[:, ::-1].astype(np.float32)   # BGR tuples on an RGB image
    outline = np.uint8([[255, 0, 0] if labels[i] == labels[1] else [0, 0, 0] for i in keep])
    want = R.render(image, maps[keep], back, colors, outline_colors=outline, outline_thickness=2)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    named = visualize.render_predictions(image, half, [f"c{i}" for i in range(61)], threshold=0.4)
    assert named.shape == image.shape and not np.array_equal(named, visualize.render_predictions(image, half, threshold=0.4))
    # the combined view: each fill followed by its heat layer
    unc = torch.from_numpy(R.golden_inputs("combined")[1][:1].repeat(len(boxes), 0))[:, None] * 0.5
    got = visualize.render_predictions(image, b, threshold=0.4, uncertainty=unc, bgr=True)
    twice = np.repeat(keep, 2)
    m2, c2 = maps[twice].copy(), visualize.colors_for_labels(torch.from_numpy(labels[twice])).numpy().astype(np.float32)
    m2[1::2], c2[1::2] = unc[keep, 0].numpy(), HEAT_BGR
    p2 = np.full(len(twice), 0.5, np.float32)
    p2[1::2] = _gains(scores[keep])
    want = R.render(image, m2, boxes[twice], c2, kinds=np.tile(np.int32([0, 1]), len(keep)), params=p2,
                    outline_colors=np.zeros((len(twice), 3), np.uint8), outline_thickness=2)
    assert np.array_equal(got, want)


def test_render_predictions_refuses_pasted_masks():
    image, b = _boxlist("fill_b")
    b.add_field("mask", torch.zeros((len(b), 1) + image.shape[:2], dtype=torch.bool))
    with pytest.raises(ValueError, match="MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS"):
        visualize.render_predictions(image, b)


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"ovis_tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_infer_net_visualize_writes_the_rendered_originals(tmp_path):
    """``tools/infer_net.py --visualize 2`` on the tiny dataset, MODEL.DEVICE cpu: two PNGs at the ORIGINAL image sizes that
    equal ``render_predictions`` on the saved predictions; without the flag no ``vis/`` directory appears."""
    from PIL import Image

    from cvpr22_cross_modal_pseudo_labeling_amd.data.build import build_dataset
    from cvpr22_cross_modal_pseudo_labeling_amd.data.catalog import DatasetCatalog
    paths = tiny_coco.write(tmp_path / "data")
    name = "coco_not_zeroshot_val"
    argv = ["--config-file", YAML, "--dataset-catalog", paths["catalog"], "--data-dir", paths["root"]]
    opts = ["MODEL.DEVICE", "cpu", "DATALOADER.NUM_WORKERS", "0", "INPUT.MIN_SIZE_TEST", "80", "INPUT.MAX_SIZE_TEST", "128",
            "TEST.IMS_PER_BATCH", "2", "MODEL.RPN.PRE_NMS_TOP_N_TEST", "200", "MODEL.RPN.POST_NMS_TOP_N_TEST", "40",
            "DATASETS.TEST", f"('{name}',)"]
    plain, vis = str(tmp_path / "plain"), str(tmp_path / "vis")
    tool = _tool("infer_net")
    tool.main(argv + opts + ["OUTPUT_DIR", plain])
    assert os.path.isfile(os.path.join(plain, "inference", name, "predictions.pth"))
    assert not os.path.exists(os.path.join(plain, "inference", name, "vis"))
    tool.main(argv + ["--visualize", "2", "--vis-threshold", "0.0"] + opts + ["OUTPUT_DIR", vis])
    folder = os.path.join(vis, "inference", name, "vis")
    preds = torch.load(os.path.join(vis, "inference", name, "predictions.pth"), weights_only=False)
    cfg = tiny_coco.small_cfg(extra=["MODEL.DEVICE", "cpu"])
    dataset = build_dataset(cfg, name, DatasetCatalog(paths["catalog"], paths["root"]))
    files = {i: (f, w, h) for i, f, w, h, _ in tiny_coco.IMAGES}
    stems = [os.path.splitext(files[i][0])[0] for i in tiny_coco.IDS_WITH_VALID_ANNOTATION[:2]]
    assert sorted(os.listdir(folder)) == sorted(s + ".png" for s in stems)
    unseen = [dataset.json_category_id_to_contiguous_id[c] for c in dataset.class_splits.get("unseen", [])]
    drawn = 0
    for idx, image_id in enumerate(tiny_coco.IDS_WITH_VALID_ANNOTATION[:2]):
        _, w, h = files[image_id]
        got = np.asarray(Image.open(os.path.join(folder, stems[idx] + ".png")))
        original = dataset.original_image(idx)
        assert got.shape == (h, w, 3) and original.shape == (h, w, 3)
        assert np.array_equal(original, np.array(dataset._load(idx)[1]))   # the image the loader trains and tests on
        want = visualize.render_predictions(original, preds[idx], dataset.class_names, threshold=0.0, unseen_labels=unseen)
        assert np.array_equal(got, want)
        drawn += int(not np.array_equal(got, original))
    assert drawn or sum(len(p) for p in preds[:2]) == 0
