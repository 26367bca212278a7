"""Writes tests/golden/render.npz: what the REFERENCE's own rendering functions make of the seeded cases of
tests/render_reference.py::GOLDEN_CASES (python tests/golden/make_render_golden.py, where /root/reference is present).

  * ``fill_*``: ``overlay_filled_mask`` (mb/engine/inference.py:557-569) over ``Masker(threshold=0.5, padding=1)``.  The
    function draws its colours from ``np.random``: it is seeded, and the colours it drew are recorded (``<case>_colors``).
  * ``heat_*``: ``overlay_uncertainty_mask`` (:571-589) over ``Masker(threshold=-1, padding=1)``, the un-thresholded paste.
  * ``combined``: the per-instance fill / heat sequence of ``visualization_uncertainty``'s combined view (:330-343).
  * ``labels`` / ``label_colors``: ``compute_colors_for_labels`` (:510-517).

The inputs are not stored (``render_reference.golden_inputs`` is a frozen seeded stream; ``crc`` holds the CRC-32 of each
case's image and maps); a result is stored XOR its input image, which is zero outside the boxes and compresses to a few KB.

The module is imported through ref_import.py; its cv2 stand-in lacks the font constants inference.py uses as default
arguments, and the module's dataset-evaluation and test-time-augmentation imports need torchvision: both are stubbed HERE.
Should the module fail to import, the generator stops and says so.  It re-checks, for the cases it writes, what
tests/test_render_reference.py asserts: the restatement's fills EQUAL the reference's (pick another seed if a tie at the
threshold splits torch's bilinear kernel and the float32 expression), its heat within 1 grey level at <= 0.1 % of the pixels.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import render_reference as R  # noqa: E402


def reference_module():
    import ref_import
    ref_import.install()
    import cv2
    cv2.FONT_HERSHEY_PLAIN, cv2.FONT_HERSHEY_SIMPLEX = 1, 0
    ref_import._empty("maskrcnn_benchmark.data.datasets.evaluation", evaluate=None)
    ref_import._empty("maskrcnn_benchmark.engine.bbox_aug", im_detect_bbox_aug=None)
    try:
        return ref_import.load_file_as("maskrcnn_benchmark.engine.inference", "maskrcnn_benchmark/engine/inference.py")
    except Exception as e:  # noqa: BLE001
        raise SystemExit(f"the reference's engine/inference.py cannot be imported here ({type(e).__name__}: {e}); "
                         "no fixture written -- a restatement would prove nothing")


def main():
    ref = reference_module()
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.inference import Masker
    from maskrcnn_benchmark.structures.bounding_box import BoxList

    def boxlist(name):
        image, maps, boxes, scores, labels = R.golden_inputs(name)
        h, w = image.shape[:2]
        b = BoxList(torch.from_numpy(boxes), (w, h), mode="xyxy")
        b.add_field("labels", torch.from_numpy(labels))
        b.add_field("scores", torch.from_numpy(scores))
        return image, torch.from_numpy(maps)[:, None], b

    out = {"crc": np.array([R.golden_crc(n) for n in sorted(R.GOLDEN_CASES)], dtype=np.int64)}
    for name in sorted(R.GOLDEN_CASES):
        image, masks, b = boxlist(name)
        _, maps, boxes, scores, _ = R.golden_inputs(name)
        h, w = image.shape[:2]
        k = len(b)
        gains = [np.float32(0.2 / s) for s in b.get_field("scores").tolist()]
        binary = Masker(threshold=0.5, padding=1)([masks], [b])[0]
        soft = Masker(threshold=-1, padding=1)([masks], [b])[0]
        for i in range(k):  # the restatement decides every fill as the reference does
            assert np.array_equal(R.paste_binary(maps[i], boxes[i], h, w), binary[i, 0].numpy()), (name, i, "pick another seed")
        seed = 1000 + R.GOLDEN_CASES[name][0]
        np.random.seed(seed)
        colors = np.stack([ref.random_color(rgb=True, maximum=255) for _ in range(k)]).astype(np.float32)
        np.random.seed(seed)
        if name.startswith("fill"):
            b.add_field("mask", binary)
            got = ref.overlay_filled_mask(image, b)
            mine = R.render(image, maps, boxes, colors)
            assert np.array_equal(mine, got), name
            out[name + "_colors"] = colors
        elif name.startswith("heat"):
            b.add_field("mask", soft)
            got = ref.overlay_uncertainty_mask(image, b)
            mine = R.render(image, maps, boxes, np.tile(np.float32([0, 0, 255]), (k, 1)), kinds=[R.HEAT] * k, params=gains)
        else:  # inference.py:330-343, one instance at a time: fill (one colour drawn per call), then heat
            got = image
            for i in range(k):
                one = b[[i]]
                one.add_field("mask", binary[i:i + 1])
                got = ref.overlay_filled_mask(got, one)
                one.add_field("mask", soft[i:i + 1])
                got = ref.overlay_uncertainty_mask(got, one)
            out[name + "_colors"] = colors
            inter = np.repeat(np.arange(k), 2)
            cols = colors[inter].copy()
            cols[1::2] = np.float32([0, 0, 255])
            params = np.float32([0.5, 0] * k)
            params[1::2] = gains
            mine = R.render(image, maps[inter], boxes[inter], cols, kinds=[R.FILL, R.HEAT] * k, params=params)
        assert got.dtype == np.uint8 and got.shape == image.shape and not np.array_equal(got, image)
        diff = np.abs(mine.astype(np.int16) - got.astype(np.int16))
        pixels = int((diff != 0).any(2).sum())
        print(name, "pixels differing from the restatement:", pixels, "of", h * w, "max", int(diff.max()))
        assert diff.max() <= 1 and pixels <= 1e-3 * h * w, name
        out[name] = got ^ image
    labels = torch.tensor([0, 1, 2, 3, 17, 44, 59, 80, 1203], dtype=torch.int64)
    out["labels"] = labels.numpy()
    out["label_colors"] = ref.compute_colors_for_labels(labels)
    path = os.path.join(HERE, "render.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
