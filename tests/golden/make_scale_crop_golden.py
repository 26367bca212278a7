"""Writes tests/golden/scale_crop.npz: ground truth through the REFERENCE's own crops -- ``BoxList.crop`` followed by
``clip_to_image(remove_empty=True)`` (structures/bounding_box.py:167-193, 214-225), ``PolygonInstance.crop`` and
``BinaryMaskList.crop`` (structures/segmentation_mask.py:273-299, 118-136) -- recorded where the reference is available
(python tests/golden/make_scale_crop_golden.py; oracle/_ref/ref_C.so built first).

The boxes, windows, polygons and seeded bitmaps are those of tests/scale_crop_reference.py and are NOT stored.  Per window k:
``boxes_<k>`` the cropped boxes and ``box_size_<k>``; ``kept_<k>`` the indices clip_to_image keeps and ``clipped_<k>`` their
boxes; ``poly_<k>_<g>_<q>`` polygon q of instance g cropped, ``poly_size_<k>``; ``mask_<k>`` the cropped bitmaps, bits packed,
``mask_size_<k>``.  Only data is written.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_import  # noqa: E402
from tests import scale_crop_reference as sc  # noqa: E402


def main():
    ref_import.install()
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.segmentation_mask import BinaryMaskList, PolygonInstance

    out = {}
    bitmaps = torch.from_numpy(sc.golden_masks().astype(np.uint8))
    for k, window in enumerate(sc.GOLDEN_WINDOWS):
        boxes = BoxList(torch.from_numpy(sc.GOLDEN_BOXES.copy()), sc.FRAME, mode="xyxy")
        boxes.add_field("index", torch.arange(len(sc.GOLDEN_BOXES)))
        cropped = boxes.crop(window)
        out[f"boxes_{k}"] = cropped.bbox.numpy().copy()
        out[f"box_size_{k}"] = np.asarray(cropped.size, dtype=np.float64)
        clipped = cropped.clip_to_image(remove_empty=True)
        out[f"kept_{k}"] = clipped.get_field("index").numpy().copy()
        out[f"clipped_{k}"] = clipped.bbox.numpy().copy()
        for g, polys in enumerate(sc.GOLDEN_POLYGONS):
            inst = PolygonInstance(polys, sc.FRAME).crop(window)
            for q, p in enumerate(inst.polygons):
                assert p.dtype == torch.float32
                out[f"poly_{k}_{g}_{q}"] = p.numpy().copy()
            size = np.asarray(inst.size, dtype=np.float64)
            assert f"poly_size_{k}" not in out or np.array_equal(out[f"poly_size_{k}"], size)
            out[f"poly_size_{k}"] = size
        masks = BinaryMaskList(bitmaps, sc.FRAME).crop(window)
        assert tuple(masks.masks.shape[1:]) == (masks.size[1], masks.size[0])
        out[f"mask_{k}"] = np.packbits(masks.masks.numpy().astype(bool))
        out[f"mask_size_{k}"] = np.asarray(masks.size, dtype=np.int64)
    path = os.path.join(HERE, "scale_crop.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
