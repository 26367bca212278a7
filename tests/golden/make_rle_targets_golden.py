"""Writes tests/golden/rle_targets.npz: bitmap ground truth through the REFERENCE's own ``SegmentationMask(tensor, size,
mode='mask')`` -- ``.resize`` to the training size, ``.transpose`` for the flips, then per box ``.crop``, ``.resize((M, M))``
and ``.get_mask_tensor()`` (structures/segmentation_mask.py:33-158, what mask_head/loss.py:11-42 does per positive) --
recorded where the reference is available (python tests/golden/make_rle_targets_golden.py; oracle/_ref/ref_C.so built
first).  tests/golden/ref_import.py stubs pycocotools, so tensors are handed in, not RLE dicts.

Per case (a shape of tests/rle_targets_reference.py and a flip combination): the seeded salt-and-pepper source bitmap is NOT
stored (the test regenerates it); ``stage1_<k>`` is the reference's resized and flipped mask, bits packed; ``boxes_<k>`` the
boxes; ``stage2_<k>`` the reference's M x M targets, computed from that stage-1 output, bits packed.  Only data is written.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import ref_import  # noqa: E402
import rle_targets_reference as rt  # noqa: E402

M, BOXES = rt.GOLDEN_RESOLUTION, rt.GOLDEN_BOXES


def main():
    ref_import.install()
    from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask

    out = {"resolution": np.int64(M)}
    for k, (h0, w0), (h1, w1), flip_h, flip_v, mask_seed, box_seed in rt.golden_cases():
        source = rt.salt_and_pepper(1, h0, w0, mask_seed)
        seg = SegmentationMask(torch.from_numpy(source.astype(np.uint8)), (w0, h0), mode="mask")
        if (h1, w1) != (h0, w0):
            seg = seg.resize((w1, h1))
        if flip_h:
            seg = seg.transpose(0)
        if flip_v:
            seg = seg.transpose(1)
        stage1 = seg.get_mask_tensor()
        assert stage1.dtype == torch.uint8 and tuple(stage1.shape) == (h1, w1) and int(stage1.max()) <= 1
        boxes = rt.random_boxes(BOXES, w1, h1, box_seed)
        stage2 = torch.stack([seg.crop(b.tolist()).resize((M, M)).get_mask_tensor() for b in boxes])
        assert tuple(stage2.shape) == (BOXES, M, M) and int(stage2.max()) <= 1
        out[f"stage1_{k}"] = np.packbits(stage1.numpy().astype(bool))
        out[f"boxes_{k}"] = boxes
        out[f"stage2_{k}"] = np.packbits(stage2.numpy().astype(bool))
    path = os.path.join(HERE, "rle_targets.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
