"""Writes tests/golden/input_transform.npz: what the REFERENCE's input transform computes, recorded where its libraries are
installed (python tests/golden/make_input_transform_golden.py).

  * ``pil_<i>``: ``PIL.Image.resize((out_w, out_h), BILINEAR)`` of case i of tests/input_transform_ref.py::CASES -- the
    call torchvision's ``F.resize`` makes for mb/data/transforms/transforms.py:57-62.  The uint8 INPUTS are not stored
    (300 x 200 x 3 random bytes alone are 180 KB): they are ``input_transform_ref.case_input(i)``, a frozen seeded stream,
    and ``crc`` holds the CRC-32 of each so that a drifted generator fails loudly.  ``pil_version`` names the PIL used.
  * ``box_*`` / ``poly_*``: ``BoxList.resize / transpose`` (mb/structures/bounding_box.py:91-166) and
    ``SegmentationMask(mode='poly').resize / transpose`` (mb/structures/segmentation_mask.py:250-325) of seeded boxes and
    polygons, for a size change with EQUAL ratios (600 x 400 -> 1200 x 800) and one with a ratio per axis (640 x 480 ->
    1066 x 800), by the reference's own classes through ref_import.py.  (Should they ever fail to import, the generator
    says so and stops: a restatement would prove nothing the tests' own arithmetic does not.)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import input_transform_ref as R  # noqa: E402

SIZE_CASES = {"equal": ((600, 400), (1200, 800)), "per_axis": ((640, 480), (1066, 800))}  # (width, height)


def geometry_inputs(size, seed):
    """Seeded float32 boxes [5, 4] xyxy and per box one or two polygons inside a (width, height) image."""
    g = torch.Generator().manual_seed(seed)
    w, h = size
    wh = torch.rand(5, 2, generator=g) * torch.tensor([w * 0.4, h * 0.4]) + 8
    xy = torch.rand(5, 2, generator=g) * (torch.tensor([float(w), float(h)]) - wh - 1)
    boxes = torch.cat([xy, xy + wh], 1)
    polys = []
    for i, (x0, y0, x1, y1) in enumerate(boxes.tolist()):
        n = 3 + i
        pts = torch.rand(n, 2, generator=g) * torch.tensor([x1 - x0, y1 - y0]) + torch.tensor([x0, y0])
        inst = [pts.reshape(-1).tolist()]
        if i % 2:
            inst.append((torch.rand(4, 2, generator=g) * torch.tensor([x1 - x0, y1 - y0]) + torch.tensor([x0, y0])).reshape(-1).tolist())
        polys.append(inst)
    return boxes, polys


def _flat(seg):
    return np.concatenate([p.numpy() for inst in seg.instances.polygons for p in inst.polygons]).astype(np.float32)


def main():
    from PIL import Image
    import PIL

    out = {"pil_version": np.array(PIL.__version__), "crc": np.array([R.crc(R.case_input(i)) for i in range(len(R.CASES))], dtype=np.int64)}
    for i, (_, _, oh, ow) in enumerate(R.CASES):
        out[f"pil_{i}"] = np.asarray(Image.fromarray(R.case_input(i)).resize((ow, oh), Image.BILINEAR))

    import ref_import
    ref_import.install()
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask

    for k, (name, (size, new_size)) in enumerate(sorted(SIZE_CASES.items())):
        boxes, polys = geometry_inputs(size, 77 + k)
        t = BoxList(boxes, size, mode="xyxy")
        t.add_field("masks", SegmentationMask(polys, size, mode="poly"))
        r = t.resize(new_size)
        out[f"box_{name}_resize"] = r.bbox.numpy()
        out[f"poly_{name}_resize"] = _flat(r.get_field("masks"))
        for method in (0, 1):
            f = r.transpose(method)
            out[f"box_{name}_flip{method}"] = f.bbox.numpy()
            out[f"poly_{name}_flip{method}"] = _flat(f.get_field("masks"))
    path = os.path.join(HERE, "input_transform.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
