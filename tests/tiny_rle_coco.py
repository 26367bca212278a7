"""TEST-ONLY: the dataset of tests/tiny_coco.py with BITMAP ground truth.  ``write`` adds ``instances_bitmap.json`` beside
the files ``tiny_coco.write`` made: every non-crowd annotation of every image but 101 carries the RLE of a seeded bitmap --
its box filled, with salt-and-pepper holes, clipped to the image -- compressed for odd annotation ids, as the uncompressed
list for even ones; image 101 keeps its polygons (different images of one file may use different kinds).  Encodings come
from tests/coco_rle_reference.py."""
import json
import os

import numpy as np

from tests import coco_rle_reference as rle_ref
from tests import tiny_coco

POLYGON_IMAGE = 101


def bitmap(ann_id, box, width, height):
    """bool [height, width]: the xywh box filled (clipped to the image), about a third of it knocked out."""
    x, y, w, h = box
    m = np.zeros((height, width), dtype=bool)
    x0, y0, x1, y1 = int(np.floor(x)), int(np.floor(y)), int(np.ceil(x + w)), int(np.ceil(y + h))
    m[max(y0, 0):max(min(y1, height), 0), max(x0, 0):max(min(x1, width), 0)] = True
    return m & (np.random.default_rng(ann_id).random((height, width)) > 0.3)


def bitmaps():
    """{annotation id: bool [h, w]} of the non-crowd annotations that become RLE."""
    size = {i: (w, h) for i, _, w, h, _ in tiny_coco.IMAGES}
    return {a: bitmap(a, box, *size[i]) for a, i, _, box, _, crowd in tiny_coco.ANNOTATIONS if not crowd and i != POLYGON_IMAGE}


def segmentation(ann_id, mask):
    counts = rle_ref.rle_encode(mask)
    return {"size": [int(mask.shape[0]), int(mask.shape[1])],
            "counts": rle_ref.rle_to_string(counts).decode("ascii") if ann_id % 2 else [int(c) for c in counts]}


def write(paths, name="instances_bitmap", edit=None):
    """Writes ``<root>/<name>.json`` (``edit(data)`` may change the dataset dict first) -> its path."""
    with open(paths["instances"]) as f:
        data = json.load(f)
    masks = bitmaps()
    for a in data["annotations"]:
        if a["id"] in masks:
            a["segmentation"] = segmentation(a["id"], masks[a["id"]])
    if edit is not None:
        edit(data)
    path = os.path.join(paths["root"], name + ".json")
    with open(path, "w") as f:
        json.dump(data, f)
    return path
