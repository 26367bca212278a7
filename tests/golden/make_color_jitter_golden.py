"""Writes tests/golden/color_jitter.npz: what PIL ITSELF produces for the colour jitter -- ImageEnhance.Brightness / Contrast /
Color and the HSV round trip (convert('HSV'), uint8 addition on H, merge, convert('RGB')), composed as torchvision 0.4-0.7's
functional_pil composes them (written out in ``pil_chain``; torchvision is not needed and was not run).  The fixture records
the PIL version, small seeded inputs with their outputs, Image.blend over every (d, x) pair at six factors, and only
CRC32s for the image of all 2^24 colours.  tests/test_color_jitter_reference.py pins the NumPy restatement
(tests/color_jitter_reference.py) to it.

    python -m tests.golden.make_color_jitter_golden
"""
import itertools
import os
import zlib

import numpy as np

SHIFTS = (0, 1, 127, 128, 255)
FACTORS = (0.0, 0.37, 1.0, float(np.nextafter(np.float32(1), np.float32(2))), 1.5, 2.0)
ORDERS = [list(p) for p in itertools.permutations(range(4))]
SUBSETS = [[c for c in range(4) if mask >> c & 1] for mask in range(16)]
PARAMS = {0: 1.3, 1: 0.6, 2: 1.7, 3: 37.0}   # per operation code: three factors and a hue shift


def seeded_image(h=16, w=23, seed=7):
    return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)


def half_mean_image():
    """Greys 10 and 11: the contrast mean is exactly 10.5 -> 11."""
    return np.array([[[10, 10, 10], [11, 11, 11]]], dtype=np.uint8)


def constant_image():
    return np.tile(np.array([77, 13, 200], dtype=np.uint8), (4, 4, 1))


def one_pixel():
    return np.array([[[201, 54, 9]]], dtype=np.uint8)


def row(ops):
    """([4 codes], [4 parameters]) of a list of operation codes with the parameters of PARAMS."""
    return list(ops) + [-1] * (4 - len(ops)), [PARAMS[o] for o in ops] + [0.0] * (4 - len(ops))


def pil_chain(img, ops, params):
    from PIL import Image, ImageEnhance

    im = Image.fromarray(img)
    for o, p in zip(ops, params):
        if o == -1:
            break
        if o == 0:
            im = ImageEnhance.Brightness(im).enhance(float(p))
        elif o == 1:
            im = ImageEnhance.Contrast(im).enhance(float(p))
        elif o == 2:
            im = ImageEnhance.Color(im).enhance(float(p))
        else:
            h, s, v = im.convert("HSV").split()
            np_h = np.array(h, dtype=np.uint8)
            with np.errstate(over="ignore"):
                np_h += np.uint8(int(p))
            im = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
    return np.asarray(im)


def pil_blend_table(factor):
    """uint8 [256, 256]: Image.blend(d, x, factor) with d down the rows and x along the columns."""
    from PIL import Image

    d, x = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    return np.asarray(Image.blend(Image.fromarray(d, "L"), Image.fromarray(x, "L"), factor))


def all_colours():
    idx = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def main():
    import PIL

    img = seeded_image()
    out = {"pil_version": np.array(PIL.__version__), "img": img,
           "orders": np.stack([pil_chain(img, *row(o)) for o in ORDERS]),
           "subsets": np.stack([pil_chain(img, *row(s)) for s in SUBSETS]),
           "blend": np.stack([pil_blend_table(f) for f in FACTORS]),
           "hue_small": np.stack([pil_chain(img, [3, -1, -1, -1], [float(s), 0, 0, 0]) for s in SHIFTS])}
    for name, small in (("half", half_mean_image()), ("constant", constant_image()), ("pixel", one_pixel())):
        out[name] = np.stack([pil_chain(small, *row(o)) for o in ORDERS] +
                             [pil_chain(small, [1, -1, -1, -1], [f, 0, 0, 0]) for f in (0.0, 2.0)])
    colours = all_colours()
    out["hue_crc"] = np.array([zlib.crc32(pil_chain(colours, [3, -1, -1, -1], [float(s), 0, 0, 0]).tobytes()) for s in SHIFTS],
                              dtype=np.int64)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "color_jitter.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes, PIL", PIL.__version__)


if __name__ == "__main__":
    main()
