"""NumPy restatement of the colour-jitter rule of include/ovis_hip.h (``ovis_color_jitter_u8``), written from that text and
not from the C++: the yardstick of tests/test_color_jitter*.py.  Every function takes and returns uint8 arrays [..., 3]
(or scalars / arrays of channel values for ``blend``); float32 steps are NumPy float32 operations, one rounding each."""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE, UNUSED = 0, 1, 2, 3, -1
F32, F64 = np.float32, np.float64


def blend(d, x, a):
    """blend(d, x, a) per element -> uint8."""
    a = F32(a)
    d32, x32 = np.asarray(d).astype(F32), np.asarray(x).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        diff = x32 - d32
        prod = a * diff
        t = d32 + prod
    assert t.dtype == F32
    if 0 <= a <= 1:
        return t.astype(np.int32).astype(np.uint8)
    out = np.where(t >= 255, F32(255), t)
    out = np.where(out > 0, out, F32(0))      # t <= 0 and NaN -> 0
    return out.astype(np.int32).astype(np.uint8)


def grey(img):
    v = img.astype(np.int64)
    return (v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast_mean(img):
    g = grey(img)
    return int(float(int(g.sum())) / float(g.size) + 0.5)


def contrast(img, f):
    return blend(np.full_like(img, contrast_mean(img)), img, f)


def saturation(img, f):
    g = grey(img).astype(np.uint8)
    return blend(np.repeat(g[..., None], 3, axis=-1), img, f)


def _clip8(v):
    return np.clip(v, 0, 255)


def rgb_to_hsv(img):
    r, g, b = (img[..., k].astype(np.int32) for k in range(3))
    maxc, minc = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    flat = maxc == minc
    with np.errstate(divide="ignore", invalid="ignore"):
        cr = (maxc - minc).astype(F32)
        maxf = maxc.astype(F32)
        sat = cr / maxf
        rc, gc, bc = ((maxc - c).astype(F32) / cr for c in (r, g, b))
        h_r = bc - gc
        h_g = (F64(2.0) + rc.astype(F64) - bc.astype(F64)).astype(F32)
        h_b = (F64(4.0) + gc.astype(F64) - rc.astype(F64)).astype(F32)
        hf = np.where(r == maxc, h_r, np.where(g == maxc, h_g, h_b))
        assert hf.dtype == F32 and sat.dtype == F32
        hf = np.fmod(hf.astype(F64) / 6.0 + 1.0, 1.0).astype(F32)
        h = _clip8(np.where(flat, 0, (hf.astype(F64) * 255.0)).astype(np.int32))
        s = _clip8(np.where(flat, 0, sat * F32(255)).astype(np.int32))
    return np.stack([np.where(flat, 0, h), np.where(flat, 0, s), maxc], axis=-1).astype(np.uint8)


def hsv_to_rgb(hsv):
    h, s, v = (hsv[..., k].astype(F64) for k in range(3))
    hh = h * 6.0 / 255.0
    i = np.floor(hh)
    f = hh - i
    fs = s / 255.0

    def rnd(x):
        return _clip8(np.floor(x + 0.5)).astype(np.uint8)

    p, q, t = rnd(v * (1.0 - fs)), rnd(v * (1.0 - fs * f)), rnd(v * (1.0 - fs * (1.0 - f)))
    v8 = hsv[..., 2]
    sel = i.astype(np.int32) % 6
    table = (((v8, t, p), (q, v8, p), (p, v8, t), (p, q, v8), (t, p, v8), (v8, p, q)))
    out = np.stack([np.choose(sel, [row[k] for row in table]) for k in range(3)], axis=-1)
    grey_px = hsv[..., 1] == 0
    return np.where(grey_px[..., None], v8[..., None], out).astype(np.uint8)


def hue(img, shift):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + int(shift)) & 255).astype(np.uint8)
    return hsv_to_rgb(hsv)


def all_colours():
    """The 4096 x 4096 image that holds every RGB triple once: pixel index = r * 65536 + g * 256 + b."""
    idx = np.arange(1 << 24, dtype=np.uint32)
    return np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], axis=-1).astype(np.uint8).reshape(4096, 4096, 3)


def hue_many(img, shifts):
    """``hue`` at several shifts, sharing the RGB -> HSV pass and one HSV -> RGB table over all (h, s, v)."""
    hsv = rgb_to_hsv(img).astype(np.int32)
    idx = np.arange(1 << 24, dtype=np.uint32)
    table = hsv_to_rgb(np.stack([(idx >> 16) & 255, (idx >> 8) & 255, idx & 255], axis=-1).astype(np.uint8))
    base = hsv[..., 1] * 256 + hsv[..., 2]
    return [table[(((hsv[..., 0] + int(s)) & 255) << 16) + base] for s in shifts]


def apply_chain(img, ops, params):
    """One image [h, w, 3] through its row of the tables: ``ops`` codes in application order (UNUSED for trailing slots),
    ``params`` the factors (the shift for HUE).  A malformed row leaves the image unchanged."""
    ops = [int(o) for o in ops]
    used = [o for o in ops if o != UNUSED]
    if (any(o < -1 or o > 3 for o in ops) or len(set(used)) != len(used)
            or any(a == UNUSED and b != UNUSED for a, b in zip(ops, ops[1:]))):
        return img.copy()
    out = img.copy()
    for o, p in zip(ops, params):
        if o == UNUSED:
            break
        if o == HUE:
            p = float(p)
            out = hue(out, int(p) if 0 <= p <= 255 else 0)
        else:
            out = (brightness, contrast, saturation)[o](out, p)
    return out


def apply_batch(data, desc, ops, params):
    """The packed buffer of ``_C.color_jitter``: data uint8 [bytes], desc [B, 7], ops / params [B, 4] -> uint8 [bytes]."""
    data, out = np.asarray(data), np.asarray(data).copy()
    for d, o, p in zip(np.asarray(desc), np.asarray(ops), np.asarray(params)):
        off, h, w = int(d[0]), int(d[1]), int(d[2])
        out[off:off + 3 * h * w] = apply_chain(data[off:off + 3 * h * w].reshape(h, w, 3), o, p).reshape(-1)
    return out


def pack(images):
    """(data, desc) of a list of uint8 [h, w, 3] images; the output size is the input's, no flips."""
    desc, off = [], 0
    for im in images:
        h, w = im.shape[:2]
        desc.append([off, h, w, h, w, 0, 0])
        off += 3 * h * w
    return np.concatenate([im.reshape(-1) for im in images]), np.array(desc, dtype=np.int32)
