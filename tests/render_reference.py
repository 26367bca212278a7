"""TEST-ONLY: a NumPy restatement of the prediction compositor (``_C.render_instances``), independent of the package's
code -- the Masker paste as csrc/pasted_value.h spells it (float32, one rounding per operation, in that order), the two
blends of mb/engine/inference.py:557-589 as NumPy itself evaluates them, and the outline rule of include/ovis_hip.h.
Pinned to the reference's own functions by tests/golden/render.npz (tests/test_render_reference.py)."""
import numpy as np

F = np.float32
FILL, HEAT = 0, 1


def pasted_rect(box, m):
    """(x0, y0, x1, y1, bw, bh): the box expanded by (M+2)/M about its centre, truncated toward zero; extents >= 1."""
    gx0, gy0, gx1, gy1 = (F(v) for v in box)
    scale = F(F(m + 2) / F(m))
    w_half = F(F(F(gx1 - gx0) * F(0.5)) * scale)
    h_half = F(F(F(gy1 - gy0) * F(0.5)) * scale)
    x_c = F(F(gx1 + gx0) * F(0.5))
    y_c = F(F(gy1 + gy0) * F(0.5))
    x0, y0, x1, y1 = int(F(x_c - w_half)), int(F(y_c - h_half)), int(F(x_c + w_half)), int(F(y_c + h_half))
    return x0, y0, x1, y1, max(x1 - x0 + 1, 1), max(y1 - y0 + 1, 1)


def _axis(pos, origin, extent, s):
    """Source cells and weight of output positions ``pos`` along one axis (align_corners=False, clamped at 0)."""
    scale = F(F(s) / F(extent))
    src = np.maximum(scale * ((pos - origin).astype(F) + F(0.5)) - F(0.5), F(0))
    assert src.dtype == F
    i0 = src.astype(np.int64)
    i1 = i0 + (i0 < s - 1)
    return i0, i1, src - i0.astype(F)


def pasted_values(prob, box, height, width):
    """float32 [height, width]: the un-thresholded paste of one [M, M] map (zero outside the integer box), and the bool
    array of the pixels inside the box and the image."""
    m = prob.shape[0]
    s = m + 2
    padded = np.zeros((s, s), dtype=F)
    padded[1:-1, 1:-1] = prob
    x0, y0, x1, y1, bw, bh = pasted_rect(box, m)
    cx0, cx1, cy0, cy1 = max(x0, 0), min(x1, width - 1), max(y0, 0), min(y1, height - 1)
    values = np.zeros((height, width), dtype=F)
    inside = np.zeros((height, width), dtype=bool)
    if cx1 < cx0 or cy1 < cy0:
        return values, inside
    ya0, ya1, ly = _axis(np.arange(cy0, cy1 + 1), y0, bh, s)
    xa0, xa1, lx = _axis(np.arange(cx0, cx1 + 1), x0, bw, s)
    ly, lx = ly[:, None], lx[None, :]
    one = F(1)
    top = (one - lx) * padded[ya0[:, None], xa0[None, :]] + lx * padded[ya0[:, None], xa1[None, :]]
    bottom = (one - lx) * padded[ya1[:, None], xa0[None, :]] + lx * padded[ya1[:, None], xa1[None, :]]
    v = (one - ly) * top + ly * bottom
    assert v.dtype == F
    values[cy0:cy1 + 1, cx0:cx1 + 1] = v
    inside[cy0:cy1 + 1, cx0:cx1 + 1] = True
    return values, inside


def paste_binary(prob, box, height, width, threshold=0.5):
    values, inside = pasted_values(prob, box, height, width)
    return inside & (values > F(threshold))


def fill(image, mask, color, alpha=0.5):
    """overlay_filled_mask's assignment for one instance: float64, truncated into the uint8 image."""
    a = np.float64(F(alpha))
    out = image.copy()
    for c in range(3):
        blended = image[:, :, c] * (1.0 - a) + a * np.float64(F(color[c]))
        out[:, :, c] = np.where(mask, blended, image[:, :, c])
    return out


def heat(image, values, gain, color):
    """overlay_uncertainty_mask's assignment for one instance: float32 throughout, truncated into the uint8 image."""
    m = np.clip(values * F(gain), F(0), F(1))
    assert m.dtype == F
    out = image.copy()
    for c in range(3):
        blended = image[:, :, c].astype(F) * (F(1) - m) + m * F(color[c])
        assert blended.dtype == F
        out[:, :, c] = np.where(m != 0, blended, image[:, :, c])
    return out


def outline_mask(box, thickness, height, width):
    """The rule of include/ovis_hip.h: corners truncated toward zero and ordered; an edge at c covers c - floor(t/2) ...
    c + ceil(t/2) - 1; square corners; clipped to the image."""
    x0, y0, x1, y1 = (int(F(v)) for v in box)
    xa, xb, ya, yb = min(x0, x1), max(x0, x1), min(y0, y1), max(y0, y1)
    lo, hi = thickness // 2, (thickness + 1) // 2 - 1
    ys, xs = np.arange(height)[:, None], np.arange(width)[None, :]
    outer = (xs >= xa - lo) & (xs <= xb + hi) & (ys >= ya - lo) & (ys <= yb + hi)
    band = (xs <= xa + hi) | (xs >= xb - lo) | (ys <= ya + hi) | (ys >= yb - lo)
    return outer & band


def render(image, maps, boxes, colors, kinds=None, params=None, alpha=0.5, outline_colors=None, outline_thickness=2):
    """uint8 [H, W, 3]: every outline first, then the layers in index order."""
    image, maps, boxes, colors = np.asarray(image), np.asarray(maps, dtype=F), np.asarray(boxes, dtype=F), np.asarray(colors, dtype=F)
    k = maps.shape[0]
    height, width = image.shape[:2]
    kinds = np.zeros(k, dtype=np.int32) if kinds is None else np.asarray(kinds)
    params = np.full(k, 0.5 if params is None else params, dtype=F) if params is None or np.isscalar(params) else np.asarray(params, dtype=F)
    out = image.copy()
    if outline_colors is not None:
        for i in range(k):
            out[outline_mask(boxes[i], outline_thickness, height, width)] = np.asarray(outline_colors)[i]
    for i in range(k):
        values, inside = pasted_values(maps[i], boxes[i], height, width)
        if kinds[i] == FILL:
            out = fill(out, inside & (values > params[i]), colors[i], alpha)
        elif kinds[i] == HEAT:
            out = heat(out, values, params[i], colors[i])
    return out


# ---- the inputs of tests/golden/render.npz: seeded, not stored (the fixture holds what the reference made of them) ----------
# name -> (seed, height, width, M, boxes xyxy); the boxes leave the image on every side, one is narrower than a pixel
GOLDEN_CASES = {
    "fill_a": (11, 61, 97, 14, [[8.3, 5.1, 60.2, 40.7], [-9.5, 20.0, 30.4, 70.9], [50.0, -6.2, 110.3, 33.3], [40.2, 30.1, 40.6, 55.0]]),
    "fill_b": (12, 29, 41, 28, [[3.0, 2.0, 30.5, 20.5], [20.1, 10.7, 47.0, 35.2], [-4.0, -3.0, 12.0, 9.9]]),
    "heat_a": (13, 31, 37, 14, [[2.2, 3.3, 25.1, 22.8], [15.0, -5.0, 44.0, 18.0], [-6.0, 12.0, 14.0, 36.0]]),
    "heat_b": (14, 33, 40, 56, [[1.0, 1.0, 38.0, 31.0], [10.5, 8.5, 22.5, 29.5]]),
    "combined": (15, 31, 41, 14, [[4.0, 3.0, 28.0, 24.0], [12.0, 6.0, 39.5, 29.0], [-3.0, 14.0, 20.0, 35.0]]),
}


def golden_inputs(name):
    """image uint8 [H, W, 3], maps f32 [K, M, M] in (0, 1), boxes f32 [K, 4], scores f32 [K], labels int64 [K]."""
    seed, h, w, m, boxes = GOLDEN_CASES[name]
    rs = np.random.RandomState(seed)
    k = len(boxes)
    image = rs.randint(0, 256, (h, w, 3)).astype(np.uint8)
    # smooth blobs rather than noise: a decision boundary that crosses the box, as a mask head's output has
    yy, xx = np.mgrid[0:m, 0:m].astype(np.float64) / (m - 1)
    maps = np.stack([np.exp(-(((yy - rs.uniform(0.3, 0.7)) / rs.uniform(0.2, 0.5)) ** 2 + ((xx - rs.uniform(0.3, 0.7)) / rs.uniform(0.2, 0.5)) ** 2))
                     for _ in range(k)]) * rs.uniform(0.7, 1.0, (k, 1, 1)) + rs.uniform(0.0, 0.02, (k, m, m))
    scores = rs.uniform(0.3, 0.95, k).astype(F)
    labels = rs.randint(1, 60, k).astype(np.int64)
    maps = np.round(maps * 4096.0) / 4096.0  # exact in float32, and out of reach of a last-bit difference between exp()s
    return image, maps.astype(F), np.asarray(boxes, dtype=F), scores, labels


def golden_crc(name):
    import zlib
    image, maps = golden_inputs(name)[:2]
    return zlib.crc32(maps.tobytes(), zlib.crc32(image.tobytes()))
