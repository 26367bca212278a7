"""TEST INFRASTRUCTURE ONLY -- scalar fp64 restatement of the reference's deformable CUDA kernels.

Plain Python loops over flat, contiguous NumPy arrays with explicit index arithmetic: no torch, no autograd, and no code
shared with oracle/dcn.py, which this module exists to pin (tests/test_dcn_pins.py).  The backward functions restate the
reference's hand-written backward kernels as they are written -- the neighbourhood scan of col2im, the coordinate
kernels with their reset of outside samples -- not the derivative of the forward; that the two coincide is what the
pins test.  Every function names the lines of maskrcnn_benchmark/csrc/cuda/ it restates.

Layouts (all C-contiguous, flattened): x [B, C, H, W]; offset [B, dg * 2 * KH * KW, Ho, Wo] with the row offset of
tap k of deformable group g in plane g * 2K + 2k and its column offset in plane g * 2K + 2k + 1; mask
[B, dg * K, Ho, Wo]; weight [Cout, C / groups, KH, KW]; columns [C * K, B, Ho, Wo].
"""
import math
from collections import namedtuple

import numpy as np

Geom = namedtuple("Geom", "B C H W Cout KH KW sh sw ph pw dh dw groups dg Ho Wo")


def geometry(x_shape, w_shape, stride, padding, dilation, groups, dg):
    """Output size as deform_conv_kernel_cuda.cu:262-263 (and deform_conv_cuda.cu:190-193) form it."""
    B, C, H, W = x_shape
    Cout, _, KH, KW = w_shape
    (sh, sw), (ph, pw), (dh, dw) = stride, padding, dilation
    Ho = (H + 2 * ph - (dh * (KH - 1) + 1)) // sh + 1
    Wo = (W + 2 * pw - (dw * (KW - 1) + 1)) // sw + 1
    return Geom(B, C, H, W, Cout, KH, KW, sh, sw, ph, pw, dh, dw, groups, dg, Ho, Wo)


def _flat(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(-1)


# ------------------------------------------------------------------ device functions
def bilinear(x, base, H, W, h, w):
    """deform_conv_kernel_cuda.cu:92-122 (== :475-505): each of the four corners is read only if it is a cell of the
    map (the per-corner rule); a corner outside contributes 0 with its weight kept."""
    h0, w0 = math.floor(h), math.floor(w)
    h1, w1 = h0 + 1, w0 + 1
    fh, fw = h - h0, w - w0
    a = x[base + h0 * W + w0] if (h0 >= 0 and w0 >= 0) else 0.0
    b = x[base + h0 * W + w1] if (h0 >= 0 and w1 <= W - 1) else 0.0
    c = x[base + h1 * W + w0] if (h1 <= H - 1 and w0 >= 0) else 0.0
    d = x[base + h1 * W + w1] if (h1 <= H - 1 and w1 <= W - 1) else 0.0
    return (1 - fh) * (1 - fw) * a + (1 - fh) * fw * b + fh * (1 - fw) * c + fh * fw * d


def gradient_weight(h, w, cy, cx, H, W):
    """deform_conv_kernel_cuda.cu:125-150 (== :507-532): the share of cell (cy, cx) in a sample at (h, w); 0 for a
    sample on or outside the open box (-1, H) x (-1, W)."""
    if h <= -1 or h >= H or w <= -1 or w >= W:
        return 0.0
    h0, w0 = math.floor(h), math.floor(w)
    h1, w1 = h0 + 1, w0 + 1
    g = 0.0
    if cy == h0 and cx == w0:
        g = (cy + 1 - h) * (cx + 1 - w)
    if cy == h0 and cx == w1:
        g = (cy + 1 - h) * (w + 1 - cx)
    if cy == h1 and cx == w0:
        g = (h + 1 - cy) * (cx + 1 - w)
    if cy == h1 and cx == w1:
        g = (h + 1 - cy) * (w + 1 - cx)
    return g


def coordinate_weight(h, w, H, W, x, base, direction):
    """deform_conv_kernel_cuda.cu:153-195 (== :534-575): the change of the sample with its row (direction 0) or column
    (direction 1) coordinate, corner by corner under the per-corner rule; 0 on or outside the open box."""
    if h <= -1 or h >= H or w <= -1 or w >= W:
        return 0.0
    h0, w0 = math.floor(h), math.floor(w)
    h1, w1 = h0 + 1, w0 + 1
    g = 0.0
    if direction == 0:
        if h0 >= 0 and w0 >= 0:
            g -= (w0 + 1 - w) * x[base + h0 * W + w0]
        if h0 >= 0 and w1 <= W - 1:
            g -= (w - w0) * x[base + h0 * W + w1]
        if h1 <= H - 1 and w0 >= 0:
            g += (w0 + 1 - w) * x[base + h1 * W + w0]
        if h1 <= H - 1 and w1 <= W - 1:
            g += (w - w0) * x[base + h1 * W + w1]
    else:
        if h0 >= 0 and w0 >= 0:
            g -= (h0 + 1 - h) * x[base + h0 * W + w0]
        if h0 >= 0 and w1 <= W - 1:
            g += (h0 + 1 - h) * x[base + h0 * W + w1]
        if h1 <= H - 1 and w0 >= 0:
            g -= (h - h0) * x[base + h1 * W + w0]
        if h1 <= H - 1 and w1 <= W - 1:
            g += (h - h0) * x[base + h1 * W + w1]
    return g


def _position(off, G, b, g, k, ho, wo):
    """The sampling position of tap k: the offset pointer arithmetic of deform_conv_kernel_cuda.cu:220-233 (col2im
    :311-319, coord :420-427; modulated :601-618, :667-679, :741-752)."""
    K, plane = G.KH * G.KW, G.Ho * G.Wo
    at = (b * G.dg + g) * 2 * K * plane + ho * G.Wo + wo
    i, j = k // G.KW, k % G.KW
    h = ho * G.sh - G.ph + i * G.dh + off[at + (2 * k) * plane]
    w = wo * G.sw - G.pw + j * G.dw + off[at + (2 * k + 1) * plane]
    return h, w


# ------------------------------------------------------------------ kernels
def im2col(x, off, mask, G):
    """deformable_im2col_gpu_kernel, deform_conv_kernel_cuda.cu:198-250, and its modulated twin :578-640 (mask given):
    one pass per (channel, image, output pixel) over the taps; the sample is taken only inside the open box
    (-1, H) x (-1, W), else 0."""
    K, plane = G.KH * G.KW, G.Ho * G.Wo
    col = np.zeros(G.C * K * G.B * plane)
    per = G.C // G.dg
    for c in range(G.C):
        g = c // per
        for b in range(G.B):
            img = (b * G.C + c) * G.H * G.W
            for ho in range(G.Ho):
                for wo in range(G.Wo):
                    for k in range(K):
                        h, w = _position(off, G, b, g, k, ho, wo)
                        v = 0.0
                        if h > -1 and w > -1 and h < G.H and w < G.W:
                            v = bilinear(x, img, G.H, G.W, h, w)
                        if mask is not None:
                            v *= mask[((b * G.dg + g) * K + k) * plane + ho * G.Wo + wo]
                        col[(((c * K + k) * G.B + b) * G.Ho + ho) * G.Wo + wo] = v
    return col


def col2im(dcol, off, mask, G):
    """deformable_col2im_gpu_kernel, deform_conv_kernel_cuda.cu:287-342 (modulated :643-700): every column entry is
    spread over the 5x5 cells around the position TRUNCATED towards zero ((int), not floor); a cell takes part if it
    is on the map and closer than 1 in both coordinates, with the weight of gradient_weight."""
    K, plane = G.KH * G.KW, G.Ho * G.Wo
    dx = np.zeros(G.B * G.C * G.H * G.W)
    per = G.C // G.dg
    for c in range(G.C):
        g = c // per
        for k in range(K):
            for b in range(G.B):
                for ho in range(G.Ho):
                    for wo in range(G.Wo):
                        h, w = _position(off, G, b, g, k, ho, wo)
                        top = dcol[(((c * K + k) * G.B + b) * G.Ho + ho) * G.Wo + wo]
                        if mask is not None:
                            top *= mask[((b * G.dg + g) * K + k) * plane + ho * G.Wo + wo]
                        th, tw = int(h), int(w)
                        for cy in range(th - 2, th + 3):
                            if cy < 0 or cy >= G.H or not abs(h - cy) < 1:
                                continue
                            for cx in range(tw - 2, tw + 3):
                                if cx < 0 or cx >= G.W or not abs(w - cx) < 1:
                                    continue
                                dx[((b * G.C + c) * G.H + cy) * G.W + cx] += gradient_weight(h, w, cy, cx, G.H, G.W) * top
    return dx


def col2im_coord(dcol, x, off, mask, G):
    """deformable_col2im_coord_gpu_kernel, deform_conv_kernel_cuda.cu:381-443, and the modulated :703-774: one result
    per offset plane and output pixel.  The walk starts at the plane's tap and steps by K through the column rows of
    the plane's deformable group (one row per channel of the group); a sample on or outside the open box is moved to
    (-2, -2) so that its weight is 0, and only the others add to the mask gradient (the unmasked sample times the
    column gradient), which is stored by the row-direction plane alone."""
    K, plane = G.KH * G.KW, G.Ho * G.Wo
    rows_per_group = G.C * K // G.dg
    doff = np.zeros(G.B * G.dg * 2 * K * plane)
    dmask = None if mask is None else np.zeros(G.B * G.dg * K * plane)
    for b in range(G.B):
        for oc in range(2 * K * G.dg):
            g = oc // (2 * K)
            t = oc - g * 2 * K
            direction = t % 2
            first_row = g * rows_per_group
            first_img = ((b * G.dg + g) * rows_per_group // G.KH // G.KW) * G.H * G.W
            for ho in range(G.Ho):
                for wo in range(G.Wo):
                    acc, macc, n = 0.0, 0.0, 0
                    row = t // 2
                    while row < rows_per_group:
                        k = ((row // G.KW) % G.KH) * G.KW + row % G.KW
                        at = (((first_row + row) * G.B + b) * G.Ho + ho) * G.Wo + wo
                        h, w = _position(off, G, b, g, k, ho, wo)
                        img = first_img + n * G.H * G.W
                        if h <= -1 or w <= -1 or h >= G.H or w >= G.W:
                            h = w = -2.0
                        elif mask is not None:
                            macc += dcol[at] * bilinear(x, img, G.H, G.W, h, w)
                        cw = coordinate_weight(h, w, G.H, G.W, x, img, direction)
                        m = 1.0 if mask is None else mask[((b * G.dg + g) * K + k) * plane + ho * G.Wo + wo]
                        acc += cw * dcol[at] * m
                        n += 1
                        row += K
                    doff[((b * G.dg * 2 * K + oc) * G.Ho + ho) * G.Wo + wo] = acc
                    if mask is not None and direction == 0:
                        dmask[(((b * G.dg + g) * K + t // 2) * G.Ho + ho) * G.Wo + wo] = macc
    return doff, dmask


# ------------------------------------------------------------------ host side
def deform_conv_forward(x, offset, weight, mask=None, bias=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1,
                        deformable_groups=1):
    """deform_conv_forward_cuda (deform_conv_cuda.cu:231-245) / modulated_deform_conv_cuda_forward (:548-577): columns,
    then per image and group the product weight[g] (Cout/groups x R) . columns[g] (R x Ho*Wo), R = C/groups * K, then the
    bias (v2).  Returns (out [B, Cout, Ho, Wo], columns)."""
    G = geometry(x.shape, weight.shape, stride, padding, dilation, groups, deformable_groups)
    col = im2col(_flat(x), _flat(offset), _flat(mask), G)
    K, plane = G.KH * G.KW, G.Ho * G.Wo
    R, Og = G.C // groups * K, G.Cout // groups
    wf = _flat(weight)
    out = np.zeros(G.B * G.Cout * plane)
    for b in range(G.B):
        for g in range(groups):
            for o in range(Og):
                wrow = wf[(g * Og + o) * R:(g * Og + o + 1) * R]
                acc = np.zeros(plane)
                for r in range(R):
                    at = ((g * R + r) * G.B + b) * plane
                    acc += wrow[r] * col[at:at + plane]
                if bias is not None:
                    acc += float(bias.reshape(-1)[g * Og + o])
                at = (b * G.Cout + g * Og + o) * plane
                out[at:at + plane] = acc
    return out.reshape(G.B, G.Cout, G.Ho, G.Wo), col


def deform_conv_backward(x, offset, weight, gout, mask=None, stride=(1, 1), padding=(0, 0), dilation=(1, 1), groups=1,
                         deformable_groups=1):
    """deform_conv_backward_input_cuda (deform_conv_cuda.cu:332-360), deform_conv_backward_parameters_cuda (:455-480, scale
    1) and modulated_deform_conv_cuda_backward (:626-683): column gradient = weight[g]^T . gout[g]; the coordinate kernel
    and col2im on it; weight gradient = gout[g] . columns[g]^T with the (masked) forward columns; bias gradient = row sums
    of gout.  Returns dict(x, offset, weight, mask, bias); mask and bias are None for v1."""
    G = geometry(x.shape, weight.shape, stride, padding, dilation, groups, deformable_groups)
    xf, of, mf, wf, gf = _flat(x), _flat(offset), _flat(mask), _flat(weight), _flat(gout)
    K, plane = G.KH * G.KW, G.Ho * G.Wo
    R, Og = G.C // groups * K, G.Cout // groups
    dcol = np.zeros(G.C * K * G.B * plane)
    for b in range(G.B):
        for g in range(groups):
            for r in range(R):
                acc = np.zeros(plane)
                for o in range(Og):
                    at = (b * G.Cout + g * Og + o) * plane
                    acc += wf[(g * Og + o) * R + r] * gf[at:at + plane]
                at = ((g * R + r) * G.B + b) * plane
                dcol[at:at + plane] = acc
    doff, dmask = col2im_coord(dcol, xf, of, mf, G)
    dx = col2im(dcol, of, mf, G)
    col = im2col(xf, of, mf, G)
    dw = np.zeros(G.Cout * R)
    for b in range(G.B):
        for g in range(groups):
            for o in range(Og):
                at = (b * G.Cout + g * Og + o) * plane
                go = gf[at:at + plane]
                for r in range(R):
                    ct = ((g * R + r) * G.B + b) * plane
                    dw[(g * Og + o) * R + r] += float(np.dot(go, col[ct:ct + plane]))
    db = None
    if mask is not None:
        db = np.zeros(G.Cout)
        for b in range(G.B):
            for o in range(G.Cout):
                at = (b * G.Cout + o) * plane
                db[o] += float(gf[at:at + plane].sum())
    return dict(x=dx.reshape(x.shape), offset=doff.reshape(offset.shape), weight=dw.reshape(weight.shape),
                mask=None if dmask is None else dmask.reshape(mask.shape), bias=db)


def sample_positions(offset, w_shape, x_shape, stride, padding, dilation, deformable_groups):
    """All sampling positions of a call, as two flat arrays (rows, columns) -- for the tests' edge counters."""
    G = geometry(x_shape, w_shape, stride, padding, dilation, 1, deformable_groups)
    of = _flat(offset)
    hs, ws = [], []
    for b in range(G.B):
        for g in range(G.dg):
            for k in range(G.KH * G.KW):
                for ho in range(G.Ho):
                    for wo in range(G.Wo):
                        h, w = _position(of, G, b, g, k, ho, wo)
                        hs.append(h)
                        ws.append(w)
    return np.array(hs), np.array(ws)


# ------------------------------------------------------------------ deformable PS-RoI pooling
_f32, _f64 = np.float32, np.float64


def _roundf(v):
    """C round(): halves away from zero."""
    v = _f32(v)
    return _f32(math.floor(float(v) + 0.5)) if v >= 0 else _f32(math.ceil(float(v) - 0.5))


def _bin_geometry(rois, trans, n, ctop, ph, pw, scale, P, od, no_trans, gs, part, spp, std, classes):
    """The shared preamble of deform_pool_kernel_cuda.cu:76-116 (forward) and :180-209 (backward), in float32 with the
    promotions to double that the reference's double literals (0.5, 1., 0.1) cause."""
    scale, std = _f32(scale), _f32(std)
    r = rois[n * 5:n * 5 + 5]
    start_w = _f32(_f64(_roundf(r[1]) * scale) - 0.5)
    start_h = _f32(_f64(_roundf(r[2]) * scale) - 0.5)
    end_w = _f32(_f64(_f32(_f64(_roundf(r[3])) + 1.0) * scale) - 0.5)
    end_h = _f32(_f64(_f32(_f64(_roundf(r[4])) + 1.0) * scale) - 0.5)
    roi_w = _f32(max(_f64(end_w - start_w), 0.1))
    roi_h = _f32(max(_f64(end_h - start_h), 0.1))
    bin_h, bin_w = roi_h / _f32(P), roi_w / _f32(P)
    sub_h, sub_w = bin_h / _f32(spp), bin_w / _f32(spp)
    part_h = math.floor(_f32(ph) / _f32(P) * _f32(part))
    part_w = math.floor(_f32(pw) / _f32(P) * _f32(part))
    cls = ctop // (od if no_trans else od // classes)
    tx_at = (((n * classes + cls) * 2) * part + part_h) * part + part_w
    ty_at = (((n * classes + cls) * 2 + 1) * part + part_h) * part + part_w
    tx = _f32(0) if no_trans else _f32(trans[tx_at]) * std
    ty = _f32(0) if no_trans else _f32(trans[ty_at]) * std
    wstart = _f32(pw) * bin_w + start_w
    wstart = wstart + tx * roi_w
    hstart = _f32(ph) * bin_h + start_h
    hstart = hstart + ty * roi_h
    gw = min(max(math.floor(_f32(pw) * _f32(gs) / _f32(P)), 0), gs - 1)
    gh = min(max(math.floor(_f32(ph) * _f32(gs) / _f32(P)), 0), gs - 1)
    return int(r[0]), roi_w, roi_h, sub_w, sub_h, wstart, hstart, (ctop * gs + gh) * gs + gw, tx_at, ty_at


def _bin_samples(wstart, hstart, sub_w, sub_h, spp, H, W):
    """The sample loop of deform_pool_kernel_cuda.cu:119-137 / :222-234: a sample counts unless it lies beyond half a
    cell outside the map (tested on the UNCLAMPED position, in double); its weights come from the position CLAMPED to the
    map.  Yields (x0, x1, y0, y1, dist_x, dist_y) with floor / ceil cells and float32 distances promoted to double."""
    for ih in range(spp):
        for iw in range(spp):
            w = wstart + _f32(iw) * sub_w
            h = hstart + _f32(ih) * sub_h
            if _f64(w) < -0.5 or _f64(w) > W - 0.5 or _f64(h) < -0.5 or _f64(h) > H - 0.5:
                continue
            w = _f32(min(max(_f64(w), 0.0), W - 1.0))
            h = _f32(min(max(_f64(h), 0.0), H - 1.0))
            x0, x1, y0, y1 = math.floor(w), math.ceil(w), math.floor(h), math.ceil(h)
            yield x0, x1, y0, y1, float(w - _f32(x0)), float(h - _f32(y0)), float(w), float(h)


def psroi_forward(data, rois, trans, scale, P, od, no_trans, gs, part, spp, std):
    """DeformablePSROIPoolForwardKernel, deform_pool_kernel_cuda.cu:54-139 (bilinear_interp :31-52): the mean of the
    counted samples of each bin, and the count.  data [B, C, H, W], rois [n, 5], trans [n, 2 * classes, part, part].
    Returns (out, count)."""
    B, C, H, W = data.shape
    n_rois = rois.shape[0]
    classes = 1 if no_trans else trans.shape[1] // 2
    d, r, t = _flat(data), np.ascontiguousarray(rois, dtype=_f32).reshape(-1), None if no_trans else _flat(trans)
    out, cnt = np.zeros(n_rois * od * P * P), np.zeros(n_rois * od * P * P)
    for n in range(n_rois):
        for ctop in range(od):
            for ph in range(P):
                for pw in range(P):
                    b, _, _, sub_w, sub_h, wstart, hstart, c, _, _ = _bin_geometry(r, t, n, ctop, ph, pw, scale, P, od, no_trans,
                                                                                  gs, part, spp, std, classes)
                    base = (b * C + c) * H * W
                    total, count = 0.0, 0
                    for x0, x1, y0, y1, fx, fy, _, _ in _bin_samples(wstart, hstart, sub_w, sub_h, spp, H, W):
                        total += ((1 - fx) * (1 - fy) * d[base + y0 * W + x0] + (1 - fx) * fy * d[base + y1 * W + x0]
                                  + fx * (1 - fy) * d[base + y0 * W + x1] + fx * fy * d[base + y1 * W + x1])
                        count += 1
                    at = ((n * od + ctop) * P + ph) * P + pw
                    out[at] = 0.0 if count == 0 else total / count
                    cnt[at] = count
    return out.reshape(n_rois, od, P, P), cnt.reshape(n_rois, od, P, P)


def psroi_positions(data_shape, rois, trans, scale, P, od, no_trans, gs, part, spp, std):
    """Unclamped (w, h) of every sample of every bin, as float64 arrays -- for the tests' edge counters."""
    n_rois = rois.shape[0]
    classes = 1 if no_trans else trans.shape[1] // 2
    r, t = np.ascontiguousarray(rois, dtype=_f32).reshape(-1), None if no_trans else _flat(trans)
    ws, hs = [], []
    for n in range(n_rois):
        for ctop in range(od):
            for ph in range(P):
                for pw in range(P):
                    _, _, _, sub_w, sub_h, wstart, hstart, _, _, _ = _bin_geometry(r, t, n, ctop, ph, pw, scale, P, od, no_trans,
                                                                                  gs, part, spp, std, classes)
                    for ih in range(spp):
                        for iw in range(spp):
                            ws.append(float(wstart + _f32(iw) * sub_w))
                            hs.append(float(hstart + _f32(ih) * sub_h))
    return np.array(ws), np.array(hs)


def psroi_backward(gout, count, data, rois, trans, scale, P, od, no_trans, gs, part, spp, std):
    """DeformablePSROIPoolBackwardAccKernel, deform_pool_kernel_cuda.cu:144-263: bins with a count of 0 are passed over;
    each counted sample adds gout / count to its four cells with the weights of its clamped position, and to the two
    trans entries of its part the difference of the cell values across that position times trans_std, gout / count and
    the RoI's width (height).  Returns (ddata, dtrans); dtrans is None when no_trans."""
    B, C, H, W = data.shape
    n_rois = rois.shape[0]
    classes = 1 if no_trans else trans.shape[1] // 2
    d, r, t = _flat(data), np.ascontiguousarray(rois, dtype=_f32).reshape(-1), None if no_trans else _flat(trans)
    go, cn = _flat(gout), _flat(count)
    dd = np.zeros(B * C * H * W)
    dt = None if no_trans else np.zeros(t.size)
    for n in range(n_rois):
        for ctop in range(od):
            for ph in range(P):
                for pw in range(P):
                    at = ((n * od + ctop) * P + ph) * P + pw
                    if cn[at] <= 0:
                        continue
                    b, roi_w, roi_h, sub_w, sub_h, wstart, hstart, c, tx_at, ty_at = _bin_geometry(
                        r, t, n, ctop, ph, pw, scale, P, od, no_trans, gs, part, spp, std, classes)
                    share = go[at] / cn[at]
                    base = (b * C + c) * H * W
                    for x0, x1, y0, y1, fx, fy, _, _ in _bin_samples(wstart, hstart, sub_w, sub_h, spp, H, W):
                        dd[base + y0 * W + x0] += (1 - fx) * (1 - fy) * share
                        dd[base + y1 * W + x0] += (1 - fx) * fy * share
                        dd[base + y0 * W + x1] += fx * (1 - fy) * share
                        dd[base + y1 * W + x1] += fx * fy * share
                        if no_trans:
                            continue
                        u00, u01 = d[base + y0 * W + x0], d[base + y1 * W + x0]
                        u10, u11 = d[base + y0 * W + x1], d[base + y1 * W + x1]
                        across = (u11 * fy + u10 * (1 - fy) - u01 * fy - u00 * (1 - fy)) * float(_f32(std)) * share
                        down = (u11 * fx + u01 * (1 - fx) - u10 * fx - u00 * (1 - fx)) * float(_f32(std)) * share
                        dt[tx_at] += across * float(roi_w)
                        dt[ty_at] += down * float(roi_h)
    return dd.reshape(data.shape), None if no_trans else dt.reshape(trans.shape)
