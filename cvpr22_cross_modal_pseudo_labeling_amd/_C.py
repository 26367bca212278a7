"""Operator surface of ``maskrcnn_benchmark._C`` (maskrcnn_benchmark/csrc/vision.cpp:9-25) on MI355X.

Same names, argument order and return conventions as the reference's pybind module; every op
is a thin tensor<->pointer shim over the C ABI in ``include/ovis_hip.h``.  Like the reference's module
(csrc/ROIAlign.h:11-25, csrc/nms.h:10-28) the entry points the CPU-only configuration needs dispatch on the
tensor's device: HOST tensors go to ``_cpu.py`` (RoIAlign, NMS: ``libovis_cpu.so``; heads / losses: the
reference's torch-op formulas), DEVICE tensors to the HIP kernels -- never across.  Every other op raises on
host tensors (the reference raises "Not implemented on the CPU", csrc/ROIAlign.h:44,
csrc/SigmoidFocalLoss.h:23,40).
"""
import contextlib
import functools
import ctypes
import threading

import torch

from . import _cpu, _lib

_L = _lib.load()


def _stream():
    # the raw handle of the current stream of the current device (the `with _on(...)` around every launch makes that
    # the operands' device); ~10x cheaper than building a torch.cuda.Stream object per launch
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


class _Same:
    """No-op context: the operands already live on the current device (every launch of a one-GPU-per-process run)."""

    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_SAME = _Same()


def _on(device):
    """``torch.cuda.device(device)`` only when it would change the current device."""
    return _SAME if device.index == torch.cuda.current_device() else torch.cuda.device(device)


def _check_dev(t, name, dtype=torch.float32):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a HIP device tensor: this op has no host implementation (as in the reference)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")


def _dev(t, name, dtype=torch.float32):
    _check_dev(t, name, dtype)
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    return t


# ---- what every shim does around a launch ------------------------------------------------------
def _ptr(t):
    """The device pointer of an optional tensor: NULL for None."""
    return 0 if t is None else t.data_ptr()


def _workspace(nbytes, device, at_least=0):
    """uint8 device scratch of max(nbytes, at_least) bytes, or None (NULL through ``_ptr``) when that is 0.  ``at_least``
    is the entry point's convention for a problem that needs no scratch: a 1-byte dummy (RoIAlign, transform_images), 256
    bytes (bottleneck_identity_backward), nothing (everything else)."""
    nbytes = max(nbytes, at_least)
    return torch.empty((nbytes,), dtype=torch.uint8, device=device) if nbytes else None


def _check_pairs(op, **operands):
    for name, t in operands.items():
        if not (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 2 and t.stride(1) == 1):
            raise RuntimeError(f"{op}: {name} must be a 2-D bfloat16 HIP tensor in pair layout")


def _gemm_results(m, n, out_f32, out_pair, device):
    """(C f32 [M, N] or None, C in pair layout [M, 2N] or None) of the split-GEMM family, uninitialised."""
    return (torch.empty((m, n), dtype=torch.float32, device=device) if out_f32 else None,
            torch.empty((m, 2 * n), dtype=torch.bfloat16, device=device) if out_pair else None)


# ---- RoIAlign (csrc/ROIAlign.h:11-46) ---------------------------------------------------------
def _roi_align_forward(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio, exact):
    if not input.is_cuda:
        return _cpu.roi_align_forward(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio)
    input, rois = _dev(input, "input"), _dev(rois, "rois")
    if rois.dim() != 2 or rois.size(1) != 5 or input.dim() != 4:
        raise RuntimeError("roi_align_forward: expected input [N,C,H,W] and rois [R,5]")
    n, c, h, w = input.shape
    r = rois.size(0)
    out = torch.empty((r, c, pooled_height, pooled_width), dtype=input.dtype, device=input.device)
    if out.numel() == 0:
        return out
    with _on(input.device):
        if exact:
            rc = _L.ovis_roi_align_forward_f32(input.data_ptr(), rois.data_ptr(), out.data_ptr(), r, n, c, h, w,
                                               pooled_height, pooled_width, spatial_scale, sampling_ratio, _stream())
        else:
            nbytes = _L.ovis_roi_align_forward_workspace_bytes(r, h, w)
            ws = _workspace(nbytes, input.device, at_least=1)
            rc = _L.ovis_roi_align_forward_ws_f32(input.data_ptr(), rois.data_ptr(), out.data_ptr(), r, n, c, h, w,
                                                  pooled_height, pooled_width, spatial_scale, sampling_ratio,
                                                  ws.data_ptr(), nbytes, _stream())
    _lib.check(rc, "roi_align_forward")
    return out


def roi_align_forward(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio):
    """The reference's `_C.roi_align_forward`: bit-identical to the reference CPU kernel
    (cpu/ROIAlign_cpu.cpp:114-219) on finite inputs -- same IEEE operation sequence, FP contraction off."""
    return _roi_align_forward(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio, True)


def roi_align_forward_mfma(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio):
    """Matrix-core forward (extension): separable weights as bf16 hi/lo MFMA operands, same values up to ~2^-15 of
    sum |w x|.  Round-1 timing: on par with the exact kernel (0.33-0.36 vs 0.31-0.32 ms on uniform RoIs, 0.44-0.45 vs
    0.46-0.52 ms on RPN-like ones at [2,1024,50,84], R=1024) -- both sit on the 0.8 MB/RoI output write.  Falls back to the exact kernel for maps below
    16 x 16 or pooled sizes above 16 x 16.  Finite maps only: a window is read in 16-cell block footprints whose cells outside
    the window meet zero weights, so a NaN or an infinity anywhere in a block reaches the bins (0 * NaN); the exact kernel
    reads only the cells its taps touch."""
    return _roi_align_forward(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio, False)


def _roi_align_forward_strided(name, input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio, bin_stride, pair):
    """The one strided pooler, ``ovis_roi_align_forward_strided_from_nhwc_f32``.  It reads NHWC memory: a channels-last
    ``input`` (the NCHW view of the trunk's NHWC result) is pooled in place, any other layout is copied to channels-last
    first.  Returns (fp32 NHWC bins or pair rows, (oh, ow))."""
    _check_dev(input, "input")
    rois = _dev(rois, "rois")
    if rois.dim() != 2 or rois.size(1) != 5 or input.dim() != 4:
        raise RuntimeError(f"{name}: expected input [N,C,H,W] and rois [R,5]")
    n, c, h, w = input.shape
    r = rois.size(0)
    s = bin_stride
    oh, ow = -(-pooled_height // s), -(-pooled_width // s)
    if not pair and c % 4:
        # the kernels pool float4 channel groups; other channel counts (tests only) take the definition of the op
        full = roi_align_forward(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio)
        return full[:, :, ::s, ::s].permute(0, 2, 3, 1).contiguous(), (oh, ow)
    if pair:
        out = torch.empty((r * oh * ow, 2 * c), dtype=torch.bfloat16, device=input.device)
    else:
        out = torch.empty((r, oh, ow, c), dtype=input.dtype, device=input.device)
    if out.numel():
        if not (input.permute(0, 2, 3, 1).is_contiguous() and input.data_ptr() % 16 == 0):
            input = input.contiguous(memory_format=torch.channels_last)
            if input.data_ptr() % 16:
                input = input.clone()
        with _on(input.device):
            rc = _L.ovis_roi_align_forward_strided_from_nhwc_f32(input.data_ptr(), rois.data_ptr(), out.data_ptr(), r, n, c, h, w,
                                                                 pooled_height, pooled_width, s, spatial_scale,
                                                                 sampling_ratio, int(pair), _stream())
        _lib.check(rc, name)   # pair rows need channels % 32 == 0: OVIS_ERANGE otherwise
    return out, (oh, ow)


def roi_align_forward_strided_nhwc(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio, bin_stride):
    """Extension: bins (bin_stride*i, bin_stride*j) only, as [R, ceil(PH/s), ceil(PW/s), C] (NHWC); bit-identical to
    ``roi_align_forward(...)[:, :, ::s, ::s].permute(0, 2, 3, 1)``.  A channels-last ``input`` is pooled in place, any
    other layout through one copy to channels-last (``_roi_align_forward_strided``)."""
    return _roi_align_forward_strided("roi_align_forward_strided_nhwc", input, rois, spatial_scale, pooled_height, pooled_width,
                                      sampling_ratio, bin_stride, False)[0]


def roi_align_forward_strided_pair(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio, bin_stride):
    """``roi_align_forward_strided_nhwc`` written in pair layout: [R*oh*ow, 2*C] bf16 (exactly ``split_pair`` of the fp32
    bins), the operand of the res5 head's first split GEMM.  Returns (pair rows, (oh, ow)).  C % 32 == 0."""
    return _roi_align_forward_strided("roi_align_forward_strided_pair", input, rois, spatial_scale, pooled_height, pooled_width,
                                      sampling_ratio, bin_stride, True)


def _roi_align_backward(name, entry, ws_query, grad, rois, batch_size, channels, height, width, tail, none_if_unsupported):
    """What the three backward shims share: grad_input [N, C, H, W] and the plan workspace (``ws_query``: the size query and
    its arguments behind the RoI count) are allocated, ``entry`` is launched (``tail``: its arguments between width and the
    workspace), and OVIS_ERANGE comes back as None where the shim's contract says so."""
    r = rois.size(0)
    gin = torch.empty((batch_size, channels, height, width), dtype=grad.dtype, device=grad.device)
    if gin.numel() == 0:
        return gin
    with _on(grad.device):
        nbytes = ws_query[0](r, *ws_query[1:])
        ws = _workspace(nbytes, grad.device, at_least=1)
        rc = entry(grad.data_ptr(), rois.data_ptr(), gin.data_ptr(), r, batch_size, channels, height, width, *tail,
                   ws.data_ptr(), nbytes, _stream())
    if none_if_unsupported and rc == _lib.OVIS_ERANGE:
        return None
    _lib.check(rc, name)
    return gin


def roi_align_backward(grad, rois, spatial_scale, pooled_height, pooled_width, batch_size, channels, height,
                       width, sampling_ratio):
    if not grad.is_cuda:
        return _cpu.roi_align_backward(grad, rois, spatial_scale, pooled_height, pooled_width, batch_size, channels, height,
                                       width, sampling_ratio)
    grad, rois = _dev(grad, "grad"), _dev(rois, "rois")
    # plane-owner MFMA kernel when the H x W plane fits LDS (needs a per-call table workspace); the
    # library falls back to the window-gather + atomic kernel for larger maps
    return _roi_align_backward("roi_align_backward", _L.ovis_roi_align_backward_ws_f32,
                               (_L.ovis_roi_align_backward_workspace_bytes, batch_size, height, width), grad, rois,
                               batch_size, channels, height, width,
                               (pooled_height, pooled_width, spatial_scale, sampling_ratio), False)


def roi_align_backward_strided(grad, rois, spatial_scale, pooled_height, pooled_width, batch_size, channels, height,
                               width, sampling_ratio, bin_stride):
    """Backward of ``roi_align_forward_strided_nhwc``: ``grad`` [R, C, ceil(PH/s), ceil(PW/s)] (the gradient of the bins
    the strided pooler produced) -> grad_input [N, C, H, W].  Returns None when the plane-owner kernel does not cover the
    shape (the caller scatters into a full tile and uses ``roi_align_backward``)."""
    grad, rois = _dev(grad, "grad"), _dev(rois, "rois")
    return _roi_align_backward("roi_align_backward_strided", _L.ovis_roi_align_backward_strided_ws_f32,
                               (_L.ovis_roi_align_backward_workspace_bytes, batch_size, height, width), grad, rois,
                               batch_size, channels, height, width,
                               (pooled_height, pooled_width, bin_stride, spatial_scale, sampling_ratio), True)


def roi_align_backward_strided_nhwc(grad_nhwc, rois, spatial_scale, pooled_height, pooled_width, batch_size, channels,
                                    height, width, sampling_ratio, bin_stride):
    """Backward of ``roi_align_forward_strided_nhwc`` from the NHWC gradient itself: ``grad_nhwc`` [R, ceil(PH/s), ceil(PW/s), C]
    contiguous (as the res5 head's data-gradient GEMM leaves it) -> grad_input [N, C, H, W].  The library re-lays it into
    pre-split bf16 hi | lo tiles (no permute copy here, no split arithmetic in the plane-owner kernel).  Returns None when the
    shape is not covered (tiles above 8 x 8, planes that do not fit): the caller uses ``roi_align_backward_strided``."""
    grad_nhwc, rois = _dev(grad_nhwc, "grad"), _dev(rois, "rois")
    r, th, tw, c = grad_nhwc.shape
    if c != channels or r != rois.size(0):
        raise RuntimeError(f"roi_align_backward_strided_nhwc: gradient {tuple(grad_nhwc.shape)} for {rois.size(0)} RoIs x {channels} channels")
    if th > 8 or tw > 8:
        return None
    return _roi_align_backward("roi_align_backward_strided_nhwc", _L.ovis_roi_align_backward_strided_nhwc_ws_f32,
                               (_L.ovis_roi_align_backward_strided_nhwc_workspace_bytes, batch_size, channels, height, width),
                               grad_nhwc, rois, batch_size, channels, height, width,
                               (pooled_height, pooled_width, bin_stride, spatial_scale, sampling_ratio), True)


# ---- NMS (csrc/nms.h:10-28) -------------------------------------------------------------------
NMS_MAX_CANDIDATES = _lib.OVIS_NMS_MAX_CANDIDATES  # what one nms / nms_grouped call accepts


def _nms_padded(dets, scores, groups, threshold, ge_mode):
    """``ovis_nms_f32``, or ``ovis_nms_grouped_f32`` when ``groups`` is given."""
    what = "nms" if groups is None else "nms_grouped"
    dets, scores = _dev(dets, "dets"), _dev(scores, "scores")
    if groups is not None:
        groups = _dev(groups.to(torch.int32), "groups", torch.int32)
    k = dets.size(0)
    keep = torch.empty((k,), dtype=torch.int64, device=dets.device)
    num = torch.zeros((1,), dtype=torch.int32, device=dets.device)
    if k == 0:
        return keep, num
    if dets.dim() != 2 or dets.size(1) != 4 or scores.numel() != k or (groups is not None and groups.numel() != k):
        raise RuntimeError(f"{what}: expected dets [K,4]" + (" and scores [K]" if groups is None else ", scores [K] and groups [K]"))
    with _on(dets.device):
        nbytes = _L.ovis_nms_workspace_bytes(k)
        ws = _workspace(nbytes, dets.device)
        tail = (k, threshold, int(bool(ge_mode)), _ptr(ws), nbytes, keep.data_ptr(), num.data_ptr(), _stream())
        if groups is None:
            rc = _L.ovis_nms_f32(dets.data_ptr(), scores.data_ptr(), *tail)
        else:
            rc = _L.ovis_nms_grouped_f32(dets.data_ptr(), scores.data_ptr(), groups.data_ptr(), *tail)
    _lib.check(rc, what)
    return keep, num


def nms_padded(dets, scores, threshold, ge_mode=False):
    """Sync-free form: returns (keep[K] int64 -- first n entries valid, ascending; n as a
    1-element int32 device tensor).  Extension of the reference API for device pipelines."""
    if not dets.is_cuda:
        return _cpu.nms_padded(dets, scores, threshold)
    return _nms_padded(dets, scores, None, threshold, ge_mode)


def nms_grouped_padded(dets, scores, groups, threshold, ge_mode=False):
    """NMS inside every group of boxes in one launch (groups [K] integer labels): (keep[K] int64 -- first n entries
    valid, ascending indices into the K candidates; n as a 1-element int32 device tensor).  Equals ``nms`` run on
    every group separately (the per-class loop of box_head/inference.py:137-150)."""
    return _nms_padded(dets, scores, groups, threshold, ge_mode)


def nms_grouped(dets, scores, groups, threshold):
    keep, num = nms_grouped_padded(dets, scores, groups, threshold)
    return keep[: int(num.item())]


def nms(dets, scores, threshold):
    if dets.is_cuda and dets.numel() == 0:
        # the reference returns a CPU tensor for the empty case (csrc/nms.h:17-18)
        return torch.empty((0,), dtype=torch.int64, device="cpu")
    keep, num = nms_padded(dets, scores, threshold)
    return keep[: int(num.item())]


def nms_presorted_batched(boxes, drop, threshold, below=0, ge_mode=False):
    """NMS of every image's score-sorted candidates in one mask + one reduce launch (``ovis_nms_presorted_batched_f32``):
    boxes [N, K, 4] in descending score order, drop [N, K] int32 (negative = removed in front of the NMS) or None ->
    (keep [N, K] int64: per image the survivors' indices ascending, zeros behind them; counts [N, 2] int32 = number of
    survivors, number of survivors with index < ``below``)."""
    boxes = _dev(boxes, "boxes")
    n, k = boxes.shape[0], boxes.shape[1]
    keep = torch.empty((n, k), dtype=torch.int64, device=boxes.device)
    counts = torch.zeros((n, 2), dtype=torch.int32, device=boxes.device)
    if n == 0 or k == 0:
        return keep, counts
    if boxes.dim() != 3 or boxes.size(2) != 4:
        raise RuntimeError("nms_presorted_batched: expected boxes [N,K,4]")
    if drop is not None:
        drop = _dev(drop, "drop", torch.int32)
        if drop.shape != (n, k):
            raise RuntimeError("nms_presorted_batched: drop must be [N,K] int32")
    with _on(boxes.device):
        nbytes = _nms_presorted_ws_bytes(n, k)
        ws = _workspace(nbytes, boxes.device)
        rc = _L.ovis_nms_presorted_batched_f32(boxes.data_ptr(), _ptr(drop), n, k, threshold, int(bool(ge_mode)), int(below),
                                               _ptr(ws), nbytes, keep.data_ptr(), counts.data_ptr(), _stream())
    _lib.check(rc, "nms_presorted_batched")
    return keep, counts


def topk_sorted(scores, k):
    """``scores.topk(k, dim=1, sorted=True)`` of a [N, A] score matrix in three launches (``ovis_topk_sorted_f32``: one device
    radix sort of the batch; rpn/inference.py:95) -> (values [N, k] descending, indices [N, k] int64).  Equal scores come in
    ascending index order."""
    if not scores.is_cuda or scores.dtype != torch.float32 or scores.dim() != 2:
        raise RuntimeError("topk_sorted: float32 HIP tensor [N, A] expected (the product path has no CPU fallback)")
    n, a = scores.shape
    if not 0 <= k <= a:
        raise RuntimeError(f"topk_sorted: k = {k} out of range for rows of {a}")
    if a > 1 and scores.stride(1) != 1:
        scores = scores.contiguous()
    vals = torch.empty((n, k), dtype=torch.float32, device=scores.device)
    idx = torch.empty((n, k), dtype=torch.int64, device=scores.device)
    if n == 0 or k == 0:
        return vals, idx
    need = _topk_ws_bytes(n, a)
    if need == 0:
        raise RuntimeError(f"topk_sorted: unsupported size [{n}, {a}]")
    ws = _workspace(need, scores.device)
    with _on(scores.device):
        rc = _L.ovis_topk_sorted_f32(scores.data_ptr(), scores.stride(0) if n > 1 else a, n, a, k, vals.data_ptr(),
                                     idx.data_ptr(), ws.data_ptr(), need, _stream())
    _lib.check(rc, "topk_sorted")
    return vals, idx


def rpn_decode(box_regression, topk_idx, cell_anchors, image_wh, weights, xform_clip, min_size, anchor_stride):
    """Decode + clip + small-box flag of the top-k RPN candidates of a batch in one launch (``ovis_rpn_decode_f32``;
    rpn/inference.py:95-114).  box_regression [N, 4A, H, W] (any strides with stride(2) == W * stride(3): NCHW, or the
    NCHW view of an NHWC GEMM result), topk_idx [N, K] int64 into the (h, w, a) anchor order, cell_anchors [A, 4],
    image_wh [N, 2] float32 (width, height) -> (boxes [N, K, 4], drop [N, K] int32: -1 for boxes below min_size)."""
    if not box_regression.is_cuda or box_regression.dtype != torch.float32:
        raise RuntimeError("rpn_decode: float32 HIP tensor expected (the product path has no CPU fallback)")
    n, c4, h, w = box_regression.shape
    a = cell_anchors.shape[0]
    if c4 != 4 * a or topk_idx.dtype != torch.int64 or topk_idx.dim() != 2 or topk_idx.shape[0] != n:
        raise RuntimeError("rpn_decode: expected box_regression [N,4A,H,W], topk_idx [N,K] int64, cell_anchors [A,4]")
    if h > 1 and box_regression.stride(2) != w * box_regression.stride(3):
        box_regression = box_regression.contiguous()
    topk_idx = topk_idx.contiguous()
    cell_anchors = _dev(cell_anchors, "cell_anchors")
    image_wh = _dev(image_wh, "image_wh")
    k = topk_idx.shape[1]
    boxes = torch.empty((n, k, 4), dtype=torch.float32, device=box_regression.device)
    drop = torch.empty((n, k), dtype=torch.int32, device=box_regression.device)
    if n == 0 or k == 0:
        return boxes, drop
    wx, wy, ww, wh = weights
    with _on(box_regression.device):
        rc = _L.ovis_rpn_decode_f32(box_regression.data_ptr(), box_regression.stride(0), box_regression.stride(3),
                                    box_regression.stride(1), topk_idx.data_ptr(), cell_anchors.data_ptr(),
                                    image_wh.data_ptr(), n, k, a, w, float(anchor_stride), wx, wy, ww, wh, xform_clip,
                                    float(min_size), boxes.data_ptr(), drop.data_ptr(), _stream())
    _lib.check(rc, "rpn_decode")
    return boxes, drop


def box_decode(rel_codes, boxes, weights, xform_clip, rows_per_image=None, image_sizes=None):
    """``BoxCoder.decode`` (modeling/box_coder.py:49-95) in one launch (``ovis_box_decode_f32``): rel_codes [R, 4K] (any row
    stride), boxes [R, 4] -> [R, 4K].  With ``rows_per_image`` (ints, image-major rows) and ``image_sizes`` ((width, height)
    per image) every row is also clipped to its image (``BoxList.clip_to_image``, structures/bounding_box.py:214-225)."""
    if not rel_codes.is_cuda or rel_codes.dtype != torch.float32 or rel_codes.dim() != 2 or rel_codes.shape[1] % 4:
        raise RuntimeError("box_decode: rel_codes must be a float32 HIP tensor [R, 4K] (the product path has no CPU fallback)")
    if boxes.shape != (rel_codes.shape[0], 4):
        raise RuntimeError("box_decode: boxes must be [R, 4]")
    boxes = boxes.to(torch.float32)
    if rel_codes.stride(1) != 1:
        rel_codes = rel_codes.contiguous()
    if boxes.stride(1) != 1:
        boxes = boxes.contiguous()
    r, k = rel_codes.shape[0], rel_codes.shape[1] // 4
    out = torch.empty((r, 4 * k), dtype=torch.float32, device=rel_codes.device)
    if r == 0:
        return out
    n = 0 if rows_per_image is None else len(rows_per_image)
    wx, wy, ww, wh_ = weights
    # image sizes travel as kernel arguments, at most OVIS_BOX_DECODE_MAX_IMAGES per launch: rows are image-major, so a longer
    # batch is a few launches over consecutive row ranges (as ovis_rois_from_boxes_f32 does internally)
    if n and (len(image_sizes) != n or sum(int(c) for c in rows_per_image) != r):
        raise RuntimeError(f"box_decode: rows_per_image must list {r} rows over {n} images with one (width, height) each")
    i0 = row0 = 0
    with _on(rel_codes.device):
        while True:
            m = min(n - i0, _lib.OVIS_BOX_DECODE_MAX_IMAGES)
            counts = wh = None
            rows = r
            if n:
                cs = [int(c) for c in rows_per_image[i0:i0 + m]]
                rows = sum(cs)
                counts = (ctypes.c_int32 * m)(*cs)
                wh = (ctypes.c_float * (2 * m))(*[float(v) for size in image_sizes[i0:i0 + m] for v in size])
            if rows:
                rc = _L.ovis_box_decode_f32(rel_codes.data_ptr() + 4 * row0 * rel_codes.stride(0), rel_codes.stride(0),
                                            boxes.data_ptr() + 4 * row0 * boxes.stride(0), boxes.stride(0), rows, k, wx, wy,
                                            ww, wh_, xform_clip, m, counts, wh, out.data_ptr() + 16 * k * row0, _stream())
                _lib.check(rc, "box_decode")
            i0 += m
            row0 += rows
            if i0 >= n:
                break
    return out


def _merge_segments(segments, num_rows):
    """The (row_start, row_count, image, view_width, flip, ratio_w, ratio_h) records as checked python values: rows inside
    [0, num_rows), images 0, 1, ... in order, each with at least one segment.  Raises before anything is launched."""
    out, last = [], -1
    for k, seg in enumerate(segments):
        if len(seg) != 7:
            raise RuntimeError(f"merge_view_detections: segment {k} must be (row_start, row_count, image, view_width, flip, "
                               "ratio_w, ratio_h)")
        row_start, row_count, image, width = (int(v) for v in seg[:4])
        if row_start < 0 or row_count < 0 or row_start + row_count > num_rows:
            raise RuntimeError(f"merge_view_detections: segment {k} covers rows [{row_start}, {row_start + row_count}) of "
                               f"{num_rows}")
        if image not in (last, last + 1) or width < 0:
            raise RuntimeError(f"merge_view_detections: segment {k}: images must come in order 0, 1, ... (image-major, every "
                               f"image with a segment) and widths be >= 0; got image {image} after {last}, width {width}")
        last = image
        out.append((row_start, row_count, image, width, int(bool(seg[4])), float(seg[5]), float(seg[6])))
    return out, last + 1


def merge_view_detections(boxes, scores, segments, num_classes, score_thresh):
    """The candidate list of a batch's test-time-augmentation views (engine/bbox_aug.py:53-60 followed by the
    ``scores > thresh`` of box_head/inference.py:137-143), ``ovis_view_merge_*``: boxes [R, C, 4] / scores [R, C] float32,
    every view's class-specific detections in the view's own frame; ``segments``: one (row_start, row_count, image,
    view_width, flip, ratio_w, ratio_h) per (image, view), image-major then view order, rows contiguous, ``ratio_*`` =
    ``float(target) / float(view)`` (rounded to float32 here, as a float32 tensor times a python float does).
    -> (cand_boxes [K, 4], cand_scores [K], cand_group [K] int32 = image * C + class, offsets [B * C + 1] int32): every
    box flipped back (``BoxList.transpose(0)``) and scaled (``BoxList.resize``), the classes >= 1 with score > thresh (a NaN
    is not kept), ordered image, class, segment, row.  Device tensors: three launches per OVIS_VIEW_MERGE_MAX_SEGMENTS (64)
    segments -- a longer list is cut at image boundaries, one image may not have more views than that -- and ONE host read
    (K); host tensors: the BoxList route as the reference writes it (``_cpu.merge_view_detections``)."""
    if boxes.is_cuda != scores.is_cuda:
        raise RuntimeError("merge_view_detections: host and device tensors mixed in one call")
    c = int(num_classes)
    if (scores.dim() != 2 or scores.shape[1] != c or c < 1 or boxes.dim() != 3 or boxes.shape != (scores.shape[0], c, 4)
            or boxes.dtype != torch.float32 or scores.dtype != torch.float32):
        raise RuntimeError(f"merge_view_detections: expected float32 boxes [R, {c}, 4] and scores [R, {c}], got "
                           f"{boxes.dtype} {tuple(boxes.shape)} and {scores.dtype} {tuple(scores.shape)}")
    r = scores.shape[0]
    segs, b = _merge_segments(segments, r)
    if r * c >= 2 ** 31 or b * c >= 2 ** 31 - 1:
        raise RuntimeError("merge_view_detections: R * C and B * C must stay below 2^31")
    if not boxes.is_cuda:
        return _cpu.merge_view_detections(boxes, scores, segs, c, b, float(score_thresh))
    boxes, scores = _dev(boxes, "boxes"), _dev(scores, "scores")
    dev = boxes.device
    offsets = torch.empty((b * c + 1,), dtype=torch.int32, device=dev)
    # launches: whole images, at most OVIS_VIEW_MERGE_MAX_SEGMENTS segments each; (first segment, count, first count entry)
    per_image = [0] * b
    for seg in segs:
        per_image[seg[2]] += 1
    if b and max(per_image) > _lib.OVIS_VIEW_MERGE_MAX_SEGMENTS:
        raise RuntimeError(f"merge_view_detections: image {per_image.index(max(per_image))} has {max(per_image)} views, more "
                           f"than the {_lib.OVIS_VIEW_MERGE_MAX_SEGMENTS} segments of one launch")
    calls, first, entries, image = [], 0, 0, 0
    while image < b:
        n = 0
        while image < b and n + per_image[image] <= _lib.OVIS_VIEW_MERGE_MAX_SEGMENTS:
            n += per_image[image]
            image += 1
        part = segs[first:first + n]
        num = c * sum(max(1, -(-seg[1] // _lib.OVIS_VIEW_MERGE_TILE_ROWS)) for seg in part)
        ints = (ctypes.c_int32 * (5 * n))(*[int(v) for seg in part for v in seg[:5]])
        ratios = (ctypes.c_float * (2 * n))(*[v for seg in part for v in seg[5:]])
        calls.append((ints, ratios, n, entries, num))
        entries += num
        first += n
    counts = torch.empty((max(entries, 1),), dtype=torch.int32, device=dev)
    with _on(dev):
        stream = _stream()
        for ints, ratios, n, at, num in calls:
            _lib.check(_L.ovis_view_merge_count_f32(scores.data_ptr(), r, c, b, ints, ratios, n, score_thresh,
                                                    counts.data_ptr() + 4 * at, num, stream), "merge_view_detections (count)")
        _lib.check(_L.ovis_view_merge_scan_i32(counts.data_ptr(), entries, offsets.data_ptr() + 4 * b * c, stream),
                   "merge_view_detections (scan)")
        k = int(offsets[-1].item())   # the one host read: the outputs' size (nms_grouped needs K on the host as well)
        cand_boxes = torch.empty((k, 4), dtype=torch.float32, device=dev)
        cand_scores = torch.empty((k,), dtype=torch.float32, device=dev)
        cand_group = torch.empty((k,), dtype=torch.int32, device=dev)
        for ints, ratios, n, at, num in calls:
            _lib.check(_L.ovis_view_merge_scatter_f32(boxes.data_ptr(), scores.data_ptr(), r, c, b, ints, ratios, n,
                                                      score_thresh, counts.data_ptr() + 4 * at, num, k,
                                                      cand_boxes.data_ptr(), cand_scores.data_ptr(), cand_group.data_ptr(),
                                                      offsets.data_ptr(), stream), "merge_view_detections (scatter)")
    return cand_boxes, cand_scores, cand_group, offsets


def vote_boxes(cand_boxes, cand_scores, offsets, cand_group, kept, vote_thresh):
    """Box voting over the candidate list of ``merge_view_detections`` (Detectron's ``box_voting``, scoring method ID; not
    in the reference), ``ovis_vote_boxes_f32``: cand_boxes [K, 4] / cand_scores [K] float32, offsets [B * C + 1] and
    cand_group [K] int32, kept [D] int64 = the candidate indices of the detections the NMS kept -> [D, 4] float32, row j =
    sum s_k box_k / sum s_k over the candidates k of kept[j]'s own (image, class) run with IoU(box_kept[j], box_k) >=
    vote_thresh (the NMS's IoU expression and comparison).  One wavefront per detection and a fixed butterfly: the same bits
    on every call.  A kept index outside [0, K) or outside its group's run raises (the kernel reads nothing through it; the
    status costs ONE host read).  D == 0 or K == 0: an empty result, nothing launched (K == 0 with D > 0 raises).  Host
    tensors: ``libovis_cpu.so``, the same operations in the same order."""
    tensors = (cand_boxes, cand_scores, offsets, cand_group, kept)
    if len({t.is_cuda for t in tensors}) != 1:
        raise RuntimeError("vote_boxes: host and device tensors mixed in one call")
    k = cand_boxes.shape[0] if cand_boxes.dim() == 2 else -1
    if (k < 0 or cand_boxes.shape[1] != 4 or tuple(cand_scores.shape) != (k,) or tuple(cand_group.shape) != (k,)
            or offsets.dim() != 1 or offsets.numel() < 1 or kept.dim() != 1 or cand_boxes.dtype != torch.float32
            or cand_scores.dtype != torch.float32 or offsets.dtype != torch.int32 or cand_group.dtype != torch.int32
            or kept.dtype != torch.int64):
        raise RuntimeError("vote_boxes: expected float32 cand_boxes [K, 4] and cand_scores [K], int32 offsets [G + 1] and "
                           f"cand_group [K], int64 kept [D]; got {[(str(t.dtype), tuple(t.shape)) for t in tensors]}")
    d = kept.shape[0]
    if d and not k:
        raise RuntimeError(f"vote_boxes: {d} kept indices into an empty candidate list")
    if not cand_boxes.is_cuda:
        return _cpu.vote_boxes(*(t.contiguous() for t in tensors), float(vote_thresh))
    dev = cand_boxes.device
    out = torch.empty((d, 4), dtype=torch.float32, device=dev)
    if d == 0:
        return out
    cand_boxes = _dev(cand_boxes, "cand_boxes")
    cand_scores, offsets, cand_group, kept = (t.contiguous() for t in tensors[1:])
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(_L.ovis_vote_boxes_f32(cand_boxes.data_ptr(), cand_scores.data_ptr(), offsets.data_ptr(),
                                          cand_group.data_ptr(), k, offsets.numel() - 1, kept.data_ptr(), d,
                                          float(vote_thresh), out.data_ptr(), status.data_ptr(), _stream()), "vote_boxes")
    if int(status.item()):
        raise RuntimeError("vote_boxes: OVIS_ERANGE (a kept index outside the candidate list or outside its (image, class) run)")
    return out


SOFT_NMS_METHODS = {"linear": _lib.OVIS_SOFT_NMS_LINEAR, "gaussian": _lib.OVIS_SOFT_NMS_GAUSSIAN,
                    "hard": _lib.OVIS_SOFT_NMS_HARD}


def soft_nms(cand_boxes, cand_scores, offsets, method="linear", nms_thresh=0.5, sigma=0.5, min_score=0.0):
    """Soft-NMS (Bodla et al., ICCV 2017; not in the reference) over the runs of a candidate list, ``ovis_soft_nms_f32``:
    cand_boxes [K, 4] / cand_scores [K] float32 and offsets [G + 1] int32 as ``merge_view_detections`` returns them (run g =
    candidates offsets[g] .. offsets[g + 1], back to back from 0 to K) -> soft_scores [K] float32.  Per run, while a candidate
    is alive the one with the largest working score (ties: the lower index) is selected with that score, and every other
    alive candidate's score is multiplied by a weight of its IoU with it (the NMS's float32 IoU): ``linear`` 1 - IoU above
    ``nms_thresh``, ``gaussian`` exp(-IoU^2 / sigma) (a float64 exponential rounded once), ``hard`` 0 above ``nms_thresh``; a
    score that falls below ``min_score`` (strictly; or to exactly 0) discards its candidate.  soft_scores[k] = the final score
    of a selected candidate (> 0), 0 for a discarded one; ``hard`` with min_score 0 keeps what ``nms`` keeps.  The rule in
    full: include/ovis_hip.h.  One launch whatever the run lengths, the same bits on every call; malformed offsets raise
    (the kernel reads nothing through them; the status costs ONE host read).  K == 0: an empty result, nothing launched.
    Host tensors: ``libovis_cpu.so``, the same operations, the same bits."""
    tensors = (cand_boxes, cand_scores, offsets)
    if len({t.is_cuda for t in tensors}) != 1:
        raise RuntimeError("soft_nms: host and device tensors mixed in one call")
    if method not in SOFT_NMS_METHODS:
        raise ValueError(f"soft_nms: method must be one of {sorted(SOFT_NMS_METHODS)}, got {method!r}")
    if not float(sigma) > 0.0 or not float(min_score) >= 0.0:
        raise ValueError(f"soft_nms: sigma must be > 0 and min_score >= 0, got {sigma} and {min_score}")
    k = cand_boxes.shape[0] if cand_boxes.dim() == 2 else -1
    if (k < 0 or cand_boxes.shape[1] != 4 or tuple(cand_scores.shape) != (k,) or offsets.dim() != 1 or offsets.numel() < 1
            or cand_boxes.dtype != torch.float32 or cand_scores.dtype != torch.float32 or offsets.dtype != torch.int32):
        raise RuntimeError("soft_nms: expected float32 cand_boxes [K, 4] and cand_scores [K] and int32 offsets [G + 1]; got "
                           f"{[(str(t.dtype), tuple(t.shape)) for t in tensors]}")
    code = SOFT_NMS_METHODS[method]
    if k and offsets.numel() == 1:
        raise RuntimeError(f"soft_nms: {k} candidates and no run (offsets must end at the number of candidates)")
    if not cand_boxes.is_cuda:
        return _cpu.soft_nms(*(t.contiguous() for t in tensors), code, nms_thresh, sigma, min_score)
    dev = cand_boxes.device
    out = torch.empty((k,), dtype=torch.float32, device=dev)
    if k == 0:
        return out
    cand_boxes = _dev(cand_boxes, "cand_boxes")
    cand_scores, offsets = cand_scores.contiguous(), offsets.contiguous()
    status = torch.zeros((1,), dtype=torch.int32, device=dev)
    with _on(dev):
        _lib.check(_L.ovis_soft_nms_f32(cand_boxes.data_ptr(), cand_scores.data_ptr(), offsets.data_ptr(), k,
                                        offsets.numel() - 1, code, float(nms_thresh), float(sigma), float(min_score),
                                        out.data_ptr(), status.data_ptr(), _stream()), "soft_nms")
    if int(status.item()):
        raise RuntimeError("soft_nms: OVIS_ERANGE (malformed offsets: not 0 first, decreasing, negative, or not ending at the "
                           "number of candidates)")
    return out


def average_view_masks(maps, flips):
    """The mean of the views' mask maps (``ovis_average_view_masks_f32``; not in the reference): maps [V, D, 1, M, M]
    float32, ``flips``: V booleans -> [D, 1, M, M] = (((m_0 + m_1) + m_2) + ...) / float(V) in float32, the columns of a
    mirrored view reversed first.  A division: one unflipped view returns its input bit for bit.  V <= 64.  Host tensors:
    ``libovis_cpu.so``."""
    flips = [bool(f) for f in flips]
    if (maps.dim() != 5 or maps.shape[2] != 1 or maps.shape[3] != maps.shape[4] or maps.shape[3] < 1 or maps.shape[0] < 1
            or maps.dtype != torch.float32 or len(flips) != maps.shape[0]):
        raise RuntimeError(f"average_view_masks: expected float32 maps [V >= 1, D, 1, M, M] and V flips, got {maps.dtype} "
                           f"{tuple(maps.shape)} and {len(flips)} flips")
    v, d, _, m, _ = maps.shape
    if v > 64:
        raise RuntimeError(f"average_view_masks: OVIS_ERANGE ({v} views, at most 64)")
    flip_bits = sum(1 << i for i, f in enumerate(flips) if f)
    maps = maps.contiguous()
    if not maps.is_cuda:
        return _cpu.average_view_masks(maps, flip_bits)
    out = torch.empty((d, 1, m, m), dtype=torch.float32, device=maps.device)
    if d:
        with _on(maps.device):
            _lib.check(_L.ovis_average_view_masks_f32(maps.data_ptr(), v, d, m, flip_bits, out.data_ptr(), _stream()),
                       "average_view_masks")
    return out


def rois_from_boxes(boxes, image_ids=None):
    """``Pooler.convert_to_roi_format`` (modeling/poolers.py:73-86) in one launch (``ovis_rois_from_boxes_f32``): a list of
    per-image [n_i, 4] float32 HIP tensors -> [sum n_i, 5] rows (image index, x1, y1, x2, y2); the image index of list
    entry i is ``image_ids[i]`` (default i)."""
    if not boxes:
        raise RuntimeError("rois_from_boxes: at least one image expected")
    boxes = [_dev(b, "boxes") for b in boxes]
    if any(b.dim() != 2 or b.shape[1] != 4 for b in boxes):
        raise RuntimeError("rois_from_boxes: [n, 4] tensors expected")
    n = len(boxes)
    rois = torch.empty((sum(b.shape[0] for b in boxes), 5), dtype=torch.float32, device=boxes[0].device)
    if rois.shape[0]:
        ptrs = (ctypes.c_void_p * n)(*[b.data_ptr() if b.shape[0] else None for b in boxes])
        counts = (ctypes.c_int32 * n)(*[b.shape[0] for b in boxes])
        ids = None if image_ids is None else (ctypes.c_int32 * n)(*[int(i) for i in image_ids])
        with _on(rois.device):
            rc = _L.ovis_rois_from_boxes_f32(ptrs, counts, ids, n, rois.data_ptr(), _stream())
        _lib.check(rc, "rois_from_boxes")
    return rois


def smooth_l1_picked_fwd_bwd(box_regression, regression_targets, positives, labels, column0, beta, denominator,
                             need_grad=True):
    """Box-regression loss of the box head (roi_heads/box_head/loss.py:147-170) with its gradient in one pass
    (``ovis_smooth_l1_picked_fwd_bwd_f32``): sum over the positives of smooth_l1(box_regression[p, col0 + c] -
    regression_targets[p, c]) / denominator, col0 = 4 * labels[p] (``labels`` given) or ``column0``.
    -> (loss scalar tensor, d loss / d box_regression [R, C] or None)."""
    if not box_regression.is_cuda or box_regression.dtype != torch.float32 or box_regression.dim() != 2:
        raise RuntimeError("smooth_l1_picked: float32 HIP tensor [R, C] expected (the product path has no CPU fallback)")
    if box_regression.stride(1) != 1:
        box_regression = box_regression.contiguous()
    regression_targets = _dev(regression_targets, "regression_targets")
    positives = _dev(positives, "positives", torch.int64)
    labels = None if labels is None else _dev(labels, "labels", torch.int64)
    r, c = box_regression.shape
    loss = torch.empty((1,), dtype=torch.float32, device=box_regression.device)
    grad = torch.empty((r, c), dtype=torch.float32, device=box_regression.device) if need_grad else None
    with _on(box_regression.device):
        rc = _L.ovis_smooth_l1_picked_fwd_bwd_f32(box_regression.data_ptr(), box_regression.stride(0), r, c,
                                                  regression_targets.data_ptr(), regression_targets.stride(0),
                                                  positives.data_ptr(), _ptr(labels), positives.numel(), column0, beta,
                                                  float(denominator), loss.data_ptr(), _ptr(grad), _stream())
    _lib.check(rc, "smooth_l1_picked_fwd_bwd")
    return loss[0], grad


# ---- sigmoid focal loss (csrc/SigmoidFocalLoss.h:10-41) ----------------------------------------
def sigmoid_focalloss_forward(logits, targets, num_classes, gamma, alpha):
    logits, targets = _dev(logits, "logits"), _dev(targets, "targets", torch.int32)
    if logits.dim() != 2:
        raise RuntimeError("logits should be NxClass")
    losses = torch.empty_like(logits)
    if losses.numel() == 0:
        return losses
    with _on(logits.device):
        rc = _L.ovis_sigmoid_focal_loss_forward_f32(logits.data_ptr(), targets.data_ptr(), losses.data_ptr(),
                                                    logits.size(0), logits.size(1), gamma, alpha, _stream())
    _lib.check(rc, "sigmoid_focalloss_forward")
    return losses


def sigmoid_focalloss_backward(logits, targets, d_losses, num_classes, gamma, alpha):
    logits, targets = _dev(logits, "logits"), _dev(targets, "targets", torch.int32)
    d_losses = _dev(d_losses, "d_losses")
    if logits.dim() != 2 or logits.size(1) != num_classes:
        raise RuntimeError("logits.size(1) should be num_classes")
    d_logits = torch.zeros_like(logits)
    if d_logits.numel() == 0:
        return d_logits
    with _on(logits.device):
        rc = _L.ovis_sigmoid_focal_loss_backward_f32(logits.data_ptr(), targets.data_ptr(), d_losses.data_ptr(),
                                                     d_logits.data_ptr(), logits.size(0), num_classes, gamma,
                                                     alpha, _stream())
    _lib.check(rc, "sigmoid_focalloss_backward")
    return d_logits


# ---- ROIPool (csrc/ROIPool.h:11-48) ---------------------------------------------------------------
def roi_pool_forward(input, rois, spatial_scale, pooled_height, pooled_width):
    """The reference's `_C.roi_pool_forward`: (output, argmax int32), exact vs cuda/ROIPool_cuda.cu:17-77."""
    input, rois = _dev(input, "input"), _dev(rois, "rois")
    if rois.dim() != 2 or rois.size(1) != 5 or input.dim() != 4:
        raise RuntimeError("roi_pool_forward: expected input [N,C,H,W] and rois [R,5]")
    n, c, h, w = input.shape
    r = rois.size(0)
    out = torch.empty((r, c, pooled_height, pooled_width), dtype=input.dtype, device=input.device)
    argmax = torch.zeros((r, c, pooled_height, pooled_width), dtype=torch.int32, device=input.device)
    if out.numel():
        with _on(input.device):
            rc = _L.ovis_roi_pool_forward_f32(input.data_ptr(), rois.data_ptr(), out.data_ptr(), argmax.data_ptr(), r, n, c, h,
                                              w, pooled_height, pooled_width, spatial_scale, _stream())
        _lib.check(rc, "roi_pool_forward")
    return out, argmax


def roi_pool_backward(grad, input, rois, argmax, spatial_scale, pooled_height, pooled_width, batch_size, channels,
                      height, width):
    """The reference's `_C.roi_pool_backward` (cuda/ROIPool_cuda.cu:80-108); `input` / `spatial_scale` are part of
    the reference signature and unused, as upstream."""
    grad, rois = _dev(grad, "grad"), _dev(rois, "rois")
    argmax = argmax.to(torch.int32).contiguous()
    gin = torch.empty((batch_size, channels, height, width), dtype=grad.dtype, device=grad.device)
    if gin.numel():
        with _on(grad.device):
            rc = _L.ovis_roi_pool_backward_f32(grad.data_ptr(), argmax.data_ptr(), rois.data_ptr(), gin.data_ptr(),
                                               rois.size(0), batch_size, channels, height, width, pooled_height,
                                               pooled_width, _stream())
        _lib.check(rc, "roi_pool_backward")
    return gin


# ---- deformable position-sensitive RoI pooling (csrc/deform_pool.h:11-70) -----------------------------
def _psroi_dims(input, bbox, trans, out, no_trans):
    for t, name in ((input, "input"), (bbox, "bbox"), (out, "out")):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise RuntimeError(f"deform_psroi_pooling: {name} must be a float32 HIP tensor: this package has no CPU implementation")
    if not input.is_contiguous():
        raise RuntimeError("input tensor has to be contiguous")  # deform_pool_cuda.cu:45
    if bbox.size(0) != out.size(0):
        raise RuntimeError(f"Output shape and bbox number wont match: ({out.size(0)} vs {bbox.size(0)}).")
    channels_trans = 2 if no_trans else trans.size(1)
    return input.size(0), input.size(1), input.size(2), input.size(3), channels_trans, bbox.size(0)


def deform_psroi_pooling_forward(input, bbox, trans, out, top_count, no_trans, spatial_scale, output_dim, group_size,
                                 pooled_size, part_size, sample_per_part, trans_std):
    """The reference's `_C.deform_psroi_pooling_forward` (deform_pool.h:11-38): fills ``out`` and ``top_count`` in place."""
    batch, channels, height, width, channels_trans, n = _psroi_dims(input, bbox, trans, out, no_trans)
    bbox = bbox.contiguous()
    tr = 0 if no_trans else _dev(trans, "trans").data_ptr()
    if not (out.is_contiguous() and top_count.is_contiguous() and top_count.dtype == torch.float32):
        raise RuntimeError("deform_psroi_pooling_forward: out / top_count must be contiguous float32")
    with _on(input.device):
        rc = _L.ovis_deform_psroi_pool_forward_f32(input.data_ptr(), bbox.data_ptr(), tr, out.data_ptr(),
                                                   top_count.data_ptr(), n, batch, channels, height, width, channels_trans,
                                                   int(bool(no_trans)), spatial_scale, output_dim, group_size,
                                                   pooled_size, part_size, sample_per_part, trans_std, _stream())
    _lib.check(rc, "deform_psroi_pooling_forward")


def deform_psroi_pooling_backward(out_grad, input, bbox, trans, top_count, input_grad, trans_grad, no_trans,
                                  spatial_scale, output_dim, group_size, pooled_size, part_size, sample_per_part,
                                  trans_std):
    """The reference's `_C.deform_psroi_pooling_backward` (deform_pool.h:40-70): ACCUMULATES into ``input_grad`` and
    ``trans_grad`` (zero-filled by the caller, deform_pool_func.py:68-70)."""
    if not out_grad.is_contiguous():
        raise RuntimeError("out_grad tensor has to be contiguous")  # deform_pool_cuda.cu:71
    batch, channels, height, width, channels_trans, n = _psroi_dims(input, bbox, trans, out_grad, no_trans)
    bbox = bbox.contiguous()
    if not (input_grad.is_cuda and input_grad.is_contiguous() and input_grad.shape == input.shape):
        raise RuntimeError("deform_psroi_pooling_backward: input_grad must be a contiguous HIP tensor shaped like input")
    tr = tg = 0
    if not no_trans:
        tr = _dev(trans, "trans").data_ptr()
        if not (trans_grad.is_cuda and trans_grad.is_contiguous() and trans_grad.shape == trans.shape):
            raise RuntimeError("deform_psroi_pooling_backward: trans_grad must be a contiguous HIP tensor shaped like trans")
        tg = trans_grad.data_ptr()
    with _on(input.device):
        rc = _L.ovis_deform_psroi_pool_backward_f32(out_grad.data_ptr(), top_count.data_ptr(), input.data_ptr(),
                                                    bbox.data_ptr(), tr, input_grad.data_ptr(), tg, n, batch, channels,
                                                    height, width, channels_trans, int(bool(no_trans)), spatial_scale,
                                                    output_dim, group_size, pooled_size, part_size, sample_per_part,
                                                    trans_std, _stream())
    _lib.check(rc, "deform_psroi_pooling_backward")


# ---- cross-modal head + student losses (extensions beyond vision.cpp; include/ovis_hip.h) --------------
def split_bf16x3(x, mode):
    """x [rows, cols] f32 (row-strided view ok) -> [rows, 3*cols] bf16, rows = [hi|hi|lo] (mode 0) / [hi|lo|hi]
    (mode 1).  See include/ovis_hip.h."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise RuntimeError("split_bf16x3: 2-D float32 HIP tensor expected")
    if x.stride(1) != 1:
        x = x.contiguous()
    rows, cols = x.shape
    out = torch.empty((rows, 3 * cols), dtype=torch.bfloat16, device=x.device)
    if out.numel() == 0:
        return out
    with _on(x.device):
        rc = _L.ovis_split_bf16x3_f32(x.data_ptr(), x.stride(0), out.data_ptr(), rows, cols, mode, _stream())
    _lib.check(rc, "split_bf16x3")
    return out


def im2col_split_bf16x3(x, kh, kw, flip=False):
    """x [R, H, W, C] f32 contiguous (NHWC) -> [R*H*W, 3*kh*kw*C] bf16 rows [hi taps | hi taps | lo taps]
    (stride 1, zero "same" padding; flip = taps in reverse order).  See include/ovis_hip.h."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise RuntimeError("im2col_split_bf16x3: contiguous [R,H,W,C] float32 HIP tensor expected")
    r, h, w, c = x.shape
    out = torch.empty((r * h * w, 3 * kh * kw * c), dtype=torch.bfloat16, device=x.device)
    if out.numel() == 0:
        return out
    with _on(x.device):
        rc = _L.ovis_im2col_split_bf16x3_f32(x.data_ptr(), out.data_ptr(), r, h, w, c, kh, kw, int(bool(flip)), _stream())
    _lib.check(rc, "im2col_split_bf16x3")
    return out


def match_encode(gt_boxes, gt_labels, proposals, high, low, weights=None, between_keeps_label=False):
    """IoU match + labels (+ box-delta targets when ``weights`` is given) in one launch; see include/ovis_hip.h.
    Returns (matched_idx int64 [P], labels int64 [P], regression_targets f32 [P,4] or None)."""
    gt_boxes, proposals = _dev(gt_boxes, "gt_boxes"), _dev(proposals, "proposals")
    gt_labels = gt_labels.to(torch.int64).contiguous()
    g, p = gt_boxes.shape[0], proposals.shape[0]
    if g == 0:
        raise ValueError("No ground-truth boxes available for one of the images during training")
    idx = torch.empty((p,), dtype=torch.int64, device=proposals.device)
    lab = torch.empty((p,), dtype=torch.int64, device=proposals.device)
    reg = torch.empty((p, 4), dtype=torch.float32, device=proposals.device) if weights is not None else None
    if p:
        wx, wy, ww, wh = weights if weights is not None else (1.0, 1.0, 1.0, 1.0)
        with _on(proposals.device):
            rc = _L.ovis_match_encode_f32(gt_boxes.data_ptr(), gt_labels.data_ptr(), proposals.data_ptr(), g, p, high, low,
                                          int(bool(between_keeps_label)), wx, wy, ww, wh, idx.data_ptr(), lab.data_ptr(),
                                          _ptr(reg), _stream())
        _lib.check(rc, "match_encode")
    return idx, lab, reg


def rpn_match_encode(gt_boxes, anchors, visibility, high_threshold, low_threshold, allow_low_quality_matches, weights):
    """The RPN's per-image targets in two launches (``ovis_rpn_match_encode_f32``; rpn/loss.py:21-89): gt_boxes [G, 4],
    anchors [A, 4], visibility [A] bool -> (labels [A] int64: 1 / 0 / -1, regression targets [A, 4])."""
    gt_boxes, anchors = _dev(gt_boxes, "gt_boxes"), _dev(anchors, "anchors")
    if not (visibility.is_cuda and visibility.dtype == torch.bool and visibility.shape == (anchors.shape[0],)):
        raise RuntimeError("rpn_match_encode: visibility must be a bool HIP tensor [A]")
    visibility = visibility.contiguous()
    g, a = gt_boxes.shape[0], anchors.shape[0]
    if g == 0:
        raise ValueError("No ground-truth boxes available for one of the images during training")
    labels = torch.empty((a,), dtype=torch.int64, device=anchors.device)
    reg = torch.empty((a, 4), dtype=torch.float32, device=anchors.device)
    scratch = torch.empty((g,), dtype=torch.int32, device=anchors.device)
    wx, wy, ww, wh = weights
    with _on(anchors.device):
        rc = _L.ovis_rpn_match_encode_f32(gt_boxes.data_ptr(), anchors.data_ptr(), visibility.data_ptr(), g, a, high_threshold,
                                          low_threshold, int(bool(allow_low_quality_matches)), wx, wy, ww, wh, scratch.data_ptr(),
                                          labels.data_ptr(), reg.data_ptr(), _stream())
    _lib.check(rc, "rpn_match_encode")
    return labels, reg


def project_masks(masks, gt_index, boxes, resolution):
    """masks [G,H,W] bool / uint8, gt_index [P] int64, boxes [P,4] -> [P, M, M] f32 mask targets (one launch)."""
    if not (masks.is_cuda and masks.dim() == 3 and masks.dtype in (torch.bool, torch.uint8)):
        raise RuntimeError("project_masks: [G,H,W] bool / uint8 HIP tensor expected")
    masks = masks.contiguous()
    boxes = _dev(boxes, "boxes")
    gt_index = gt_index.to(torch.int64).contiguous()
    p = boxes.shape[0]
    out = torch.empty((p, resolution, resolution), dtype=torch.float32, device=boxes.device)
    if p:
        with _on(boxes.device):
            rc = _L.ovis_project_masks_f32(masks.data_ptr(), gt_index.data_ptr(), boxes.data_ptr(), p, masks.shape[1],
                                           masks.shape[2], resolution, int(masks.dtype == torch.bool), out.data_ptr(),
                                           _stream())
        _lib.check(rc, "project_masks")
    return out


def sample_fg_bg(labels, batch_size, max_positives, seed):
    """fg / bg sampling of one image on the device (``ovis_sample_fg_bg``; balanced_positive_negative_sampler.py:19-68):
    labels [P] int64 -> (selected [batch_size] int64: chosen indices ascending, zero padded; positive_slots [batch_size]:
    positions of the positives inside ``selected``; counts [2] int32: number selected, positives among them)."""
    if not labels.is_cuda or labels.dtype != torch.int64 or labels.dim() != 1:
        raise RuntimeError("sample_fg_bg: 1-D int64 HIP tensor expected (the product path has no CPU fallback)")
    labels = labels.contiguous()
    sel = torch.empty((batch_size,), dtype=torch.int64, device=labels.device)
    slots = torch.empty((batch_size,), dtype=torch.int64, device=labels.device)
    counts = torch.empty((2,), dtype=torch.int32, device=labels.device)
    with _on(labels.device):
        rc = _L.ovis_sample_fg_bg(labels.data_ptr(), labels.numel(), int(batch_size), int(max_positives),
                                  int(seed) & 0xFFFFFFFFFFFFFFFF, sel.data_ptr(), slots.data_ptr(), counts.data_ptr(), _stream())
    _lib.check(rc, "sample_fg_bg")
    return sel, slots, counts


BRANCH_ROI_UNION_MAX_IMAGES = _lib.OVIS_BOX_DECODE_MAX_IMAGES  # the per-image pointers travel as kernel arguments


def branch_roi_union(branch0, branch1, image_ids=None):
    """Union of the RoIs two branches sampled from proposal lists of the same images (``ovis_branch_roi_union``), one
    launch, nothing read back.  ``branch0`` / ``branch1``: per image a tuple (boxes [P, 4] float32, selected, positive_slots,
    counts) -- the image's proposals and what ``sample_fg_bg`` returned for them.  A branch-1 row whose four box words equal
    a branch-0 row's of the same image (bit patterns) shares that row; the others follow all branch-0 rows.
    -> (rois [R, 5]: the union rows' RoIs, R = images * (batch0 + batch1) rounded up to 32, rows behind the union copies of
    its last row; map1 [images * batch1] int64: union row of every branch-1 row, dense; positive_rows int64: ascending union
    rows positive in either branch; slots0, slots1: each branch's positives as positions in ``positive_rows``;
    counts [images, 2] int32: (new rows, entries of positive_rows) per image)."""
    n = len(branch0)
    if n == 0 or len(branch1) != n:
        raise RuntimeError("branch_roi_union: the same, non-zero number of images expected in both branches")
    cols = []
    for name, branch in (("branch0", branch0), ("branch1", branch1)):
        boxes = [_dev(b[0], f"{name} boxes") for b in branch]
        sel = [_dev(b[1], f"{name} selected", torch.int64) for b in branch]
        slots = [_dev(b[2], f"{name} positive_slots", torch.int64) for b in branch]
        counts = [_dev(b[3], f"{name} counts", torch.int32) for b in branch]
        batch = sel[0].numel()
        if any(b.dim() != 2 or b.shape[1] != 4 for b in boxes) or any(c.numel() != 2 for c in counts) \
                or any(s.numel() != batch for s in sel + slots) or batch == 0:
            raise RuntimeError(f"branch_roi_union: {name}: [P, 4] boxes, equally long selected / positive_slots and [2] counts expected")
        cols.append((boxes, sel, slots, counts, batch))
    dev = cols[0][0][0].device
    b0, b1 = cols[0][4], cols[1][4]
    rows = -(-n * (b0 + b1) // 32) * 32
    rois = torch.empty((rows, 5), dtype=torch.float32, device=dev)
    i64 = torch.empty((n * (2 * b0 + 3 * b1),), dtype=torch.int64, device=dev)
    map1, positive_rows, slots0, slots1 = i64.split([n * b1, n * (b0 + b1), n * b0, n * b1])
    i32 = torch.empty((b0 + 2 * n,), dtype=torch.int32, device=dev)

    def table(tensors, ctype=ctypes.c_void_p):
        return (ctype * n)(*[t.data_ptr() if t.numel() else None for t in tensors])
    args = []
    for boxes, sel, slots, counts, _ in cols:
        args += [table(boxes), (ctypes.c_int32 * n)(*[b.shape[0] for b in boxes]), table(sel), table(slots), table(counts)]
    ids = None if image_ids is None else (ctypes.c_int32 * n)(*[int(i) for i in image_ids])
    with _on(dev):
        rc = _L.ovis_branch_roi_union(*args, ids, n, b0, b1, rois.data_ptr(), rows, map1.data_ptr(), positive_rows.data_ptr(),
                                      slots0.data_ptr(), slots1.data_ptr(), i32.data_ptr(), i32[b0:].data_ptr(), _stream())
    _lib.check(rc, "branch_roi_union")
    return rois, map1, positive_rows, slots0, slots1, i32[b0:].view(n, 2)


def gather_rows(index, boxes_a=None, boxes_b=None, ints_a=None, ints_b=None):
    """``x.index_select(0, index)`` for up to two [P, 4] float32 and two [P] int64 tensors in one launch
    (``ovis_gather_rows``) -> tuple of the gathered tensors (None where the source is None)."""
    index = _dev(index, "index", torch.int64)
    n = index.numel()
    srcs = [None if t is None else _dev(t, "boxes", torch.float32) for t in (boxes_a, boxes_b)] + \
           [None if t is None else _dev(t, "ints", torch.int64) for t in (ints_a, ints_b)]
    for t in srcs[:2]:
        if t is not None and (t.dim() != 2 or t.shape[1] != 4):
            raise RuntimeError("gather_rows: float sources must be [P, 4]")
    for t in srcs[2:]:
        if t is not None and t.dim() != 1:
            raise RuntimeError("gather_rows: int64 sources must be [P]")
    outs = [None if t is None else torch.empty((n,) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device) for t in srcs]
    if n:
        with _on(index.device):
            rc = _L.ovis_gather_rows(index.data_ptr(), n, _ptr(srcs[0]), _ptr(outs[0]), _ptr(srcs[1]), _ptr(outs[1]),
                                     _ptr(srcs[2]), _ptr(outs[2]), _ptr(srcs[3]), _ptr(outs[3]), _stream())
        _lib.check(rc, "gather_rows")
    return tuple(outs)


def project_pasted_masks(mask_probs, gt_boxes, gt_index, boxes, image_size, resolution, threshold=0.5):
    """Mask targets [P, resolution, resolution] for boxes [P, 4] whose ground truth gt_index[p] has its binary mask
    defined by (mask_probs [G, M, M], gt_boxes [G, 4]) through the Masker paste (``ovis_project_pasted_masks_f32``);
    image_size = (height, width)."""
    mask_probs, gt_boxes, boxes = _dev(mask_probs, "mask_probs"), _dev(gt_boxes, "gt_boxes"), _dev(boxes, "boxes")
    gt_index = _dev(gt_index, "gt_index", torch.int64)
    p = boxes.shape[0]
    out = torch.empty((p, resolution, resolution), dtype=torch.float32, device=boxes.device)
    if p == 0:
        return out
    if mask_probs.dim() != 3 or mask_probs.shape[1] != mask_probs.shape[2] or gt_boxes.shape != (mask_probs.shape[0], 4):
        raise RuntimeError("project_pasted_masks: expected mask_probs [G,M,M] and gt_boxes [G,4]")
    with _on(boxes.device):
        rc = _L.ovis_project_pasted_masks_f32(mask_probs.data_ptr(), gt_boxes.data_ptr(), gt_index.data_ptr(),
                                              boxes.data_ptr(), p, int(image_size[0]), int(image_size[1]),
                                              mask_probs.shape[1], int(resolution), float(threshold), out.data_ptr(), _stream())
    _lib.check(rc, "project_pasted_masks")
    return out


def paste_masks(probs, boxes, image_size, threshold=0.5):
    """bool [P, H, W]: the masks ``Masker(threshold, padding=1)`` pastes for probs [P, M, M] and boxes [P, 4] xyxy
    (``ovis_paste_masks_u8``; mask_head/inference.py:100-205), image_size = (height, width).  One launch, no host read;
    the kernel writes every byte, so the canvas is not filled first."""
    probs, boxes = _dev(probs, "probs"), _dev(boxes, "boxes")
    if probs.dim() != 3 or probs.shape[1] != probs.shape[2] or boxes.shape != (probs.shape[0], 4):
        raise RuntimeError("paste_masks: expected probs [P,M,M] and boxes [P,4]")
    p, h, w = probs.shape[0], int(image_size[0]), int(image_size[1])
    out = torch.empty((p, h, w), dtype=torch.bool, device=probs.device)
    if p == 0:
        return out
    with _on(probs.device):
        rc = _L.ovis_paste_masks_u8(probs.data_ptr(), boxes.data_ptr(), p, probs.shape[1], h, w, float(threshold),
                                    out.data_ptr(), _stream())
    _lib.check(rc, "paste_masks")
    return out


def _pasted_runs(name, probs, boxes, sizes, threshold, with_chars):
    """-> (counts int32 [total], offsets int64 [P + 1], the strings' lengths int32 [P] or None), all on the device.  The
    one host read: the P run totals, which also carry the kernel's verdict on every size."""
    probs, boxes, sizes = _dev(probs, "probs"), _dev(boxes, "boxes"), _dev(sizes, "sizes", torch.int32)
    if probs.dim() != 3 or probs.shape[1] != probs.shape[2] or probs.shape[1] < 1 or boxes.shape != (probs.shape[0], 4) \
            or sizes.shape != (probs.shape[0], 2):
        raise RuntimeError(f"{name}: expected probs [P,M,M], boxes [P,4] and sizes int32 [P,2] (height, width)")
    p, m, dev = probs.shape[0], probs.shape[1], probs.device
    num_runs = torch.empty(p, dtype=torch.int32, device=dev)
    with _on(dev):
        rc = _L.ovis_pasted_rle_count(probs.data_ptr(), boxes.data_ptr(), sizes.data_ptr(), p, m, float(threshold),
                                      num_runs.data_ptr(), _stream())
    _lib.check(rc, name)
    totals = num_runs.cpu()
    if p and int(totals.min()) < 1:
        raise RuntimeError(f"{name}: every size needs height >= 1, width >= 1 and height * width <= 0x7fffffef")
    offsets_host = torch.zeros(p + 1, dtype=torch.int64)
    torch.cumsum(totals, 0, out=offsets_host[1:])
    offsets = offsets_host.to(dev)
    counts = torch.empty(int(offsets_host[-1]), dtype=torch.int32, device=dev)
    num_chars = torch.empty(p, dtype=torch.int32, device=dev) if with_chars else None
    with _on(dev):
        rc = _L.ovis_pasted_rle_runs(probs.data_ptr(), boxes.data_ptr(), sizes.data_ptr(), p, m, float(threshold),
                                     offsets.data_ptr(), counts.data_ptr(), num_chars.data_ptr() if with_chars else 0, _stream())
    _lib.check(rc, name)
    return counts, offsets, num_chars


def pasted_masks_runs(probs, boxes, sizes, threshold=0.5):
    """(counts int32 [total], offsets int64 [P + 1]), both on the device: ``counts[offsets[p]:offsets[p + 1]]`` is the
    uncompressed COCO RLE (pycocotools' ``rleEncode``: column-major, zeros first) of the mask ``paste_masks`` would make of
    probs[p] [M, M] and boxes[p] xyxy on an image of sizes[p] = (height, width) -- per mask, so one call serves images of
    different sizes (``ovis_pasted_rle_count`` / ``_runs``; coco_eval.py:108-144).  No canvas is written; the host reads
    the P run totals once.  Device tensors only, as in the reference there is no host form."""
    counts, offsets, _ = _pasted_runs("pasted_masks_runs", probs, boxes, sizes, threshold, False)
    return counts, offsets


def pasted_masks_rle(probs, boxes, sizes, threshold=0.5):
    """(data uint8 [total_chars], offsets int64 [P + 1]), both on the device: ``bytes(data[offsets[p]:offsets[p + 1]])`` is
    the compressed ``counts`` string (pycocotools' ``rleToString``) of mask p of ``pasted_masks_runs`` -- what
    ``mask_util.encode`` returns for the pasted mask (``ovis_pasted_rle_*``; coco_eval.py:139-144).  Two host reads: the
    run totals and the string lengths."""
    counts, run_offsets, num_chars = _pasted_runs("pasted_masks_rle", probs, boxes, sizes, threshold, True)
    p, dev = num_chars.shape[0], num_chars.device
    offsets_host = torch.zeros(p + 1, dtype=torch.int64)
    torch.cumsum(num_chars.cpu(), 0, out=offsets_host[1:])
    offsets = offsets_host.to(dev)
    data = torch.empty(int(offsets_host[-1]), dtype=torch.uint8, device=dev)
    with _on(dev):
        rc = _L.ovis_pasted_rle_string(counts.data_ptr(), run_offsets.data_ptr(), offsets.data_ptr(), p, data.data_ptr(),
                                       _stream())
    _lib.check(rc, "pasted_masks_rle")
    return data, offsets


def render_instances(image, maps, boxes, colors, kinds=None, params=None, alpha=0.5, outline_colors=None, outline_thickness=2):
    """uint8 [H, W, 3]: box outlines, filled masks and uncertainty heat layers composited onto ``image`` uint8 [H, W, 3]
    (``ovis_render_instances_u8``; engine/inference.py:519-589 over the Masker paste).  Layer i is (maps[i] [M, M] f32,
    boxes[i] xyxy, kinds[i], params[i], colors[i] [3] f32 in 0..255), applied in index order: kind 0 fills where the pasted
    value exceeds params[i] (``p * (1 - alpha) + alpha * colour``), kind 1 blends by ``clamp(value * params[i], 0, 1)``
    (params[i] = float32(0.2 / score)).  kinds: int32 [K], default all fill; params: a number or f32 [K], default 0.5.
    outline_colors uint8 [K, 3] draws every box (our band rule, include/ovis_hip.h) before any layer.  One launch on the
    device of ``image``; host tensors take the host twin (``libovis_cpu.so``), same bytes."""
    k = maps.shape[0] if maps.dim() == 3 else -1
    if image.dim() != 3 or image.shape[2] != 3 or image.dtype != torch.uint8:
        raise RuntimeError("render_instances: expected image uint8 [H, W, 3]")
    if k < 0 or maps.shape[1] != maps.shape[2] or tuple(boxes.shape) != (k, 4) or tuple(colors.shape) != (k, 3):
        raise RuntimeError("render_instances: expected maps [K,M,M], boxes [K,4] and colors [K,3]")
    dev = image.device
    kinds = torch.zeros(k, dtype=torch.int32, device=dev) if kinds is None else kinds
    if not torch.is_tensor(params):
        params = torch.full((k,), 0.5 if params is None else float(params), dtype=torch.float32, device=dev)
    if tuple(kinds.shape) != (k,) or tuple(params.shape) != (k,) or (outline_colors is not None and tuple(outline_colors.shape) != (k, 3)):
        raise RuntimeError("render_instances: expected kinds [K], params [K] and outline_colors [K,3]")
    if not image.is_cuda:
        return _cpu.render_instances(
            _cpu._host(image, "image", torch.uint8), _cpu._host(maps, "maps"), _cpu._host(boxes, "boxes"),
            _cpu._host(colors, "colors"), _cpu._host(kinds, "kinds", torch.int32), _cpu._host(params, "params"), alpha,
            None if outline_colors is None else _cpu._host(outline_colors, "outline_colors", torch.uint8), outline_thickness)
    image = _dev(image, "image", torch.uint8)
    maps, boxes, colors, params = _dev(maps, "maps"), _dev(boxes, "boxes"), _dev(colors, "colors"), _dev(params, "params")
    kinds = _dev(kinds, "kinds", torch.int32)
    if outline_colors is not None:
        outline_colors = _dev(outline_colors, "outline_colors", torch.uint8)
    out = torch.empty_like(image)
    with _on(dev):
        rc = _L.ovis_render_instances_u8(
            image.data_ptr(), image.shape[0], image.shape[1], maps.data_ptr() if k else 0, boxes.data_ptr() if k else 0, k,
            maps.shape[1] if k else 0, kinds.data_ptr() if k else 0, params.data_ptr() if k else 0,
            colors.data_ptr() if k else 0, float(alpha), outline_colors.data_ptr() if (k and outline_colors is not None) else 0,
            int(outline_thickness), out.data_ptr(), _stream())
    _lib.check(rc, "render_instances")
    return out


def split_pair(x):
    """x [rows, cols] f32 (row-strided view ok, cols % 32 == 0) -> pair layout [rows, 2*cols] bf16: per 32 values
    [hi(32) | lo(32)].  See include/ovis_hip.h."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise RuntimeError("split_pair: 2-D float32 HIP tensor expected")
    if x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16:
        x = x.contiguous()
    rows, cols = x.shape
    out = torch.empty((rows, 2 * cols), dtype=torch.bfloat16, device=x.device)
    if out.numel() == 0:
        return out
    with _on(x.device):
        rc = _L.ovis_split_pair_f32(x.data_ptr(), x.stride(0), out.data_ptr(), rows, cols, _stream())
    _lib.check(rc, "split_pair")
    return out


def gate_split_pair(dy, gate=None, want_f32=False, pooled=None, pool_rows=0, selected=None, group_slot=None):
    """g = (dy + pooled[row // pool_rows] / pool_rows) * (y > 0) in pair layout (and as fp32 when ``want_f32``); gate =
    y as fp32 [rows, cols] or as its pair form [rows, 2*cols] bf16 (contiguous), None = no gate; ``pooled`` = the
    gradient of a mean over every ``pool_rows`` consecutive rows ([rows / pool_rows, cols] f32) or None; ``dy`` may be
    None when ``pooled`` is given.  ``selected`` [S * pool_rows, cols] f32 with ``group_slot`` [rows / pool_rows] int32
    (index into ``selected`` of a group of pool_rows rows, -1 = none): the gradient of a gather of whole row groups, added
    on the fly instead of being scattered into a zero tensor first.  Returns (g_pair, g_f32 or None)."""
    if dy is None and pooled is None:
        raise RuntimeError("gate_split_pair: dy or pooled must be given")
    if (selected is None) != (group_slot is None):
        raise RuntimeError("gate_split_pair: selected and group_slot are given together")
    if pooled is not None:
        if not (pooled.is_cuda and pooled.dtype == torch.float32 and pooled.dim() == 2):
            raise RuntimeError("gate_split_pair: pooled must be a 2-D float32 HIP tensor")
        pooled = pooled.contiguous()
    if dy is not None:
        if not (dy.is_cuda and dy.dtype == torch.float32 and dy.dim() == 2):
            raise RuntimeError("gate_split_pair: 2-D float32 HIP tensor expected")
        if dy.stride(1) != 1 or dy.stride(0) % 4 or dy.data_ptr() % 16:
            dy = dy.contiguous()
        rows, cols = dy.shape
    else:
        rows, cols = pooled.shape[0] * pool_rows, pooled.shape[1]
    if pooled is not None and (pool_rows <= 0 or pooled.shape != (rows // max(pool_rows, 1), cols) or rows % pool_rows):
        raise RuntimeError("gate_split_pair: pooled must be [rows / pool_rows, cols]")
    dev = dy.device if dy is not None else pooled.device
    is_pair = 0
    if gate is not None:
        is_pair = int(gate.dtype == torch.bfloat16)
        if not (gate.is_cuda and gate.is_contiguous() and gate.shape == (rows, cols * (2 if is_pair else 1))
                and gate.dtype in (torch.bfloat16, torch.float32)):
            raise RuntimeError("gate_split_pair: gate must be the contiguous fp32 or pair form of the forward output")
    out = torch.empty((rows, 2 * cols), dtype=torch.bfloat16, device=dev)
    g32 = torch.empty((rows, cols), dtype=torch.float32, device=dev) if want_f32 else None
    if out.numel() == 0:
        return out, g32
    if selected is not None:
        selected, group_slot = _dev(selected, "selected"), _dev(group_slot, "group_slot", torch.int32)
        if pool_rows <= 0 or rows % pool_rows or selected.dim() != 2 or selected.shape[1] != cols or \
                selected.shape[0] % pool_rows or group_slot.numel() != rows // pool_rows:
            raise RuntimeError("gate_split_pair: selected must be [S * pool_rows, cols] and group_slot [rows / pool_rows]")
    with _on(dev):
        rc = _L.ovis_gate_split_pair_rows_f32(_ptr(dy), 0 if dy is None else dy.stride(0), _ptr(gate), is_pair, out.data_ptr(),
                                              _ptr(g32), rows, cols, _ptr(pooled), pool_rows, _ptr(selected),
                                              _ptr(group_slot), _stream())
    _lib.check(rc, "gate_split_pair")
    return out, g32


def im2col_pair(xp, h, w, kh, kw):
    """xp [R*h*w, 2*C] pair rows of an NHWC tensor -> [R*h*w, 2*kh*kw*C] pair rows (tap-major, zero rows outside
    the map): the M-contracting operand of a 3x3 weight gradient."""
    if not (xp.is_cuda and xp.dtype == torch.bfloat16 and xp.dim() == 2 and xp.is_contiguous()):
        raise RuntimeError("im2col_pair: contiguous 2-D bfloat16 HIP tensor (pair layout) expected")
    m, c2 = xp.shape
    if m % (h * w):
        raise RuntimeError("im2col_pair: rows must be a multiple of h*w")
    out = torch.empty((m, kh * kw * c2), dtype=torch.bfloat16, device=xp.device)
    if out.numel() == 0:
        return out
    with _on(xp.device):
        rc = _L.ovis_im2col_pair(xp.data_ptr(), out.data_ptr(), m // (h * w), h, w, c2 // 2, kh, kw, _stream())
    _lib.check(rc, "im2col_pair")
    return out


def im2col_nchw_pair(x, kh, kw, stride, pad):
    """x [N, C, H, W] f32 contiguous -> (pair rows [N*Ho*Wo, 2*Kp] of the strided convolution's patches, k =
    (ky*kw + kx)*C + c zero-padded to Kp % 32 == 0, (Ho, Wo)).  See include/ovis_hip.h."""
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 4 and x.is_contiguous()):
        raise RuntimeError("im2col_nchw_pair: contiguous [N,C,H,W] float32 HIP tensor expected")
    n, c, h, w = x.shape
    ho, wo = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    kp = -(-(kh * kw * c) // 32) * 32
    out = torch.empty((n * ho * wo, 2 * kp), dtype=torch.bfloat16, device=x.device)
    if out.numel():
        with _on(x.device):
            rc = _L.ovis_im2col_nchw_pair_f32(x.data_ptr(), out.data_ptr(), n, c, h, w, kh, kw, stride, pad, kp, _stream())
        _lib.check(rc, "im2col_nchw_pair")
    return out, (ho, wo)


_GEMM_TLS = threading.local()


@contextlib.contextmanager
def co_scheduled(on=True):
    """Split-GEMM launches issued inside run BESIDE other work (the frozen half of the student-teacher step on its side stream,
    ``engine/trainer.py``): the library then cuts K for least total work instead of least duration (config bit 16 of
    ``ovis_split_gemm_pair*``).  Per thread: the look-ahead half may be issued by a worker thread."""
    prev = getattr(_GEMM_TLS, "co", False)
    _GEMM_TLS.co = bool(on)
    try:
        yield
    finally:
        _GEMM_TLS.co = prev


# Size queries of the library are pure functions of their arguments (shape + config bits): asked once per distinct
# argument tuple, not once per launch -- 98 ctypes round trips per student step for the split GEMM's workspace alone.
@functools.lru_cache(maxsize=None)
def _gemm_ws_bytes(m, n, ch, ch2, kh, kw, w, config):
    return int(_L.ovis_split_gemm_pair_workspace_bytes_ex(m, n, ch, ch2, kh, kw, w, config))


@functools.lru_cache(maxsize=None)
def _tn_slices(m, n, ch, taps):
    return int(_L.ovis_split_gemm_tn_slices(m, n, ch, taps))


@functools.lru_cache(maxsize=None)
def _tn_map_slices(m, n, ch, kh, kw, h, w):
    return int(_L.ovis_split_gemm_tn_map_slices(m, n, ch, kh, kw, h, w))


@functools.lru_cache(maxsize=None)
def _gemm_f32_ws_bytes(m, n, k):
    return int(_L.ovis_gemm_f32_workspace_bytes(m, n, k))


@functools.lru_cache(maxsize=None)
def _nms_presorted_ws_bytes(n, k):
    return int(_L.ovis_nms_presorted_workspace_bytes(n, k))


@functools.lru_cache(maxsize=None)
def _topk_ws_bytes(n, a):
    return int(_L.ovis_topk_sorted_workspace_bytes(n, a))


def _gemm_cfg(config):
    return config | (0x10000 if getattr(_GEMM_TLS, "co", False) else 0)


def _gemm_workspace(device, m, n, ch, ch2, kh, kw, w, config):
    """(split-K scratch of the launch plan or None, its size); config bit 8 = no K slices."""
    nbytes = 0 if config & 8 else _gemm_ws_bytes(m, n, ch, ch2, kh, kw, w, config)
    return _workspace(nbytes, device), nbytes


def split_gemm_pair(a_pair, b_pair, bias=None, residual=None, relu=False, out_f32=True, out_pair=False, conv=None,
                    config=0, a2_pair=None, residual_pair=None):
    """act(A @ B^T + bias + residual) with A [M, 2*ch] / B [N, 2*K] in pair layout (``split_pair``); fp32-accurate
    three-term bf16 hi/lo product on the matrix cores (csrc/split_gemm.hip).  conv = (h, w, kh, kw, flip): A is an
    NHWC tensor [M/(h*w), h, w, ch] and B holds [N, kh*kw*ch] tap-major weights -- stride-1 "same" convolution as an
    implicit GEMM.  a2_pair [M, 2*ch2]: a second operand whose products follow A's along K (B = [N, 2*(ch + ch2)]):
    conv3 + projection shortcut of a bottleneck as one product.  ``config``: 0 = choose; test / measurement bits as in
    include/ovis_hip.h.  Returns (C f32 [M, N] or None, C in pair layout [M, 2*N] or None)."""
    _check_pairs("split_gemm_pair", a_pair=a_pair, b_pair=b_pair)
    m, ch = a_pair.shape[0], a_pair.shape[1] // 2
    n, k = b_pair.shape[0], b_pair.shape[1] // 2
    ch2 = 0
    if a2_pair is not None:
        _check_pairs("split_gemm_pair", a2_pair=a2_pair)
        if conv is not None or a2_pair.shape[0] != m:
            raise RuntimeError("split_gemm_pair: a2_pair needs a plain product and as many rows as a_pair")
        ch2 = a2_pair.shape[1] // 2
    h = w = 0
    kh = kw = 1
    flip = False
    if conv is not None:
        h, w, kh, kw, flip = conv
        if m % (h * w):
            raise RuntimeError("split_gemm_pair: rows must be a multiple of h*w")
    if k != kh * kw * ch + ch2:
        raise RuntimeError(f"split_gemm_pair: contraction mismatch (A has {ch} channels x {kh * kw} taps + {ch2}, B has {k})")
    dev = a_pair.device
    c, cp = _gemm_results(m, n, out_f32, out_pair, dev)
    if m == 0 or n == 0:
        return c, cp
    if bias is not None:
        bias = _dev(bias, "bias")
    if residual_pair is not None:
        # shortcut in pair layout (hi + lo, exact in fp32): plain 1x1 products only
        if residual is not None or conv is not None or a2_pair is not None or n % 32 or not (
                residual_pair.is_cuda and residual_pair.dtype == torch.bfloat16 and residual_pair.dim() == 2
                and residual_pair.stride(1) == 1 and residual_pair.shape == (m, 2 * n)):
            raise RuntimeError("split_gemm_pair: residual_pair must be [M, 2N] bfloat16 pair rows of a plain product")
        with _on(dev):
            config = _gemm_cfg(config)
            ws, nbytes = _gemm_workspace(dev, m, n, ch, 0, 1, 1, 0, config)
            rc = _L.ovis_split_gemm_pair_rp(a_pair.data_ptr(), 2 * a_pair.stride(0), b_pair.data_ptr(), 2 * b_pair.stride(0),
                                            _ptr(c), n, _ptr(cp), 4 * n, _ptr(bias), residual_pair.data_ptr(),
                                            2 * residual_pair.stride(0), m, n, ch, int(bool(relu)), _ptr(ws), nbytes, config,
                                            _stream())
        _lib.check(rc, "split_gemm_pair_rp")
        return c, cp
    if residual is not None and not (residual.is_cuda and residual.dtype == torch.float32 and residual.dim() == 2
                                     and residual.stride(1) == 1 and residual.shape == (m, n)):
        raise RuntimeError("split_gemm_pair: residual must be a float32 [M, N] HIP tensor with unit column stride")
    with _on(dev):
        config = _gemm_cfg(config)
        ws, nbytes = _gemm_workspace(dev, m, n, ch, ch2, kh, kw, w, config)
        rc = _L.ovis_split_gemm_pair(a_pair.data_ptr(), 2 * a_pair.stride(0), _ptr(a2_pair),
                                     0 if a2_pair is None else 2 * a2_pair.stride(0), b_pair.data_ptr(), 2 * b_pair.stride(0),
                                     _ptr(c), n, _ptr(cp), 4 * n, _ptr(bias), _ptr(residual),
                                     0 if residual is None else residual.stride(0), m, n, ch, ch2, kh, kw, h, w,
                                     int(bool(flip)), int(bool(relu)), _ptr(ws), nbytes, config, _stream())
    _lib.check(rc, "split_gemm_pair")
    return c, cp


def split_gemm_pair_pool_supported(m, n, ch, pool_rows):
    return bool(_L.ovis_split_gemm_pair_pool_supported(int(m), int(n), int(ch), int(pool_rows)))


def split_gemm_pair_rp_pool(a_pair, b_pair, bias, residual_pair, relu, out_f32, out_pair, pool_rows):
    """``split_gemm_pair(..., residual_pair=...)`` of the LAST bottleneck of a res5 chain with the head's average pooling in the
    epilogue (``ovis_split_gemm_pair_rp_pool``): also returns the mean of the result over every group of ``pool_rows`` rows
    ([M / pool_rows, N] fp32); with ``out_f32`` and ``out_pair`` both False the result itself is never written.
    -> (C f32 or None, C pair or None, pooled)."""
    _check_pairs("split_gemm_pair_rp_pool", a_pair=a_pair, b_pair=b_pair)
    if residual_pair is not None:
        _check_pairs("split_gemm_pair_rp_pool", residual_pair=residual_pair)
    m, ch = a_pair.shape[0], a_pair.shape[1] // 2
    n, k = b_pair.shape[0], b_pair.shape[1] // 2
    if k != ch or m % pool_rows or (residual_pair is not None and residual_pair.shape != (m, 2 * n)):
        raise RuntimeError("split_gemm_pair_rp_pool: shape mismatch")
    dev = a_pair.device
    c, cp = _gemm_results(m, n, out_f32, out_pair, dev)
    pooled = torch.zeros((m // pool_rows, n), dtype=torch.float32, device=dev)
    if m == 0 or n == 0:
        return c, cp, pooled
    if bias is not None:
        bias = _dev(bias, "bias")
    with _on(dev):
        rc = _L.ovis_split_gemm_pair_rp_pool(a_pair.data_ptr(), 2 * a_pair.stride(0), b_pair.data_ptr(), 2 * b_pair.stride(0),
                                             _ptr(c), n, _ptr(cp), 4 * n, _ptr(bias), _ptr(residual_pair),
                                             0 if residual_pair is None else 2 * residual_pair.stride(0), m, n, ch,
                                             int(bool(relu)), pooled.data_ptr(), int(pool_rows), 1.0 / pool_rows, _stream())
    _lib.check(rc, "split_gemm_pair_rp_pool")
    return c, cp, pooled


def weight_prep_pair(w, scale=None, want_transposed=False):
    """w [N, C, KH, KW] f32 (times scale[N]) -> (pair [N, 2*KH*KW*C] tap-major, transposed pair [C, 2*KH*KW*N] or None)
    in one launch; see include/ovis_hip.h."""
    if not (w.is_cuda and w.dtype == torch.float32 and w.dim() == 4):
        raise RuntimeError("weight_prep_pair: [N,C,KH,KW] float32 HIP tensor expected")
    w = w.detach().contiguous()
    n, c, kh, kw = w.shape
    t = kh * kw
    fwd = torch.empty((n, 2 * t * c), dtype=torch.bfloat16, device=w.device)
    bwd = torch.empty((c, 2 * t * n), dtype=torch.bfloat16, device=w.device) if want_transposed else None
    if scale is not None:
        scale = _dev(scale.detach(), "scale")
    with _on(w.device):
        rc = _L.ovis_weight_prep_pair_f32(w.data_ptr(), _ptr(scale), fwd.data_ptr(), _ptr(bwd), n, c, t, _stream())
    _lib.check(rc, "weight_prep_pair")
    return fwd, bwd


def split_gemm_pair_gated(a_pair, b_pair, gate_pair, conv=None, out_f32=False, out_pair=True, config=0):
    """(A @ B^T) * (y > 0) with y given in pair layout (``gate_pair`` [M, 2N]): the data gradient of a layer behind a
    ReLU, gated and split for the next backward GEMM in the epilogue.  Returns (f32 or None, pair or None)."""
    _check_pairs("split_gemm_pair_gated", a_pair=a_pair, b_pair=b_pair, gate_pair=gate_pair)
    m, ch = a_pair.shape[0], a_pair.shape[1] // 2
    n, k = b_pair.shape[0], b_pair.shape[1] // 2
    h = w = 0
    kh = kw = 1
    flip = False
    if conv is not None:
        h, w, kh, kw, flip = conv
    if k != kh * kw * ch or gate_pair.shape != (m, 2 * n):
        raise RuntimeError("split_gemm_pair_gated: shape mismatch")
    dev = a_pair.device
    c, cp = _gemm_results(m, n, out_f32, out_pair, dev)
    if m == 0 or n == 0:
        return c, cp
    with _on(dev):
        # under-filled grids take the plan's K slices (the slab reduction applies the gate)
        config = _gemm_cfg(config)
        ws, nbytes = _gemm_workspace(dev, m, n, ch, 0, kh, kw, w, config)
        rc = _L.ovis_split_gemm_pair_gated_ws(a_pair.data_ptr(), 2 * a_pair.stride(0), b_pair.data_ptr(),
                                              2 * b_pair.stride(0), _ptr(c), n, _ptr(cp), 4 * n, gate_pair.data_ptr(),
                                              2 * gate_pair.stride(0), m, n, ch, kh, kw, h, w, int(bool(flip)),
                                              _ptr(ws), nbytes, config, _stream())
    _lib.check(rc, "split_gemm_pair_gated")
    return c, cp


def split_gemm_pair_rp_gated(a_pair, b_pair, residual_pair, gate_pair, out_f32=False, out_pair=True, config=0):
    """(A @ B^T + r) * (x > 0) with r (``residual_pair``) and x (``gate_pair``) [M, 2N] in pair layout: the input gradient
    of an identity bottleneck, gated by the ReLU of the block below and split for its backward GEMMs in the epilogue
    (``ovis_split_gemm_pair_rp_gated``).  Returns (f32 or None, pair or None)."""
    _check_pairs("split_gemm_pair_rp_gated", a_pair=a_pair, b_pair=b_pair, residual_pair=residual_pair, gate_pair=gate_pair)
    m, ch = a_pair.shape[0], a_pair.shape[1] // 2
    n, k = b_pair.shape[0], b_pair.shape[1] // 2
    if k != ch or gate_pair.shape != (m, 2 * n) or residual_pair.shape != (m, 2 * n):
        raise RuntimeError("split_gemm_pair_rp_gated: shape mismatch")
    dev = a_pair.device
    c, cp = _gemm_results(m, n, out_f32, out_pair, dev)
    if m == 0 or n == 0:
        return c, cp
    with _on(dev):
        rc = _L.ovis_split_gemm_pair_rp_gated(a_pair.data_ptr(), 2 * a_pair.stride(0), b_pair.data_ptr(),
                                              2 * b_pair.stride(0), _ptr(c), n, _ptr(cp), 4 * n, residual_pair.data_ptr(),
                                              2 * residual_pair.stride(0), gate_pair.data_ptr(), 2 * gate_pair.stride(0), m, n,
                                              ch, config, _stream())
    _lib.check(rc, "split_gemm_pair_rp_gated")
    return c, cp


def split_gemm_pair_tn_supported(n, ch, conv=None):
    if n % 128 or ch % 128:
        return False
    if conv is not None:
        h, w, kh, kw = conv
        return kh % 2 == 1 and kw % 2 == 1
    return True


def split_gemm_pair_tn(g_pair, x_pair, conv=None, scale=None, weight_shape=None):
    """dW [N, taps*ch] = G^T X over the rows: G [M, 2N], X [M, 2*ch] in pair layout; conv = (h, w, kh, kw): X is an
    NHWC tensor read shifted by every tap (the 3x3 weight gradient without im2col rows).  With ``weight_shape`` =
    (N, ch, kh, kw) the slabs are reduced straight into that layout, times ``scale[N]`` (the folded FrozenBN scale) --
    the gradient of the raw convolution weight in one extra launch.  csrc/split_gemm.hip."""
    _check_pairs("split_gemm_pair_tn", g_pair=g_pair, x_pair=x_pair)
    m, n, ch = g_pair.shape[0], g_pair.shape[1] // 2, x_pair.shape[1] // 2
    if x_pair.shape[0] != m:
        raise RuntimeError("split_gemm_pair_tn: row counts differ")
    h = w = 0
    kh = kw = 1
    if conv is not None:
        h, w, kh, kw = conv
        if m % (h * w):
            raise RuntimeError("split_gemm_pair_tn: rows must be a multiple of h*w")
    dev = g_pair.device
    if m == 0:
        z = torch.zeros((n, kh * kw * ch), dtype=torch.float32, device=dev)
        return z if weight_shape is None else z.new_zeros(weight_shape)
    slices = _tn_slices(m, n, ch, 1) if conv is None else _tn_map_slices(m, n, ch, kh, kw, h, w)
    slabs = torch.empty((slices, n, kh * kw * ch), dtype=torch.float32, device=dev)
    with _on(dev):
        rc = _L.ovis_split_gemm_pair_tn(g_pair.data_ptr(), 2 * g_pair.stride(0), x_pair.data_ptr(), 2 * x_pair.stride(0),
                                        slabs.data_ptr(), slices, m, n, ch, kh, kw, h, w, _stream())
        _lib.check(rc, "split_gemm_pair_tn")
        if weight_shape is None:
            return slabs[0] if slices == 1 else slabs.sum(0)
        if tuple(weight_shape) != (n, ch, kh, kw):
            raise RuntimeError("split_gemm_pair_tn: weight_shape must be (N, ch, kh, kw)")
        dw = torch.empty(weight_shape, dtype=torch.float32, device=dev)
        if scale is not None:
            scale = _dev(scale.detach(), "scale")
        rc = _L.ovis_slab_reduce_f32(slabs.data_ptr(), _ptr(scale), dw.data_ptr(), slices, n, ch, kh * kw, _stream())
    _lib.check(rc, "slab_reduce")
    return dw


def bias_act_(y, bias=None, residual=None, relu=True):
    """In place: y[rows, cols] = act(y + bias[col] (+ residual)); contiguous f32, cols % 4 == 0."""
    if not (y.is_cuda and y.dtype == torch.float32 and y.dim() == 2 and y.is_contiguous()):
        raise RuntimeError("bias_act_: contiguous 2-D float32 HIP tensor expected")
    if residual is not None and not (residual.is_contiguous() and residual.shape == y.shape):
        raise RuntimeError("bias_act_: residual must be contiguous with y's shape")
    if y.numel() == 0:
        return y
    with _on(y.device):
        rc = _L.ovis_bias_act_f32(y.data_ptr(), _ptr(bias), _ptr(residual), y.shape[0], y.shape[1], int(bool(relu)), _stream())
    _lib.check(rc, "bias_act")
    return y


def gemm_nt(a, b, bias=None):
    """a [M,K] @ b[N,K]^T (+ bias[N]) -> [M,N] on the fp32 matrix cores.  a / b may be any 2-D strided views."""
    if not a.is_cuda and not b.is_cuda:
        return _cpu.gemm_nt(a, b, bias)
    if not (a.is_cuda and b.is_cuda):
        raise RuntimeError("gemm_nt: HIP device tensors only")
    if a.dtype != torch.float32 or b.dtype != torch.float32:
        raise RuntimeError("gemm_nt: float32 only")
    m, k = a.shape
    n, k2 = b.shape
    if k != k2:
        raise RuntimeError(f"gemm_nt: inner dimensions differ ({k} vs {k2})")
    out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    if m == 0 or n == 0:
        return out
    if k == 0:
        return out.zero_() if bias is None else out.copy_(bias.expand(m, n))
    if bias is not None:
        bias = _dev(bias, "bias")
    with _on(a.device):
        _gemm_raw(a.data_ptr(), a.stride(0), a.stride(1), b.data_ptr(), b.stride(0), b.stride(1), out.data_ptr(), n, m, n, k,
                  bias_ptr=_ptr(bias), device=a.device)
    return out


def region_noun_align(region_emb, noun_emb):
    """-> (raw max score [W], sigmoid score [W], argmax region [W] int64)"""
    if not region_emb.is_cuda:
        return _cpu.region_noun_align(region_emb, noun_emb)
    region_emb, noun_emb = _dev(region_emb, "region_emb"), _dev(noun_emb, "noun_emb")
    p, d = region_emb.shape
    w = noun_emb.shape[0]
    raw = torch.empty((w,), dtype=torch.float32, device=region_emb.device)
    prob = torch.empty_like(raw)
    idx = torch.empty((w,), dtype=torch.int64, device=region_emb.device)
    if w == 0:
        return raw, prob, idx
    with _on(region_emb.device):
        rc = _L.ovis_region_noun_align_f32(region_emb.data_ptr(), noun_emb.data_ptr(), raw.data_ptr(),
                                           prob.data_ptr(), idx.data_ptr(), p, w, d, _stream())
    _lib.check(rc, "region_noun_align")
    return raw, prob, idx


def text_embed(table, input_ids, special_tokens_mask):
    """Word embeddings of tokenised strings (``ovis_text_embed_f32``; language_backbone/transformers.py:27-68 +
    st_generalized_rcnn.py:202-209): table [V, D] float32, input_ids / special_tokens_mask [N, L] integer tensors as the
    tokenizer pads them -> [N, D] unit-norm rows (masked mean of the table rows, then F.normalize)."""
    if not table.is_cuda:  # MODEL.DEVICE cpu: the reference's tensor-op formula on host tensors
        return _cpu.text_embed(table.detach(), input_ids.to(torch.int64), special_tokens_mask.to(torch.int64))
    table = _dev(table, "table")
    if table.dim() != 2 or input_ids.dim() != 2 or input_ids.shape != special_tokens_mask.shape:
        raise RuntimeError("text_embed: expected table [V, D] and input_ids / special_tokens_mask [N, L]")
    if table.requires_grad:
        raise RuntimeError("text_embed: the embedding table is frozen on this path (MODEL.LANGUAGE_BACKBONE.FT_EMB False)")
    ids = input_ids.to(device=table.device, dtype=torch.int32).contiguous()
    sp = special_tokens_mask.to(device=table.device, dtype=torch.int32).contiguous()
    n, l = ids.shape
    out = torch.empty((n, table.shape[1]), dtype=torch.float32, device=table.device)
    if n:
        with _on(table.device):
            rc = _L.ovis_text_embed_f32(table.data_ptr(), table.shape[0], table.shape[1], ids.data_ptr(), sp.data_ptr(), n, l,
                                        out.data_ptr(), _stream())
        _lib.check(rc, "text_embed")
    return out


def project_polygon_masks(coords, polygon_start, instance_start, gt_index, boxes, image_size, resolution):
    """Mask targets [P, M, M] for boxes [P, 4] from POLYGON ground truth (``ovis_project_polygon_masks_f32``;
    mask_head/loss.py:11-42 through PolygonInstance.crop / resize / convert_to_binarymask, segmentation_mask.py:270-334).
    coords float32 [T] (x, y pairs of all polygons), polygon_start int32 [NP + 1] (float offsets), instance_start int32
    [G + 1] (polygon ranges), gt_index [P] int64, image_size = (width, height)."""
    if not boxes.is_cuda:
        return _cpu.project_polygon_masks(coords, polygon_start, instance_start, gt_index, boxes, image_size, resolution)
    boxes = _dev(boxes, "boxes")
    coords = _dev(coords, "coords") if coords.numel() else coords
    polygon_start = _dev(polygon_start, "polygon_start", torch.int32)
    instance_start = _dev(instance_start, "instance_start", torch.int32)
    gt_index = _dev(gt_index, "gt_index", torch.int64)
    p = boxes.shape[0]
    out = torch.empty((p, resolution, resolution), dtype=torch.float32, device=boxes.device)
    if p:
        with _on(boxes.device):
            rc = _L.ovis_project_polygon_masks_f32(coords.data_ptr() if coords.numel() else 0, polygon_start.data_ptr(),
                                                   instance_start.data_ptr(), gt_index.data_ptr(), boxes.data_ptr(), p,
                                                   int(image_size[0]), int(image_size[1]), int(resolution), out.data_ptr(),
                                                   _stream())
        _lib.check(rc, "project_polygon_masks")
    return out


def polygons_to_masks(coords, polygon_start, instance_start, size):
    """uint8 [G, height, width]: every polygon instance rasterised over the whole image (``ovis_polygons_to_masks_u8``;
    segmentation_mask.py:326-334), any image size.  The layout of ``project_polygon_masks``; size = (width, height).
    Device tensors only: host polygons are ``_cpu.polygons_to_masks``."""
    polygon_start = _dev(polygon_start, "polygon_start", torch.int32)
    instance_start = _dev(instance_start, "instance_start", torch.int32)
    coords = _dev(coords, "coords") if coords.numel() else coords
    g, npoly = instance_start.numel() - 1, polygon_start.numel() - 1
    w, h = int(size[0]), int(size[1])
    out = torch.empty((g, h, w), dtype=torch.uint8, device=polygon_start.device)
    if g:
        with _on(out.device):
            nbytes = _L.ovis_polygons_to_masks_workspace_bytes(npoly, w, h)
            ws = _workspace(nbytes, out.device)
            rc = _L.ovis_polygons_to_masks_u8(coords.data_ptr() if coords.numel() else 0, polygon_start.data_ptr(),
                                              instance_start.data_ptr(), g, npoly, w, h, _ptr(ws), nbytes, out.data_ptr(),
                                              _stream())
        _lib.check(rc, "polygons_to_masks")
    return out


def transform_images(data, desc, mean, std, to_bgr255, pad_hw, max_in_hw=None):
    """float32 [B, 3, pad_h, pad_w]: B raw RGB images resized (PIL bilinear, bit for bit), flipped, normalised and zero
    padded (``ovis_transform_images_u8``; data/transforms/transforms.py:27-120, structures/image_list.py:29-70).  data uint8
    [bytes]: the images HWC back to back; desc int32 [B, 7] = (byte offset, in_h, in_w, out_h, out_w, flip_h, flip_v); mean,
    std: three python floats each; pad_hw = (pad_h, pad_w).  Device tensors: max_in_hw = (largest in_h, largest in_w) of
    the batch -- the descriptors stay on the device, the caller that packed them knows it.  Two launches, every element of
    the result written once, no host read.  Host tensors: ``libovis_cpu.so``, same bits."""
    if not data.is_cuda:
        return _cpu.transform_images(data, desc, mean, std, to_bgr255, pad_hw)
    data, desc = _dev(data, "data", torch.uint8), _dev(desc, "desc", torch.int32)
    if data.dim() != 1 or desc.dim() != 2 or desc.shape[1] != 7 or max_in_hw is None:
        raise RuntimeError("transform_images: expected data [bytes] uint8, desc [B,7] int32 and max_in_hw")
    b, (pad_h, pad_w), (max_h, max_w) = desc.shape[0], (int(pad_hw[0]), int(pad_hw[1])), (int(max_in_hw[0]), int(max_in_hw[1]))
    m3, s3 = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
    with _on(data.device):
        nbytes = _L.ovis_transform_images_workspace_bytes(b, max_h, pad_w)
        out = torch.empty((b, 3, pad_h, pad_w), dtype=torch.float32, device=data.device)
        if b:
            ws = _workspace(nbytes, data.device, at_least=1)
            rc = _L.ovis_transform_images_u8(data.data_ptr(), data.numel(), desc.data_ptr(), b, max_h, max_w, m3, s3,
                                             int(bool(to_bgr255)), pad_h, pad_w, ws.data_ptr(), nbytes, out.data_ptr(), _stream())
            _lib.check(rc, "transform_images")
    return out


def transform_images_window(data, desc, mean, std, to_bgr255, pad_hw, max_in_hw=None):
    """float32 [B, 3, pad_h, pad_w]: ``transform_images`` through a crop window (``ovis_transform_images_window_u8``: scale
    jitter + fixed-size crop; include/ovis_hip.h states the rule).  desc int32 [B, 11] = the seven of ``transform_images``
    followed by (win_y, win_x, win_h, win_w), the window in the frame of the resized, flipped image; out_h / out_w are the
    full resized size, never materialised.  Element (Y, X) inside win_h x win_w is pixel (win_y + Y, win_x + X) of that
    image, with the bits of the same slice of ``transform_images``' output; zero elsewhere.  Two launches, no host read.
    Host tensors: ``libovis_cpu.so``, same bits."""
    if not data.is_cuda:
        return _cpu.transform_images_window(data, desc, mean, std, to_bgr255, pad_hw)
    data, desc = _dev(data, "data", torch.uint8), _dev(desc, "desc", torch.int32)
    if data.dim() != 1 or desc.dim() != 2 or desc.shape[1] != 11 or max_in_hw is None:
        raise RuntimeError("transform_images_window: expected data [bytes] uint8, desc [B,11] int32 and max_in_hw")
    b, (pad_h, pad_w), (max_h, max_w) = desc.shape[0], (int(pad_hw[0]), int(pad_hw[1])), (int(max_in_hw[0]), int(max_in_hw[1]))
    m3, s3 = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
    with _on(data.device):
        nbytes = _L.ovis_transform_images_window_workspace_bytes(b, max_h, pad_w)
        out = torch.empty((b, 3, pad_h, pad_w), dtype=torch.float32, device=data.device)
        if b:
            ws = _workspace(nbytes, data.device, at_least=1)
            rc = _L.ovis_transform_images_window_u8(data.data_ptr(), data.numel(), desc.data_ptr(), b, max_h, max_w, m3, s3,
                                                    int(bool(to_bgr255)), pad_h, pad_w, ws.data_ptr(), nbytes, out.data_ptr(),
                                                    _stream())
            _lib.check(rc, "transform_images_window")
    return out


def color_jitter(data, desc, ops, params, max_in_hw=None, contrast=True):
    """uint8 [bytes]: the packed raw images of ``transform_images`` after ColorJitter (``ovis_color_jitter_u8``;
    data/transforms/transforms.py:88-102), with the bytes PIL produces; a new tensor, ``data`` is left as it is.  ops int32
    [B, 4]: per image the operations in application order (0 brightness, 1 contrast, 2 saturation, 3 hue, -1 unused trailing
    slot); params float32 [B, 4]: the factor of each slot, for hue the shift 0..255.  Device tensors: max_in_hw as for
    ``transform_images``; at most two launches, the tables are never read back.  ``contrast=False`` is the caller's
    statement that no row holds contrast: the grey-sum launch and its workspace are skipped.  Host tensors:
    ``libovis_cpu.so``, same bytes."""
    if not data.is_cuda:
        return _cpu.color_jitter(data, desc, ops, params)
    data, desc = _dev(data, "data", torch.uint8), _dev(desc, "desc", torch.int32)
    ops, params = _dev(ops, "ops", torch.int32), _dev(params, "params")
    b = desc.shape[0] if desc.dim() == 2 else -1
    if (data.dim() != 1 or desc.dim() != 2 or desc.shape[1] != 7 or tuple(ops.shape) != (b, 4) or tuple(params.shape) != (b, 4)
            or max_in_hw is None):
        raise RuntimeError("color_jitter: expected data [bytes] uint8, desc [B,7] int32, ops [B,4] int32, params [B,4] float32 "
                           "and max_in_hw")
    max_h, max_w = int(max_in_hw[0]), int(max_in_hw[1])
    with _on(data.device):
        out = torch.empty_like(data)
        if b:
            nbytes = _L.ovis_color_jitter_workspace_bytes(b) if contrast else 0
            ws = _workspace(nbytes, data.device)
            rc = _L.ovis_color_jitter_u8(data.data_ptr(), data.numel(), desc.data_ptr(), ops.data_ptr(), params.data_ptr(), b,
                                         max_h, max_w, _ptr(ws), nbytes, out.data_ptr(), _stream())
            _lib.check(rc, "color_jitter")
    return out


COPY_PASTE_MAX_IMAGES = _lib.OVIS_BOX_DECODE_MAX_IMAGES  # the per-image alphas travel as kernel arguments


def copy_paste_masks(masks, num_own):
    """Copy-paste, the mask half (``ovis_copy_paste_masks_u8``; include/ovis_hip.h states the rule).  masks uint8
    [G_own + G_paste, h, w], the first ``num_own`` rows the image's own: they become ``mask & ~alpha`` IN PLACE.
    -> (alpha uint8 [h, w]: the OR of the pasted rows, 0 / 1; stats int32 [num_own, 6] = (pixels before, pixels after, x1,
    y1, x2, y2): the tight box of what is left, (0, 0, -1, -1) when nothing is).  Two launches on the current stream, no
    atomics, nothing read back."""
    _check_dev(masks, "masks", torch.uint8)
    num_own = int(num_own)
    if masks.dim() != 3 or not masks.is_contiguous() or not 0 <= num_own <= masks.shape[0]:
        raise RuntimeError("copy_paste_masks: contiguous [G_own + G_paste, h, w] uint8 masks and 0 <= num_own <= G expected")
    h, w = masks.shape[1], masks.shape[2]
    alpha = torch.empty((h, w), dtype=torch.uint8, device=masks.device)
    stats = torch.empty((num_own, 6), dtype=torch.int32, device=masks.device)
    with _on(masks.device):
        rc = _L.ovis_copy_paste_masks_u8(masks.data_ptr() if masks.shape[0] else 0, num_own, masks.shape[0] - num_own, h, w,
                                         alpha.data_ptr(), stats.data_ptr() if num_own else 0, _stream())
    _lib.check(rc, "copy_paste_masks")
    return alpha, stats


def copy_paste_images(batch, alphas, paste_src):
    """Copy-paste, the pixel half (``ovis_copy_paste_images_f32``), IN PLACE on batch float32 [B, C, pad_h, pad_w]:
    ``batch[i, c, y, x] = batch[paste_src[i], c, y, x]`` (its pre-paste bits) where ``alphas[i][y, x]`` is set.  alphas: per
    image a uint8 [h, w] device tensor no larger than the canvas (zero outside its frame), or None where paste_src[i] is -1;
    paste_src: B python ints.  At most COPY_PASTE_MAX_IMAGES images; one launch on the current stream.  -> batch."""
    _check_dev(batch, "batch")
    paste_src = [int(s) for s in paste_src]
    b = batch.shape[0] if batch.dim() == 4 else -1
    if batch.dim() != 4 or not batch.is_contiguous() or len(paste_src) != b or len(alphas) != b:
        raise RuntimeError("copy_paste_images: contiguous [B, C, pad_h, pad_w] float32 batch, B alphas and B sources expected")
    ptrs, hw = [], []
    for a, s in zip(alphas, paste_src):
        if s >= 0:
            if a is None or not a.is_cuda or a.device != batch.device or a.dtype != torch.uint8 or a.dim() != 2 \
                    or not a.is_contiguous():
                raise RuntimeError("copy_paste_images: a contiguous [h, w] uint8 alpha on the batch's device for every image "
                                   "with a source expected")
            ptrs.append(a.data_ptr())
            hw += [a.shape[0], a.shape[1]]
        else:
            ptrs.append(0)
            hw += [0, 0]
    if b:
        with _on(batch.device):
            rc = _L.ovis_copy_paste_images_f32(batch.data_ptr(), b, batch.shape[1], batch.shape[2], batch.shape[3],
                                               (ctypes.c_void_p * b)(*ptrs), (ctypes.c_int32 * (2 * b))(*hw),
                                               (ctypes.c_int32 * b)(*paste_src), _stream())
        _lib.check(rc, "copy_paste_images")
    return batch


def weighted_ce_fwd_bwd(logits, labels, bg_weight, need_grad=True):
    """-> (loss scalar tensor, dlogits or None)"""
    if not logits.is_cuda:
        return _cpu.weighted_ce_fwd_bwd(logits, labels, bg_weight, need_grad)
    logits, labels = _dev(logits, "logits"), _dev(labels, "labels", torch.int64)
    p, c = logits.shape
    loss = torch.empty((1,), dtype=torch.float32, device=logits.device)
    dlogits = torch.empty_like(logits) if need_grad else None
    scratch = torch.empty((max(p, 1),), dtype=torch.float32, device=logits.device)
    with _on(logits.device):
        rc = _L.ovis_weighted_ce_fwd_bwd_f32(logits.data_ptr(), labels.data_ptr(), bg_weight, loss.data_ptr(),
                                             _ptr(dlogits), scratch.data_ptr(), p, c, _stream())
    _lib.check(rc, "weighted_ce_fwd_bwd")
    return loss[0], dlogits


def mask_bce_stochastic_fwd_bwd(mu, sigma, eps, pos_index, targets, channel, need_grad=True):
    """mu [P,C,M,M]; sigma [P,1,M,M] or None; eps [P,C,M,M] or None; pos_index [Pp]; targets [Pp,M,M]; channel: int (one
    logit channel for every positive: class-agnostic masks) or int64 tensor [Pp] (the positives' class labels:
    mask_logits[positive_inds, labels_pos], mask_head/loss.py:131-141) -> (loss, dmu or None, dsigma or None)"""
    if not mu.is_cuda:
        return _cpu.mask_bce_stochastic_fwd_bwd(mu, sigma, eps, pos_index, targets, channel, need_grad)
    mu = _dev(mu, "mu")
    p, c = mu.shape[0], mu.shape[1]
    mm = mu.shape[2] * mu.shape[3]
    pos_index, targets = _dev(pos_index, "pos_index", torch.int64), _dev(targets, "targets")
    sigma = None if sigma is None else _dev(sigma, "sigma")
    eps = None if eps is None else _dev(eps, "eps")
    npos = pos_index.numel()
    loss = torch.empty((1,), dtype=torch.float32, device=mu.device)
    dmu = torch.empty_like(mu) if need_grad else None
    dsigma = torch.empty((p, 1, mu.shape[2], mu.shape[3]), dtype=torch.float32, device=mu.device) \
        if (need_grad and sigma is not None) else None
    scratch = torch.empty((max(npos, 1),), dtype=torch.float32, device=mu.device)
    with _on(mu.device):
        if torch.is_tensor(channel):
            channel = _dev(channel, "channel", torch.int64)
            if channel.numel() != npos:
                raise RuntimeError(f"mask_bce_stochastic_fwd_bwd: {channel.numel()} channels for {npos} positives")
            rc = _L.ovis_mask_bce_stochastic_classes_fwd_bwd_f32(mu.data_ptr(), _ptr(sigma), _ptr(eps), pos_index.data_ptr(),
                                                                 channel.data_ptr(), targets.data_ptr(), loss.data_ptr(),
                                                                 _ptr(dmu), _ptr(dsigma), scratch.data_ptr(), p, npos, c, mm,
                                                                 _stream())
        else:
            rc = _L.ovis_mask_bce_stochastic_fwd_bwd_f32(mu.data_ptr(), _ptr(sigma), _ptr(eps), pos_index.data_ptr(),
                                                         targets.data_ptr(), loss.data_ptr(), _ptr(dmu), _ptr(dsigma),
                                                         scratch.data_ptr(), p, npos, c, mm, channel, _stream())
    _lib.check(rc, "mask_bce_stochastic_fwd_bwd")
    return loss[0], dmu, dsigma


# ---- deformable convolution (csrc/deform_conv.h:11-190; host loops deform_conv_cuda.cu:161-694) ---------
def _gemm_raw(a_ptr, a_rs, a_ks, b_ptr, b_rs, b_ks, c_ptr, c_rs, m, n, k, bias_ptr=0, bias_per_row=0, alpha=1.0,
              accumulate=0, device=None):
    """C = alpha * A . B^T (+ C) + bias on raw pointers.  Products with too few tiles to fill the chip are cut along K
    into slabs of a workspace allocated here (summed in slice order by the library: no atomics)."""
    ws_bytes = _gemm_f32_ws_bytes(m, n, k)
    ws = _workspace(ws_bytes, device or torch.device("cuda", torch.cuda.current_device()))
    rc = _L.ovis_gemm_ex_ws_f32(a_ptr, a_rs, a_ks, b_ptr, b_rs, b_ks, bias_ptr, bias_per_row, alpha, accumulate, c_ptr,
                                c_rs, m, n, k, _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "gemm_ex_ws_f32")


dcn_implicit = True  # False: the column route (im2col + GEMM) also where the implicit GEMM applies (cross-check in the tests)


def _dcn_dims(input, weight, kH, kW, dH, dW, padH, padW, dilH, dilW):
    b, cin, h, w = input.shape
    ho = (h + 2 * padH - (dilH * (kH - 1) + 1)) // dH + 1
    wo = (w + 2 * padW - (dilW * (kW - 1) + 1)) // dW + 1
    if ho <= 0 or wo <= 0:
        raise RuntimeError(f"deform_conv: output size is too small ({ho}x{wo})")
    return b, cin, h, w, ho, wo


def _dcn_check(input, weight, offset, mask, kH, kW, group, dg, ho, wo):
    b, cin = input.shape[0], input.shape[1]
    if weight.dim() != 4 or weight.shape[2] != kH or weight.shape[3] != kW:
        raise RuntimeError("deform_conv: kernel size does not match the weight")
    if cin % group or weight.shape[0] % group or weight.shape[1] != cin // group or cin % dg:
        raise RuntimeError("deform_conv: channels are not divisible by group / deformable_group")
    if tuple(offset.shape) != (b, dg * 2 * kH * kW, ho, wo):
        raise RuntimeError(f"deform_conv: invalid offset shape {tuple(offset.shape)}")
    if mask is not None and tuple(mask.shape) != (b, dg * kH * kW, ho, wo):
        raise RuntimeError(f"deform_conv: invalid mask shape {tuple(mask.shape)}")


def _dcn_forward(input, weight, bias, offset, mask, output, kH, kW, dH, dW, padH, padW, dilH, dilW, group, dg, step):
    input, weight, offset = _dev(input, "input"), _dev(weight, "weight"), _dev(offset, "offset")
    mask = None if mask is None else _dev(mask, "mask")
    b, cin, h, w, ho, wo = _dcn_dims(input, weight, kH, kW, dH, dW, padH, padW, dilH, dilW)
    _dcn_check(input, weight, offset, mask, kH, kW, group, dg, ho, wo)
    cout = weight.shape[0]
    if tuple(output.shape) != (b, cout, ho, wo) or not output.is_contiguous():
        raise RuntimeError("deform_conv: output must be a contiguous [B, C_out, H_out, W_out] tensor")
    K, plane = kH * kW, ho * wo
    cin_g, cout_g = cin // group, cout // group
    if dcn_implicit and group == 1 and (cin // dg) % 32 == 0 and cout % 4 == 0 and b * plane > 0:
        # no column buffer: one implicit GEMM on the pair-layout split GEMM, the A tiles sampled in the kernel
        x_nhwc = input.permute(0, 2, 3, 1).contiguous()
        wp, _ = weight_prep_pair(weight, None)
        rows = torch.empty((b * plane, cout), dtype=torch.float32, device=input.device)
        with _on(input.device):
            rc = _L.ovis_deform_conv_implicit_f32(x_nhwc.data_ptr(), offset.data_ptr(),
                                                  _ptr(mask), wp.data_ptr(), 2 * wp.stride(0),
                                                  0 if bias is None else _dev(bias, "bias").data_ptr(), rows.data_ptr(),
                                                  cout, b, cin, h, w, cout, ho, wo, kH, kW, dH, dW, padH, padW, dilH, dilW,
                                                  dg, _stream())
        _lib.check(rc, "deform_conv_implicit")
        output.copy_(rows.view(b, ho, wo, cout).permute(0, 3, 1, 2))
        return 1
    step = max(1, min(step, b))
    col = torch.empty((cin * K, step, plane), dtype=torch.float32, device=input.device)
    with _on(input.device):
        for s0 in range(0, b, step):
            nb = min(step, b - s0)
            rc = _L.ovis_deform_im2col_f32(input[s0].data_ptr(), offset[s0].data_ptr(),
                                           0 if mask is None else mask[s0].data_ptr(), col.data_ptr(), nb, cin, h, w,
                                           kH, kW, padH, padW, dH, dW, dilH, dilW, dg, _stream())
            _lib.check(rc, "deform_im2col")
            for i in range(nb):
                for g in range(group):
                    _gemm_raw(weight[g * cout_g].data_ptr(), cin_g * K, 1,
                              col.data_ptr() + 4 * ((g * cin_g * K) * nb * plane + i * plane), 1, nb * plane,
                              output[s0 + i, g * cout_g].data_ptr(), plane, cout_g, plane, cin_g * K,
                              0 if bias is None else bias[g * cout_g:].data_ptr(), 1)
    return 1


def deform_conv_forward(input, weight, offset, output, columns, ones, kW, kH, dW, dH, padW, padH, dilationW,
                        dilationH, group, deformable_group, im2col_step):
    """Writes ``output`` in place; ``columns`` / ``ones`` are accepted for signature compatibility (the reference
    re-allocates them internally as well, deform_conv_cuda.cu:207-214).  Note W-before-H argument order."""
    return _dcn_forward(input, weight, None, offset, None, output, kH, kW, dH, dW, padH, padW, dilationH, dilationW,
                        group, deformable_group, im2col_step)


def _dcn_backward(input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask, grad_weight, scale,
                  kH, kW, dH, dW, padH, padW, dilH, dilW, group, dg, step):
    input, weight, offset = _dev(input, "input"), _dev(weight, "weight"), _dev(offset, "offset")
    grad_output = _dev(grad_output, "grad_output")
    mask = None if mask is None else _dev(mask, "mask")
    b, cin, h, w, ho, wo = _dcn_dims(input, weight, kH, kW, dH, dW, padH, padW, dilH, dilW)
    _dcn_check(input, weight, offset, mask, kH, kW, group, dg, ho, wo)
    cout = weight.shape[0]
    K, plane = kH * kW, ho * wo
    cin_g, cout_g = cin // group, cout // group
    step = max(1, min(step, b))
    for t in (grad_input, grad_offset, grad_mask, grad_weight):
        if t is not None and not t.is_contiguous():
            raise RuntimeError("deform_conv backward: gradient buffers must be contiguous")
    if dcn_implicit and group == 1 and (cin // dg) % 32 == 0 and cout % 32 == 0 and b * plane > 0:
        return _dcn_backward_rows(input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask, grad_weight,
                                  scale, kH, kW, dH, dW, padH, padW, dilH, dilW, dg, b, cin, h, w, ho, wo, cout)
    col = torch.empty((cin * K, step, plane), dtype=torch.float32, device=input.device)
    with _on(input.device):
        for s0 in range(0, b, step):
            nb = min(step, b - s0)
            if grad_input is not None or grad_offset is not None:
                # columns = W^T . grad_output  (per image, per group)
                for i in range(nb):
                    for g in range(group):
                        _gemm_raw(weight[g * cout_g].data_ptr(), 1, cin_g * K,
                                  grad_output[s0 + i, g * cout_g].data_ptr(), 1, plane,
                                  col.data_ptr() + 4 * ((g * cin_g * K) * nb * plane + i * plane), nb * plane,
                                  cin_g * K, plane, cout_g)
                if grad_offset is not None:
                    rc = _L.ovis_deform_col2im_coord_f32(
                        col.data_ptr(), input[s0].data_ptr(), offset[s0].data_ptr(),
                        0 if mask is None else mask[s0].data_ptr(), grad_offset[s0].data_ptr(),
                        0 if grad_mask is None else grad_mask[s0].data_ptr(), nb, cin, h, w, kH, kW, padH, padW, dH,
                        dW, dilH, dilW, dg, _stream())
                    _lib.check(rc, "deform_col2im_coord")
                if grad_input is not None:
                    rc = _L.ovis_deform_col2im_f32(col.data_ptr(), offset[s0].data_ptr(),
                                                   0 if mask is None else mask[s0].data_ptr(),
                                                   grad_input[s0].data_ptr(), nb, cin, h, w, kH, kW, padH, padW, dH, dW,
                                                   dilH, dilW, dg, _stream())
                    _lib.check(rc, "deform_col2im")
            if grad_weight is not None:
                rc = _L.ovis_deform_im2col_f32(input[s0].data_ptr(), offset[s0].data_ptr(),
                                               0 if mask is None else mask[s0].data_ptr(), col.data_ptr(), nb, cin, h,
                                               w, kH, kW, padH, padW, dH, dW, dilH, dilW, dg, _stream())
                _lib.check(rc, "deform_im2col")
                for i in range(nb):
                    for g in range(group):
                        _gemm_raw(grad_output[s0 + i, g * cout_g].data_ptr(), plane, 1,
                                  col.data_ptr() + 4 * ((g * cin_g * K) * nb * plane + i * plane), nb * plane, 1,
                                  grad_weight[g * cout_g].data_ptr(), cin_g * K, cout_g, cin_g * K, plane,
                                  alpha=scale, accumulate=1)


def _dcn_backward_rows(input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask, grad_weight, scale,
                       kH, kW, dH, dW, padH, padW, dilH, dilW, dg, b, cin, h, w, ho, wo, cout):
    """The backward without the reference-layout column buffer (csrc/deform_conv_rows.hip): rows = (image, h_out, w_out),
    k = (tap, channel); dcol = dY . W as ONE split GEMM consumed by one scatter / gather pass (dX in NHWC with coalesced
    atomics, offset and mask gradients reduced in the wave), the weight gradient as ONE transpose-read split GEMM over the
    sampled rows written once in pair layout.  Same accumulate / overwrite conventions as the column route."""
    dev = input.device
    T, rows = kH * kW, b * ho * wo
    x_nhwc = input.permute(0, 2, 3, 1).contiguous()
    gy = grad_output.permute(0, 2, 3, 1).reshape(rows, cout)              # NHWC rows of dY
    gyp = split_pair(gy.contiguous())
    geom = (b, cin, h, w, ho, wo, kH, kW, dH, dW, padH, padW, dilH, dilW, dg)
    mptr = _ptr(mask)
    if grad_input is not None or grad_offset is not None:
        wt = split_pair(weight.permute(2, 3, 1, 0).reshape(T * cin, cout).contiguous())   # B[(t, c), n] = w[n, c, t]
        dcol, _ = split_gemm_pair(gyp, wt)                                                   # [rows, T * cin] f32
        dx = torch.zeros((b, h, w, cin), dtype=torch.float32, device=dev) if grad_input is not None else None
        if grad_offset is not None:
            grad_offset.zero_()
            if grad_mask is not None:
                grad_mask.zero_()
        with _on(dev):
            rc = _L.ovis_deform_col2im_rows_f32(dcol.data_ptr(), dcol.stride(0), x_nhwc.data_ptr(), offset.data_ptr(), mptr,
                                                _ptr(dx), _ptr(grad_offset), _ptr(grad_mask), *geom, _stream())
        _lib.check(rc, "deform_col2im_rows")
        if dx is not None:
            grad_input += dx.permute(0, 3, 1, 2)
    if grad_weight is not None:
        colp = torch.empty((rows, 2 * T * cin), dtype=torch.bfloat16, device=dev)
        with _on(dev):
            rc = _L.ovis_deform_im2col_pair_rows_f32(x_nhwc.data_ptr(), offset.data_ptr(), mptr, colp.data_ptr(),
                                                     2 * colp.stride(0), *geom, _stream())
        _lib.check(rc, "deform_im2col_pair_rows")
        if split_gemm_pair_tn_supported(cout, T * cin):
            dwm = split_gemm_pair_tn(gyp, colp)                                              # [cout, T * cin]
        else:  # shapes the transpose-read kernel does not take: one library bf16 product, the four hi / lo quadrants summed
            q = torch.mm(gyp.t(), colp, out_dtype=torch.float32)
            dwm = q.view(cout // 32, 2, 32, T * cin // 32, 2, 32).sum(dim=(1, 4)).reshape(cout, T * cin)
        grad_weight.add_(dwm.view(cout, kH, kW, cin).permute(0, 3, 1, 2), alpha=scale)


def deform_conv_backward_input(input, offset, gradOutput, gradInput, gradOffset, weight, columns, kW, kH, dW, dH, padW,
                               padH, dilationW, dilationH, group, deformable_group, im2col_step):
    """gradInput is accumulated into (callers pass zeros, dcn/deform_conv_func.py:85-86); gradOffset is overwritten."""
    _dcn_backward(input, weight, offset, None, gradOutput, gradInput, gradOffset, None, None, 1.0, kH, kW, dH, dW, padH,
                  padW, dilationH, dilationW, group, deformable_group, im2col_step)
    return 1


def deform_conv_backward_parameters(input, offset, gradOutput, gradWeight, columns, ones, kW, kH, dW, dH, padW, padH,
                                    dilationW, dilationH, group, deformable_group, scale, im2col_step):
    """gradWeight += scale * d(loss)/d(weight)."""
    _dcn_backward(input, gradWeight, offset, None, gradOutput, None, None, None, gradWeight, float(scale), kH, kW, dH,
                  dW, padH, padW, dilationH, dilationW, group, deformable_group, im2col_step)
    return 1


def modulated_deform_conv_forward(input, weight, bias, ones, offset, mask, output, columns, kernel_h, kernel_w, stride_h,
                                  stride_w, pad_h, pad_w, dilation_h, dilation_w, group, deformable_group, with_bias):
    _dcn_forward(input, weight, _dev(bias, "bias") if with_bias else None, offset, mask, output, kernel_h, kernel_w,
                 stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, deformable_group, 8)


def modulated_deform_conv_backward(input, weight, bias, ones, offset, mask, columns, grad_input, grad_weight, grad_bias,
                                   grad_offset, grad_mask, grad_output, kernel_h, kernel_w, stride_h, stride_w, pad_h,
                                   pad_w, dilation_h, dilation_w, group, deformable_group, with_bias):
    """grad_input / grad_weight / grad_bias are accumulated into (callers pass zeros); grad_offset / grad_mask are
    overwritten (deform_conv_cuda.cu:580-694)."""
    _dcn_backward(input, weight, offset, mask, grad_output, grad_input, grad_offset, grad_mask, grad_weight, 1.0,
                  kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group, deformable_group,
                  8)
    if with_bias:
        grad_bias += grad_output.sum(dim=(0, 2, 3))


# ---- optimizer (engine/solver.py) ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bottleneck_bwd_ws_bytes(m, cin, mid, kh, kw, w, config):
    return int(_L.ovis_bottleneck_identity_backward_workspace_bytes(m, cin, mid, kh, kw, w, config))


def bottleneck_identity_backward(g3p, xp, o1p, o2p, t1, t2, t3, scales, geom, weight_shapes, side_stream=None):
    """The backward of an identity bottleneck of a pair-only chain in ONE native call (``ovis_bottleneck_identity_backward``:
    the nine launches of the separate wrappers, the three weight gradients on ``side_stream`` beside the data-gradient chain).
    g3p [M, 2C] gated output gradient, xp / o1p / o2p the block's input and conv1 / conv2 outputs, t1 / t2 / t3 the transposed
    weight pair forms, scales (s1, s2, s3) or Nones, geom (h, w, kh, kw), weight_shapes (w1, w2, w3 shapes) ->
    (gx pair [M, 2C], dw1, dw2, dw3).  Pair tensors: 2-D bfloat16 with unit column stride."""
    _check_pairs("bottleneck_identity_backward", g3p=g3p, xp=xp, o1p=o1p, o2p=o2p, t1=t1, t2=t2, t3=t3)
    m, cin, mid = g3p.shape[0], g3p.shape[1] // 2, o1p.shape[1] // 2
    h, w, kh, kw = geom
    if (xp.shape != (m, 2 * cin) or o1p.shape[0] != m or o2p.shape != (m, 2 * mid) or t1.shape != (cin, 2 * mid)
            or t2.shape != (mid, 2 * kh * kw * mid) or t3.shape != (mid, 2 * cin) or m % (h * w)):
        raise RuntimeError("bottleneck_identity_backward: shape mismatch")
    dev = g3p.device
    g2p = torch.empty((m, 2 * mid), dtype=torch.bfloat16, device=dev)
    g1p = torch.empty((m, 2 * mid), dtype=torch.bfloat16, device=dev)
    gx = torch.empty((m, 2 * cin), dtype=torch.bfloat16, device=dev)
    dw1, dw2, dw3 = (torch.empty(tuple(sh), dtype=torch.float32, device=dev) for sh in weight_shapes)
    config = _gemm_cfg(0)
    ws = _workspace(_bottleneck_bwd_ws_bytes(m, cin, mid, kh, kw, w, config), dev, at_least=256)
    s1, s2, s3 = (None if s is None else _dev(s.detach(), "scale") for s in scales)
    with _on(dev):
        rc = _L.ovis_bottleneck_identity_backward(
            g3p.data_ptr(), 2 * g3p.stride(0), xp.data_ptr(), 2 * xp.stride(0), o1p.data_ptr(), 2 * o1p.stride(0),
            o2p.data_ptr(), 2 * o2p.stride(0), t1.data_ptr(), 2 * t1.stride(0), t2.data_ptr(), 2 * t2.stride(0),
            t3.data_ptr(), 2 * t3.stride(0), _ptr(s1), _ptr(s2), _ptr(s3), m, cin, mid, kh, kw, h, w, g2p.data_ptr(),
            g1p.data_ptr(), gx.data_ptr(), dw1.data_ptr(), dw2.data_ptr(), dw3.data_ptr(), ws.data_ptr(), ws.numel(), config,
            _stream(), 0 if side_stream is None else side_stream.cuda_stream)
    _lib.check(rc, "bottleneck_identity_backward")
    return gx, dw1, dw2, dw3


def weight_prep_tile():
    return int(_L.ovis_weight_prep_tile())


def weight_prep_pair_multi(items, blocks, max_taps):
    """One launch of the weight preparation over the convolutions described by ``items`` (uint8 device table of 64-byte
    records) and ``blocks`` (int32 [B, 2] = (item, 32 x 32 tile)); ``max_taps`` = the largest KH * KW in the table; see
    include/ovis_hip.h and layers/pair_bottleneck.py::WeightPrepPlan, which builds the tables."""
    if not (items.is_cuda and blocks.is_cuda and items.dtype == torch.uint8 and blocks.dtype == torch.int32):
        raise RuntimeError("weight_prep_pair_multi: uint8 / int32 HIP device tables expected")
    with _on(items.device):
        rc = _L.ovis_weight_prep_pair_multi_f32(items.data_ptr(), blocks.data_ptr(), blocks.size(0), int(max_taps), _stream())
    _lib.check(rc, "weight_prep_pair_multi")


def sgd_chunk_elements():
    return int(_L.ovis_sgd_chunk_elements())


def sgd_momentum_multi(items, blocks, lr, weight_decay, momentum, apply_weight_decay):
    """One launch of the fused SGD update over the tensors described by ``items`` (uint8 device table of 32-byte records
    {p, g, buf, n}) and ``blocks`` (int32 [B, 2] = (item, chunk)); see include/ovis_hip.h."""
    if not (items.is_cuda and blocks.is_cuda):
        raise RuntimeError("sgd_momentum_multi: HIP device tensors only")
    with _on(items.device):
        rc = _L.ovis_sgd_momentum_multi_f32(items.data_ptr(), blocks.data_ptr(), blocks.size(0), lr, weight_decay, momentum,
                                            int(bool(apply_weight_decay)), _stream())
    _lib.check(rc, "sgd_momentum_multi")


def sgd_momentum_ema_multi(items, blocks, lr, weight_decay, momentum, apply_weight_decay, ema_weight):
    """``sgd_momentum_multi`` with the weight average moved in the same pass: ``items`` = uint8 device table of 40-byte
    records {p, g, buf, ema, n}; behind the SGD update of an element, ema += (p_new - ema) * ``ema_weight`` (three fp32
    roundings; the rule is in include/ovis_hip.h)."""
    if not (items.is_cuda and blocks.is_cuda):
        raise RuntimeError("sgd_momentum_ema_multi: HIP device tensors only")
    with _on(items.device):
        rc = _L.ovis_sgd_momentum_ema_multi_f32(items.data_ptr(), blocks.data_ptr(), blocks.size(0), lr, weight_decay,
                                                momentum, int(bool(apply_weight_decay)), ema_weight, _stream())
    _lib.check(rc, "sgd_momentum_ema_multi")


def swap_multi(items, blocks):
    """One launch that exchanges a[i] and b[i] bit-wise, in place, over the tensor pairs of ``items`` (uint8 device table of
    24-byte records {a, b, n}, n in 4-byte elements); ``blocks`` as for ``sgd_momentum_multi``."""
    if not (items.is_cuda and blocks.is_cuda):
        raise RuntimeError("swap_multi: HIP device tensors only")
    with _on(items.device):
        rc = _L.ovis_swap_multi_f32(items.data_ptr(), blocks.data_ptr(), blocks.size(0), _stream())
    _lib.check(rc, "swap_multi")


# ---- COCO scoring (evaluation/coco/coco_eval.py:315-333 -> pycocotools' COCOeval; csrc/coco_eval.hip) -------------------
class CocoProblems:
    """The (image, category) problems of a chunk of images, the table of include/ovis_hip.h: ``table`` HOST int64 [P, 8] =
    (det_start, det_count, gt_start, gt_count, iou_offset, det_word_start, gt_word_start, words_per_mask).  Kept on the
    host (the ops check every row against their buffers there: the kernels trust the table) and uploaded once."""

    def __init__(self, table, device):
        table = torch.as_tensor(table, dtype=torch.int64).reshape(-1, 8).contiguous()
        if table.is_cuda or bool((table < 0).any()):
            raise RuntimeError("CocoProblems: a host table of non-negative int64 [P, 8] expected")
        self.host = table
        self.pairs = table[:, 1] * table[:, 3]
        self.max_pairs = int(self.pairs.max()) if len(table) else 0
        self.max_gts = int(table[:, 3].max()) if len(table) else 0
        self.iou_numel = int((table[:, 4] + self.pairs).max()) if len(table) else 0
        self.dev = table.to(device)

    def __len__(self):
        return self.host.shape[0]

    @classmethod
    def dense(cls, num_dets, num_gts, device, words=0):
        """One problem over all rows: its IoU block is the whole [num_dets, num_gts] matrix."""
        return cls([[0, num_dets, 0, num_gts, 0, 0, 0, words]], device)

    def check(self, what, num_dets, num_gts, iou_numel=None, det_words=None, gt_words=None):
        t = self.host
        bad = (t[:, 0] + t[:, 1] > num_dets) | (t[:, 2] + t[:, 3] > num_gts)
        if iou_numel is not None:
            bad |= t[:, 4] + self.pairs > iou_numel
        if det_words is not None:
            bad |= (t[:, 5] + t[:, 1] * t[:, 7] > det_words) | (t[:, 6] + t[:, 3] * t[:, 7] > gt_words)
        if bool(bad.any()):
            raise RuntimeError(f"{what}: problem {int(torch.nonzero(bad)[0])} of the table points outside its buffers")


def coco_box_iou(dets, gts, gt_crowd, problems=None):
    """fp64 IoU of xywh boxes, COCOeval.computeIoU for bbox (``ovis_coco_box_iou_f64``): dets [D, 4], gts [G, 4] fp64,
    gt_crowd [G] uint8 (a crowd's union is the detection's area).  Without ``problems``: the dense [D, G] matrix; with a
    ``CocoProblems``: the flat buffer that holds every problem's block.  Bit-identical to the formula in
    include/ovis_hip.h."""
    dets, gts = _dev(dets, "dets", torch.float64), _dev(gts, "gts", torch.float64)
    gt_crowd = _dev(gt_crowd, "gt_crowd", torch.uint8)
    if dets.dim() != 2 or dets.shape[1] != 4 or gts.dim() != 2 or gts.shape[1] != 4 or gt_crowd.shape != (gts.shape[0],):
        raise RuntimeError("coco_box_iou: expected dets [D,4], gts [G,4] and gt_crowd [G]")
    d, g = dets.shape[0], gts.shape[0]
    dense = problems is None
    if dense and (d == 0 or g == 0):
        return torch.empty((d, g), dtype=torch.float64, device=dets.device)
    if dense:
        problems = CocoProblems.dense(d, g, dets.device)
    problems.check("coco_box_iou", d, g)
    out = torch.zeros((problems.iou_numel,), dtype=torch.float64, device=dets.device)
    if problems.max_pairs:
        with _on(dets.device):
            rc = _L.ovis_coco_box_iou_f64(dets.data_ptr(), gts.data_ptr(), gt_crowd.data_ptr(), problems.dev.data_ptr(),
                                          len(problems), problems.max_pairs, out.data_ptr(), _stream())
        _lib.check(rc, "coco_box_iou")
    return out.view(d, g) if dense else out


def coco_pack_masks(masks):
    """(words int64 [P, ceil(H * W / 64)], areas int64 [P]): bool / uint8 masks [P, H, W] -- what ``paste_masks`` and
    ``polygons_to_masks`` return -- as bit words (pixel p of the row-major mask = bit p % 64 of word p / 64, the tail
    zero-filled) and their pixel counts (``ovis_coco_pack_masks_u64``).  The words are stored in int64 tensors."""
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)
    masks = _dev(masks, "masks", torch.uint8)
    if masks.dim() != 3:
        raise RuntimeError("coco_pack_masks: expected masks [P,H,W]")
    p, pixels = masks.shape[0], masks.shape[1] * masks.shape[2]
    words = torch.empty((p, (pixels + 63) // 64), dtype=torch.int64, device=masks.device)
    areas = torch.empty((p,), dtype=torch.int64, device=masks.device)
    if p == 0 or pixels == 0:
        return words, areas.zero_()
    with _on(masks.device):
        rc = _L.ovis_coco_pack_masks_u64(masks.data_ptr(), p, pixels, words.data_ptr(), areas.data_ptr(), _stream())
    _lib.check(rc, "coco_pack_masks")
    return words, areas


def coco_mask_iou(det_words, det_areas, gt_words, gt_areas, gt_crowd, problems=None):
    """fp64 IoU of packed masks, COCOeval.computeIoU for segm (``ovis_coco_mask_iou_f64``): the intersection is the
    popcount of the ANDed words, the result the ratio of two integers -- exact.  Without ``problems``: det_words [D, Wn],
    gt_words [G, Wn] -> [D, G]; with a ``CocoProblems``: flat word buffers addressed by the table -> the flat IoU buffer."""
    det_words, gt_words = _dev(det_words, "det_words", torch.int64), _dev(gt_words, "gt_words", torch.int64)
    det_areas, gt_areas = _dev(det_areas, "det_areas", torch.int64), _dev(gt_areas, "gt_areas", torch.int64)
    gt_crowd = _dev(gt_crowd, "gt_crowd", torch.uint8)
    d, g = det_areas.numel(), gt_areas.numel()
    if gt_crowd.shape != (g,):
        raise RuntimeError("coco_mask_iou: expected gt_crowd [G]")
    dense = problems is None
    if dense:
        if det_words.dim() != 2 or gt_words.dim() != 2 or det_words.shape[0] != d or gt_words.shape[0] != g \
                or det_words.shape[1] != gt_words.shape[1]:
            raise RuntimeError("coco_mask_iou: expected det_words [D,Wn] and gt_words [G,Wn]")
        if d == 0 or g == 0:
            return torch.empty((d, g), dtype=torch.float64, device=det_words.device)
        problems = CocoProblems.dense(d, g, det_words.device, det_words.shape[1])
    problems.check("coco_mask_iou", d, g, det_words=det_words.numel(), gt_words=gt_words.numel())
    out = torch.zeros((problems.iou_numel,), dtype=torch.float64, device=det_words.device)
    if problems.max_pairs:
        with _on(det_words.device):
            rc = _L.ovis_coco_mask_iou_f64(det_words.data_ptr(), det_areas.data_ptr(), gt_words.data_ptr(), gt_areas.data_ptr(),
                                           gt_crowd.data_ptr(), problems.dev.data_ptr(), len(problems), problems.max_pairs,
                                           out.data_ptr(), _stream())
        _lib.check(rc, "coco_mask_iou")
    return out.view(d, g) if dense else out


def coco_boundary_words(words, height, width, dilation):
    """(boundary words int64 [P, Wn], boundary areas int64 [P]) of packed masks ``words`` [P, Wn = ceil(height * width /
    64)] of ONE image size (``coco_pack_masks``' layout): ``m & ~eroded(m)``, eroded = ``dilation`` iterations of a 3x3
    erosion with the outside of the image 0 (``ovis_coco_boundary_words_u64``; the rule: include/ovis_hip.h).  The caller
    computes ``dilation`` (engine/coco_eval.py: ``boundary_dilation``).  Enqueue only; P words of scratch are allocated."""
    words = _dev(words, "words", torch.int64)
    height, width, dilation = int(height), int(width), int(dilation)
    if words.dim() != 2 or (height >= 1 and width >= 1 and words.shape[1] != (height * width + 63) // 64):
        raise RuntimeError(f"coco_boundary_words: expected words [P, ceil({height} * {width} / 64)], got {tuple(words.shape)}")
    p = words.shape[0]
    out, areas = torch.empty_like(words), torch.zeros((p,), dtype=torch.int64, device=words.device)
    scratch = torch.empty_like(words)
    with _on(words.device):
        rc = _L.ovis_coco_boundary_words_u64(words.data_ptr() if p else 0, p, height, width, dilation,
                                             scratch.data_ptr() if p else 0, out.data_ptr() if p else 0,
                                             areas.data_ptr() if p else 0, _stream())
    _lib.check(rc, "coco_boundary_words")
    return out, areas


def coco_boundary_iou(det_words, det_bwords, det_areas, det_bareas, gt_words, gt_bwords, gt_areas, gt_bareas, gt_crowd,
                      problems=None):
    """fp64 min(mask IoU, boundary IoU) of packed masks and their boundaries (``coco_boundary_words``) -- the IoU Boundary AP
    matches (``ovis_coco_boundary_iou_f64``): both ratios as in ``coco_mask_iou``, the crowd form included, so exact and
    elementwise <= ``coco_mask_iou`` of the same masks.  Without ``problems``: words [D, Wn] / [G, Wn] -> [D, G]; with a
    ``CocoProblems``: flat word buffers addressed by the table (the boundary words lie as the mask words do) -> the flat IoU
    buffer ``coco_match`` takes."""
    det_words, gt_words = _dev(det_words, "det_words", torch.int64), _dev(gt_words, "gt_words", torch.int64)
    det_bwords, gt_bwords = _dev(det_bwords, "det_bwords", torch.int64), _dev(gt_bwords, "gt_bwords", torch.int64)
    det_areas, gt_areas = _dev(det_areas, "det_areas", torch.int64), _dev(gt_areas, "gt_areas", torch.int64)
    det_bareas, gt_bareas = _dev(det_bareas, "det_bareas", torch.int64), _dev(gt_bareas, "gt_bareas", torch.int64)
    gt_crowd = _dev(gt_crowd, "gt_crowd", torch.uint8)
    d, g = det_areas.numel(), gt_areas.numel()
    if gt_crowd.shape != (g,) or det_bareas.numel() != d or gt_bareas.numel() != g \
            or det_bwords.shape != det_words.shape or gt_bwords.shape != gt_words.shape:
        raise RuntimeError("coco_boundary_iou: expected gt_crowd [G], boundary areas [D] / [G] and boundary words shaped "
                           "as the mask words")
    dense = problems is None
    if dense:
        if det_words.dim() != 2 or gt_words.dim() != 2 or det_words.shape[0] != d or gt_words.shape[0] != g \
                or det_words.shape[1] != gt_words.shape[1]:
            raise RuntimeError("coco_boundary_iou: expected det_words [D,Wn] and gt_words [G,Wn]")
        if d == 0 or g == 0:
            return torch.empty((d, g), dtype=torch.float64, device=det_words.device)
        problems = CocoProblems.dense(d, g, det_words.device, det_words.shape[1])
    problems.check("coco_boundary_iou", d, g, det_words=det_words.numel(), gt_words=gt_words.numel())
    out = torch.zeros((problems.iou_numel,), dtype=torch.float64, device=det_words.device)
    if problems.max_pairs:
        with _on(det_words.device):
            rc = _L.ovis_coco_boundary_iou_f64(det_words.data_ptr(), det_bwords.data_ptr(), det_areas.data_ptr(),
                                               det_bareas.data_ptr(), gt_words.data_ptr(), gt_bwords.data_ptr(),
                                               gt_areas.data_ptr(), gt_bareas.data_ptr(), gt_crowd.data_ptr(),
                                               problems.dev.data_ptr(), len(problems), problems.max_pairs, out.data_ptr(),
                                               _stream())
        _lib.check(rc, "coco_boundary_iou")
    return out.view(d, g) if dense else out


def coco_match(iou, problems, det_areas, gt_areas, gt_crowd, area_ranges, thresholds):
    """COCOeval.evaluateImg for every problem, area range and IoU threshold in one launch (``ovis_coco_match``).  iou:
    the flat fp64 buffer of ``coco_box_iou`` / ``coco_mask_iou`` for the same ``problems``; det_areas [D], gt_areas [G]
    fp64, gt_crowd [G] uint8, area_ranges [A, 2] and thresholds [T] fp64, all on the device.  -> (dt_match int32
    [A, T, D]: the matched ground truth's index inside its problem or -1, dt_ignore bool [A, T, D], gt_ignore bool
    [A, G]).  Rows no problem covers come back as -1 / False."""
    iou, det_areas, gt_areas = _dev(iou, "iou", torch.float64), _dev(det_areas, "det_areas", torch.float64), \
        _dev(gt_areas, "gt_areas", torch.float64)
    gt_crowd = _dev(gt_crowd, "gt_crowd", torch.uint8)
    area_ranges, thresholds = _dev(area_ranges, "area_ranges", torch.float64), _dev(thresholds, "thresholds", torch.float64)
    if area_ranges.dim() != 2 or area_ranges.shape[1] != 2 or thresholds.dim() != 1 or gt_crowd.shape != gt_areas.shape \
            or det_areas.dim() != 1 or gt_areas.dim() != 1 or not area_ranges.numel() or not thresholds.numel():
        raise RuntimeError("coco_match: expected det_areas [D], gt_areas / gt_crowd [G], area_ranges [A,2], thresholds [T]")
    d, g, a, t = det_areas.numel(), gt_areas.numel(), area_ranges.shape[0], thresholds.numel()
    problems.check("coco_match", d, g, iou_numel=iou.numel())
    dt_match = torch.full((a, t, d), -1, dtype=torch.int32, device=iou.device)
    dt_ignore = torch.zeros((a, t, d), dtype=torch.bool, device=iou.device)
    gt_ignore = torch.zeros((a, g), dtype=torch.bool, device=iou.device)
    if len(problems) == 0:
        return dt_match, dt_ignore, gt_ignore
    with _on(iou.device):
        rc = _L.ovis_coco_match(iou.data_ptr() if iou.numel() else 0, problems.dev.data_ptr(), len(problems), problems.max_gts,
                                det_areas.data_ptr() if d else 0, gt_areas.data_ptr() if g else 0,
                                gt_crowd.data_ptr() if g else 0, area_ranges.data_ptr(), a, thresholds.data_ptr(), t, d, g,
                                dt_match.data_ptr() if d else 0, dt_ignore.data_ptr() if d else 0,
                                gt_ignore.data_ptr() if g else 0, _stream())
    _lib.check(rc, "coco_match")
    return dt_match, dt_ignore, gt_ignore


def lvis_match(iou, problems, det_areas, gt_areas, gt_ignore_in, problem_not_exhaustive, area_ranges, thresholds):
    """The matching of LVIS-style federated scoring (rules 7 and 8 of include/ovis_hip.h) for every problem, area range and
    IoU threshold in one launch (``ovis_lvis_match``): ``coco_match``'s inputs and outputs, with gt_ignore_in [G] uint8 (the
    ground truths' input ignore flags; a matched ground truth is never matched again) in place of gt_crowd, and
    problem_not_exhaustive [P] uint8, one flag per row of ``problems``, ORed into the ignore flag of that problem's
    unmatched detections.  ``iou`` is the non-crowd form: the buffer of ``coco_box_iou`` / ``coco_mask_iou`` /
    ``coco_boundary_iou`` called with all-zero crowd flags."""
    iou, det_areas, gt_areas = _dev(iou, "iou", torch.float64), _dev(det_areas, "det_areas", torch.float64), \
        _dev(gt_areas, "gt_areas", torch.float64)
    gt_ignore_in = _dev(gt_ignore_in, "gt_ignore_in", torch.uint8)
    problem_not_exhaustive = _dev(problem_not_exhaustive, "problem_not_exhaustive", torch.uint8)
    area_ranges, thresholds = _dev(area_ranges, "area_ranges", torch.float64), _dev(thresholds, "thresholds", torch.float64)
    if area_ranges.dim() != 2 or area_ranges.shape[1] != 2 or thresholds.dim() != 1 or gt_ignore_in.shape != gt_areas.shape \
            or det_areas.dim() != 1 or gt_areas.dim() != 1 or not area_ranges.numel() or not thresholds.numel() \
            or problem_not_exhaustive.shape != (len(problems),):
        raise RuntimeError("lvis_match: expected det_areas [D], gt_areas / gt_ignore_in [G], problem_not_exhaustive [P], "
                           "area_ranges [A,2], thresholds [T]")
    d, g, a, t = det_areas.numel(), gt_areas.numel(), area_ranges.shape[0], thresholds.numel()
    problems.check("lvis_match", d, g, iou_numel=iou.numel())
    dt_match = torch.full((a, t, d), -1, dtype=torch.int32, device=iou.device)
    dt_ignore = torch.zeros((a, t, d), dtype=torch.bool, device=iou.device)
    gt_ignore = torch.zeros((a, g), dtype=torch.bool, device=iou.device)
    if len(problems) == 0:
        return dt_match, dt_ignore, gt_ignore
    with _on(iou.device):
        rc = _L.ovis_lvis_match(iou.data_ptr() if iou.numel() else 0, problems.dev.data_ptr(), len(problems), problems.max_gts,
                                det_areas.data_ptr() if d else 0, gt_areas.data_ptr() if g else 0,
                                gt_ignore_in.data_ptr() if g else 0, problem_not_exhaustive.data_ptr(), area_ranges.data_ptr(),
                                a, thresholds.data_ptr(), t, d, g, dt_match.data_ptr() if d else 0,
                                dt_ignore.data_ptr() if d else 0, gt_ignore.data_ptr() if g else 0, _stream())
    _lib.check(rc, "lvis_match")
    return dt_match, dt_ignore, gt_ignore


ERROR_TYPES = ("none", "Cls", "Loc", "Both", "Dupe", "Bkg")  # the codes of err_type (include/ovis_hip.h, "Error analysis")


def error_types(iou, images, det_category, det_match, det_ignore, gt_category, gt_crowd, fg_threshold=0.5, bg_threshold=0.1):
    """The error type of every detection and the missed ground truths of a chunk of images (``ovis_error_types``; the rules:
    "Error analysis" in include/ovis_hip.h).  images: a ``CocoProblems`` with ONE ROW PER IMAGE; iou: the flat fp64 buffer
    ``coco_box_iou`` / ``coco_mask_iou`` return for that table -- every detection of an image against every ground truth of
    it; det_category int32 [D]; det_match int32 [D], the chunk-global row of the ground truth the base matching gave the
    detection or -1; det_ignore uint8 [D]; gt_category int32 [G]; gt_crowd uint8 [G]; all on the device.  -> (err_type uint8
    [D]: the index into ``ERROR_TYPES``, err_gt int32 [D]: the chunk-global row of the target or -1, gt_missed uint8 [G]).
    Rows no image of the table covers come back as 0 / -1 / 0."""
    iou = _dev(iou, "iou", torch.float64)
    det_category, det_match = _dev(det_category, "det_category", torch.int32), _dev(det_match, "det_match", torch.int32)
    det_ignore = _dev(det_ignore, "det_ignore", torch.uint8)
    gt_category, gt_crowd = _dev(gt_category, "gt_category", torch.int32), _dev(gt_crowd, "gt_crowd", torch.uint8)
    if det_category.dim() != 1 or det_match.shape != det_category.shape or det_ignore.shape != det_category.shape \
            or gt_category.dim() != 1 or gt_crowd.shape != gt_category.shape:
        raise RuntimeError("error_types: expected det_category / det_match / det_ignore [D] and gt_category / gt_crowd [G]")
    d, g = det_category.numel(), gt_category.numel()
    images.check("error_types", d, g, iou_numel=iou.numel())
    host = images.host
    if len(images) > 1 and (bool((host[1:, 0] < host[:-1, 0] + host[:-1, 1]).any())
                            or bool((host[1:, 2] < host[:-1, 2] + host[:-1, 3]).any())):
        raise RuntimeError("error_types: the images of the table must hold disjoint, ascending row ranges")
    err_type = torch.zeros((d,), dtype=torch.uint8, device=iou.device)
    err_gt = torch.full((d,), -1, dtype=torch.int32, device=iou.device)
    gt_missed = torch.zeros((g,), dtype=torch.uint8, device=iou.device)
    if len(images) == 0 or (d == 0 and g == 0):
        return err_type, err_gt, gt_missed
    with _on(iou.device):
        rc = _L.ovis_error_types(iou.data_ptr() if iou.numel() else 0, images.dev.data_ptr(), len(images),
                                 int(host[:, 1].max()), images.max_gts, det_category.data_ptr() if d else 0,
                                 det_match.data_ptr() if d else 0, det_ignore.data_ptr() if d else 0,
                                 gt_category.data_ptr() if g else 0, gt_crowd.data_ptr() if g else 0, float(fg_threshold),
                                 float(bg_threshold), d, g, err_type.data_ptr() if d else 0, err_gt.data_ptr() if d else 0,
                                 gt_missed.data_ptr() if g else 0, _stream())
    _lib.check(rc, "error_types")
    return err_type, err_gt, gt_missed


COCO_RLE_STATUS = {_lib.OVIS_COCO_RLE_BAD_CHAR: "a character outside '0'..'o'",
                   _lib.OVIS_COCO_RLE_UNTERMINATED: "the last value is not terminated",
                   _lib.OVIS_COCO_RLE_OVERFLOW: "a value does not fit 32 bits",
                   _lib.OVIS_COCO_RLE_NEGATIVE_RUN: "a negative run",
                   _lib.OVIS_COCO_RLE_BAD_SUM: "the runs do not add up to height x width",
                   _lib.OVIS_COCO_RLE_BAD_SIZE: "height < 1, width < 1 or height x width > 0x7fffffef"}


def coco_rle_words(strings_or_runs, sizes):
    """(words int64 [total], word_offsets int64 [P + 1], areas int64 [P], status int32 [P]), all on the device of ``sizes``:
    the COCO RLE masks of a results file or of RLE annotations as the bit words of ``coco_pack_masks`` -- mask p's
    ``words[word_offsets[p]:word_offsets[p + 1]]`` equals ``coco_pack_masks`` of the decoded mask, ``areas[p]`` its pixel
    count (``ovis_coco_rle_count`` / ``_runs`` / ``ovis_coco_runs_to_words``; pycocotools' rleFrString + decode).
    ``strings_or_runs``: a list whose items are ``str`` / ``bytes`` (the compressed ``counts``) or integer sequences (the
    uncompressed ones), mixed freely; ``sizes``: int32 DEVICE tensor [P, 2] of (height, width), one per item -- masks of
    different sizes share a call.  Nothing is checked here beyond dtypes and lengths: ``status[p]`` is 0 for a good mask and
    a key of ``COCO_RLE_STATUS`` otherwise (all-zero words, area 0); the caller turns it into an error.  Integers outside
    int32 in a list are clamped to its ends (such a list cannot add up to a valid size).  Two host reads: the sizes and the
    value counts of the strings."""
    sizes = _dev(sizes, "sizes", torch.int32)
    items = list(strings_or_runs)
    p, dev = len(items), sizes.device
    if sizes.shape != (p, 2):
        raise RuntimeError(f"coco_rle_words: expected sizes int32 [{p},2] (height, width), one row per mask")
    if p > 65535:
        raise RuntimeError("coco_rle_words: at most 65535 masks a call")
    hw = sizes.cpu().long()
    pixels = hw[:, 0] * hw[:, 1]
    usable = (hw[:, 0] >= 1) & (hw[:, 1] >= 1) & (pixels <= 0x7fffffef)
    word_offsets_host = torch.zeros(p + 1, dtype=torch.int64)
    torch.cumsum(torch.where(usable, (pixels + 63) // 64, torch.zeros_like(pixels)), 0, out=word_offsets_host[1:])
    words = torch.empty(int(word_offsets_host[-1]), dtype=torch.int64, device=dev)
    areas, status = torch.empty(p, dtype=torch.int64, device=dev), torch.zeros(p, dtype=torch.int32, device=dev)
    word_offsets = word_offsets_host.to(dev)
    if p == 0:
        return words, word_offsets, areas, status
    texts, lists, lengths = [], {}, torch.zeros(p, dtype=torch.int64)
    for k, item in enumerate(items):
        if isinstance(item, str):
            texts.append(item.encode("latin-1", "replace"))  # a character beyond a byte becomes '?': refused by the kernel
        elif isinstance(item, (bytes, bytearray)):
            texts.append(bytes(item))
        else:
            texts.append(b"")
            values = torch.as_tensor(item).reshape(-1)
            if values.is_floating_point() or values.dtype == torch.bool or values.is_complex():
                raise RuntimeError(f"coco_rle_words: item {k} is neither a string nor a sequence of integers")
            lists[k] = values.long().clamp(-2 ** 31, 2 ** 31 - 1).int()
            lengths[k] = lists[k].numel()
    char_offsets_host = torch.zeros(p + 1, dtype=torch.int64)
    torch.cumsum(torch.tensor([len(t) for t in texts], dtype=torch.int64), 0, out=char_offsets_host[1:])
    if int(char_offsets_host[-1]) > 2 ** 31 - 1:
        raise RuntimeError("coco_rle_words: more than 2^31 - 1 characters in one call")
    compressed = len(lists) < p
    if compressed:
        chars = torch.frombuffer(bytearray(b"".join(texts)) or bytearray(1), dtype=torch.uint8).to(dev)
        char_offsets = char_offsets_host.to(dev)
        num_runs = torch.empty(p, dtype=torch.int32, device=dev)
        with _on(dev):
            rc = _L.ovis_coco_rle_count(chars.data_ptr(), char_offsets.data_ptr(), p, num_runs.data_ptr(), _stream())
        _lib.check(rc, "coco_rle_words")
        lengths = lengths + num_runs.cpu().long()
    run_offsets_host = torch.zeros(p + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=run_offsets_host[1:])
    run_offsets = run_offsets_host.to(dev)
    total = int(run_offsets_host[-1])
    if lists and not compressed:
        runs = torch.cat(list(lists.values())).to(dev)
    else:
        runs = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    if compressed:
        _coco_rle_runs(chars, char_offsets, run_offsets, p, runs, status)
        if lists:  # the uncompressed items of a mixed call, into their slices
            slots = torch.cat([torch.arange(len(v)) + run_offsets_host[k] for k, v in lists.items()])
            runs[slots.to(dev)] = torch.cat(list(lists.values())).to(dev)
    max_words = int((word_offsets_host[1:] - word_offsets_host[:-1]).max())
    _coco_runs_to_words(runs, run_offsets, total, sizes, word_offsets, p, max_words, words, areas, status)
    return words, word_offsets, areas, status


def _coco_rle_runs(chars, char_offsets, run_offsets, p, runs, status):
    with _on(runs.device):
        rc = _L.ovis_coco_rle_runs(chars.data_ptr(), char_offsets.data_ptr(), run_offsets.data_ptr(), p, runs.data_ptr(),
                                   status.data_ptr(), _stream())
    _lib.check(rc, "coco_rle_words")


def _coco_runs_to_words(runs, run_offsets, total_runs, sizes, word_offsets, p, max_words, words, areas, status):
    run_ends = torch.empty(max(total_runs, 1), dtype=torch.int32, device=runs.device)
    with _on(runs.device):
        rc = _L.ovis_coco_runs_to_words(runs.data_ptr(), run_offsets.data_ptr(), sizes.data_ptr(), word_offsets.data_ptr(), p,
                                        max_words, run_ends.data_ptr(), words.data_ptr() if words.numel() else 0,
                                        areas.data_ptr(), status.data_ptr(), _stream())
    _lib.check(rc, "coco_rle_words")


def coco_rle_words_staged(chars, char_offsets, runs, run_offsets, sizes, word_offsets, *, total_words, max_words,
                          compressed=True):
    """``coco_rle_words`` for inputs that are ALREADY on the device, with everything the host has to know handed in -- no
    device-to-host copy, so it can run on a training stream (``RleMasks.decode_many``; the same ``ovis_coco_rle_runs`` /
    ``ovis_coco_runs_to_words`` entry points; the value counts ``ovis_coco_rle_count`` would report come from the host, in
    ``run_offsets``).  chars uint8 [C] + char_offsets int64 [P + 1]: the compressed strings back to back (an uncompressed
    item has none); runs int32 [R] + run_offsets int64 [P + 1]: one slot per value of every item, an uncompressed item's
    values in place (the strings' slots are overwritten: ``runs`` is modified); sizes int32 [P, 2] (height, width);
    word_offsets int64 [P + 1] with mask p owning ceil(height * width / 64) words.  Host integers: ``total_words`` =
    word_offsets[P], ``max_words`` = the largest slice; ``compressed``: whether any item is a string.
    -> (words int64 [total_words], areas int64 [P], status int32 [P]) as ``coco_rle_words``."""
    chars, runs, sizes = _dev(chars, "chars", torch.uint8), _dev(runs, "runs", torch.int32), _dev(sizes, "sizes", torch.int32)
    char_offsets, run_offsets = _dev(char_offsets, "char_offsets", torch.int64), _dev(run_offsets, "run_offsets", torch.int64)
    word_offsets = _dev(word_offsets, "word_offsets", torch.int64)
    p, dev = sizes.shape[0], sizes.device
    if sizes.dim() != 2 or sizes.shape[1] != 2 or any(t.shape != (p + 1,) for t in (char_offsets, run_offsets, word_offsets)):
        raise RuntimeError(f"coco_rle_words_staged: expected sizes int32 [P,2] and three int64 [P + 1] offset tensors")
    if p > 65535:
        raise RuntimeError("coco_rle_words_staged: at most 65535 masks a call")
    words = torch.empty(int(total_words), dtype=torch.int64, device=dev)
    areas, status = torch.empty(p, dtype=torch.int64, device=dev), torch.zeros(p, dtype=torch.int32, device=dev)
    if p == 0:
        return words, areas, status
    if not runs.numel():
        runs = torch.empty(1, dtype=torch.int32, device=dev)
    if compressed:
        _coco_rle_runs(chars if chars.numel() else torch.empty(1, dtype=torch.uint8, device=dev), char_offsets, run_offsets, p,
                       runs, status)
    _coco_runs_to_words(runs, run_offsets, runs.numel(), sizes, word_offsets, p, int(max_words), words, areas, status)
    return words, areas, status


def project_rle_masks(rle_masks, gt_index, boxes, resolution):
    """Mask targets [P, resolution, resolution] f32 for boxes [P, 4] whose ground truth gt_index[p] is an instance of
    ``rle_masks`` (modeling/structures.py::RleMasks on the device): its recorded resize and flips, then crop + resize, from
    the decoded bit words in one launch (``ovis_project_rle_masks_f32``).  P == 0: empty, no launch."""
    boxes = _dev(boxes, "boxes")
    gt_index = _dev(gt_index, "gt_index", torch.int64)
    p = boxes.shape[0]
    out = torch.empty((p, resolution, resolution), dtype=torch.float32, device=boxes.device)
    if p == 0:
        return out
    if boxes.dim() != 2 or boxes.shape[1] != 4 or gt_index.shape != (p,):
        raise RuntimeError("project_rle_masks: expected boxes [P,4] and gt_index [P]")
    m = rle_masks.decoded()
    if m.words is None:
        raise RuntimeError("project_rle_masks: positives but no ground-truth mask")
    words, word_offsets = _dev(m.words, "words", torch.int64), _dev(m.word_offsets, "word_offsets", torch.int64)
    instance = _dev(m.instance, "instance", torch.int64)
    window = getattr(m, "window", None)
    (h0, w0), (w1, h1) = m.source_hw, (m.size if window is None else m.frame_size)
    with _on(boxes.device):
        if window is None:
            rc = _L.ovis_project_rle_masks_f32(words.data_ptr(), word_offsets.data_ptr(), word_offsets.numel() - 1,
                                               m.decoded_words_per_mask, instance.data_ptr() if instance.numel() else 0, instance.numel(),
                                               gt_index.data_ptr(), boxes.data_ptr(), p, h0, w0, h1, w1, int(m.flip_h),
                                               int(m.flip_v), int(resolution), out.data_ptr(), _stream())
        else:  # RleMasks.crop: (win_x, win_y, win_w, win_h) of the resized, flipped frame; the boxes are in the window's frame
            win_x, win_y, win_w, win_h = window
            rc = _L.ovis_project_rle_masks_window_f32(words.data_ptr(), word_offsets.data_ptr(), word_offsets.numel() - 1,
                                                      m.decoded_words_per_mask, instance.data_ptr() if instance.numel() else 0,
                                                      instance.numel(), gt_index.data_ptr(), boxes.data_ptr(), p, h0, w0, h1, w1,
                                                      int(m.flip_h), int(m.flip_v), win_y, win_x, win_h, win_w, int(resolution),
                                                      out.data_ptr(), _stream())
    _lib.check(rc, "project_rle_masks")
    return out


# ---- box-proposal recall (evaluation/coco/coco_eval.py:199-312; csrc/proposal_recall.hip) ---------------------------------
def proposal_gt_overlaps(proposals, gt_boxes, gt_areas, images, area_ranges, limits):
    """The matching of the reference's ``evaluate_box_proposals`` (coco_eval.py:269-290 over ``boxlist_iou``) for a chunk of
    images, every area range and every limit in one launch (``ovis_proposal_gt_overlaps``).  proposals [P, 4] and gt_boxes
    [G, 4] fp32 xyxy in one frame, proposals best first inside an image; gt_areas [G] fp32; area_ranges [A, 2] fp32 -- all on
    the device.  images: a HOST int64 [N, 4] table (prop_start, prop_count, gt_start, gt_count), checked here row by row
    against the buffers (the kernel trusts it) and uploaded; limits: a sequence of L positive ints.  -> fp32 [A, L, G]: per
    ground truth the IoU of the round that consumed it, 0 when it is inside the area range (both ends inclusive) but was
    never consumed, -1 when it is outside; rows of no image stay -1.  ValueError: a reversed box, x2 - x1 + 1 <= 0 or
    y2 - y1 + 1 <= 0 (its union with another box could be <= 0; x2 < x1 by less than a pixel is a decoded box narrower than
    a pixel, which the reference scores).  More ground truths in an image than ``_lib.OVIS_PROPOSAL_RECALL_MAX_GTS`` or a limit
    above ``_lib.OVIS_PROPOSAL_RECALL_MAX_LIMIT``: OVIS_ERANGE."""
    proposals, gt_boxes = _dev(proposals, "proposals"), _dev(gt_boxes, "gt_boxes")
    gt_areas, area_ranges = _dev(gt_areas, "gt_areas"), _dev(area_ranges, "area_ranges")
    if proposals.dim() != 2 or proposals.shape[1] != 4 or gt_boxes.dim() != 2 or gt_boxes.shape[1] != 4 \
            or gt_areas.shape != (gt_boxes.shape[0],) or area_ranges.dim() != 2 or area_ranges.shape[1] != 2 \
            or not area_ranges.shape[0]:
        raise RuntimeError("proposal_gt_overlaps: expected proposals [P,4], gt_boxes [G,4], gt_areas [G] and area_ranges [A,2]")
    table = torch.as_tensor(images, dtype=torch.int64).reshape(-1, 4).contiguous()
    if table.is_cuda or bool((table < 0).any()):
        raise RuntimeError("proposal_gt_overlaps: a host table of non-negative int64 [N, 4] expected")
    limits = torch.as_tensor(limits, dtype=torch.int32).reshape(-1)
    if limits.is_cuda or not limits.numel() or bool((limits < 1).any()):
        raise RuntimeError("proposal_gt_overlaps: limits is a host sequence of positive ints")
    p, g, a, n_limits = proposals.shape[0], gt_boxes.shape[0], area_ranges.shape[0], limits.numel()
    bad = (table[:, 0] + table[:, 1] > p) | (table[:, 2] + table[:, 3] > g)
    if bool(bad.any()):
        raise RuntimeError(f"proposal_gt_overlaps: image {int(torch.nonzero(bad)[0])} of the table points outside its buffers")
    for name, boxes in (("proposals", proposals), ("gt_boxes", gt_boxes)):
        # a decoded box narrower than a pixel has x2 < x1 by less than 1 and a positive width x2 - x1 + 1: the reference
        # scores it, and so does the kernel; a width or height that is not positive could make the union <= 0
        if boxes.numel() and bool(((boxes[:, 2] - boxes[:, 0] + 1 <= 0) | (boxes[:, 3] - boxes[:, 1] + 1 <= 0)).any()):
            raise ValueError(f"proposal_gt_overlaps: {name} holds a reversed box: x2 - x1 + 1 <= 0 or y2 - y1 + 1 <= 0")
    out = torch.full((a, n_limits, g), -1.0, dtype=torch.float32, device=gt_boxes.device)
    n = table.shape[0]
    if n == 0:
        return out
    # the uploads are held in names until the launch is enqueued: a temporary's block would go back to the caching
    # allocator at once and be handed to the next upload
    table_dev, limits_dev = table.to(gt_boxes.device), limits.to(gt_boxes.device)
    with _on(gt_boxes.device):
        rc = _L.ovis_proposal_gt_overlaps(proposals.data_ptr() if p else 0, gt_boxes.data_ptr() if g else 0,
                                          gt_areas.data_ptr() if g else 0, table_dev.data_ptr(), n,
                                          int(table[:, 3].max()), area_ranges.data_ptr(), a,
                                          limits_dev.data_ptr(), n_limits, int(limits.max()), g,
                                          out.data_ptr() if g else 0, _stream())
    _lib.check(rc, "proposal_gt_overlaps")
    return out
