"""Per-op micro-benchmarks on the shapes of SURVEY.md 8(d) / BASELINE.md 3: achieved GB/s (or
TFLOP/s) of each hand-written kernel against its algorithmic byte / flop count.

    python tools/bench_ops.py [--ops roi_fwd,roi_bwd,nms,focal] [--iters 20]
Opt-in ops outside the default list: topk, paste, mask_rle, polygons, transform, transform_window, color_jitter, copy_paste, render, view_merge, rle_targets, sgd, sgd_ema (``--ops paste,...,sgd_ema``).
Prints one JSON object per op.  Timing: HIP events on torch's current stream (the stream the
kernels are launched on), `iters` launches after 3 warm-ups.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if "--lib" in sys.argv:  # an experiment build (tools/experiments/*_variants.sh) instead of the regular library
    from cvpr22_cross_modal_pseudo_labeling_amd import _lib  # noqa: E402
    _lib.LIB_PATH = os.path.abspath(sys.argv[sys.argv.index("--lib") + 1])
from cvpr22_cross_modal_pseudo_labeling_amd import _C  # noqa: E402

HBM_PEAK_GBS = 8000.0


def timeit(fn, iters, warmup=3, warm_seconds=0.3):
    """Mean ms per call over `iters` launches after the GPU has been kept busy with the same op for `warm_seconds` (an idle part
    needs a few hundred ms of load to reach its sustained clock: 20 launches from idle read 4-20 % slow, box dependent)."""
    import time
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < warm_seconds:
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters  # ms


def bench_rois(r, n_img, g, kind="uniform"):
    b = torch.randint(0, n_img, (r, 1), generator=g).float()
    if kind == "uniform":  # x1~U[0,1066], y1~U[0,640], w,h~U[16,316], clipped
        x1 = torch.rand(r, 1, generator=g) * 1066
        y1 = torch.rand(r, 1, generator=g) * 640
        w = torch.rand(r, 1, generator=g) * 300 + 16
        h = torch.rand(r, 1, generator=g) * 300 + 16
    else:  # RPN-like: log-uniform areas 32^2..512^2, ratios {.5,1,2}
        area = torch.exp(torch.rand(r, 1, generator=g) * (2 * torch.log(torch.tensor(512.0 / 32))) + 2 * torch.log(torch.tensor(32.0)))
        ratio = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (r, 1), generator=g)]
        w, h = torch.sqrt(area / ratio), torch.sqrt(area * ratio)
        x1 = torch.rand(r, 1, generator=g) * (1333 - w).clamp(min=1)
        y1 = torch.rand(r, 1, generator=g) * (800 - h).clamp(min=1)
    return torch.cat([b, x1, y1, (x1 + w).clamp(max=1332), (y1 + h).clamp(max=799)], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ops", default="roi_fwd,roi_bwd,roi_bwd_strided,nms,focal,gemm,dcn,res5,split_gemm")
    ap.add_argument("--lib", default="", help="path of an experiment build of libovis_hip.so (handled before the import)")
    ap.add_argument("--roi-kinds", default="uniform,rpn_like", help="RoI distributions of the RoIAlign micro-benchmarks")
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    ops = args.ops.split(",")
    g = torch.Generator().manual_seed(1234)
    dev = "cuda"
    res = []
    if "roi_fwd" in ops or "roi_bwd" in ops or "roi_bwd_strided" in ops:
        n, c, h, w, r = 2, 1024, 50, 84, 1024
        x = torch.randn(n, c, h, w, generator=g).to(dev)
        for kind in args.roi_kinds.split(","):
            rois = bench_rois(r, n, g, kind).to(dev)
            alg = 4 * r * c * 196 + 4 * n * c * h * w + 20 * r
            if "roi_fwd" in ops:
                ms = timeit(lambda: _C.roi_align_forward_mfma(x, rois, 1 / 16, 14, 14, 0), args.iters)
                res.append({"op": "roi_align_forward_mfma", "rois": kind, "ms": ms, "alg_MB": alg / 1e6,
                            "GBps": alg / ms / 1e6, "frac_hbm": alg / ms / 1e6 / HBM_PEAK_GBS})
                ms = timeit(lambda: _C.roi_align_forward(x, rois, 1 / 16, 14, 14, 0), args.iters)
                res.append({"op": "roi_align_forward", "rois": kind, "ms": ms, "alg_MB": alg / 1e6,
                            "GBps": alg / ms / 1e6, "frac_hbm": alg / ms / 1e6 / HBM_PEAK_GBS})
            if "roi_fwd" in ops:
                x_cl = x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)  # channels-last map: pooled in place
                ms = timeit(lambda: _C.roi_align_forward_strided_nhwc(x_cl, rois, 1 / 16, 14, 14, 0, 2), args.iters)
                alg_s = 4 * r * c * 49 + 4 * n * c * h * w + 20 * r
                res.append({"op": "roi_align_forward_strided_nhwc(s=2, channels-last map)", "rois": kind, "ms": ms,
                            "alg_MB": alg_s / 1e6, "GBps": alg_s / ms / 1e6, "frac_hbm": alg_s / ms / 1e6 / HBM_PEAK_GBS})
                ms = timeit(lambda: _C.roi_align_forward_strided_pair(x_cl, rois, 1 / 16, 14, 14, 0, 2), args.iters)
                res.append({"op": "roi_align_forward_strided_pair(s=2, channels-last map)", "rois": kind, "ms": ms,
                            "alg_MB": alg_s / 1e6, "GBps": alg_s / ms / 1e6, "frac_hbm": alg_s / ms / 1e6 / HBM_PEAK_GBS})
                del x_cl
            if "roi_bwd" in ops:
                go = torch.randn(r, c, 14, 14, generator=g).to(dev)
                ms = timeit(lambda: _C.roi_align_backward(go, rois, 1 / 16, 14, 14, n, c, h, w, 0), args.iters)
                res.append({"op": "roi_align_backward", "rois": kind, "ms": ms, "alg_MB": alg / 1e6,
                            "GBps": alg / ms / 1e6, "frac_hbm": alg / ms / 1e6 / HBM_PEAK_GBS})
                del go
            if "roi_bwd_strided" in ops:
                # the teacher step's form: gradient of the 7 x 7 computed bins, NHWC as the res5 data-gradient GEMM leaves it
                gs = torch.randn(r, 7, 7, c, generator=g).to(dev)
                alg_s = 4 * r * c * 49 + 4 * n * c * h * w + 20 * r
                ms = timeit(lambda: _C.roi_align_backward_strided(gs.permute(0, 3, 1, 2).contiguous(), rois, 1 / 16, 14, 14, n, c, h, w, 0, 2), args.iters)
                res.append({"op": "roi_align_backward_strided(s=2) after permute+contiguous", "rois": kind, "ms": ms,
                            "alg_MB": alg_s / 1e6, "GBps": alg_s / ms / 1e6, "frac_hbm": alg_s / ms / 1e6 / HBM_PEAK_GBS})
                if hasattr(_C, "roi_align_backward_strided_nhwc"):
                    ms = timeit(lambda: _C.roi_align_backward_strided_nhwc(gs, rois, 1 / 16, 14, 14, n, c, h, w, 0, 2), args.iters)
                    res.append({"op": "roi_align_backward_strided_nhwc(s=2, pre-split tiles)", "rois": kind, "ms": ms,
                                "alg_MB": alg_s / 1e6, "GBps": alg_s / ms / 1e6, "frac_hbm": alg_s / ms / 1e6 / HBM_PEAK_GBS})
                del gs
        del x
    if "res5" in ops:  # byte kernels of the NHWC res5 head at the student pass's shapes (R = 1024 -> M = 50176 rows)
        m = 1024 * 49
        for cols in (512, 1024, 2048):
            xm = torch.randn(m, cols, generator=g).to(dev)
            ms = timeit(lambda: _C.split_bf16x3(xm, 0), args.iters)
            res.append({"op": "split_bf16x3", "shape": f"{m}x{cols}", "ms": ms, "alg_MB": 10 * xm.numel() / 1e6,
                        "GBps": 10 * xm.numel() / ms / 1e6, "frac_hbm": 10 * xm.numel() / ms / 1e6 / HBM_PEAK_GBS})
            ym = torch.randn(m, cols, generator=g).to(dev)
            bm = torch.randn(cols, generator=g).to(dev)
            ms = timeit(lambda: _C.bias_act_(ym, bm, xm, True), args.iters)
            res.append({"op": "bias_act(+shortcut)", "shape": f"{m}x{cols}", "ms": ms, "alg_MB": 12 * xm.numel() / 1e6,
                        "GBps": 12 * xm.numel() / ms / 1e6, "frac_hbm": 12 * xm.numel() / ms / 1e6 / HBM_PEAK_GBS})
            del xm, ym
        xi = torch.randn(1024, 7, 7, 512, generator=g).to(dev)
        ms = timeit(lambda: _C.im2col_split_bf16x3(xi, 3, 3), args.iters)
        res.append({"op": "im2col_split_bf16x3", "shape": "[1024,7,7,512] 3x3", "ms": ms, "alg_MB": 58 * xi.numel() / 1e6,
                    "GBps": 58 * xi.numel() / ms / 1e6, "frac_hbm": 58 * xi.numel() / ms / 1e6 / HBM_PEAK_GBS})
        del xi
    if "split_gemm" in ops:  # pair-layout split GEMMs of the res5 head at R = 1024 (M = 50176 rows): forward / dX, 3x3, dW
        m = 1024 * 49
        peak = 2500.0  # dense bf16 TFLOP/s; 3 bf16 products per fp32-accurate product
        for tag, k, n in (("conv1 b0", 1024, 512), ("shortcut", 1024, 2048), ("conv3", 512, 2048), ("conv1 b1", 2048, 512)):
            ap = _C.split_pair(torch.randn(m, k, generator=g).to(dev))
            bp = _C.split_pair(torch.randn(n, k, generator=g).to(dev))
            ms = timeit(lambda: _C.split_gemm_pair(ap, bp), args.iters)
            fl = 6.0 * m * n * k
            res.append({"op": "split_gemm_pair", "shape": f"{tag} [{m}x{k}]x[{n}x{k}]^T", "ms": ms, "TFLOPs_bf16": fl / ms / 1e9,
                        "TFLOPs_fp32_equiv": fl / 3 / ms / 1e9, "frac_mfma": fl / ms / 1e9 / peak})
            gp = _C.split_pair(torch.randn(m, n, generator=g).to(dev))
            ms = timeit(lambda: _C.split_gemm_pair_tn(gp, ap), args.iters)
            res.append({"op": "split_gemm_pair_tn", "shape": f"{tag} dW [{m}x{n}]^T[{m}x{k}]", "ms": ms,
                        "TFLOPs_bf16": fl / ms / 1e9, "TFLOPs_fp32_equiv": fl / 3 / ms / 1e9, "frac_mfma": fl / ms / 1e9 / peak})
            del ap, bp, gp
        xp = _C.split_pair(torch.randn(m, 512, generator=g).to(dev))
        wp = _C.split_pair(torch.randn(512, 9 * 512, generator=g).to(dev))
        gp = _C.split_pair(torch.randn(m, 512, generator=g).to(dev))
        fl = 6.0 * m * 512 * 9 * 512
        ms = timeit(lambda: _C.split_gemm_pair(xp, wp, conv=(7, 7, 3, 3, False)), args.iters)
        res.append({"op": "split_gemm_pair(3x3 implicit)", "shape": "[1024,7,7,512]->512", "ms": ms, "TFLOPs_bf16": fl / ms / 1e9,
                    "TFLOPs_fp32_equiv": fl / 3 / ms / 1e9, "frac_mfma": fl / ms / 1e9 / peak})
        ms = timeit(lambda: _C.split_gemm_pair_tn(gp, xp, (7, 7, 3, 3)), args.iters)
        res.append({"op": "split_gemm_pair_tn(3x3 dW)", "shape": "[1024,7,7,512]->512", "ms": ms, "TFLOPs_bf16": fl / ms / 1e9,
                    "TFLOPs_fp32_equiv": fl / 3 / ms / 1e9, "frac_mfma": fl / ms / 1e9 / peak})
        for cols in (512, 2048):
            xm = torch.randn(m, cols, generator=g).to(dev)
            ms = timeit(lambda: _C.split_pair(xm), args.iters)
            res.append({"op": "split_pair", "shape": f"{m}x{cols}", "ms": ms, "alg_MB": 8 * xm.numel() / 1e6,
                        "GBps": 8 * xm.numel() / ms / 1e6, "frac_hbm": 8 * xm.numel() / ms / 1e6 / HBM_PEAK_GBS})
            ym = torch.randn(m, cols, generator=g).to(dev)
            ms = timeit(lambda: _C.gate_split_pair(xm, ym, want_f32=True), args.iters)
            res.append({"op": "gate_split_pair(f32 gate, +f32 out)", "shape": f"{m}x{cols}", "ms": ms, "alg_MB": 16 * xm.numel() / 1e6,
                        "GBps": 16 * xm.numel() / ms / 1e6, "frac_hbm": 16 * xm.numel() / ms / 1e6 / HBM_PEAK_GBS})
            del xm, ym
        img = torch.randn(2, 3, 800, 1333, generator=g).to(dev)
        ms = timeit(lambda: _C.im2col_nchw_pair(img, 7, 7, 2, 3), args.iters)
        rows = 2 * 400 * 667
        res.append({"op": "im2col_nchw_pair(stem 7x7/2)", "shape": "[2,3,800,1333]", "ms": ms, "alg_MB": (img.numel() * 4 + rows * 640) / 1e6,
                    "GBps": (img.numel() * 4 + rows * 640) / ms / 1e6, "frac_hbm": (img.numel() * 4 + rows * 640) / ms / 1e6 / HBM_PEAK_GBS})
    if "nms" in ops:
        for k in (6000, 12000):
            xy = torch.rand(k, 2, generator=g) * torch.tensor([1200.0, 720.0])
            wh = torch.rand(k, 2, generator=g) * 200 + 8
            boxes = torch.cat([xy, xy + wh], 1).to(dev)
            scores = torch.rand(k, generator=g).to(dev)
            ms = timeit(lambda: _C.nms_padded(boxes, scores, 0.7), args.iters)
            nb = (k + 63) // 64
            alg = 20 * k + 2 * 8 * k * nb + 8 * k
            keep, num = _C.nms_padded(boxes, scores, 0.7)
            res.append({"op": "nms", "K": k, "kept": int(num), "ms": ms, "alg_MB": alg / 1e6, "GBps": alg / ms / 1e6,
                        "MIoU_per_s": k * (k - 1) / 2 / ms / 1e3})
    if "topk" in ops:  # the RPN's sorted top-k: 12000 of 50 * 84 * 15 = 63000 scores per image, two images
        sc = torch.rand(2, 63000, generator=g).to(dev)
        ms = timeit(lambda: _C.topk_sorted(sc, 12000), args.iters)
        ms_t = timeit(lambda: sc.topk(12000, dim=1, sorted=True), args.iters)
        res.append({"op": "topk_sorted", "shape": "[2,63000] k=12000", "ms": ms, "torch_topk_ms": ms_t})
    if "focal" in ops:
        m, c = 400000, 80
        logits = (torch.randn(m, c, generator=g) * 2).to(dev)
        targets = torch.where(torch.rand(m, generator=g) < 0.01, torch.randint(1, c + 1, (m,), generator=g),
                              torch.zeros(m, dtype=torch.int64)).int().to(dev)
        d = torch.rand(m, c, generator=g).to(dev)
        ms = timeit(lambda: _C.sigmoid_focalloss_forward(logits, targets, c, 2.0, 0.25), args.iters)
        alg = 8 * m * c + 4 * m
        res.append({"op": "sigmoid_focal_forward", "ms": ms, "alg_MB": alg / 1e6, "GBps": alg / ms / 1e6,
                    "frac_hbm": alg / ms / 1e6 / HBM_PEAK_GBS})
        ms = timeit(lambda: _C.sigmoid_focalloss_backward(logits, targets, d, c, 2.0, 0.25), args.iters)
        alg = 12 * m * c + 4 * m
        res.append({"op": "sigmoid_focal_backward", "ms": ms, "alg_MB": alg / 1e6, "GBps": alg / ms / 1e6,
                    "frac_hbm": alg / ms / 1e6 / HBM_PEAK_GBS})
    if "gemm" in ops:
        for (m, n, k, what) in ((1024, 776, 2048, "emb_pred+bbox_pred fwd"), (1024, 1203, 768, "text logits LVIS"),
                                (2000, 776, 2048, "teacher pass"), (1024, 49, 768, "text logits COCO")):
            a, b = torch.randn(m, k, generator=g).to(dev), torch.randn(n, k, generator=g).to(dev)
            ms = timeit(lambda: _C.gemm_nt(a, b), args.iters)
            res.append({"op": "gemm_f32_mfma", "shape": f"{m}x{n}x{k}", "what": what, "ms": ms,
                        "TFLOPs": 2.0 * m * n * k / ms / 1e9, "frac_fp32_mfma_peak": 2.0 * m * n * k / ms / 1e9 / 157.3})
            # the route the cross-modal head takes (layers/cross_modal.py::_LinearPair): operand split + pair-layout split
            # GEMM on the bf16 matrix cores; "gemm only" = operands already in pair layout (cached class matrix)
            from cvpr22_cross_modal_pseudo_labeling_amd.layers import linear_mfma
            with torch.no_grad():
                ms = timeit(lambda: linear_mfma(a, b), args.iters)
                n_pad = -(-n // 128) * 128
                ap = _C.split_pair(a)
                bp = _C.split_pair(torch.nn.functional.pad(b, (0, 0, 0, n_pad - n)))
                ms_g = timeit(lambda: _C.split_gemm_pair(ap, bp), args.iters)
            res.append({"op": "linear_pair(split GEMM)", "shape": f"{m}x{n}x{k}", "what": what, "ms": ms, "ms_gemm_only": ms_g,
                        "TFLOPs_fp32_equiv": 2.0 * m * n * k / ms / 1e9, "TFLOPs_fp32_equiv_gemm_only": 2.0 * m * n * k / ms_g / 1e9,
                        "TFLOPs_bf16_issued_gemm_only": 6.0 * m * n_pad * k / ms_g / 1e9})
    if "dcn" in ops:
        from cvpr22_cross_modal_pseudo_labeling_amd.layers import deform_conv
        x = torch.randn(2, 512, 100, 168, generator=g).to(dev)
        w = (torch.randn(512, 512, 3, 3, generator=g) * 0.02).to(dev)
        off = (torch.randn(2, 18, 100, 168, generator=g) * 2).to(dev)
        ms = timeit(lambda: deform_conv(x, off, w, 1, 1, 1, 1, 1, 2), max(3, args.iters // 4))
        fl = 2.0 * 512 * 512 * 9 * 2 * 100 * 168
        from cvpr22_cross_modal_pseudo_labeling_amd import _C as _ops
        _ops.dcn_implicit = False
        ms_col = timeit(lambda: deform_conv(x, off, w, 1, 1, 1, 1, 1, 2), max(3, args.iters // 4))
        _ops.dcn_implicit = True
        res.append({"op": "deform_conv_forward (column route: im2col + fp32 GEMM)", "shape": "[2,512,100,168] 3x3 -> 512",
                    "ms": ms_col, "TFLOPs": fl / ms_col / 1e9})
        res.append({"op": "deform_conv_forward", "shape": "[2,512,100,168] 3x3 -> 512", "ms": ms, "TFLOPs": fl / ms / 1e9,
                    "frac_fp32_mfma_peak": fl / ms / 1e9 / 157.3, "col_MB": 4 * 512 * 9 * 2 * 100 * 168 / 1e6})
    if "dcn" in ops:
        # backward (dX, dOffset, dW) of the same layer: rows route (split GEMMs, no reference-layout column buffer) vs the
        # column route (fp32-MFMA GEMMs around im2col / col2im / col2im_coord)
        from cvpr22_cross_modal_pseudo_labeling_amd import _C as _ops
        xg, og, wg = x.clone().requires_grad_(True), off.clone().requires_grad_(True), w.clone().requires_grad_(True)
        gy = torch.randn(2, 512, 100, 168, generator=g).to(dev)

        def fwd_bwd():
            for t in (xg, og, wg):
                t.grad = None
            deform_conv(xg, og, wg, 1, 1, 1, 1, 1, 2).backward(gy)

        ms_fb = timeit(fwd_bwd, max(3, args.iters // 4))
        _ops.dcn_implicit = False
        ms_fb_col = timeit(fwd_bwd, max(3, args.iters // 4))
        _ops.dcn_implicit = True
        res.append({"op": "deform_conv forward+backward (column route)", "shape": "[2,512,100,168] 3x3 -> 512", "ms": ms_fb_col,
                    "backward_ms": ms_fb_col - ms_col})
        res.append({"op": "deform_conv forward+backward (rows route)", "shape": "[2,512,100,168] 3x3 -> 512", "ms": ms_fb,
                    "backward_ms": ms_fb - ms, "backward_over_forward": (ms_fb - ms) / ms})
    if "paste" in ops or "mask_rle" in ops:  # the inputs both entries share: 100 detections of one 800 x 1333 image, M = 14
        p_, m_, h_, w_ = 100, 14, 800, 1333
        probs = torch.rand(p_, m_, m_, generator=g).to(dev)
        boxes = bench_rois(p_, 1, g, "rpn_like")[:, 1:].contiguous().to(dev)
    if "paste" in ops:  # opt-in: the evaluation pass's Masker paste
        from cvpr22_cross_modal_pseudo_labeling_amd.modeling.roi_heads import Masker
        from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList
        masks, boxlist, masker = probs[:, None], BoxList(boxes, (w_, h_)), Masker(0.5, 1)
        equal = torch.equal(_C.paste_masks(probs, boxes, (h_, w_)), masker._loop(masks, boxlist)[:, 0])
        k_ms, l_ms = [], []
        for _ in range(3):  # the two routes alternate inside this one call
            k_ms.append(timeit(lambda: _C.paste_masks(probs, boxes, (h_, w_)), args.iters))
            l_ms.append(timeit(lambda: masker._loop(masks, boxlist), max(3, args.iters // 4)))
        ms, ms_loop, nbytes = sorted(k_ms)[1], sorted(l_ms)[1], p_ * h_ * w_
        res.append({"op": "paste_masks (one launch)", "shape": "P=100 M=14 800x1333 rpn_like boxes", "ms": ms, "rounds_ms": [round(v, 4) for v in k_ms],
                    "bytes_MB": nbytes / 1e6, "GBps": nbytes / ms / 1e6, "frac_hbm_write_bound": nbytes / ms / 1e6 / HBM_PEAK_GBS,
                    "masker_loop_ms": ms_loop, "masker_loop_rounds_ms": [round(v, 4) for v in l_ms], "loop_over_kernel": ms_loop / ms,
                    "outputs_equal": equal})
    if "mask_rle" in ops:  # opt-in: the results export's mask encoder against what it replaces, strings on the host either way
        import time

        from tests import coco_rle_reference as rle
        sizes = torch.tensor([[h_, w_]] * p_, dtype=torch.int32).to(dev)

        def fused():  # three launches, two reads of P totals, then the strings and their offsets
            data, offsets = _C.pasted_masks_rle(probs, boxes, sizes)
            return data.cpu(), offsets.cpu()

        def paste_and_copy():  # the canvases, all of them across the link
            return _C.paste_masks(probs, boxes, (h_, w_)).cpu()

        def wall(fn, n):
            fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                out = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n * 1e3, out

        f_ms, c_ms = [], []
        for _ in range(3):  # the two routes alternate inside this one call
            ms, (data, offsets) = wall(fused, args.iters)
            f_ms.append(ms)
            ms, masks = wall(paste_and_copy, max(3, args.iters // 4))
            c_ms.append(ms)
        t0 = time.perf_counter()
        strings = [rle.rle_to_string(rle.rle_encode(m)) for m in masks.numpy()]
        encode_ms = (time.perf_counter() - t0) * 1e3
        o = offsets.tolist()
        equal = strings == [bytes(data[a:b].numpy()) for a, b in zip(o[:-1], o[1:])]
        ms, ms_copy = sorted(f_ms)[1], sorted(c_ms)[1]
        res.append({"op": "pasted_masks_rle (3 launches + copies of the strings)", "shape": "P=100 M=14 800x1333 rpn_like boxes",
                    "ms": ms, "rounds_ms": [round(v, 4) for v in f_ms], "to_host_bytes": data.numel() + 8 * (p_ + 1) + 2 * 4 * p_,
                    "string_bytes": data.numel(), "runs": int(_C.pasted_masks_runs(probs, boxes, sizes)[0].numel()),
                    "paste_masks_plus_copy_ms": ms_copy, "paste_masks_plus_copy_rounds_ms": [round(v, 4) for v in c_ms],
                    "numpy_encode_ms": encode_ms, "replaced_total_ms": ms_copy + encode_ms, "replaced_to_host_bytes": p_ * h_ * w_,
                    "replaced_over_fused": (ms_copy + encode_ms) / ms, "copy_alone_over_fused": ms_copy / ms, "outputs_equal": equal})
    if "polygons" in ops:  # opt-in: whole-image ground-truth masks, 20 instances of 30-200 vertices at 800 x 1333
        import math
        import time

        from cvpr22_cross_modal_pseudo_labeling_amd import _cpu
        from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import PolygonMasks
        g_, h_, w_ = 20, 800, 1333
        inst = []
        for k in torch.randint(30, 201, (g_,), generator=g).tolist():
            cx, cy = float(torch.rand(1, generator=g)) * w_, float(torch.rand(1, generator=g)) * h_
            rad = (torch.rand(k, generator=g) * 0.6 + 0.4) * (40 + 260 * float(torch.rand(1, generator=g)))
            inst.append([[v for i in range(k) for v in (cx + float(rad[i]) * math.cos(2 * math.pi * i / k),
                                                        cy + float(rad[i]) * math.sin(2 * math.pi * i / k))]])
        pm = PolygonMasks(inst, (w_, h_))
        pd = pm.to(dev)
        host = torch.empty((g_, h_, w_), dtype=torch.uint8)

        def on_host():
            _cpu.load().ovis_cpu_polygons_to_masks_u8(pm.coords.data_ptr(), pm.polygon_start.data_ptr(), pm.instance_start.data_ptr(),
                                                      g_, w_, h_, host.data_ptr(), 16)

        ms = timeit(lambda: _C.polygons_to_masks(pd.coords, pd.polygon_start, pd.instance_start, pd.size), args.iters)
        on_host()
        t0 = time.perf_counter()
        for _ in range(3):
            on_host()
        ms_host = (time.perf_counter() - t0) / 3 * 1e3
        equal = torch.equal(_C.polygons_to_masks(pd.coords, pd.polygon_start, pd.instance_start, pd.size).cpu(), host)
        res.append({"op": "polygons_to_masks (memset + 4 kernels)", "shape": "G=20 x 30-200 vertices, 800x1333", "ms": ms,
                    "out_MB": g_ * h_ * w_ / 1e6, "host_16_threads_ms": ms_host, "host_over_device": ms_host / ms,
                    "outputs_equal": equal})
    if "transform" in ops:  # opt-in: the input transform, 2 x (480 x 640 -> 800 x 1066), against its 16-thread host twin
        import time

        b_, ih, iw, oh, ow = 2, 480, 640, 800, 1066
        data = torch.randint(0, 256, (b_ * ih * iw * 3,), dtype=torch.uint8, generator=g)
        desc = torch.tensor([[i * ih * iw * 3, ih, iw, oh, ow, i % 2, 0] for i in range(b_)], dtype=torch.int32)
        mean, std = (102.9801, 115.9465, 122.7717), (1.0, 1.0, 1.0)
        dd, dc = data.to(dev), desc.to(dev)
        ms = timeit(lambda: _C.transform_images(dd, dc, mean, std, True, (oh, ow), (ih, iw)), args.iters)
        _C.transform_images(data, desc, mean, std, True, (oh, ow))
        t0 = time.perf_counter()
        for _ in range(3):
            host = _C.transform_images(data, desc, mean, std, True, (oh, ow))
        ms_host = (time.perf_counter() - t0) / 3 * 1e3
        equal = torch.equal(_C.transform_images(dd, dc, mean, std, True, (oh, ow), (ih, iw)).cpu(), host)
        nbytes = b_ * 3 * oh * ow * 4 + 2 * b_ * ih * ow * 3 + b_ * ih * iw * 3  # output + intermediate (written, read) + input
        res.append({"op": "transform_images (2 launches)", "shape": "2 x (480x640 -> 800x1066) uint8 -> f32", "ms": ms,
                    "bytes_MB": nbytes / 1e6, "GBps": nbytes / ms / 1e6, "frac_hbm_bound": nbytes / ms / 1e6 / HBM_PEAK_GBS,
                    "host_twin_ms": ms_host, "host_over_device": ms_host / ms, "outputs_equal": equal})
    if "transform_window" in ops:  # opt-in: scale jitter + crop on 2 x 480 x 640 with a 1024 x 1024 canvas, against the un-windowed route
        b_, ih, iw, canvas = 2, 480, 640, 1024
        data = torch.randint(0, 256, (b_ * ih * iw * 3,), dtype=torch.uint8, generator=g).to(dev)
        mean, std = (102.9801, 115.9465, 122.7717), (1.0, 1.0, 1.0)
        for scale, (oh, ow), (wy, wx, wh, ww) in ((2.0, (1536, 2048), (256, 512, 1024, 1024)), (0.5, (384, 512), (0, 0, 384, 512))):
            full = torch.tensor([[i * ih * iw * 3, ih, iw, oh, ow, i % 2, 0] for i in range(b_)], dtype=torch.int32)
            win = torch.cat([full, torch.tensor([[wy, wx, wh, ww]] * b_, dtype=torch.int32)], 1).to(dev)
            full = full.to(dev)
            pad = (max(oh, canvas), max(ow, canvas))  # the un-windowed route: the full resize, then the slice copy

            def sliced():
                return _C.transform_images(data, full, mean, std, True, pad, (ih, iw))[:, :, wy:wy + canvas, wx:wx + canvas].contiguous()

            ms_full = timeit(sliced, args.iters)
            ms = timeit(lambda: _C.transform_images_window(data, win, mean, std, True, (canvas, canvas), (ih, iw)), args.iters)
            equal = torch.equal(_C.transform_images_window(data, win, mean, std, True, (canvas, canvas), (ih, iw)), sliced())
            out_bytes = b_ * 3 * canvas * canvas * 4
            rows = min(ih, -(-wh * ih // oh) + 2)  # the input rows the window's rows read, about
            nbytes = out_bytes + 2 * b_ * rows * ww * 3 + b_ * rows * iw * 3  # output + intermediate (written, read) + input rows
            full_bytes = b_ * 3 * pad[0] * pad[1] * 4 + 2 * b_ * ih * ow * 3 + b_ * ih * iw * 3 + (2 * out_bytes if scale > 1 else 0)
            res.append({"op": "transform_images_window (2 launches)", "shape": f"2 x (480x640 -> {oh}x{ow}, scale {scale}) -> 1024x1024",
                        "ms": ms, "bytes_MB": nbytes / 1e6, "GBps": nbytes / ms / 1e6, "frac_hbm_bound": nbytes / ms / 1e6 / HBM_PEAK_GBS,
                        "transform_images_then_slice_ms": ms_full, "then_slice_bytes_MB": full_bytes / 1e6,
                        "then_slice_over_window": ms_full / ms, "outputs_equal": equal})
    if "color_jitter" in ops:  # opt-in: the colour jitter in front of the input transform, 2 x 480 x 640, three chains
        b_, ih, iw = 2, 480, 640
        data = torch.randint(0, 256, (b_ * ih * iw * 3,), dtype=torch.uint8, generator=g)
        desc = torch.tensor([[i * ih * iw * 3, ih, iw, ih, iw, 0, 0] for i in range(b_)], dtype=torch.int32)
        dd, dc = data.to(dev), desc.to(dev)
        for name, codes, factors in (("brightness only", [0, -1, -1, -1], [1.3, 0.0, 0.0, 0.0]),
                                     ("all four, contrast last", [0, 2, 3, 1], [1.3, 0.7, 37.0, 1.2]),
                                     ("hue only", [3, -1, -1, -1], [37.0, 0.0, 0.0, 0.0])):
            jo, jp = torch.tensor([codes] * b_, dtype=torch.int32), torch.tensor([factors] * b_, dtype=torch.float32)
            jod, jpd, contrast = jo.to(dev), jp.to(dev), 1 in codes
            ms = timeit(lambda: _C.color_jitter(dd, dc, jod, jpd, (ih, iw), contrast=contrast), args.iters)
            equal = torch.equal(_C.color_jitter(dd, dc, jod, jpd, (ih, iw), contrast=contrast).cpu(), _C.color_jitter(data, desc, jo, jp))
            nbytes = 2 * data.numel()  # the apply kernel's traffic: the raw bytes read and written once
            res.append({"op": f"color_jitter ({'memset + 2 launches' if contrast else '1 launch'}): {name}",
                        "shape": "2 x 480x640 uint8", "ms": ms, "bytes_MB": nbytes / 1e6, "GBps": nbytes / ms / 1e6,
                        "frac_hbm_bound": nbytes / ms / 1e6 / HBM_PEAK_GBS, "outputs_equal": equal})
    if "copy_paste" in ops:  # opt-in: copy-paste on 2 x 1024 x 1024, 8 own + 4 pasted instances per image, the rasterise included
        import math

        from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import PolygonMasks

        b_, canvas, n_own, n_paste = 2, 1024, 8, 4
        rs = torch.rand(b_, n_own + n_paste, 4, generator=g)
        polygons = []
        for i in range(b_):  # hexagons of 100..400 pixels across, spread over the canvas
            inst = []
            for cx, cy, r, _ in rs[i].tolist():
                cx, cy, r = 100 + cx * 824, 100 + cy * 824, 50 + r * 150
                inst.append([[v for k in range(6) for v in (cx + r * math.cos(k * math.pi / 3), cy + r * math.sin(k * math.pi / 3))]])
            polygons.append(PolygonMasks(inst, (canvas, canvas)).to(dev))
        batch = torch.randn(b_, 3, canvas, canvas, generator=g).to(dev)
        paste_src = [1, 0]

        def masks_only():
            out = []
            for p in polygons:
                m = p.convert_to_binarymask()
                out.append((m,) + _C.copy_paste_masks(m, n_own))
            return out

        def whole():
            made = masks_only()
            _C.copy_paste_images(batch, [a for _, a, _ in made], paste_src)
            return made

        ms_masks, ms = timeit(masks_only, args.iters), timeit(whole, args.iters)
        ms_raster = timeit(lambda: [p.convert_to_binarymask() for p in polygons], args.iters)
        made = whole()
        covered = sum(int(a.sum()) for _, a, _ in made)
        plane = canvas * canvas
        # the copy-paste kernels' own traffic: alpha (pasted read, alpha written), own masks (read, alpha read; stores only where
        # covered, not counted), pixels (alpha read; pasted values read and written)
        nbytes = b_ * (n_paste * plane + plane + n_own * 2 * plane + plane) + covered * 3 * 4 * 2
        res.append({"op": "copy_paste (per image: rasterise + 2 launches; + 1 launch for the batch)",
                    "shape": f"{b_} x {canvas}x{canvas}, {n_own} own + {n_paste} pasted, {covered} pasted pixels", "ms": ms,
                    "rasterise_ms": ms_raster, "masks_ms": ms_masks - ms_raster, "images_ms": ms - ms_masks,
                    "bytes_MB": nbytes / 1e6, "GBps_without_rasterise": nbytes / (ms - ms_raster) / 1e6,
                    "frac_hbm_without_rasterise": nbytes / (ms - ms_raster) / 1e6 / HBM_PEAK_GBS})
    if "render" in ops:  # opt-in: the prediction compositor, 100 fill layers on one 480 x 640 image, M = 14
        k_, m_, h_, w_ = 100, 14, 480, 640
        probs = torch.rand(k_, m_, m_, generator=g).to(dev)
        boxes = (bench_rois(k_, 1, g, "rpn_like")[:, 1:] * (w_ / 1333.0)).contiguous().to(dev)  # the 800 x 1333 boxes at this size
        colors = torch.randint(0, 256, (k_, 3), generator=g).float().to(dev)
        image = torch.randint(0, 256, (h_, w_, 3), dtype=torch.uint8, generator=g).to(dev)

        def over_paste_masks():  # what the library offered before: [K, H, W] masks, then K blending passes in torch
            masks = _C.paste_masks(probs, boxes, (h_, w_))
            img = image
            for i in range(k_):
                blended = (img.double() * (1.0 - 0.5) + 0.5 * colors[i].double()).to(torch.uint8)
                img = torch.where(masks[i][:, :, None], blended, img)
            return img

        equal = torch.equal(_C.render_instances(image, probs, boxes, colors), over_paste_masks())
        k_ms, t_ms = [], []
        for _ in range(3):  # the two routes alternate inside this one call
            k_ms.append(timeit(lambda: _C.render_instances(image, probs, boxes, colors), args.iters))
            t_ms.append(timeit(over_paste_masks, max(3, args.iters // 4)))
        ms, ms_torch = sorted(k_ms)[1], sorted(t_ms)[1]
        px = h_ * w_
        nbytes = 2 * 3 * px + 4 * k_ * (m_ * m_ + 4 + 3 + 2)       # image in, picture out, the layers' maps / boxes / colours / kind / param
        # counted, not measured: the masks written once (K px); per layer and pixel-channel img.double() (1 + 8), the product
        # (8 + 8), the sum (8 + 8), .to(uint8) (8 + 1), where() (1 + 1 + 1 out) = 53 bytes, plus the mask byte where() reads
        nbytes_torch = k_ * px + k_ * px * (3 * 53 + 1)
        res.append({"op": "render_instances (one launch)", "shape": "K=100 fill layers M=14 480x640 rpn_like boxes", "ms": ms,
                    "rounds_ms": [round(v, 4) for v in k_ms], "bytes_MB": nbytes / 1e6, "GBps": nbytes / ms / 1e6,
                    "paste_masks_plus_torch_ms": ms_torch, "paste_masks_plus_torch_rounds_ms": [round(v, 4) for v in t_ms],
                    "paste_masks_plus_torch_bytes_MB": nbytes_torch / 1e6, "mask_bytes_MB": k_ * px / 1e6,
                    "torch_over_kernel": ms_torch / ms, "outputs_equal": equal})
    if "view_merge" in ops:  # opt-in: TEST.BBOX_AUG merge + filter, 2 images x 6 views x 1000 proposals x 66 classes
        from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
        from cvpr22_cross_modal_pseudo_labeling_amd.modeling.roi_heads import PostProcessor
        from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList

        n_img, rows, nc = 2, 1000, 66
        views = [((1066, 800), 0), ((1066, 800), 1), ((533, 400), 0), ((533, 400), 1), ((1599, 1200), 0), ((1599, 1200), 1)]
        post = PostProcessor(get_defaults())
        lists, segments, row = [], [], 0
        for i in range(n_img):
            lists.append([])
            for (w, h), flip in views:
                xy = torch.rand(rows, nc, 2, generator=g) * torch.tensor([w * 0.7, h * 0.7])
                wh = torch.rand(rows, nc, 2, generator=g) * torch.tensor([w * 0.3, h * 0.3]) + 4
                bl = BoxList(torch.cat([xy, (xy + wh).clamp(max=min(w, h) - 1)], 2).reshape(-1, 4).to(dev), (w, h))
                # softmax scores as the box head makes them: a few per cent of the (row, class) pairs pass SCORE_THRESH 0.05
                bl.add_field("scores", torch.softmax(torch.randn(rows, nc, generator=g) * 2.0, 1).reshape(-1).to(dev))
                lists[i].append((bl, flip))
                segments.append((row, rows, i, w, flip, float(views[0][0][0]) / float(w), float(views[0][0][1]) / float(h)))
                row += rows
        all_boxes = torch.cat([bl.bbox for per in lists for bl, _ in per]).reshape(-1, nc, 4)
        all_scores = torch.cat([bl.get_field("scores") for per in lists for bl, _ in per]).reshape(-1, nc)
        sizes = [views[0][0]] * n_img

        from cvpr22_cross_modal_pseudo_labeling_amd.engine.bbox_aug import NMS_SLICE_CANDIDATES

        def kernel_route(limit=NMS_SLICE_CANDIDATES):  # as engine/bbox_aug.py::im_detect_bbox_aug runs the stage
            merged = _C.merge_view_detections(all_boxes, all_scores, segments, nc, post.score_thresh)
            return post.filter_merged(merged, sizes, nc, slice_candidates=limit), merged[0].shape[0]

        def boxlist_route():  # engine/bbox_aug.py:53-69 of the reference with the tensors on the device
            out = []
            for per in lists:
                mapped = []
                for bl, flip in per:
                    if flip:
                        bl = bl.transpose(0)
                    mapped.append(bl if not mapped else bl.resize(mapped[0].size))
                cat = BoxList(torch.cat([m.bbox for m in mapped]), mapped[0].size)
                cat.add_field("scores", torch.cat([m.get_field("scores") for m in mapped]))
                out.append(post.filter_results(cat, nc))
            return out

        def candidates_by_tensor_ops():  # the part of boxlist_route the merge kernels replace: map, cat, threshold, gather
            out = []
            for per in lists:
                mapped = []
                for bl, flip in per:
                    if flip:
                        bl = bl.transpose(0)
                    mapped.append(bl if not mapped else bl.resize(mapped[0].size))
                boxes = torch.cat([m.bbox for m in mapped]).reshape(-1, nc, 4)
                scores = torch.cat([m.get_field("scores") for m in mapped]).reshape(-1, nc)
                cls, row = (scores.t()[1:] > post.score_thresh).nonzero(as_tuple=True)  # PostProcessor.filter_results
                out.append((boxes[row, cls + 1], scores[row, cls + 1], cls + 1))
            return out

        def kernels(fn):  # device kernels of one call, from the profiler; None where it is unavailable
            try:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    fn()
                    torch.cuda.synchronize()
                return sum(str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()
                           for e in prof.events())
            except Exception:  # noqa: BLE001 -- a number for the report, not part of the result
                return None

        got, k_ = kernel_route()
        want = boxlist_route()
        equal = all(torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores"))
                    and torch.equal(a.get_field("labels"), b.get_field("labels")) for a, b in zip(got, want))
        k_ms, t_ms = [], []
        for _ in range(3):  # the two routes alternate inside this one call
            k_ms.append(timeit(kernel_route, args.iters))
            t_ms.append(timeit(boxlist_route, args.iters))
        # the parts: the merge alone, and the filter at other slice limits (the grouped NMS visits all K^2 / 2 pairs of a call)
        def merge_only():
            return _C.merge_view_detections(all_boxes, all_scores, segments, nc, post.score_thresh)

        merge_ms, tensor_ms = timeit(merge_only, args.iters), timeit(candidates_by_tensor_ops, args.iters)
        by_limit = {str(lim): round(timeit(lambda: kernel_route(lim), args.iters), 4)
                    for lim in (_C.NMS_MAX_CANDIDATES, 32768, 16384, 8192, 4096, 2048)}
        res.append({"op": "merge_view_detections + filter_merged", "shape": f"{n_img} images x {len(views)} views x {rows} rows x {nc} classes",
                    "ms": sorted(k_ms)[1], "rounds_ms": [round(v, 4) for v in k_ms], "candidates": k_,
                    "nms_slice_candidates": NMS_SLICE_CANDIDATES, "merge_only_ms": merge_ms, "merge_only_kernels": kernels(merge_only),
                    "candidates_by_tensor_ops_ms": tensor_ms, "candidates_by_tensor_ops_kernels": kernels(candidates_by_tensor_ops),
                    "ms_by_slice_limit": by_limit,
                    "fraction_above_threshold": k_ / (all_scores.numel() * (nc - 1) / nc),
                    "boxlist_route_ms": sorted(t_ms)[1], "boxlist_route_rounds_ms": [round(v, 4) for v in t_ms],
                    "boxlist_over_kernel": sorted(t_ms)[1] / sorted(k_ms)[1],
                    "kernels": kernels(kernel_route), "boxlist_route_kernels": kernels(boxlist_route),
                    "outputs_equal": equal})
    if "rle_targets" in ops:  # opt-in: mask targets from RLE ground truth, 480 x 640 -> 800 x 1067, against the dense route
        import numpy as np
        import torch.nn.functional as F

        from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import RleMasks

        def to_string(counts):  # pycocotools' rleToString
            out = bytearray()
            for i, x in enumerate(counts):
                x = int(x) - (int(counts[i - 2]) if i > 2 else 0)
                more = True
                while more:
                    c = x & 0x1f
                    x >>= 5
                    more = (x != -1) if (c & 0x10) else (x != 0)
                    out.append((c | 0x20 if more else c) + 48)
            return bytes(out)

        n_img, n_gt, n_pos, m_res, (h0, w0), (h1, w1) = 2, 8, 64, 14, (480, 640), (800, 1067)
        rs = np.random.default_rng(7)
        yy, xx = np.mgrid[:h0, :w0]
        host, all_boxes, all_index = [], [], []
        for _ in range(n_img):
            items, gt = [], []
            for _ in range(n_gt):  # an ellipse with a hole: a few hundred runs, like an instance mask
                cx, cy, a, b = rs.uniform(80, w0 - 80), rs.uniform(80, h0 - 80), rs.uniform(30, 150), rs.uniform(30, 150)
                d = ((xx - cx) / a) ** 2 + ((yy - cy) / b) ** 2
                v = ((d < 1) & (d > 0.05)).T.reshape(-1).astype(np.int8)   # column-major
                ends = np.flatnonzero(np.diff(np.concatenate([[0], v])))
                items.append(to_string(np.diff(np.concatenate([[0], ends, [v.size]])).tolist()))
                gt.append([cx - a, cy - b, cx + a, cy + b])
            host.append(RleMasks(items, (h0, w0)).resize((w1, h1)).transpose(0))
            idx = rs.integers(0, n_gt, n_pos)
            scale = np.array([w1 / w0, h1 / h0] * 2)
            bx = (np.array(gt)[idx] + rs.uniform(-12, 12, (n_pos, 4))) * scale
            bx[:, 0::2] = w1 - 1 - bx[:, [2, 0]]   # the boxes follow the flip
            all_boxes.append(torch.from_numpy(np.clip(bx, 0, [w1 - 1, h1 - 1] * 2).astype(np.float32)).to(dev))
            all_index.append(torch.from_numpy(idx).to(dev))
        shifts = torch.arange(64, device=dev)

        staged = [m.to(dev) for m in host]

        def undecoded():
            for m in staged:
                m.words = m.word_offsets = None
            return staged

        def kernel_route():
            masks = undecoded()
            RleMasks.decode_many(masks)
            return [_C.project_rle_masks(m, i, b, m_res) for m, i, b in zip(masks, all_index, all_boxes)]

        def dense_route():  # the same decode, then a uint8 canvas per instance: unpack, resize, truncate, flip, project_masks
            masks = undecoded()
            RleMasks.decode_many(masks)
            out = []
            for m, i, b in zip(masks, all_index, all_boxes):
                bits = ((m.words.view(len(masks), n_gt, -1)[masks.index(m)][:, :, None] >> shifts) & 1).reshape(n_gt, -1)
                canvas = bits[:, :h0 * w0].reshape(n_gt, 1, h0, w0).float()
                canvas = F.interpolate(canvas, size=(h1, w1), mode="bilinear", align_corners=False)[:, 0].to(torch.uint8).flip(2)
                out.append(_C.project_masks(canvas, i, b, m_res))
            return out

        def decode_only():
            RleMasks.decode_many(undecoded())

        got, want = kernel_route(), dense_route()
        differ = sum(int((a != b).sum()) for a, b in zip(got, want))
        k_ms, d_ms = [], []
        for _ in range(3):  # the two routes alternate inside this one call
            k_ms.append(timeit(kernel_route, args.iters))
            d_ms.append(timeit(dense_route, args.iters))
        res.append({"op": "decode_many + project_rle_masks", "shape": f"{n_img} images x {n_gt} masks {h0}x{w0} -> {h1}x{w1}, flipped, "
                    f"{n_pos} positives each, M = {m_res}", "ms": sorted(k_ms)[1], "rounds_ms": [round(v, 4) for v in k_ms],
                    "decode_only_ms": timeit(decode_only, args.iters), "dense_route_ms": sorted(d_ms)[1],
                    "dense_route_rounds_ms": [round(v, 4) for v in d_ms], "dense_over_kernel": sorted(d_ms)[1] / sorted(k_ms)[1],
                    "dense_canvas_MB": n_img * n_gt * h1 * w1 * 5 / 1e6, "target_pixels": n_img * n_pos * m_res * m_res,
                    "target_pixels_that_differ_from_the_dense_route": differ})
    if "sgd" in ops or "sgd_ema" in ops:  # opt-in: the optimizer launches on the teacher configuration's parameter set
        from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
        from cvpr22_cross_modal_pseudo_labeling_amd.engine import solver
        from cvpr22_cross_modal_pseudo_labeling_amd.modeling.detector import build_detection_model

        cfg = get_defaults()
        cfg.merge_from_file(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                         "configs/coco_cap_det/zeroshot_mask.yaml"))
        cfg.freeze()
        model = build_detection_model(cfg).to(dev)
        trainable = [p for p in model.parameters() if p.requires_grad]
        elements = sum(p.numel() for p in trainable)
        flat = torch.randn(elements + 3, generator=g).to(dev) * 1e-3   # gradient views at odd element offsets, as the reducer's
        off = 3
        for p in trainable:
            p.grad = flat[off:off + p.numel()].view_as(p)
            off += p.numel()
        shape = f"{len(trainable)} tensors, {elements} elements"

        def launches_of(opt):
            """The cached launches of a steady-state step as one callable (the host's list walk left out)."""
            opt.step()
            opt.step()
            fast = opt._native_tables["fast"]
            groups = opt.param_groups
            calls = [(items, blocks, float(groups[members[0]]["lr"]), float(groups[members[0]]["weight_decay"]),
                      float(groups[members[0]]["momentum"])) for members, items, blocks, _ in fast[2]]
            return calls

        def row(op, fn, bytes_per_element, extra=None):
            rounds = [timeit(fn, args.iters) for _ in range(3)]
            ms = sorted(rounds)[1]
            alg = bytes_per_element * elements
            res.append(dict({"op": op, "shape": shape, "ms": ms, "rounds_ms": [round(v, 4) for v in rounds],
                             "bytes_per_element": bytes_per_element, "alg_MB": alg / 1e6, "GBps": alg / ms / 1e6,
                             "frac_hbm": alg / ms / 1e6 / HBM_PEAK_GBS}, **(extra or {})))

        opt = solver.make_optimizer(cfg, model)
        plain = launches_of(opt)

        def sgd():
            for items, blocks, lr, wd, mom in plain:
                _C.sgd_momentum_multi(items, blocks, lr, wd, mom, True)

        if "sgd" in ops:
            row("sgd_momentum_multi", sgd, 20, {"launches": len(plain)})
            row("GroupFusedSGD.step (cached route, host walk included)", opt.step, 20, {"launches": len(plain)})
        if "sgd_ema" in ops:
            from cvpr22_cross_modal_pseudo_labeling_amd.engine.ema import ModelEma

            ema = ModelEma(model, 0.999)
            emas = [ema.tensor_of(p) for p in trainable]
            w = ema.weight()

            def sgd_then_foreach():  # the existing launch, then the average as three multi-tensor passes
                sgd()
                diff = torch._foreach_sub(trainable, emas)
                torch._foreach_mul_(diff, w)
                torch._foreach_add_(emas, diff)

            with torch.no_grad():
                row("sgd_momentum_multi + 3 foreach passes (EMA)", sgd_then_foreach, 20 + 32, {"launches": len(plain)})
            opt_ema = solver.make_optimizer(cfg, model)
            opt_ema.ema = ema
            fused = launches_of(opt_ema)

            def sgd_ema():
                for items, blocks, lr, wd, mom in fused:
                    _C.sgd_momentum_ema_multi(items, blocks, lr, wd, mom, True, w)

            row("sgd_momentum_ema_multi", sgd_ema, 28, {"launches": len(fused)})
            row("GroupFusedSGD.step with ema (cached route, host walk included)", opt_ema.step, 28, {"launches": len(fused)})
            swap_ms = timeit(lambda: ema.swap(model), args.iters)   # (an even count of exchanges: the model is as it was)
            res.append({"op": "swap_multi (ModelEma.swap)", "shape": shape, "ms": swap_ms, "bytes_per_element": 16,
                        "alg_MB": 16 * elements / 1e6, "GBps": 16 * elements / swap_ms / 1e6,
                        "frac_hbm": 16 * elements / swap_ms / 1e6 / HBM_PEAK_GBS})
    for r_ in res:
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in r_.items()}))


if __name__ == "__main__":
    main()
