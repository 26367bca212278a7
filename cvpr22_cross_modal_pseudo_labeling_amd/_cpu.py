"""HOST-tensor side of ``_C``: the reference's CPU-only configuration (``MODEL.DEVICE cpu``, BASELINE.json configs[0]).

The reference's native module dispatches on the tensor's device (csrc/ROIAlign.h:11-25, csrc/nms.h:10-28): host tensors go to
``csrc/cpu/ROIAlign_cpu.cpp`` / ``csrc/cpu/nms_cpu.cpp``, and the heads / losses are plain torch ops on whatever device the
tensors live on.  This module is that side: RoIAlign forward, its transpose and NMS in ``libovis_cpu.so`` (C++,
``csrc/cpu/ovis_cpu.cpp``, C ABI ``include/ovis_cpu.h``), the head / loss entry points as the torch-op formulas of the
reference's modules.  It is reached ONLY with host tensors (``_C.py`` branches on ``is_cuda``); device tensors are never
routed here and host tensors never to the device, and a missing library raises."""
import ctypes
import os

import torch
import torch.nn.functional as F

from ._lib import bind, read_header

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libovis_cpu.so")

SIGNATURES, CONSTANTS = read_header("ovis_cpu.h")   # name -> (restype, argtypes); OVIS_CPU_OK / _EINVAL / _ERANGE
_lib = None


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} is missing: build it first (make -C cvpr22_cross_modal_pseudo_labeling_amd/csrc); "
                              "host tensors have no other implementation")
        _lib = bind(LIB_PATH, SIGNATURES)
    return _lib


def _host(t, name, dtype=torch.float32):
    if t.is_cuda:
        raise RuntimeError(f"{name}: host and device tensors mixed in one call")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must be {dtype}, got {t.dtype}")
    return t.contiguous()


def _check(rc, what, einval="bad argument (a RoI's batch index outside the batch, or a null / negative size)"):
    if rc == CONSTANTS["OVIS_CPU_ERANGE"]:
        raise RuntimeError(f"{what}: OVIS_ERANGE (problem size not supported by the kernel)")
    if rc < 0:
        raise RuntimeError(f"{what}: {einval}")


# ---- csrc/cpu/ROIAlign_cpu.cpp:114-219; the transpose has no host form in the reference (csrc/ROIAlign.h:44) ----------------
def roi_align_forward(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio):
    input, rois = _host(input, "input"), _host(rois, "rois")
    if rois.dim() != 2 or rois.size(1) != 5 or input.dim() != 4:
        raise RuntimeError("roi_align_forward: expected input [N,C,H,W] and rois [R,5]")
    n, c, h, w = input.shape
    r = rois.size(0)
    out = torch.empty((r, c, pooled_height, pooled_width), dtype=torch.float32)
    if out.numel():
        _check(load().ovis_cpu_roi_align_forward_f32(input.data_ptr(), rois.data_ptr(), out.data_ptr(), r, n, c, h, w,
                                                      pooled_height, pooled_width, spatial_scale, sampling_ratio, 0),
               "roi_align_forward")
    return out


def roi_align_backward(grad, rois, spatial_scale, pooled_height, pooled_width, batch_size, channels, height, width,
                       sampling_ratio):
    grad, rois = _host(grad, "grad"), _host(rois, "rois")
    gin = torch.empty((batch_size, channels, height, width), dtype=torch.float32)
    if gin.numel():
        _check(load().ovis_cpu_roi_align_backward_f32(grad.data_ptr(), rois.data_ptr(), gin.data_ptr(), rois.size(0), batch_size,
                                                       channels, height, width, pooled_height, pooled_width, spatial_scale,
                                                       sampling_ratio, 0), "roi_align_backward")
    return gin


# ---- csrc/cpu/nms_cpu.cpp:6-65 (a box goes when IoU >= threshold -- the host kernel's comparison, whatever ge_mode says) ------
def nms_padded(dets, scores, threshold, ge_mode=True):
    dets, scores = _host(dets, "dets"), _host(scores, "scores")
    k = dets.size(0)
    keep = torch.zeros((k,), dtype=torch.int64)
    if k == 0:
        return keep, torch.zeros((1,), dtype=torch.int32)
    if dets.dim() != 2 or dets.size(1) != 4 or scores.numel() != k:
        raise RuntimeError("nms: expected dets [K,4] and scores [K]")
    n = load().ovis_cpu_nms_f32(dets.data_ptr(), scores.data_ptr(), k, threshold, keep.data_ptr())
    _check(n, "nms")
    return keep, torch.tensor([n], dtype=torch.int32)


def nms(dets, scores, threshold):
    keep, num = nms_padded(dets, scores, threshold)
    return keep[: int(num)]


# ---- heads / losses: the reference's own torch-op formulas ------------------------------------------------------------
def gemm_nt(a, b, bias=None):
    """a [M, K] @ b [N, K]^T (+ bias): nn.Linear of roi_box_predictors.py:62-81 / roi_mask_predictors.py:41-65."""
    y = a @ b.t()
    return y if bias is None else y + bias


def region_noun_align(region_emb, noun_emb):
    """st_generalized_rcnn.py:236-246: per noun the best region -> (raw maximum, its sigmoid, argmax)."""
    raw, idx = torch.max(region_emb @ noun_emb.t(), dim=0)
    return raw, torch.sigmoid(raw), idx


def weighted_ce_fwd_bwd(logits, labels, bg_weight, need_grad=True):
    """box_head/loss.py:160-176: cross entropy with the background class weighted, summed over the rows and divided by
    their number -> (loss, d loss / d logits)."""
    p = labels.numel()
    logp = F.log_softmax(logits, dim=1)
    w = torch.ones(logits.shape[1], dtype=logits.dtype)
    w[0] = bg_weight
    wy = w[labels]
    loss = -(wy * logp.gather(1, labels.view(-1, 1)).squeeze(1)).sum() / max(p, 1)
    if not need_grad:
        return loss, None
    g = logp.exp()
    g.scatter_add_(1, labels.view(-1, 1), torch.full((p, 1), -1.0, dtype=logits.dtype))
    return loss, g * (wy / max(p, 1)).view(-1, 1)


def mask_bce_stochastic_fwd_bwd(mu, sigma, eps, pos_index, targets, channel, need_grad=True):
    """mask_head/loss.py:107-148 with the stochastic logits of roi_mask_predictors.py:52-63 (z = mu + eps * sigma):
    mean binary cross entropy of the positives' selected channel -> (loss, d mu, d sigma).  z = mu when either factor is
    missing, like the device path: sigma without eps gets an all-zero d sigma."""
    z = mu if (sigma is None or eps is None) else mu + eps * sigma
    sel = z[pos_index, channel]                                   # [Pp, M, M]
    npos = pos_index.numel()
    t = targets.reshape(sel.shape)
    loss = F.binary_cross_entropy_with_logits(sel, t, reduction="mean") if npos else sel.sum() * 0
    if not need_grad:
        return loss, None, None
    dsel = (torch.sigmoid(sel) - t) / max(sel.numel(), 1)
    dmu = torch.zeros_like(mu)
    dmu.index_put_((pos_index, channel if torch.is_tensor(channel) else torch.full_like(pos_index, channel)), dsel, accumulate=True)
    dsigma = None
    if sigma is not None:
        dsigma = torch.zeros_like(sigma)
    if sigma is not None and eps is not None:
        dsigma.index_put_((pos_index, torch.zeros_like(pos_index)), dsel * eps[pos_index, channel], accumulate=True)
    return loss, dmu, dsigma


# ---- mask_head/loss.py:11-42 for polygon targets (segmentation_mask.py:270-334 + pycocotools' rasteriser) ----------------------
def project_polygon_masks(coords, polygon_start, instance_start, gt_index, boxes, image_size, resolution):
    boxes = _host(boxes, "boxes")
    coords = _host(coords, "coords") if coords.numel() else coords
    polygon_start, instance_start = _host(polygon_start, "polygon_start", torch.int32), _host(instance_start, "instance_start", torch.int32)
    gt_index = _host(gt_index, "gt_index", torch.int64)
    p = boxes.shape[0]
    out = torch.empty((p, resolution, resolution), dtype=torch.float32)
    if p:
        _check(load().ovis_cpu_project_polygon_masks_f32(coords.data_ptr() if coords.numel() else 0, polygon_start.data_ptr(),
                                                        instance_start.data_ptr(), gt_index.data_ptr(), boxes.data_ptr(), p,
                                                        int(image_size[0]), int(image_size[1]), int(resolution), out.data_ptr(), 0),
               "project_polygon_masks")
    return out


def polygons_to_masks(coords, polygon_start, instance_start, image_size):
    """uint8 [G, height, width] whole-image masks of the G polygon instances (segmentation_mask.py:326-334)."""
    coords = _host(coords, "coords") if coords.numel() else coords
    polygon_start, instance_start = _host(polygon_start, "polygon_start", torch.int32), _host(instance_start, "instance_start", torch.int32)
    g = instance_start.numel() - 1
    w, h = int(image_size[0]), int(image_size[1])
    out = torch.empty((g, h, w), dtype=torch.uint8)
    if g:
        _check(load().ovis_cpu_polygons_to_masks_u8(coords.data_ptr() if coords.numel() else 0, polygon_start.data_ptr(),
                                                   instance_start.data_ptr(), g, w, h, out.data_ptr(), 0), "polygons_to_masks")
    return out


# ---- data/transforms/transforms.py:27-62,65-85,105-120 + structures/image_list.py:29-70 on packed uint8 images ---------------------
def transform_images(data, desc, mean, std, to_bgr255, pad_hw):
    """float32 [B, 3, pad_h, pad_w] from B packed RGB HWC uint8 images (``ovis_cpu_transform_images_u8``)."""
    data, desc = _host(data, "data", torch.uint8), _host(desc, "desc", torch.int32)
    if data.dim() != 1 or desc.dim() != 2 or desc.shape[1] != 7:
        raise RuntimeError("transform_images: expected data [bytes] uint8 and desc [B,7] int32")
    b, (pad_h, pad_w) = desc.shape[0], (int(pad_hw[0]), int(pad_hw[1]))
    out = torch.empty((b, 3, pad_h, pad_w), dtype=torch.float32)
    if b:
        m3, s3 = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
        _check(load().ovis_cpu_transform_images_u8(data.data_ptr(), data.numel(), desc.data_ptr(), b, m3, s3, int(bool(to_bgr255)),
                                                   pad_h, pad_w, out.data_ptr(), 0), "transform_images")
    return out


def transform_images_window(data, desc, mean, std, to_bgr255, pad_hw):
    """float32 [B, 3, pad_h, pad_w]: the crop window of every resized, flipped image (``ovis_cpu_transform_images_window_u8``;
    desc [B, 11] as ``_C.transform_images_window`` takes it)."""
    data, desc = _host(data, "data", torch.uint8), _host(desc, "desc", torch.int32)
    if data.dim() != 1 or desc.dim() != 2 or desc.shape[1] != 11:
        raise RuntimeError("transform_images_window: expected data [bytes] uint8 and desc [B,11] int32")
    b, (pad_h, pad_w) = desc.shape[0], (int(pad_hw[0]), int(pad_hw[1]))
    out = torch.empty((b, 3, pad_h, pad_w), dtype=torch.float32)
    if b:
        m3, s3 = (ctypes.c_float * 3)(*[float(v) for v in mean]), (ctypes.c_float * 3)(*[float(v) for v in std])
        _check(load().ovis_cpu_transform_images_window_u8(data.data_ptr(), data.numel(), desc.data_ptr(), b, m3, s3,
                                                          int(bool(to_bgr255)), pad_h, pad_w, out.data_ptr(), 0),
               "transform_images_window", "OVIS_EINVAL (a descriptor that leaves the byte buffer, or a window that leaves the "
               "resized image or the canvas)")
    return out


# ---- data/transforms/transforms.py:88-102 (ColorJitter) on packed uint8 images ------------------------------------------------
def color_jitter(data, desc, ops, params):
    """uint8 [bytes]: the packed images jittered (``ovis_cpu_color_jitter_u8``), the layout of ``data``."""
    data, desc = _host(data, "data", torch.uint8), _host(desc, "desc", torch.int32)
    ops, params = _host(ops, "ops", torch.int32), _host(params, "params")
    b = desc.shape[0] if desc.dim() == 2 else -1
    if data.dim() != 1 or desc.dim() != 2 or desc.shape[1] != 7 or tuple(ops.shape) != (b, 4) or tuple(params.shape) != (b, 4):
        raise RuntimeError("color_jitter: expected data [bytes] uint8, desc [B,7] int32, ops [B,4] int32 and params [B,4] float32")
    out = torch.empty_like(data)
    if b:
        _check(load().ovis_cpu_color_jitter_u8(data.data_ptr(), data.numel(), desc.data_ptr(), ops.data_ptr(), params.data_ptr(),
                                               b, out.data_ptr(), 0), "color_jitter",
               "OVIS_EINVAL (a descriptor that leaves the byte buffer)")
    return out


# ---- engine/inference.py:519-589 (overlay_boxes, overlay_filled_mask, overlay_uncertainty_mask) over the Masker paste ----------
def render_instances(image, maps, boxes, colors, kinds, params, alpha, outline_colors, outline_thickness):
    """uint8 [H, W, 3] (``ovis_cpu_render_instances_u8``); the operands as ``_C.render_instances`` prepared them."""
    out = torch.empty_like(image)
    k = maps.shape[0]
    _check(load().ovis_cpu_render_instances_u8(
        image.data_ptr(), image.shape[0], image.shape[1], maps.data_ptr() if k else 0, boxes.data_ptr() if k else 0, k,
        maps.shape[1] if k else 0, kinds.data_ptr() if k else 0, params.data_ptr() if k else 0, colors.data_ptr() if k else 0,
        float(alpha), outline_colors.data_ptr() if (k and outline_colors is not None) else 0, int(outline_thickness),
        out.data_ptr(), 0), "render_instances",
        "OVIS_EINVAL (a null or negative size, alpha outside [0, 1], an outline thickness below 1, or out overlapping image)")
    return out


# ---- st_generalized_rcnn.py:202-209 (extract_emb) on host tensors: the reference's own tensor-op formula -----------------------
def text_embed(table, input_ids, special_tokens_mask):
    keep = (1 - special_tokens_mask).to(torch.float32)
    emb = (table[input_ids] * keep[:, :, None]).sum(1) / keep.sum(1)[:, None]
    return F.normalize(emb, dim=-1)


# ---- engine/bbox_aug.py:53-60 + box_head/inference.py:137-143: the merge of test-time-augmentation views ------------------
def merge_view_detections(boxes, scores, segments, num_classes, num_images, score_thresh):
    """Host tensors: the reference's route as it writes it -- per view ``BoxList.transpose(0)`` when flipped, the two
    multiplications of ``BoxList.resize`` (the records carry the ratios ``resize`` computes from the two sizes, so the
    products are formed here with its expressions), ``torch.cat`` over an image's views, then per class
    ``nonzero(scores > thresh)``.  -> (cand_boxes, cand_scores, cand_group, offsets) as ``_C.merge_view_detections``."""
    from .modeling.structures import BoxList

    boxes, scores = _host(boxes, "boxes"), _host(scores, "scores")
    c = num_classes
    out_boxes, out_scores, out_group, offsets = [], [], [], [0]
    for image in range(num_images):
        view_boxes, view_scores = [], []
        for row_start, row_count, img, width, flip, ratio_w, ratio_h in segments:
            if img != image:
                continue
            view = BoxList(boxes[row_start:row_start + row_count].reshape(-1, 4), (width, 1))
            if flip:
                view = view.transpose(0)
            ratio_w, ratio_h = (float(torch.tensor(v, dtype=torch.float32)) for v in (ratio_w, ratio_h))
            if ratio_w == ratio_h:  # BoxList.resize
                scaled = view.bbox * ratio_w
            else:
                xmin, ymin, xmax, ymax = view.bbox.split(1, dim=-1)
                scaled = torch.cat((xmin * ratio_w, ymin * ratio_h, xmax * ratio_w, ymax * ratio_h), dim=-1)
            view_boxes.append(scaled.reshape(-1, c, 4))
            view_scores.append(scores[row_start:row_start + row_count])
        all_boxes, all_scores = torch.cat(view_boxes, 0), torch.cat(view_scores, 0)
        inds_all = all_scores > score_thresh
        offsets.append(offsets[-1])  # class 0, the background, is an empty run
        for j in range(1, c):
            inds = inds_all[:, j].nonzero().squeeze(1)
            out_boxes.append(all_boxes[inds, j])
            out_scores.append(all_scores[inds, j])
            out_group.append(torch.full((inds.numel(),), image * c + j, dtype=torch.int32))
            offsets.append(offsets[-1] + inds.numel())
    if not out_boxes:
        return (torch.zeros((0, 4)), torch.zeros((0,)), torch.zeros((0,), dtype=torch.int32),
                torch.tensor(offsets, dtype=torch.int32))
    return (torch.cat(out_boxes, 0).reshape(-1, 4), torch.cat(out_scores, 0), torch.cat(out_group, 0),
            torch.tensor(offsets, dtype=torch.int32))


# ---- box voting and view-averaged masks of test-time augmentation (not in the reference; Detectron's box_voting, method ID) ----
def vote_boxes(cand_boxes, cand_scores, offsets, cand_group, kept, vote_thresh):
    """[D, 4] (``ovis_cpu_vote_boxes_f32``); the operands as ``_C.vote_boxes`` checked them."""
    k, d = cand_boxes.shape[0], kept.shape[0]
    out = torch.empty((d, 4), dtype=torch.float32)
    if d:
        _check(load().ovis_cpu_vote_boxes_f32(cand_boxes.data_ptr() if k else 0, cand_scores.data_ptr() if k else 0,
                                              offsets.data_ptr(), cand_group.data_ptr() if k else 0, k, offsets.numel() - 1,
                                              kept.data_ptr(), d, float(vote_thresh), out.data_ptr()),
               "vote_boxes: a kept index outside the candidate list or outside its (image, class) run")
    return out


def average_view_masks(maps, flip_bits):
    """[D, 1, M, M] (``ovis_cpu_average_view_masks_f32``); the operands as ``_C.average_view_masks`` checked them."""
    v, d, _, m, _ = maps.shape
    out = torch.empty((d, 1, m, m), dtype=torch.float32)
    if d:
        _check(load().ovis_cpu_average_view_masks_f32(maps.data_ptr(), v, d, m, flip_bits, out.data_ptr()),
               "average_view_masks")
    return out


# ---- Soft-NMS over the runs of a candidate list (not in the reference; Bodla et al., ICCV 2017: include/ovis_hip.h) ---------
def soft_nms(cand_boxes, cand_scores, offsets, method, nms_thresh, sigma, min_score):
    """[K] (``ovis_cpu_soft_nms_f32``); the operands as ``_C.soft_nms`` checked them, ``method`` an OVIS_SOFT_NMS_* value."""
    k = cand_boxes.shape[0]
    out = torch.empty((k,), dtype=torch.float32)
    if k:
        _check(load().ovis_cpu_soft_nms_f32(cand_boxes.data_ptr(), cand_scores.data_ptr(), offsets.data_ptr(), k,
                                            offsets.numel() - 1, int(method), float(nms_thresh), float(sigma), float(min_score),
                                            out.data_ptr()),
               "soft_nms: malformed offsets (not 0 first, decreasing, negative, or not ending at the number of candidates)",
               "OVIS_EINVAL (an unknown method, sigma <= 0 or min_score < 0)")
    return out
