"""Pictures of what the detector found: boxes, filled instance masks, class names and -- for the pseudo-labelled
instances -- the predicted uncertainty map as a heat layer, on the original image.

Counterpart of maskrcnn_benchmark/engine/inference.py:177-196 (``select_top_predictions``), :347-442
(``visualization_mask``: overlay_boxes -> overlay_filled_mask -> overlay_class_names) and :212-345
(``visualization_uncertainty``, its combined view :330-343).  The reference pastes every mask into a full-size canvas on
the host and blends it with three whole-image ``np.where`` passes per instance; here the M x M maps, boxes and colours go
to ``_C.render_instances`` as they are -- one launch on the device the predictions live on (host tensors: the host twin),
no [K, H, W] masks.  Only the class names are drawn on the host afterwards, with PIL: cv2's Hershey stroke fonts are not
available here and not reproducible without cv2, so the text is PIL's default bitmap font on a white plate, NOT the
reference's glyphs.  Box outlines follow the band rule of include/ovis_hip.h, not cv2.rectangle's thick-line coverage.

The reference draws on ``cv2.imread``'s BGR image, so its colour tuples are BGR: (0, 0, 255) is red.  The images of this
package are RGB (data/datasets.py); ``bgr=False`` (the default) applies every reference tuple reversed, so the picture has
the reference's colours, ``bgr=True`` applies them as written.
"""
import numpy as np
import torch

from .. import _C

MASK_THRESHOLD = 0.5           # Masker(threshold=0.5, padding=1), inference.py:405-406
UNSEEN_COLOR = (0, 0, 255)     # boxes and names of unseen classes, inference.py:497,535 (BGR)
SEEN_COLOR = (0, 0, 0)
HEAT_COLOR = (0, 0, 255)       # overlay_uncertainty_mask, inference.py:575 (BGR)
HEAT_GAIN = 0.2                # np.clip(mask * (0.2 / s)), inference.py:584
BOX_THICKNESS = 2              # overlay_boxes, inference.py:532


def select_top_predictions(boxlist, threshold=0.5):
    """The detections scoring above ``threshold``, best first (inference.py:177-196)."""
    scores = boxlist.get_field("scores")
    keep = torch.nonzero(scores > threshold).squeeze(1)
    boxlist = boxlist[keep]
    _, idx = boxlist.get_field("scores").sort(0, descending=True)
    return boxlist[idx]


def colors_for_labels(labels):
    """uint8 [K, 3]: a fixed colour per class (the formula of compute_colors_for_labels, inference.py:510-517)."""
    palette = torch.tensor([2 ** 25 - 1, 2 ** 15 - 1, 2 ** 21 - 1], dtype=torch.int64)
    return ((labels.to("cpu", torch.int64)[:, None] * palette) % 255).to(torch.uint8)


def _maps(boxlist, name, value):
    if not torch.is_tensor(value) or not value.is_floating_point() or value.dim() != 4 or value.shape[1] != 1 \
            or value.shape[2] != value.shape[3] or value.shape[0] != len(boxlist):
        raise ValueError(
            f"render_predictions: field '{name}' must hold the mask head's [K, 1, M, M] probability maps, got "
            f"{getattr(value, 'dtype', type(value).__name__)} {tuple(getattr(value, 'shape', ()))}; masks that are already "
            "pasted into the image (MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS True) cannot be rendered -- run inference with "
            "MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS False")
    return value[:, 0].float()


def render_predictions(image_u8, boxlist, class_names=None, *, threshold=0.5, uncertainty=None, unseen_labels=(), bgr=False):
    """uint8 numpy [H, W, 3]: ``boxlist``'s detections drawn on ``image_u8`` (uint8 [H, W, 3], array or tensor).

    1. the BoxList is resized to the image's own size (inference.py:420);
    2. the detections scoring above ``threshold`` are kept, best first (:421);
    3. every box is outlined, black or -- for a label in ``unseen_labels`` -- red (:437, overlay_boxes);
    4. every instance's ``mask`` map is pasted, thresholded at 0.5 and filled with its class colour at alpha 0.5 (:438);
    5. with ``uncertainty`` ([K, 1, M, M], one map per box of ``boxlist``) each fill is followed by that instance's heat
       layer -- the interleaved sequence of the combined view (:330-343): gain 0.2 / score, colour HEAT_COLOR.  (The
       reference first replaces the scores by 0.01 / mean uncertainty and keeps one instance per class, :295-305; pass the
       BoxList prepared that way to get its picture);
    6. with ``class_names`` (indexed by label) the names are drawn at the boxes' top-left corners, upper-cased for unseen
       labels (:461-508) -- on the host, with PIL.
    A BoxList without a ``mask`` field (a box-only model) gets steps 3 and 6 only.  Steps 3-5 are one
    ``_C.render_instances`` call on the device of the ``mask`` field."""
    image = torch.as_tensor(np.asarray(image_u8) if not torch.is_tensor(image_u8) else image_u8)
    if image.dim() != 3 or image.shape[2] != 3 or image.dtype != torch.uint8:
        raise ValueError(f"render_predictions: expected a uint8 [H, W, 3] image, got {image.dtype} {tuple(image.shape)}")
    height, width = int(image.shape[0]), int(image.shape[1])
    if not boxlist.has_field("mask"):  # a box-only model: outlines and names (a 1 x 1 zero map fills nothing)
        boxlist = boxlist[torch.arange(len(boxlist), device=boxlist.bbox.device)]
        boxlist.add_field("mask", torch.zeros((len(boxlist), 1, 1, 1), dtype=torch.float32, device=boxlist.bbox.device))
    maps = _maps(boxlist, "mask", boxlist.get_field("mask"))
    if uncertainty is not None:
        _maps(boxlist, "uncertainty", uncertainty)
        boxlist = boxlist[torch.arange(len(boxlist), device=boxlist.bbox.device)]  # a copy: the caller's fields stay
        boxlist.add_field("_uncertainty", uncertainty)
    top = select_top_predictions(boxlist.resize((width, height)), threshold)
    k = len(top)
    device = maps.device
    order = [0, 1, 2] if bgr else [2, 1, 0]
    labels = top.get_field("labels").to("cpu", torch.int64)
    unseen = torch.tensor([int(l) in set(int(u) for u in unseen_labels) for l in labels.tolist()], dtype=torch.bool)
    maps = top.get_field("mask")[:, 0].float()
    fill_colors = colors_for_labels(labels).float()[:, order]
    outline = torch.tensor(SEEN_COLOR, dtype=torch.uint8).repeat(k, 1)
    outline[unseen] = torch.tensor([UNSEEN_COLOR[c] for c in order], dtype=torch.uint8)
    boxes = top.bbox.float()
    if uncertainty is None:
        kinds = torch.zeros(k, dtype=torch.int32)
        params = torch.full((k,), MASK_THRESHOLD, dtype=torch.float32)
        colors = fill_colors
    else:  # fill_0, heat_0, fill_1, heat_1, ...
        twice = torch.arange(k).repeat_interleave(2)
        gains = torch.tensor([np.float32(HEAT_GAIN / s) for s in top.get_field("scores").tolist()], dtype=torch.float32)
        maps = torch.stack((maps, top.get_field("_uncertainty")[:, 0].float().to(device)), 1).reshape(2 * k, *maps.shape[1:])
        boxes, outline = boxes[twice.to(boxes.device)], outline[twice]
        kinds = torch.tensor([0, 1], dtype=torch.int32).repeat(k)
        params = torch.stack((torch.full((k,), MASK_THRESHOLD), gains), 1).reshape(-1)
        colors = torch.stack((fill_colors, torch.tensor([HEAT_COLOR[c] for c in order], dtype=torch.float32).repeat(k, 1)), 1).reshape(-1, 3)
    out = _C.render_instances(image.to(device), maps.contiguous(), boxes.to(device).contiguous(), colors.to(device).contiguous(),
                              kinds.to(device), params.to(device), 0.5, outline.to(device).contiguous(), BOX_THICKNESS)
    out = out.cpu().numpy()
    if class_names is None or k == 0:
        return out
    return _draw_names(out, top.bbox.cpu(), labels.tolist(), unseen.tolist(), class_names, order)


def _draw_names(image, boxes, labels, unseen, class_names, order):
    """overlay_class_names (inference.py:461-508, display_score=False) with PIL: the name on a white plate at the box's
    top-left corner (truncated toward zero), red and upper-cased for an unseen label."""
    from PIL import Image, ImageDraw, ImageFont

    canvas = Image.fromarray(image)
    draw = ImageDraw.Draw(canvas)
    font = ImageFont.load_default()
    for box, label, is_unseen in zip(boxes.to(torch.int64).tolist(), labels, unseen):
        name = str(class_names[label])
        name = name.upper() if is_unseen else name
        x, y = box[0], box[1]
        draw.rectangle(draw.textbbox((x, y), name, font=font), fill=(255, 255, 255))
        draw.text((x, y), name, fill=tuple((UNSEEN_COLOR if is_unseen else SEEN_COLOR)[c] for c in order), font=font)
    return np.asarray(canvas).copy()
