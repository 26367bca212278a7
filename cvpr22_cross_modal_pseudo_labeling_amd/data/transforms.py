"""The input transform, split where the bytes are smallest (maskrcnn_benchmark/data/transforms/build.py:5-46 over
transforms.py:27-120, and the zero padding of structures/image_list.py:29-70).

The reference runs Resize -> RandomHorizontalFlip -> RandomVerticalFlip -> ToTensor -> Normalize per image in the loader
workers and ships float32 3 x 800 x 1333 images to the device.  Here the loader worker only DECIDES (``host``: the size, the
flips, the targets' geometry) and packs the raw uint8 images with a seven-int descriptor each; the pixels are produced on
the device (``device``: ``_C.transform_images``, two launches per batch) with the values PIL would have produced, bit for
bit.  A raw 480 x 640 image is 0.9 MB against 12.8 MB of float32 at 800 x 1066.

Colour jitter (INPUT.BRIGHTNESS / CONTRAST / SATURATION / HUE; transforms.py:88-102, first in the training Compose) is split
the same way: ``host`` draws each image's factors and the order of its operations, ``device`` runs them on the packed bytes
in front of the resize (``_C.color_jitter``, at most two launches per batch), with the bytes PIL produces.  The draw rule
(``jitter_draws``) and the composition of the PIL calls are torchvision 0.4-0.7's ``ColorJitter`` written out, not run
against torchvision.  It is an opt-in of ``build_transforms(..., color_jitter=True)`` (tools/train_net.py --color-jitter);
without it non-zero values raise where the transform is built, and evaluation transforms never jitter.

Scale jitter with a fixed-size crop (large-scale jitter; Detectron2's ResizeScale + FixedSizeCrop restated, not run against
Detectron2) is a third opt-in, ``build_transforms(..., scale_jitter=(lo, hi), crop_size=(h, w))`` (tools/train_net.py
--scale-jitter LO HI [--crop-size H W]).  ``host`` draws a scale in place of the size and a crop window behind the flips
(``scale_crop_draws``; include/ovis_hip.h states the rule in full), crops the targets to the window and emits 11-column
descriptors; ``device`` makes only the window's pixels (``_C.transform_images_window``).  Every batch is [B, 3, canvas].

Copy-paste (the other half of Simple Copy-Paste, Ghiasi et al. 2021; this project's own rule, stated in include/ovis_hip.h and
NOT compared with any other implementation's output) is a fourth opt-in on top of scale jitter,
``build_transforms(..., copy_paste=P)`` (tools/train_net.py --copy-paste P).  ``host`` decides, behind every per-image draw,
which image receives which instances of its neighbour in the batch (``copy_paste_draws``, ``paste_target``); calling the
transform with a staged batch rasterises, covers and re-boxes the masks on the copy stream and composites the pixels in
place on the training stream (``InputTransform.paste``: ``_C.copy_paste_masks`` / ``_C.copy_paste_images``).
"""
import random

import numpy as np
import torch

from .. import _C
from ..modeling.structures import BoxList, CopyPasteMasks, ImageList, PolygonMasks, RleMasks, TensorHolder, raise_on_bad_rle
from .prefetch import copy_stream

FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM = 0, 1


def get_size(w, h, min_size, max_size):
    """(out_h, out_w) of ``Resize.get_size`` (transforms.py:35-55) for a (w, h) image and the chosen ``min_size``."""
    size = min_size
    if max_size is not None:
        min_original_size = float(min((w, h)))
        max_original_size = float(max((w, h)))
        if max_original_size / min_original_size * size > max_size:
            size = int(round(max_size * min_original_size / max_original_size))
    if (w <= h and w == size) or (h <= w and h == size):
        return (h, w)
    if w < h:
        ow = size
        oh = int(size * h / w)
    else:
        oh = size
        ow = int(size * w / h)
    return (oh, ow)


JITTER_KEYS = ("BRIGHTNESS", "CONTRAST", "SATURATION", "HUE")  # their positions are the operation codes of _C.color_jitter


def check_color_jitter(values):
    """(brightness, contrast, saturation, hue) as floats; a value below 0, or HUE above 0.5, is a ValueError naming the key."""
    values = tuple(float(v) for v in values)
    if len(values) != 4:
        raise ValueError("color_jitter: expected (brightness, contrast, saturation, hue)")
    for key, v in zip(JITTER_KEYS, values):
        if not 0 <= v <= (0.5 if key == "HUE" else float("inf")):
            raise ValueError(f"INPUT.{key} = {v}: expected a value " + ("in [0, 0.5]" if key == "HUE" else ">= 0"))
    return values


def jitter_draws(rng, values):
    """One image's ([4 operation codes], [4 parameters]) of ``_C.color_jitter``, drawn as torchvision 0.4-0.7's
    ``ColorJitter.get_params`` draws on Python's ``random`` (our rule: not run against torchvision).  The keys in the order
    brightness, contrast, saturation, hue: one ``rng.uniform`` per key whose value is non-zero -- [max(0, 1 - v), 1 + v],
    for hue [-v, v] -- then ONE ``rng.shuffle`` of the active operations.  The hue parameter is the shift PIL's uint8
    addition makes, ``int(hue_factor * 255) % 256`` in Python doubles (truncation toward zero, then the wrap)."""
    active = []
    for code, v in enumerate(values):
        if v != 0:
            f = rng.uniform(-v, v) if code == 3 else rng.uniform(max(0.0, 1.0 - v), 1.0 + v)
            active.append((code, float(int(f * 255) % 256) if code == 3 else f))
    rng.shuffle(active)
    pad = 4 - len(active)
    return [code for code, _ in active] + [-1] * pad, [p for _, p in active] + [0.0] * pad


CROP_SIZE = (1024, 1024)   # the default canvas of scale jitter
MAX_REDRAWS = 8            # of a crop window that leaves an annotated image without a box
MAX_DIM = 16384            # kResampleMaxDim of csrc/resample_geom.h: every image, resized and canvas dimension


def check_scale_jitter(scale_jitter, crop_size=None):
    """((lo, hi), (crop_h, crop_w)) checked: 0 < lo <= hi, canvas sides >= 1, hi * side <= 16384 (the largest resized
    dimension the kernels take).  A ValueError names what is off."""
    try:
        lo, hi = (float(v) for v in scale_jitter)
        crop_h, crop_w = (int(v) for v in (crop_size if crop_size is not None else CROP_SIZE))
    except (TypeError, ValueError):
        raise ValueError(f"scale_jitter = {scale_jitter}, crop_size = {crop_size}: expected (lo, hi) and (height, width)")
    if not 0 < lo <= hi or hi == float("inf"):
        raise ValueError(f"scale_jitter = ({lo}, {hi}): expected 0 < lo <= hi")
    if crop_h < 1 or crop_w < 1:
        raise ValueError(f"crop_size = ({crop_h}, {crop_w}): a canvas side is at least 1")
    if hi * max(crop_h, crop_w) > MAX_DIM:
        raise ValueError(f"scale_jitter hi = {hi} times crop_size = ({crop_h}, {crop_w}) is above {MAX_DIM}, the largest "
                         "resized dimension the transform takes")
    return (lo, hi), (crop_h, crop_w)


def jittered_size(h, w, s, crop_size):
    """(out_h, out_w) of an h x w image at scale ``s`` of the canvas: ResizeScale -- the canvas times s, the image fitted
    inside it with its aspect ratio; Python doubles and Python's round."""
    crop_h, crop_w = crop_size
    r = min(crop_h * s / h, crop_w * s / w)
    return max(1, round(h * r)), max(1, round(w * r))


def crop_window(rng, out_hw, crop_size):
    """(win_y, win_x, win_h, win_w) of FixedSizeCrop in an out_h x out_w image: two draws, whatever the sizes."""
    (out_h, out_w), (crop_h, crop_w) = out_hw, crop_size
    fy, fx = rng.random(), rng.random()
    win_y, win_x = round(fy * max(out_h - crop_h, 0)), round(fx * max(out_w - crop_w, 0))
    return win_y, win_x, min(crop_h, out_h - win_y), min(crop_w, out_w - win_x)


def crop_target(target, window):
    """``target`` (in the frame of the resized, flipped image) through the window: BoxList.crop, fields through their own
    ``crop``, then clip_to_image(remove_empty=True).  Its size is (win_w, win_h)."""
    win_y, win_x, win_h, win_w = window
    return target.crop((win_x, win_y, win_x + win_w, win_y + win_h)).clip_to_image(remove_empty=True)


def scale_crop_draws(rng, out_hw, crop_size, target=None):
    """The window of one image, ``target`` its resized and flipped BoxList (or None): a window is drawn; when the image has
    a box and none survives the crop it is drawn again, at most MAX_REDRAWS times -- the last draw stands.
    -> (window, the cropped target or None)."""
    boxes = None
    if target is not None and len(target):
        boxes = type(target)(target.bbox, target.size)  # the survival test needs no field
    for _ in range(1 + MAX_REDRAWS):
        window = crop_window(rng, out_hw, crop_size)
        if boxes is None or len(crop_target(boxes, window)):
            break
    return window, (crop_target(target, window) if target is not None else None)


def check_copy_paste(p):
    """P of copy-paste as a float in (0, 1]; anything else is a ValueError."""
    try:
        p = float(p)
    except (TypeError, ValueError):
        raise ValueError(f"copy_paste = {p!r}: expected a probability in (0, 1]")
    if not 0 < p <= 1:
        raise ValueError(f"copy_paste = {p}: expected a probability in (0, 1]")
    return p


def copy_paste_draws(rng, p, counts):
    """What is pasted where in a batch whose cropped targets hold ``counts[i]`` instances: for i = 0 .. B-1 in order the
    source is j = (i + 1) % B; ``u = rng.random()``, image i receives a paste iff u < p; then one ``rng.random()`` per
    instance of j, in order, an instance selected iff its draw is < 0.5.  -> per image (j, [selected rows of j]), or None
    when it receives nothing (u >= p, a source without instances, no instance selected)."""
    plan = []
    for i in range(len(counts)):
        j = (i + 1) % len(counts)
        picked = []
        if rng.random() < p:
            picked = [g for g in range(counts[j]) if rng.random() < 0.5]
        plan.append((j, picked) if picked else None)
    return plan


def _polygon_masks(target, i, role):
    masks = target.get_field("masks") if target.has_field("masks") else None
    if not isinstance(masks, PolygonMasks):
        what = "RLE masks" if isinstance(masks, RleMasks) else ("no masks" if masks is None else type(masks).__name__)
        name = f"image {i} of the batch" + (f" (image id {masks.image_id})" if isinstance(masks, RleMasks) else "")
        raise ValueError(f"{name}, the {role} of a copy-paste, carries {what}: copy-paste needs polygon ground truth")
    return masks


def paste_target(dst, src, picked, i, j):
    """The target of image i once rows ``picked`` of image j's target are pasted over it, both in the canvas frame (their
    windows start at its origin): size the element-wise maximum of the two, boxes and labels cat(own, picked), the source's
    boxes as they are; ``masks`` a ``CopyPasteMasks`` for the device half; every other field the destination's."""
    own, pasted = _polygon_masks(dst, i, "destination"), _polygon_masks(src, j, "source")
    size = (max(dst.size[0], src.size[0]), max(dst.size[1], src.size[1]))
    rows = torch.tensor(picked, dtype=torch.int64)
    out = BoxList(torch.cat([dst.bbox, src.bbox[rows]]), size)
    for k, v in dst.extra_fields.items():
        if k == "labels":
            v = torch.cat([v, src.get_field("labels")[rows]])
        elif k == "masks":
            v = CopyPasteMasks(own, pasted[rows], size, j)
        out.add_field(k, v)
    return out


class InputTransform:
    """``host(images, targets)`` in the loader worker, ``device(raw)`` on the training process' stream; calling the object
    with a staged batch ``(raw, targets, ...)`` applies the device half -- the form ``DevicePrefetcher(transform=)`` takes.
    ``color_jitter``: (brightness, contrast, saturation, hue) of ColorJitter, None or all zero for none.
    ``scale_jitter``: (lo, hi), the scale range of large-scale jitter on the canvas ``crop_size`` = (height, width), default
    1024 x 1024; None for none -- then ``crop_size`` must be None too, and both halves are what they are without it.
    ``copy_paste``: P in (0, 1], the probability that an image receives objects of its neighbour in the batch; needs
    ``scale_jitter``; None for none -- then no draw, no launch and no field differs."""

    def __init__(self, min_size, max_size, flip_horizontal_prob, flip_vertical_prob, mean, std, to_bgr255, size_divisible=0,
                 seed=0, color_jitter=None, scale_jitter=None, crop_size=None, copy_paste=None):
        if scale_jitter is None and crop_size is not None:
            raise ValueError("crop_size is the canvas of scale_jitter: give scale_jitter too")
        if copy_paste is not None and scale_jitter is None:
            raise ValueError("copy_paste pastes at the same position of a fixed canvas: give scale_jitter too")
        self.copy_paste = check_copy_paste(copy_paste) if copy_paste is not None else None
        self.scale_jitter, self.crop_size = check_scale_jitter(scale_jitter, crop_size) if scale_jitter is not None else (None, None)
        self.color_jitter = check_color_jitter(color_jitter) if color_jitter is not None else (0.0,) * 4
        if not any(self.color_jitter):
            self.color_jitter = None
        self.min_size = tuple(min_size) if isinstance(min_size, (list, tuple)) else (min_size,)
        self.max_size = max_size
        self.flip_horizontal_prob, self.flip_vertical_prob = float(flip_horizontal_prob), float(flip_vertical_prob)
        self.mean, self.std = [float(v) for v in mean], [float(v) for v in std]
        self.to_bgr255, self.size_divisible = bool(to_bgr255), int(size_divisible)
        self.rng = random.Random(seed)
        self._pending_rle = None  # (status in pinned host memory, the event of its copy, names) of the last decoded batch

    # -- host half ----------------------------------------------------------------------------------------------------
    def host(self, images, targets=None, rng=None):
        """images: uint8 [h, w, 3] RGB arrays / host tensors of any sizes; targets: their BoxLists (or None).
        -> (raw, targets): ``raw`` holds the packed bytes, the descriptors and the sizes the device half needs as python
        ints; the targets are resized and flipped copies.  The random draws are the reference's, in its order (the colour
        jitter's when it is on -- ``jitter_draws``, then ``raw`` also holds ``jitter_ops`` / ``jitter_params`` [B, 4] -- the
        size, then one draw per flip), from ``rng`` or the transform's own seeded generator.  With ``scale_jitter`` the
        size draw is the scale's, the window's draws follow the flips (``scale_crop_draws``), the descriptors have 11
        columns, ``image_sizes`` holds the windows' (win_h, win_w), ``pad_hw`` is the canvas and the targets are cropped.
        With ``copy_paste``, a batch of at least two images and targets, the copy-paste draws follow ALL of those
        (``copy_paste_draws``); ``raw["paste_src"]`` int32 [B] then holds every image's source or -1, and a pasted-into image
        has its new frame in ``image_sizes`` and the target of ``paste_target``."""
        rng = rng or self.rng
        if len(images) == 0:
            raise ValueError("InputTransform.host: an empty batch has no padded size")
        desc, chunks, sizes, out_targets, offset, jitter = [], [], [], [], 0, []
        for i, img in enumerate(images):
            img = torch.as_tensor(np.ascontiguousarray(img) if isinstance(img, np.ndarray) else img)
            if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
                raise ValueError(f"image {i}: expected uint8 [h, w, 3], got {img.dtype} {tuple(img.shape)}")
            h, w = int(img.shape[0]), int(img.shape[1])
            if self.color_jitter is not None:  # ColorJitter is first in the Compose
                jitter.append(jitter_draws(rng, self.color_jitter))
            if self.scale_jitter is not None:  # in place of the size draw
                oh, ow = jittered_size(h, w, rng.uniform(*self.scale_jitter), self.crop_size)
            else:
                oh, ow = get_size(w, h, rng.choice(self.min_size), self.max_size)
            flip_h = rng.random() < self.flip_horizontal_prob
            flip_v = rng.random() < self.flip_vertical_prob
            desc.append([offset, h, w, oh, ow, int(flip_h), int(flip_v)])
            chunks.append(img.contiguous().view(-1))
            offset += h * w * 3
            if offset >= 2 ** 31:
                raise ValueError("a batch of raw images is limited to 2 GiB")
            t = None
            if targets is not None:
                t = targets[i].resize((ow, oh))
                if flip_h:
                    t = t.transpose(FLIP_LEFT_RIGHT)
                if flip_v:
                    t = t.transpose(FLIP_TOP_BOTTOM)
            if self.scale_jitter is not None:  # the window lives in the frame of the resized, flipped image
                window, t = scale_crop_draws(rng, (oh, ow), self.crop_size, t)
                desc[-1] += list(window)
                sizes.append((window[2], window[3]))
            else:
                sizes.append((oh, ow))
            if targets is not None:
                out_targets.append(t)
        paste_src = None
        if self.copy_paste is not None and targets is not None and len(images) >= 2:
            plan = copy_paste_draws(rng, self.copy_paste, [len(t) for t in out_targets])
            before = out_targets  # sources are the pre-paste targets: nothing is pasted onward
            out_targets = [t if p is None else paste_target(t, before[p[0]], p[1], i, p[0])
                           for i, (t, p) in enumerate(zip(before, plan))]
            sizes = [s if p is None else (t.size[1], t.size[0]) for s, t, p in zip(sizes, out_targets, plan)]
            paste_src = torch.tensor([-1 if p is None else p[0] for p in plan], dtype=torch.int32)
        pad_h, pad_w = self.crop_size or (max(s[0] for s in sizes), max(s[1] for s in sizes))
        if self.size_divisible > 0:  # image_list.py:54-61
            d = self.size_divisible
            pad_h, pad_w = -(-pad_h // d) * d, -(-pad_w // d) * d
        raw = {"data": torch.cat(chunks), "desc": torch.tensor(desc, dtype=torch.int32), "image_sizes": sizes,
               "pad_hw": (pad_h, pad_w), "max_in_hw": (max(d[1] for d in desc), max(d[2] for d in desc))}
        if paste_src is not None:
            raw["paste_src"] = paste_src
        if jitter:
            raw["jitter_ops"] = torch.tensor([ops for ops, _ in jitter], dtype=torch.int32)
            raw["jitter_params"] = torch.tensor([params for _, params in jitter], dtype=torch.float32)
        return raw, (out_targets if targets is not None else None)

    # -- device half --------------------------------------------------------------------------------------------------
    def device(self, raw):
        """-> ImageList [B, 3, pad_h, pad_w] with the per-image (h, w), on the device ``raw``'s tensors live on."""
        data = raw["data"]
        if "jitter_ops" in raw:  # the host half knows whether contrast can occur: its grey-sum launch is skipped otherwise
            data = _C.color_jitter(data, raw["desc"][:, :7], raw["jitter_ops"], raw["jitter_params"], raw["max_in_hw"],
                                   contrast=self.color_jitter is None or self.color_jitter[1] != 0)
        make = _C.transform_images_window if self.scale_jitter is not None else _C.transform_images
        tensors = make(data, raw["desc"], self.mean, self.std, self.to_bgr255, raw["pad_hw"], raw["max_in_hw"])
        return ImageList(tensors, [tuple(s) for s in raw["image_sizes"]])

    def decode_masks(self, targets):
        """The RLE ground truth of a staged batch (``RleMasks`` fields of its BoxLists) as bit words, ONE decode call for
        the batch on the current stream, sizes and value counts from the host: nothing is read back.  A malformed
        encoding decodes to an all-zero mask; its status goes to pinned host memory without blocking and is examined when
        the NEXT batch comes through here (``flush``: and when the iterator ends) -- a ValueError naming the image and the
        annotation, at most one step late and without a synchronisation on the training stream."""
        self.flush()
        masks = []
        for t in targets or ():
            for v in (t.extra_fields.values() if hasattr(t, "extra_fields") else ()):
                if isinstance(v, RleMasks) and v.chars.is_cuda:
                    masks.append(v)
        status, names = RleMasks.decode_many(masks)
        if status is not None:
            host = torch.empty(status.shape, dtype=status.dtype, pin_memory=True)
            host.copy_(status, non_blocking=True)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(status.device))
            self._pending_rle = (host, done, names, status)

    def flush(self):
        """Examine the decode status of the last batch (its copy was enqueued a step ago)."""
        pending, self._pending_rle = self._pending_rle, None
        if pending is not None:
            host, done, names, _ = pending
            done.synchronize()
            raise_on_bad_rle(host, names)

    def paste(self, images, targets):
        """The device half of copy-paste for a staged batch: ``images`` the ImageList ``device`` made, ``targets`` the staged
        BoxLists; every target whose ``masks`` is a ``CopyPasteMasks`` receives its source's objects.  -> the new targets.
        The mask work -- rasterise own + pasted polygons at the new frame, alpha = OR of the pasted, own &= ~alpha, the
        per-mask counts and tight boxes, the table's copy to pinned memory, and the few row gathers the host's decision
        asks for -- runs on the copy stream (``prefetch.copy_stream``), which already orders the staged polygons' copies:
        the host waits for an EVENT of that stream, never for the training stream and the step queued on it.  The training
        stream waits for the same stream's last event before the pixels are composited in place on it."""
        holders = [t.get_field("masks") if (t is not None and t.has_field("masks")) else None for t in targets]
        todo = [i for i, m in enumerate(holders) if isinstance(m, CopyPasteMasks)]
        if not todo:
            return targets
        batch = images.tensors
        if not batch.is_cuda:
            raise NotImplementedError("copy-paste is device code: MODEL.DEVICE cpu is not supported")
        cur, side = torch.cuda.current_stream(batch.device), copy_stream(batch.device)
        out, made = list(targets), []
        with torch.cuda.stream(side):
            masks, alphas, stats = {}, [None] * len(targets), []
            for i in todo:
                masks[i] = holders[i].polygons.convert_to_binarymask()  # uint8 [G_own + G_paste, h, w] at the new frame
                alphas[i], table = _C.copy_paste_masks(masks[i], holders[i].num_own)
                stats.append(table)
            table = torch.cat(stats)
            host = torch.empty(table.shape, dtype=torch.int32, pin_memory=True)
            host.copy_(table, non_blocking=True)
            read = torch.cuda.Event()
            read.record(side)
            read.synchronize()  # the only read-back
            at = 0
            for i in todo:
                t, n_own, g = targets[i], holders[i].num_own, len(holders[i])
                keep, tight = copy_paste_keep(host[at:at + n_own].tolist())
                at += n_own
                rows = keep + list(range(n_own, g))  # pasted instances always stay
                bbox, labels, dense = t.bbox, t.get_field("labels"), masks[i]
                if len(rows) != g:
                    index = torch.tensor(rows, dtype=torch.int64).to(batch.device)
                    bbox, labels, dense = bbox[index], labels[index], dense[index]
                if tight:
                    bbox = bbox.clone() if bbox is t.bbox else bbox
                    where = torch.tensor([rows.index(k) for k in tight], dtype=torch.int64).to(batch.device)
                    bbox[where] = torch.tensor([tight[k] for k in tight], dtype=torch.float32).to(batch.device)
                new = BoxList(bbox, t.size)
                for k, v in t.extra_fields.items():
                    new.add_field(k, labels if k == "labels" else dense if k == "masks" else v)
                out[i] = new
                made += [bbox, labels, dense, alphas[i]]
            done = torch.cuda.Event()
            done.record(side)
        for t in made:  # allocated on the copy stream, read by the step
            t.record_stream(cur)
        cur.wait_event(done)
        _C.copy_paste_images(batch, alphas, [holders[i].source if i in masks else -1 for i in range(len(targets))])
        return out

    def __call__(self, batch):
        if len(batch) > 1:
            self.decode_masks(batch[1])
        images = self.device(batch[0])
        if "paste_src" in batch[0]:
            return (images, self.paste(images, batch[1])) + tuple(batch[2:])
        return (images,) + tuple(batch[1:])


def copy_paste_keep(stats):
    """The host's decision over the table of ``_C.copy_paste_masks``: rows (pixels before, pixels after, x1, y1, x2, y2) of
    an image's own instances.  An instance whose count did not change is untouched: it stays with its annotation box, even
    at a count of 0.  A touched one takes the tight box and stays iff x2 > x1 and y2 > y1 -- the test of
    ``clip_to_image(remove_empty=True)``, no new threshold.  -> (the rows kept, ascending; {kept touched row: its box})."""
    keep, tight = [], {}
    for g, (before, after, x1, y1, x2, y2) in enumerate(stats):
        if after == before:
            keep.append(g)
        elif x2 > x1 and y2 > y1:
            keep.append(g)
            tight[g] = [float(x1), float(y1), float(x2), float(y2)]
    return keep, tight


class ViewBatch(TensorHolder):
    """The test-time-augmentation views of one batch (TEST.BBOX_AUG): ``views[v]`` is the ``ImageList`` of view v over the
    same images, ``flips[v]`` whether that view is mirrored left-right.  View 0 is the un-augmented one: detections are
    reported in its frame and size."""

    _TENSORS = ("views",)

    def __init__(self, views, flips):
        self.views, self.flips = list(views), [bool(f) for f in flips]
        if not self.views or len(self.views) != len(self.flips):
            raise ValueError("ViewBatch: one flip flag per view, at least one view")

    def __len__(self):
        return len(self.views)


class ViewTransform:
    """The input transform of multi-scale / flip testing, with ``InputTransform``'s interface.  ``plan`` lists the views as
    (min_size, max_size, flip) in the reference's order (engine/bbox_aug.py:26-51).  The reference re-runs PIL per view in
    the loader; here ``host`` packs the bytes ONCE and emits one descriptor table per view over the same byte offsets (sizes
    from ``get_size``, the flip forced, not drawn; the flip acts after the resize, as Resize -> RandomHorizontalFlip(1.0)
    does), and ``device`` makes every view from the one upload, one ``_C.transform_images`` call per view."""

    def __init__(self, plan, mean, std, to_bgr255, size_divisible=0):
        self.plan = [(int(lo), int(hi), bool(flip)) for lo, hi, flip in plan]
        if not self.plan:
            raise ValueError("ViewTransform: at least one view")
        self.mean, self.std = [float(v) for v in mean], [float(v) for v in std]
        self.to_bgr255, self.size_divisible = bool(to_bgr255), int(size_divisible)

    def host(self, images, targets=None, rng=None):
        """-> (raw, None): ``raw["data"]`` the packed bytes; per view v ``raw["desc"][v]`` its [B, 7] descriptors,
        ``raw["image_sizes"][v]`` and ``raw["pad_hw"][v]`` (DATALOADER.SIZE_DIVISIBILITY applied per view).  The tensors sit
        at the top level of ``raw``, as ``InputTransform``'s do.  Evaluation only: targets are not transformed."""
        if targets is not None:
            raise ValueError("ViewTransform.host: test-time augmentation is an evaluation transform, it takes no targets")
        if len(images) == 0:
            raise ValueError("ViewTransform.host: an empty batch has no padded size")
        chunks, geom, offset = [], [], 0
        for i, img in enumerate(images):
            img = torch.as_tensor(np.ascontiguousarray(img) if isinstance(img, np.ndarray) else img)
            if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
                raise ValueError(f"image {i}: expected uint8 [h, w, 3], got {img.dtype} {tuple(img.shape)}")
            h, w = int(img.shape[0]), int(img.shape[1])
            geom.append((offset, h, w))
            chunks.append(img.contiguous().view(-1))
            offset += h * w * 3
            if offset >= 2 ** 31:
                raise ValueError("a batch of raw images is limited to 2 GiB")
        descs, view_sizes, pads = [], [], []
        for min_size, max_size, flip in self.plan:
            sizes = [get_size(w, h, min_size, max_size) for _, h, w in geom]
            desc = [[off, h, w, oh, ow, int(flip), 0] for (off, h, w), (oh, ow) in zip(geom, sizes)]
            pad_h, pad_w = max(s[0] for s in sizes), max(s[1] for s in sizes)
            if self.size_divisible > 0:  # image_list.py:54-61
                d = self.size_divisible
                pad_h, pad_w = -(-pad_h // d) * d, -(-pad_w // d) * d
            descs.append(desc)
            view_sizes.append(sizes)
            pads.append((pad_h, pad_w))
        raw = {"data": torch.cat(chunks), "desc": torch.tensor(descs, dtype=torch.int32), "image_sizes": view_sizes, "pad_hw": pads,
               "max_in_hw": (max(g[1] for g in geom), max(g[2] for g in geom))}
        return raw, None

    def device(self, raw):
        """-> ViewBatch on the device ``raw``'s tensors live on."""
        lists = []
        for desc, sizes, pad_hw in zip(raw["desc"], raw["image_sizes"], raw["pad_hw"]):
            tensors = _C.transform_images(raw["data"], desc, self.mean, self.std, self.to_bgr255, pad_hw, raw["max_in_hw"])
            lists.append(ImageList(tensors, [tuple(s) for s in sizes]))
        return ViewBatch(lists, [flip for _, _, flip in self.plan])

    def __call__(self, batch):
        return (self.device(batch[0]),) + tuple(batch[1:])


def view_plan(cfg):
    """The (min_size, max_size, flip) of every view of TEST.BBOX_AUG, in the order engine/bbox_aug.py:26-51 runs them."""
    aug = cfg.TEST.BBOX_AUG
    plan = [(cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, False)]
    if aug.H_FLIP:
        plan.append((cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, True))
    for scale in aug.SCALES:
        plan.append((scale, aug.MAX_SIZE, False))
        if aug.SCALE_H_FLIP:
            plan.append((scale, aug.MAX_SIZE, True))
    return plan


def build_transforms(cfg, is_train=True, seed=0, color_jitter=False, scale_jitter=None, crop_size=None, copy_paste=None):
    """build.py:5-46 for this package's split transform; the evaluation transform of TEST.BBOX_AUG.ENABLED makes every
    view (``ViewTransform``).  ``color_jitter=True`` honours INPUT.BRIGHTNESS / CONTRAST / SATURATION / HUE in the training
    transform; without the switch a non-zero key raises, and evaluation transforms never jitter.  ``scale_jitter`` =
    (lo, hi) with ``crop_size`` = (height, width): large-scale jitter in the training transform (INPUT.MIN_SIZE_TRAIN /
    MAX_SIZE_TRAIN are then not read); evaluation transforms and ``ViewTransform`` never scale-jitter.  ``copy_paste`` = P
    in (0, 1], with ``scale_jitter``: copy-paste between the images of a training batch; evaluation transforms never paste."""
    jitter = None
    if scale_jitter is None and crop_size is not None:
        raise ValueError("crop_size is the canvas of scale_jitter: give scale_jitter too")
    if copy_paste is not None and scale_jitter is None:
        raise ValueError("copy_paste pastes at the same position of a fixed canvas: give scale_jitter too")
    if is_train:
        min_size, max_size = cfg.INPUT.MIN_SIZE_TRAIN, cfg.INPUT.MAX_SIZE_TRAIN
        flip_h, flip_v = cfg.INPUT.HORIZONTAL_FLIP_PROB_TRAIN, cfg.INPUT.VERTICAL_FLIP_PROB_TRAIN
        values = {k: getattr(cfg.INPUT, k) for k in JITTER_KEYS}
        if color_jitter:
            jitter = check_color_jitter(values[k] for k in JITTER_KEYS)
        elif any(v != 0 for v in values.values()):
            raise NotImplementedError(f"colour jitter is an opt-in of the device input transform: build_transforms(..., "
                                      f"color_jitter=True) / tools/train_net.py --color-jitter honour INPUT {values}")
    else:
        if cfg.TEST.BBOX_AUG.ENABLED:
            return ViewTransform(view_plan(cfg), cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, cfg.INPUT.TO_BGR255,
                                 cfg.DATALOADER.SIZE_DIVISIBILITY)
        min_size, max_size = cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST
        flip_h = flip_v = 0.0
        scale_jitter = crop_size = copy_paste = None
    return InputTransform(min_size, max_size, flip_h, flip_v, cfg.INPUT.PIXEL_MEAN, cfg.INPUT.PIXEL_STD, cfg.INPUT.TO_BGR255,
                          cfg.DATALOADER.SIZE_DIVISIBILITY, seed=seed, color_jitter=jitter, scale_jitter=scale_jitter,
                          crop_size=crop_size, copy_paste=copy_paste)
