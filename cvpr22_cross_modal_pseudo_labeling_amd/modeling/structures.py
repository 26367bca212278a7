"""Box containers and box arithmetic with the reference's +1-pixel convention.

Behavioural counterpart of maskrcnn_benchmark/structures/bounding_box.py:9-255 (``BoxList``),
structures/boxlist_ops.py:9-129 (``boxlist_nms / remove_small_boxes / boxlist_iou / cat_boxlist``)
and structures/image_list.py:7-72, reduced to what the training hot path touches: boxes are always
``xyxy`` float32 tensors on the device, fields are plain tensors (or python objects), and instance
masks are a field in one of four forms: a dense ``[G, H, W]`` tensor, or ``PolygonMasks`` / ``RleMasks`` /
``PastedMasks``, which stay lazy and answer ``project`` for the mask head's targets (``CopyPasteMasks`` lives only between
the two halves of the input transform, which turns it into the dense form).

Every structure that carries tensors is a ``TensorHolder``: it declares the attributes that hold them, and
``map_tensors`` / ``to`` / ``device_tensors`` follow from that declaration (input staging: data/prefetch.py, stream
bookkeeping: engine/trainer.py::_record_stream).
"""
import numpy as np
import torch

from ..layers import nms as _nms

TO_REMOVE = 1.0


def map_tensors(obj, fn):
    """``obj`` -- a tensor, a list / tuple / dict, a ``TensorHolder``, nested in any way -- with ``fn`` applied to every
    tensor: the same nesting and types.  Anything else (None, strings, numbers) is carried over."""
    if torch.is_tensor(obj):
        return fn(obj)
    if isinstance(obj, (list, tuple)):
        return type(obj)(map_tensors(o, fn) for o in obj)
    if isinstance(obj, dict):
        return {k: map_tensors(v, fn) for k, v in obj.items()}
    if hasattr(obj, "map_tensors"):
        return obj.map_tensors(fn)
    return obj


class TensorHolder:
    """An object that holds tensors: ``_TENSORS`` names the attributes whose values are tensors, None, or lists / dicts /
    holders of tensors; every other attribute is state that a copy shares."""

    _TENSORS = ()

    def _with(self, **changes):
        """A shallow copy with the given attributes replaced."""
        out = object.__new__(type(self))
        out.__dict__ = {**self.__dict__, **changes}
        return out

    def map_tensors(self, fn):
        """A copy of the same type with ``fn`` applied to every tensor held."""
        held = self.__dict__
        return self._with(**{k: map_tensors(held[k], fn) for k in self._TENSORS})

    def to(self, *args, **kwargs):
        return self.map_tensors(lambda t: t.to(*args, **kwargs))

    def device_tensors(self):
        """What a stream has to be told about (engine/trainer.py::_record_stream): the values held, as they are -- a
        read-only walk, nothing is built."""
        held = self.__dict__
        return [held[k] for k in self._TENSORS if held[k] is not None]


class BoxList(TensorHolder):
    """xyxy boxes of one image + named per-box fields.  ``size`` is (width, height)."""

    _TENSORS = ("bbox", "extra_fields")  # a field that is a tensor or a holder is mapped, a string or other object carried over

    def __init__(self, bbox, image_size, mode="xyxy"):
        bbox = torch.as_tensor(bbox, dtype=torch.float32)
        if bbox.dim() != 2 or bbox.size(-1) != 4:
            raise ValueError(f"bbox should be [N,4], got {tuple(bbox.shape)}")
        if mode == "xywh":  # bounding_box.py:83-93
            x, y, w, h = bbox.unbind(1)
            bbox = torch.stack((x, y, x + (w - TO_REMOVE).clamp(min=0), y + (h - TO_REMOVE).clamp(min=0)), 1)
        elif mode != "xyxy":
            raise ValueError("mode should be 'xyxy' or 'xywh'")
        self.bbox = bbox
        self.size = tuple(image_size)
        self.mode = "xyxy"
        self.extra_fields = {}

    # -- fields ---------------------------------------------------------------
    def add_field(self, name, value):
        self.extra_fields[name] = value

    def get_field(self, name):
        return self.extra_fields[name]

    def has_field(self, name):
        return name in self.extra_fields

    def fields(self):
        return list(self.extra_fields.keys())

    def copy_with_fields(self, fields, skip_missing=False):
        out = BoxList(self.bbox, self.size)
        for f in [fields] if isinstance(fields, str) else fields:
            if self.has_field(f):
                out.add_field(f, self.get_field(f))
            elif not skip_missing:
                raise KeyError(f"field '{f}' not found")
        return out

    # -- tensor-like ------------------------------------------------------------
    def __len__(self):
        return self.bbox.shape[0]

    def __getitem__(self, item):
        if torch.is_tensor(item) and item.dtype == torch.bool:
            item = torch.nonzero(item).squeeze(1)  # ONE nonzero instead of one per indexed field
        out = BoxList(self.bbox[item], self.size)
        for k, v in self.extra_fields.items():
            if torch.is_tensor(v):
                out.add_field(k, v[item] if v.dim() > 0 and v.shape[0] == len(self) else v)
            elif isinstance(v, TensorHolder) and hasattr(v, "__getitem__"):
                out.add_field(k, v[item])  # per-box masks that can be indexed follow the boxes (bounding_box.py:233-242)
            else:
                out.add_field(k, v)
        return out

    def area(self):
        b = self.bbox
        return (b[:, 2] - b[:, 0] + TO_REMOVE) * (b[:, 3] - b[:, 1] + TO_REMOVE)

    def clip_to_image(self, remove_empty=True):  # bounding_box.py:214-225
        w, h = self.size
        b = self.bbox
        b[:, 0].clamp_(min=0, max=w - TO_REMOVE)
        b[:, 1].clamp_(min=0, max=h - TO_REMOVE)
        b[:, 2].clamp_(min=0, max=w - TO_REMOVE)
        b[:, 3].clamp_(min=0, max=h - TO_REMOVE)
        if remove_empty:
            keep = (b[:, 3] > b[:, 1]) & (b[:, 2] > b[:, 0])
            return self[keep]
        return self

    def _fields_follow(self, out, what, *args):
        """Fields of a resized / flipped / cropped copy: per-box tensors (labels, ids) and strings are geometry-free and
        carried over, as bounding_box.py:105-108 does; an object follows through its own ``resize`` / ``transpose`` / ``crop``.  A dense [G, H, W]
        mask tensor is tied to the old pixel grid and has neither: it raises instead of going stale."""
        for k, v in self.extra_fields.items():
            if torch.is_tensor(v):
                if v.dim() == 3 and v.shape[0] == len(self) and tuple(v.shape[1:]) == (self.size[1], self.size[0]):
                    raise NotImplementedError(f"BoxList.{what}: field '{k}' is a dense mask tensor; use PolygonMasks")
            elif not isinstance(v, str):
                if not hasattr(v, what):
                    raise NotImplementedError(f"BoxList.{what}: field '{k}' ({type(v).__name__}) has no {what}()")
                v = getattr(v, what)(*args)
            out.add_field(k, v)
        return out

    def resize(self, size):
        """A copy scaled to ``size`` = (width, height): bounding_box.py:91-127 (one ratio when both axes agree, else one
        per axis)."""
        size = tuple(int(s) for s in size)
        ratios = tuple(float(s) / float(s_orig) for s, s_orig in zip(size, self.size))
        if ratios[0] == ratios[1]:
            scaled = self.bbox * ratios[0]
        else:
            xmin, ymin, xmax, ymax = self.bbox.split(1, dim=-1)
            scaled = torch.cat((xmin * ratios[0], ymin * ratios[1], xmax * ratios[0], ymax * ratios[1]), dim=-1)
        return self._fields_follow(BoxList(scaled, size), "resize", size)

    def transpose(self, method):
        """FLIP_LEFT_RIGHT (0): x -> width - x - 1; FLIP_TOP_BOTTOM (1): y -> height - y (bounding_box.py:129-166)."""
        if method not in (0, 1):
            raise NotImplementedError("Only FLIP_LEFT_RIGHT and FLIP_TOP_BOTTOM implemented")
        width, height = self.size
        xmin, ymin, xmax, ymax = self.bbox.split(1, dim=-1)
        if method == 0:
            flipped = torch.cat((width - xmax - TO_REMOVE, ymin, width - xmin - TO_REMOVE, ymax), dim=-1)
        else:
            flipped = torch.cat((xmin, height - ymax, xmax, height - ymin), dim=-1)
        return self._fields_follow(BoxList(flipped, self.size), "transpose", method)

    def crop(self, box):
        """A copy cropped to ``box`` = (left, upper, right, lower): every coordinate moved into the box's frame and clamped
        to [0, w] / [0, h], the size (w, h) = (right - left, lower - upper) (bounding_box.py:167-193).  Empty boxes stay:
        ``clip_to_image`` drops them."""
        w, h = box[2] - box[0], box[3] - box[1]
        xmin, ymin, xmax, ymax = self.bbox.split(1, dim=-1)
        cropped = torch.cat(((xmin - box[0]).clamp(min=0, max=w), (ymin - box[1]).clamp(min=0, max=h),
                             (xmax - box[0]).clamp(min=0, max=w), (ymax - box[1]).clamp(min=0, max=h)), dim=-1)
        return self._fields_follow(BoxList(cropped, (w, h)), "crop", box)

    def __repr__(self):
        return f"BoxList(num_boxes={len(self)}, image_width={self.size[0]}, image_height={self.size[1]})"


class SampledBoxList(BoxList):
    """A proposal list as the box head's sampler hands it out (roi_heads.py::FastRCNNLossComputation.subsample_many), with
    what the sampler knows about its positives: ``pos_index`` int64 [npos], the rows whose label is > 0 (None: the
    tensor-op sampler made the list, ask ``nonzero``), ``all_positive``: every row is a positive, matched to the ground-truth
    box in its ``matched_gt`` field.  Takes bbox, size and fields from ``boxlist``.  Only ``to`` and ``map_tensors`` keep the
    type: indexing, ``copy_with_fields`` and ``cat_boxlist`` change the rows, so they yield a plain ``BoxList``."""

    _TENSORS = BoxList._TENSORS + ("pos_index",)

    def __init__(self, boxlist, pos_index=None, all_positive=False):
        super().__init__(boxlist.bbox, boxlist.size)
        self.extra_fields = dict(boxlist.extra_fields)
        self.pos_index, self.all_positive = pos_index, all_positive


class PastedMasks(TensorHolder):
    """Binary instance masks of one image that are DEFINED by per-instance probability maps and boxes through the
    Masker paste (mask_head/inference.py:100-160) -- the pseudo labels' masks (st_generalized_rcnn.py:266-271) -- kept in
    that form: the student's mask targets are computed from the maps directly (``_C.project_pasted_masks``), so the
    H x W canvases are only built when something asks for them (``materialize``).  probs [G, M, M], boxes [G, 4],
    image_size = (height, width)."""

    _TENSORS = ("probs", "boxes")

    def __init__(self, probs, boxes, image_size, threshold=0.5, padding=1):
        assert padding == 1, "the device kernel implements the reference's Masker(padding=1)"
        self.probs, self.boxes, self.image_size, self.threshold, self.padding = probs, boxes, tuple(image_size), threshold, padding

    def __len__(self):
        return self.probs.shape[0]

    def project(self, gt_index, boxes, resolution):
        """float32 [P, M, M] mask targets of ``boxes``, straight from the probability maps; host boxes (a device step
        replayed on the CPU): the pasted canvases through the tensor-op projection, the same bits."""
        from .. import _C
        if not boxes.is_cuda:
            from .roi_heads import project_masks_on_boxes
            return project_masks_on_boxes(self.materialize(), gt_index, boxes, resolution)
        return _C.project_pasted_masks(self.probs, self.boxes, gt_index, boxes, self.image_size, resolution, self.threshold)

    def materialize(self):
        """bool [G, H, W]: what Masker(threshold, padding) pastes."""
        from .roi_heads import Masker
        h, w = self.image_size
        return Masker(self.threshold, self.padding)(self.probs[:, None], BoxList(self.boxes, (w, h)))[:, 0]


class PolygonMasks(TensorHolder):
    """Polygon ground-truth masks of one image, the reference's ``SegmentationMask(polygons, size, mode='poly')``
    (structures/segmentation_mask.py:348-478 over PolygonInstance :208-347) in the flat form the device kernel reads:
    ``coords`` float32 [T] -- the (x, y) pairs of every polygon back to back --, ``polygon_start`` int32 [NP + 1] (offsets
    in floats) and ``instance_start`` int32 [G + 1] (polygon ranges of the G instances).  ``size`` = (width, height).
    Polygons with fewer than 3 vertices are dropped at construction, as ``PolygonInstance.__init__`` does.  The mask
    head's targets come from ``_C.project_polygon_masks`` (crop -> resize -> rasterise per positive, one launch);
    ``convert_to_binarymask`` rasterises whole-image masks at any image size (``_C.polygons_to_masks`` on the device,
    ``_cpu.polygons_to_masks`` on the host)."""

    _TENSORS = ("coords", "polygon_start", "instance_start")

    def __init__(self, instances, size):
        self.size = tuple(size)
        coords, pstart, istart = [], [0], [0]
        for polys in instances:
            for poly in polys:
                flat = [float(v) for v in (poly.tolist() if hasattr(poly, "tolist") else poly)]
                if len(flat) >= 6:  # 3 * 2 coordinates (segmentation_mask.py:227)
                    coords.extend(flat[: len(flat) // 2 * 2])
                    pstart.append(len(coords))
            istart.append(len(pstart) - 1)
        self.coords = torch.tensor(coords, dtype=torch.float32)
        self.polygon_start = torch.tensor(pstart, dtype=torch.int32)
        self.instance_start = torch.tensor(istart, dtype=torch.int32)

    def __len__(self):
        return self.instance_start.numel() - 1

    def project(self, gt_index, boxes, resolution):
        """float32 [P, M, M] mask targets of ``boxes``: crop + resize + rasterise every positive's polygons in one launch
        (csrc/polygons.hip), on the device ``boxes`` live on."""
        from .. import _C
        m = self if self.coords.device == boxes.device else self.to(boxes.device)
        return _C.project_polygon_masks(m.coords, m.polygon_start, m.instance_start, gt_index, boxes, m.size, resolution)

    def instances(self):
        """Back to the nested-list form: per instance a list of flat float32 polygons (host tensors)."""
        c, ps, ist = self.coords.cpu(), self.polygon_start.tolist(), self.instance_start.tolist()
        return [[c[ps[q]:ps[q + 1]] for q in range(ist[g], ist[g + 1])] for g in range(len(self))]

    def __getitem__(self, item):
        """Instances selected by an int, a slice, an index tensor or a boolean mask (SegmentationMask.__getitem__,
        segmentation_mask.py:437-458) -- re-packed on the host: ground-truth lists are a handful of instances."""
        inst = self.instances()
        if isinstance(item, int):
            picked = [inst[item]]
        elif isinstance(item, slice):
            picked = inst[item]
        else:
            item = torch.as_tensor(item).cpu()
            idx = torch.nonzero(item).squeeze(1).tolist() if item.dtype == torch.bool else item.reshape(-1).tolist()
            picked = [inst[i] for i in idx]
        return PolygonMasks(picked, self.size).to(self.coords.device)

    def transpose(self, method):
        """FLIP_LEFT_RIGHT (0) / FLIP_TOP_BOTTOM (1): segmentation_mask.py:250-268 (``dim - p - 1`` on one coordinate)."""
        if method not in (0, 1):
            raise NotImplementedError("Only FLIP_LEFT_RIGHT and FLIP_TOP_BOTTOM implemented")
        c = self.coords.clone()
        c[method::2] = self.size[method] - self.coords[method::2] - TO_REMOVE
        return self._with(coords=c)

    def resize(self, size):
        """Polygons scaled to ``size`` = (width, height): segmentation_mask.py:301-324 (one ratio when both axes agree)."""
        size = tuple(int(s) for s in size)
        ratios = tuple(float(s) / float(s_orig) for s, s_orig in zip(size, self.size))
        if ratios[0] == ratios[1]:
            c = self.coords * ratios[0]
        else:
            c = self.coords.clone()
            c[0::2] *= ratios[0]
            c[1::2] *= ratios[1]
        return self._with(coords=c, size=size)

    def crop(self, box):
        """Polygons moved into the frame of ``box`` = (xmin, ymin, xmax, ymax): PolygonInstance.crop
        (segmentation_mask.py:273-299) -- the box clamped to the current size (at least one pixel), xmin / ymin subtracted
        in float32, the vertices NOT clamped; the new size is the clamped (w, h)."""
        current_width, current_height = self.size
        xmin, ymin, xmax, ymax = map(float, box)
        if not (xmin <= xmax and ymin <= ymax):
            raise ValueError(f"PolygonMasks.crop: {tuple(box)}")
        xmin, ymin = min(max(xmin, 0), current_width - 1), min(max(ymin, 0), current_height - 1)
        xmax, ymax = min(max(xmax, 0), current_width), min(max(ymax, 0), current_height)
        xmax, ymax = max(xmax, xmin + 1), max(ymax, ymin + 1)
        c = self.coords.clone()
        c[0::2] = c[0::2] - xmin
        c[1::2] = c[1::2] - ymin
        # whole numbers as ints: the size goes to the rasteriser as the canvas
        size = tuple(int(v) if float(v).is_integer() else v for v in (xmax - xmin, ymax - ymin))
        return self._with(coords=c, size=size)

    def convert_to_binarymask(self):
        """uint8 [G, height, width]: every instance rasterised over the whole image (segmentation_mask.py:326-334)."""
        from .. import _C
        if not self.coords.is_cuda:  # host polygons (dataset side, MODEL.DEVICE cpu): any image size, libovis_cpu.so
            from .. import _cpu
            return _cpu.polygons_to_masks(self.coords, self.polygon_start, self.instance_start, self.size)
        return _C.polygons_to_masks(self.coords, self.polygon_start, self.instance_start, self.size)


class CopyPasteMasks(TensorHolder):
    """The ground-truth masks of an image that RECEIVES a copy-paste (data/transforms.py; include/ovis_hip.h states the
    rule), between the two halves of the input transform: ``polygons`` -- a ``PolygonMasks`` in the image's new frame
    holding its own instances first and the pasted ones behind them -- and ``num_own``, how many are its own; ``source``:
    the batch index the pasted ones come from.  The host half builds it, staging moves it like every holder, and the device
    half replaces it with the dense uint8 [G', h, w] masks that are left once the pasted objects cover the own ones.  It is
    never a mask target's source and has no geometry of its own: nothing resizes, flips or crops behind the host half."""

    _TENSORS = ("polygons",)

    def __init__(self, own, pasted, size, source):
        self.size, self.num_own, self.source = tuple(size), len(own), int(source)
        self.polygons = PolygonMasks(own.instances() + pasted.instances(), self.size)

    def __len__(self):
        return len(self.polygons)

    def _no(self, what):
        raise NotImplementedError(f"CopyPasteMasks.{what}: the holder lives between the host and the device half of the input "
                                  "transform; the device half turns it into dense masks (InputTransform.__call__)")

    def resize(self, size):
        self._no("resize")

    def transpose(self, method):
        self._no("transpose")

    def crop(self, box):
        self._no("crop")

    def project(self, gt_index, boxes, resolution):
        self._no("project")


class RleMasks(TensorHolder):
    """Bitmap (COCO RLE) ground-truth masks of one image, the reference's ``SegmentationMask(rles, size, mode='mask')``
    (``BinaryMaskList``, structures/segmentation_mask.py:33-158), kept LAZY: the encodings, the geometry that was asked
    for, and an instance index -- never a canvas.  The mask head's targets come straight from the decoded bit words
    (``_C.project_rle_masks``, csrc/rle_targets.hip), which evaluates resize -> flips -> crop -> resize per target pixel.

    ``items``: one per instance, as ``_C.coco_rle_words`` takes them -- compressed ``counts`` (``str`` / ``bytes``) or the
    uncompressed integer list; ``source_hw`` = the (height, width) every encoding has.  Host form (made in the loader
    worker, NumPy only): ``chars`` uint8 + ``char_offsets`` int64 [N + 1] (the strings back to back), ``runs`` int32 +
    ``run_offsets`` int64 [N + 1] (one slot per value of every item: the lists' values in place, the strings' slots are
    filled by the device decoder), ``sizes`` int32 [N, 2]; the number of values of a string is counted here -- its
    characters c with ((c - 48) & 0x20) == 0 -- so the device decode needs no host read.  ``size`` = (width, height) of the
    frame the masks are asked for in (``resize`` records it, ``transpose`` toggles the flips, both act after the decode,
    in the reference's order: resize, then flips; ``crop`` records one integer ``window`` of that frame behind them, and
    ``size`` becomes the window's); ``instance`` int64 [G]: the encoding behind each instance --
    ``__getitem__`` indexes it and repacks nothing.  ``decoded()`` adds ``words`` / ``word_offsets`` (device) and
    ``decoded_words_per_mask``, the words every slice was given.
    ``image_id`` / ``ann_ids`` name the masks in the error a malformed encoding raises."""

    _TENSORS = ("chars", "char_offsets", "runs", "run_offsets", "sizes", "instance", "words", "word_offsets")

    def __init__(self, items, source_hw, image_id=None, ann_ids=None):
        h0, w0 = int(source_hw[0]), int(source_hw[1])
        if h0 < 1 or w0 < 1 or h0 * w0 > 0x7fffffef:
            raise ValueError(f"RleMasks: source size {h0} x {w0} is outside what the decoder takes")
        texts, lists = [], []
        for k, item in enumerate(items):
            if isinstance(item, str):
                texts.append(item.encode("latin-1", "replace"))  # beyond a byte: '?', which the decoder refuses
                lists.append(None)
            elif isinstance(item, (bytes, bytearray)):
                texts.append(bytes(item))
                lists.append(None)
            else:
                values = np.asarray(item).reshape(-1)
                if values.dtype.kind not in "iu":
                    raise ValueError(f"RleMasks: item {k} is neither a string nor a sequence of integers")
                texts.append(b"")
                lists.append(np.clip(values.astype(np.int64), -2 ** 31, 2 ** 31 - 1).astype(np.int32))
        n = len(texts)
        chars = np.frombuffer(b"".join(texts), dtype=np.uint8)
        char_offsets = np.zeros(n + 1, dtype=np.int64)
        np.cumsum([len(t) for t in texts], out=char_offsets[1:])
        ends = ((chars.astype(np.int32) - 48) & 0x20) == 0  # a value ends at such a character
        ends_before = np.concatenate(([0], np.cumsum(ends, dtype=np.int64)))
        counts = ends_before[char_offsets[1:]] - ends_before[char_offsets[:-1]]
        counts = counts + np.array([0 if v is None else len(v) for v in lists], dtype=np.int64)
        run_offsets = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(counts, out=run_offsets[1:])
        runs = np.zeros(int(run_offsets[-1]), dtype=np.int32)
        for k, v in enumerate(lists):
            if v is not None:
                runs[run_offsets[k]:run_offsets[k + 1]] = v
        self.chars, self.char_offsets = torch.from_numpy(chars.copy()), torch.from_numpy(char_offsets)
        self.runs, self.run_offsets = torch.from_numpy(runs), torch.from_numpy(run_offsets)
        self.sizes = torch.tensor([[h0, w0]] * n, dtype=torch.int32).reshape(n, 2)
        self.instance = torch.arange(n, dtype=torch.int64)
        self.words = self.word_offsets = self.decoded_words_per_mask = None
        self.num_chars, self.num_runs, self.num_items = int(char_offsets[-1]), int(run_offsets[-1]), n
        self.source_hw, self.size = (h0, w0), (w0, h0)
        self.flip_h = self.flip_v = False
        self.window = self.frame_size = None  # ``crop``: one window behind the resize and the flips
        self.image_id = image_id
        self.ann_ids = list(ann_ids) if ann_ids is not None else list(range(n))

    @property
    def words_per_mask(self):
        return (self.source_hw[0] * self.source_hw[1] + 63) // 64

    def __len__(self):
        return self.instance.numel()

    def project(self, gt_index, boxes, resolution):
        """float32 [P, M, M] mask targets of ``boxes``: the decoded bit words tested per target pixel in one launch
        (csrc/rle_targets.hip), on the device ``boxes`` live on."""
        from .. import _C
        if not boxes.is_cuda:
            raise NotImplementedError("RLE ground-truth masks under MODEL.DEVICE cpu are not supported: the decoder and "
                                      "the target kernel are device code; train on the GPU or use polygon ground truth")
        m = self if self.instance.device == boxes.device else self.to(boxes.device)
        return _C.project_rle_masks(m, gt_index, boxes, resolution)

    def __getitem__(self, item):
        """Instances selected by an int, a slice, an index tensor or a boolean mask: the instance index is indexed, the
        encodings and the words stay as they are."""
        if isinstance(item, int):
            item = slice(item, item + 1) if item != -1 else slice(item, None)
        elif not isinstance(item, slice):
            item = torch.as_tensor(item, device=self.instance.device)
            if item.dtype == torch.bool:
                item = torch.nonzero(item).squeeze(1)
            item = item.reshape(-1)
        return self._with(instance=self.instance[item])

    def resize(self, size):
        """Records ``size`` = (width, height) as the frame the masks are resampled to (BinaryMaskList.resize,
        segmentation_mask.py:138-156).  One resize, in front of the flips: that is the chain the kernel evaluates."""
        size = tuple(int(s) for s in size)
        if self.window is not None:
            raise NotImplementedError("RleMasks.resize: a resize behind a crop is not the chain the kernel evaluates")
        if size == self.size:
            return self._with()
        if self.size != (self.source_hw[1], self.source_hw[0]):
            raise NotImplementedError(f"RleMasks.resize: already resized to {self.size}; a second resize to {size} would be "
                                      "a resample of a resample")
        if self.flip_h or self.flip_v:
            raise NotImplementedError("RleMasks.resize: a resize behind a flip is not the chain the kernel evaluates")
        if size[0] < 1 or size[1] < 1:
            raise ValueError(f"RleMasks.resize: {size}")
        return self._with(size=size)

    def transpose(self, method):
        """FLIP_LEFT_RIGHT (0) / FLIP_TOP_BOTTOM (1): segmentation_mask.py:113-116."""
        if method not in (0, 1):
            raise NotImplementedError("Only FLIP_LEFT_RIGHT and FLIP_TOP_BOTTOM implemented")
        if self.window is not None:
            raise NotImplementedError("RleMasks.transpose: a flip behind a crop is not the chain the kernel evaluates")
        return self._with(flip_h=not self.flip_h) if method == 0 else self._with(flip_v=not self.flip_v)

    def crop(self, box):
        """Records ONE integer window, applied behind the recorded resize and flips: ``box`` = (xmin, ymin, xmax, ymax)
        rounded and clamped as BinaryMaskList.crop does (segmentation_mask.py:118-136: python round, inside the frame, at
        least one pixel).  ``window`` = (win_x, win_y, win_w, win_h) of ``frame_size``, the (width, height) before the crop;
        ``size`` becomes (win_w, win_h).  ``project`` then evaluates decode -> resize -> flips -> the window -> the box crop
        -> resize (``ovis_project_rle_masks_window_f32``).  A second crop raises, as a resize or a flip behind one does."""
        if self.window is not None:
            raise NotImplementedError("RleMasks.crop: already cropped; a second crop is not the chain the kernel evaluates")
        current_width, current_height = self.size
        xmin, ymin, xmax, ymax = [round(float(b)) for b in box]
        if not (xmin <= xmax and ymin <= ymax):
            raise ValueError(f"RleMasks.crop: {tuple(box)}")
        xmin, ymin = min(max(xmin, 0), current_width - 1), min(max(ymin, 0), current_height - 1)
        xmax, ymax = min(max(xmax, 0), current_width), min(max(ymax, 0), current_height)
        xmax, ymax = max(xmax, xmin + 1), max(ymax, ymin + 1)
        return self._with(window=(xmin, ymin, xmax - xmin, ymax - ymin), frame_size=self.size, size=(xmax - xmin, ymax - ymin))

    def names(self):
        """What every encoding is, for an error message."""
        return [f"image {self.image_id}: annotation {a}" for a in self.ann_ids]

    @staticmethod
    def decode_many(masks):
        """ONE ``_C.coco_rle_words_staged`` call for all the (device-resident) ``RleMasks`` of a batch: every structure gets
        its ``words`` / ``word_offsets`` (absolute offsets into the call's shared word buffer).  Sizes and value counts are
        the host's, so nothing is read back.  -> (status int32 [total] on the device, names: one string per encoding), or
        (None, []) when there is nothing to decode."""
        from .. import _C
        masks = [m for m in masks if m.num_items > 0 and m.words is None]
        if not masks:
            return None, []
        dev = masks[0].chars.device
        chars_at = runs_at = words_at = 0
        char_offsets, run_offsets, word_offsets, names = [], [], [], []
        for m in masks:
            char_offsets.append(m.char_offsets[:-1] + chars_at)
            run_offsets.append(m.run_offsets[:-1] + runs_at)
            m_words = torch.arange(m.num_items + 1, dtype=torch.int64, device=dev) * m.words_per_mask + words_at
            word_offsets.append(m_words)
            chars_at, runs_at, words_at = chars_at + m.num_chars, runs_at + m.num_runs, words_at + m.num_items * m.words_per_mask
            names += m.names()
        char_offsets.append(torch.full((1,), chars_at, dtype=torch.int64, device=dev))
        run_offsets.append(torch.full((1,), runs_at, dtype=torch.int64, device=dev))
        all_word_offsets = torch.cat([w[:-1] for w in word_offsets] + [torch.full((1,), words_at, dtype=torch.int64, device=dev)])
        words, _, status = _C.coco_rle_words_staged(
            torch.cat([m.chars for m in masks]), torch.cat(char_offsets), torch.cat([m.runs for m in masks]),
            torch.cat(run_offsets), torch.cat([m.sizes for m in masks]), all_word_offsets, total_words=words_at,
            max_words=max(m.words_per_mask for m in masks), compressed=chars_at > 0)
        for m, w in zip(masks, word_offsets):
            m.words, m.word_offsets, m.decoded_words_per_mask = words, w, m.words_per_mask
        return status, names

    def decoded(self):
        """This structure with ``words`` / ``word_offsets`` on the device.  Already decoded (the input transform decodes a
        batch in one call and checks it without a synchronisation): itself.  Else it decodes alone and CHECKS -- one host
        read; a malformed encoding raises ValueError."""
        if self.words is not None or self.num_items == 0:
            return self
        if not self.chars.is_cuda:
            raise NotImplementedError("RleMasks.decoded: the RLE decoder is a device kernel; move the masks to the GPU first "
                                      "(RLE ground truth under MODEL.DEVICE cpu is not supported)")
        status, names = RleMasks.decode_many([self])
        raise_on_bad_rle(status.cpu(), names)
        return self


def raise_on_bad_rle(status, names):
    """ValueError naming the first malformed encoding of a decoded batch (``status``: host int32, one per name)."""
    from .. import _C
    bad = torch.nonzero(status).reshape(-1).tolist()
    if bad:
        k = bad[0]
        raise ValueError(f"{names[k]}: malformed RLE segmentation: {_C.COCO_RLE_STATUS.get(int(status[k]), int(status[k]))}"
                         + (f" (and {len(bad) - 1} more)" if len(bad) > 1 else ""))


def cat_boxlist(boxlists):  # boxlist_ops.py:107-129
    size = boxlists[0].size
    fields = set(boxlists[0].fields())
    assert all(b.size == size and set(b.fields()) == fields for b in boxlists)
    out = BoxList(torch.cat([b.bbox for b in boxlists], 0), size)
    for f in fields:
        out.add_field(f, torch.cat([b.get_field(f) for b in boxlists], 0))
    return out


def box_iou(a, b):
    """IoU matrix [len(a), len(b)] of two xyxy tensors (boxlist_ops.py:53-89)."""
    area_a = (a[:, 2] - a[:, 0] + TO_REMOVE) * (a[:, 3] - a[:, 1] + TO_REMOVE)
    area_b = (b[:, 2] - b[:, 0] + TO_REMOVE) * (b[:, 3] - b[:, 1] + TO_REMOVE)
    lt = torch.max(a[:, None, :2], b[:, :2])
    rb = torch.min(a[:, None, 2:], b[:, 2:])
    wh = (rb - lt + TO_REMOVE).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area_a[:, None] + area_b - inter)


def boxlist_iou(boxlist1, boxlist2):
    if boxlist1.size != boxlist2.size:
        raise RuntimeError(f"boxlists should have same image size, got {boxlist1}, {boxlist2}")
    return box_iou(boxlist1.bbox, boxlist2.bbox)


def boxlist_nms(boxlist, nms_thresh, max_proposals=-1, score_field="scores"):  # boxlist_ops.py:9-31
    if nms_thresh <= 0:
        return boxlist
    keep = _nms(boxlist.bbox, boxlist.get_field(score_field), nms_thresh)
    if max_proposals > 0:
        keep = keep[:max_proposals]
    return boxlist[keep.to(boxlist.bbox.device)]


def remove_small_boxes(boxlist, min_size):  # boxlist_ops.py:34-49
    b = boxlist.bbox
    ws = b[:, 2] - b[:, 0] + TO_REMOVE
    hs = b[:, 3] - b[:, 1] + TO_REMOVE
    return boxlist[(ws >= min_size) & (hs >= min_size)]


class ImageList(TensorHolder):
    """Batched images padded to a common size (image_list.py:7-72)."""

    _TENSORS = ("tensors",)  # the padded batch to_image_list allocates

    def __init__(self, tensors, image_sizes):
        self.tensors = tensors
        self.image_sizes = list(image_sizes)  # (height, width) per image


def to_image_list(tensors, size_divisible=0):
    if isinstance(tensors, ImageList):
        return tensors
    if torch.is_tensor(tensors):
        if tensors.dim() == 3:
            tensors = tensors[None]
        return ImageList(tensors, [tuple(t.shape[-2:]) for t in tensors])
    max_size = [max(s) for s in zip(*[img.shape for img in tensors])]
    if size_divisible > 0:
        import math

        max_size[1] = int(math.ceil(max_size[1] / size_divisible) * size_divisible)
        max_size[2] = int(math.ceil(max_size[2] / size_divisible) * size_divisible)
    batched = tensors[0].new_zeros((len(tensors), *max_size))
    for img, pad in zip(tensors, batched):
        pad[: img.shape[0], : img.shape[1], : img.shape[2]].copy_(img)
    return ImageList(batched, [tuple(im.shape[-2:]) for im in tensors])
