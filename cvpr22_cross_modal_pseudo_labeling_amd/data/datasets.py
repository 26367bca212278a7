"""COCO-format datasets for the raw input path: ``COCODataset`` (maskrcnn_benchmark/data/datasets/coco.py:42-140) and
``COCOCapDetDataset`` (datasets/coco_cap_det.py:55-188) over the pycocotools-free index of data/coco_json.py.

An item is what ``data.synthetic.make_raw_batch`` fakes: ``(image uint8 [h, w, 3] RGB numpy array, BoxList, idx)`` with
polygon ground truth (``PolygonMasks``) or, for an image whose non-crowd annotations are all RLE (compressed or not),
bitmap ground truth (``RleMasks``: packed here, decoded on the device).  No transform runs here: the loader's collate
function applies the host half of data/transforms.py to the whole batch (data/build.py) and the device half makes the
pixels and decodes the RLE masks.  Polygons and RLE mixed within one image, an RLE of another size than its image and
keypoints are not supported: they raise, naming the image and the annotation.
"""
import os

import numpy as np
import torch
from PIL import Image

from ..modeling.language_backbone import normalize_class_names
from ..modeling.structures import BoxList, PolygonMasks, RleMasks
from .caption_parser import CaptionParser
from .coco_json import COCOIndex


def has_valid_annotation(anno):
    """coco.py:24-39 without the keypoint branch: at least one annotation, and not every box <= 1 pixel wide or high."""
    return len(anno) > 0 and not all(any(o <= 1 for o in obj["bbox"][2:]) for obj in anno)


class COCODataset(torch.utils.data.Dataset):
    remove_empty = True  # clip_to_image(remove_empty=...) of __getitem__ (coco.py:130)

    def __init__(self, ann_file, root, remove_images_without_annotations, extra_args=None):
        self.coco = COCOIndex(ann_file)
        self.root = root
        self.ids = sorted(self.coco.img_ids())
        if remove_images_without_annotations:
            self.ids = [i for i in self.ids if has_valid_annotation(self.coco.anns(i))]
        self.categories = {cat["id"]: cat["name"] for cat in self.coco.cats.values()}
        self.json_category_id_to_contiguous_id = {v: i + 1 for i, v in enumerate(self.coco.cat_ids())}
        self.contiguous_category_id_to_json_id = {v: k for k, v in self.json_category_id_to_contiguous_id.items()}
        self.id_to_img_map = dict(enumerate(self.ids))

        self.class_splits = {}
        if extra_args is not None and extra_args.get("LOAD_EMBEDDINGS", False):
            embeddings = {}
            for item in self.coco.dataset["categories"]:
                if "embedding" not in item or extra_args["EMB_KEY"] not in item["embedding"]:
                    raise KeyError(f"{ann_file}: category {item['id']} has no embedding '{extra_args['EMB_KEY']}' "
                                   "(DATASETS.DATASET_ARGS.LOAD_EMBEDDINGS is set)")
                embeddings[item["id"]] = np.asarray(item["embedding"][extra_args["EMB_KEY"]], dtype=np.float32)
                if "split" in item:
                    self.class_splits.setdefault(item["split"], []).append(item["id"])
            mtx = np.zeros((len(self.contiguous_category_id_to_json_id) + 1, extra_args["EMB_DIM"]), dtype=np.float32)
            for i, cid in self.contiguous_category_id_to_json_id.items():
                mtx[i, :] = embeddings[cid]
            self.class_emb_mtx = torch.from_numpy(mtx)  # row 0, the background, stays zero

        class_names = [""] * (len(self.categories) + 1)
        for json_id, name in self.categories.items():
            class_names[self.json_category_id_to_contiguous_id[json_id]] = name
        class_names[0] = "bg"
        self.class_names = normalize_class_names(class_names)

    def __len__(self):
        return len(self.ids)

    def _open(self, idx):
        with Image.open(os.path.join(self.root, self.coco.imgs[self.ids[idx]]["file_name"])) as f:
            return f.convert("RGB")

    def original_image(self, idx):
        """The decoded image of dataset index ``idx`` at its own size, before any transform: RGB uint8 [h, w, 3]."""
        return np.array(self._open(idx))

    def _load(self, idx):
        """-> (image id, RGB uint8 [h, w, 3], the non-crowd annotations, the BoxList with labels and masks, unclipped)."""
        img_id = self.ids[idx]
        img = self._open(idx)
        anno = [obj for obj in self.coco.anns(img_id) if obj["iscrowd"] == 0]
        boxes = torch.as_tensor([obj["bbox"] for obj in anno], dtype=torch.float32).reshape(-1, 4)  # guards against no boxes
        target = BoxList(boxes, img.size, mode="xywh")
        target.add_field("labels", torch.tensor([self.json_category_id_to_contiguous_id[obj["category_id"]] for obj in anno],
                                                dtype=torch.int64))
        return img_id, img, anno, target

    def _add_masks(self, target, anno, img_id):
        if anno and "segmentation" in anno[0]:
            rle = [isinstance(obj["segmentation"], dict) for obj in anno]
            if not any(rle):
                target.add_field("masks", PolygonMasks([obj["segmentation"] for obj in anno], target.size))
                return
            width, height = target.size
            for obj, is_rle in zip(anno, rle):
                if not is_rle:
                    raise ValueError(f"image {img_id}: annotation {obj.get('id')} has polygons beside the RLE segmentations "
                                     "of the image's other annotations; one kind per image is supported")
                if [int(v) for v in obj["segmentation"].get("size", ())] != [height, width]:
                    raise ValueError(f"image {img_id}: annotation {obj.get('id')} has an RLE segmentation of size "
                                     f"{obj['segmentation'].get('size')}, the image is [{height}, {width}] (height, width)")
            target.add_field("masks", RleMasks([obj["segmentation"]["counts"] for obj in anno], (height, width), image_id=img_id,
                                               ann_ids=[obj.get("id") for obj in anno]))

    def __getitem__(self, idx):
        img_id, img, anno, target = self._load(idx)
        self._add_masks(target, anno, img_id)
        return np.array(img), target.clip_to_image(remove_empty=self.remove_empty), idx

    def get_img_info(self, index):
        return self.coco.imgs[self.id_to_img_map[index]]


class COCOCapDetDataset(COCODataset):
    """Detection ground truth plus the image's captions and their nouns as caption-vocabulary ids.  ``vocab_file``: the
    LVIS-format categories JSON of data/caption_parser.py; ``lemmatize``: its lemmatiser (None: spaCy when loadable, else
    whitespace tokens -- NOT the reference's lemmatisation).  A caption annotation that carries ``"ids_cap"`` (a list of
    0-based vocabulary ids, optionally ``"nn_caption"``: their noun strings) gives the image's nouns as they are -- the first
    such annotation of the image wins over parsing, so the reference's exact nouns can be baked into the file offline."""

    remove_empty = False  # coco_cap_det.py:178

    def __init__(self, ann_file, ann_file_cap, root, remove_images_without_annotations, extra_args=None, vocab_file=None,
                 lemmatize=None):
        super().__init__(ann_file, root, remove_images_without_annotations, extra_args)
        self.coco_cap = COCOIndex(ann_file_cap)
        self.parser = CaptionParser.from_file(vocab_file, lemmatize) if vocab_file else None

    def _nouns(self, img_id, captions):
        for cap in captions:
            if "ids_cap" in cap:
                ids = [int(i) for i in cap["ids_cap"]]
                if "nn_caption" in cap:
                    return list(cap["nn_caption"]), ids
                return [self.parser.class_names[i] if self.parser else str(i) for i in ids], ids
        if self.parser is None:
            if not captions:
                return [], []
            raise ValueError(f"image {img_id}: its captions carry no precomputed 'ids_cap' and the dataset has no "
                             "'vocab_file' to parse them with")
        return self.parser.extract_obj([cap["caption"] for cap in captions])

    def __getitem__(self, idx):
        img_id, img, anno, target = self._load(idx)
        captions = self.coco_cap.anns(img_id)
        nns_cap, ids_cap = self._nouns(img_id, captions)
        target.add_field("caption", "/".join(cap["caption"] for cap in captions))
        target.add_field("nn_caption", "/".join(nns_cap))
        target.add_field("ids_cap", torch.tensor(ids_cap, dtype=torch.int64))
        target.add_field("dataset_name", "MSCOCO")
        target.add_field("is_det", "Yes")
        self._add_masks(target, anno, img_id)
        return np.array(img), target.clip_to_image(remove_empty=self.remove_empty), idx
