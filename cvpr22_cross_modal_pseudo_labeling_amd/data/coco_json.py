"""The slice of ``pycocotools.coco.COCO`` the dataset classes use, over plain ``json`` (pycocotools is not a dependency):
images by id, annotations by image id in FILE order (``getAnnIds(imgIds=i)`` + ``loadAnns``), the category ids sorted
(``getCatIds``).  A captions file (``annotations`` of ``{"image_id", "caption"}``) is indexed by the same class.
"""
import json


class COCOIndex:
    def __init__(self, ann_file):
        with open(ann_file) as f:
            self.dataset = json.load(f)
        if not isinstance(self.dataset, dict):
            raise ValueError(f"{ann_file}: a COCO-format file is a JSON object, got {type(self.dataset).__name__}")
        self.ann_file = ann_file
        self.imgs = {img["id"]: img for img in self.dataset.get("images", [])}
        self.cats = {cat["id"]: cat for cat in self.dataset.get("categories", [])}
        self._anns = {}
        for ann in self.dataset.get("annotations", []):
            self._anns.setdefault(ann["image_id"], []).append(ann)

    def img_ids(self):
        return list(self.imgs)

    def cat_ids(self):
        return sorted(self.cats)

    def anns(self, img_id):
        """The annotations of one image, in file order (crowd ones included)."""
        return self._anns.get(img_id, [])
