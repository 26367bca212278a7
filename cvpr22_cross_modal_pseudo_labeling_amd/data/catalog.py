"""Dataset names -> files.  The reference resolves ``DATASETS.TRAIN / TEST`` names through a python module
(maskrcnn_benchmark/config/paths_catalog.py); here the catalog is a JSON file of settings:

    {name: {"img_dir": ..., "ann_file": ..., "ann_file_cap": optional, "vocab_file": optional}}

``ann_file_cap`` (the captions file) makes the entry a ``COCOCapDetDataset``, otherwise it is a ``COCODataset``;
``vocab_file`` is the caption vocabulary of data/caption_parser.py.  Relative paths are taken from ``data_dir``.
configs/dataset_catalog.example.json lists the names the shipped yaml files use.
"""
import json
import os

PATH_KEYS = ("img_dir", "ann_file", "ann_file_cap", "vocab_file")


class DatasetCatalog:
    def __init__(self, catalog_file, data_dir=""):
        if not os.path.isfile(catalog_file):
            raise FileNotFoundError(f"dataset catalog '{catalog_file}' does not exist")
        with open(catalog_file) as f:
            self.entries = json.load(f)
        self.catalog_file, self.data_dir = catalog_file, data_dir or ""

    def get(self, name):
        """The entry of ``name`` with its paths resolved; an unknown name or a missing file raises, naming it."""
        if name not in self.entries:
            raise KeyError(f"dataset '{name}' is not in the catalog {self.catalog_file} (it has: {sorted(self.entries)})")
        entry = dict(self.entries[name])
        for key in ("img_dir", "ann_file"):
            if key not in entry:
                raise KeyError(f"dataset '{name}' in {self.catalog_file} has no '{key}'")
        for key in PATH_KEYS:
            if key in entry:
                entry[key] = os.path.join(self.data_dir, entry[key])
                exists = os.path.isdir(entry[key]) if key == "img_dir" else os.path.isfile(entry[key])
                if not exists:
                    raise FileNotFoundError(f"dataset '{name}': {key} '{entry[key]}' does not exist")
        return entry
