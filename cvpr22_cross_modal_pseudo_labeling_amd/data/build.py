"""Datasets -> batches in the forms the raw input path takes (maskrcnn_benchmark/data/build.py:18-192 and
collate_batch.py, for this package's split transform).

A training batch is ``(raw, targets)`` -- exactly what ``data.synthetic.RawSyntheticBatches`` yields: the HOST half of
data/transforms.py over the collated items, made in the loader worker; ``DevicePrefetcher(loader, device,
transform=transform)`` stages it and makes the pixels on the device.  An evaluation batch is ``(raw, None, dataset
indices)``; behind the same prefetcher it is the ``(ImageList, None, ids)`` of ``data.synthetic.raw_test_batches``.

Worker processes decode, decide and pack: they return host tensors only and never open the device.  ``raw["loader"]``
reports, per batch, its dataset indices, the worker that made it and whether that process had the GPU initialised.
"""
import bisect
import random

import torch
import torch.utils.data

from . import samplers
from .datasets import COCOCapDetDataset, COCODataset

_WORKER = {"cuda_initialized": False}


def _worker_init(worker_id):
    torch.set_num_threads(1)  # NUM_WORKERS single-threaded decoders, not NUM_WORKERS teams as wide as the machine
    _WORKER["cuda_initialized"] = torch.cuda.is_initialized()


def _loader_report(idx):
    info = torch.utils.data.get_worker_info()
    return {"indices": [int(i) for i in idx], "worker": None if info is None else info.id,
            "cuda_initialized": _WORKER["cuda_initialized"] or torch.cuda.is_initialized()}


def batch_seed(seed, rank, first_index, epoch=0):
    """The seed of a training batch's random draws (size choice, flips): a function of the run's seed, the rank, the
    batch's first dataset index and the epoch (the iteration its pass over the data began at, what ``set_epoch`` got) --
    not of the worker that happens to make the batch.  With the epoch in it an image draws anew in every pass, also when it
    leads its batch every time (one image per GPU)."""
    return ((int(seed) * 1000003 + int(rank)) * 1000003 + int(epoch)) * 1000003 + int(first_index)


class EpochItems(torch.utils.data.Dataset):
    """``dataset`` addressed by ``(index, epoch)``: the epoch of the pass rides along with the item to the collate function,
    whichever worker process fetches it."""

    def __init__(self, dataset):
        self.dataset = dataset

    def __len__(self):
        return len(self.dataset)

    def __getitem__(self, key):
        idx, epoch = key
        return self.dataset[idx] + (epoch,)


class EpochBatches(torch.utils.data.Sampler):
    """The index batches of ``batch_sampler``, every index paired with the epoch ``sampler`` is in when the batch is drawn."""

    def __init__(self, batch_sampler, sampler):
        self.batch_sampler, self.sampler = batch_sampler, sampler

    def __iter__(self):
        for batch in self.batch_sampler:
            yield [(i, self.sampler.epoch) for i in batch]

    def __len__(self):
        return len(self.batch_sampler)


class TrainCollator:
    def __init__(self, transform, seed=0, rank=0):
        self.transform, self.seed, self.rank = transform, seed, rank

    def __call__(self, batch):
        images, targets, idx, epochs = zip(*batch)
        rng = random.Random(batch_seed(self.seed, self.rank, idx[0], epochs[0]))
        raw, targets = self.transform.host(list(images), list(targets), rng=rng)
        raw["loader"] = dict(_loader_report(idx), epoch=int(epochs[0]))
        return raw, targets


class EvalCollator:
    def __init__(self, transform):
        self.transform = transform

    def __call__(self, batch):
        images, _, idx = zip(*batch)
        raw, _ = self.transform.host(list(images))
        raw["loader"] = _loader_report(idx)
        return raw, None, [int(i) for i in idx]


def build_dataset(cfg, name, catalog):
    """The dataset of one catalog name.  As in the reference, a ``COCODataset`` drops the images without a usable
    annotation (build.py:44-45) and a ``COCOCapDetDataset`` keeps every image (paths_catalog.py:285-296)."""
    entry = catalog.get(name)
    args = cfg.DATASETS.DATASET_ARGS
    if "ann_file_cap" in entry:
        return COCOCapDetDataset(entry["ann_file"], entry["ann_file_cap"], entry["img_dir"], False, extra_args=args,
                                 vocab_file=entry.get("vocab_file"))
    return COCODataset(entry["ann_file"], entry["img_dir"], True, extra_args=args)


def build_train_dataset(cfg, catalog):
    names = tuple(cfg.DATASETS.TRAIN)
    if len(names) != 1:
        raise NotImplementedError(f"DATASETS.TRAIN {names}: exactly one training set is supported (no ConcatDataset)")
    return build_dataset(cfg, names[0], catalog)


def aspect_group_ids(dataset, bins=(1,)):
    """build.py:76-89: the bin of height / width of every image, from ``get_img_info``."""
    bins = sorted(bins)
    out = []
    for i in range(len(dataset)):
        info = dataset.get_img_info(i)
        out.append(bisect.bisect_right(bins, float(info["height"]) / float(info["width"])))
    return out


def make_batch_sampler(dataset, sampler, aspect_grouping, images_per_batch, num_iters=None, start_iter=0, drop_last=False):
    if aspect_grouping:
        batch_sampler = samplers.GroupedBatchSampler(sampler, aspect_group_ids(dataset), images_per_batch, drop_uneven=drop_last)
    else:
        batch_sampler = torch.utils.data.sampler.BatchSampler(sampler, images_per_batch, drop_last=drop_last)
    if num_iters is not None:
        batch_sampler = samplers.IterationBasedBatchSampler(batch_sampler, num_iters, start_iter)
    return batch_sampler


def make_data_loader(cfg, dataset, transform, is_train, rank, world, start_iter=0, num_workers=None, seed=0, max_iter=None):
    """``torch.utils.data.DataLoader`` over ``dataset`` for rank ``rank`` of ``world``.

    Training: shuffled per epoch (seeded by the iteration the epoch starts at, the same on every rank), sharded, grouped
    by aspect ratio when DATALOADER.ASPECT_RATIO_GROUPING, SOLVER.IMS_PER_BATCH // world images per batch, batches until
    iteration ``max_iter`` (SOLVER.MAX_ITER) counted from ``start_iter``; yields ``(raw, targets)``.  A batch's draws are
    seeded by ``batch_seed(seed, rank, its first index, the epoch)``: NUM_WORKERS 0 and N give the same batches in the same
    order, and every pass over the data draws anew.  DATALOADER.DROP_LAST is not a key of this config tree: short batches
    are kept, the reference's default.
    Evaluation: in index order, sharded in contiguous slices, TEST.IMS_PER_BATCH // world per batch; yields ``(raw, None,
    dataset indices)``.  The last rank's slice may wrap around to index 0 to even the shares out: the detections are
    merged by index, so an image predicted twice is kept once."""
    if is_train:
        images_per_batch = cfg.SOLVER.IMS_PER_BATCH
        if images_per_batch % world != 0:
            raise ValueError("SOLVER.IMS_PER_BATCH ({}) must be divisible by the number of GPUs ({}) used.".format(
                images_per_batch, world))
        shuffle, num_iters = True, (cfg.SOLVER.MAX_ITER if max_iter is None else max_iter)
        collate = TrainCollator(transform, seed, rank)
    else:
        images_per_batch = cfg.TEST.IMS_PER_BATCH
        if images_per_batch % world != 0:
            raise ValueError("TEST.IMS_PER_BATCH ({}) must be divisible by the number of GPUs ({}) used.".format(
                images_per_batch, world))
        shuffle, num_iters, start_iter = False, None, 0
        collate = EvalCollator(transform)
    if len(dataset) == 0:
        raise ValueError("the dataset has no images (after dropping those without a usable annotation)")
    sampler = samplers.DistributedSampler(len(dataset), world, rank, shuffle=shuffle)
    batch_sampler = make_batch_sampler(dataset, sampler, cfg.DATALOADER.ASPECT_RATIO_GROUPING, images_per_batch // world,
                                       num_iters, start_iter)
    num_workers = cfg.DATALOADER.NUM_WORKERS if num_workers is None else num_workers
    if is_train:
        dataset, batch_sampler = EpochItems(dataset), EpochBatches(batch_sampler, sampler)
    return torch.utils.data.DataLoader(dataset, num_workers=num_workers, batch_sampler=batch_sampler, collate_fn=collate,
                                       worker_init_fn=_worker_init)
