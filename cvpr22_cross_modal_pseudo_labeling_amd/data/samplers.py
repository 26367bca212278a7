"""The reference's index samplers (maskrcnn_benchmark/data/samplers/distributed.py, grouped_batch_sampler.py,
iteration_based_batch_sampler.py), restated: the index batches of every rank are the reference's own
(tests/test_samplers_vs_reference.py holds them to a recording of its classes).  Rank and world size are ARGUMENTS -- no
process group is needed, so loader workers and tests build them freely.
"""
import math

import torch
from torch.utils.data.sampler import Sampler


class DistributedSampler(Sampler):
    """This rank's share of ``range(n)``: the epoch-seeded ``torch.randperm`` (or the identity), padded to a multiple of
    the world size by wrapping around to its own start, cut into one contiguous slice per rank."""

    def __init__(self, n, num_replicas, rank, shuffle=True):
        if not 0 <= rank < num_replicas:
            raise ValueError(f"rank {rank} is outside a world of {num_replicas}")
        self.n, self.num_replicas, self.rank, self.shuffle = int(n), int(num_replicas), int(rank), bool(shuffle)
        self.epoch = 0
        self.num_samples = int(math.ceil(self.n / self.num_replicas))
        self.total_size = self.num_samples * self.num_replicas

    def __iter__(self):
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.epoch)
            indices = torch.randperm(self.n, generator=g).tolist()
        else:
            indices = list(range(self.n))
        indices += indices[: self.total_size - self.n]
        return iter(indices[self.num_samples * self.rank: self.num_samples * (self.rank + 1)])

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch):
        self.epoch = epoch


class GroupedBatchSampler(Sampler):
    """Batches of ``batch_size`` indices that share a group id (the aspect-ratio bin).  Within a group the sampler's order
    is kept; the batches of all groups are then ordered by where their FIRST element stands in the sampler's order.
    ``drop_uneven`` drops the batches that came out short."""

    def __init__(self, sampler, group_ids, batch_size, drop_uneven=False):
        self.sampler, self.group_ids = sampler, [int(g) for g in group_ids]
        self.batch_size, self.drop_uneven = int(batch_size), bool(drop_uneven)
        self._batches, self._reuse = None, False

    def _prepare_batches(self):
        position = {}  # dataset index -> its (last) position in this pass of the sampler
        for p, i in enumerate(self.sampler):
            position[i] = p
        by_group = {}
        for i in sorted(position, key=position.get):
            by_group.setdefault(self.group_ids[i], []).append(i)
        batches = []
        for g in sorted(by_group):
            members = by_group[g]
            batches.extend(members[k:k + self.batch_size] for k in range(0, len(members), self.batch_size))
        batches.sort(key=lambda b: position[b[0]])
        if self.drop_uneven:
            batches = [b for b in batches if len(b) == self.batch_size]
        return batches

    def __iter__(self):
        # a ``len()`` BEFORE the first pass had to run the sampler to know the count: that pass yields those batches
        if not self._reuse:
            self._batches = self._prepare_batches()
        self._reuse = False
        return iter(self._batches)

    def __len__(self):
        """The number of batches of the latest pass (of the coming one before the first)."""
        if self._batches is None:
            self._batches, self._reuse = self._prepare_batches(), True
        return len(self._batches)


class IterationBasedBatchSampler(Sampler):
    """Passes through ``batch_sampler`` again and again until ``num_iterations`` batches were counted from ``start_iter``;
    every pass begins with ``sampler.set_epoch(iteration)`` (where the sampler has one), so each pass is another shuffle."""

    def __init__(self, batch_sampler, num_iterations, start_iter=0):
        self.batch_sampler, self.num_iterations, self.start_iter = batch_sampler, num_iterations, start_iter

    def __iter__(self):
        iteration = self.start_iter
        while iteration <= self.num_iterations:
            if hasattr(self.batch_sampler.sampler, "set_epoch"):
                self.batch_sampler.sampler.set_epoch(iteration)
            before = iteration
            for batch in self.batch_sampler:
                iteration += 1
                if iteration > self.num_iterations:
                    break
                yield batch
            if iteration == before:
                raise RuntimeError("the batch sampler yields no batch: an empty dataset (or share of it) cannot be iterated")

    def __len__(self):
        return self.num_iterations
