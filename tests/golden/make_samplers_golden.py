"""Writes tests/golden/samplers.npz: the index batches of the REFERENCE's own ``DistributedSampler``,
``GroupedBatchSampler`` and ``IterationBasedBatchSampler`` (maskrcnn_benchmark/data/samplers/*.py, imported through
ref_import.py) for the cases of ``CASES`` below, one list of batches per rank (python tests/golden/make_samplers_golden.py).
Should the reference's classes fail to import, the generator stops: a restatement would prove nothing.

Per case c and rank r: ``c<c>_r<r>_flat`` (the indices of all batches back to back) and ``c<c>_r<r>_len`` (the batch
lengths).  ``heights`` / ``widths`` are the image sizes the aspect-ratio groups come from, ``group_ids`` is
``bisect_right([1], height / width)`` of each (the reference's ``_quantize``, data/build.py:76-89, whose module cannot be
imported without torchvision) and ``cases`` the table itself.
"""
import bisect
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

# (height, width) of 11 images: five wide, five tall, one exactly square (ratio 1.0 falls into the tall bin)
SIZES = [(480, 640), (640, 480), (427, 640), (640, 427), (500, 500), (375, 500), (500, 375), (480, 640), (640, 426),
         (333, 500), (600, 400)]
# (world, grouping, batch, drop_uneven, shuffle, start_iter, iterations)
CASES = [(1, 1, 2, 0, 1, 0, 13), (3, 1, 2, 0, 1, 0, 13), (1, 1, 2, 1, 1, 0, 13), (2, 0, 2, 0, 0, 4, 13)]


def main():
    import ref_import
    ref_import.install()
    from maskrcnn_benchmark.data.samplers import DistributedSampler, GroupedBatchSampler, IterationBasedBatchSampler

    n = len(SIZES)
    group_ids = [bisect.bisect_right([1], float(h) / float(w)) for h, w in SIZES]
    out = {"heights": np.array([s[0] for s in SIZES], dtype=np.int64), "widths": np.array([s[1] for s in SIZES], dtype=np.int64),
           "group_ids": np.array(group_ids, dtype=np.int64), "cases": np.array(CASES, dtype=np.int64)}
    for c, (world, grouping, batch, drop_uneven, shuffle, start_iter, iterations) in enumerate(CASES):
        for rank in range(world):
            sampler = DistributedSampler(list(range(n)), num_replicas=world, rank=rank, shuffle=bool(shuffle))
            if grouping:
                batch_sampler = GroupedBatchSampler(sampler, group_ids, batch, drop_uneven=bool(drop_uneven))
            else:
                batch_sampler = torch.utils.data.sampler.BatchSampler(sampler, batch, drop_last=bool(drop_uneven))
            batches = list(IterationBasedBatchSampler(batch_sampler, iterations, start_iter))
            assert len(batches) == iterations - start_iter
            out[f"c{c}_r{rank}_flat"] = np.array([i for b in batches for i in b], dtype=np.int64)
            out[f"c{c}_r{rank}_len"] = np.array([len(b) for b in batches], dtype=np.int64)
    path = os.path.join(HERE, "samplers.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
