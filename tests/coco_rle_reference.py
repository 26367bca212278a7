"""TEST-ONLY: pycocotools' ``rleEncode`` and ``rleToString`` (common/maskApi.c) restated in plain NumPy / Python -- the
expected values of the device encoder (csrc/mask_rle.hip), which has no host twin.  pycocotools is not a dependency; this
restatement is itself held to ``coco_eval.rle_decode`` (written independently, for the scorer) and to known strings by
tests/test_coco_results.py."""
import numpy as np


def rle_encode(mask):
    """The uncompressed counts (a list of ints) of a [H, W] mask: column-major, zeros first -- a run ends at every j with
    v(j) != v(j - 1), v(-1) = 0, and the counts are the gaps between consecutive ends from 0 up to H * W."""
    mask = np.asarray(mask)
    assert mask.ndim == 2
    v = (mask != 0).T.reshape(-1).astype(np.int8)   # column-major
    ends = np.flatnonzero(np.diff(np.concatenate([[0], v])))
    return np.diff(np.concatenate([[0], ends, [v.size]])).astype(np.int64).tolist()


def rle_to_string(counts):
    """The compressed ``counts`` string (bytes) of a list of counts."""
    out = bytearray()
    for i, x in enumerate(counts):
        x = int(x)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5          # Python's >> is arithmetic
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(c + 48)
    return bytes(out)


def encode(mask):
    """{"size": [h, w], "counts": str} as ``pycocotools.mask.encode`` + ``.decode("utf-8")`` give it."""
    mask = np.asarray(mask)
    return {"size": [int(mask.shape[0]), int(mask.shape[1])], "counts": rle_to_string(rle_encode(mask)).decode("ascii")}
