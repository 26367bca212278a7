"""Copy-paste augmentation restated in NumPy as plain loops over given masks and images (steps 2-5 of the rule in
include/ovis_hip.h and its keep rule), independent of how the kernels are organised.  The rule is this project's own: this
file checks the kernels against the written rule, not against any other implementation."""
import numpy as np


def alpha_of(pasted, hw):
    """uint8 [h, w], 0 / 1: the OR of the pasted masks (all zero without any)."""
    h, w = hw
    alpha = np.zeros((h, w), dtype=np.uint8)
    for m in pasted:
        for y in range(h):
            for x in range(w):
                if m[y, x]:
                    alpha[y, x] = 1
    return alpha


def cover(own, alpha):
    """(the own masks with the covered pixels removed, the table int32 [G_own, 6]): per mask the pixels before, the pixels
    after, and the tight box x1, y1, x2, y2 of what is left in pixel indices -- (0, 0, -1, -1) when nothing is."""
    own = np.array(own, dtype=np.uint8, copy=True).reshape((-1,) + alpha.shape)
    table = np.zeros((own.shape[0], 6), dtype=np.int32)
    h, w = alpha.shape
    for g in range(own.shape[0]):
        before = after = 0
        xs, ys = [], []
        for y in range(h):
            for x in range(w):
                if own[g, y, x]:
                    before += 1
                    if alpha[y, x]:
                        own[g, y, x] = 0
                    else:
                        after += 1
                        xs.append(x)
                        ys.append(y)
        table[g] = (before, after) + ((min(xs), min(ys), max(xs), max(ys)) if after else (0, 0, -1, -1))
    return own, table


def keep_rule(table, boxes):
    """(rows kept, their boxes float32 [K, 4]) of the own instances: an untouched one (count unchanged) stays with its
    annotation box, even at a count of 0; a touched one takes the tight box and stays iff x2 > x1 and y2 > y1."""
    keep, out = [], []
    for g, (before, after, x1, y1, x2, y2) in enumerate(np.asarray(table).tolist()):
        if after == before:
            keep.append(g)
            out.append([float(v) for v in boxes[g]])
        elif x2 > x1 and y2 > y1:
            keep.append(g)
            out.append([float(x1), float(y1), float(x2), float(y2)])
    return keep, np.array(out, dtype=np.float32).reshape(-1, 4)


def paste_image_targets(own_masks, own_boxes, own_labels, pasted_masks, pasted_boxes, pasted_labels, hw):
    """One pasted-into image: -> (alpha, boxes float32 [G', 4], labels [G'], dense masks uint8 [G', h, w]), own rows first."""
    alpha = alpha_of(pasted_masks, hw)
    covered, table = cover(own_masks, alpha)
    keep, boxes = keep_rule(table, own_boxes)
    pasted_masks = np.asarray(pasted_masks, dtype=np.uint8).reshape((-1,) + tuple(hw))
    boxes = np.concatenate([boxes, np.asarray(pasted_boxes, dtype=np.float32).reshape(-1, 4)])
    labels = np.concatenate([np.asarray(own_labels)[keep], np.asarray(pasted_labels)])
    return alpha, boxes, labels, np.concatenate([covered[keep], pasted_masks])


def paste_pixels(batch, alphas, paste_src):
    """The batch [B, C, H, W] (any 4-byte dtype: the copy is bit-wise) with, for every image i whose source is >= 0,
    out[i, c, y, x] = in[paste_src[i], c, y, x] where alphas[i][y, x] is set; the right-hand side is the batch as given."""
    out = batch.copy()
    for i, src in enumerate(paste_src):
        if src < 0:
            continue
        a = alphas[i]
        for y in range(a.shape[0]):
            for x in range(a.shape[1]):
                if a[y, x]:
                    out[i, :, y, x] = batch[src, :, y, x]
    return out
