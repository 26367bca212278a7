"""GPU: ``ovis_coco_boundary_words_u64`` (csrc/coco_boundary.hip) against the iterated 3x3 erosion of
tests/boundary_reference.py -- words and counts EXACTLY (they are integers), for widths on both sides of a word, heights
from one row up, erosion depths whose window 2d + 1 crosses 64 bits, depths at which nothing survives, masks built to leak
across row ends and across the masks of one call, an output buffer pre-filled with -1, the error codes and the empty call.

Every (height, width) runs every depth on one batch of masks in one call each; the reference erodes each mask once, 33
iterations, and keeps the depths that are asked for."""
import ctypes

import numpy as np
import pytest
import torch

from tests import boundary_reference as bref

pytestmark = pytest.mark.gpu

DEV = "cuda"
WIDTHS = (1, 7, 63, 64, 65, 100, 129)
HEIGHTS = (1, 5, 33, 70)
DEPTHS = (1, 2, 3, 16, 31, 32, 33)


def _erosions(mask, depths):
    """{d: ``bref.erode(mask, d)``} from ONE run of the iteration."""
    out, m = {}, np.asarray(mask, dtype=bool)
    for d in range(1, max(depths) + 1):
        m = bref.erode(m, 1)
        if d in depths:
            out[d] = m
    return out


def _nearly_full(h, w, d, rs):
    """All ones minus 3-6 random zeros; of up to 200 draws the first whose eroded set is not empty (decided from the zeros
    alone: a survivor is a pixel of the inner (h - 2d) x (w - 2d) block farther than d from every zero), else the last."""
    ys, xs = np.mgrid[0:h, 0:w]
    inner = (ys >= d) & (ys < h - d) & (xs >= d) & (xs < w - d)
    for _ in range(200):
        k = min(int(rs.randint(3, 7)), h * w)
        zeros = rs.choice(h * w, k, replace=False)
        alive = inner.copy()
        for z in zeros:
            alive &= np.maximum(np.abs(ys - z // w), np.abs(xs - z % w)) > d
        if alive.any():
            break
    mask = np.ones((h, w), dtype=bool)
    mask.reshape(-1)[zeros] = False
    return mask


def _fixed_masks(h, w, rs):
    """-> (names, masks).  Neighbours in the batch are chosen so that a read across a mask's word slice would show: a mask
    whose LAST rows are full is followed by one whose FIRST rows are full, and full masks follow each other."""
    def blank():
        return np.zeros((h, w), dtype=bool)
    named = [("full", np.ones((h, w), dtype=bool)), ("full again", np.ones((h, w), dtype=bool)), ("empty", blank())]
    for name, (y, x) in (("top left", (0, 0)), ("top right", (0, w - 1)), ("bottom left", (h - 1, 0)),
                         ("bottom right", (h - 1, w - 1))):
        m = blank()
        m[y, x] = True
        named.append((name, m))
    row, col = blank(), blank()
    row[h // 2, :] = True
    col[:, w // 2] = True
    named += [("one row", row), ("one column", col)]
    ys, xs = np.mgrid[0:h, 0:w]
    named.append(("checkerboard", (ys + xs) % 2 == 0))
    hole = np.ones((h, w), dtype=bool)
    hole[h // 2, w // 2] = False
    named.append(("hole", hole))
    bottom, top = blank(), blank()
    bottom[h // 2:, :] = True       # ends in full rows ...
    top[:h - h // 2, :] = True      # ... and the next mask starts in full rows
    named += [("bottom rows", bottom), ("top rows", top)]
    # rows y and y + 1 full around the row end, the rest of the image full as well except the far columns: the last pixel
    # of row y and the first of row y + 1 are neighbours in the flat stream and must not keep each other alive
    wrap = np.ones((h, w), dtype=bool)
    if w > 4:
        wrap[:, w // 2] = False
    named.append(("row ends", wrap))
    named.append(("random", rs.rand(h, w) < .5))
    return [n for n, _ in named], np.stack([m for _, m in named])


def _raw_call(words, h, w, d, out=None, scratch=None, areas=None):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    n = words.shape[0]
    out = torch.full_like(words, -1) if out is None else out
    scratch = torch.full_like(words, -1) if scratch is None else scratch
    areas = torch.full((n,), -1, dtype=torch.int64, device=words.device) if areas is None else areas
    rc = _C._L.ovis_coco_boundary_words_u64(words.data_ptr(), n, h, w, d, scratch.data_ptr(), out.data_ptr(), areas.data_ptr(),
                                            _C._stream())
    return rc, out, areas


@pytest.mark.parametrize("h", HEIGHTS)
@pytest.mark.parametrize("w", WIDTHS)
def test_boundary_words_and_counts_equal_the_iterated_erosion(h, w):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    rs = np.random.RandomState(1000 * h + w)
    names, fixed = _fixed_masks(h, w, rs)
    eroded = [_erosions(m, DEPTHS) for m in fixed]
    nwords = (h * w + 63) // 64
    nontrivial = 0
    for d in DEPTHS:
        nearly = [_nearly_full(h, w, d, rs) for _ in range(2)]
        masks = np.concatenate([fixed, np.stack(nearly)])
        er = np.stack([e[d] for e in eroded] + [bref.erode(m, d) for m in nearly])
        if min(h, w) >= 2 * d + 8:   # room for survivors: the nearly full cases must not be vacuous
            for e, m in zip(er[len(fixed):], nearly):
                assert 0 < e.sum() < m.sum(), (h, w, d)
        if min(h, w) < 2 * d + 1:    # d >= min(h, w) / 2: nothing survives, the boundary is the mask
            assert not er.any()
        nontrivial += int(sum(0 < e.sum() < m.sum() for e, m in zip(er, masks)))
        want = masks & ~er
        want_words, want_areas = bref.pack(want), want.reshape(len(want), -1).sum(1)
        words = torch.from_numpy(bref.pack(masks)).to(DEV)
        rc, got, areas = _raw_call(words, h, w, d)   # out, scratch and areas pre-filled with -1
        assert rc == 0
        got_np = got.cpu().numpy()
        for k, name in enumerate(names + ["nearly full"] * 2):
            assert np.array_equal(got_np[k], want_words[k]), (h, w, d, name)
        assert torch.equal(got.cpu(), torch.from_numpy(want_words)) and got.shape == (len(masks), nwords)
        assert areas.cpu().tolist() == want_areas.tolist(), (h, w, d)
        if h * w % 64:   # every tail bit is zero
            assert not (got_np.view(np.uint64)[:, -1] >> np.uint64(h * w % 64)).any()
        rc2, again, areas2 = _raw_call(words, h, w, d)
        assert rc2 == 0 and torch.equal(again, got) and torch.equal(areas2, areas)   # the same bits on every call
        if d == DEPTHS[0]:
            by_wrapper = _C.coco_boundary_words(words, h, w, d)
            assert torch.equal(by_wrapper[0], got) and torch.equal(by_wrapper[1], areas)
    if min(h, w) >= 33:
        assert nontrivial >= len(fixed)   # the full, holed, banded and nearly full masks keep a real eroded set at small depths


def test_more_than_one_workgroup_per_mask_and_a_depth_of_its_own():
    """129 x 260 = 525 words: three workgroups of 256 words per mask, so the column pass reads across workgroup borders;
    d = 6 is the size's own depth, 40 a window of 81 bits."""
    h, w = 129, 260
    assert bref.dilation(h, w) == 6
    rs = np.random.RandomState(7)
    masks = np.stack([np.ones((h, w), dtype=bool), _nearly_full(h, w, 40, rs), rs.rand(h, w) < .97, rs.rand(h, w) < .5])
    words = torch.from_numpy(bref.pack(masks)).to(DEV)
    for d in (6, 40):
        er = np.stack([bref.erode(m, d) for m in masks])
        assert all(0 < e.sum() < m.sum() for e, m in zip(er[:2], masks[:2]))
        want = masks & ~er
        rc, got, areas = _raw_call(words, h, w, d)
        assert rc == 0 and torch.equal(got.cpu(), torch.from_numpy(bref.pack(want)))
        assert areas.cpu().tolist() == want.reshape(len(want), -1).sum(1).tolist()


def test_bad_arguments_and_the_empty_call():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C, _lib
    words = torch.zeros((2, 1), dtype=torch.int64, device=DEV)
    for h, w, d, n, code in ((5, 7, 0, 2, _lib.OVIS_EINVAL), (5, 7, -1, 2, _lib.OVIS_EINVAL), (0, 7, 1, 2, _lib.OVIS_EINVAL),
                             (5, 0, 1, 2, _lib.OVIS_EINVAL), (5, 7, 1, -1, _lib.OVIS_EINVAL),
                             (46341, 46341, 1, 2, _lib.OVIS_ERANGE), (1, 0x7ffffff0, 1, 2, _lib.OVIS_ERANGE)):
        out, areas = torch.full_like(words, -1), torch.full((2,), -1, dtype=torch.int64, device=DEV)
        rc = _C._L.ovis_coco_boundary_words_u64(words.data_ptr(), n, h, w, d, out.data_ptr(), out.data_ptr(), areas.data_ptr(),
                                                _C._stream())
        assert rc == code, (h, w, d, n, rc)
        assert (out == -1).all() and (areas == -1).all()   # refused before any launch
    null = ctypes.c_void_p(0)
    assert _C._L.ovis_coco_boundary_words_u64(null, 2, 5, 7, 1, null, null, null, _C._stream()) == _lib.OVIS_EINVAL
    assert _C._L.ovis_coco_boundary_words_u64(null, 0, 5, 7, 1, null, null, null, _C._stream()) == _lib.OVIS_OK   # n == 0
    got, areas = _C.coco_boundary_words(torch.zeros((0, 1), dtype=torch.int64, device=DEV), 5, 7, 1)
    assert got.shape == (0, 1) and areas.shape == (0,) and got.dtype == torch.int64 and areas.dtype == torch.int64
    with pytest.raises(RuntimeError) as e:
        _C.coco_boundary_words(words, 5, 7, 0)
    assert "OVIS_EINVAL" in str(e.value)
    with pytest.raises(RuntimeError):
        _C.coco_boundary_words(words, 5, 30, 1)        # 150 pixels are three words, not one
    with pytest.raises(RuntimeError):
        _C.coco_boundary_words(words.cpu(), 5, 7, 1)   # no host implementation
    # the largest size the entry accepts is the encoder's: one pixel fewer is not refused for its size (n == 0: no launch)
    assert _C._L.ovis_coco_boundary_words_u64(null, 0, 1, 0x7fffffef, 1, null, null, null, _C._stream()) == _lib.OVIS_OK
