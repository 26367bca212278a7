"""CPU: the NumPy restatement of the RLE-target chain (tests/rle_targets_reference.py -- what the GPU tests hold
``_C.project_rle_masks`` to) against the reference's own ``SegmentationMask(mode='mask')`` chain, recorded in
tests/golden/rle_targets.npz by tests/golden/make_rle_targets_golden.py.

The restatement applies the exact rule (a resampled pixel is 1 iff every tap with a non-zero weight is set); the reference
sums the taps in fp32 and truncates.  With E the exact interpolated value (fp64, from the restatement's own fp32 lams), the
two must agree wherever E < 1 - 2^-21 or E > 1: the reference's sum has at most five fp32 roundings at magnitude <= 1, and
5 * 2^-24 < 2^-21.  Inside that band they may differ in either direction (an all-set pixel that sums to 0.99999994 and is
dropped; a pixel with an unset tap of weight ~1e-9 that sums to 1.0 and is kept), and the pixels that use this allowance
must stay below 5 % of the compared pixels of each stage of each case.  The two stages are judged separately: stage 2 of
the restatement is computed from the REFERENCE's stage-1 output."""
import os

import numpy as np
import pytest

from tests import rle_targets_reference as rt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rle_targets.npz")
BAND_LO = 1.0 - 2.0 ** -21


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def _judge(ours, theirs, exact, what):
    """ours / theirs bool, exact fp64, same shape -> the fraction of pixels that differ (all of them inside the band)."""
    differ = ours != theirs
    outside = (exact < BAND_LO) | (exact > 1.0)
    assert not (differ & outside).any(), f"{what}: {int((differ & outside).sum())} differences outside the rounding band"
    frac = differ.sum() / differ.size
    print(f"{what}: {int(differ.sum())} of {differ.size} pixels differ inside the band ({100 * frac:.2f} %)")
    assert frac < 0.05, f"{what}: {100 * frac:.2f} % of the pixels need the rounding band"
    return frac


@pytest.mark.parametrize("case", list(rt.golden_cases()), ids=lambda c: f"{c[1][0]}x{c[1][1]}-{c[2][0]}x{c[2][1]}-h{int(c[3])}v{int(c[4])}")
def test_restatement_agrees_with_the_reference_outside_the_rounding_band(golden, case):
    k, (h0, w0), (h1, w1), flip_h, flip_v, mask_seed, box_seed = case
    M = int(golden["resolution"])
    source = rt.salt_and_pepper(1, h0, w0, mask_seed)
    # stage 1: resize + flips
    ref1 = np.unpackbits(golden[f"stage1_{k}"])[: h1 * w1].reshape(h1, w1).astype(bool)
    ours1 = rt.resized_flipped(source, (h1, w1), flip_h, flip_v)[0]
    exact1 = rt.resize_exact(source, h1, w1)[0]
    exact1 = exact1[::-1] if flip_v else exact1
    exact1 = exact1[:, ::-1] if flip_h else exact1
    _judge(ours1, ref1, exact1, "stage 1")
    if (h0, w0) == (h1, w1):
        assert np.array_equal(ours1, ref1)  # no resize recorded: every lam is 0, R = S
    # stage 2: crop + resize of the reference's stage-1 output
    boxes = golden[f"boxes_{k}"]
    assert np.array_equal(boxes, rt.random_boxes(rt.GOLDEN_BOXES, w1, h1, box_seed))
    ref2 = np.unpackbits(golden[f"stage2_{k}"])[: len(boxes) * M * M].reshape(len(boxes), M, M).astype(bool)
    ours2 = rt.crop_resize(ref1[None], np.zeros(len(boxes), dtype=np.int64), boxes, M).astype(bool)
    exact2 = np.stack([rt.resize_exact(ref1[y0:y1, x0:x1], M, M)
                       for x0, y0, x1, y1 in (rt.crop_window(b, w1, h1) for b in boxes)])
    _judge(ours2, ref2, exact2, "stage 2")
    assert ours2.any() and not ours2.all()


def test_rule_on_integer_positions_reads_one_tap():
    """A crop whose size is a multiple of the output size puts every source position on a pixel (lam == 0 exactly, thanks
    to the correctly rounded in / out scale): the second tap has no weight and must not be asked."""
    mask = rt.salt_and_pepper(1, 42, 28, 3)[0]
    for n_in, n_out in ((14, 14), (28, 14), (42, 14), (42, 7)):
        i0, i1, lam = rt.axis_taps(n_in, n_out)
        if n_in == n_out:
            assert (lam == 0).all() and (i0 == np.arange(n_out)).all()
        else:
            assert (lam == 0.5).all() if (n_in // n_out) % 2 == 0 else (lam == 0).all()
    assert np.array_equal(rt.resize_rule(mask, 42, 28), mask)
    assert np.array_equal(rt.resize_rule(mask, 14, 28), mask[1::3])   # 42 -> 14: src = 3 d + 1, one tap


def test_crop_window_rounds_half_to_even_and_clamps():
    assert rt.crop_window([0.5, 1.5, 2.5, 3.5], 50, 40) == (0, 2, 2, 4)
    assert rt.crop_window([-5.0, -3.0, 10.5, 7.5], 50, 40) == (0, 0, 10, 8)
    assert rt.crop_window([47.0, 38.0, 59.0, 44.0], 50, 40) == (47, 38, 50, 40)
    assert rt.crop_window([60.0, 50.0, 70.0, 60.0], 50, 40) == (49, 39, 50, 40)
    assert rt.crop_window([30.0, 20.0, 30.0, 20.0], 50, 40) == (30, 20, 31, 21)
