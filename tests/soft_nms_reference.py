"""NumPy restatement of Soft-NMS (Bodla et al., ICCV 2017) over the runs of a candidate list, as include/ovis_hip.h states the
rule, and the hand-made cases the host twin (tests/test_soft_nms_reference.py) and the device kernel
(tests/test_soft_nms_gpu.py) are both held to, bit for bit.

Plain Python loops over NumPy float32 scalars: every intermediate is rounded to float32, nothing is contracted.  The IoU is
``tests/box_vote_ref.py::iou32`` (csrc/nms.hip's expression), the Gaussian weight ``np.float32(np.exp(-np.float64(q)))``.
Nothing here reads the code under test.
"""
import numpy as np

from tests.box_vote_ref import BELOW_HALF_Y2, _cluster, _iou32_many, iou32

F = np.float32
ONE = F(1.0)
ZERO = F(0.0)


def soft_nms_run(boxes, scores, method, nt, sigma, min_score):
    """One run: boxes [n, 4] / scores [n] float32 -> soft scores [n] float32 (0: discarded)."""
    n = len(scores)
    nt, sigma, min_score = F(nt), F(sigma), F(min_score)
    w = [F(s) for s in scores]
    alive = [bool(s > ZERO) for s in w]          # a score that is not > 0 counts as discarded
    out = np.zeros((n,), dtype=F)
    while any(alive):
        m = -1
        for k in range(n):                       # the largest working score; ties go to the lower index
            if alive[k] and (m < 0 or w[k] > w[m]):
                m = k
        out[m] = w[m]
        alive[m] = False
        for k in range(n):
            if not alive[k]:
                continue
            ov = iou32(boxes[m], boxes[k])
            if method == "linear":
                weight = F(ONE - ov) if ov > nt else ONE
            elif method == "hard":
                weight = ZERO if ov > nt else ONE
            else:
                assert method == "gaussian"
                q = F(F(ov * ov) / sigma)
                weight = np.float32(np.exp(-np.float64(q)))
            w[k] = F(w[k] * weight)
            if w[k] < min_score or not w[k] > ZERO:
                alive[k] = False
    return out


def soft_nms_run_rows(boxes, scores, method, nt, sigma, min_score):
    """``soft_nms_run`` with the inner loop over k written on float32 ARRAYS (``box_vote_ref._iou32_many``: the same
    roundings, element by element), for the runs of a few thousand candidates the scalar loops would take minutes over.
    tests/test_soft_nms_reference.py holds it to ``soft_nms_run`` bit for bit."""
    boxes = np.asarray(boxes, dtype=F).reshape(-1, 4)
    nt, sigma, min_score = F(nt), F(sigma), F(min_score)
    w = np.array(scores, dtype=F)
    alive = w > ZERO
    out = np.zeros((len(w),), dtype=F)
    while alive.any():
        m = int(np.argmax(np.where(alive, w, F(-1.0))))          # argmax returns the FIRST maximum: the lower index
        out[m] = w[m]
        alive[m] = False
        idx = np.nonzero(alive)[0]
        ov = _iou32_many(boxes[m], boxes[idx])
        if method == "linear":
            weight = np.where(ov > nt, ONE - ov, ONE)
        elif method == "hard":
            weight = np.where(ov > nt, ZERO, ONE)
        else:
            assert method == "gaussian"
            weight = np.exp(-((ov * ov) / sigma).astype(np.float64)).astype(F)
        assert weight.dtype == F
        w[idx] = w[idx] * weight
        alive[idx] = ~((w[idx] < min_score) | ~(w[idx] > ZERO))
    return out


def soft_nms(cand_boxes, cand_scores, offsets, method="linear", nt=0.5, sigma=0.5, min_score=0.0, run=soft_nms_run):
    """The whole list: arrays as ``_C.soft_nms`` takes them -> soft_scores [K] float32."""
    cand_boxes = np.asarray(cand_boxes, dtype=F).reshape(-1, 4)
    cand_scores = np.asarray(cand_scores, dtype=F)
    out = np.zeros((len(cand_scores),), dtype=F)
    with np.errstate(over="ignore", invalid="ignore"):
        for g in range(len(offsets) - 1):
            lo, hi = int(offsets[g]), int(offsets[g + 1])
            out[lo:hi] = run(cand_boxes[lo:hi], cand_scores[lo:hi], method, nt, sigma, min_score)
    return out


def greedy_nms_keep(boxes, scores, nt):
    """Greedy NMS in `>` mode, written on its own (descending score, stable: the lower index first; a box goes when its
    IoU with a kept box is > nt) -> the kept indices, ascending."""
    order = sorted(range(len(scores)), key=lambda k: -float(scores[k]))   # sorted() is stable
    gone, keep = set(), []
    for pos, i in enumerate(order):
        if i in gone:
            continue
        keep.append(i)
        for j in order[pos + 1:]:
            if j not in gone and iou32(boxes[i], boxes[j]) > F(nt):
                gone.add(j)
    return sorted(keep)


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def pack(runs):
    """runs: a list of [(box, score), ...] -> (cand_boxes [K, 4], cand_scores [K], offsets [G + 1] int32)."""
    boxes, scores, offsets = [], [], [0]
    for run in runs:
        for box, score in run:
            boxes.append(box)
            scores.append(score)
        offsets.append(len(boxes))
    return (np.asarray(boxes, dtype=F).reshape(-1, 4), np.asarray(scores, dtype=F), np.asarray(offsets, dtype=np.int32))


def clustered(seed, lengths, spread=8.0):
    """One run per entry of ``lengths``: jittered copies of three base boxes (box_vote_ref._cluster), so most neighbours
    overlap, decays compound and discards are frequent."""
    rs = np.random.RandomState(seed)
    return pack([_cluster(rs, n, spread) if n else [] for n in lengths])


# Boxes with exact IoUs under the +1 convention: TEN against HALF is 50 / 100 = 0.5 exactly, against BELOW the float32 just
# below 0.5 (box_vote_ref.BELOW_HALF_Y2) and against JUST_ABOVE the float32 just above it; planted() asserts all three
TEN, HALF, FAR = [0.0, 0.0, 9.0, 9.0], [0.0, 0.0, 9.0, 4.0], [100.0, 100.0, 109.0, 109.0]
BELOW = [0.0, 0.0, 9.0, BELOW_HALF_Y2]
JUST_ABOVE = [0.0, 0.0, 9.0, 4.0 + 2.0 ** -21]


def f32(pattern):
    """The float32 with this bit pattern, as a Python float."""
    return float(np.array([pattern], dtype=np.uint32).view(F)[0])


def planted():
    """name -> ((cand_boxes, cand_scores, offsets), method, nt, sigma, min_score, want).  ``want`` is written out as literals,
    worked out by hand in the comment above each case (bit patterns where the value is no short decimal)."""
    assert float(iou32(TEN, HALF)) == 0.5 and iou32(TEN, BELOW) == np.nextafter(F(0.5), ZERO)
    assert iou32(TEN, JUST_ABOVE) == np.nextafter(F(0.5), ONE)
    cases = {}
    # one candidate; an empty run between two full ones (disjoint boxes: nothing decays)
    cases["one_candidate"] = (pack([[(TEN, 0.75)]]), "linear", 0.5, 0.5, 0.0, [0.75])
    cases["empty_run_between_two"] = (pack([[(TEN, 0.5), (FAR, 0.25)], [], [(TEN, 0.125)]]), "linear", 0.5, 0.5, 0.0,
                                      [0.5, 0.25, 0.125])
    # The decay changes the order of selection.  A = [0,0,9,9] 0.875, B = [0,0,9,7] 0.75, C disjoint 0.5.  IoU(A, B) = 80 / 100
    # = float32(0.8) = 0x3f4ccccd > 0.5; 1 - that = 0x3e4ccccc exactly; B = 0.75 * 0x3e4ccccc = 0x3e199999 (0.14999999) falls
    # below C, which is selected second and does not touch B.  Without the decay the order would be A, B, C.
    cases["decay_reorders"] = (pack([[([0.0, 0.0, 9.0, 9.0], 0.875), ([0.0, 0.0, 9.0, 7.0], 0.75), (FAR, 0.5)]]),
                               "linear", 0.5, 0.5, 0.0, [0.875, f32(0x3e199999), 0.5])
    # Decayed by several selected boxes in turn, Nt = 0.3.  TEN 1.0 (area 100), BIG = [0,0,9,19] 0.5 (200), HALF 0.75 (50),
    # Y = [0,0,9,14] 0.9375 (150).  Select TEN: BIG 0.5 * (1 - 100/200) = 0.25; HALF 0.75 * (1 - 50/100) = 0.375;
    # Y 0.9375 * (1 - float32(100/150)) = 0.9375 * 0x3eaaaaaa, just under 0.3125.  Select HALF (0.375): IoU(HALF, BIG) = 50/200 =
    # 0.25, not > 0.3: BIG stays 0.25; IoU(HALF, Y) = 50/150 > 0.3: Y *= 1 - float32(1/3) = 0x3f2aaaaa, about 0.2083.  Select BIG
    # (0.25 > 0.2083): IoU(BIG, Y) = 150/200 = 0.75: Y *= 0.25 -> 0x3d555553 (0.052083325).
    cases["decays_in_turn"] = (pack([[(TEN, 1.0), ([0.0, 0.0, 9.0, 19.0], 0.5), (HALF, 0.75), ([0.0, 0.0, 9.0, 14.0], 0.9375)]]),
                               "linear", 0.3, 0.5, 0.0, [1.0, 0.25, 0.375, f32(0x3d555553)])
    # Decayed to EXACTLY min_score: kept, the comparison is strict.  0.125 * (1 - 0.5) = 0.0625 against min_score 0.0625; the
    # same candidate one float32 lower, 0.125 - 2^-27 = 0x3dffffff, lands one float32 under 0.0625 and is discarded.
    cases["exactly_min_score_is_kept"] = (pack([[(TEN, 1.0), (HALF, 0.125)]]), "linear", 0.25, 0.5, 0.0625, [1.0, 0.0625])
    cases["one_float_below_min_score_is_discarded"] = (pack([[(TEN, 1.0), (HALF, f32(0x3dffffff))]]), "linear", 0.25, 0.5,
                                                       0.0625, [1.0, 0.0])
    # An IoU exactly at Nt does not decay (> is strict), the float32 just above it does (linear: 0.5 * (1 - 0x3f000001) =
    # 0.5 * 0x3efffffe = 0x3e7ffffe; hard: gone), the float32 just below it does not.
    at_nt = pack([[(TEN, 1.0), (HALF, 0.5)], [(TEN, 1.0), (JUST_ABOVE, 0.5)], [(TEN, 1.0), (BELOW, 0.5)]])
    cases["iou_at_nt_linear"] = (at_nt, "linear", 0.5, 0.5, 0.0, [1.0, 0.5, 1.0, f32(0x3e7ffffe), 1.0, 0.5])
    cases["iou_at_nt_hard"] = (at_nt, "hard", 0.5, 0.5, 0.0, [1.0, 0.5, 1.0, 0.0, 1.0, 0.5])
    # Two alive candidates with equal working scores that overlap each other (IoU 0.5 > 0.25): the LOWER index is selected
    # and keeps 0.5, the other one shows it with 0.5 * 0.5 = 0.25 -- whichever box comes first.
    cases["tie_lower_index_first"] = (pack([[(HALF, 0.5), (TEN, 0.5)]]), "linear", 0.25, 0.5, 0.0, [0.5, 0.25])
    cases["tie_lower_index_first_reversed"] = (pack([[(TEN, 0.5), (HALF, 0.5)]]), "linear", 0.25, 0.5, 0.0, [0.5, 0.25])
    # A tie that arises from a decay.  S = [0,0,4,4] 1.0 (area 25), P = [0,0,4,9] 0.5 (50), Q = [0,5,4,9] 0.25 (25):
    # IoU(S, P) = 25/50 = 0.5, IoU(S, Q) = 0, IoU(P, Q) = 25/50 = 0.5.  S is selected, P becomes 0.25 and ties with Q; the one
    # with the lower index is selected with 0.25 and the other ends at 0.125.
    s_box, p_box, q_box = [0.0, 0.0, 4.0, 4.0], [0.0, 0.0, 4.0, 9.0], [0.0, 5.0, 4.0, 9.0]
    cases["tie_from_a_decay_q_first"] = (pack([[(q_box, 0.25), (s_box, 1.0), (p_box, 0.5)]]), "linear", 0.25, 0.5, 0.0,
                                         [0.25, 1.0, 0.125])
    cases["tie_from_a_decay_p_first"] = (pack([[(p_box, 0.5), (s_box, 1.0), (q_box, 0.25)]]), "linear", 0.25, 0.5, 0.0,
                                         [0.25, 1.0, 0.125])
    # Nt = 1: no IoU is > 1, every candidate keeps its score, coincident boxes included.
    same = pack([[(TEN, 0.5), (TEN, 0.75), (HALF, 0.25), (TEN, 0.75)]])
    cases["nt_one_linear"] = (same, "linear", 1.0, 0.5, 0.0, [0.5, 0.75, 0.25, 0.75])
    cases["nt_one_hard"] = (same, "hard", 1.0, 0.5, 0.0, [0.5, 0.75, 0.25, 0.75])
    # gaussian: every overlapping candidate decays whatever Nt says, a disjoint one keeps its bits (weight exp(-0) = 1).
    # IoU 0.5, sigma 0.5: q = 0.25 / 0.5 = 0.5, weight = float32(exp(-0.5)) = 0x3f1b4598 (0.60653067); times 0.5 is exact.
    cases["gaussian_decays_all_overlaps"] = (pack([[(TEN, 1.0), (HALF, 0.5), (FAR, 0.3)]]), "gaussian", 0.9, 0.5, 0.0,
                                             [1.0, f32(0x3e9b4598), f32(0x3e99999a)])
    # min_score 0: a product that is exactly 0 (coincident boxes, linear: 1 - 1 = 0) is discarded like any other.
    cases["zero_product_is_discarded"] = (pack([[(TEN, 1.0), (TEN, 0.5)]]), "linear", 0.5, 0.5, 0.0, [1.0, 0.0])
    return cases


PLANTED = planted()


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F)).view(np.uint32)
