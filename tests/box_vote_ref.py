"""NumPy restatement of box voting (Detectron's ``box_voting``, scoring method ID) over a merged candidate list, and the
hand-made case table the host twin (tests/test_box_vote_reference.py) and the device kernel (tests/test_box_vote_gpu.py) are
both held to.

Who votes is decided by the float32 IoU, evaluated operand for operand like csrc/nms.hip (``iou32``: every intermediate is
rounded to float32 by NumPy's float32 scalars, nothing is contracted); the weighted means are float64.  ``vote`` also
returns the number of voters ``n`` of every detection, which the tests' error bound is made of:

    all coordinates are >= 0 (clipped boxes) and all scores > 0, so every term is non-negative; one rounding per product,
    two sums of n terms in any order and one quotient give, to first order, |got - want| <= (2 n + 4) * 2^-24 * want

per coordinate (``assert_within_bound``); a coordinate whose voters are all 0 has want == 0 and must come out exactly 0.
"""
import numpy as np

F = np.float32
ONE = F(1.0)
ZERO = F(0.0)


def iou32(a, b):
    """csrc/nms.hip::iou_xyxy on two float32 boxes, float32 operation by float32 operation."""
    a = [F(v) for v in a]
    b = [F(v) for v in b]
    left, right = max(a[0], b[0]), min(a[2], b[2])
    top, bottom = max(a[1], b[1]), min(a[3], b[3])
    width = max(F(F(right - left) + ONE), ZERO)
    height = max(F(F(bottom - top) + ONE), ZERO)
    inter = F(width * height)
    sa = F(F(F(a[2] - a[0]) + ONE) * F(F(a[3] - a[1]) + ONE))
    sb = F(F(F(b[2] - b[0]) + ONE) * F(F(b[3] - b[1]) + ONE))
    return F(inter / F(F(sa + sb) - inter))


def _iou32_many(a, boxes):
    """``iou32`` of one box against [n, 4] float32 boxes (float32 arrays: the same roundings, vectorised)."""
    a = np.asarray(a, dtype=F)
    left, right = np.maximum(a[0], boxes[:, 0]), np.minimum(a[2], boxes[:, 2])
    top, bottom = np.maximum(a[1], boxes[:, 1]), np.minimum(a[3], boxes[:, 3])
    width = np.maximum((right - left) + ONE, ZERO)
    height = np.maximum((bottom - top) + ONE, ZERO)
    inter = width * height
    sa = ((a[2] - a[0]) + ONE) * ((a[3] - a[1]) + ONE)
    sb = ((boxes[:, 2] - boxes[:, 0]) + ONE) * ((boxes[:, 3] - boxes[:, 1]) + ONE)
    out = inter / ((sa + sb) - inter)
    assert out.dtype == F
    return out


def vote(cand_boxes, cand_scores, offsets, cand_group, kept, vote_thresh):
    """-> (voted float64 [D, 4], n int64 [D]).  Arrays as ``_C.vote_boxes`` takes them; every kept index must lie in the
    run of its group."""
    cand_boxes = np.asarray(cand_boxes, dtype=F).reshape(-1, 4)
    cand_scores = np.asarray(cand_scores, dtype=F)
    thr = F(vote_thresh)
    voted, count = np.zeros((len(kept), 4), dtype=np.float64), np.zeros((len(kept),), dtype=np.int64)
    for j, d in enumerate(int(v) for v in kept):
        g = int(cand_group[d])
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        assert lo <= d < hi
        voters = lo + np.nonzero(_iou32_many(cand_boxes[d], cand_boxes[lo:hi]) >= thr)[0]
        s = cand_scores[voters].astype(np.float64)
        voted[j] = (s[:, None] * cand_boxes[voters].astype(np.float64)).sum(0) / s.sum()
        count[j] = len(voters)
    return voted, count


def assert_within_bound(got, want, n, what=""):
    got = np.asarray(got, dtype=np.float64)
    bound = (2.0 * n[:, None] + 4.0) * 2.0 ** -24 * want
    err = np.abs(got - want)
    assert (err <= bound).all(), (what, float((err - bound).max()), np.argwhere(err > bound)[:4].tolist())
    assert (got[want == 0.0] == 0.0).all(), what


# ---- the case table ---------------------------------------------------------------------------------------------------------
def _pack(runs, num_groups):
    """runs: {group: [(box, score), ...]} -> (cand_boxes, cand_scores, offsets, cand_group) in the merge's layout."""
    boxes, scores, group, offsets = [], [], [], [0]
    for g in range(num_groups):
        for box, score in runs.get(g, []):
            boxes.append(box)
            scores.append(score)
            group.append(g)
        offsets.append(len(boxes))
    return (np.asarray(boxes, dtype=F).reshape(-1, 4), np.asarray(scores, dtype=F), np.asarray(offsets, dtype=np.int32),
            np.asarray(group, dtype=np.int32))


def _cluster(rs, n, spread, bases=3):
    """n jittered copies of ``bases`` base boxes, clipped to a 200 x 150 image: most neighbours of a base overlap well."""
    base = np.array([[0.0, 0.0, 40.0, 60.0], [60.0, 20.0, 150.0, 100.0], [20.0, 30.0, 90.0, 110.0]])[rs.randint(0, bases, n)]
    boxes = base + rs.uniform(-spread, spread, (n, 4))
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0.0, 199.0)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0.0, 149.0)
    return [(b, s) for b, s in zip(boxes.astype(F), rs.uniform(0.05, 1.0, n).astype(F))]


BELOW_HALF_Y2 = 4.0 - 2.0 ** -21   # [0, 0, 9, y2] against [0, 0, 9, 9]: float32 IoU = the float32 just below 0.5


def build_cases():
    """name -> (cand_boxes, cand_scores, offsets, cand_group, kept, vote_thresh)."""
    cases = {}
    rs = np.random.RandomState(20)
    # the lane-stride edges: runs of 1, 63, 64, 65 and 129 candidates (classes 1..5 of one image; class 0 is empty), the
    # kept detections at the first and the last index of every run and a few in between
    lengths = [1, 63, 64, 65, 129]
    packed = _pack({g + 1: _cluster(rs, n, 6.0, 1 if n > 64 else 3) for g, n in enumerate(lengths)}, 6)   # one cluster: > 64 voters
    kept = []
    for g in range(1, 6):
        lo, hi = int(packed[2][g]), int(packed[2][g + 1])
        kept += sorted({lo, hi - 1, (lo + hi) // 2, min(lo + 63, hi - 1), min(lo + 64, hi - 1)})
    cases["lane_stride_edges"] = packed + (np.asarray(kept, dtype=np.int64), 0.5)
    cases["lane_stride_edges_thr_0.8"] = packed + (np.asarray(kept[::-1], dtype=np.int64), 0.8)   # kept in any order

    # two images x three classes, an empty run between two non-empty ones (image 0 class 2 and image 1 class 0), and boxes
    # with d's coordinates in another class of the same image / the same class of the other image: they must not vote
    d, near = [10.0, 10.0, 50.0, 50.0], [12.0, 12.0, 52.0, 52.0]
    runs = {1: [(d, 0.5), (near, 0.9), ([100.0, 100.0, 120.0, 120.0], 0.7)],           # image 0, class 1
            4: [(d, 1.0), (near, 0.25)],                                               # image 1, class 1: d's class
            5: [(d, 1.0), ([11.0, 9.0, 49.0, 51.0], 0.3)]}                             # image 1, class 2
    packed = _pack(runs, 6)
    assert packed[2].tolist() == [0, 0, 3, 3, 3, 5, 7]
    cases["two_images_three_classes"] = packed + (np.asarray([0, 2, 3, 4, 6], dtype=np.int64), 0.5)
    runs[2] = [(d, 1.0)]                                                               # image 0, class 2: d's image
    packed = _pack(runs, 6)
    cases["same_box_in_other_class_and_other_image"] = packed + (np.asarray([0, 1, 3, 4], dtype=np.int64), 0.5)

    # planted ties: a 10 x 10 box against its own 10 x 5 half is IoU 0.5 exactly under the +1 convention, against its 5 x 5
    # corner 0.25 exactly; the tied candidate votes, the neighbour one float32 below the threshold does not
    ten, half, corner = [0.0, 0.0, 9.0, 9.0], [0.0, 0.0, 9.0, 4.0], [0.0, 0.0, 4.0, 4.0]
    below = [0.0, 0.0, 9.0, BELOW_HALF_Y2]
    packed = _pack({1: [(ten, 0.5), (half, 0.9), (below, 0.8)], 2: [(ten, 0.5), (corner, 0.9)]}, 3)
    cases["ties_at_0.5"] = packed + (np.asarray([0, 1, 2], dtype=np.int64), 0.5)
    cases["ties_at_0.25"] = packed + (np.asarray([3, 4], dtype=np.int64), 0.25)

    # vote_thresh 1.0: only coincident boxes vote
    box = [7.0, 3.0, 61.0, 47.0]
    almost = [7.0, 3.0, 61.0, float(np.nextafter(F(47.0), F(0.0)))]
    packed = _pack({1: [(box, 0.3), (almost, 0.9), (box, 0.6), ([7.0, 3.0, 61.0, 48.0], 0.95), (box, 0.2)]}, 2)
    cases["coincident_only_at_1.0"] = packed + (np.asarray([0, 1, 4], dtype=np.int64), 1.0)

    # nothing kept, and nothing at all
    cases["no_detections"] = packed + (np.zeros((0,), dtype=np.int64), 0.5)
    cases["no_candidates"] = _pack({}, 4) + (np.zeros((0,), dtype=np.int64), 0.5)
    return cases


CASES = build_cases()
_WANT = {}


def want(name):
    """The restatement's (voted, n) of a case, computed once and shared."""
    if name not in _WANT:
        _WANT[name] = vote(*CASES[name])
        for a in _WANT[name]:
            a.setflags(write=False)
    return _WANT[name]
