"""GPU: ``_C.lvis_match`` (csrc/lvis_eval.hip: rules 7 and 8 of LVIS-style federated scoring, include/ovis_hip.h) against
the matching of tests/lvis_reference.py on random and planted problem tables.  The tables are integers and flags: they are
compared exactly.  With all-zero flags the entry returns what ``_C.coco_match`` returns, bit for bit."""
import numpy as np
import pytest
import torch

from tests import lvis_reference as lref

pytestmark = pytest.mark.gpu

DEV = "cuda"
THRESHOLDS = np.linspace(.5, .95, 10)
AREA_RANGES = np.array([[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], dtype=np.float64)
EDGE_AREAS = np.array([32.0 ** 2, 96.0 ** 2, np.nextafter(32.0 ** 2, 0), np.nextafter(32.0 ** 2, 1e9), np.nextafter(96.0 ** 2, 0),
                       np.nextafter(96.0 ** 2, 1e9), 0.0, 1e10, 100.0, 5000.0, 20000.0])


def _problem(rs, nd, ng, flag, kind="random"):
    """One problem: (ious [nd, ng], det areas, gt areas, gt input ignore flags, not-exhaustive flag).  IoUs are drawn from
    a handful of values -- the ten thresholds themselves, their neighbours and values below .5 -- so that ties and IoUs
    exactly at a threshold are the rule, not the exception; areas from the edges of the area ranges."""
    values = np.concatenate([THRESHOLDS, np.nextafter(THRESHOLDS, 0), np.nextafter(THRESHOLDS, 1), [0.0, .25, .49, 1.0,
                             1 - 1e-10, np.nextafter(1 - 1e-10, 0)]])
    ious = rs.choice(values, size=(nd, ng))
    if kind == "sparse":      # most pairs do not overlap: detections mostly find one ground truth, or none
        ious = np.where(rs.rand(nd, ng) < 3.0 / max(ng, 1), ious, 0.0)
    if kind == "tied":        # whole rows of one value: the later ground truth must win, then the one before it, ...
        ious = np.repeat(rs.choice(THRESHOLDS, size=(nd, 1)), ng, axis=1)
    ignore = (rs.rand(ng) < .3).astype(np.uint8)
    if kind == "all_ignored":
        ignore[:] = 1
    return ious, rs.choice(EDGE_AREAS, size=nd), rs.choice(EDGE_AREAS, size=ng), ignore, flag


def _table(problems):
    """The device inputs of a list of problems and the reference's tables for them."""
    rows, d0, g0, off = [], 0, 0, 0
    want_m, want_di, want_gi = [], [], []
    for ious, da, ga, ig, flag in problems:
        nd, ng = ious.shape
        rows.append([d0, nd, g0, ng, off, 0, 0, 0])
        d0, g0, off = d0 + nd, g0 + ng, off + nd * ng
        m, di, gi = lref.match_problem(ious.tolist(), da.tolist(), ga.tolist(), ig.tolist(), flag)
        want_m.append(m)
        want_di.append(di)
        want_gi.append(gi)
    cat = lambda parts, dtype: torch.from_numpy(np.concatenate([np.asarray(p, dtype=dtype).reshape(-1) for p in parts]  # noqa: E731
                                                               + [np.zeros(0, dtype)])).to(DEV)
    return {"rows": rows, "iou": cat([p[0] for p in problems], np.float64), "det_areas": cat([p[1] for p in problems], np.float64),
            "gt_areas": cat([p[2] for p in problems], np.float64), "gt_ignore_in": cat([p[3] for p in problems], np.uint8),
            "flags": cat([[p[4]] for p in problems], np.uint8),
            "dt_match": np.concatenate(want_m, axis=2), "dt_ignore": np.concatenate(want_di, axis=2),
            "gt_ignore": np.concatenate(want_gi, axis=1)}


def _run(table, entry="lvis", zero_flags=False):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    problems = _C.CocoProblems(table["rows"], DEV)
    ranges, thresholds = torch.from_numpy(AREA_RANGES).to(DEV), torch.from_numpy(THRESHOLDS).to(DEV)
    ignore_in = torch.zeros_like(table["gt_ignore_in"]) if zero_flags else table["gt_ignore_in"]
    flags = torch.zeros_like(table["flags"]) if zero_flags else table["flags"]
    if entry == "coco":
        out = _C.coco_match(table["iou"], problems, table["det_areas"], table["gt_areas"], ignore_in, ranges, thresholds)
    else:
        out = _C.lvis_match(table["iou"], problems, table["det_areas"], table["gt_areas"], ignore_in, flags, ranges, thresholds)
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def mixed():
    """Every size at which the kernel takes another path, side by side in one table: no ground truth (flag clear and set),
    1, 63, 64, 65 (a second slot for lane 0 only) and 4096 (all 64 slots of every lane) ground truths, no detection, tied
    rows, all-ignored ground truths.  The reference is computed once."""
    rs = np.random.RandomState(7)
    return _table([_problem(rs, 3, 0, 0), _problem(rs, 3, 0, 1), _problem(rs, 70, 0, 1),   # 70: more detections than lanes
                   _problem(rs, 5, 1, 0), _problem(rs, 5, 1, 1),
                   _problem(rs, 7, 63, 1, "sparse"), _problem(rs, 7, 64, 0, "sparse"), _problem(rs, 9, 65, 1, "sparse"),
                   _problem(rs, 6, 65, 0, "tied"), _problem(rs, 4, 6, 0, "all_ignored"), _problem(rs, 4, 6, 1, "all_ignored"),
                   _problem(rs, 0, 5, 1), _problem(rs, 8, 8, 0), _problem(rs, 8, 8, 1),
                   _problem(rs, 3, 4096, 1, "sparse"), _problem(rs, 2, 130, 0, "tied")])


def test_lvis_match_equals_the_restatement(mixed):
    dt_match, dt_ignore, gt_ignore = _run(mixed)
    assert dt_match.dtype == torch.int32 and dt_ignore.dtype == torch.bool and gt_ignore.dtype == torch.bool
    assert np.array_equal(dt_match.cpu().numpy(), mixed["dt_match"])
    assert np.array_equal(dt_ignore.cpu().numpy(), mixed["dt_ignore"])
    assert np.array_equal(gt_ignore.cpu().numpy(), mixed["gt_ignore"])
    # the cases are what they claim to be: matches exist, at every threshold some and not all; both flag values bite
    assert (mixed["dt_match"] >= 0).any(axis=2).all() and (mixed["dt_match"] < 0).any(axis=2).all()
    assert mixed["dt_ignore"][0, 0, 3:6].all() and not mixed["dt_ignore"][0, 0, 0:3].any()   # area "all": the flag alone


def test_planted_rules():
    """Hand-made problems, the expected tables written out: a matched ignored ground truth is not matched again; an equal
    IoU goes to the later ground truth; an IoU equal to the threshold matches; a non-ignored match beats a better ignored
    one; the not-exhaustive flag touches unmatched detections only; areas exactly 32^2 and 96^2 lie inside both ranges."""
    z = np.zeros
    t50, t60, t70, t75 = THRESHOLDS[[0, 2, 4, 5]]   # the thresholds' own fp64 values: "equal to the threshold" is exact
    problems = [
        (np.array([[1.0], [1.0]]), np.array([100.0, 100.0]), np.array([100.0]), np.array([1], np.uint8), 0),
        (np.array([[t70, t70, t70], [t70, t70, t70]]), np.array([100.0, 100.0]), np.array([100.0] * 3), z(3, np.uint8), 0),
        (np.array([[t50], [t75]]), np.array([100.0, 100.0]), np.array([100.0]), z(1, np.uint8), 0),
        (np.array([[.9, t60]]), np.array([100.0]), np.array([100.0, 100.0]), np.array([1, 0], np.uint8), 0),
        (np.array([[.9], [.1]]), np.array([100.0, 100.0]), np.array([100.0]), z(1, np.uint8), 1),
        (np.array([[1.0, 0.0], [0.0, 1.0], [0.0, 0.0], [0.0, 0.0]]), np.array([1024.0, 9216.0, 1024.0, 9216.0]),
         np.array([1024.0, 9216.0]), z(2, np.uint8), 0)]
    table = _table(problems)
    dt_match, dt_ignore, gt_ignore = (x.cpu().numpy() for x in _run(table))
    assert np.array_equal(dt_match, table["dt_match"]) and np.array_equal(dt_ignore, table["dt_ignore"])
    assert np.array_equal(gt_ignore, table["gt_ignore"])
    assert dt_match[0, :, 0:2].tolist() == [[0, -1]] * 10 and dt_ignore[0, :, 0:2].tolist() == [[True, False]] * 10
    assert dt_match[0, 4, 2:4].tolist() == [2, 1] and dt_match[0, 5, 2:4].tolist() == [-1, -1]      # t70: thresholds 0..4
    assert dt_match[0, :, 4].tolist() == [0] + [-1] * 9 and dt_match[0, :, 5].tolist() == [-1] + [0] * 5 + [-1] * 4
    assert dt_match[0, 2, 6] == 1 and not dt_ignore[0, 2, 6] and dt_match[0, 3, 6] == 0 and dt_ignore[0, 3, 6]   # t60 < .65
    assert dt_match[0, 0, 7:9].tolist() == [0, -1] and dt_ignore[0, 0, 7:9].tolist() == [False, True]
    # area ranges all, small, medium, large: 1024 is small AND medium, 9216 medium AND large
    assert gt_ignore[:, 8:10].tolist() == [[False, False], [False, True], [False, False], [True, False]]
    assert dt_ignore[:, 0, 11].tolist() == [False, False, False, True] and dt_ignore[:, 0, 12].tolist() == [False, True, False, False]


def test_all_zero_flags_equal_coco_match_bit_for_bit(mixed):
    lvis, coco = _run(mixed, "lvis", zero_flags=True), _run(mixed, "coco", zero_flags=True)
    for a, b in zip(lvis, coco):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    assert not torch.equal(lvis[1], _run(mixed)[1])   # the flags of the fixture do change the tables


def test_no_pair_at_all_and_empty_tables(monkeypatch):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    rs = np.random.RandomState(3)
    table = _table([_problem(rs, 2, 0, 1), _problem(rs, 0, 3, 0), _problem(rs, 4, 0, 0)])
    assert table["iou"].numel() == 0                      # the IoU buffer is empty: the entry gets a null pointer
    dt_match, dt_ignore, gt_ignore = (x.cpu().numpy() for x in _run(table))
    assert (dt_match == -1).all() and np.array_equal(dt_ignore, table["dt_ignore"]) and np.array_equal(gt_ignore, table["gt_ignore"])
    assert dt_ignore[0, :, :2].all()

    def boom(*a):
        raise AssertionError("launched on an empty table")
    monkeypatch.setattr(_C._L, "ovis_lvis_match", boom)
    empty = {"rows": [], "iou": torch.zeros(0, dtype=torch.float64, device=DEV), "det_areas": torch.zeros(0, dtype=torch.float64, device=DEV),
             "gt_areas": torch.zeros(0, dtype=torch.float64, device=DEV), "gt_ignore_in": torch.zeros(0, dtype=torch.uint8, device=DEV),
             "flags": torch.zeros(0, dtype=torch.uint8, device=DEV)}
    out = _run(empty)
    assert out[0].shape == (4, 10, 0) and out[1].shape == (4, 10, 0) and out[2].shape == (4, 0)


def test_more_than_4096_ground_truths_is_a_range_error():
    z = lambda n, dtype: torch.zeros(n, dtype=dtype, device=DEV)   # noqa: E731
    table = {"rows": [[0, 1, 0, 4097, 0, 0, 0, 0]], "iou": z(4097, torch.float64), "det_areas": z(1, torch.float64),
             "gt_areas": z(4097, torch.float64), "gt_ignore_in": z(4097, torch.uint8), "flags": z(1, torch.uint8)}
    with pytest.raises(RuntimeError, match="OVIS_ERANGE"):
        _run(table)
    with pytest.raises(RuntimeError):   # one flag per row of the problem table
        table["flags"] = z(2, torch.uint8)
        _run(table)
