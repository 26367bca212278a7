"""GPU: ``_C.error_types`` (csrc/error_types.hip: the TYPES and MISSED rules of the error analysis, include/ovis_hip.h)
against ``classify`` of tests/error_reference.py.  The image-level IoU is the device's own (``_C.coco_box_iou`` on a table with
one row per image), so the three output arrays are compared exactly.  One segm case goes through ``score_chunk`` with two
image sizes: the image-level word offsets."""
import numpy as np
import pytest
import torch

from tests import error_reference as eref

pytestmark = pytest.mark.gpu

DEV = "cuda"
UNIT = [0.0, 0.0, 10.0, 10.0]   # the detection of the planted cases; [0, 0, 10, h] has IoU 10 / h with it


def tall(h, x=0.0):
    return [x, 0.0, 10.0, float(h)]


def image(dets, gts):
    """dets: [(category, xywh, base match: a ground-truth row of THIS image or -1, ignored)], gts: [(category, xywh, crowd)]."""
    return {"dets": list(dets), "gts": list(gts)}


def run(images, t_f=0.5, t_b=0.1):
    """-> (the device's outputs as NumPy arrays, the reference's on the device's own IoU values, the device tensors)."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    rows, d0, g0, off = [], 0, 0, 0
    for im in images:
        nd, ng = len(im["dets"]), len(im["gts"])
        rows.append([d0, nd, g0, ng, off, 0, 0, 0])
        d0, g0, off = d0 + nd, g0 + ng, off + nd * ng
    table = _C.CocoProblems(rows, DEV)
    flat = lambda values, dtype, shape=(-1,): torch.from_numpy(np.asarray(values, dtype=dtype).reshape(shape)).to(DEV)   # noqa: E731
    det_boxes = flat([d[1] for im in images for d in im["dets"]], np.float64, (-1, 4))
    gt_boxes = flat([g[1] for im in images for g in im["gts"]], np.float64, (-1, 4))
    crowd = flat([g[2] for im in images for g in im["gts"]], np.uint8)
    det_cat = flat([d[0] for im in images for d in im["dets"]], np.int32)
    gt_cat = flat([g[0] for im in images for g in im["gts"]], np.int32)
    det_match = flat([d[2] + r[2] if d[2] >= 0 else -1 for im, r in zip(images, rows) for d in im["dets"]], np.int32)
    det_ignore = flat([d[3] for im in images for d in im["dets"]], np.uint8)
    iou = _C.coco_box_iou(det_boxes, gt_boxes, crowd, table)
    got = _C.error_types(iou, table, det_cat, det_match, det_ignore, gt_cat, crowd, t_f, t_b)
    torch.cuda.synchronize()
    host_iou = iou.cpu().numpy()
    want = ([], [], [])
    for im, r in zip(images, rows):
        block = host_iou[r[4]:r[4] + r[1] * r[3]].reshape(r[1], r[3]).tolist() if r[1] * r[3] else [[] for _ in range(r[1])]
        t, targets, missed = eref.classify(block, [d[0] for d in im["dets"]], [d[2] for d in im["dets"]], [d[3] for d in im["dets"]],
                                           [g[0] for g in im["gts"]], [g[2] for g in im["gts"]], t_f, t_b)
        want[0].extend(t)
        want[1].extend(x + r[2] if x >= 0 else -1 for x in targets)
        want[2].extend(missed)
    want = (np.asarray(want[0], np.uint8), np.asarray(want[1], np.int32), np.asarray(want[2], np.uint8))
    assert got[0].dtype == torch.uint8 and got[1].dtype == torch.int32 and got[2].dtype == torch.uint8
    return tuple(x.cpu().numpy() for x in got), want, got


def equal(got, want):
    return all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, want))


def names(types):
    return [eref.TYPES[t] for t in types]


def stride_image(num_gts, second=12):
    """``num_gts`` ground truths of alternating category, all poor (IoU .25) but the last two rows, which hold the best of
    their categories: row n - 1 IoU 10 / 11, row n - 2 IoU 10 / ``second``.  A detection of category 0 and one of category
    1, both unmatched: for one of them the last row is "same", for the other it is "other".  second = 12: both maxima are
    >= t_f, both detections are Cls and their targets show the "other" maxima; second = 25 (IoU .4): one is Dupe, one Loc,
    and their targets show the "same" maxima."""
    gts = [(j % 2, tall(40), 0) for j in range(num_gts)]
    gts[-1] = ((num_gts - 1) % 2, tall(11), 0)
    if num_gts > 1:
        gts[-2] = ((num_gts - 2) % 2, tall(second), 0)
    return image([(0, UNIT, -1, 0), (1, UNIT, -1, 0)], gts)


def mixed_images():
    rs = np.random.RandomState(5)
    random_gts = [(int(rs.randint(3)), [float(v) for v in np.r_[rs.randint(0, 40, 2), rs.randint(5, 30, 2)]], int(rs.rand() < .2))
                  for _ in range(7)]
    random_dets = []
    for _ in range(130):   # more detections than a block has waves, than a wave has lanes
        g = random_gts[rs.randint(7)]
        box = [g[1][0] + float(rs.randint(-5, 6)), g[1][1] + float(rs.randint(-5, 6)), max(1.0, g[1][2] + float(rs.randint(-6, 7))),
               max(1.0, g[1][3] + float(rs.randint(-6, 7)))]
        match = int(rs.randint(7)) if rs.rand() < .3 else -1
        random_dets.append((int(rs.randint(3)), box, match, int(match >= 0 and rs.rand() < .3)))
    images = [image([(0, UNIT, -1, 0), (2, tall(30), -1, 0)], []),                       # 0: no ground truth
              image([], [(0, UNIT, 0), (1, tall(20), 0), (1, tall(20), 1)]),             # 1: no detection
              stride_image(1), stride_image(63), stride_image(64), stride_image(65), stride_image(130),   # 2 .. 6
              image(random_dets, random_gts),                                            # 7: 130 detections
              image([(0, UNIT, -1, 0)], [(0, UNIT, 0)] * 3 + [(1, UNIT, 0)] * 2 + [(0, tall(40), 0)]),   # 8: ties
              image([(0, tall(20), 0, 0), (0, UNIT, -1, 0), (1, UNIT, -1, 0)], [(0, tall(20), 0)]),      # 9: IoU == t_f
              image([(0, UNIT, -1, 0), (1, UNIT, -1, 0)], [(0, tall(100), 0)]),          # 10: IoU == t_b
              image([(0, UNIT, -1, 0), (0, UNIT, 0, 1)], [(0, UNIT, 1), (1, UNIT, 1)]),  # 11: crowds at IoU 1
              image([(1, UNIT, -1, 0)], [(0, tall(25), 0)]),                             # 12: Both
              stride_image(63, 25), stride_image(64, 25), stride_image(65, 25), stride_image(130, 25)]   # 13 .. 16
    return images


@pytest.fixture(scope="module")
def mixed():
    """Every case side by side in ONE chunk -- so every image but the first has non-zero row and IoU offsets -- run once."""
    images = mixed_images()
    return images, run(images)


def test_error_types_equal_the_restatement(mixed):
    images, (got, want, _) = mixed
    assert equal(got, want)
    assert len(got[0]) == sum(len(im["dets"]) for im in images) and len(got[2]) == sum(len(im["gts"]) for im in images)
    first = sum(len(im["dets"]) for im in images[:7])
    assert set(got[0][first:first + 130].tolist()) == {0, 1, 2, 3, 4, 5}       # the random image has every type


def test_planted_cases_are_what_they_claim(mixed):
    images, (got, _, _) = mixed
    d0 = np.cumsum([0] + [len(im["dets"]) for im in images])
    g0 = np.cumsum([0] + [len(im["gts"]) for im in images])
    of = lambda i: (names(got[0][d0[i]:d0[i + 1]]), (got[1][d0[i]:d0[i + 1]] - g0[i]).tolist(), got[2][g0[i]:g0[i + 1]].tolist())   # noqa: E731
    assert got[0][:2].tolist() == [5, 5] and got[1][:2].tolist() == [-1, -1]           # no ground truth: all Bkg, targets -1
    assert got[2][g0[1]:g0[2]].tolist() == [1, 1, 0]                                   # no detection: all missed but the crowd
    # one ground truth of category 0 at IoU 10 / 11: Dupe for the detection of its class, Cls for the other
    assert of(2) == (["Dupe", "Cls"], [0, 0], [0])
    for i, n in ((3, 63), (4, 64), (5, 65), (6, 130)):   # the lane-stride edges: the best of each kind sits in the last rows
        same_last = (n - 1) % 2 == 0   # the last row is of category 0
        # detection 0 (category 0): s >= t_f is checked after o >= t_f -> Cls aimed at the best "other"
        assert of(i)[0] == ["Cls", "Cls"] and of(i)[1] == ([n - 2, n - 1] if same_last else [n - 1, n - 2]), n
        assert sum(of(i)[2]) == n - 2 and of(i)[2][-2:] == [0, 0], n
    for i, n in ((13, 63), (14, 64), (15, 65), (16, 130)):   # ... and the "same" maxima: Dupe at row n - 1, Loc at row n - 2
        same_last = (n - 1) % 2 == 0
        assert of(i)[:2] == ((["Dupe", "Loc"], [n - 1, n - 2]) if same_last else (["Loc", "Dupe"], [n - 2, n - 1])), n
        assert sum(of(i)[2]) == n - 1 and of(i)[2][-2:] == [0, 1], n   # a Dupe target that nobody matched is missed
    # ties: three "same" at IoU 1 (rows 0..2) and two "other" at IoU 1 (rows 3, 4): "other" wins as Cls, at the later row
    assert of(8) == (["Cls"], [4], [1, 1, 1, 1, 0, 1])
    # IoU exactly t_f: as "same" Dupe (its ground truth is taken), never Loc; as "other" Cls
    assert of(9) == (["none", "Dupe", "Cls"], [-1 - int(g0[9]), 0, 0], [0])
    # IoU exactly t_b: as "same" Loc; as "other" with s = 0 Bkg
    assert of(10) == (["Loc", "Bkg"], [0, -1 - int(g0[10])], [0])
    # crowds take no part: Bkg although both overlap fully; the ignored detection is no error; a crowd is never missed
    assert of(11) == (["Bkg", "none"], [-1 - int(g0[11])] * 2, [0, 0])
    assert of(12) == (["Both"], [-1 - int(g0[12])], [1])


def test_the_later_row_wins_among_equal_same_class_ious():
    got, want, _ = run([image([(0, UNIT, -1, 0)], [(0, tall(30), 0), (0, tall(30, 0.0), 0), (1, tall(50), 0), (0, tall(60), 0)])])
    assert equal(got, want) and names(got[0]) == ["Loc"] and got[1].tolist() == [1]


def test_single_images_and_thresholds_as_keywords():
    for n in (1, 130):   # 1 and 130 detections against 5 ground truths, an image alone in its chunk
        gts = [(j % 2, tall(12 + 7 * j), 0) for j in range(5)]
        dets = [(k % 3, tall(10 + k % 9), -1 if k % 4 else k % 5, 0) for k in range(n)]
        got, want, _ = run([image(dets, gts)])
        assert equal(got, want), n
    case = [image([(0, UNIT, -1, 0)], [(0, tall(25), 0)])]   # IoU .4
    assert names(run(case)[0][0]) == ["Loc"] and names(run(case, 0.4, 0.1)[0][0]) == ["Dupe"]
    assert names(run(case, 0.9, 0.45)[0][0]) == ["Bkg"]
    got, want, _ = run(case, 0.4, 0.1)
    assert equal(got, want)


def test_two_calls_give_the_same_bytes(mixed):
    images, (_, _, first) = mixed
    _, _, second = run(images)
    for a, b in zip(first, second):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_empty_call_launches_nothing_and_bad_arguments_are_einval(monkeypatch):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C, _lib
    lib = _C._L
    assert lib.ovis_error_types(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.5, 0.1, 0, 0, 0, 0, 0, 0) == _lib.OVIS_OK   # nothing at all
    table = _C.CocoProblems([[0, 0, 0, 0, 0, 0, 0, 0]], DEV)
    assert lib.ovis_error_types(0, table.dev.data_ptr(), 1, 0, 0, 0, 0, 0, 0, 0, 0.5, 0.1, 0, 0, 0, 0, 0, 0) == _lib.OVIS_OK
    buf = torch.zeros(64, dtype=torch.int64, device=DEV).data_ptr()
    bad = [dict(num_images=-1), dict(num_dets=-1), dict(num_gts=-1), dict(max_dets=-1), dict(max_gts=-1), dict(images=0),
           dict(det_category=0), dict(det_match=0), dict(det_ignore=0), dict(gt_category=0), dict(gt_crowd=0), dict(err_type=0),
           dict(err_gt=0), dict(gt_missed=0)]
    order = ("iou", "images", "num_images", "max_dets", "max_gts", "det_category", "det_match", "det_ignore", "gt_category",
             "gt_crowd", "t_f", "t_b", "num_dets", "num_gts", "err_type", "err_gt", "gt_missed", "stream")
    for change in bad:   # every one is refused before anything is launched: the buffers are never touched
        args = dict(iou=buf, images=table.dev.data_ptr(), num_images=1, max_dets=0, max_gts=0, det_category=buf, det_match=buf,
                    det_ignore=buf, gt_category=buf, gt_crowd=buf, t_f=0.5, t_b=0.1, num_dets=1, num_gts=1, err_type=buf,
                    err_gt=buf, gt_missed=buf, stream=0)
        args.update(change)
        assert lib.ovis_error_types(*[args[k] for k in order]) == _lib.OVIS_EINVAL, change

    def boom(*a):
        raise AssertionError("launched on an empty input")
    monkeypatch.setattr(lib, "ovis_error_types", boom)
    z = lambda dtype: torch.zeros(0, dtype=dtype, device=DEV)   # noqa: E731
    out = _C.error_types(z(torch.float64), _C.CocoProblems([], DEV), z(torch.int32), z(torch.int32), z(torch.uint8), z(torch.int32),
                         z(torch.uint8))
    assert [tuple(x.shape) for x in out] == [(0,), (0,), (0,)]
    out = _C.error_types(z(torch.float64), table, z(torch.int32), z(torch.int32), z(torch.uint8), z(torch.int32), z(torch.uint8))
    assert [tuple(x.shape) for x in out] == [(0,), (0,), (0,)]
    with pytest.raises(RuntimeError):   # a table that points outside the arrays is refused on the host
        _C.error_types(z(torch.float64), _C.CocoProblems([[0, 1, 0, 0, 0, 0, 0, 0]], DEV), z(torch.int32), z(torch.int32),
                       z(torch.uint8), z(torch.int32), z(torch.uint8))


def test_segm_image_level_words_through_score_chunk():
    """Two images of 15 x 20 and 45 x 60 in one chunk, masks as RLE on both sides: the image-level table addresses each
    image's words by its own words-per-mask.  The reference works on the dense masks."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import coco_eval
    rs = np.random.RandomState(2)

    def rle(mask):
        flat = np.asarray(mask, dtype=np.uint8).T.reshape(-1)
        cuts = np.flatnonzero(np.diff(flat)) + 1
        runs = np.diff(np.concatenate([[0], cuts, [len(flat)]])).tolist()
        return {"size": list(mask.shape), "counts": ([0] if flat[0] else []) + runs}

    def rect(h, w, y0, y1, x0, x1):
        m = np.zeros((h, w), dtype=bool)
        m[y0:y1, x0:x1] = True
        return m
    images, dets, reference = [], [], []
    for (h, w), scale in (((15, 20), 1), ((45, 60), 3)):
        s = scale
        gt_masks = [rect(h, w, 2 * s, 10 * s, 2 * s, 10 * s), rect(h, w, 3 * s, 12 * s, 11 * s, 19 * s), rect(h, w, 0, 2 * s, 0, 20 * s)]
        gt_cats, crowd = [0, 1, 1], [0, 0, 1]
        det_masks = [rect(h, w, 2 * s, 10 * s, 2 * s, 10 * s), rect(h, w, 2 * s, 10 * s, 2 * s, 9 * s), rect(h, w, 2 * s, 6 * s, 2 * s, 10 * s),
                     rect(h, w, 3 * s, 12 * s, 11 * s, 19 * s), rect(h, w, 12 * s, 15 * s, 0, 3 * s), rect(h, w, 0, 2 * s, 0, 10 * s),
                     rect(h, w, 4 * s, 12 * s, 8 * s, 14 * s) & (rs.rand(h, w) < .8)]
        det_cats, scores = [0, 0, 0, 0, 1, 1, 1], [.9, .8, .7, .6, .5, .4, .3]
        order = np.lexsort((-np.asarray(scores), det_cats))
        anns = [{"id": k, "segmentation": rle(m)} for k, m in enumerate(gt_masks)]
        images.append({"id": len(images), "width": w, "height": h, "anns": anns, "boxes": np.zeros((3, 4)), "polygons": 0,
                       "cats": np.asarray(gt_cats, np.int64), "areas": np.asarray([float(m.sum()) for m in gt_masks]),
                       "crowd": np.asarray(crowd, np.uint8)})
        dets.append({"cats": np.asarray(det_cats, np.int64)[order], "scores": np.asarray(scores)[order], "xywh": np.zeros((7, 4)),
                     "xyxy": None, "maps": None, "rle": [rle(det_masks[k]) for k in order], "entry": order})
        reference.append({"dets": [{"category": c, "score": sc, "mask": m} for c, sc, m in zip(det_cats, scores, det_masks)],
                          "gts": [{"category": c, "mask": m, "area": float(m.sum()), "iscrowd": k} for c, m, k in zip(gt_cats, gt_masks, crowd)]})
    plain = coco_eval.score_chunk(images, dets, "segm", torch.device(DEV))
    tables = coco_eval.score_chunk(images, dets, "segm", torch.device(DEV), error_thresholds=(0.5, 0.1))
    assert sorted(set(tables) - set(plain)) == ["det_image", "err_gt", "err_type", "gt_image", "gt_missed", "num_images"]
    for key in plain:
        assert np.array_equal(plain[key], tables[key]), key
    want = eref.rows(reference, "segm")
    assert tables["err_type"].tolist() == want["err_type"] and tables["err_gt"].tolist() == want["err_gt"]
    assert tables["gt_missed"].tolist() == [int(m) for m in want["gt_missed"]]
    assert tables["det_image"].tolist() == want["det_image"] and tables["gt_image"].tolist() == want["gt_image"]
    # both images hold the same scene at two scales: the same types, and not trivial ones
    assert names(tables["err_type"][:7]) == names(tables["err_type"][7:]) and len(set(names(tables["err_type"]))) >= 4
