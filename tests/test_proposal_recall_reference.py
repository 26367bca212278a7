"""CPU: box-proposal recall.  The NumPy float32 restatement (tests/proposal_recall_reference.py) against the fixture the
REFERENCE's own ``evaluate_box_proposals`` wrote (tests/golden/proposal_recall.npz, made by
tests/golden/make_proposal_recall_golden.py): the sorted overlaps bit-equal, ``num_pos`` equal, AR within 1e-6 -- the margin
covers only the summation order of the fp32 mean of ten recalls <= 1 (nine additions, each within 2^-24 of a sum < 10).
Then hand-derived cases of the tie rules, the host half of the product (engine/proposal_recall.py) and the command line."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import proposal_recall_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AREAS = ("all", "small", "medium", "large")


@pytest.fixture(scope="module")
def fixture():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "proposal_recall.npz")))


def test_thresholds_are_the_reference_arange():
    want = torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32).numpy()
    assert ref.THRESHOLDS.dtype == np.float32 and np.array_equal(ref.THRESHOLDS, want) and len(want) == 10


def test_restatement_equals_the_reference_fixture(fixture):
    assert fixture["areas"].tolist() == list(AREAS) and fixture["limits"].tolist() == list(ref.LIMITS)
    rows = ref.fixture_rows(fixture)
    assert len(rows) == 5 and sorted(len(r["props"]) for r in rows) == [0, 5, 60, 200, 1000]
    table = ref.overlaps_table(rows)
    assert table.dtype == np.float32 and table.shape == (4, 2, sum(len(r["gt_boxes"]) for r in rows))
    results = ref.evaluate(rows)
    # the reference's vector leaves out the ground truths of an image without proposals (coco_eval.py:266-267 comes before
    # the append); they are positives all the same (:261), recorded here as zeros
    proposed = np.concatenate([np.full(len(r["gt_boxes"]), len(r["props"]) > 0) for r in rows])
    assert 0 < np.count_nonzero(~proposed) < len(proposed)
    for l, limit in enumerate(ref.LIMITS):
        for a, area in enumerate(AREAS):
            ar, num_pos, _ = ref.average_recall(table[a, l])
            overlaps = ref.average_recall(table[a, l][proposed])[2]
            want = fixture[f"gt_overlaps_{area}_{limit}"]
            assert num_pos == int(fixture[f"num_pos_{area}_{limit}"]) >= 5 and np.all(table[a, l][~proposed] <= 0)
            assert overlaps.dtype == want.dtype == np.float32 and np.array_equal(overlaps.view(np.int32), want.view(np.int32)), \
                (area, limit)
            assert abs(ar - float(fixture[f"ar_{area}_{limit}"])) <= 1e-6, (area, limit, ar)
            assert results[f"AR{ref.AREA_SUFFIXES[a]}@{limit}"] == ar
    assert list(results) == ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"]
    assert results["AR@100"] != results["AR@1000"] and 0.3 < results["AR@1000"] < 0.8


def test_matrix_equals_the_scalar_formula():
    rs = np.random.RandomState(0)
    xy = rs.rand(40, 2).astype(np.float32) * 50
    boxes = np.concatenate([xy, xy + rs.rand(40, 2).astype(np.float32) * 40], 1)
    m = ref.iou_matrix(boxes[:25], boxes[25:])
    for i in range(25):
        for j in range(15):
            assert m[i, j] == ref.box_iou(boxes[i], boxes[25 + j]) and isinstance(ref.box_iou(boxes[i], boxes[25 + j]), np.float32)
    assert ref.box_iou([0, 0, 9, 9], [0, 0, 9, 9]) == 1 and ref.box_iou([0, 0, 9, 9], [10, 0, 19, 9]) == 0
    assert ref.box_iou([0, 0, 9, 9], [5, 0, 14, 9]) == np.float32(50) / np.float32(150)    # TO_REMOVE = 1: widths are 10


def test_tie_rules_and_fallback_by_hand():
    gts = [[0, 0, 9, 9], [100, 0, 109, 9]]
    areas = [100, 100]
    # two identical proposals on ground truth 0 and nothing on 1: round 1 takes (gt 0, proposal 0) at IoU 1; round 2 has
    # only zeros left and consumes the first live proposal for ground truth 1, recording 0
    out = ref.gt_overlaps([[0, 0, 9, 9], [0, 0, 9, 9]], gts, areas, ref.AREA_RANGES[0], 100)
    assert out.tolist() == [1.0, 0.0]
    # equally covered ground truths: the lowest index goes first -- and takes the only proposal
    out = ref.gt_overlaps([[0, 0, 109, 9]], gts, areas, ref.AREA_RANGES[0], 100)
    assert out[0] == ref.box_iou([0, 0, 109, 9], gts[0]) == ref.box_iou([0, 0, 109, 9], gts[1]) and out[1] == 0
    # ground truth 1's best proposal (0) is taken by the better-covered ground truth 0: it falls back to proposal 1
    gts = [[0, 0, 9, 9], [2, 0, 11, 9]]
    props = [[0, 0, 9, 9], [5, 0, 14, 9]]
    m = ref.iou_matrix(props, gts)
    assert m[0, 0] == 1 and m[0, 1] > m[1, 1] > 0
    assert ref.gt_overlaps(props, gts, areas, ref.AREA_RANGES[0], 100).tolist() == [1.0, float(m[1, 1])]
    # the limit cuts the list, the area range marks with -1, both bounds inclusive
    assert ref.gt_overlaps(props, gts, areas, ref.AREA_RANGES[0], 1).tolist() == [1.0, 0.0]
    assert ref.gt_overlaps(props, gts, [1024, 1025], ref.AREA_RANGES[1], 100).tolist() == [1.0, -1.0]
    assert ref.gt_overlaps(props, gts, [1024, 9216], ref.AREA_RANGES[2], 100).tolist() == [1.0, float(m[1, 1])]
    assert ref.average_recall([-1, -1])[:2] == (-1.0, 0)
    assert ref.average_recall([1.0, 0.0, -1.0])[:2] == (0.5, 2)


def test_host_average_recall_is_the_reference_arithmetic(fixture):
    """The product's host half on the reference's own overlaps gives the reference's AR exactly: the same torch calls."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import proposal_recall

    assert proposal_recall.LIMITS == ref.LIMITS and proposal_recall.AREA_SUFFIXES == ref.AREA_SUFFIXES
    assert np.array_equal(np.asarray(proposal_recall.AREA_RANGES, dtype=np.float32), np.asarray(ref.AREA_RANGES, dtype=np.float32))
    assert proposal_recall.AREA_RANGES[0][1] == 1e5 ** 2
    for limit in ref.LIMITS:
        for area in AREAS:
            values = torch.from_numpy(fixture[f"gt_overlaps_{area}_{limit}"])
            missing = int(fixture[f"num_pos_{area}_{limit}"]) - len(values)   # positives of the image without proposals
            assert missing >= 0
            # ... enter as zeros; ground truths outside the range (-1) do not count
            padded = torch.cat([values, torch.zeros(missing), torch.full((3,), -1.0)])
            assert proposal_recall.average_recall(padded) == float(fixture[f"ar_{area}_{limit}"])
    assert proposal_recall.average_recall(torch.full((4,), -1.0)) == -1.0
    assert proposal_recall.average_recall(torch.zeros(0)) == -1.0


def test_evaluate_box_proposals_refuses_the_host():
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import proposal_recall

    with pytest.raises(ValueError):
        proposal_recall.evaluate_box_proposals(None, [], "cpu")


def test_proposal_gt_overlaps_refuses_host_tensors():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C, _lib

    assert _lib.OVIS_PROPOSAL_RECALL_MAX_LIMIT >= 1000 and _lib.OVIS_PROPOSAL_RECALL_MAX_GTS >= 70
    with pytest.raises(RuntimeError):
        _C.proposal_gt_overlaps(torch.zeros(1, 4), torch.zeros(1, 4), torch.zeros(1), [[0, 1, 0, 1]], torch.zeros(1, 2), [100])


def _tool(name):
    spec = importlib.util.spec_from_file_location(f"ovis_tool_{name}", os.path.join(ROOT, "tools", f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_recall_flags_are_command_line_errors_without_what_they_need(tmp_path, capsys):
    tool = _tool("infer_net")
    argv = ["--dataset-catalog", str(tmp_path / "none.json")]
    cases = ((["--recall", "MODEL.DEVICE", "cuda", "OUTPUT_DIR", str(tmp_path)], "give --evaluate"),
             (["--rpn-recall", "MODEL.DEVICE", "cuda", "OUTPUT_DIR", ""], "set OUTPUT_DIR"),
             (["--rpn-recall", "MODEL.DEVICE", "cpu", "OUTPUT_DIR", str(tmp_path)], "set MODEL.DEVICE cuda"),
             (["--rpn-recall", "--evaluate", "MODEL.DEVICE", "cuda", "OUTPUT_DIR", str(tmp_path)], "makes no detections"))
    for opts, word in cases:
        with pytest.raises(SystemExit) as e:
            tool.main(argv + opts)
        assert e.value.code == 2 and word in capsys.readouterr().err, opts
    assert not os.listdir(tmp_path)
