"""CPU: the Soft-NMS restatement (tests/soft_nms_reference.py) against hand-computed cases written out as literals, and the host
twin (``ovis_cpu_soft_nms_f32`` through ``_C.soft_nms`` on host tensors) against the restatement, bit for bit."""
import numpy as np
import pytest
import torch

from tests import soft_nms_reference as R

METHODS = ("linear", "gaussian", "hard")


def _twin(packed, method, nt, sigma, min_score):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    got = _C.soft_nms(*(torch.from_numpy(a) for a in packed), method=method, nms_thresh=nt, sigma=sigma, min_score=min_score)
    assert not got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == (packed[0].shape[0],)
    return got.numpy()


def _same_bits(got, want, what):
    got, want = R.bits(got), R.bits(want)
    assert got.shape == want.shape and (got == want).all(), (what, np.nonzero(got != want)[0][:8].tolist())


@pytest.mark.parametrize("name", list(R.PLANTED))
def test_restatement_and_host_twin_on_the_planted_cases(name):
    packed, method, nt, sigma, min_score, want = R.PLANTED[name]
    _same_bits(R.soft_nms(*packed, method, nt, sigma, min_score), want, name + ": restatement")
    _same_bits(_twin(packed, method, nt, sigma, min_score), want, name + ": host twin")


def test_the_planted_cases_show_what_they_claim():
    """The order of selection does change, the tie does go to the lower index, and so on: read off the literals."""
    want = {name: case[5] for name, case in R.PLANTED.items()}
    assert want["decay_reorders"][1] < want["decay_reorders"][2]                    # B fell below C
    assert want["decays_in_turn"][3] < 0.9375 * 0.5 * 0.5                            # more than two decays' worth
    assert want["exactly_min_score_is_kept"][1] == R.PLANTED["exactly_min_score_is_kept"][4] == 0.0625
    assert want["one_float_below_min_score_is_discarded"][1] == 0.0
    assert want["iou_at_nt_linear"][1] == 0.5 and want["iou_at_nt_linear"][3] < 0.5 and want["iou_at_nt_linear"][5] == 0.5
    for name in ("tie_lower_index_first", "tie_lower_index_first_reversed"):
        assert want[name] == [0.5, 0.25]
    assert want["gaussian_decays_all_overlaps"][2] == float(np.float32(0.3))        # the disjoint one keeps its bits


@pytest.mark.parametrize("method", METHODS)
def test_host_twin_equals_restatement_on_clustered_runs(method):
    """Runs of 0 ... 70 candidates around three base boxes: decays compound, discards are frequent (asserted)."""
    packed = R.clustered(31, [0, 17, 1, 0, 70, 2, 33, 0])
    for nt, sigma, min_score in ((0.5, 0.5, 0.05), (0.3, 0.25, 0.0)):
        want = R.soft_nms(*packed, method, nt, sigma, min_score)
        _same_bits(_twin(packed, method, nt, sigma, min_score), want, (method, nt))
        decayed = (want > 0) & (want < packed[1])
        assert (method == "hard" or decayed.any()) and (want <= packed[1]).all()
        assert (want == 0).any() or (min_score == 0.0 and method != "hard")   # a soft decay alone never reaches 0


@pytest.mark.parametrize("method", METHODS)
def test_the_array_form_of_the_restatement_has_the_same_bits(method):
    """``soft_nms_run_rows`` (what the GPU tests use for runs of thousands) against the scalar loops, planted cases included."""
    packed = R.clustered(36, [0, 70, 1, 129, 2])
    for nt, sigma, min_score in ((0.5, 0.5, 0.05), (0.3, 0.25, 0.0)):
        _same_bits(R.soft_nms(*packed, method, nt, sigma, min_score, run=R.soft_nms_run_rows),
                   R.soft_nms(*packed, method, nt, sigma, min_score), (method, nt))
    for name, (planted, m, nt, sigma, min_score, want) in R.PLANTED.items():
        _same_bits(R.soft_nms(*planted, m, nt, sigma, min_score, run=R.soft_nms_run_rows), want, name)


def test_hard_with_min_score_zero_is_the_greedy_nms():
    packed = R.clustered(32, [40, 0, 65, 9])
    boxes, scores, offsets = packed
    for nt in (0.3, 0.5, 0.7):
        soft = R.soft_nms(*packed, "hard", nt, 0.5, 0.0)
        twin = _twin(packed, "hard", nt, 0.5, 0.0)
        for g in range(len(offsets) - 1):
            lo, hi = int(offsets[g]), int(offsets[g + 1])
            keep = R.greedy_nms_keep(boxes[lo:hi], scores[lo:hi], nt)
            assert 0 < len(keep) < hi - lo or hi == lo
            for got in (soft, twin):
                assert np.nonzero(got[lo:hi] > 0)[0].tolist() == keep
                _same_bits(got[lo:hi][keep], scores[lo:hi][keep], "survivors keep their scores")


def test_hard_with_min_score_zero_keeps_what_the_package_nms_keeps():
    """Against the host NMS the package already ships (``>=`` there: a threshold no IoU of the input equals)."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    boxes, scores, offsets = R.clustered(33, [120])
    ious = {float(R.iou32(a, b)) for a in boxes[:40] for b in boxes[:40]}
    nt = 0.45
    assert nt not in ious
    keep = _C.nms(torch.from_numpy(boxes), torch.from_numpy(scores), nt)
    soft = _twin((boxes, scores, offsets), "hard", nt, 0.5, 0.0)
    assert np.nonzero(soft > 0)[0].tolist() == keep.tolist()


def test_wrapper_refuses_what_it_cannot_serve():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    boxes, scores, offsets = (torch.from_numpy(a) for a in R.clustered(34, [5, 3]))
    with pytest.raises(ValueError, match="method"):
        _C.soft_nms(boxes, scores, offsets, method="exponential")
    with pytest.raises(ValueError, match="sigma"):
        _C.soft_nms(boxes, scores, offsets, sigma=0.0)
    with pytest.raises(ValueError, match="min_score"):
        _C.soft_nms(boxes, scores, offsets, min_score=-0.1)
    with pytest.raises(RuntimeError, match="expected"):
        _C.soft_nms(boxes, scores, offsets.long())
    with pytest.raises(RuntimeError, match="expected"):
        _C.soft_nms(boxes, scores[:-1], offsets)
    empty = _C.soft_nms(boxes[:0], scores[:0], torch.zeros(4, dtype=torch.int32))
    assert tuple(empty.shape) == (0,) and empty.dtype == torch.float32
    # malformed offsets on the host: refused, and nothing is read through them
    for bad in ([0, 5, 7], [0, 9, 8], [1, 5, 8], [0, -1, 8], [0, 6, 5, 8]):
        with pytest.raises(RuntimeError, match="offsets"):
            _C.soft_nms(boxes, scores, torch.tensor(bad, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="offsets"):
        _C.soft_nms(boxes, scores, torch.zeros(1, dtype=torch.int32))


def test_host_twin_serves_the_runs_in_front_of_the_damage():
    """The library entry itself: status OVIS_CPU_ERANGE, the well-formed runs in front of the first bad entry right, zeros
    from there on."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _cpu

    boxes, scores, offsets = R.clustered(35, [20, 12, 30])
    want = R.soft_nms(boxes, scores, offsets, "linear", 0.5, 0.5, 0.05)
    lib = _cpu.load()
    def run(bad):
        off = torch.tensor(bad, dtype=torch.int32)
        out = torch.full((62,), 7.0)
        rc = lib.ovis_cpu_soft_nms_f32(boxes.ctypes.data, scores.ctypes.data, off.data_ptr(), 62, 3, 0, 0.5, 0.5, 0.05,
                                       out.data_ptr())
        assert rc == _cpu.CONSTANTS["OVIS_CPU_ERANGE"], bad
        return out.numpy()

    for bad, good_until in (([0, 20, 19, 62], 20), ([0, 20, -3, 62], 20), ([0, 20, 32, 63], 32), ([2, 20, 32, 62], 0)):
        out = run(bad)
        _same_bits(out[:good_until], want[:good_until], bad)
        assert (out[good_until:] == 0).all(), bad
    # a last entry short of K: every run is well-formed and served as it is given, the candidate behind them gets 0
    short = [0, 20, 32, 61]
    out = run(short)
    _same_bits(out[:61], R.soft_nms(boxes[:61], scores[:61], short, "linear", 0.5, 0.5, 0.05), short)
    assert out[61] == 0


def test_the_rule_is_in_the_header_and_the_documents():
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "ovis_hip.h")) as f:
        header = " ".join(f.read().split())
    for phrase in ("ovis_soft_nms_f32", "ties go to the LOWER candidate index", "rounded ONCE to float32",
                   "OVIS_SOFT_NMS_LDS_CANDIDATES", "counts as discarded"):
        assert phrase in header, phrase
    for name in ("README.md", "DESIGN.md"):
        with open(os.path.join(root, name)) as f:
            text = " ".join(f.read().split())
        assert "--soft-nms" in text and "Soft-NMS" in text, name
