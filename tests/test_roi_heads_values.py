"""The RoI heads take what a pass needs as values: the class-embedding matrix is an argument of the predictor (no forward
pass writes ``FastRCNNPredictor.cls_score``), the sampled proposal lists are ``SampledBoxList`` records that declare where
their positives sit, and the box loss takes the lists it belongs to as an argument."""
import contextlib
import os

import pytest
import torch

from cvpr22_cross_modal_pseudo_labeling_amd.modeling import roi_heads as RH
from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList, SampledBoxList, box_iou, cat_boxlist
from tests.test_components import small_cfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICES = [pytest.param("cpu"), pytest.param("cuda", marks=pytest.mark.gpu)]


def _ops(device):
    """Host tensors: the native ops routed to the oracle (as every host test does); device tensors: the HIP library."""
    if device == "cpu":
        from tests.oracle_backend import oracle_ops
        return oracle_ops()
    return contextlib.nullcontext()


# ------------------------------------------------------------------------------------------------------------------
# class embeddings
# ------------------------------------------------------------------------------------------------------------------
def test_no_forward_pass_writes_a_class_matrix(monkeypatch):
    """One training step's forward and one evaluation forward of the tiny student-teacher model: ``set_class_embeddings`` of
    a predictor is not called, ``cls_score`` of a predictor is not assigned, both predictors hold the objects they held."""
    from tests.tiny_model import build_tiny

    model, e_vocab, e_seen, images, targets = build_tiny("student_teacher_mask_rcnn_uncertainty", batch=1)
    model.set_class_embeddings(e_seen)
    model.set_caption_vocab(e_vocab)
    teacher, student = model.roi_heads["box"].predictor, model.roi_heads_student["box"].predictor
    before = (teacher.cls_score, student.cls_score)
    assert torch.is_tensor(before[0])

    calls, writes = [], []
    set_embs, set_attr = RH.FastRCNNPredictor.set_class_embeddings, RH.FastRCNNPredictor.__setattr__

    def counted_set(self, embs):
        calls.append(self)
        return set_embs(self, embs)

    def counted_setattr(self, name, value):
        if name == "cls_score":
            writes.append(self)
        return set_attr(self, name, value)

    monkeypatch.setattr(RH.FastRCNNPredictor, "set_class_embeddings", counted_set)
    monkeypatch.setattr(RH.FastRCNNPredictor, "__setattr__", counted_setattr)
    with _ops("cpu"):
        losses = model(images, targets)
        model.eval()
        with torch.no_grad():
            detections = model(images)
    assert len(losses) == 6 and len(detections) == len(targets)
    assert calls == [] and writes == []
    assert teacher.cls_score is before[0] and student.cls_score is before[1]
    assert not hasattr(model, "_seen_cls")
    model.set_class_embeddings(e_seen)  # the wrappers do count
    assert calls == [teacher] and writes == [teacher]


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("c", [1, 49])  # the teacher's dummy matrix; no multiple of the GEMM's 128-column pad
def test_predictor_takes_the_class_matrix_as_an_argument(device, c):
    g = torch.Generator().manual_seed(c)
    cfg = small_cfg()
    pred = RH.FastRCNNPredictor(cfg, 96).to(device)
    x = torch.randn(5, 96, generator=g).to(device)  # below one 128-row tile
    embs = torch.randn(c, cfg.MODEL.ROI_BOX_HEAD.EMB_DIM, generator=g).to(device)
    other = torch.randn(7, cfg.MODEL.ROI_BOX_HEAD.EMB_DIM, generator=g).to(device)
    with _ops(device), torch.no_grad():
        pred.set_class_embeddings(other)
        logits, deltas = pred(x, cls_embs=embs)
        assert pred.cls_score is other  # the stored matrix is neither used nor replaced
        pred.set_class_embeddings(embs)
        want_logits, want_deltas = pred(x)
    assert logits.shape == (5, c) and torch.equal(logits, want_logits) and torch.equal(deltas, want_deltas)


# ------------------------------------------------------------------------------------------------------------------
# sampled proposals
# ------------------------------------------------------------------------------------------------------------------
SIZE = (240, 200)  # (width, height)
N_PROPOSALS = 40
JITTER = torch.tensor([[3.0, -2.0, 4.0, 1.0], [-4.0, 3.0, -2.0, -3.0], [2.0, 2.0, -3.0, 4.0]])  # IoU with the box > 0.8


def _background(n):
    """10 x 10 boxes on a grid: IoU with a ground-truth box of 70 px and more is below 0.03."""
    i = torch.arange(n, dtype=torch.float32)
    x, y = 4 + 28 * (i % 8), 4 + 36 * (i // 8)
    return torch.stack([x, y, x + 9, y + 9], 1)


def _scene(gt, labels, jitters_per_gt, first_positive_row):
    """-> (proposals [40, 4], ground-truth boxes, labels): ``jitters_per_gt`` proposals around every ground-truth box, put
    behind ``first_positive_row`` background boxes, the other background boxes behind them."""
    gt = torch.tensor(gt, dtype=torch.float32)
    near = (gt[:, None, :] + JITTER[None, :jitters_per_gt, :]).reshape(-1, 4)
    bg = _background(N_PROPOSALS - near.shape[0])
    return torch.cat([bg[:first_positive_row], near, bg[first_positive_row:]], 0), gt, torch.tensor(labels)


SCENES = {
    "A": _scene([[20, 20, 90, 90], [120, 30, 200, 100], [40, 110, 130, 180]], [1, 2, 3], 3, 10),  # 9 positives > quota 4
    "B": _scene([[60, 50, 150, 140]], [2], 2, 5),                                                # 2 positives < quota
    "C": _scene([[100, 60, 180, 150]], [1], 0, 0),                                               # none
}
POSITIVES = {"A": 9, "B": 2, "C": 0}
GROUPS = (("A", "B"), ("C", "A"))
QUOTA, PER_IMAGE = 4, 16


def _sampler_cfg():
    cfg = small_cfg()
    cfg.merge_from_list(["MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", PER_IMAGE, "MODEL.ROI_HEADS.POSITIVE_FRACTION", 0.25])
    return cfg


def _group(names, device):
    props, tgts = [], []
    for n in names:
        boxes, gt, labels = SCENES[n]
        props.append(BoxList(boxes.clone(), SIZE).to(device))
        t = BoxList(gt.clone(), SIZE)
        t.add_field("labels", labels.clone())
        tgts.append(t.to(device))
    return props, tgts


def _evaluator(device, device_sampler):
    ev = RH.FastRCNNLossComputation(_sampler_cfg())
    ev.device_sampler = device_sampler
    ev.generator = torch.Generator(device=device).manual_seed(7)
    return ev


def test_scenes_have_the_stated_positives():
    rh = _sampler_cfg().MODEL.ROI_HEADS
    assert int(rh.BATCH_SIZE_PER_IMAGE * rh.POSITIVE_FRACTION) == QUOTA
    for name, (boxes, gt, _) in SCENES.items():
        best = box_iou(gt, boxes).max(0).values
        assert boxes.shape == (N_PROPOSALS, 4) and int((best >= rh.FG_IOU_THRESHOLD).sum()) == POSITIVES[name], name
        assert float(best[best < rh.FG_IOU_THRESHOLD].max()) < min(rh.BG_IOU_THRESHOLD, 0.03)  # the others: background
    assert POSITIVES["A"] >= 8 and POSITIVES["B"] == 2 < QUOTA and POSITIVES["C"] == 0


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("device_sampler", [True, False])
def test_sampled_lists_declare_their_positives(device, device_sampler):
    ev = _evaluator(device, device_sampler)
    with _ops(device):
        sampled = ev.subsample_many([_group(names, device) for names in GROUPS])
    assert [len(g) for g in sampled] == [2, 2] and ev._proposals is sampled[-1]
    by_index = device == "cuda" and device_sampler  # the device sampler knows the rows; the tensor-op sampler does not
    for names, lists in zip(GROUPS, sampled):
        for name, s in zip(names, lists):
            labels = s.get_field("labels")
            want = torch.nonzero(labels > 0).squeeze(1)
            assert type(s) is SampledBoxList and s.all_positive is False and len(s) == PER_IMAGE
            assert want.numel() == min(POSITIVES[name], QUOTA)
            if by_index:
                assert s.pos_index.dtype == torch.int64 and torch.equal(s.pos_index, want)
            else:
                assert s.pos_index is None
            # a list with other rows is a plain BoxList: the index does not travel where it would be wrong
            for other in (s[torch.arange(3, device=device)], s[labels > 0], s.copy_with_fields(["labels"]),
                          cat_boxlist([s, lists[0]])):
                assert type(other) is BoxList and not hasattr(other, "pos_index") and not hasattr(other, "all_positive")
            moved = s.to("cpu")
            assert type(moved) is SampledBoxList and moved.all_positive is False and torch.equal(moved.bbox, s.bbox.cpu())
            assert (moved.pos_index is None) if not by_index else torch.equal(moved.pos_index, want.cpu())
    if by_index:
        assert RH.positives_index(sampled[0]).tolist() == (
            sampled[0][0].pos_index.tolist() + (sampled[0][1].pos_index + PER_IMAGE).tolist())
        assert sampled[1][0].pos_index.numel() == 0
        positives = RH.positive_proposals(sampled[0][0])
        assert type(positives) is SampledBoxList and positives.all_positive is True and positives.pos_index is None
        assert torch.equal(positives.bbox, sampled[0][0].bbox[sampled[0][0].pos_index])
    else:
        assert RH.positives_index(sampled[0]) is None


def test_to_keeps_a_declared_index_on_host_tensors():
    boxes, _, _ = SCENES["B"]
    plain = BoxList(boxes, SIZE)
    plain.add_field("labels", (torch.arange(N_PROPOSALS) % 7 == 0).long())
    index = torch.nonzero(plain.get_field("labels") > 0).squeeze(1)
    s = SampledBoxList(plain, index)
    assert s.fields() == ["labels"] and s.get_field("labels") is plain.get_field("labels") and s.bbox is plain.bbox
    moved = s.to("cpu")
    assert type(moved) is SampledBoxList and torch.equal(moved.pos_index, index) and moved.all_positive is False
    assert type(s[index]) is BoxList and not hasattr(s[index], "pos_index")
    assert any(t is index for t in s.device_tensors()) and not any(t is index for t in plain.device_tensors())


@pytest.mark.parametrize("device", DEVICES)
@pytest.mark.parametrize("device_sampler", [True, False])
def test_box_loss_takes_its_proposals_as_an_argument(device, device_sampler):
    """The loss of group 0, asked for after ``subsample_many`` stored the LAST group, against the reference's protocol
    (``subsample`` of group 0 alone, then the call without proposals) with the same sampler seed."""
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(2 * PER_IMAGE, 5, generator=g).to(device)
    deltas = torch.randn(2 * PER_IMAGE, 8, generator=g).to(device)
    with _ops(device):
        ev = _evaluator(device, device_sampler)
        sampled = ev.subsample_many([_group(names, device) for names in GROUPS])
        got = ev(logits, deltas, proposals=sampled[0])
        assert ev._proposals is sampled[1]
        ref = _evaluator(device, device_sampler)
        alone = ref.subsample(*_group(GROUPS[0], device))
        want = ref(logits, deltas)
    assert all(torch.equal(a.bbox, b.bbox) for a, b in zip(alone, sampled[0]))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert float(got[0]) > 0 and float(got[1]) > 0
    with _ops(device):
        last = ev(logits, deltas)  # the stored lists are those of the last group: other labels, another loss
    assert not torch.equal(last[0], got[0])


# ------------------------------------------------------------------------------------------------------------------
# the trainer's stream bookkeeping
# ------------------------------------------------------------------------------------------------------------------
def test_trainer_does_not_name_the_sampled_index():
    with open(os.path.join(ROOT, "cvpr22_cross_modal_pseudo_labeling_amd", "engine", "trainer.py")) as f:
        assert "pos_index" not in f.read()


@pytest.mark.gpu
def test_record_stream_visits_the_index_of_a_sampled_list(monkeypatch):
    """``Tensor.record_stream`` only takes device tensors, hence the marker; the stream is a stub that records."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import trainer

    ev = _evaluator("cuda", True)
    (s, _), = ev.subsample_many([_group(GROUPS[0], "cuda")])
    assert s.pos_index.numel() == QUOTA
    visited, stub = [], object()
    monkeypatch.setattr(torch.Tensor, "record_stream", lambda self, stream: visited.append((self, stream)))
    trainer._record_stream({"proposals": [s]}, stub)
    assert all(stream is stub for _, stream in visited)
    for t in (s.pos_index, s.bbox, s.get_field("labels"), s.get_field("regression_targets"), s.get_field("matched_gt")):
        assert sum(v is t for v, _ in visited) == 1
