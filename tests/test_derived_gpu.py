"""GPU: the device users of layers/derived.py follow their weights -- the RPN head's GEMM operands after writes no version
counter sees and after a ``.data`` swap -- and prepare a frozen weight once: the RPN head, ``linear_mfma``'s pair form (with no
entry left behind for a dead weight) and the box predictor's concatenated operand."""
import gc

import pytest
import torch
import torch.nn.functional as F

from cvpr22_cross_modal_pseudo_labeling_amd import _C
from cvpr22_cross_modal_pseudo_labeling_amd.layers import linear_mfma
from cvpr22_cross_modal_pseudo_labeling_amd.layers.derived import _STORE
from cvpr22_cross_modal_pseudo_labeling_amd.modeling.rpn import RPNHead

pytestmark = pytest.mark.gpu


@pytest.fixture
def splits(monkeypatch):
    """Shapes of the matrices ``_C.split_pair`` was asked to split, in call order."""
    shapes, real = [], _C.split_pair

    def counting(x, *args, **kwargs):
        shapes.append(tuple(x.shape))
        return real(x, *args, **kwargs)
    monkeypatch.setattr(_C, "split_pair", counting)
    return shapes


def _rpn_head(trainable):
    torch.manual_seed(9)
    head = RPNHead(64, 15).cuda()
    for p in head.parameters():
        p.data.normal_(0, 0.05)
        p.requires_grad = trainable
    return head, torch.randn(2, 64, 13, 21, device="cuda")


def _assert_head_matches_convolutions(head, x, obj, reg):
    """The bound of tests/test_split_gemm_pair.py::test_rpn_head_gemm_matches_convolutions, against the head's weights as they are."""
    t = F.relu(F.conv2d(x.double(), head.conv.weight.double(), head.conv.bias.double(), padding=1))
    obj_ref = F.conv2d(t, head.cls_logits.weight.double(), head.cls_logits.bias.double())
    reg_ref = F.conv2d(t, head.bbox_pred.weight.double(), head.bbox_pred.bias.double())
    assert obj.shape == obj_ref.shape and reg.shape == reg_ref.shape
    assert (obj.double() - obj_ref).abs().max().item() <= 1e-5 * obj_ref.abs().max().item()
    assert (reg.double() - reg_ref).abs().max().item() <= 1e-5 * reg_ref.abs().max().item()


@torch.no_grad()
def test_trainable_rpn_head_follows_writes_no_version_counter_sees():
    """Evaluation between optimizer steps (the fused SGD writes through raw pointers): the operands are those of the weights now."""
    head, x = _rpn_head(trainable=True)
    assert head._gemm_ok(x)
    _assert_head_matches_convolutions(head, x, *head(x))
    versions = [p._version for p in head.parameters()]
    for p in head.parameters():
        p.data.normal_(0, 0.05)
    assert [p._version for p in head.parameters()] == versions
    _assert_head_matches_convolutions(head, x, *head(x))


def test_frozen_rpn_head_prepares_once_and_follows_a_data_swap(splits):
    head, x = _rpn_head(trainable=False)
    assert head._gemm_ok(x)
    rows = (x.shape[0] * x.shape[2] * x.shape[3], x.shape[1])
    obj, reg = head(x)
    assert len(splits) == 3 and rows in splits  # the activation, the 3x3 and the concatenated 1x1 weights
    del splits[:]
    obj2, reg2 = head(x)
    assert splits == [rows]  # the activation only
    assert torch.equal(obj, obj2) and torch.equal(reg, reg2)
    for p in head.parameters():
        p.data = torch.randn_like(p) * 0.05
    _assert_head_matches_convolutions(head, x, *head(x))


def test_linear_mfma_prepares_a_frozen_weight_once_and_keeps_no_dead_entry(splits):
    torch.manual_seed(3)
    x = torch.randn(4, 128, device="cuda")
    w = torch.randn(32, 128, device="cuda") * 0.1
    y = linear_mfma(x, w)
    assert splits == [(4, 128), (128, 128)]  # x, and the weight padded to the GEMM's 128-row tile
    ref = x.double() @ w.double().t()
    assert (y.double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item()
    del splits[:]
    assert torch.equal(linear_mfma(x, w), y) and splits == [(4, 128)]
    gc.collect()
    before = len(_STORE)
    for i in range(200):
        linear_mfma(x, torch.full((32, 128), float(i), device="cuda"))
    gc.collect()
    assert len(_STORE) <= before  # every one of the 200 weights is dead


def test_frozen_box_predictor_concatenates_and_splits_its_weight_once(splits, monkeypatch):
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling import roi_heads as RH
    from tests.test_components import small_cfg

    torch.manual_seed(5)
    pred = RH.FastRCNNPredictor(small_cfg(), 128).cuda()
    for p in pred.parameters():
        p.requires_grad = False
    pred.set_class_embeddings(torch.randn(5, pred.emb_dim, device="cuda"))
    x = torch.randn(4, 128, device="cuda")
    padded = (128, 128)  # the [48 + 8, 128] weights of emb_pred and bbox_pred, zero rows up to the GEMM's 128-row tile
    cats, real_cat = [], torch.cat

    def counting_cat(tensors, *args, **kwargs):
        out = real_cat(tensors, *args, **kwargs)
        cats.append(tuple(out.shape))
        return out
    monkeypatch.setattr(torch, "cat", counting_cat)
    logits, box = pred(x)
    assert cats.count(padded) == 1 and splits.count(padded) == 1
    del cats[:], splits[:]
    logits2, box2 = pred(x)
    assert padded not in cats and padded not in splits
    assert torch.equal(logits, logits2) and torch.equal(box, box2)
