"""CPU: host-side components of the hot path against fixtures produced by the reference's own Python
modules (tests/golden/make_golden.py::gen_heads), plus the config surface and a tiny end-to-end step
with the native ops routed to the oracle (tests/oracle_backend.py)."""
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
from cvpr22_cross_modal_pseudo_labeling_amd.modeling import roi_heads as RH
from cvpr22_cross_modal_pseudo_labeling_amd.modeling.box_coder import BoxCoder
from cvpr22_cross_modal_pseudo_labeling_amd.modeling.matcher import Matcher
from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList, box_iou

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "heads.npz"))


def T(a):
    return torch.from_numpy(np.asarray(a))


def small_cfg(**over):
    cfg = get_defaults()
    cfg.merge_from_file(os.path.join(ROOT, "configs/coco_cap_det/student_teacher_mask_rcnn_uncertainty.yaml"))
    cfg.merge_from_list(["MODEL.ROI_BOX_HEAD.EMB_DIM", 48, "MODEL.ROI_MASK_HEAD.CONV_LAYERS", (24, 24, 24, 24)])
    return cfg


def test_box_predictor_matches_reference(z):
    from tests.oracle_backend import oracle_ops

    pred = RH.FastRCNNPredictor(small_cfg(), 96)
    pred.load_state_dict({k[5:]: T(z[k]) for k in z.files if k.startswith("pred_") and k[5:] in pred.state_dict()})
    x = T(z["pred_x"])
    with oracle_ops():  # host logic (pooling, weight concat, slicing) on CPU; the HIP GEMM itself: test_heads_gpu.py
        for c in (1, 49, 1203):
            pred.set_class_embeddings(T(z[f"pred_cls{c}"]))
            logits, box = pred(x)
            assert logits.shape == (24, c)
            assert torch.allclose(logits, T(z[f"pred_logits{c}"]), rtol=1e-4, atol=1e-5)
    assert torch.allclose(box, T(z["pred_box"]), rtol=1e-4, atol=1e-6)


def test_box_loss_matches_reference(z):
    ev = RH.FastRCNNLossComputation(small_cfg())
    P = z["boxloss_labels"].shape[0]
    prop = BoxList(torch.zeros(P, 4), (100, 100))
    prop.add_field("labels", T(z["boxloss_labels"]))
    prop.add_field("regression_targets", T(z["boxloss_targets"]))
    ev._proposals = [prop]
    from tests.oracle_backend import oracle_ops

    with oracle_ops():
        lc, lb = ev(T(z["boxloss_logits"]), T(z["boxloss_reg"]))
    assert torch.allclose(lc, T(z["boxloss_cls"]), rtol=1e-5)
    assert torch.allclose(lb, T(z["boxloss_box"]), rtol=1e-5)


def test_mask_predictor_and_loss_match_reference(z):
    mp = RH.MaskRCNNC4Predictor(small_cfg(), 64)
    mp.load_state_dict({k[9:]: T(z[k]) for k in z.files if k.startswith("maskpred_")})
    x = T(z["mask_x"])
    mp.train()
    logits5, scale = mp(x, True, eps=T(z["mask_eps"]))
    assert logits5.shape == (1, 6, 2, 14, 14) and scale.shape == (6, 1, 14, 14)
    assert torch.allclose(scale, T(z["mask_scale"]), rtol=1e-5, atol=1e-6)
    assert torch.allclose(logits5, T(z["mask_logits5"]), rtol=1e-4, atol=1e-5)
    mp.eval()
    assert torch.allclose(mp(x), T(z["mask_logits_eval"]), rtol=1e-4, atol=1e-5)
    flat = torch.flatten(logits5, 0, 1)
    loss = F.binary_cross_entropy_with_logits(flat[torch.arange(6), torch.ones(6, dtype=torch.long)],
                                              T(z["mask_targets"]), reduction="none").mean()
    assert torch.allclose(loss, T(z["mask_loss"]), rtol=1e-5)


def test_numeric_helpers_match_reference(z):
    from cvpr22_cross_modal_pseudo_labeling_amd.layers import FrozenBatchNorm2d, smooth_l1_loss

    coder = BoxCoder(weights=(10.0, 10.0, 5.0, 5.0))
    assert torch.allclose(coder.encode(T(z["coder_ref"]), T(z["coder_prop"])), T(z["coder_enc"]), rtol=1e-5, atol=1e-6)
    assert torch.allclose(coder.decode(T(z["coder_codes"]), T(z["coder_prop"])), T(z["coder_dec"]), rtol=1e-5, atol=1e-3)
    iou = box_iou(T(z["coder_ref"])[:7], T(z["coder_prop"]))
    assert torch.allclose(iou, T(z["iou"]), rtol=1e-6, atol=1e-7)
    assert torch.equal(Matcher(0.5, 0.5, False)(T(z["iou"])), T(z["match_plain"]))
    assert torch.equal(Matcher(0.7, 0.3, True)(T(z["iou"])), T(z["match_rpn"]))
    a, b = T(z["sl1_a"]), T(z["sl1_b"])
    assert torch.allclose(smooth_l1_loss(a, b, beta=1, size_average=False), T(z["sl1_beta1_sum"]))
    assert torch.allclose(smooth_l1_loss(a, b), T(z["sl1_beta9_mean"]))
    bn = FrozenBatchNorm2d(5)
    bn.load_state_dict({k[3:]: T(z[k]) for k in z.files if k.startswith("bn_") and k not in ("bn_x", "bn_y")})
    assert torch.allclose(bn(T(z["bn_x"])), T(z["bn_y"]), rtol=1e-6, atol=1e-6)


def test_frozen_bn_fold_into_conv_is_equivalent():
    from cvpr22_cross_modal_pseudo_labeling_amd.layers import Conv2d, FrozenBatchNorm2d
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.backbone import ConvBN

    g = torch.Generator().manual_seed(0)
    conv, bn = Conv2d(6, 9, 3, stride=2, padding=1, bias=False), FrozenBatchNorm2d(9)
    bn.weight.copy_(torch.randn(9, generator=g)); bn.bias.copy_(torch.randn(9, generator=g))
    bn.running_mean.copy_(torch.randn(9, generator=g)); bn.running_var.copy_(torch.rand(9, generator=g) + 0.5)
    x = torch.randn(2, 6, 11, 13, generator=g)
    fused = ConvBN(conv, bn)
    assert torch.allclose(fused(x), bn(conv(x)), rtol=1e-5, atol=1e-5)
    fused(x).sum().backward()  # gradient reaches the (trainable) conv weight through the fold
    gf = conv.weight.grad.clone()
    conv.weight.grad = None
    bn(conv(x)).sum().backward()
    assert torch.allclose(gf, conv.weight.grad, rtol=1e-4, atol=1e-4)


def test_anchors_and_rpn_proposals_match_reference(z):
    from tests.oracle_backend import oracle_ops
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling import rpn as R

    ag = R.AnchorGenerator((32, 64, 128, 256, 512), (0.5, 1.0, 2.0), 16, 0)
    assert torch.equal(ag.cell_anchors, T(z["cell_anchors"]))
    H, W = 9, 12
    sizes = [(H * 16, W * 16), (H * 16 - 10, W * 16 - 7)]
    anchors = ag(sizes, torch.zeros(2, 1, H, W))
    assert torch.equal(anchors[1].bbox, T(z["anchors_img1"]))
    assert torch.equal(anchors[1].get_field("visibility"), T(z["anchors_vis1"]))
    pp = R.RPNPostProcessor(600, 50, 0.7, 0, BoxCoder(weights=(1.0, 1.0, 1.0, 1.0)))
    with oracle_ops():
        res = pp(anchors, T(z["rpn_obj"]), T(z["rpn_reg"]))
    for i, r in enumerate(res):
        assert torch.allclose(r.bbox, T(z[f"rpn_boxes{i}"]), rtol=1e-5, atol=1e-4)
        assert torch.allclose(r.get_field("objectness"), T(z[f"rpn_scores{i}"]))


def _rpn_loss_case(z, device="cpu"):
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling import rpn as R
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.matcher import BalancedPositiveNegativeSampler, Matcher
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList

    ag = R.AnchorGenerator((32, 64, 128, 256, 512), (0.5, 1.0, 2.0), 16, 0).to(device)
    H, W = 9, 12
    sizes = [(H * 16, W * 16), (H * 16 - 10, W * 16 - 7)]
    anchors = ag(sizes, torch.zeros(2, 1, H, W, device=device))
    targets = [BoxList(T(z[f"rpnloss_gt{i}"]), (sizes[i][1], sizes[i][0])).to(device) for i in range(2)]
    loss = R.RPNLossComputation(Matcher(0.7, 0.3, allow_low_quality_matches=True), BalancedPositiveNegativeSampler(10 ** 6, 0.5),
                                BoxCoder(weights=(1.0, 1.0, 1.0, 1.0)))
    return loss, anchors, T(z["rpn_obj"]).to(device), T(z["rpn_reg"]).to(device), targets


def test_rpn_loss_matches_reference_fixture(z):
    """RPNLossComputation (rpn/loss.py:21-131), tensor-op form: the reference's two losses on the reference's anchors with
    quotas that cover every candidate (no dependence on the random stream)."""
    loss, anchors, obj, reg, targets = _rpn_loss_case(z)
    lo, lb = loss(anchors, obj, reg, targets)
    assert abs(float(lo) - float(z["rpnloss_objectness"])) <= 1e-6 * float(z["rpnloss_objectness"])
    assert abs(float(lb) - float(z["rpnloss_box"])) <= 1e-5 * float(z["rpnloss_box"])


def test_sampler_matches_reference_fixture(z):
    """BalancedPositiveNegativeSampler (tensor-op form): the reference's masks when every candidate is taken, its counts
    otherwise (balanced_positive_negative_sampler.py:39-47)."""
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.matcher import BalancedPositiveNegativeSampler
    lab = T(z["sampler_labels"])
    pos, neg = BalancedPositiveNegativeSampler(4096, 0.25)([lab])
    assert torch.equal(pos[0], T(z["sampler_pos_all"])) and torch.equal(neg[0], T(z["sampler_neg_all"]))
    for batch, frac, key in ((512, 0.25, "sampler_counts_512_025"), (256, 1.0, "sampler_counts_256_100")):
        pos, neg = BalancedPositiveNegativeSampler(batch, frac)([lab])
        assert [int(pos[0].sum()), int(neg[0].sum())] == z[key].tolist()
        assert not bool((pos[0] & neg[0]).any()) and bool((lab[pos[0]] >= 1).all()) and bool((lab[neg[0]] == 0).all())


def test_paste_mask_matches_reference(z):
    m = T(z["paste_mask"])
    for i in range(3):
        got = RH.paste_mask_in_image(m, T(z[f"paste_box{i}"]), 120, 160)
        assert torch.equal(got, T(z[f"paste_out{i}"]))


def test_project_masks_on_boxes_semantics():
    # rectangles: an analytic case -- crop inside a filled rectangle gives all ones, outside all zeros
    masks = torch.zeros(2, 60, 80, dtype=torch.bool)
    masks[0, 10:40, 20:60] = True
    boxes = torch.tensor([[25.0, 15.0, 50.0, 35.0], [0.0, 45.0, 15.0, 58.0], [10.0, 5.0, 30.0, 20.0]])
    out = RH.project_masks_on_boxes(masks, torch.tensor([0, 0, 0]), boxes, 14)
    assert out.shape == (3, 14, 14) and out.dtype == torch.float32
    assert bool((out[0] == 1).all()) and bool((out[1] == 0).all())
    # straddling box: against the straightforward crop + F.interpolate restatement of the reference steps
    xmin, ymin, xmax, ymax = 10, 5, 30, 20
    ref = F.interpolate(masks[0:1, ymin:ymax, xmin:xmax][None].float(), size=(14, 14), mode="bilinear",
                        align_corners=False)[0, 0]
    assert torch.equal(out[2], (ref != 0).float())
    # uint8 masks truncate after interpolation (type_as); a cell whose true value is 1 can land on either
    # side of 1.0 by one ulp depending on the interpolation kernel, so compare away from that edge
    u8 = RH.project_masks_on_boxes(masks.to(torch.uint8), torch.tensor([0]), boxes[2:], 14)
    safe = (ref < 0.999) | (ref == 1.0)
    assert torch.equal(u8[0][safe], ref.to(torch.uint8).float()[safe])
    assert bool(((u8 == 0) | (u8 == 1)).all())


def test_config_surface():
    cfg = get_defaults()
    cfg.merge_from_file(os.path.join(ROOT, "configs/coco_cap_det/student_teacher_mask_rcnn_uncertainty.yaml"))
    cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", "16", "MODEL.RPN.NMS_THRESH", 0.6])
    assert cfg.MODEL.META_ARCHITECTURE == "STGeneralizedRCNN" and cfg.SOLVER.IMS_PER_BATCH == 16
    assert cfg.SOLVER.STEPS == (20000, 50000) and cfg.MODEL.RPN.NMS_THRESH == 0.6
    with pytest.raises(KeyError):
        cfg.merge_from_list(["MODEL.NOT_A_KEY", 1])
    with pytest.raises(ValueError):
        cfg.merge_from_list(["SOLVER.IMS_PER_BATCH", "many"])
    cfg.freeze()
    with pytest.raises(AttributeError):
        cfg.SOLVER.BASE_LR = 1.0
    assert cfg.clone().SOLVER.BASE_LR == cfg.SOLVER.BASE_LR


@pytest.mark.parametrize("name", ["student_teacher_mask_rcnn_uncertainty", "zeroshot_mask"])
def test_tiny_train_step_on_cpu_with_oracle_ops(name):
    """BASELINE.json configs[0] (CPU plumbing): both meta-architectures step on CPU tensors when -- and
    only when -- the test harness routes the native ops to the oracle."""
    from tests.oracle_backend import oracle_ops
    from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import calibrate_stem_bn, make_batch, make_embeddings
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import comm, solver, trainer
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.detector import build_detection_model

    torch.manual_seed(0)
    cfg = get_defaults()
    cfg.merge_from_file(os.path.join(ROOT, f"configs/coco_cap_det/{name}.yaml"))
    cfg.merge_from_list(["MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 300, "MODEL.RPN.PRE_NMS_TOP_N_TEST", 200,
                         "MODEL.RPN.POST_NMS_TOP_N_TRAIN", 60, "MODEL.RPN.POST_NMS_TOP_N_TEST", 40,
                         "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 16, "SOLVER.BASE_LR", 1e-5])
    cfg.freeze()
    model = build_detection_model(cfg)
    e_vocab, e_seen = make_embeddings(n_vocab=50)
    model.set_class_embeddings(e_seen)
    if hasattr(model, "set_caption_vocab"):
        model.set_caption_vocab(e_vocab)
    images, targets = make_batch(2, height=128, width=160, num_gt=3, num_nouns=2, n_vocab=50)
    calibrate_stem_bn(model, images)
    model.train()
    opt = solver.make_optimizer(cfg, model)
    red = comm.BucketedGradReducer(model)
    with oracle_ops():
        before = {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
        losses = trainer.train_step(model, opt, red, images, targets)
    want = {"loss_classifier", "loss_box_reg", "loss_mask"}
    if name.startswith("student"):
        want |= {k + "_pseudo" for k in want}
        frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
        assert any(n.startswith("backbone.") for n in frozen) and any(n.startswith("roi_heads.") for n in frozen)
        assert all(n.startswith("roi_heads_student.") or n == "lambda_exemplar" for n in before)
    else:
        want |= {"loss_objectness", "loss_rpn_box_reg"}
    assert set(losses) == want
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    moved = [n for n, p in model.named_parameters() if p.requires_grad and not torch.equal(p.detach(), before[n])]
    assert len(moved) > 10


def test_group_fused_sgd_matches_torch_sgd():
    """One-group-per-parameter SGD (solver/build.py:8-37) as six multi-tensor ops: same trajectory, same state_dict."""
    from cvpr22_cross_modal_pseudo_labeling_amd.engine.solver import GroupFusedSGD
    g = torch.Generator().manual_seed(0)
    ps = [torch.randn(5, 3, generator=g, requires_grad=True), torch.randn(7, generator=g, requires_grad=True),
          torch.randn(2, 2, generator=g, requires_grad=True)]
    qs = [p.detach().clone().requires_grad_(True) for p in ps]

    def groups(l):
        return [{"params": [l[0]], "lr": 0.1, "weight_decay": 1e-2}, {"params": [l[1]], "lr": 0.2, "weight_decay": 0.0},
                {"params": [l[2]], "lr": 0.05, "weight_decay": 1e-3}]

    a, b = GroupFusedSGD(groups(ps), 0.1, momentum=0.9), torch.optim.SGD(groups(qs), 0.1, momentum=0.9)
    for it in range(5):
        for p, q in zip(ps, qs):
            gr = torch.randn(p.shape, generator=g)
            p.grad, q.grad = gr.clone(), gr.clone()
        if it == 3:
            ps[1].grad = None  # a parameter without a gradient is skipped, as in torch
            qs[1].grad = None
        a.step()
        b.step()
        for p, q in zip(ps, qs):
            assert (p - q).abs().max().item() <= 1e-6
    b.load_state_dict(a.state_dict())
    assert len(a.state_dict()["param_groups"]) == 3


def test_checkpoint_suffix_alignment_and_roundtrip(tmp_path):
    """Reference wire format (utils/model_serialization.py:10-89, utils/checkpoint.py:14-154): DDP ``module.`` prefix,
    longest-suffix key alignment, substring rewrites, strict load, model_<iter>.pth + last_checkpoint tag file."""
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.engine import solver
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.detector import build_detection_model
    from cvpr22_cross_modal_pseudo_labeling_amd.utils.checkpoint import (DetectronCheckpointer, align_and_update_state_dicts,
                                                                           load_state_dict, strip_prefix_if_present)
    cfg = get_defaults()
    cfg.merge_from_file(os.path.join(ROOT, "configs/coco_cap_det/zeroshot_mask.yaml"))
    cfg.freeze()
    torch.manual_seed(0)
    src = build_detection_model(cfg)
    torch.manual_seed(1)
    dst = build_detection_model(cfg)
    sd = src.state_dict()
    assert any(k.startswith("backbone.body.layer1.0.conv1") for k in sd) and "rpn.head.conv.weight" in sd
    # (a) a DDP checkpoint: every key prefixed with "module."
    ddp = {"module." + k: v for k, v in sd.items()}
    assert set(strip_prefix_if_present(dict(ddp), "module.")) == set(sd)
    matched = load_state_dict(dst, ddp)
    assert len(matched) == len(sd)
    for k, v in dst.state_dict().items():
        assert torch.equal(v, sd[k]), k
    # (b) backbone-only weights saved WITHOUT the "backbone.body." nesting (an ImageNet-style trunk file), plus a decoy
    # shorter suffix that must lose against the longer match
    torch.manual_seed(2)
    dst2 = build_detection_model(cfg)
    before = {k: v.clone() for k, v in dst2.state_dict().items()}
    trunk = {k[len("backbone.body."):]: v for k, v in sd.items() if k.startswith("backbone.body.")}
    assert sum(k.endswith("stem.conv1.weight") for k in sd) == 1
    trunk["conv1.weight"] = torch.zeros_like(sd["backbone.body.stem.conv1.weight"])  # a shorter suffix of the same key
    model_sd = {"backbone.body.stem.conv1.weight": before["backbone.body.stem.conv1.weight"].clone()}
    align_and_update_state_dicts(model_sd, trunk)
    assert torch.equal(model_sd["backbone.body.stem.conv1.weight"], sd["backbone.body.stem.conv1.weight"])  # longest won
    del trunk["conv1.weight"]
    matched = load_state_dict(dst2, trunk)
    after = dst2.state_dict()
    assert matched and all(k.startswith("backbone.body.") for k in matched)
    assert torch.equal(after["backbone.body.layer3.5.conv3.weight"], sd["backbone.body.layer3.5.conv3.weight"])
    assert torch.equal(after["rpn.head.conv.weight"], before["rpn.head.conv.weight"])  # unmatched keys untouched
    # (c) rewrite rule: an MMSS projection head becomes emb_pred; cls_score kept out
    model_sd = {"roi_heads.box.predictor.emb_pred.weight": torch.zeros(2, 2)}
    loaded = {"mmss_heads.GroundingHead.v2l_projection.weight": torch.ones(2, 2)}
    align_and_update_state_dicts(model_sd, loaded, {"mmss_heads.GroundingHead.v2l_projection": "roi_heads.box.predictor.emb_pred"})
    assert bool((model_sd["roi_heads.box.predictor.emb_pred.weight"] == 1).all())
    # (d) save / resume round trip in the reference's directory layout
    opt = solver.make_optimizer(cfg, src)
    sched = solver.make_lr_scheduler(cfg, opt)
    ck = DetectronCheckpointer(cfg, src, opt, sched, save_dir=str(tmp_path))
    path = ck.save("model_0000007", iteration=7)
    assert os.path.basename(path) == "model_0000007.pth" and open(tmp_path / "last_checkpoint").read() == path
    torch.manual_seed(3)
    fresh = build_detection_model(cfg)
    opt2 = solver.make_optimizer(cfg, fresh)
    extra = DetectronCheckpointer(cfg, fresh, opt2, solver.make_lr_scheduler(cfg, opt2), save_dir=str(tmp_path)).load()
    assert extra == {"iteration": 7}
    for k, v in fresh.state_dict().items():
        assert torch.equal(v, sd[k]), k
    with pytest.raises(RuntimeError, match="not present in the catalog"):  # other sources: utils/weight_sources.py
        ck._load_file("catalog://ImageNetPretrained/MSRA/R-18")


def test_masker_batched_host_read_equals_per_mask_paste():
    """Masker (one host read of all expanded boxes, one padded / canvas fill) == the reference's per-mask
    paste_mask_in_image loop (mask_head/inference.py:124-205), incl. degenerate and out-of-image boxes."""
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.roi_heads import Masker, paste_mask_in_image
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList

    g = torch.Generator().manual_seed(0)
    P = 12
    masks = torch.rand(P, 1, 14, 14, generator=g)
    xy = torch.rand(P, 2, generator=g) * torch.tensor([300.0, 200.0]) - 20
    boxes = torch.cat([xy, xy + torch.rand(P, 2, generator=g) * 150 + 1], 1)
    boxes[3] = torch.tensor([50.0, 60.0, 50.0, 60.0])
    boxes[4] = torch.tensor([-100.0, -100.0, -50.0, -60.0])
    got = Masker(0.5, 1)(masks, BoxList(boxes, (320, 240)))
    want = torch.stack([paste_mask_in_image(m[0], b, 240, 320, 0.5, 1) for m, b in zip(masks, boxes)])[:, None]
    assert got.dtype == torch.bool and torch.equal(got, want) and int(got[4].sum()) == 0
    assert Masker()(masks[:0], BoxList(boxes[:0], (320, 240))).shape == (0, 1, 240, 320)


def test_device_prefetcher_order_structure_and_errors():
    """data.prefetch.DevicePrefetcher: batches come out in source order with the same nested structure (tensors, BoxLists
    with tensor and non-tensor fields), the source ends cleanly, and a source exception surfaces in the consumer."""
    from cvpr22_cross_modal_pseudo_labeling_amd.data.prefetch import DevicePrefetcher
    from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import make_batch

    def source(n, fail_at=None):
        for i in range(n):
            if i == fail_at:
                raise RuntimeError("broken sample")
            yield make_batch(1, seed=i, height=32, width=48, num_gt=2, num_nouns=2)

    got = list(DevicePrefetcher(source(5), "cpu", depth=2))
    assert len(got) == 5
    for i, (images, targets) in enumerate(got):
        want_images, want_targets = make_batch(1, seed=i, height=32, width=48, num_gt=2, num_nouns=2)
        assert torch.equal(images, want_images) and len(targets) == 1
        t, w = targets[0], want_targets[0]
        assert torch.equal(t.bbox, w.bbox) and t.size == w.size and t.get_field("is_det") == "Yes"
        assert torch.equal(t.get_field("masks"), w.get_field("masks")) and torch.equal(t.get_field("ids_cap"), w.get_field("ids_cap"))
    it = DevicePrefetcher(source(4, fail_at=2), "cpu", depth=1)
    assert next(it) is not None and next(it) is not None
    with pytest.raises(RuntimeError, match="broken sample"):
        next(it)


def test_synthetic_batches_through_worker_processes_keep_their_order():
    """SyntheticBatches behind a 2-worker DataLoader + DevicePrefetcher: batch it == make_batch(seed0 + 1000 * it + rank)."""
    from cvpr22_cross_modal_pseudo_labeling_amd.data.prefetch import DevicePrefetcher
    from cvpr22_cross_modal_pseudo_labeling_amd.data.synthetic import SyntheticBatches, make_batch

    kw = dict(height=32, width=48, num_gt=2, num_nouns=2)
    loader = torch.utils.data.DataLoader(SyntheticBatches(2, seed0=77, rank=3, **kw), batch_size=None, num_workers=2,
                                         prefetch_factor=2)
    pre = DevicePrefetcher(loader, "cpu", depth=2)
    for it in range(5):
        images, targets = next(pre)
        want_images, want_targets = make_batch(2, seed=77 + 1000 * it + 3, **kw)
        assert torch.equal(images, want_images)
        assert all(torch.equal(a.bbox, b.bbox) for a, b in zip(targets, want_targets))
    pre.close()


# ---- the structures that hold tensors: one declaration, three derived protocols (modeling/structures.py::TensorHolder) ----
def _gt_list(seed=0):
    """A BoxList with every kind of field: a label tensor, a string, polygon masks and (resized, flipped) RLE masks."""
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import PolygonMasks, RleMasks

    b = BoxList(torch.tensor([[2.0, 3.0, 20.0, 18.0], [10.0, 5.0, 30.0, 25.0]]) + seed, (50, 37))
    b.add_field("labels", torch.tensor([3, 1]) + seed)
    b.add_field("is_det", "Yes")
    b.add_field("polygons", PolygonMasks([[[2.0, 3.0, 20.0, 3.0, 20.0, 18.0]], [[10.0, 5.0, 30.0, 5.0, 30.0, 25.0, 10.0, 25.0]]], (50, 37)))
    rle = RleMasks([[100, 50, 37 * 50 - 150], "0000"], (37, 50), image_id=9, ann_ids=[41, 42])
    b.add_field("rle", rle.resize((100, 74)).transpose(0))
    return b


def _sampled_list(seed=0):
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import SampledBoxList

    return SampledBoxList(_gt_list(seed), torch.tensor([1]), all_positive=True)


def _image_list(n=2):
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import ImageList

    return ImageList(torch.arange(n * 3 * 4 * 6, dtype=torch.float32).view(n, 3, 4, 6), [(4, 5), (3, 6)][:n])


def _holder(name):
    """-> (holder, the non-tensor attributes a copy must keep)."""
    from cvpr22_cross_modal_pseudo_labeling_amd.data.transforms import ViewBatch
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import PastedMasks

    if name == "BoxList":
        return _gt_list(), ("size", "mode")
    if name == "SampledBoxList":
        return _sampled_list(), ("size", "mode", "all_positive")
    if name == "PastedMasks":
        return PastedMasks(torch.rand(2, 14, 14), torch.tensor([[1.0, 2.0, 9.0, 8.0], [0.0, 0.0, 5.0, 5.0]]), (37, 50), 0.4, 1), \
            ("image_size", "threshold", "padding")
    if name == "PolygonMasks":
        return _gt_list().get_field("polygons"), ("size",)
    if name == "RleMasks":
        return _gt_list().get_field("rle"), ("size", "flip_h", "flip_v", "source_hw", "image_id", "ann_ids", "num_items")
    if name == "ImageList":
        return _image_list(), ("image_sizes",)
    assert name == "ViewBatch"
    return ViewBatch([_image_list(), _image_list()], [False, True]), ("flips",)


HOLDERS = ["BoxList", "SampledBoxList", "PastedMasks", "PolygonMasks", "RleMasks", "ImageList", "ViewBatch"]


def _reached(obj, out):
    """The tensors a recursive walk of ``device_tensors()`` reaches -- engine/trainer.py::_record_stream's walk."""
    if torch.is_tensor(obj):
        out.append(obj)
    elif isinstance(obj, dict):
        for v in obj.values():
            _reached(v, out)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _reached(v, out)
    elif hasattr(obj, "device_tensors"):
        _reached(obj.device_tensors(), out)
    return out


def _same_state(a, b, names):
    assert type(a) is type(b)
    for n in names:
        assert getattr(a, n) == getattr(b, n), n


@pytest.mark.parametrize("name", HOLDERS)
def test_map_tensors_keeps_type_tensors_and_state(name):
    holder, state = _holder(name)
    copy = holder.map_tensors(lambda t: t.clone())
    _same_state(holder, copy, state)
    mine, theirs = _reached(holder, []), _reached(copy, [])
    assert len(mine) == len(theirs) > 0
    for a, b in zip(mine, theirs):
        assert a is not b and a.dtype == b.dtype and torch.equal(a, b)
    if name in ("BoxList", "SampledBoxList"):
        assert copy.fields() == holder.fields() and copy.get_field("is_det") == "Yes"
        _same_state(holder.get_field("polygons"), copy.get_field("polygons"), ("size",))
        _same_state(holder.get_field("rle"), copy.get_field("rle"), ("size", "flip_h", "source_hw", "image_id", "ann_ids"))
        assert copy.get_field("rle").size == (100, 74) and copy.get_field("rle").flip_h is True
    if name == "SampledBoxList":
        assert copy.all_positive is True and torch.equal(copy.pos_index, holder.pos_index)
        moved = holder.to("cpu")
        assert type(moved) is type(holder) and moved.all_positive is True and torch.equal(moved.pos_index, holder.pos_index)
    if name == "RleMasks":
        assert copy.words is None and copy.word_offsets is None   # None entries stay None
    if name == "ImageList":
        assert holder.to(torch.float64).tensors.dtype == torch.float64   # ``to`` keeps accepting a dtype
    if name == "ViewBatch":
        assert [v.image_sizes for v in copy.views] == [v.image_sizes for v in holder.views]


@pytest.mark.parametrize("name", HOLDERS)
def test_map_tensors_visits_what_device_tensors_reaches(name):
    """One declaration feeds both protocols: the tensors ``map_tensors`` visits, by identity, are those a recursive walk of
    ``device_tensors()`` reaches, each once."""
    holder, _ = _holder(name)
    visited = []
    holder.map_tensors(lambda t: (visited.append(t), t)[1])
    reached = _reached(holder, [])
    assert len(visited) == len(set(map(id, visited))) and len(reached) == len(set(map(id, reached)))
    assert set(map(id, visited)) == set(map(id, reached)) and len(visited) > 0


def test_map_over_a_nested_batch_visits_every_tensor_once():
    """data.prefetch._map over (ImageList, [BoxList, SampledBoxList], {"k": tensor}): the same nesting and types, every
    tensor visited exactly once."""
    from cvpr22_cross_modal_pseudo_labeling_amd.data.prefetch import _map
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import ImageList, SampledBoxList

    batch = (_image_list(), [_gt_list(0), _sampled_list(1)], {"k": torch.tensor([1.0, 2.0])})
    visited = []
    out = _map(batch, lambda t: (visited.append(t), t.clone())[1])
    reached = _reached(batch, [])
    assert sorted(map(id, visited)) == sorted(map(id, reached)) and len(set(map(id, visited))) == len(visited) == 1 + 11 + 12 + 1
    assert type(out) is tuple and type(out[0]) is ImageList and type(out[1]) is list and type(out[2]) is dict
    assert type(out[1][0]) is BoxList and type(out[1][1]) is SampledBoxList and out[1][1].all_positive is True
    assert list(out[2]) == ["k"] and torch.equal(out[2]["k"], batch[2]["k"]) and out[2]["k"] is not batch[2]["k"]
    for a, b in zip(reached, _reached(out, [])):
        assert a is not b and torch.equal(a, b)
    assert out[0].image_sizes == batch[0].image_sizes and out[1][0].get_field("is_det") == "Yes"


def test_mask_targets_of_host_pasted_masks_equal_those_of_the_pasted_canvases():
    """Pseudo-label masks moved to the host (a device step replayed on the CPU) give the targets their dense form gives."""
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import PastedMasks

    gt = torch.tensor([[4.0, 5.0, 20.0, 30.0], [25.0, 3.0, 40.0, 20.0]])
    pasted = PastedMasks(torch.rand(2, 14, 14, generator=torch.Generator().manual_seed(1)), gt, (40, 60))
    prop = BoxList(torch.cat([gt + 1.0, gt - 0.5, torch.tensor([[45.0, 25.0, 55.0, 35.0]])]), (60, 40))
    got = []
    for masks in (pasted, pasted.materialize()):
        target = BoxList(gt, (60, 40))
        target.add_field("labels", torch.tensor([2, 1]))
        target.add_field("masks", masks)
        got.append(RH.MaskRCNNLossComputation(get_defaults()).prepare_targets([prop], [target]))
    (labels_a,), (targets_a,) = got[0]
    (labels_b,), (targets_b,) = got[1]
    assert labels_a.tolist() == labels_b.tolist() == [2, 1, 2, 1, 0]
    assert targets_a.shape == (4, 14, 14) and torch.equal(targets_a, targets_b) and 0.05 < float(targets_a.mean()) < 0.95


def test_box_decode_with_image_clip_equals_decode_then_clip_to_image(z):
    """``BoxCoder.decode(..., rows_per_image, image_sizes)`` (the form the box post-processor calls; on the device one
    kernel) on CPU tensors: the reference's decode (fixture) followed by ``BoxList.clip_to_image`` per image."""
    coder = BoxCoder(weights=(10.0, 10.0, 5.0, 5.0))
    codes, boxes = T(z["coder_codes"]).clone(), T(z["coder_prop"]).clone()
    codes[::3] *= 40.0  # push some boxes outside the images
    n = codes.shape[0]
    per_img, sizes = [n // 3, 0, n - n // 3], [(60, 40), (10, 10), (35, 55)]
    want = coder.decode(codes, boxes)
    at = 0
    for cnt, size in zip(per_img, sizes):
        for j in range(want.shape[1] // 4):  # clip_to_image clamps in place through the column-slice views
            BoxList(want[at:at + cnt, 4 * j:4 * j + 4], size).clip_to_image(remove_empty=False)
        at += cnt
    got = coder.decode(codes, boxes, per_img, sizes)
    assert torch.equal(got, want)
    assert float(got[:, 0::2].max()) <= 59.0 and float(got.min()) >= 0.0


def test_total_loss_is_the_sum_of_the_terms():
    from cvpr22_cross_modal_pseudo_labeling_amd.engine.trainer import total_loss

    terms = {"a": torch.tensor(1.5, requires_grad=True), "b": torch.tensor(2.25, requires_grad=True),
             "c": torch.tensor(-0.5, requires_grad=True), "d": 0.0}
    t = total_loss(terms)
    assert float(t) == 3.25
    t.backward()
    assert all(float(v.grad) == 1.0 for v in terms.values() if torch.is_tensor(v))


def test_c2_names_catalog_and_cache_paths_match_reference(golden_dir, tmp_path, monkeypatch):
    """utils/weight_sources.py against name pairs / URLs produced by the reference's own functions
    (tests/golden/c2_names.json, written by make_golden.py::gen_c2_names): every blob of an R-50-C4 Detectron / ImageNet
    checkpoint, the momentum blobs dropped, catalog names, and cache_url's file naming (model_zoo.py:40-48)."""
    import json

    from cvpr22_cross_modal_pseudo_labeling_amd.utils import weight_sources as ws

    with open(os.path.join(golden_dir, "c2_names.json")) as f:
        gold = json.load(f)
    assert len(gold["names"]) >= 170
    for blob, want in gold["names"].items():
        assert ws.c2_name_to_torch(blob) == want, blob
    assert all(ws.c2_name_to_torch(b) is None for b in gold["momentum"])
    with pytest.raises(RuntimeError):
        ws.c2_name_to_torch("fpn_inner_res5_2_sum_lateral_w")
    for name, url in gold["catalog"].items():
        assert ws.catalog_url(name) == url
    with pytest.raises(RuntimeError):
        ws.catalog_url("ImageNetPretrained/MSRA/R-18")
    monkeypatch.setenv("TORCH_MODEL_ZOO", str(tmp_path))
    assert ws.cache_path(gold["catalog"]["ImageNetPretrained/MSRA/R-50"]) == str(tmp_path / "R-50.pkl")
    det = ws.cache_path(gold["catalog"]["Caffe2Detectron/COCO/35858791/e2e_mask_rcnn_R-50-C4_1x"])
    assert os.path.dirname(det) == str(tmp_path) and os.path.basename(det).startswith("_detectron_35858791_12_2017_baselines_")
    assert det.endswith("_generalized_rcnn_model_final.pkl")


def test_detectron_checkpointer_loads_c2_pickle_and_catalog_names(tmp_path, monkeypatch):
    """A Caffe2-format pickle (``blobs`` of numpy arrays under C2 names, incl. momentum blobs) of the ResNet-C4 trunk +
    res5 head round-trips into the model through ``DetectronCheckpointer`` -- by path and by ``catalog://`` name served
    from the model cache (no network) -- and a missing cache file fails with the path it belongs at."""
    import pickle

    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.detector import build_detection_model
    from cvpr22_cross_modal_pseudo_labeling_amd.utils.checkpoint import DetectronCheckpointer

    cfg = get_defaults()
    cfg.merge_from_file(os.path.join(ROOT, "configs/coco_cap_det/zeroshot_mask.yaml"))
    cfg.freeze()
    torch.manual_seed(7)
    model = build_detection_model(cfg)
    inv_branch = {"conv1": "2a", "conv2": "2b", "conv3": "2c", "bn1": "2a_bn", "bn2": "2b_bn", "bn3": "2c_bn"}

    def c2_name(key):  # torch name -> C2 blob name, for the tensors a C2 checkpoint holds
        p = key.split(".")
        kind = {"weight": "w", "bias": "b"}.get(p[-1])
        if kind is None:
            return None
        if p[0] == "conv1":
            return f"conv1_{kind}"
        if p[0] == "bn1":
            return f"res_conv1_bn_{'s' if kind == 'w' else 'b'}"
        if p[0].startswith("layer"):
            stage, block, mod = int(p[0][5:]) + 1, p[1], p[2]
            if mod == "downsample":
                bn = p[3] == "1"
                return f"res{stage}_{block}_branch1{'_bn' if bn else ''}_{('s' if kind == 'w' else 'b') if bn else kind}"
            bn = mod.startswith("bn")
            return f"res{stage}_{block}_branch{inv_branch[mod]}_{('s' if kind == 'w' else 'b') if bn else kind}"
        return None

    blobs, expect = {}, {}
    g = torch.Generator().manual_seed(1)
    for scope, prefix in ((model.backbone.body, "backbone.body."), (model.roi_heads["box"].feature_extractor.head,
                                                                     "roi_heads.box.feature_extractor.head.")):
        for key, t in scope.state_dict().items():
            key = key.replace("stem.", "")
            blob = c2_name(key)
            if blob is None or not torch.is_floating_point(t):
                continue
            v = torch.randn(t.shape, generator=g)
            blobs[blob] = v.numpy()
            expect[prefix + ("stem." if key.split(".")[0] in ("conv1", "bn1") else "") + key] = v
    blobs["conv1_w_momentum"] = np.zeros(3, np.float32)
    assert len(blobs) > 150
    path = tmp_path / "R-50.pkl"
    with open(path, "wb") as f:
        pickle.dump({"blobs": blobs}, f)

    def check(m):
        sd = m.state_dict()
        for k, v in expect.items():
            assert torch.equal(sd[k], v), k

    DetectronCheckpointer(cfg, model).load(str(path))
    check(model)
    monkeypatch.setenv("TORCH_MODEL_ZOO", str(tmp_path))
    model2 = build_detection_model(cfg)
    DetectronCheckpointer(cfg, model2).load("catalog://ImageNetPretrained/MSRA/R-50")
    check(model2)
    with pytest.raises(RuntimeError, match="R-101.pkl"):
        DetectronCheckpointer(cfg, model2).load("catalog://ImageNetPretrained/MSRA/R-101")


def test_project_masks_formula_on_crops_that_are_multiples_of_the_resolution():
    """The host side of tests/test_targets_gpu.py's case (crop sizes 14 k: exact-zero second-tap weights)."""
    from tests.test_targets_gpu import test_project_masks_on_crops_that_are_multiples_of_the_resolution as case
    case(False)


def test_accumulation_windows_follow_iteration_numbers_like_the_reference_loop():
    """engine/trainer.py:96-98,135-141: the optimizer steps at iterations whose NUMBER is a multiple of
    SOLVER.GRADIENT_ACCUMULATION_STEPS -- a run resumed at an odd iteration, or a window that lost a batch to the empty-target
    skip, steps where the reference's does -- against that loop written out on a copy of the model."""
    import copy

    from cvpr22_cross_modal_pseudo_labeling_amd.engine import comm, trainer

    torch.manual_seed(0)
    ref = torch.nn.Linear(4, 3)
    mine = copy.deepcopy(ref)
    xs = [torch.randn(5, 4) for _ in range(7)]
    k = 3
    # the reference loop: iterations 5 .. 11 of a resumed run, iteration 8 skipped (an image without targets)
    opt_r = torch.optim.SGD(ref.parameters(), lr=0.1, momentum=0.9)
    steps_r = []
    for it, x in zip(range(5, 12), xs):
        if it == 8:
            continue
        (ref(x).pow(2).mean() / k).backward()
        if it % k == 0:
            torch.nn.utils.clip_grad_norm_(ref.parameters(), 0.5)
            opt_r.step()
            opt_r.zero_grad()
            steps_r.append(it)

    class Wrap(torch.nn.Module):
        def __init__(self, m):
            super().__init__()
            self.m = m

        def forward(self, x, targets):
            return {"loss": self.m(x).pow(2).mean()}

    model = Wrap(mine)
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9)
    reducer = comm.BucketedGradReducer(model)
    policy = trainer.StepPolicy(k, 0.5)
    steps = []
    for it, x in zip(range(5, 12), xs):
        if it == 8:
            continue
        before = mine.weight.detach().clone()
        trainer.train_step(model, opt, reducer, x, None, None, policy, iteration=it)
        if not torch.equal(before, mine.weight.detach()):
            steps.append(it)
    reducer.remove()
    assert steps == steps_r == [6, 9]
    assert torch.allclose(mine.weight, ref.weight, rtol=1e-6, atol=1e-7) and torch.allclose(mine.bias, ref.bias, rtol=1e-6, atol=1e-7)


def test_branch_run_ahead_joins_precomputed_gradients_to_the_graph():
    """``modeling.rpn._BranchRunAhead`` (the node that joins the teacher step's run-ahead RPN branch to the graph), on host
    tensors and without streams: identity on the feature and the loss values; the backward hands on the incoming feature
    gradient plus the branch's pre-computed one and the parameters' pre-computed gradients, each times the gradient the loss
    values receive (1 for a plain sum, 1 / k inside an accumulation window); two loss terms weighted differently give NaN
    instead of silently wrong gradients; a branch that reaches no parameter at all passes the feature gradient through."""
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.rpn import _BranchRunAhead

    g = torch.Generator().manual_seed(3)
    feature = torch.randn(2, 3, 4, 5, generator=g, requires_grad=True)
    params = [torch.randn(4, 3, generator=g, requires_grad=True), torch.randn(4, generator=g, requires_grad=True),
              torch.randn(2, generator=g, requires_grad=True)]
    pre = [torch.randn(2, 3, 4, 5, generator=g), torch.randn(4, 3, generator=g), None, torch.randn(2, generator=g)]
    lo, lb = torch.tensor(0.7), torch.tensor(1.9)

    def run(scale_lo, scale_lb, pre_=pre):
        for t in [feature] + params:
            t.grad = None
        joined, lo2, lb2 = _BranchRunAhead.apply((None, None), pre_, feature, lo, lb, *params)
        assert torch.equal(joined, feature) and float(lo2.detach()) == float(lo) and float(lb2.detach()) == float(lb)
        assert lo2.requires_grad and lb2.requires_grad
        ((joined * 2.0).sum() + scale_lo * lo2 + scale_lb * lb2).backward()
        return feature.grad, [p.grad for p in params]

    for s in (1.0, 0.5):
        gf, gp = run(s, s)
        assert torch.equal(gf, 2.0 + s * pre[0])
        assert torch.equal(gp[0], s * pre[1]) and gp[1] is None and torch.equal(gp[2], s * pre[3])
    gf, gp = run(1.0, 0.25)
    assert torch.isnan(gf).all() and torch.isnan(gp[0]).all() and torch.isnan(gp[2]).all()
    gf, gp = run(1.0, 1.0, [None, None, None, None])
    assert torch.equal(gf, torch.full_like(feature, 2.0)) and all(x is None for x in gp)
    gf, gp = run(1.0, 1.0, [None] + pre[1:])   # a frozen trunk: only the head trains
    assert torch.equal(gf, torch.full_like(feature, 2.0)) and torch.equal(gp[0], pre[1])



def test_roi_feature_extractor_hands_out_the_head_record_on_host_tensors():
    """``ResNet50Conv5ROIFeatureExtractor`` returns ``HeadFeatures`` on the host route too, with nothing but the maps in it
    (``pooled`` / ``selected`` are outputs of the device route's last autograd node); ``FastRCNNPredictor`` on those maps
    gives the logits of the pass without the record -- pooler bins -> ``ResNetHead`` -> predictor, bit for bit -- which are
    avgpool -> Linear -> product with the class matrix (fp64; bound: the two fp32 dot products of 2048 and 768 terms at
    2^-24 per term, worst case)."""
    from tests.oracle_backend import oracle_ops
    from tests.tiny_model import build_tiny
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.backbone import HeadFeatures

    model, _, e_seen, _, _ = build_tiny("zeroshot_mask")
    box = model.roi_heads["box"].eval()
    box.predictor.set_class_embeddings(e_seen)
    fe, pred = box.feature_extractor, box.predictor
    g = torch.Generator().manual_seed(2)
    feat = torch.randn(2, fe.head.layer4[0].conv1.in_channels, 10, 12, generator=g)
    props = []
    for n in (5, 3):
        xy = torch.rand(n, 2, generator=g) * torch.tensor([120.0, 100.0])
        props.append(BoxList(torch.cat([xy, xy + 16 + torch.rand(n, 2, generator=g) * 50], 1), (192, 160)))
    with oracle_ops(), torch.no_grad():
        feats = fe([feat], props)
        assert isinstance(feats, HeadFeatures) and feats.pooled is None and feats.selected is None
        assert feats.maps.shape == (8, fe.out_channels, 7, 7)
        by_rois = fe.forward_rois([feat], fe.pooler.convert_to_roi_format(props))
        assert isinstance(by_rois, HeadFeatures) and by_rois[1:] == (None, None) and torch.equal(by_rois.maps, feats.maps)
        logits, deltas = pred(feats.maps)
        plain = fe.head(fe.pooler([feat], props))
        assert torch.equal(plain, feats.maps)
        want_logits, want_deltas = pred(plain)
        assert torch.equal(logits, want_logits) and torch.equal(deltas, want_deltas)
        assert torch.equal(pred.pooled(feats.maps), feats.maps.mean(dim=(2, 3))) and pred.pooled(deltas) is deltas
        x_box, _, _ = box([feat], [p.copy_with_fields([]) for p in props])
        assert torch.equal(x_box, feats.maps)  # the box features of a host pass stay the maps
    pooled = feats.maps.double().mean(dim=(2, 3))
    emb = F.linear(pooled, pred.emb_pred.weight.double(), pred.emb_pred.bias.double())
    ref_logits = emb @ pred.cls_score.double().t()
    ref_deltas = F.linear(pooled, pred.bbox_pred.weight.double(), pred.bbox_pred.bias.double())
    tol = (2048 + 768) * 2.0 ** -24
    assert logits.shape == ref_logits.shape and (logits.double() - ref_logits).abs().max().item() <= tol * ref_logits.abs().max().item()
    assert (deltas.double() - ref_deltas).abs().max().item() <= tol * ref_deltas.abs().max().item()
