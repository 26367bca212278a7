"""GPU parity of the cross-modal head kernels (MFMA GEMM, region<->noun alignment, fused losses): against
fixtures produced by the reference's own Python modules (tests/golden/heads.npz) and against plain fp32/fp64
torch formulas (what the reference computes these with) on seeded inputs."""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def z(golden_dir):
    return np.load(os.path.join(golden_dir, "heads.npz"))


def T(a):
    return torch.from_numpy(np.asarray(a))


def test_box_predictor_fixture(z):
    from tests.test_components import small_cfg
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling import roi_heads as RH

    pred = RH.FastRCNNPredictor(small_cfg(), 96).cuda()
    pred.load_state_dict({k[5:]: T(z[k]) for k in z.files if k.startswith("pred_") and k[5:] in pred.state_dict()})
    x = T(z["pred_x"]).cuda()
    for c in (1, 49, 1203):
        pred.set_class_embeddings(T(z[f"pred_cls{c}"]).cuda())
        logits, box = pred(x)
        assert torch.allclose(logits.cpu(), T(z[f"pred_logits{c}"]), rtol=1e-4, atol=1e-5)  # north_star: 1e-3 rel
    assert torch.allclose(box.cpu(), T(z["pred_box"]), rtol=1e-4, atol=1e-6)


def test_box_loss_fixture(z):
    from tests.test_components import small_cfg
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling import roi_heads as RH
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.structures import BoxList

    ev = RH.FastRCNNLossComputation(small_cfg())
    P = z["boxloss_labels"].shape[0]
    prop = BoxList(torch.zeros(P, 4), (100, 100))
    prop.add_field("labels", T(z["boxloss_labels"]).cuda())
    prop.add_field("regression_targets", T(z["boxloss_targets"]).cuda())
    ev._proposals = [prop]
    lc, lb = ev(T(z["boxloss_logits"]).cuda(), T(z["boxloss_reg"]).cuda())
    assert torch.allclose(lc.cpu(), T(z["boxloss_cls"]), rtol=1e-5)
    assert torch.allclose(lb.cpu(), T(z["boxloss_box"]), rtol=1e-5)


def test_mask_predictor_and_fused_loss_fixture(z):
    from tests.test_components import small_cfg
    from cvpr22_cross_modal_pseudo_labeling_amd.layers import stochastic_mask_bce
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling import roi_heads as RH

    mp = RH.MaskRCNNC4Predictor(small_cfg(), 64).cuda()
    mp.load_state_dict({k[9:]: T(z[k]) for k in z.files if k.startswith("maskpred_")})
    x = T(z["mask_x"]).cuda()
    mp.train()
    eps = T(z["mask_eps"]).cuda()
    logits5, scale = mp(x, True, eps=eps)
    assert torch.allclose(logits5.cpu(), T(z["mask_logits5"]), rtol=1e-4, atol=1e-5)
    mu, sigma = mp.forward_parts(x)
    loss = stochastic_mask_bce(mu, sigma, eps[0], torch.arange(6, device="cuda"), T(z["mask_targets"]).cuda().reshape(6, -1), 1)
    assert torch.allclose(loss.cpu(), T(z["mask_loss"]), rtol=1e-5)


@pytest.mark.parametrize("m,n,k", [(512, 776, 2048), (1000, 1203, 768), (1024, 49, 768), (7, 5, 768), (65, 130, 33),
                                   (1, 1, 1)])
def test_gemm_and_linear_autograd_vs_torch(m, n, k):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.layers import cross_modal, linear_mfma

    g = torch.Generator().manual_seed(m * 7 + n)
    a, b, bias = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g), torch.randn(n, generator=g)
    want = (a.double() @ b.double().t() + bias.double())
    got = _C.gemm_nt(a.cuda(), b.cuda(), bias.cuda()).cpu().double()
    tol = 2e-6 * (a.double().abs() @ b.double().abs().t() + bias.double().abs())  # fp32 round-off class bound
    assert bool(((got - want).abs() <= tol + 1e-30).all())
    # strided operands (the backward products) and autograd
    gy = torch.randn(m, n, generator=g)
    ar, br, biasr = a.double().requires_grad_(True), b.double().requires_grad_(True), bias.double().requires_grad_(True)
    (ar @ br.t() + biasr).backward(gy.double())
    mags = (gy.double().abs() @ b.double().abs(), gy.double().abs().t() @ a.double().abs())

    def grads(fn):
        ad, bd, biasd = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
        fn(ad, bd, biasd).backward(gy.cuda())
        return ad.grad, bd.grad, biasd.grad

    def max_norm_check(got_g, want_g):
        scale = want_g.abs().max().item() + 1e-12
        assert (got_g.cpu().double() - want_g).abs().max().item() <= 1e-5 * scale * max(1.0, (m + n + k) ** 0.5 / 8)

    # The fp32 GEMM's two backward layouts (dA = gy B: B read row-contiguous; dB = gy^T A: both operands row-contiguous),
    # element-wise in the forward's round-off class: |dA - ref| <= 2e-6 |gy||B|, |dB - ref| <= 2e-6 |gy|^T|A|.
    # ``linear_mfma`` sends K % 128 == 0, N >= 32 to the three-term bf16 split GEMM instead, whose class is 3e-5 (its own
    # test below); there the fp32 GEMM's autograd node is held to 2e-6 directly and ``linear_mfma`` keeps its earlier bound
    # (its dA at 1024x49x768 measures 3.2 x 2e-6 |gy||B| -- a contraction over 49 terms does not average the split's error --
    # where the fp32 GEMM measures 0.17; the other split-routed gradients measure 0.47 .. 0.86, the fp32 ones at most 0.17).
    pair = cross_modal._pair_ok(a.cuda(), b.cuda())
    routes = [("linear_mfma", linear_mfma)] + ([("fp32 GEMM autograd", cross_modal._LinearMFMA.apply)] if pair else [])
    for route, fn in routes:
        da, db, dbias = grads(fn)
        for name, got_g, want_g, mag in (("dA", da, ar.grad, mags[0]), ("dB", db, br.grad, mags[1])):
            err = (got_g.cpu().double() - want_g).abs()
            print(f"{route} {m}x{n}x{k} {name}: error / (2e-6 magnitude) = {(err / (2e-6 * mag + 1e-30)).max().item():.3f}")
            if fn is linear_mfma and pair:
                max_norm_check(got_g, want_g)
            else:
                assert bool((err <= 2e-6 * mag + 1e-30).all())
        max_norm_check(dbias, biasr.grad)


@pytest.mark.parametrize("m,n,k", [(1024, 776, 2048), (2000, 768, 2048), (1024, 1203, 768), (1024, 49, 768), (3, 776, 2048)])
def test_linear_pair_split_gemm_vs_fp64_and_deterministic(m, n, k):
    """The cross-modal head's products through the pair-layout split GEMM (layers.cross_modal._LinearPair): inside the
    three-term bf16 split's bound 3e-5 * sum|a||b| of the fp64 product (a single product can reach 2^-17 + 2^-17 + 2^-18 =
    1.9e-5 plus the fp32 accumulation; long sums measure ~1e-6), forward and both gradients,
    and bit-identical run to run (K slices are reduced in a fixed order, no atomics)."""
    from cvpr22_cross_modal_pseudo_labeling_amd.layers import cross_modal

    g = torch.Generator().manual_seed(m + n + k)
    a, b, bias = torch.randn(m, k, generator=g) * 0.5, torch.randn(n, k, generator=g) * 0.05, torch.randn(n, generator=g)
    gy = torch.randn(m, n, generator=g)
    assert cross_modal._pair_ok(a.cuda(), b.cuda())

    def run():
        ad, bd, biasd = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True), bias.cuda().requires_grad_(True)
        y = cross_modal.linear_mfma(ad, bd, biasd)
        y.backward(gy.cuda())
        return y.detach(), ad.grad, bd.grad, biasd.grad

    y, da, db, dbias = run()
    a64, b64, g64 = a.double(), b.double(), gy.double()
    for got, want, bound in ((y, a64 @ b64.t() + bias.double(), a64.abs() @ b64.abs().t() + bias.double().abs()),
                             (da, g64 @ b64, g64.abs() @ b64.abs()), (db, g64.t() @ a64, g64.abs().t() @ a64.abs())):
        assert got.shape == want.shape
        assert bool(((got.cpu().double() - want).abs() <= 3e-5 * bound + 1e-30).all())
    assert torch.allclose(dbias.cpu().double(), g64.sum(0), rtol=1e-5, atol=1e-5)
    for t1, t2 in zip(run(), (y, da, db, dbias)):
        assert torch.equal(t1, t2)


def test_region_noun_align_vs_torch():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    g = torch.Generator().manual_seed(3)
    emb = torch.randn(1000, 768, generator=g) * 0.05
    nouns = F.normalize(torch.randn(9, 768, generator=g), dim=-1)
    raw, idx = torch.max(emb.double() @ nouns.double().t(), dim=0)
    r, p, i = _C.region_noun_align(emb.cuda(), nouns.cuda())
    assert torch.equal(i.cpu(), idx)  # indices exact (the fixture has no near-ties)
    assert torch.allclose(r.cpu().double(), raw, rtol=1e-5, atol=1e-6)
    assert torch.allclose(p.cpu().double(), torch.sigmoid(raw), rtol=1e-5)
    # exact ties: lowest region index wins, like torch.max
    emb2 = torch.zeros(10, 8)
    emb2[3, 0] = emb2[7, 0] = 2.0
    _, _, i2 = _C.region_noun_align(emb2.cuda(), torch.eye(8)[:1].cuda())
    assert i2.tolist() == [3]
    r0, p0, i0 = _C.region_noun_align(emb.cuda(), torch.zeros(0, 768).cuda())
    assert r0.numel() == 0 and i0.numel() == 0


@pytest.mark.parametrize("p,c", [(1024, 1203), (512, 49), (3, 2), (1, 1)])
def test_weighted_ce_vs_torch(p, c):
    from cvpr22_cross_modal_pseudo_labeling_amd.layers import weighted_cross_entropy

    g = torch.Generator().manual_seed(p + c)
    x = torch.randn(p, c, generator=g) * 3
    lab = torch.randint(0, c, (p,), generator=g)
    lab[::3] = 0
    w = torch.ones(c, dtype=torch.float64)
    w[0] = 0.2
    xr = x.double().requires_grad_(True)
    want = (F.cross_entropy(xr, lab, weight=w, reduction="none") / p).sum()
    want.backward()
    xd = x.cuda().requires_grad_(True)
    got = weighted_cross_entropy(xd, lab.cuda(), 0.2)
    (got * 1.7).backward()
    assert abs(got.item() - want.item()) <= 1e-5 * max(abs(want.item()), 1e-3)
    assert torch.allclose(xd.grad.cpu().double(), 1.7 * xr.grad, rtol=1e-4, atol=1e-8)


def test_stochastic_mask_bce_vs_torch():
    from cvpr22_cross_modal_pseudo_labeling_amd.layers import stochastic_mask_bce

    g = torch.Generator().manual_seed(11)
    P, M = 37, 14
    mu = torch.randn(P, 2, M, M, generator=g) * 2
    sigma = torch.rand(P, 1, M, M, generator=g) + 0.3
    eps = torch.randn(P, 2, M, M, generator=g)
    pos = torch.tensor([0, 3, 4, 9, 20, 36])
    tgt = (torch.rand(pos.numel(), M * M, generator=g) > 0.5).float()
    mr, sr = mu.double().requires_grad_(True), sigma.double().requires_grad_(True)
    z_ = mr + eps.double() * (mr * 0.0 + sr)
    want = F.binary_cross_entropy_with_logits(z_[pos, 1].reshape(pos.numel(), -1), tgt.double(), reduction="none").mean()
    want.backward()
    md, sd = mu.cuda().requires_grad_(True), sigma.cuda().requires_grad_(True)
    got = stochastic_mask_bce(md, sd, eps.cuda(), pos.cuda(), tgt.cuda(), 1)
    got.backward()
    assert abs(got.item() - want.item()) <= 1e-5 * abs(want.item())
    assert torch.allclose(md.grad.cpu().double(), mr.grad, rtol=1e-4, atol=1e-9)
    assert torch.allclose(sd.grad.cpu().double(), sr.grad, rtol=1e-4, atol=1e-9)
    # deterministic variant (no sigma / eps) and the empty-positives case
    got2 = stochastic_mask_bce(mu.cuda(), None, None, pos.cuda(), tgt.cuda(), 1)
    want2 = F.binary_cross_entropy_with_logits(mu[pos, 1].reshape(pos.numel(), -1), tgt)
    assert abs(got2.item() - want2.item()) <= 1e-5 * abs(want2.item())


# ---------------------------------------------------------------- bf16 hi/lo split GEMM + the NHWC res5 head
def test_split_bf16x3_layout_and_precision():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    g = torch.Generator().manual_seed(4)
    x = (torch.randn(37, 64, generator=g) * torch.logspace(-3, 3, 64)).cuda()
    for mode in (0, 1):
        s = _C.split_bf16x3(x, mode)
        assert s.shape == (37, 192) and s.dtype == torch.bfloat16
        hi = x.to(torch.bfloat16)
        lo = (x - hi.float()).to(torch.bfloat16)
        parts = (hi, hi, lo) if mode == 0 else (hi, lo, hi)
        for i, p in enumerate(parts):
            assert torch.equal(s[:, 64 * i: 64 * (i + 1)], p)  # round-to-nearest-even, exact remainder
        assert ((hi.double() + lo.double() - x.double()).abs() <= 2.0 ** -16 * x.double().abs()).all()
    # a row-strided view is read in place
    v = x[:, :32]
    assert torch.equal(_C.split_bf16x3(v, 0)[:, :32], v.to(torch.bfloat16))


@pytest.mark.parametrize("with_bias,with_residual,relu", list(itertools.product((False, True), repeat=3)))
def test_bias_act_in_place(with_bias, with_residual, relu):
    """_C.bias_act_: y <- act((y + bias[col]) + residual) in place, the kernel's order of operations, bit for bit; the
    rows span more than one pass of its grid-stride loop.  A column count that is not a multiple of 4 is refused."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    g = torch.Generator().manual_seed(5)
    rows, cols = 2600, 1028
    y = torch.randn(rows, cols, generator=g).cuda()
    bias = torch.randn(cols, generator=g).cuda() if with_bias else None
    residual = torch.randn(rows, cols, generator=g).cuda() if with_residual else None
    want = y.clone()
    if bias is not None:
        want = want + bias
    if residual is not None:
        want = want + residual
    if relu:
        want = torch.relu(want)
    assert _C.bias_act_(y, bias, residual, relu=relu) is y
    assert torch.equal(y, want)
    with pytest.raises(RuntimeError):
        _C.bias_act_(torch.zeros(8, 6, device="cuda"), torch.zeros(6, device="cuda") if with_bias else None,
                     torch.zeros(8, 6, device="cuda") if with_residual else None, relu=relu)


def test_im2col_split_layout():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 4, 8, generator=g).cuda()
    for flip in (False, True):
        rows = _C.im2col_split_bf16x3(x, 3, 3, flip=flip)
        assert rows.shape == (24, 3 * 9 * 8)
        hi = x.to(torch.bfloat16)
        pad = F.pad(hi.permute(0, 3, 1, 2), (1, 1, 1, 1)).permute(0, 2, 3, 1)  # [2, 5, 6, 8]
        for t in range(9):
            ts = 8 - t if flip else t
            want = pad[:, ts // 3: ts // 3 + 3, ts % 3: ts % 3 + 4, :].reshape(24, 8)
            assert torch.equal(rows[:, t * 8:(t + 1) * 8], want)
            assert torch.equal(rows[:, 72 + t * 8: 72 + (t + 1) * 8], want)


def test_res5_head_nhwc_paths_match_conv_path():
    """ResNetHead: the NHWC chain (pair-layout split GEMM, one autograd node per bottleneck) against the plain per-layer
    convolution path on the same weights."""
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.backbone import ResNetHead

    cfg = get_defaults()
    cfg.freeze()
    torch.manual_seed(0)
    head = ResNetHead(cfg).cuda()
    for m in head.modules():  # non-trivial FrozenBN affine so the fold matters
        if hasattr(m, "running_var"):
            m.weight.uniform_(0.5, 1.5)
            m.bias.uniform_(-0.2, 0.2)
    x = torch.randn(24, 1024, 14, 14, device="cuda")

    def run(nhwc):
        head.nhwc = nhwc
        xx = x.clone().requires_grad_(True)
        y = head(xx)
        head.zero_grad()
        (y * torch.linspace(-1, 1, y.numel(), device="cuda").view_as(y)).sum().backward()
        return y.detach(), xx.grad, head.layer4[0].conv1.weight.grad.clone(), head.layer4[2].conv3.weight.grad.clone()

    ref = run(False)
    got = run(True)
    assert got[0].shape == ref[0].shape
    assert (got[0] - ref[0]).abs().max().item() <= 2e-4 * ref[0].abs().max().item()
    # gradients: a pre-activation within rounding of zero may flip its ReLU gate, which moves isolated entries
    # by O(1) -- compare in the L2 norm
    for a, b in zip(got[1:], ref[1:]):
        assert (a - b).norm().item() <= 5e-3 * b.norm().item()


def test_res5_head_nhwc_empty_and_single_roi():
    """R = 0 (an image without positives) and R = 1 go through the split-GEMM path without special cases."""
    from cvpr22_cross_modal_pseudo_labeling_amd.config import get_defaults
    from cvpr22_cross_modal_pseudo_labeling_amd.modeling.backbone import ResNetHead

    cfg = get_defaults()
    cfg.freeze()
    torch.manual_seed(0)
    head = ResNetHead(cfg).cuda()
    y0 = head(torch.zeros(0, 1024, 14, 14, device="cuda", requires_grad=True))
    assert y0.shape == (0, 2048, 7, 7)
    y0.sum().backward()
    x1 = torch.randn(1, 1024, 14, 14, device="cuda")
    head.nhwc = False
    ref = head(x1)
    head.nhwc = True
    got = head(x1)
    assert (got - ref).abs().max().item() <= 2e-4 * ref.abs().max().item()
