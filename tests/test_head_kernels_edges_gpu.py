"""GPU: the cross-modal head's kernels -- the strided fp32 GEMM with its split-K route and epilogue and the region<->noun
alignment (csrc/gemm_f32.hip), the weighted cross entropy and the stochastic mask BCE (csrc/losses.hip) -- against the
NumPy float64 restatement of their formulas (tests/head_reference.py, pinned by tests/test_head_reference.py) at the sizes
and values where such kernels go wrong silently: every pairing of the three operand-load modes (the generic one reached
three ways), ragged tiles and k-steps, split-K with accumulate and row bias, a strided output whose neighbours must stay
bit-unchanged; negative and tied alignment scores within and across waves and chunks; logits far from the row maximum,
ignored labels, class counts around the wave stride; saturated mask logits, clamped per-positive channels, a missing
noise factor, and gradients that must be exactly zero outside the selected planes.

Integer outputs and "must not be touched" memory are compared exactly; values are bounded against fp64 with the bounds
the project already uses for these kernels (tests/test_heads_gpu.py).  Every test prints its largest error-to-bound
ratio (run with ``-s``).

Largest measured error-to-bound ratios on an MI355X, against the fp64 reference:
  gemm, workspace route        0.13   of 2e-6 * magnitude            (128x192x40, A and B g_rs2, row bias)
  gemm, one slice              0.13   of the same bound              (70x130x1000, A g_off1, B rc, accumulate)
  region_noun_align raw score  0.10   of 2e-6 * sum|emb||noun|       (P1-D8-mixed)
  region_noun_align sigmoid    0.04   of atol 1e-8 + rtol 1e-5       (P3-D7-negative)
  weighted_ce loss             0.02   of 1e-5 * max(|loss|, 1e-3)    (P1030-C130, every planted row)
  weighted_ce gradient         0.004  of atol 1e-8 + rtol 1e-4       (P1030-C130-base-bg1)
  mask_bce loss                0.02   of 1e-5 * |loss|               (P4-C2-28x28, eps only, extreme)
  mask_bce gradient            0.10   of atol 1e-9 + rtol 1e-4       (P5-C3-63x1, raw entry)
No kernel missed a check.
"""
import numpy as np
import pytest
import torch

from tests import head_reference as R

pytestmark = pytest.mark.gpu

OVIS_OK, OVIS_EINVAL, OVIS_ENOSPC = 0, -1, -2


def C(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32)


# ------------------------------------------------------------------ fp32 GEMM
def _operand(x, layout):
    """-> (device buffer to keep alive, pointer of element [0, 0], row stride, k stride)"""
    buf, off, rs, ks = R.lay_out(x, layout)
    t = C(buf)
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + 4 * off, rs, ks


def _gemm_call(case, a_op, b_op, bias_dev, c0, route, workspace=None, workspace_bytes=None):
    """One product into a fresh copy of c0 (row stride N + C_EXTRA).  route "raw": ``_C._gemm_raw`` (brings the workspace the
    library asks for); "one-slice": ``ovis_gemm_ex_f32`` (no workspace, K is not cut); "ws": ``ovis_gemm_ex_ws_f32`` with the
    given workspace.  -> (return code, the whole output matrix)."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    c = C(c0)
    bias_ptr = 0 if bias_dev is None else bias_dev.data_ptr()
    per_row = int(case.bias == "row")
    ops = (a_op[1], a_op[2], a_op[3], b_op[1], b_op[2], b_op[3])
    c_rs = case.n + R.C_EXTRA
    rc = OVIS_OK
    if route == "raw":
        _C._gemm_raw(*ops, c.data_ptr(), c_rs, case.m, case.n, case.k, bias_ptr=bias_ptr, bias_per_row=per_row,
                     alpha=case.alpha, accumulate=case.accumulate)
    elif route == "one-slice":
        rc = _C._L.ovis_gemm_ex_f32(*ops, bias_ptr, per_row, case.alpha, case.accumulate, c.data_ptr(), c_rs, case.m, case.n,
                                    case.k, _C._stream())
    else:
        rc = _C._L.ovis_gemm_ex_ws_f32(*ops, bias_ptr, per_row, case.alpha, case.accumulate, c.data_ptr(), c_rs, case.m,
                                       case.n, case.k, 0 if workspace is None else workspace.data_ptr(), workspace_bytes,
                                       _C._stream())
    torch.cuda.synchronize()
    return rc, c.cpu().numpy()


@pytest.mark.parametrize("case", R.gemm_cases(), ids=lambda c: c.name)
def test_gemm_f32_edges(case):
    """C = alpha A B^T (+ C) + bias into the left N columns of a random [M, N + 5] matrix: element-wise within
    2e-6 * (|alpha| |A||B|^T + |bias| + |C_in|) of fp64 with the workspace the library asks for AND without one (one slice),
    the five columns to the right bit-unchanged, the workspace route bit-identical across two runs.  The operands are
    strided views inside PAD-filled allocations (head_reference.lay_out)."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    a, b, bias, c0 = R.gemm_data(case)
    want, mag = R.gemm_expected(case, a, b, bias, c0)
    a_op, b_op = _operand(a, case.a_layout), _operand(b, case.b_layout)
    assert (a_op[1] % 16 != 0) == (case.a_layout == "g_off1") and (b_op[1] % 16 != 0) == (case.b_layout == "g_off1")
    bias_dev = None if bias is None else C(bias)
    ws_bytes = _C._L.ovis_gemm_f32_workspace_bytes(case.m, case.n, case.k)
    if (case.m, case.n, case.k) in R.GEMM_SPLIT_SHAPES:
        assert ws_bytes > 0          # these cases do take the split-K route
    if case.k == 0:
        assert ws_bytes == 0
    worst = {}
    outs = []
    for route in ("raw", "raw", "one-slice"):
        rc, got = _gemm_call(case, a_op, b_op, bias_dev, c0, route)
        assert rc == OVIS_OK
        assert np.array_equal(_bits(got[:, case.n:]), _bits(c0[:, case.n:])), "columns right of the result were written"
        err = np.abs(got[:, :case.n].astype(np.float64) - want)
        assert bool(np.isfinite(got[:, :case.n]).all())
        bound = 2e-6 * mag
        worst[route] = float((err / (bound + 1e-30)).max())
        assert bool((err <= bound + 1e-30).all()), (route, worst[route])
        outs.append(got)
    assert np.array_equal(_bits(outs[0]), _bits(outs[1])), "the workspace route is not bit-reproducible"
    print(f"gemm {case.name}: ws_bytes={ws_bytes}, error / bound = {worst['raw']:.3f} (workspace) {worst['one-slice']:.3f} (one slice)")


@pytest.mark.parametrize("shape", R.GEMM_SPLIT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_f32_workspace_one_byte_short_is_enospc_and_leaves_c_untouched(shape):
    m, n, k = shape
    case = R.GemmCase("short-workspace", m, n, k, "kc", "kc", "col", 1.0, 0, 77)
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    a, b, bias, c0 = R.gemm_data(case)
    a_op, b_op = _operand(a, "kc"), _operand(b, "kc")
    need = _C._L.ovis_gemm_f32_workspace_bytes(m, n, k)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc, got = _gemm_call(case, a_op, b_op, C(bias), c0, "ws", ws, need - 1)
    assert rc == OVIS_ENOSPC
    assert np.array_equal(_bits(got), _bits(c0))
    rc, got = _gemm_call(case, a_op, b_op, C(bias), c0, "ws", ws, need)     # ... and the exact size is enough
    want, mag = R.gemm_expected(case, a, b, bias, c0)
    assert rc == OVIS_OK and bool((np.abs(got[:, :n] - want) <= 2e-6 * mag).all())


def test_gemm_f32_null_operands_and_empty_problems():
    """A null A, B or C with M, N > 0 is OVIS_EINVAL, a negative size too; M = 0 or N = 0 returns OK, launches nothing and
    writes nothing (even with null pointers)."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    case = R.GemmCase("null", 5, 7, 16, "kc", "kc", "none", 1.0, 0, 78)
    a, b, _, c0 = R.gemm_data(case)
    a_op, b_op, c = _operand(a, "kc"), _operand(b, "kc"), C(c0)
    L, s = _C._L, _C._stream()

    def call(a_ptr, b_ptr, c_ptr, m, n, k, ws=True):
        tail = (c_ptr, 7 + R.C_EXTRA, m, n, k)
        if ws:
            return L.ovis_gemm_ex_ws_f32(a_ptr, a_op[2], 1, b_ptr, b_op[2], 1, 0, 0, 1.0, 0, *tail, 0, 0, s)
        return L.ovis_gemm_ex_f32(a_ptr, a_op[2], 1, b_ptr, b_op[2], 1, 0, 0, 1.0, 0, *tail, s)

    for ws in (True, False):
        assert call(0, b_op[1], c.data_ptr(), 5, 7, 16, ws) == OVIS_EINVAL
        assert call(a_op[1], 0, c.data_ptr(), 5, 7, 16, ws) == OVIS_EINVAL
        assert call(a_op[1], b_op[1], 0, 5, 7, 16, ws) == OVIS_EINVAL
        assert call(a_op[1], b_op[1], c.data_ptr(), -1, 7, 16, ws) == OVIS_EINVAL
        assert call(a_op[1], b_op[1], c.data_ptr(), 5, 7, -1, ws) == OVIS_EINVAL
        assert call(a_op[1], b_op[1], c.data_ptr(), 0, 7, 16, ws) == OVIS_OK
        assert call(a_op[1], b_op[1], c.data_ptr(), 5, 0, 16, ws) == OVIS_OK
        assert call(0, 0, 0, 0, 0, 16, ws) == OVIS_OK
    torch.cuda.synchronize()
    assert np.array_equal(_bits(c.cpu().numpy()), _bits(c0))
    assert L.ovis_gemm_f32_workspace_bytes(0, 7, 256) == 0 and L.ovis_gemm_f32_workspace_bytes(5, 7, 0) == 0


# ------------------------------------------------------------------ region <-> noun alignment
@pytest.mark.parametrize("case", R.region_cases(), ids=lambda c: c.name)
def test_region_noun_align_edges(case):
    """P around the four waves and the 64-region chunk, D on the float4 path (8, 260, 768) and the scalar one (7, 50),
    W 1 / 9 / 65; random, all-negative and mixed-sign scores; exact ties inside a wave, between waves and between chunks,
    positive and negative.  Indices exact (tests/test_head_reference.py proves each case tie-free by twice the score bound,
    or an exact tie whose lowest index must win), raw scores within 2e-6 * sum|emb||noun| of fp64, the sigmoid as in
    test_region_noun_align_vs_torch (rtol 1e-5), two runs bit-identical."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    emb, nouns = R.region_data(case)
    _, mag = R.region_noun_scores(emb, nouns)
    want_raw, want_prob, want_idx, _ = R.region_noun(emb, nouns)
    if case.tie:
        assert bool((want_idx == case.tie[0]).all())
    emb_dev = C(emb)
    worst_raw = worst_prob = 0.0
    for w in R.REGION_W:
        nouns_dev = C(nouns[:w])
        raw, prob, idx = (t.cpu().numpy() for t in _C.region_noun_align(emb_dev, nouns_dev))
        raw2, prob2, idx2 = (t.cpu().numpy() for t in _C.region_noun_align(emb_dev, nouns_dev))
        assert raw.shape == prob.shape == idx.shape == (w,) and idx.dtype == np.int64
        assert np.array_equal(idx, want_idx[:w]), (w, idx, want_idx[:w])
        bound = R.SCORE_BOUND * mag[want_idx[:w], np.arange(w)]
        err = np.abs(raw.astype(np.float64) - want_raw[:w])
        worst_raw = max(worst_raw, float((err / (bound + 1e-30)).max()))
        assert bool((err <= bound + 1e-30).all())
        perr = np.abs(prob.astype(np.float64) - want_prob[:w]) / (1e-8 + 1e-5 * np.abs(want_prob[:w]))
        worst_prob = max(worst_prob, float(perr.max()))
        assert np.allclose(prob.astype(np.float64), want_prob[:w], rtol=1e-5, atol=1e-8)
        assert np.array_equal(_bits(raw), _bits(raw2)) and np.array_equal(_bits(prob), _bits(prob2)) and np.array_equal(idx, idx2)
    print(f"region_noun_align {case.name}: raw error / bound = {worst_raw:.3f}, sigmoid error / tolerance = {worst_prob:.3f}")


# ------------------------------------------------------------------ weighted cross entropy
def _ce_ratios(loss, grad, want_loss, want_grad, scale=1.0):
    """(loss error over 1e-5 * max(|want|, 1e-3), gradient error over atol 1e-8 + rtol 1e-4): test_weighted_ce_vs_torch's."""
    g = grad.cpu().numpy().astype(np.float64)
    return (abs(float(loss) - want_loss) / (1e-5 * max(abs(want_loss), 1e-3)),
            float((np.abs(g - scale * want_grad) / (1e-8 + 1e-4 * np.abs(scale * want_grad))).max()))


@pytest.mark.parametrize("case", R.ce_cases(), ids=lambda c: c.name)
def test_weighted_ce_edges(case):
    """C 1 / 63 / 64 / 65 / 130 and P 5 / 4 / 7 / 9 / 1030 (sum_kernel's second trip); labels with 0 and C - 1, all
    background, and -1 / C / -100 mixed in (zero loss, exactly zero gradient row, still counted in P); bg_weight 0 / 0.2 /
    1; rows that are constant, hold one entry at +-1e4 at or away from the label, are scaled x 30 or hold a -inf.  The raw
    entry and the layer with an upstream scale; ``need_grad=False`` returns None and the same loss bits."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.layers import weighted_cross_entropy

    x, lab = R.ce_data(case)
    want_loss, want_grad = R.weighted_ce(x, lab, case.bg_weight)
    xd, labd = C(x), C(lab)
    loss, grad = _C.weighted_ce_fwd_bwd(xd, labd, case.bg_weight)
    assert grad.shape == x.shape and bool(torch.isfinite(grad).all()) and bool(torch.isfinite(loss))
    r_loss, r_grad = _ce_ratios(loss, grad, want_loss, want_grad)
    print(f"weighted_ce {case.name}: loss {float(loss):.6g}, loss error / tolerance = {r_loss:.3f}, gradient error / tolerance = {r_grad:.3f}")
    assert r_loss <= 1.0
    assert np.allclose(grad.cpu().numpy().astype(np.float64), want_grad, rtol=1e-4, atol=1e-8)
    ignored = (lab < 0) | (lab >= case.c)
    assert not grad.cpu().numpy()[ignored].any()                     # exactly zero rows
    if case.bg_weight == 0:
        assert not grad.cpu().numpy()[lab == 0].any()
    loss2, none = _C.weighted_ce_fwd_bwd(xd, labd, case.bg_weight, need_grad=False)
    assert none is None and np.array_equal(_bits(loss2.cpu().numpy()), _bits(loss.cpu().numpy()))
    # the layer, with an upstream scale
    xg = C(x).requires_grad_(True)
    got = weighted_cross_entropy(xg, labd, case.bg_weight)
    (got * 1.7).backward()
    assert np.array_equal(_bits(got.detach().cpu().numpy()), _bits(loss.cpu().numpy()))
    assert np.allclose(xg.grad.cpu().numpy().astype(np.float64), 1.7 * want_grad, rtol=1e-4, atol=1e-8)
    assert not xg.grad.cpu().numpy()[ignored].any()


# ------------------------------------------------------------------ stochastic mask BCE
def _mask_raw(d, case, need_grad=True):
    """The C entry points themselves, ``mask_pixels`` given directly: the fixed-channel entry for an int channel, the
    per-class entry for a channel tensor.  -> (loss tensor [1], dmu, dsigma)"""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    mu, pos, tg = C(d["mu"]), C(d["pos"]), C(d["targets"])
    sigma = None if d["sigma"] is None else C(d["sigma"])
    eps = None if d["eps"] is None else C(d["eps"])
    p, c, npos = case.p, case.c, case.npos
    mm = int(np.prod(case.shape))
    loss = torch.full((1,), 123.0, device="cuda")
    dmu = torch.full_like(mu, 7.0) if need_grad else None
    dsigma = torch.full_like(sigma, 7.0) if (need_grad and sigma is not None) else None
    scratch = torch.empty(max(npos, 1), device="cuda")
    ptr = lambda t: 0 if t is None else t.data_ptr()
    if np.ndim(d["channel"]) == 0:
        rc = _C._L.ovis_mask_bce_stochastic_fwd_bwd_f32(mu.data_ptr(), ptr(sigma), ptr(eps), pos.data_ptr(), tg.data_ptr(),
                                                        loss.data_ptr(), ptr(dmu), ptr(dsigma), scratch.data_ptr(), p, npos, c,
                                                        mm, int(d["channel"]), _C._stream())
    else:
        ch = C(d["channel"])
        rc = _C._L.ovis_mask_bce_stochastic_classes_fwd_bwd_f32(mu.data_ptr(), ptr(sigma), ptr(eps), pos.data_ptr(),
                                                                ch.data_ptr(), tg.data_ptr(), loss.data_ptr(), ptr(dmu),
                                                                ptr(dsigma), scratch.data_ptr(), p, npos, c, mm, _C._stream())
    torch.cuda.synchronize()
    assert rc == OVIS_OK
    return loss[0], dmu, dsigma


def _mask_check(case, d, loss, dmu, dsigma, want, scale=1.0):
    """Loss 1e-5 relative, gradients rtol 1e-4 / atol 1e-9 (test_stochastic_mask_bce_vs_torch's), exactly 0.0 outside the
    selected planes.  -> (loss ratio, gradient ratio)"""
    want_loss, want_dmu, want_dsigma = want
    assert bool(torch.isfinite(loss))
    r_loss = abs(float(loss) - want_loss) / (1e-5 * abs(want_loss)) if want_loss else float(float(loss) != 0.0)
    assert abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss), r_loss
    g = dmu.cpu().numpy()
    assert g.shape == d["mu"].shape and bool(np.isfinite(g).all())
    r_grad = float((np.abs(g - scale * want_dmu) / (1e-9 + 1e-4 * np.abs(scale * want_dmu))).max())
    assert np.allclose(g.astype(np.float64), scale * want_dmu, rtol=1e-4, atol=1e-9), r_grad
    sel = R.selected_planes(d["mu"].shape, d["pos"], d["channel"])
    assert not g[~sel].any()                                          # exactly 0.0 outside the selected planes
    if case.npos:
        assert bool(g[sel].any(axis=tuple(range(1, g[sel].ndim))).all())   # ... and every selected plane did get one
    assert (dsigma is None) == (d["sigma"] is None)
    if dsigma is not None:
        gs = dsigma.cpu().numpy()
        assert gs.shape == d["sigma"].shape
        assert np.allclose(gs.astype(np.float64), scale * want_dsigma, rtol=1e-4, atol=1e-9)
        r_grad = max(r_grad, float((np.abs(gs - scale * want_dsigma) / (1e-9 + 1e-4 * np.abs(scale * want_dsigma))).max()))
        rest = np.ones(case.p, dtype=bool)
        rest[d["pos"]] = False
        assert not gs[rest].any()
        if d["eps"] is None:
            assert not gs.any()                                       # sigma without eps: z = mu, d sigma = 0
    return r_loss, r_grad


@pytest.mark.parametrize("case", R.mask_cases(), ids=lambda c: c.name)
def test_mask_bce_edges(case):
    """MM 1 / 196 / 256 / 784 and flat 63 / 255 / 257 (through the C entries with ``mask_pixels`` given directly); npos 0 /
    1 / P / 1030; unsorted positives; channel 0, C - 1 and per-positive channels with -1 and C (the clamp shows in which
    plane holds the gradient); sigma and eps both, neither, and one without the other (z = mu); mu = +-100 and +-1e4 against
    both target values (loss term |z| or 0, gradient +-1/n or 0, everything finite).  Both C entry points, ``_C``, and the
    layer with an upstream scale; ``need_grad=False`` returns the same loss bits."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    from cvpr22_cross_modal_pseudo_labeling_amd.layers import stochastic_mask_bce

    d = R.mask_data(case)
    want = R.mask_bce(d["mu"], d["sigma"], d["eps"], d["pos"], d["channel"], d["targets"])
    loss, dmu, dsigma = _mask_raw(d, case)
    ratios = _mask_check(case, d, loss, dmu, dsigma, want)
    print(f"mask_bce {case.name}: loss {float(loss):.6g}, loss error / tolerance = {ratios[0]:.3f}, gradient error / tolerance = {ratios[1]:.3f}")
    loss_ng, none1, none2 = _mask_raw(d, case, need_grad=False)
    assert none1 is None and none2 is None and np.array_equal(_bits(loss_ng.cpu().numpy()), _bits(loss.cpu().numpy()))
    n = max(case.npos, 1) * int(np.prod(case.shape))
    if case.extreme:
        ch0 = int(R.clamp_channels(d["channel"], case.npos, case.c)[0])
        g8 = dmu.cpu().numpy().reshape(case.p, case.c, -1)[d["pos"][0], ch0, :8].astype(np.float64) * n
        assert np.allclose(g8, [1, 0, 0, -1, 1, 0, 0, -1], rtol=0, atol=1e-6)
    if np.ndim(d["channel"]) == 0 and case.npos:   # the per-class entry given the same channel for every positive: same bits
        same = dict(d, channel=np.full(case.npos, d["channel"], dtype=np.int64))
        loss_c, dmu_c, _ = _mask_raw(same, case)
        assert np.array_equal(_bits(loss_c.cpu().numpy()), _bits(loss.cpu().numpy())) and torch.equal(dmu_c, dmu)
    if case.raw:
        return
    # the package's entry and the layer (maps [.., M, M]; the channel as an int or a tensor)
    mu, pos, tg = C(d["mu"]), C(d["pos"]), C(d["targets"])
    sigma = None if d["sigma"] is None else C(d["sigma"])
    eps = None if d["eps"] is None else C(d["eps"])
    channel = d["channel"] if np.ndim(d["channel"]) == 0 else C(d["channel"])
    loss_p, dmu_p, dsigma_p = _C.mask_bce_stochastic_fwd_bwd(mu, sigma, eps, pos, tg, channel)
    assert np.array_equal(_bits(loss_p.cpu().numpy()), _bits(loss.cpu().numpy())) and torch.equal(dmu_p, dmu)
    assert (dsigma_p is None) == (dsigma is None) and (dsigma is None or torch.equal(dsigma_p, dsigma))
    loss_p2, n1, n2 = _C.mask_bce_stochastic_fwd_bwd(mu, sigma, eps, pos, tg, channel, need_grad=False)
    assert n1 is None and n2 is None and np.array_equal(_bits(loss_p2.cpu().numpy()), _bits(loss.cpu().numpy()))
    mu_g = C(d["mu"]).requires_grad_(True)
    sigma_g = None if sigma is None else C(d["sigma"]).requires_grad_(True)
    got = stochastic_mask_bce(mu_g, sigma_g, eps, pos, tg.reshape(case.npos, int(np.prod(case.shape))), channel)
    (got * 0.6).backward()
    assert np.array_equal(_bits(got.detach().cpu().numpy()), _bits(loss.cpu().numpy()))
    _mask_check(case, d, got.detach(), mu_g.grad, None if sigma_g is None else sigma_g.grad, want, scale=0.6)
