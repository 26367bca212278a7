"""CPU: pins tests/head_reference.py before any kernel is measured against it -- the GEMM to torch float64 matmul, the two
losses to torch float64 autograd of ``F.cross_entropy(weight=...)`` and ``F.binary_cross_entropy_with_logits`` on every case
the GPU tests use (tests/test_head_kernels_edges_gpu.py), the alignment to ``torch.max`` in float64 -- and proves each
case's own precondition: operand layouts that lie inside their allocation and select the load mode they claim, alignment
cases that are tie-free by a stated gap or exact ties, planted rows that are what their names say."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import head_reference as R


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _close(got, want, rel=1e-12, floor=1e-300):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return bool((np.abs(got - want) <= rel * np.maximum(np.abs(want), floor)).all())


# ------------------------------------------------------------------ GEMM
def test_gemm_case_list_covers_what_it_claims():
    cases = R.gemm_cases()
    assert len({c.name for c in cases}) == len(cases)
    for shape in R.GEMM_SHAPES:
        here = [c for c in cases if (c.m, c.n, c.k) == shape]
        assert {(c.a_layout, c.b_layout) for c in here} == {(a, b) for a in R.LAYOUTS for b in R.LAYOUTS}
    assert {(c.bias, c.alpha, c.accumulate) for c in cases} == set(R.EPILOGUES)
    for shape in ((65, 63, 17),) + R.GEMM_SPLIT_SHAPES + ((5, 7, 0),):
        assert {(c.bias, c.alpha, c.accumulate) for c in cases if (c.m, c.n, c.k) == shape} == set(R.EPILOGUES), shape
    assert any((c.m, c.n, c.k) in R.GEMM_SPLIT_SHAPES and c.accumulate and c.bias == "row" for c in cases)


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("rows,k", [(64, 16), (65, 17), (130, 1000), (1, 1), (5, 0)])
def test_layouts_lie_inside_their_buffer_and_select_their_mode(layout, rows, k):
    """The strided view reproduces the operand, touches nothing outside the buffer, leaves PAD everywhere else, and its
    (strides, offset) are what the library's mode choice looks at: kc / rc qualify for a float4 mode, the three generic
    ones each fail exactly the condition they are named after."""
    x = np.random.default_rng(rows + k).standard_normal((rows, k)).astype(np.float32)
    buf, off, rs, ks = R.lay_out(x, layout)
    idx = off + np.arange(rows)[:, None] * rs + np.arange(k)[None, :] * ks
    if idx.size:
        assert 0 <= idx.min() and idx.max() < buf.size and np.unique(idx).size == idx.size
        assert np.array_equal(buf[idx], x)
    rest = np.ones(buf.size, dtype=bool)
    rest[idx.ravel()] = False
    assert bool((buf[rest] == R.PAD).all())
    aligned = off % 4 == 0  # the buffer itself is uploaded to a 16-byte aligned allocation
    k_vec = ks == 1 and rs % 4 == 0 and aligned
    r_vec = rs == 1 and ks % 4 == 0 and aligned
    assert (k_vec, r_vec) == {"kc": (True, False), "rc": (False, True)}.get(layout, (False, False))
    if layout == "g_2d":
        assert rs > 1 and ks > 1
    if layout == "g_rs2":
        assert ks == 1 and rs % 4 == 2 and aligned
    if layout == "g_off1":
        assert ks == 1 and rs % 4 == 0 and off == 1


@pytest.mark.parametrize("case", R.gemm_cases(), ids=lambda c: c.name)
def test_gemm_vs_torch_float64(case):
    a, b, bias, c0 = R.gemm_data(case)
    want, mag = R.gemm_expected(case, a, b, bias, c0)
    ref = case.alpha * (T(a).double() @ T(b).double().t())
    bound = abs(case.alpha) * (T(a).double().abs() @ T(b).double().abs().t())
    if case.accumulate:
        ref, bound = ref + T(c0[:, :case.n]).double(), bound + T(c0[:, :case.n]).double().abs()
    if bias is not None:
        v = T(bias).double()[:, None] if case.bias == "row" else T(bias).double()[None, :]
        ref, bound = ref + v, bound + v.abs()
    assert want.shape == (case.m, case.n) == mag.shape
    assert bool((np.abs(want - ref.numpy()) <= 1e-13 * bound.numpy() + 1e-300).all())
    assert _close(mag, bound.numpy())
    if case.k == 0:  # the empty sum: the bias, or C + bias
        by_hand = np.zeros((case.m, case.n)) + (c0[:, :case.n].astype(np.float64) if case.accumulate else 0.0)
        if bias is not None:
            by_hand = by_hand + (bias.astype(np.float64)[:, None] if case.bias == "row" else bias.astype(np.float64)[None, :])
        assert np.array_equal(want, by_hand)


# ------------------------------------------------------------------ region <-> noun alignment
@pytest.mark.parametrize("case", R.region_cases(), ids=lambda c: c.name)
def test_region_noun_vs_torch_max_and_case_preconditions(case):
    emb, nouns = R.region_data(case)
    assert emb.shape == (case.p, case.d) and nouns.shape == (max(R.REGION_W), case.d)
    raw, prob, idx, gap = R.region_noun(emb, nouns)
    scores = T(emb).double() @ T(nouns).double().t()
    t_raw, t_idx = torch.max(scores, dim=0)
    assert _close(raw, t_raw.numpy(), rel=1e-12, floor=1e-6)
    assert _close(prob, torch.sigmoid(t_raw).numpy(), rel=1e-10)
    min_gap = R.region_min_gap(emb, nouns)
    assert bool((min_gap > 0).all())
    if case.tie is None:
        # tie-free: the runner-up is further away than twice the kernel's score bound, so the index is decided
        assert np.array_equal(idx, t_idx.numpy())
        assert bool((gap >= min_gap).all())
    else:
        lo, hi = case.tie
        assert np.array_equal(emb[lo], emb[hi]) and lo < hi
        assert bool((gap == 0).all()) and bool((idx == lo).all())          # an exact tie, the lowest index
        without = R.region_noun(np.delete(emb, hi, axis=0), nouns)
        assert bool((without[2] == lo).all()) and bool((without[3] >= min_gap).all())   # ... and nothing else near it
    for w in R.REGION_W:  # a case's nouns are the first W rows: the per-noun results do not depend on W
        part = R.region_noun(emb, nouns[:w])
        assert np.array_equal(part[0], raw[:w]) and np.array_equal(part[2], idx[:w])
    if case.kind in ("negative", "tie-negative"):
        assert bool((R.region_noun_scores(emb, nouns)[0] < 0).all())
    if case.kind == "tie-positive":
        assert bool((raw > 0).all())
    if case.kind == "mixed":  # negative maxima for the even nouns (noun 0 among them: W = 1), positive for the odd ones
        assert bool((raw[0::2] < 0).all()) and bool((raw[1::2] > 0).all())
    if case.kind == "random" and case.p >= 63:
        assert bool((raw > 0).any())


def test_region_case_list():
    cases = R.region_cases()
    assert len({c.name for c in cases}) == len(cases)
    plain = {(c.p, c.d, c.kind) for c in cases if c.tie is None}
    assert plain == {(p, d, k) for p in R.REGION_P for d in R.REGION_D for k in R.REGION_KINDS}
    assert {c.tie for c in cases if c.tie} == set(R.REGION_TIES)
    # rows 1 and 2: different waves (p % 4) of one chunk (p // 64); 1 and 5: one wave; 5 and 70: different chunks
    assert (1 // 64, 1 % 4) != (2 // 64, 2 % 4) and 1 // 64 == 2 // 64 and 1 % 4 == 5 % 4 and 5 // 64 != 70 // 64


# ------------------------------------------------------------------ weighted cross entropy
def _torch_ce(x, lab, bg):
    xr = T(x).double().requires_grad_(True)
    w = torch.ones(x.shape[1], dtype=torch.float64)
    w[0] = float(np.float32(bg))
    loss = (F.cross_entropy(xr, T(lab), weight=w, reduction="none") / x.shape[0]).sum()
    loss.backward()
    return loss.item(), xr.grad.numpy()


@pytest.mark.parametrize("case", R.ce_cases(), ids=lambda c: c.name)
def test_weighted_ce_vs_torch_float64_autograd(case):
    x, lab = R.ce_data(case)
    p, c = case.p, case.c
    assert x.shape == (p, c) and lab.shape == (p,)
    loss, grad = R.weighted_ce(x, lab, case.bg_weight)
    assert np.isfinite(loss) and bool(np.isfinite(grad).all())
    valid = (lab >= 0) & (lab < c)
    if case.labels == "ignored":
        # torch refuses labels outside [0, C): pinned through the rows that count -- the ignored rows add nothing to
        # the sum, get a zero gradient row and still divide it, so the valid rows' result scales by their share of P
        assert {-1, c, -100} <= set(lab.tolist()) and 0 < valid.sum() < p and lab[0] == c - 1
        t_loss, t_grad = _torch_ce(x[valid], lab[valid], case.bg_weight)
        share = valid.sum() / p
        assert abs(loss - t_loss * share) <= 1e-12 * abs(t_loss)
        assert _close(grad[valid], t_grad * share, rel=1e-10, floor=1e-30)
        assert not grad[~valid].any()
    else:
        assert bool(valid.all())
        t_loss, t_grad = _torch_ce(x, lab, case.bg_weight)
        assert abs(loss - t_loss) <= 1e-12 * max(abs(t_loss), 1e-30)
        assert _close(grad, t_grad, rel=1e-10, floor=1e-30)
    if case.labels == "random" and case.logits == "randn3":
        assert 0 in lab and c - 1 in lab
    if case.labels == "background":
        assert not lab.any()
        if case.bg_weight == 0:
            assert loss == 0.0 and not grad.any()
    if case.logits != "randn3":  # the planted rows are what they are called
        for r, plant in enumerate(case.logits):
            row, l = x[r].astype(np.float64), lab[r]
            others = np.delete(row, l)
            if plant == "const":
                assert bool((row == row[0]).all())
            elif plant == "big-off-label":
                assert others.max() == 1e4 and abs(row[l]) < 50
            elif plant == "big-at-label":
                assert row[l] == 1e4
            elif plant == "small-at-label":
                assert row[l] == -1e4
            elif plant == "small-off-label":
                assert others.min() == -1e4 and abs(row[l]) < 50
            elif plant == "x30":
                assert np.abs(row).max() > 30 or c == 1
            elif plant == "neginf-off-label":
                assert np.isneginf(others).sum() == 1 and np.isfinite(row[l])


def test_ce_case_list():
    cases = R.ce_cases()
    assert len({c.name for c in cases}) == len(cases)
    for p, c in R.CE_SHAPES:
        here = [k for k in cases if (k.p, k.c) == (p, c)]
        assert {k.bg_weight for k in here if k.logits == "randn3" and k.labels == "random"} == {0.0, 0.2, 1.0}
        assert {k.labels for k in here} == {"random", "background", "ignored"}
        planted = {pl for k in here if k.logits != "randn3" for pl in k.logits}
        assert planted == {name for name, two in R.CE_PLANTS if c > 1 or not two}


# ------------------------------------------------------------------ mask BCE
@pytest.mark.parametrize("case", R.mask_cases(), ids=lambda c: c.name)
def test_mask_bce_vs_torch_float64_autograd(case):
    d = R.mask_data(case)
    mu, sigma, eps, pos, channel, tg = d["mu"], d["sigma"], d["eps"], d["pos"], d["channel"], d["targets"]
    p, c, npos = case.p, case.c, case.npos
    assert pos.size == npos and np.unique(pos).size == npos and (npos < 3 or not bool((np.diff(pos) > 0).all()))
    assert (sigma is not None, eps is not None) == {"both": (True, True), "neither": (False, False),
                                                    "sigma-only": (True, False), "eps-only": (False, True)}[case.noise]
    loss, dmu, dsigma = R.mask_bce(mu, sigma, eps, pos, channel, tg)
    assert dmu.shape == mu.shape and (dsigma is None) == (sigma is None) and (sigma is None or dsigma.shape == sigma.shape)
    assert np.isfinite(loss) and bool(np.isfinite(dmu).all())
    sel = R.selected_planes(mu.shape, pos, channel)
    assert sel.sum() == npos and not dmu[~sel].any()
    ch = R.clamp_channels(channel, npos, c)
    if case.channel == "per" and npos:
        assert channel[-1] == c and (npos == 1 or channel[0] == -1) and ch.min() >= 0 and ch.max() <= c - 1
        # the clamp: the same result as with the channels clamped by hand
        again = R.mask_bce(mu, sigma, eps, pos, ch, tg)
        assert again[0] == loss and np.array_equal(again[1], dmu)
    if npos == 0:
        assert loss == 0.0 and not dmu.any() and (dsigma is None or not dsigma.any())
        return
    m = T(mu).double().requires_grad_(True)
    s = None if sigma is None else T(sigma).double().requires_grad_(True)
    z = m + T(eps).double() * s if (sigma is not None and eps is not None) else m
    picked = z[T(pos), T(ch)].reshape(npos, -1)
    want = F.binary_cross_entropy_with_logits(picked, T(tg).double().reshape(npos, -1), reduction="mean")
    want.backward()
    assert abs(loss - want.item()) <= 1e-12 * abs(want.item())
    assert _close(dmu, m.grad.numpy(), rel=1e-10, floor=1e-30)
    if sigma is not None:
        if eps is None:
            assert not dsigma.any() and s.grad is None
        else:
            assert _close(dsigma, s.grad.numpy(), rel=1e-10, floor=1e-30)
            gone = np.ones(p, dtype=bool)
            gone[pos] = False
            assert not dsigma[gone].any()
    if case.extreme:
        n = npos * int(np.prod(case.shape))
        g = dmu.reshape(p, c, -1)[pos[0], ch[0], :8] * n
        zz = picked.detach().numpy()[0, :8]
        assert bool((np.abs(zz) > 90).all()) and np.array_equal(np.sign(zz), np.sign(R.MASK_EXTREME_MU))
        # the term is |z| where the target contradicts the sign and 0 where it agrees; the gradient is +-1/n or 0
        assert np.allclose(g, [1, 0, 0, -1, 1, 0, 0, -1], rtol=0, atol=1e-12)


def test_mask_case_list():
    cases = R.mask_cases()
    assert len({c.name for c in cases}) == len(cases)
    for p, c, m in R.MASK_SHAPES:
        here = [k for k in cases if (k.p, k.c, k.shape) == (p, c, (m, m))]
        assert {k.noise for k in here} == set(R.MASK_NOISE) and {k.channel for k in here} == {"first", "last", "per"}
        assert {0, 1, p} <= {k.npos for k in here}
    assert {k.shape[0] for k in cases if k.raw} == set(R.MASK_FLAT_MM) and all(k.shape[1] == 1 for k in cases if k.raw)
    assert any(k.npos == 1030 and k.shape == (1, 1) for k in cases)
    assert {k.noise for k in cases if k.extreme} == set(R.MASK_NOISE)
