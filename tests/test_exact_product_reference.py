"""CPU: tests/exact_product_reference.py is what it says -- the grid's hi / lo properties, the three-term value against an
independent fp64 spelling, order independence of an fp32 accumulation, ``tap_rows`` against ``F.unfold``, and the budget
assertion.  These are the premises tests/test_split_gemm_exact_gpu.py compares the kernels with, bit for bit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import exact_product_reference as E


@pytest.mark.parametrize("lo", [True, False])
def test_grid_has_the_stated_properties(lo):
    x = E.grid(257, 96, lo, seed=3)
    assert x.dtype == np.float32 and np.array_equal(x, E.grid(257, 96, lo, seed=3))
    assert not np.array_equal(x, E.grid(257, 96, lo, seed=4))
    hi, lo_part = E.split(x)
    # the roundings agree with torch's bf16 cast
    t = torch.from_numpy(x)
    thi = t.bfloat16().float()
    assert np.array_equal(hi, thi.numpy()) and np.array_equal(lo_part, (t - thi).bfloat16().float().numpy())
    assert set(np.unique(hi)) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert set(np.unique(lo_part / E.LO_UNIT)) == ({-1.0, 0.0, 1.0} if lo else {0.0})
    assert not lo_part[hi == 0].any()
    assert np.array_equal(hi + lo_part, x)
    # the pair rows hold exactly these values, block by block
    p = E.pair_bits(x).reshape(257, 3, 2, 32)
    back = (p.astype(np.uint32) << 16).view(np.float32)
    assert np.array_equal(back[:, :, 0].reshape(257, 96), hi) and np.array_equal(back[:, :, 1].reshape(257, 96), lo_part)


def test_split_refuses_values_off_the_grid():
    with pytest.raises(AssertionError):
        E.split(np.array([[1.0 + 2.0 ** -9 + 2.0 ** -20]], dtype=np.float32))   # hi + lo != x
    with pytest.raises(AssertionError):
        E.split(np.array([[0.5]], dtype=np.float32))                   # hi not integral
    with pytest.raises(AssertionError):
        E.split(np.array([[1.0 + 2.0 ** -8]], dtype=np.float32))       # |lo| > 2^-9


@pytest.mark.parametrize("m,k,n", [(300, 4608, 132), (129, 8160, 64)])
def test_three_term_is_the_product_without_lo_lo_and_any_fp32_order_reproduces_it(m, k, n):
    A, B = E.grid(m, k, True, seed=1), E.grid(k, n, True, seed=2)
    val, S = E.three_term(A, B)
    print(f"{m} x {k} x {n}: largest budget S = {S.max():.0f}")
    assert S.max() < E.BUDGET_LO and (np.abs(val) <= S).all()
    ah, al = (t.astype(np.float64) for t in E.split(A))
    bh, bl = (t.astype(np.float64) for t in E.split(B))
    full = (ah + al) @ (bh + bl)                                       # exact in fp64: multiples of 2^-18 below 2^15
    assert np.array_equal(val, full - al @ bl)
    assert E.fp32_exact(val)
    # the dropped lo.lo term is visible in fp32: the test states three terms, not four
    assert (full.astype(np.float32) != val.astype(np.float32)).any()
    assert np.abs(al @ bl).max() >= 2.0 ** -13
    # an fp32 accumulation of the 3k terms in a shuffled order, in blocks of 37, gives the same bits
    rng = np.random.default_rng(5)
    lhs = np.concatenate([ah, ah, al], 1).astype(np.float32)
    rhs = np.concatenate([bh, bl, bh], 0).astype(np.float32)
    order = rng.permutation(3 * k)
    acc = np.zeros((m, n), dtype=np.float32)
    for s in range(0, 3 * k, 37):
        idx = order[s:s + 37]
        part = np.zeros((m, n), dtype=np.float32)
        for j in idx:                                                  # one rank-1 update per term: fp32 adds only
            part += np.outer(lhs[:, j], rhs[j])
        acc += part
    assert np.array_equal(acc, val.astype(np.float32))


def test_three_term_budget_assertion_fires_on_an_over_long_contraction():
    A, B = E.grid(4, 40000, True, seed=1), E.grid(40000, 4, True, seed=2)
    with pytest.raises(AssertionError, match="budget"):
        E.three_term(A, B)
    Ai, Bi = E.grid(4, 40000, False, seed=1), E.grid(40000, 4, False, seed=2)   # integers: the budget is 2^24
    val, S = E.three_term(Ai, Bi)
    assert S.max() < E.BUDGET_INT and np.array_equal(val, Ai.astype(np.float64) @ Bi.astype(np.float64))


@pytest.mark.parametrize("r,h,w,kh,kw", [(3, 7, 7, 3, 3), (2, 5, 9, 3, 5), (2, 1, 7, 3, 3), (2, 7, 1, 3, 5), (4, 1, 1, 3, 3),
                                         (1, 2, 8, 7, 1), (1, 8, 2, 1, 7), (2, 4, 6, 1, 1)])
def test_tap_rows_equals_unfold(r, h, w, kh, kw):
    ch = 5
    x = np.random.default_rng(r * 100 + h * 10 + w).standard_normal((r * h * w, ch))
    got = E.tap_rows(x, r, h, w, kh, kw)
    cols = F.unfold(torch.from_numpy(x).view(r, h, w, ch).permute(0, 3, 1, 2), (kh, kw), padding=(kh // 2, kw // 2))
    want = cols.view(r, ch, kh * kw, h * w).permute(0, 3, 2, 1).reshape(r * h * w, kh * kw * ch).numpy()
    assert np.array_equal(got, want)
    # flip negates the tap offsets: the taps in reverse order
    flipped = E.tap_rows(x, r, h, w, kh, kw, flip=True)
    assert np.array_equal(flipped.reshape(-1, kh * kw, ch), want.reshape(-1, kh * kw, ch)[:, ::-1])


def test_epilogue_helpers_are_exact_and_guarded():
    A, B = E.grid(128, 64, True, seed=7), E.grid(64, 32, True, seed=8)
    val, S = E.three_term(A, B)
    b, res, gate = E.bias(32, 9), E.residual(128, 32, 10), E.gate01(128, 32, 11)
    assert set(np.unique(gate)) == {0.0, 1.0}
    out = E.epilogue(val, S, b, res, relu=True, gate=gate)
    want = np.maximum(val + b.astype(np.float64) + res.astype(np.float64), 0.0) * gate
    assert out.dtype == np.float32 and np.array_equal(out.astype(np.float64), want)
    assert (out[gate == 0] == 0).all() and (out >= 0).all() and out.any()
    pooled = E.pooled_mean(out, S + np.abs(b) + np.abs(res), 64)
    assert pooled.shape == (2, 32) and np.array_equal(pooled.astype(np.float64), want.reshape(2, 64, 32).mean(1))
    with pytest.raises(AssertionError):
        E.epilogue(val, S + E.BUDGET_LO, b)
