"""TEST INFRASTRUCTURE ONLY -- operands whose three-term bf16 hi/lo product is EXACTLY representable in fp32, and the
exact value the split GEMM kernels of csrc/split_gemm.hip must then return whatever their slice plan, tile order or LDS
staging.  NumPy on the host; nothing from the package (the pair rows are written here, bit by bit, from values that are
exact in bf16).  Pinned by tests/test_exact_product_reference.py, used by tests/test_split_gemm_exact_gpu.py.

THE GRID.  x = a + b * 2^-9 with a in {-2 .. 2}, b in {-1, 0, 1}, b = 0 where a = 0.  Then hi = bf16(x) = a (|b| 2^-9 is
below half an ulp of bf16 at 1 and at 2: 2^-8 resp. 2^-7), lo = bf16(x - hi) = b 2^-9, hi + lo == x.  Every product
the kernels form -- hi.hi, hi.lo, lo.hi -- is a multiple of 2^-9 (lo.lo = 2^-18 b b' is the term they drop).  With

    S = sum_k |hi_a hi_b| + |hi_a lo_b| + |lo_a hi_b|        (THE BUDGET)

every partial sum of every subset of the terms is a multiple of 2^-9 of magnitude <= S; below 2^15 that is a 24-bit
integer times 2^-9: exact in fp32, in ANY order of accumulation.  Integer operands (``lo=False``) have unit 1 and the
budget 2^24.  The budget is a condition on the INPUTS and is asserted before any device value is looked at.
"""
import numpy as np

LO_UNIT = 2.0 ** -9
BUDGET_LO = 2.0 ** 15       # lo-bearing operands: multiples of 2^-9 below 2^15 are exact in fp32
BUDGET_INT = 2.0 ** 24      # integer operands


def grid(rows, cols, lo=True, seed=0):
    """fp32 [rows, cols] of grid values, deterministic in (rows, cols, lo, seed).  ``lo=False``: the integers a alone."""
    rng = np.random.default_rng([int(seed), int(rows), int(cols), int(bool(lo))])
    a = rng.integers(-2, 3, size=(rows, cols))
    b = rng.integers(-1, 2, size=(rows, cols)) if lo else np.zeros((rows, cols), dtype=np.int64)
    b = np.where(a == 0, 0, b)
    return (a + b * LO_UNIT).astype(np.float32)


def _bf16_round(x32):
    """fp32 -> the nearest bf16 value (ties to even) as fp32, on the bit pattern."""
    bits = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    kept = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint32) << 16
    return kept.view(np.float32).reshape(np.shape(x32))


def split(x):
    """x fp32 -> (hi, lo) fp32 by the two bf16 roundings of the pair layout; asserts the grid's properties."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = _bf16_round(x)
    lo = _bf16_round(x - hi)
    assert np.array_equal(hi + lo, x), "hi + lo != x: not a grid value"
    assert np.array_equal(hi, np.rint(hi)), "hi is not an integer"
    assert float(np.abs(lo).max(initial=0.0)) <= LO_UNIT, "|lo| > 2^-9"
    return hi, lo


def pair_bits(x):
    """x fp32 [rows, K] of grid values (K % 32 == 0) -> uint16 [rows, 2K] pair rows: per 32 values [hi(32) | lo(32)]."""
    hi, lo = split(x)
    rows, k = hi.shape
    assert k % 32 == 0
    out = np.empty((rows, k // 32, 2, 32), dtype=np.uint16)
    out[:, :, 0, :] = (hi.view(np.uint32) >> 16).astype(np.uint16).reshape(rows, k // 32, 32)
    out[:, :, 1, :] = (lo.view(np.uint32) >> 16).astype(np.uint16).reshape(rows, k // 32, 32)
    return out.reshape(rows, 2 * k)


def budget_limit(*operands):
    """2^15 when any operand carries a lo part, 2^24 for integers."""
    return BUDGET_INT if all(np.array_equal(o, np.rint(o)) for o in operands) else BUDGET_LO


def fp32_exact(v64):
    return np.array_equal(v64.astype(np.float32).astype(np.float64), v64)


def three_term(A, B):
    """A [p, q], B [q, r] fp32 grid values -> (A_hi B_hi + A_hi B_lo + A_lo B_hi as fp64 [p, r], the budget S [p, r]).
    Asserts S below the budget of the operands and the value representable in fp32."""
    ah, al = (t.astype(np.float64) for t in split(A))
    bh, bl = (t.astype(np.float64) for t in split(B))
    val = ah @ bh + ah @ bl + al @ bh
    S = np.abs(ah) @ np.abs(bh) + np.abs(ah) @ np.abs(bl) + np.abs(al) @ np.abs(bh)
    limit = budget_limit(A, B)
    assert float(S.max(initial=0.0)) < limit, f"budget {float(S.max())} >= {limit}: the contraction is too long for these operands"
    assert fp32_exact(val)
    return val, S


def tap_rows(x, r, h, w, kh, kw, flip=False):
    """x [r*h*w, ch] (NHWC rows) -> [r*h*w, kh*kw*ch] tap-major patch rows, zeros outside the map: tap (ty, tx) of pixel
    (y, x) holds pixel (y + ty - kh//2, x + tx - kw//2) of the same map -- the offsets negated when ``flip`` (the
    data-gradient convolution).  The layout of ``conv_weight_matrix``: k = (ty*kw + tx)*ch + c.  Plain index loops."""
    x = np.asarray(x)
    ch = x.shape[1]
    assert x.shape[0] == r * h * w
    src = x.reshape(r, h, w, ch)
    out = np.zeros((r, h, w, kh * kw, ch), dtype=x.dtype)
    for ty in range(kh):
        for tx in range(kw):
            dy, dx = ty - kh // 2, tx - kw // 2
            if flip:
                dy, dx = -dy, -dx
            for y in range(h):
                for xx in range(w):
                    sy, sx = y + dy, xx + dx
                    if 0 <= sy < h and 0 <= sx < w:
                        out[:, y, xx, ty * kw + tx, :] = src[:, sy, sx, :]
    return out.reshape(r * h * w, kh * kw * ch)


# ------------------------------------------------------------------ epilogue operands and the expected epilogue
def bias(n, seed):
    return grid(1, n, True, seed)[0]


def residual(m, n, seed):
    """A shortcut operand from the grid: as fp32 it is added as it is, in pair layout as hi + lo == the same value."""
    return grid(m, n, True, seed)


def gate01(m, n, seed):
    """The forward activation of a ReLU gate, 0 or 1 (both exact in bf16; the kernels read the hi halves: open where > 0)."""
    return np.random.default_rng([int(seed), int(m), int(n)]).integers(0, 2, size=(m, n)).astype(np.float32)


def epilogue(val, S, bias=None, residual=None, relu=False, gate=None, limit=BUDGET_LO):
    """act(val + bias + residual) * (gate > 0) as fp32, exact: the budget with |bias| and |residual| added stays below
    ``limit`` (asserted), so every intermediate of the kernels' fp32 epilogue is representable."""
    v = val.copy()
    S = S.copy()
    if bias is not None:
        v += bias.astype(np.float64)[None, :]
        S += np.abs(bias.astype(np.float64))[None, :]
    if residual is not None:
        v += residual.astype(np.float64)
        S += np.abs(residual.astype(np.float64))
    assert float(S.max(initial=0.0)) < limit
    if relu:
        v = np.maximum(v, 0.0)
    if gate is not None:
        v = v * (gate > 0)
    v = v + 0.0     # -0 -> +0 never arises from sums of these values; keep the representation canonical anyway
    assert fp32_exact(v)
    return v.astype(np.float32)


def pooled_mean(final, S, pool_rows, limit=BUDGET_LO):
    """Mean over every ``pool_rows`` consecutive rows of the final values, pool_rows a power of two: sums of at most
    pool_rows values of budget S each, scaled by an exact power of two."""
    m, n = final.shape
    assert m % pool_rows == 0 and pool_rows & (pool_rows - 1) == 0
    assert float(S.reshape(m // pool_rows, pool_rows, n).sum(1).max(initial=0.0)) < limit
    out = final.astype(np.float64).reshape(m // pool_rows, pool_rows, n).sum(1) / pool_rows
    assert fp32_exact(out)
    return out.astype(np.float32)
