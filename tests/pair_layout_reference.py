"""TEST INFRASTRUCTURE ONLY -- NumPy restatement of the PAIR LAYOUT of include/ovis_hip.h and of the byte-moving kernels
that write it (csrc/split_gemm.hip: split_pair, gate_split_pair, im2col_nchw_pair, weight_prep_pair, im2col_pair,
slab_reduce; csrc/weight_prep_multi.hip computes what weight_prep_pair computes).

No torch, nothing from the package: this module is pinned by tests/test_pair_layout_reference.py (hand-written answers,
torch's CPU casts, independent spellings of every layout) and judges the kernels BIT FOR BIT in
tests/test_pair_operands_edges_gpu.py.  That is possible because these kernels are integer index arithmetic plus IEEE
fp32 ``+ - *`` and two roundings to bf16 (round to nearest, ties to even), and the library is built with
``-ffp-contract=off``: every function below performs the kernel's fp32 operations in the kernel's order, in ``np.float32``.

PAIR LAYOUT of a row of K fp32 values (K % 32 == 0): K / 32 blocks of 128 bytes, each [hi(32 x bf16) | lo(32 x bf16)],
hi = bf16(x), lo = bf16(x - hi).  As uint16 that is 2 K values per row: value c of a row sits at (c >> 5) * 64 + (c & 31)
(hi) and 32 further (lo).

The last section holds the value generators both test modules share, so the CPU pins (among them: the inputs tell every
listed wrong kernel from the right one) run on exactly what the GPU tests run on.
"""
import numpy as np

F32 = np.float32


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def f32_from_bits(bits):
    return np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32)


# ------------------------------------------------------------------ the two roundings
def bf16_rne_bits(x32):
    """fp32 -> bf16 bit patterns (uint16), round to nearest, ties to even, on the bit pattern: adding 0x7fff plus the lowest
    kept bit carries into the kept half exactly when the dropped half is above a tie, or at a tie with an odd kept half.
    The carry may run through the exponent: the largest finite values round up to infinity, as IEEE asks.  NaN apart: the
    sign and upper payload with the quiet bit set (a carry would turn some NaNs into infinity)."""
    x = _f32(x32)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x)
    r[nan] = ((b[nan] >> 16) | 0x40).astype(np.uint16)
    return r


def bf16_to_f32(bits):
    """bf16 bit patterns -> the fp32 values they stand for (exact)."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_is_nan(bits):
    return (np.asarray(bits) & 0x7FFF) > 0x7F80


def split(x32, rounding=bf16_rne_bits):
    """x -> (hi bits, lo bits): hi = bf16(x), lo = bf16(fp32(x - float(hi))), the subtraction in fp32 as the kernels do
    (``v - __uint_as_float(h << 16)``).  For finite hi the subtraction is exact (test_pair_layout_reference.py)."""
    x = _f32(x32)
    hi = rounding(x)
    with np.errstate(invalid="ignore", over="ignore"):
        rest = x - bf16_to_f32(hi)
    return hi, rounding(rest)


# ------------------------------------------------------------------ the layout
def pair_rows_of(hi, lo):
    """(hi, lo) uint16 [rows, K] -> uint16 [rows, 2K] in the header's block layout."""
    rows, k = hi.shape
    assert k % 32 == 0
    out = np.empty((rows, k // 32, 2, 32), dtype=np.uint16)
    out[:, :, 0, :] = hi.reshape(rows, k // 32, 32)
    out[:, :, 1, :] = lo.reshape(rows, k // 32, 32)
    return out.reshape(rows, 2 * k)


def pair_rows(x32):
    """fp32 [rows, K] -> uint16 [rows, 2K]: what split_pair_kernel writes (as bits)."""
    x = _f32(x32)
    assert x.ndim == 2
    return pair_rows_of(*split(x))


def unpair(p):
    """uint16 [rows, 2K] pair rows -> (hi, lo) uint16 [rows, K] each: the inverse of ``pair_rows_of``."""
    p = np.asarray(p)
    rows, k2 = p.shape
    assert k2 % 64 == 0
    v = p.reshape(rows, k2 // 64, 2, 32)
    return v[:, :, 0, :].reshape(rows, k2 // 2).copy(), v[:, :, 1, :].reshape(rows, k2 // 2).copy()


# ------------------------------------------------------------------ one function per kernel
def gate_split(dy, gate=None, gate_is_pair=False, pooled=None, pool_rows=0, selected=None, group_slot=None, rows=None):
    """gate_split_pair_kernel -> (pair rows uint16 [rows, 2 cols], v fp32 [rows, cols]).

    v = dy, or dy + pooled[r // pool_rows] * fp32(1 / pool_rows) (product first, then the add), or the product alone
    when dy is None; then + selected[slot * pool_rows + r % pool_rows] for the rows of a group with slot =
    group_slot[r // pool_rows] >= 0; then +0 wherever the gate is shut: ``!(y > 0)`` for an fp32 gate [rows, cols], hi half 0
    or >= 0x8000 for a pair gate (uint16 [rows, 2 cols]; only its hi halves are read)."""
    if dy is not None:
        v = _f32(dy).copy()
        rows, cols = v.shape
    else:
        src = pooled if pooled is not None else selected
        cols = src.shape[1]
        if rows is None:
            rows = pooled.shape[0] * pool_rows
        v = np.zeros((rows, cols), dtype=np.float32)
    r = np.arange(rows)
    with np.errstate(invalid="ignore", over="ignore"):
        if pooled is not None:
            scale = F32(1) / F32(pool_rows)
            term = _f32(pooled)[r // pool_rows] * scale
            v = v + term if dy is not None else term
        if selected is not None:
            slot = np.asarray(group_slot, dtype=np.int64)[r // pool_rows]
            on = slot >= 0
            src = _f32(selected)[(slot * pool_rows + r % pool_rows)[on]]
            v[on] = v[on] + src
    if gate is not None:
        if gate_is_pair:
            gh, _ = unpair(gate)
            shut = (gh == 0) | (gh >= 0x8000)
        else:
            with np.errstate(invalid="ignore"):
                shut = ~(_f32(gate) > 0)
        v[shut] = F32(0)
    return pair_rows(v), v


def conv_out_size(size, k, stride, pad):
    return (size + 2 * pad - k) // stride + 1


def im2col_nchw_matrix(x, kh, kw, stride, pad, k_padded=None):
    """fp32 [N, C, H, W] -> fp32 [N * Ho * Wo, k_padded]: row m = (n, oy, ox), k = (ky * KW + kx) * C + c holds
    x[n, c, oy * stride - pad + ky, ox * stride - pad + kx] or +0 outside the image; columns >= KH * KW * C are +0."""
    x = _f32(x)
    n, c, h, w = x.shape
    ho, wo = conv_out_size(h, kh, stride, pad), conv_out_size(w, kw, stride, pad)
    k = kh * kw * c
    kp = -(-k // 32) * 32 if k_padded is None else k_padded
    assert kp % 32 == 0 and kp >= k and ho > 0 and wo > 0
    xp = np.zeros((n, c, h + 2 * pad, w + 2 * pad), dtype=np.float32)
    xp[:, :, pad:pad + h, pad:pad + w] = x
    iy = (np.arange(ho) * stride)[:, None] + np.arange(kh)[None, :]          # [Ho, KH], in the padded image
    ix = (np.arange(wo) * stride)[:, None] + np.arange(kw)[None, :]          # [Wo, KW]
    g = xp[:, :, iy[:, None, :, None], ix[None, :, None, :]]                  # [N, C, Ho, Wo, KH, KW]
    out = np.zeros((n * ho * wo, kp), dtype=np.float32)
    out[:, :k] = g.transpose(0, 2, 3, 4, 5, 1).reshape(n * ho * wo, k)
    return out, (ho, wo)


def im2col_nchw_pair(x, kh, kw, stride, pad, k_padded=None):
    """im2col_nchw_pair_kernel -> (pair rows uint16 [N * Ho * Wo, 2 k_padded], (Ho, Wo))."""
    m, hw = im2col_nchw_matrix(x, kh, kw, stride, pad, k_padded)
    return pair_rows(m), hw


def weight_prep_matrices(w, scale=None):
    """w [N, C, KH, KW] (or [N, C, T]) times scale[N] in fp32 (one product per value; no scale: the value itself) ->
    (forward matrix [N, T * C], k = t * C + c; transposed matrix [C, T * N], k' = t * N + n)."""
    w = _f32(w)
    n, c = w.shape[:2]
    p = w.reshape(n, c, -1)
    if scale is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            p = p * _f32(scale).reshape(n, 1, 1)
    t = p.shape[2]
    return (np.ascontiguousarray(p.transpose(0, 2, 1)).reshape(n, t * c),
            np.ascontiguousarray(p.transpose(1, 2, 0)).reshape(c, t * n))


def weight_prep(w, scale=None, transposed=True):
    """weight_prep_pair_kernel / weight_prep_pair_multi_kernel -> (forward pair rows, transposed pair rows or None)."""
    f, b = weight_prep_matrices(w, scale)
    return pair_rows(f), (pair_rows(b) if transposed else None)


def im2col_pair(xp, num, h, w, kh, kw):
    """im2col_pair_kernel: xp uint16 [num * h * w, 2C] pair rows of an NHWC tensor -> uint16 [num * h * w, kh * kw * 2C]:
    per pixel and tap (ty, tx) the whole pair row of pixel (y + ty - kh // 2, x + tx - kw // 2) of the SAME map, a zero row
    outside it.  Byte copies (the kernel moves 16 bytes at a time): a pair row is moved as it is."""
    xp = np.asarray(xp, dtype=np.uint16)
    c2 = xp.shape[1]
    assert xp.shape[0] == num * h * w
    src = xp.reshape(num, h, w, c2)
    out = np.zeros((num, h, w, kh * kw, c2), dtype=np.uint16)
    for t in range(kh * kw):
        dy, dx = t // kw - kh // 2, t % kw - kw // 2
        y0, y1 = max(0, -dy), min(h, h - dy)
        x0, x1 = max(0, -dx), min(w, w - dx)
        if y0 < y1 and x0 < x1:
            out[:, y0:y1, x0:x1, t] = src[:, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out.reshape(num * h * w, kh * kw * c2)


def slab_sum_tree(slabs):
    """The fixed summation tree of slab_reduce_kernel over axis 0 of fp32 [S, ...]: lane part p of 4 starts at +0 and, for
    s0 = p, p + 32, ..., adds ((v0 + v1) + (v2 + v3)) + ((v4 + v5) + (v6 + v7)) with v_u = slabs[s0 + 4u], +0 past S; the
    four parts are combined as (a0 + a1) + (a2 + a3)."""
    slabs = _f32(slabs)
    s_all = slabs.shape[0]
    zero = np.zeros(slabs.shape[1:], dtype=np.float32)
    parts = []
    for p in range(4):
        a = zero.copy()
        for s0 in range(p, s_all, 32):
            v = [slabs[s0 + 4 * u] if s0 + 4 * u < s_all else zero for u in range(8)]
            a = a + (((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])))
        parts.append(a)
    return (parts[0] + parts[1]) + (parts[2] + parts[3])


def slab_reduce(slabs, scale, n, c, t, total=slab_sum_tree):
    """slab_reduce_kernel: slabs fp32 [S, N, T * C] (tap-major: k = t * C + c) -> dweight fp32 [N, C, T] =
    tree sum over S, times scale[n] (no scale: times 1)."""
    slabs = _f32(slabs).reshape(-1, n, t * c)
    tot = total(slabs)
    if scale is not None:
        tot = tot * _f32(scale).reshape(n, 1)
    return np.ascontiguousarray(tot.reshape(n, t, c).transpose(0, 2, 1))


def slab_reduce_bound(slabs, scale, n, c, t):
    """(fp64 value of scale[n] * sum_s slabs, its worst-case fp32 error bound) in [N, C, T] order: S - 1 additions and one
    product, each within 2^-24 relative, in ANY order: |err| <= ((1 + 2^-24)^S - 1) |scale| sum|slab| <=
    (S + 1) 2^-24 |scale| sum|slab| for every S this library produces (S <= 256)."""
    s64 = np.asarray(slabs, dtype=np.float64).reshape(-1, n, t * c)
    sc = np.ones((n, 1)) if scale is None else np.asarray(scale, dtype=np.float64).reshape(n, 1)
    val = s64.sum(0) * sc
    bound = (s64.shape[0] + 1) * 2.0 ** -24 * np.abs(sc) * np.abs(s64).sum(0)

    def nct(a):
        return np.ascontiguousarray(a.reshape(n, t, c).transpose(0, 2, 1))

    return nct(val), nct(bound)


# ------------------------------------------------------------------ the inputs both test modules share
# fp32 bit patterns a subtly wrong rounding, or a build that flushes subnormals, treats differently
PLANTED_BITS = np.array([
    0x3F808000, 0xBF808000,      # exact ties, even kept half: stay (a tie away from zero would not)
    0x3F818000, 0xBF818000,      # exact ties, odd kept half: round up in magnitude
    0x3F807FFF, 0x3F808001,      # one ulp below / above a tie
    0x40490FDB, 0xC0490FDB,      # +-pi: rounds up, a truncation would not
    0x00000000, 0x80000000,      # +-0
    0x00800000, 0x80800000,      # the smallest normals
    0x007FFFFF,                  # the largest subnormal: hi is the smallest normal, lo = -0
    0x00018000, 0x00012345,      # subnormals above 2^-133 (the smallest bf16 subnormal, 0x00010000)
    0x00010000,
    0x00008001,                  # below 2^-133, above half of it: rounds up to 2^-133
    0x00008000,                  # 2^-134: a tie between 0 and 2^-133, goes to 0
    0x00007FFF, 0x00000001,      # below 2^-134: hi = 0 and lo = 0
    0x7F7F7FFF, 0xFF7F7FFF,      # the largest values that stay finite in bf16
    0x7F7F8000, 0xFF7F8000,      # the next ones up: hi = +-inf, lo = -+inf
    0x7F800000, 0xFF800000,      # +-inf: lo = NaN
    0x7FC00000,                  # a NaN
], dtype=np.uint32)


def edge_values(rows, cols, seed, special=True):
    """fp32 [rows, cols]: random normals over a wide log range (2^-30 .. 2^30, both signs, full mantissas) with the PLANTED
    values scattered in: every third element along each row, the rows shifted against each other, takes the next planted value.
    From three rows on, every one of the 32 column positions of a block and both 16-byte halves of a thread's 8 values hold
    planted values (test_pair_layout_reference.py asserts it).  ``special=False`` leaves inf and NaN out (operands whose sums
    must stay comparable)."""
    rng = np.random.default_rng(seed)
    mant = rng.standard_normal((rows, cols))
    expo = rng.uniform(-30.0, 30.0, size=(rows, cols))
    x = (mant * np.exp2(expo)).astype(np.float32)
    planted = PLANTED_BITS if special else PLANTED_BITS[(PLANTED_BITS & 0x7F800000) != 0x7F800000]
    r, c = np.divmod(np.arange(rows * cols), cols)
    where = np.flatnonzero((r + c) % 3 == 0)
    flat = x.reshape(-1)
    flat[where] = f32_from_bits(planted[np.arange(where.size) % planted.size])
    return flat.reshape(rows, cols)


def planted_mask(rows, cols):
    r, c = np.divmod(np.arange(rows * cols), cols)
    return ((r + c) % 3 == 0).reshape(rows, cols)


GATE_BITS = np.array([
    0x00000000, 0x80000000,      # +0, -0: shut
    0xBF800000, 0x80000001,      # negative normal, negative subnormal: shut
    0x00800000,                  # the smallest normal: open in both gate forms
    0x00400000, 0x00010000,      # subnormals whose hi half is not 0: open in both forms
    0x00008001,                  # rounds up to 2^-133: open in both forms
    0x00008000, 0x00000001,      # 0 < y <= 2^-134: hi = 0, the pair gate is shut, the fp32 gate open
    0x7F800000,                  # +inf: open
    0x3F800000, 0x7F7F8000,      # 1; a value whose hi half is +inf: open
], dtype=np.uint32)


def gate_values(rows, cols, seed):
    """fp32 [rows, cols] forward outputs y of a ReLU layer for the gate: half of them random (positive normals and exact
    zeros, as a ReLU leaves them), the other half (a checkerboard, so that both bf16 halves of a 32-bit word of the pair
    gate meet them) the GATE_BITS in turn."""
    rng = np.random.default_rng(seed)
    y = np.maximum(rng.standard_normal((rows, cols)), 0.0).astype(np.float32)
    flat = y.reshape(-1)
    r, c = np.divmod(np.arange(rows * cols), cols)
    where = np.flatnonzero((r + c) % 2 == 0)
    flat[where] = f32_from_bits(GATE_BITS[np.arange(where.size) % GATE_BITS.size])
    return flat.reshape(rows, cols)


def slab_values(s, n, k, seed):
    """fp32 [S, N, K] slabs whose sum depends on the order of the additions: magnitudes over 2^-8 .. 2^8, both signs."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((s, n, k)) * np.exp2(rng.uniform(-8.0, 8.0, size=(s, n, k)))).astype(np.float32)
