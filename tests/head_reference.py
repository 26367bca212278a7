"""TEST INFRASTRUCTURE ONLY -- NumPy float64 restatements of what the cross-modal head's kernels compute, written from the
formulas: the strided fp32 GEMM with its epilogue (csrc/gemm_f32.hip), the region<->noun alignment (same file), the
background-weighted cross entropy and the stochastic-logit mask BCE (csrc/losses.hip).

No torch and nothing from the package: this module exists to be pinned (tests/test_head_reference.py, against torch float64
matmul / autograd) and then to judge the HIP kernels at their edges (tests/test_head_kernels_edges_gpu.py).  Inputs are the
float32 arrays the kernels receive; everything is computed from them in float64.

The last sections hold the case builders both test modules share: every case is a named tuple whose first field is its
readable id, and ``*_data(case)`` makes its arrays from the case's own seed, so the CPU pins run on exactly what the GPU tests
run on.
"""
import itertools
from collections import namedtuple

import numpy as np


def _f64(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.astype(np.float64)


# ------------------------------------------------------------------ the operations, float64
def gemm(A, B, bias=None, bias_per_row=False, alpha=1.0, C_in=None):
    """C[m, n] = alpha * sum_k A[m, k] B[n, k] (+ C_in[m, n]) + bias[n] (bias[m] with ``bias_per_row``) and the magnitude
    |alpha| * sum_k |A||B| + |bias| + |C_in| that a float32 evaluation's round-off is proportional to.  K = 0 is the empty
    sum.  -> (C fp64 [M, N], magnitude fp64 [M, N])."""
    a, b = _f64(A), _f64(B)
    alpha = float(np.float32(alpha))
    out = alpha * (a @ b.T)
    mag = abs(alpha) * (np.abs(a) @ np.abs(b).T)
    if C_in is not None:
        c = _f64(C_in)
        out, mag = out + c, mag + np.abs(c)
    if bias is not None:
        v = _f64(bias)
        v = v[:, None] if bias_per_row else v[None, :]
        out, mag = out + v, mag + np.abs(v)
    return out, mag


def region_noun_scores(emb, nouns):
    """scores[p, w] = <emb[p], nouns[w]> and sum_d |emb[p, d]| |nouns[w, d]|, fp64.  One noun at a time with a row-wise
    sum, so that two identical embedding rows get bit-identical scores (a BLAS product makes no such promise)."""
    e, n = _f64(emb), _f64(nouns)
    s = np.stack([(e * n[w]).sum(axis=1) for w in range(n.shape[0])], axis=1) if n.shape[0] else np.zeros((e.shape[0], 0))
    mag = np.stack([(np.abs(e) * np.abs(n[w])).sum(axis=1) for w in range(n.shape[0])], axis=1) if n.shape[0] else s.copy()
    return s, mag


def sigmoid(x):
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def region_noun(emb, nouns):
    """Per noun w: the maximum over the regions p of <emb[p], nouns[w]>, its sigmoid, the LOWEST p that attains it, and
    the gap between the maximum and the best score of any OTHER region (0 for an exact tie, inf for one region) -- a
    case proves with it that it is tie-free or an exact tie.  -> (raw [W], sigmoid [W], index int64 [W], gap [W])."""
    s, _ = region_noun_scores(emb, nouns)
    p, w = s.shape
    idx = s.argmax(axis=0).astype(np.int64)  # the first maximum
    raw = s[idx, np.arange(w)]
    rest = s.copy()
    rest[idx, np.arange(w)] = -np.inf
    gap = raw - rest.max(axis=0) if p > 1 else np.full(w, np.inf)
    return raw, sigmoid(raw), idx, gap


def weighted_ce(logits, labels, bg_weight):
    """loss = sum_p w[label_p] * (logsumexp(x_p) - x_p[label_p]) / P with w[0] = bg_weight, w[c > 0] = 1, and its gradient
    with respect to the logits; a stable fp64 log-sum-exp (the row maximum is taken out first).

    A row whose label lies outside [0, C) contributes 0 and gets a zero gradient row but is still counted in P: that is
    what the kernel implements.  Its host twin ``_cpu.weighted_ce_fwd_bwd`` raises on such labels (it indexes the weight
    vector with them); the two differ there on purpose and neither is to be changed.
    -> (loss, d loss / d logits fp64 [P, C])."""
    x = _f64(logits)
    lab = np.asarray(labels, dtype=np.int64)
    p, c = x.shape
    bg = float(np.float32(bg_weight))
    valid = (lab >= 0) & (lab < c)
    safe = np.where(valid, lab, 0)
    w = np.where(valid, np.where(lab == 0, bg, 1.0), 0.0)
    m = x.max(axis=1)
    with np.errstate(divide="ignore"):
        lse = m + np.log(np.exp(x - m[:, None]).sum(axis=1))
    rows = np.arange(p)
    terms = np.where(valid, w * (lse - x[rows, safe]), 0.0)
    grad = np.exp(x - lse[:, None])
    grad[rows, safe] -= 1.0
    grad *= (w / p)[:, None]
    grad[~valid] = 0.0
    return float(terms.sum() / p), grad


def clamp_channels(channel, num_pos, num_channels):
    """The logit channel of every positive: one int for all, or one per positive clamped into [0, C - 1]."""
    if np.ndim(channel) == 0:
        assert 0 <= int(channel) < num_channels
        return np.full(num_pos, int(channel), dtype=np.int64)
    ch = np.asarray(channel, dtype=np.int64)
    assert ch.shape == (num_pos,)
    return np.clip(ch, 0, num_channels - 1)


def mask_bce(mu, sigma, eps, pos_index, channel, targets):
    """z = mu + eps * sigma on the selected (positive, channel) planes -- z = mu when EITHER factor is missing -- and
    loss = mean over npos * MM of max(z, 0) - z t + log1p(exp(-|z|)).  mu [P, C, ...] (MM = what follows), sigma
    [P, 1, ...] or None, eps like mu or None, pos_index [npos], channel an int or [npos] (clamped into [0, C - 1], as the
    kernel documents), targets [npos, ...].  npos = 0 gives loss 0.
    -> (loss, dmu fp64 shaped like mu, dsigma fp64 shaped like sigma or None): zero outside the selected planes; dsigma is
    all zero when eps is missing."""
    m = _f64(mu)
    shape = m.shape
    p, c = shape[:2]
    m = m.reshape(p, c, -1)
    mm = m.shape[2]
    pos = np.asarray(pos_index, dtype=np.int64)
    npos = pos.size
    dmu = np.zeros_like(m)
    dsigma = None if sigma is None else np.zeros((p, 1, mm))
    loss = 0.0
    if npos:
        ch = clamp_channels(channel, npos, c)
        z = m[pos, ch]
        noise = None
        if sigma is not None and eps is not None:
            noise = _f64(eps).reshape(p, c, mm)[pos, ch]
            z = z + noise * _f64(sigma).reshape(p, mm)[pos]
        t = _f64(targets).reshape(npos, mm)
        n = float(npos) * float(mm)
        loss = float((np.maximum(z, 0.0) - z * t + np.log1p(np.exp(-np.abs(z)))).sum() / n)
        g = (sigmoid(z) - t) / n
        dmu[pos, ch] = g
        if noise is not None:
            dsigma[pos, 0] = g * noise
    return loss, dmu.reshape(shape), (None if dsigma is None else dsigma.reshape(np.asarray(sigma).shape))


def selected_planes(shape, pos_index, channel):
    """bool [P, C]: the (positive, clamped channel) planes that may receive a gradient."""
    p, c = shape[:2]
    sel = np.zeros((p, c), dtype=bool)
    pos = np.asarray(pos_index, dtype=np.int64)
    if pos.size:
        sel[pos, clamp_channels(channel, pos.size, c)] = True
    return sel


# ------------------------------------------------------------------ GEMM cases
# How a logical operand X [rows, K] lies in memory.  The library picks an operand's load mode from (k stride, row stride,
# base alignment): "kc" and "rc" are the two float4 modes, the three "g_*" must all fall back to the element-wise mode.
LAYOUTS = ("kc", "rc", "g_2d", "g_rs2", "g_off1")
PAD = np.float32(1e30)  # what surrounds an operand inside its allocation: one stray read of it wrecks the result


def lay_out(X, layout):
    """-> (flat float32 buffer, offset, row_stride, k_stride) with X[r, k] == buffer[offset + r * row_stride + k * k_stride]
    and every other element PAD.
      kc      k contiguous, row stride a multiple of 4 (> K: a view), base 16-byte aligned
      rc      rows contiguous, k stride a multiple of 4 (> rows), base aligned
      g_2d    both strides > 1 (k stride 2, odd row stride)
      g_rs2   k contiguous with a row stride = 2 mod 4: rows are not 16-byte aligned
      g_off1  the kc layout started one element into the allocation: base not 16-byte aligned"""
    X = np.asarray(X, dtype=np.float32)
    rows, k = X.shape
    k4, r4 = -(-max(k, 1) // 4) * 4, -(-max(rows, 1) // 4) * 4
    off = 0
    if layout == "kc":
        rs, ks = k4 + 4, 1
    elif layout == "rc":
        rs, ks = 1, r4 + 4
    elif layout == "g_2d":
        rs, ks = 2 * k + 3, 2
    elif layout == "g_rs2":
        rs, ks = k4 + 2, 1
    elif layout == "g_off1":
        rs, ks, off = k4 + 4, 1, 1
    else:
        raise ValueError(layout)
    last = off + max(rows - 1, 0) * rs + max(k - 1, 0) * ks
    buf = np.full(last + 1 + 3, PAD, dtype=np.float32)
    if rows and k:
        buf[off + np.arange(rows)[:, None] * rs + np.arange(k)[None, :] * ks] = X
    return buf, off, rs, ks


GemmCase = namedtuple("GemmCase", "name m n k a_layout b_layout bias alpha accumulate seed")
C_EXTRA = 5  # c_row_stride = N + 5: the result goes into the left N columns of a wider matrix
GEMM_SHAPES = ((64, 64, 16),      # one full tile, one k-step
               (65, 63, 17),      # ragged in every dimension
               (128, 192, 40),    # full tiles, ragged last k-step: the load mode changes inside the k loop
               (64, 64, 256),     # the smallest shape that is cut along K
               (70, 130, 1000),   # split-K with ragged tiles, a ragged final step and a short last slice
               (1, 1, 1))
GEMM_SPLIT_SHAPES = ((64, 64, 256), (70, 130, 1000))  # asserted through the library's own workspace query on the GPU
EPILOGUES = tuple(itertools.product(("none", "col", "row"), (1.0, -0.5), (0, 1)))  # (bias, alpha, accumulate)


def _gemm_name(m, n, k, la, lb, bias, alpha, acc):
    return f"{m}x{n}x{k}-A:{la}-B:{lb}-bias:{bias}-alpha{alpha:g}-acc{acc}"


def gemm_cases():
    """Every shape x all 5 x 5 operand layouts (the 3 x 3 load-mode combinations with the generic mode built three ways),
    the twelve epilogues dealt round-robin over them; then EVERY epilogue on the ragged shape and the two split-K shapes
    (split-K + accumulate + row bias among them) over rotating layouts; then K = 0 with every epilogue."""
    cases, i = [], 0
    for (m, n, k) in GEMM_SHAPES:
        for la, lb in itertools.product(LAYOUTS, repeat=2):
            bias, alpha, acc = EPILOGUES[i % len(EPILOGUES)]
            cases.append(GemmCase(_gemm_name(m, n, k, la, lb, bias, alpha, acc), m, n, k, la, lb, bias, alpha, acc, 100 + i))
            i += 1
    for (m, n, k) in ((65, 63, 17),) + GEMM_SPLIT_SHAPES:
        for j, (bias, alpha, acc) in enumerate(EPILOGUES):
            la, lb = LAYOUTS[j % 5], LAYOUTS[(j // 5 + 2 * j + 1) % 5]
            name = _gemm_name(m, n, k, la, lb, bias, alpha, acc)
            if all(c.name != name for c in cases):
                cases.append(GemmCase(name, m, n, k, la, lb, bias, alpha, acc, 100 + i))
            i += 1
    for j, (bias, alpha, acc) in enumerate(EPILOGUES):
        cases.append(GemmCase(_gemm_name(5, 7, 0, "kc", "g_2d", bias, alpha, acc), 5, 7, 0, "kc", "g_2d", bias, alpha, acc, 900 + j))
    return cases


def gemm_data(case):
    """-> (A [M, K], B [N, K], bias [N] / [M] / None, C0 [M, N + C_EXTRA]) float32: C0 is what the output matrix holds
    before the call -- random everywhere, so an overwrite ignores it, an accumulate adds its left N columns and the right
    C_EXTRA columns must come back bit-unchanged."""
    rng = np.random.default_rng(case.seed)
    a = rng.standard_normal((case.m, case.k)).astype(np.float32)
    b = rng.standard_normal((case.n, case.k)).astype(np.float32)
    bias = {"none": None, "col": rng.standard_normal(case.n).astype(np.float32),
            "row": rng.standard_normal(case.m).astype(np.float32)}[case.bias]
    c0 = (rng.standard_normal((case.m, case.n + C_EXTRA)) * 3).astype(np.float32)
    return a, b, bias, c0


def gemm_expected(case, a, b, bias, c0):
    return gemm(a, b, bias, case.bias == "row", case.alpha, c0[:, :case.n] if case.accumulate else None)


# ------------------------------------------------------------------ region<->noun cases
RegionCase = namedtuple("RegionCase", "name p d kind seed tie")
REGION_P = (1, 3, 63, 64, 65, 130)       # below four waves' worth, one region short of / exactly / one past a chunk, three chunks
REGION_D = (8, 260, 768, 7, 50)          # float4 path: 2 busy lanes, a partial second trip, three full trips; scalar path: 7, 50
REGION_W = (1, 9, 65)                    # 65 needs the second finalize block; a case's nouns are the first W of its 65
REGION_KINDS = ("random", "negative", "mixed")
REGION_TIES = ((1, 2), (1, 5), (5, 70))  # different waves of one chunk | one wave | different chunks
# A "tie-free" case has gap >= MIN_GAP_FACTOR * max_p sum_d |emb||noun| for every noun: twice the bound the kernel's
# scores are held to, so ANY scores inside that bound pick the same region and the indices can be compared exactly.
SCORE_BOUND = 2e-6
MIN_GAP_FACTOR = 2 * SCORE_BOUND


def region_cases():
    cases = [RegionCase(f"P{p}-D{d}-{kind}", p, d, kind, 7000 + 97 * i, None)
             for i, (p, d, kind) in enumerate(itertools.product(REGION_P, REGION_D, REGION_KINDS))]
    for i, ((r0, r1), d, kind) in enumerate(itertools.product(REGION_TIES, (260, 50), ("tie-positive", "tie-negative"))):
        cases.append(RegionCase(f"P130-D{d}-{kind}-rows{r0}and{r1}", 130, d, kind, 9000 + i, (r0, r1)))
    return cases


def _region_draw(case, seed):
    rng = np.random.default_rng(seed)
    p, d, w = case.p, case.d, max(REGION_W)
    emb = rng.standard_normal((p, d)).astype(np.float32)
    nouns = rng.standard_normal((w, d)).astype(np.float32)
    if case.kind == "random":                      # scores of order 1, both signs
        nouns /= np.linalg.norm(nouns, axis=1, keepdims=True)
    elif case.kind == "negative":                  # every score negative
        emb, nouns = -np.abs(emb), np.abs(nouns)
    elif case.kind == "mixed":                     # even nouns: every region scores negative; odd nouns: positive maxima
        emb[:, 0] = 4 + np.abs(emb[:, 0])
        nouns[0::2, 0] = -2 * np.sqrt(d)
        nouns[1::2, 0] = 2 * np.sqrt(d)
    elif case.kind == "tie-positive":              # the duplicated row scores far above the small rest
        emb, nouns = emb * np.float32(0.05), np.abs(nouns)
        emb[case.tie[0]] = np.abs(rng.standard_normal(d)).astype(np.float32)
    elif case.kind == "tie-negative":              # every score negative, the duplicated row the closest to zero
        emb, nouns = -np.abs(emb) - np.float32(1), np.abs(nouns)
        emb[case.tie[0]] = -np.abs(rng.standard_normal(d)).astype(np.float32) * np.float32(0.01)
    else:
        raise ValueError(case.kind)
    if case.tie:
        emb[case.tie[1]] = emb[case.tie[0]]
    return np.ascontiguousarray(emb, dtype=np.float32), np.ascontiguousarray(nouns, dtype=np.float32)


def region_min_gap(emb, nouns):
    return MIN_GAP_FACTOR * region_noun_scores(emb, nouns)[1].max(axis=0)


def region_data(case):
    """-> (emb [P, D], nouns [65, D]) float32.  A draw whose runner-up (for a tie case: whose third) comes closer than
    the stated minimum gap is drawn again from the next seed, so the precondition the CPU test asserts is the builder's
    doing and not luck."""
    for attempt in range(50):
        emb, nouns = _region_draw(case, case.seed + 13 * attempt)
        probe = np.delete(emb, case.tie[1], axis=0) if case.tie else emb
        if bool((region_noun(probe, nouns)[3] >= region_min_gap(emb, nouns)).all()):
            return emb, nouns
    raise AssertionError(f"{case.name}: no tie-free draw")


# ------------------------------------------------------------------ weighted cross entropy cases
CeCase = namedtuple("CeCase", "name p c labels logits bg_weight seed")
CE_SHAPES = ((5, 1), (4, 63), (7, 64), (9, 65), (1030, 130))   # C around the 64-lane stride; P % 4 = 1, 0, 3, 1, 2; P > 1024
# planted rows: (name, needs a second class)
CE_PLANTS = (("const", False), ("big-off-label", True), ("big-at-label", False), ("small-at-label", False),
             ("small-off-label", True), ("x30", False), ("neginf-off-label", True))


def ce_cases():
    cases = []
    for i, (p, c) in enumerate(CE_SHAPES):
        s = 300 + 20 * i
        cases.append(CeCase(f"P{p}-C{c}-base-bg0.2", p, c, "random", "randn3", 0.2, s))
        cases.append(CeCase(f"P{p}-C{c}-base-bg0", p, c, "random", "randn3", 0.0, s + 1))
        cases.append(CeCase(f"P{p}-C{c}-base-bg1", p, c, "random", "randn3", 1.0, s + 2))
        cases.append(CeCase(f"P{p}-C{c}-all-background-bg0.2", p, c, "background", "randn3", 0.2, s + 3))
        cases.append(CeCase(f"P{p}-C{c}-all-background-bg0", p, c, "background", "randn3", 0.0, s + 4))
        cases.append(CeCase(f"P{p}-C{c}-ignored-labels", p, c, "ignored", "randn3", 0.2, s + 5))
        plants = [name for name, two in CE_PLANTS if c > 1 or not two]
        for j in range(0, len(plants), p):       # as many planted rows per case as the case has rows
            chunk = tuple(plants[j:j + p])
            cases.append(CeCase(f"P{p}-C{c}-extreme-{'+'.join(chunk)}", p, c, "random", chunk, (0.2, 1.0)[(j // p) % 2], s + 6 + j))
    return cases


def ce_data(case):
    """-> (logits float32 [P, C], labels int64 [P]).  "random" labels contain 0 and C - 1; "ignored" mixes -1, C and -100
    in; planted rows replace rows 0, 1, ... of ``randn * 3`` and get a label that is neither 0 (unless C = 1) so that the
    background weight cannot hide them."""
    rng = np.random.default_rng(case.seed)
    p, c = case.p, case.c
    x = (rng.standard_normal((p, c)) * 3).astype(np.float32)
    if case.labels == "background":
        lab = np.zeros(p, dtype=np.int64)
    else:
        lab = rng.integers(0, c, size=p).astype(np.int64)
        lab[0], lab[-1] = c - 1, 0
        if p > 2:
            lab[1::3] = 0
        if case.labels == "ignored":              # rows 1, 2, 3 and every seventh after them; row 0 stays valid
            bad = (-1, c, -100)
            for j, r in enumerate(list(range(1, min(p, 4))) + list(range(5, p - 1, 7))):
                lab[r] = bad[j % 3]
    if case.logits != "randn3":
        for r, plant in enumerate(case.logits):
            l = c - 1 if c > 1 else 0
            off = 0 if c > 1 else None            # a column that is not the label
            lab[r] = l
            if plant == "const":
                x[r] = np.float32(2.5)
            elif plant == "big-off-label":
                x[r, off] = 1e4
            elif plant == "big-at-label":
                x[r, l] = 1e4
            elif plant == "small-at-label":
                x[r, l] = -1e4
            elif plant == "small-off-label":
                x[r, off] = -1e4
            elif plant == "x30":
                x[r] *= np.float32(30)
            elif plant == "neginf-off-label":
                x[r, off] = -np.inf
            else:
                raise ValueError(plant)
    return x, lab


# ------------------------------------------------------------------ mask BCE cases
MaskCase = namedtuple("MaskCase", "name p c shape npos channel noise extreme raw seed")
MASK_SHAPES = ((3, 1, 1), (6, 2, 14), (5, 5, 16), (4, 2, 28))  # MM = 1, 196, 256 (exactly one trip of the 256 lanes), 784
MASK_FLAT_MM = (63, 255, 257)                                  # M x 1 maps around the wave and the 256-lane loop boundary
MASK_NOISE = ("both", "neither", "sigma-only", "eps-only")
MASK_EXTREME_MU = np.array([100, 100, -100, -100, 1e4, 1e4, -1e4, -1e4], dtype=np.float32)
MASK_EXTREME_T = np.array([0, 1, 0, 1, 0, 1, 0, 1], dtype=np.float32)


def _mask_case(p, c, shape, npos, channel, noise, extreme, raw, seed):
    dims = "x".join(str(s) for s in shape)
    name = f"P{p}-C{c}-{dims}-npos{npos}-ch:{channel}-{noise}" + ("-extreme" if extreme else "") + ("-raw" if raw else "")
    return MaskCase(name, p, c, shape, npos, channel, noise, extreme, raw, seed)


def mask_cases():
    cases, s = [], 500
    for (p, c, m) in MASK_SHAPES:
        for npos, channel, noise in ((p, "per", "both"), (p, "last", "neither"), (1, "first", "sigma-only"),
                                     (max(p - 1, 1), "per", "eps-only"), (0, "last", "both"), (p, "first", "both")):
            cases.append(_mask_case(p, c, (m, m), npos, channel, noise, False, False, s))
            s += 1
    for (p, c, m), channel, noise in (((6, 2, 14), "per", "both"), ((6, 2, 14), "last", "neither"),
                                      ((4, 2, 28), "first", "sigma-only"), ((4, 2, 28), "per", "eps-only")):
        cases.append(_mask_case(p, c, (m, m), p, channel, noise, True, False, s))
        s += 1
    for channel, noise in (("per", "both"), ("first", "neither")):           # npos > 1024: sum_kernel's second trip
        cases.append(_mask_case(1035, 2, (1, 1), 1030, channel, noise, False, False, s))
        s += 1
    for mm in MASK_FLAT_MM:
        for channel, noise in (("per", "both"), ("last", "neither")):
            cases.append(_mask_case(5, 3, (mm, 1), 4, channel, noise, False, True, s))
            s += 1
    return cases


def mask_data(case):
    """-> dict(mu [P, C, *shape], sigma [P, 1, *shape] or None, eps like mu or None, pos int64 [npos] (unique, unsorted),
    channel (int, or int64 [npos] with -1 first and C last), targets [npos, *shape] of 0 / 1).  An extreme case plants
    mu = +-100, +-1e4 against both target values at the first eight pixels of the first positive's plane."""
    rng = np.random.default_rng(case.seed)
    p, c, npos = case.p, case.c, case.npos
    mu = (rng.standard_normal((p, c) + case.shape) * 2).astype(np.float32)
    sigma = (rng.uniform(size=(p, 1) + case.shape) + 0.3).astype(np.float32)
    eps = rng.standard_normal((p, c) + case.shape).astype(np.float32)
    pos = rng.permutation(p)[:npos].astype(np.int64)
    if npos > 2 and bool((np.diff(pos) > 0).all()):
        pos = pos[::-1].copy()
    targets = (rng.uniform(size=(npos,) + case.shape) > 0.5).astype(np.float32)
    if case.channel == "per":
        channel = rng.integers(0, c, size=npos).astype(np.int64)
        if npos:
            channel[0] = -1
            channel[-1] = c
    else:
        channel = 0 if case.channel == "first" else c - 1
    if case.extreme:
        ch0 = int(clamp_channels(channel, npos, c)[0])
        mu.reshape(p, c, -1)[pos[0], ch0, :8] = MASK_EXTREME_MU
        targets.reshape(npos, -1)[0, :8] = MASK_EXTREME_T
    return dict(mu=mu, sigma=sigma if case.noise in ("both", "sigma-only") else None,
                eps=eps if case.noise in ("both", "eps-only") else None, pos=pos, channel=channel, targets=targets)
