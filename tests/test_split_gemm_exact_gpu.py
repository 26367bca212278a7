"""GPU: COMPLETENESS of the split GEMM family (csrc/split_gemm.hip) -- every row, every tap and all three hi/lo terms
multiplied exactly once -- pinned with operands whose three-term product is exactly representable in fp32
(tests/exact_product_reference.py: grid values a + b 2^-9, budget S < 2^15, integers S < 2^24).  The kernels then have to
return THE value, whatever their slice plan, tile order or LDS staging: every comparison below is ``torch.equal``.  A
missing, doubled or wrapped row changes an entry by >= 1, a missing hi.lo / lo.hi term by >= 2^-9; the fp64 bound of the
other split GEMM modules (2e-5 sum |a||b|) states precision on realistic data and sees neither at large M or K.

The expected value is always ``three_term`` (hi.hi + hi.lo + lo.hi in fp64, representable in fp32 -- asserted on the inputs
before any device value is looked at) of plainly indexed operands (``tap_rows``: index loops, no ``F.unfold``); the pair
operands are written bit by bit on the host.  Slice counts are READ from the library; nothing here restates how rows or
k-steps are cut.  Every test but the C-boundary ones fails by name on ``test_premise_exact_accumulation`` when the premise
(bf16 MFMA with fp32 accumulation and the fp32 slab sums are exact when every partial sum is representable) does not hold.

Sections, with the launches compared in a run on an MI355X -- ALL EXACT, no kernel missed an equality, nothing was fixed
in the kernels (measured, not supposed: every count below is a launch whose result was compared with ``torch.equal``):
  3.0 premise                          4 launches: 128 x 32 x 128, config 8, integers and lo-bearing operands, forward and
                                       transpose-read (one slice).  Holds.
  3.1 weight gradient, general, 1x1  141 launches: M in {1, 31, 32, 33, 95, 1000, 4129, 7999} lo-bearing and 40001 integers;
                                       (n, ch) in {(128,128), (256,128), (128,384)} (both tile-major orders); slices 1, 2, 3,
                                       7, the library's (1 .. 156) and steps + 2; column slices of wider pair tensors.
                                       ``ovis_split_gemm_pair_tn`` SERVES a count above the number of 32-row steps
                                       (OVIS_OK): the empty slices leave exact zeros (up to 1253 slices on 1251 steps).
  3.2 weight gradient, general, taps  67 launches: nine (h, w, kh, kw) among them W > 32, H = 1, W = 1 and the
                                       32 / W + 1 > H maps; r in {1, 3, one with M > 2100}; 50 x 84 with integers
  3.3 weight gradient, in-map rows    30 launches: seven shapes (3 x 3 and 5 x 5), slices 1, 2, 5, 13, the library's
  3.4 fused slab reduce                4 launches: one case of 3.1, one of 3.3, scale 2^k per channel
  3.5 forward                        398 launches: PLAIN 70 (ten shapes x seven configs), a2_pair 7, SHIFTED 198 and HALO 54
                                       (nine map geometries x {3x3, 3x5} x flip x seven configs), narrow 10, epilogues 54
                                       (bias, fp32 residual contiguous / row-strided, pair residual, relu, gate, pair
                                       residual + gate, un-sliced and through the finish kernel), gated 3x3 3, pooled 2
  3.6 coverage guard                   queries only
  4   C boundary                      65 refused calls: T > 1 with m % (height * width) != 0 -> OVIS_EINVAL, nothing launched
"""
import functools

import numpy as np
import pytest
import torch

from tests import exact_product_reference as E

pytestmark = pytest.mark.gpu

CO = 0x10000
OVIS_OK, OVIS_EINVAL = 0, -1
PREMISE = "test_premise_exact_accumulation"


def _C():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C as c
    return c


# ---------------------------------------------------------------------------------------------------------------------
# operands: host grid values + their pair rows on the device (written on the host, bit by bit)
# ---------------------------------------------------------------------------------------------------------------------
def _to_dev_pair(x):
    return torch.from_numpy(E.pair_bits(x).view(np.int16)).cuda().view(torch.bfloat16)


@functools.lru_cache(maxsize=None)
def _operand(rows, cols, lo, seed):
    """(host fp32 grid values, device pair rows) -- drawn once, shared, never written."""
    x = E.grid(rows, cols, lo, seed)
    x.setflags(write=False)
    return x, _to_dev_pair(x)


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def slices(m, n, ch, ch2, kh, kw, w, cfg):
    """The number of K slices the library's plan gives a forward launch (1: un-sliced)."""
    nbytes = int(_C()._L.ovis_split_gemm_pair_workspace_bytes_ex(m, n, ch, ch2, kh, kw, w, cfg))
    return nbytes // (4 * m * n) if nbytes else 1


def k_units(m, n, ch, kh, kw, w, cfg):
    """What the plan counts a K slice in, read from the query: a forced count of 255 is clamped to the number of units --
    channel blocks (ch / 32) on the HALO form, taps x channel blocks on the SHIFTED one."""
    return slices(m, n, ch, 0, kh, kw, w, (255 << 8) | cfg)


def _tn(gp, xp, count, m, n, ch, kh=1, kw=1, h=0, w=0):
    """ovis_split_gemm_pair_tn with ``count`` slices on NaN-filled slabs -> (status, slabs)."""
    C = _C()
    slabs = torch.full((count, n, kh * kw * ch), float("nan"), device="cuda")
    rc = C._L.ovis_split_gemm_pair_tn(gp.data_ptr(), 2 * gp.stride(0), xp.data_ptr(), 2 * xp.stride(0), slabs.data_ptr(),
                                      count, m, n, ch, kh, kw, h, w, C._stream())
    torch.cuda.synchronize()
    return rc, slabs


def _check_tn(gp, xp, counts, m, n, ch, want, geom=(1, 1, 0, 0), label=""):
    """Every slice count: OVIS_OK, no slab entry left unwritten, the sum of the slabs == want bit for bit, and at least
    count - ceil(m / 32) slabs exactly zero (a count above the number of 32-row steps leaves empty slices)."""
    kh, kw, h, w = geom
    want_t = _dev(want)
    steps = -(-m // 32)
    for count in counts:
        rc, slabs = _tn(gp, xp, count, m, n, ch, kh, kw, h, w)
        assert rc == OVIS_OK, (label, count, rc)
        assert not torch.isnan(slabs).any(), (label, count, "a slab entry was never written")
        got = slabs.sum(0)
        if not torch.equal(got, want_t):
            d = (got.double() - want_t.double()).abs()
            bad = d.nonzero()
            raise AssertionError(f"{label} slices={count}: {bad.shape[0]} of {d.numel()} entries differ, largest by "
                                 f"{d.max().item() / E.LO_UNIT:.1f} x 2^-9; first at (n, k) = {bad[0].tolist()}, "
                                 f"columns (tap*ch + c) touched: {sorted(set((bad[:, 1] // ch).tolist()))[:12]} (taps)")
        empty = sum(1 for s in range(count) if not slabs[s].any())
        assert empty >= count - steps, (label, count, empty)


# ---------------------------------------------------------------------------------------------------------------------
# 3.0 the premise
# ---------------------------------------------------------------------------------------------------------------------
_PREMISE_STATE = {}


def _premise():
    """-> {check name: bool} of the simplest launches: 128 x 32 x 128, plain, config 8 / one slice."""
    if not _PREMISE_STATE:
        C = _C()
        for lo in (False, True):
            A, ap = _operand(128, 32, lo, 1)
            B, bp = _operand(128, 32, lo, 2)
            want, _ = E.three_term(A, B.T)
            y, _ = C.split_gemm_pair(ap, bp, config=8)
            _PREMISE_STATE[f"forward {'lo-bearing' if lo else 'integers'}"] = bool(torch.equal(y, _dev(want.astype(np.float32))))
            # transpose-read: the same 128 x 32 x 128 product contracts over the 32 ROWS of G [32, 128] and X [32, 128]
            G, gp = _operand(32, 128, lo, 3)
            X, xp = _operand(32, 128, lo, 4)
            want_t, _ = E.three_term(G.T, X)
            rc, slabs = _tn(gp, xp, 1, 32, 128, 128)
            _PREMISE_STATE[f"transpose-read {'lo-bearing' if lo else 'integers'}"] = bool(
                rc == OVIS_OK and torch.equal(slabs[0], _dev(want_t.astype(np.float32))))
    return _PREMISE_STATE


def test_premise_exact_accumulation():
    """bf16 MFMA with fp32 accumulation returns the exact three-term value when every partial sum is representable:
    128 x 32 x 128, plain, ``config = 8``, integers and then lo-bearing operands, through ``split_gemm_pair`` and through
    the transpose-read kernel (one slice)."""
    state = _premise()
    print(state)
    assert all(state.values()), state


@pytest.fixture(autouse=True)
def _needs_premise(request):
    if request.node.name.startswith(("test_premise", "test_partial_last_map", "test_cases_reach")):
        return
    bad = [k for k, ok in _premise().items() if not ok]
    if bad:
        pytest.fail(f"{PREMISE} failed ({bad}): exact equality means nothing on this device")


# ---------------------------------------------------------------------------------------------------------------------
# 3.1 weight gradient, general form, 1x1
# ---------------------------------------------------------------------------------------------------------------------
TN_M = [(1, True), (31, True), (32, True), (33, True), (95, True), (1000, True), (4129, True), (7999, True), (40001, False)]
TN_NCH = [(128, 128), (256, 128), (128, 384)]        # tile-major order of the launcher: G-major, G-major, X-major


@functools.lru_cache(maxsize=None)
def _tn_plain_case(m, lo, n, ch):
    rows = 7999 if lo else 40001
    G, _ = _operand(rows, 256, lo, 11)
    X, _ = _operand(rows, 384, lo, 12)
    want, _ = E.three_term(G[:m, :n].T, X[:m, :ch])
    return G[:m, :n], X[:m, :ch], want.astype(np.float32)


@pytest.mark.parametrize("n,ch", TN_NCH)
@pytest.mark.parametrize("m,lo", TN_M)
def test_weight_gradient_1x1_every_slice_count(m, lo, n, ch):
    C = _C()
    G, X, want = _tn_plain_case(m, lo, n, ch)
    gp, xp = _to_dev_pair(G), _to_dev_pair(X)
    steps = -(-m // 32)
    counts = sorted({1, 2, 3, 7, C._tn_slices(m, n, ch, 1), steps + 2})
    print(f"[3.1] M={m} n={n} ch={ch}: slice counts {counts} (the library's: {C._tn_slices(m, n, ch, 1)})")
    _check_tn(gp, xp, counts, m, n, ch, want, label=f"tn 1x1 M={m} n={n} ch={ch}")


def test_weight_gradient_1x1_column_slices_of_wider_pair_tensors():
    """G = values 32 .. 160 of 256-value pair rows, X = values 64 .. 192 of 384-value ones (whole hi | lo groups)."""
    m, n, ch = 4129, 128, 128
    G, gw = _operand(7999, 256, True, 11)
    X, xw = _operand(7999, 384, True, 12)
    gs, xs = gw[:m, 64:64 + 2 * n], xw[:m, 128:128 + 2 * ch]
    assert gs.stride(0) > gs.shape[1] and xs.stride(0) > xs.shape[1]
    want, _ = E.three_term(G[:m, 32:32 + n].T, X[:m, 64:64 + ch])
    _check_tn(gs, xs, sorted({1, 3, _C()._tn_slices(m, n, ch, 1)}), m, n, ch, want.astype(np.float32), label="tn 1x1 column slices")


# ---------------------------------------------------------------------------------------------------------------------
# 3.2 weight gradient, general form, taps
# ---------------------------------------------------------------------------------------------------------------------
TN_TAPS = [
    # h, w, kh, kw
    (9, 8, 3, 3),     # 72 pixels: just above the in-map-rows form
    (5, 13, 3, 3),
    (3, 40, 3, 3),    # W > 32
    (2, 33, 3, 5),
    (1, 65, 1, 3),
    (65, 1, 3, 1),
    (2, 8, 7, 1),     # more than 5 taps a side on a small map: general form, 32 / W + 1 > H
    (8, 2, 1, 7),
]


def _tn_conv_want(G, X, r, h, w, kh, kw):
    want, _ = E.three_term(G.T, E.tap_rows(X, r, h, w, kh, kw))
    want = want.astype(np.float32)
    n, ch = G.shape[1], X.shape[1]
    for tap in range(kh * kw):          # a tap without any in-map row: exact zeros (a property of the expected value)
        dy, dx = tap // kw - kh // 2, tap % kw - kw // 2
        if abs(dy) >= h or abs(dx) >= w:
            assert not want.reshape(n, kh * kw, ch)[:, tap].any()
    return want


@pytest.mark.parametrize("h,w,kh,kw", TN_TAPS)
def test_weight_gradient_taps_general_form(h, w, kh, kw):
    C = _C()
    n = ch = 128
    assert h * w > 64 or max(kh, kw) > 5            # not the in-map-rows form
    for r in (1, 3, -(-2100 // (h * w))):
        m = r * h * w
        G, gp = _operand(m, n, True, 31)
        X, xp = _operand(m, ch, True, 32)
        lib = C._tn_map_slices(m, n, ch, kh, kw, h, w)
        assert lib == C._tn_slices(m, n, ch, kh * kw)
        counts = sorted({1, 3, lib} | ({5} if m > 1000 else set()))
        print(f"[3.2] {r} x {h} x {w}, {kh} x {kw} taps, M={m}: slice counts {counts} (the library's: {lib})")
        _check_tn(gp, xp, counts, m, n, ch, _tn_conv_want(G, X, r, h, w, kh, kw), (kh, kw, h, w),
                  label=f"tn {kh}x{kw} on {r}x{h}x{w}")


def test_weight_gradient_taps_general_form_large_map_integers():
    C = _C()
    r, h, w, kh, kw, n, ch = 1, 50, 84, 3, 3, 128, 128
    m = r * h * w
    G, gp = _operand(m, n, False, 33)
    X, xp = _operand(m, ch, False, 34)
    lib = C._tn_map_slices(m, n, ch, kh, kw, h, w)
    print(f"[3.2] 1 x 50 x 84, 3 x 3 taps, M={m}: the library's slice count {lib}")
    _check_tn(gp, xp, sorted({1, 3, lib}), m, n, ch, _tn_conv_want(G, X, r, h, w, kh, kw), (kh, kw, h, w), label="tn 3x3 on 50x84")


# ---------------------------------------------------------------------------------------------------------------------
# 3.3 weight gradient, in-map-rows form, dense operands
# ---------------------------------------------------------------------------------------------------------------------
TN_SMALL = [
    # r, h, w, kh, kw, n, ch
    (70, 7, 7, 3, 3, 128, 128),
    (70, 7, 7, 3, 3, 128, 256),      # X-major tile order
    (7, 5, 3, 3, 3, 128, 128),
    (5, 8, 8, 3, 3, 128, 128),
    (33, 1, 1, 3, 3, 128, 128),
    (9, 1, 7, 3, 3, 128, 128),
    (11, 7, 7, 5, 5, 128, 128),
]


@pytest.mark.parametrize("r,h,w,kh,kw,n,ch", TN_SMALL)
def test_weight_gradient_in_map_rows_dense(r, h, w, kh, kw, n, ch):
    C = _C()
    assert h * w <= 64 and max(kh, kw) <= 5
    m = r * h * w
    G, gp = _operand(m, n, True, 41)
    X, xp = _operand(m, ch, True, 42)
    lib = C._tn_map_slices(m, n, ch, kh, kw, h, w)
    counts = sorted({1, 2, 5, 13, lib})
    print(f"[3.3] {r} x {h} x {w}, {kh} x {kw} taps, n={n} ch={ch}: slice counts {counts} (the library's: {lib})")
    # (the zero-slab count of _check_tn is stated in 32-row steps of M: a lower bound here too, a tap has at most M rows)
    _check_tn(gp, xp, counts, m, n, ch, _tn_conv_want(G, X, r, h, w, kh, kw), (kh, kw, h, w), label=f"tn small {kh}x{kw} on {r}x{h}x{w}")


# ---------------------------------------------------------------------------------------------------------------------
# 3.4 fused slab reduce
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,h,w,kh,kw,n,ch", [(4129, 1, 1, 1, 1, 256, 128), (70, 7, 7, 3, 3, 128, 128)])
def test_fused_slab_reduce_is_exact_in_the_weight_layout(r, h, w, kh, kw, n, ch):
    """``split_gemm_pair_tn(..., scale = 2^k per channel, weight_shape)``: the slab sum times a power of two, relaid to
    (N, ch, kh, kw) -- exact."""
    C = _C()
    m = r * h * w
    conv = None if kh * kw == 1 else (h, w, kh, kw)
    if conv is None:
        G, X, want = _tn_plain_case(m, True, n, ch)
        gp, xp = _to_dev_pair(G), _to_dev_pair(X)
    else:
        G, gp = _operand(m, n, True, 41)
        X, xp = _operand(m, ch, True, 42)
        want = _tn_conv_want(G, X, r, h, w, kh, kw)
    scale = (2.0 ** ((np.arange(n) % 7) - 3)).astype(np.float32)
    want4 = np.ascontiguousarray((want * scale[:, None]).reshape(n, kh * kw, ch).transpose(0, 2, 1)).reshape(n, ch, kh, kw)
    got = C.split_gemm_pair_tn(gp, xp, conv, scale=_dev(scale), weight_shape=(n, ch, kh, kw))
    assert got.shape == (n, ch, kh, kw) and torch.equal(got, _dev(want4))
    assert torch.equal(C.split_gemm_pair_tn(gp, xp, conv), _dev(want))              # and the un-fused sum of the slabs


# ---------------------------------------------------------------------------------------------------------------------
# 3.5 forward, every form
# ---------------------------------------------------------------------------------------------------------------------
PLAIN_SHAPES = [(1, 4, 32), (127, 64, 512), (128, 76, 4608), (129, 132, 512), (300, 256, 4608), (300, 132, 32),
                (129, 256, 512), (1, 256, 4608), (300, 4, 4608), (128, 64, 32)]          # every M, N, K of the issue
PLAIN_CONFIGS = [0, 1, 2, 8, 2 << 8, 3 << 8, CO]


@functools.lru_cache(maxsize=None)
def _plain_ref(k):
    A, _ = _operand(300, 4608, True, 21)
    W, _ = _operand(256, 4608, True, 22)
    val, S = E.three_term(A[:, :k], W[:, :k].T)
    return val, S


def _mismatch(label, got, want_t):
    """The mismatch pattern for the assertion message: how many entries, which rows, by how many units of 2^-9."""
    d = (got.double() - want_t.double()).abs()
    bad = d.nonzero()
    rows = sorted(set(bad[:, 0].tolist()))
    return (f"{label}: {bad.shape[0]} of {d.numel()} entries differ, largest by {d.max().item() / E.LO_UNIT:.1f} x 2^-9; "
            f"rows {rows[:8]}{'...' if len(rows) > 8 else ''} ({len(rows)} rows), first at {bad[0].tolist()}")


def _assert_pair_output(label, y, yp):
    assert yp is not None and torch.equal(yp, _C().split_pair(y)), label


@pytest.mark.parametrize("cfg", PLAIN_CONFIGS)
def test_forward_plain_every_shape(cfg):
    C = _C()
    _, ap_full = _operand(300, 4608, True, 21)
    _, wp_full = _operand(256, 4608, True, 22)
    sliced = []
    for m, n, k in PLAIN_SHAPES:
        val, _ = _plain_ref(k)
        want = val[:m, :n].astype(np.float32)
        ns = slices(m, n, k, 0, 1, 1, 0, cfg)
        sliced.append(ns)
        ap, wp = ap_full[:m, :2 * k].contiguous(), wp_full[:n, :2 * k].contiguous()
        y, yp = C.split_gemm_pair(ap, wp, None, None, False, True, n % 32 == 0, config=cfg)
        label = f"[3.5] plain {m} x {n} x {k} config={cfg:#x} slices={ns}"
        print(label)
        want_t = _dev(want)
        assert torch.equal(y, want_t), _mismatch(label, y, want_t)
        if n % 32 == 0:
            _assert_pair_output(label, y, yp)
    if cfg & 8:
        assert set(sliced) == {1}                   # config 8 IS the un-sliced grid
    else:
        assert max(sliced) > 1, (hex(cfg), sliced)  # at least one case of this config really is sliced
        assert min(sliced) == 1                     # ... and one is not (the narrow kernels have no sliced form)


A2_CASES = [
    # m, ch, ch2, n, config, slices expected from the query
    (490, 160, 96, 256, 3 << 8, 3),     # 8 k-steps in 3 slices: the A | A2 seam (after step 5) lies inside a slice
    (490, 128, 128, 256, 2 << 8, 2),    # 8 k-steps in 2 slices: the seam is the slice boundary
    (490, 160, 96, 256, 8, 1),
    (490, 160, 96, 256, 0, None),
    (490, 160, 96, 256, 1, None),
    (490, 160, 96, 256, 2, None),
    (129, 32, 32, 132, 8, 1),           # one k-step either side of the seam, ragged tile
]


@pytest.mark.parametrize("m,ch,ch2,n,cfg,want_slices", A2_CASES)
def test_forward_plain_second_operand_seam(m, ch, ch2, n, cfg, want_slices):
    C = _C()
    A, ap = _operand(m, ch, True, 23)
    A2, a2p = _operand(m, ch2, True, 24)
    W, wp = _operand(n, ch + ch2, True, 25)
    ns = slices(m, n, ch, ch2, 1, 1, 0, cfg)
    if want_slices is not None:
        assert ns == want_slices
    val, _ = E.three_term(np.concatenate([A, A2], 1), W.T)
    y, yp = C.split_gemm_pair(ap, wp, None, None, False, True, n % 32 == 0, config=cfg, a2_pair=a2p)
    label = f"[3.5] a2 {m} x {n} x ({ch}+{ch2}) config={cfg:#x} slices={ns}"
    print(label)
    want_t = _dev(val.astype(np.float32))
    assert torch.equal(y, want_t), _mismatch(label, y, want_t)
    if n % 32 == 0:
        _assert_pair_output(label, y, yp)


CONV_GEOMS = [(1, 7, 7), (3, 7, 7), (5, 7, 7), (37, 7, 7),     # tiles of 128 rows start in the middle of a map
              (130, 1, 1), (20, 1, 7), (20, 7, 1), (3, 5, 9), (2, 14, 14)]
CONV_KERNELS = [(3, 3), (3, 5)]
CONV_CONFIGS = [0, 1, 8, 4, 5, 6, 12]   # HALO where the plan allows it (0; 1; un-sliced 8), SHIFTED (4; one stage 5; two stages 6;
                                        # un-sliced 12)
CONV_CH, CONV_N = 64, 128


@pytest.mark.parametrize("kh,kw", CONV_KERNELS)
@pytest.mark.parametrize("r,h,w", CONV_GEOMS)
def test_forward_implicit_convolution_shifted_and_halo(r, h, w, kh, kw):
    C = _C()
    m, ch, n = r * h * w, CONV_CH, CONV_N
    A, ap = _operand(m, ch, True, 26)
    W, wp = _operand(n, kh * kw * ch, True, 27)
    for flip in (False, True):
        val, _ = E.three_term(E.tap_rows(A, r, h, w, kh, kw, flip), W.T)
        want_t = _dev(val.astype(np.float32))
        for cfg in CONV_CONFIGS:
            ns, units = slices(m, n, ch, 0, kh, kw, w, cfg), k_units(m, n, ch, kh, kw, w, cfg)
            y, yp = C.split_gemm_pair(ap, wp, None, None, False, True, True, conv=(h, w, kh, kw, flip), config=cfg)
            label = (f"[3.5] {kh}x{kw}{' flip' if flip else ''} on {r}x{h}x{w} config={cfg:#x} slices={ns} "
                     f"form={'HALO' if units == ch // 32 else 'SHIFTED'}")
            print(label)
            assert torch.equal(y, want_t), _mismatch(label, y, want_t)
            _assert_pair_output(label, y, yp)


@pytest.mark.parametrize("n", [64, 20])
def test_forward_narrow_plain_and_3x3(n):
    C = _C()
    r, h, w, ch = 5, 7, 7, 64
    m = r * h * w
    A, ap = _operand(m, ch, True, 26)
    W, wp = _operand(n, 9 * ch, True, 28)
    for flip in (False, True):
        val, _ = E.three_term(E.tap_rows(A, r, h, w, 3, 3, flip), W.T)
        for cfg in (0, 8):
            assert slices(m, n, ch, 0, 3, 3, w, cfg) == 1
            y, yp = C.split_gemm_pair(ap, wp, None, None, False, True, n % 32 == 0, conv=(h, w, 3, 3, flip), config=cfg)
            want_t = _dev(val.astype(np.float32))
            label = f"[3.5] narrow 3x3{' flip' if flip else ''} n={n} config={cfg:#x}"
            assert torch.equal(y, want_t), _mismatch(label, y, want_t)
            if n % 32 == 0:
                _assert_pair_output(label, y, yp)
    W1, w1p = _operand(n, ch, True, 29)
    val, _ = E.three_term(A, W1.T)
    y, _ = C.split_gemm_pair(ap, w1p, None, None, False, True, False, config=0)
    assert torch.equal(y, _dev(val.astype(np.float32))), "[3.5] narrow plain"


EPI_SHAPES = [(300, 256, 512), (129, 76, 512)]     # sliced under config 0 (the finish kernel's epilogue), un-sliced under 8


@pytest.mark.parametrize("cfg", [8, 0, 3 << 8])
@pytest.mark.parametrize("m,n,k", EPI_SHAPES)
def test_forward_epilogues(m, n, k, cfg):
    C = _C()
    A, ap = _operand(m, k, True, 51)
    W, wp = _operand(n, k, True, 52)
    val, S = E.three_term(A, W.T)
    ns = slices(m, n, k, 0, 1, 1, 0, cfg)
    assert (ns > 1) == (cfg != 8)
    b, res, gate = E.bias(n, 53), E.residual(m, n, 54), E.gate01(m, n, 55)
    bd, resd = _dev(b), _dev(res)
    wide = torch.zeros(m, n + 24, device="cuda")
    wide[:, 8:8 + n] = resd
    res_view = wide[:, 8:8 + n]
    assert not res_view.is_contiguous()
    pair = n % 32 == 0
    for name, kw_ref, bias_t, res_t, relu in (
            ("bias", dict(bias=b), bd, None, False),
            ("fp32 residual", dict(residual=res), None, resd, False),
            ("fp32 residual, row-strided", dict(residual=res), None, res_view, False),
            ("relu", dict(relu=True), None, None, True),
            ("bias + residual + relu", dict(bias=b, residual=res, relu=True), bd, resd, True)):
        want = E.epilogue(val, S, **kw_ref)
        y, yp = C.split_gemm_pair(ap, wp, bias_t, res_t, relu, True, pair, config=cfg)
        label = f"[3.5] epilogue {name} {m} x {n} x {k} config={cfg:#x} slices={ns}"
        print(label)
        want_t = _dev(want)
        assert torch.equal(y, want_t), _mismatch(label, y, want_t)
        if pair:
            _assert_pair_output(label, y, yp)
    if not pair:
        return
    resp, gatep = _to_dev_pair(res), _to_dev_pair(gate)
    for name, relu, bias_t, kw_ref in (("pair residual", False, None, dict(residual=res)),
                                       ("bias + pair residual + relu", True, bd, dict(bias=b, residual=res, relu=True))):
        want_t = _dev(E.epilogue(val, S, **kw_ref))
        y, yp = C.split_gemm_pair(ap, wp, bias_t, None, relu, True, True, config=cfg, residual_pair=resp)
        label = f"[3.5] epilogue {name} config={cfg:#x} slices={ns}"
        assert torch.equal(y, want_t), _mismatch(label, y, want_t)
        _assert_pair_output(label, y, yp)
        none, only_p = C.split_gemm_pair(ap, wp, bias_t, None, relu, False, True, config=cfg, residual_pair=resp)
        assert none is None and torch.equal(only_p, yp)
    want_t = _dev(E.epilogue(val, S, gate=gate))
    y, yp = C.split_gemm_pair_gated(ap, wp, gatep, out_f32=True, out_pair=True, config=cfg)
    label = f"[3.5] epilogue gate config={cfg:#x} slices={ns}"
    assert torch.equal(y, want_t), _mismatch(label, y, want_t)
    _assert_pair_output(label, y, yp)
    assert not y[_dev(gate) == 0].any()
    # the DUAL kernel (pair shortcut + gate) is never sliced: the stage bits only
    want_t = _dev(E.epilogue(val, S, residual=res, gate=gate))
    for stage in (0, 1, 2):
        y, yp = C.split_gemm_pair_rp_gated(ap, wp, resp, gatep, out_f32=True, out_pair=True, config=(cfg & ~0xff00) | stage)
        label = f"[3.5] epilogue pair residual + gate (dual) config={(cfg & ~0xff00) | stage:#x}"
        assert torch.equal(y, want_t), _mismatch(label, y, want_t)
        _assert_pair_output(label, y, yp)


@pytest.mark.parametrize("cfg", [0, 4, (2 << 8) | 4])
def test_forward_gated_data_gradient_convolution(cfg):
    """``split_gemm_pair_gated`` on the flipped 3x3 (the data gradient of a convolution behind a ReLU): HALO, SHIFTED, and
    SHIFTED in two K slices (the finish kernel applies the gate)."""
    C = _C()
    r, h, w, ch, n = 5, 7, 7, CONV_CH, CONV_N
    m = r * h * w
    A, ap = _operand(m, ch, True, 26)
    W, wp = _operand(n, 9 * ch, True, 27)
    gate = E.gate01(m, n, 56)
    val, S = E.three_term(E.tap_rows(A, r, h, w, 3, 3, True), W.T)
    y, yp = C.split_gemm_pair_gated(ap, wp, _to_dev_pair(gate), conv=(h, w, 3, 3, True), out_f32=True, out_pair=True, config=cfg)
    want_t = _dev(E.epilogue(val, S, gate=gate))
    label = f"[3.5] gated 3x3 flip config={cfg:#x} slices={slices(m, n, ch, 0, 3, 3, w, cfg)}"
    print(label)
    assert torch.equal(y, want_t), _mismatch(label, y, want_t)
    _assert_pair_output(label, y, yp)


def test_forward_pooled_epilogue():
    """``split_gemm_pair_rp_pool`` with ``pool_rows = 64``: the 1 / 64 scale keeps the pooled means exact."""
    C = _C()
    m, n, k, pool = 320, 128, 64, 64          # 2.5 row tiles: the last one ragged, a pool group per 64-row wave span
    assert C.split_gemm_pair_pool_supported(m, n, k, pool)
    A, ap = _operand(m, k, True, 57)
    W, wp = _operand(n, k, True, 58)
    val, S = E.three_term(A, W.T)
    b, res = E.bias(n, 59), E.residual(m, n, 60)
    want = E.epilogue(val, S, bias=b, residual=res, relu=True)
    budget = S + np.abs(b.astype(np.float64))[None, :] + np.abs(res.astype(np.float64))
    want_pool = E.pooled_mean(want, budget, pool)
    y, yp, pooled = C.split_gemm_pair_rp_pool(ap, wp, _dev(b), _to_dev_pair(res), True, True, True, pool)
    want_t = _dev(want)
    assert torch.equal(y, want_t), _mismatch("[3.5] pooled epilogue", y, want_t)
    _assert_pair_output("[3.5] pooled epilogue", y, yp)
    assert torch.equal(pooled, _dev(want_pool))
    none_c, none_p, only = C.split_gemm_pair_rp_pool(ap, wp, _dev(b), _to_dev_pair(res), True, False, False, pool)
    assert none_c is None and none_p is None and torch.equal(only, _dev(want_pool))


# ---------------------------------------------------------------------------------------------------------------------
# 3.6 coverage guard
# ---------------------------------------------------------------------------------------------------------------------
def test_cases_reach_every_form():
    """From the library's queries only: the case tables above reach un-sliced and sliced launches, the one- and two-stage
    bits on forms whose plan honours them (the stage count itself is not visible in a query: bits 1 / 2 leave the slice
    count alone, which is asserted), narrow and wide tiles, the HALO and the SHIFTED form (told apart by what a forced
    slice count is clamped to), both tile-major orders of the weight gradient, and un-sliced and sliced weight gradients.
    A change of the plan that drops a form fails here instead of silently un-testing it."""
    C = _C()
    hint = "the plan changed: re-pick the shapes of tests/test_split_gemm_exact_gpu.py so that every form is exercised"
    plain = {(m, n, k, cfg): slices(m, n, k, 0, 1, 1, 0, cfg) for m, n, k in PLAIN_SHAPES for cfg in PLAIN_CONFIGS}
    assert {1} < set(plain.values()), (hint, plain)
    for cfg in PLAIN_CONFIGS:
        got = {ns for (_, _, _, c), ns in plain.items() if c == cfg}
        assert (got == {1}) if cfg & 8 else (1 in got and max(got) > 1), (hint, hex(cfg), got)
    # forced counts are honoured on a wide shape, ignored on a narrow one
    assert plain[(300, 256, 4608, 2 << 8)] == 2 and plain[(300, 256, 4608, 3 << 8)] == 3 and plain[(127, 64, 512, 3 << 8)] == 1, hint
    # stage bits: present among the cases, on wide non-HALO shapes, and they leave the slice count alone
    for m, n, k in PLAIN_SHAPES:
        assert plain[(m, n, k, 1)] == plain[(m, n, k, 0)] == plain[(m, n, k, 2)], (hint, m, n, k)
    assert any(n > 64 for _, n, _ in PLAIN_SHAPES) and any(n <= 64 for _, n, _ in PLAIN_SHAPES)
    assert {1, 2} <= set(PLAIN_CONFIGS) and {5, 6} <= set(CONV_CONFIGS)
    # HALO and SHIFTED
    forms = {}
    for r, h, w in CONV_GEOMS:
        for kh, kw in CONV_KERNELS:
            for cfg in CONV_CONFIGS:
                units = k_units(r * h * w, CONV_N, CONV_CH, kh, kw, w, cfg)
                assert units in (CONV_CH // 32, kh * kw * CONV_CH // 32), (hint, units)
                forms[(r, h, w, kh, kw, cfg)] = "HALO" if units == CONV_CH // 32 else "SHIFTED"
    print({k: v for k, v in forms.items() if v == "HALO"})
    assert forms[(37, 7, 7, 3, 3, 0)] == "HALO" and forms[(37, 7, 7, 3, 3, 1)] == "HALO", (hint, "7x7 3x3 is no longer HALO")
    assert all(v == "SHIFTED" for k, v in forms.items() if k[5] & 4), hint
    assert forms[(37, 7, 7, 3, 5, 0)] == "SHIFTED" and forms[(2, 14, 14, 3, 3, 0)] == "SHIFTED", hint
    halo_sliced = {slices(r * h * w, CONV_N, CONV_CH, 0, kh, kw, w, cfg) for (r, h, w, kh, kw, cfg), v in forms.items() if v == "HALO"}
    shifted_sliced = {slices(r * h * w, CONV_N, CONV_CH, 0, kh, kw, w, cfg) for (r, h, w, kh, kw, cfg), v in forms.items() if v == "SHIFTED"}
    assert max(halo_sliced) > 1 and 1 in halo_sliced and max(shifted_sliced) > 1 and 1 in shifted_sliced, (hint, halo_sliced, shifted_sliced)
    # weight gradient: both tile-major orders (G-major when N has at least as many 128-column tiles as ch), slice counts
    assert any(n // 128 >= ch // 128 for n, ch in TN_NCH) and any(n // 128 < ch // 128 for n, ch in TN_NCH)
    assert any(n // 128 < ch // 128 for *_, n, ch in TN_SMALL) and any(n // 128 >= ch // 128 for *_, n, ch in TN_SMALL)
    lib_plain = {C._tn_slices(m, n, ch, 1) for m, _ in TN_M for n, ch in TN_NCH}
    lib_small = {C._tn_map_slices(r * h * w, n, ch, kh, kw, h, w) for r, h, w, kh, kw, n, ch in TN_SMALL}
    assert 1 in lib_plain and max(lib_plain) > 1 and 1 in lib_small and max(lib_small) > 1, (hint, lib_plain, lib_small)


# ---------------------------------------------------------------------------------------------------------------------
# 4. the C boundary: whole maps only
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,kh,kw,m", [(7, 7, 3, 3, 50), (7, 7, 3, 3, 48), (9, 8, 3, 3, 100), (2, 8, 7, 1, 17), (1, 65, 1, 3, 64)])
def test_partial_last_map_is_refused_by_the_c_entry_points(h, w, kh, kw, m):
    """T > 1 and m % (height * width) != 0: the rows of the partial last map would read their taps behind the operand.
    ``ovis_split_gemm_pair_tn``, ``ovis_split_gemm_pair`` and ``ovis_split_gemm_pair_gated_ws`` return OVIS_EINVAL before
    any launch (valid, fully sized device buffers; the outputs stay untouched)."""
    C = _C()
    assert m % (h * w) != 0
    n = ch = 128
    t = kh * kw
    ap = torch.zeros(m, 2 * ch, dtype=torch.bfloat16, device="cuda")
    gp = torch.zeros(m, 2 * n, dtype=torch.bfloat16, device="cuda")
    wp = torch.zeros(n, 2 * t * ch, dtype=torch.bfloat16, device="cuda")
    slabs = torch.full((2, n, t * ch), 7.0, device="cuda")
    rc = C._L.ovis_split_gemm_pair_tn(gp.data_ptr(), 2 * gp.stride(0), ap.data_ptr(), 2 * ap.stride(0), slabs.data_ptr(), 2, m, n,
                                      ch, kh, kw, h, w, C._stream())
    assert rc == OVIS_EINVAL
    c = torch.full((m, n), 7.0, device="cuda")
    cp = torch.zeros(m, 2 * n, dtype=torch.bfloat16, device="cuda")
    for cfg in (0, 4, 8):
        for flip in (0, 1):
            rc = C._L.ovis_split_gemm_pair(ap.data_ptr(), 2 * ap.stride(0), 0, 0, wp.data_ptr(), 2 * wp.stride(0), c.data_ptr(), n,
                                           cp.data_ptr(), 4 * n, 0, 0, 0, m, n, ch, 0, kh, kw, h, w, flip, 0, 0, 0, cfg, C._stream())
            assert rc == OVIS_EINVAL, (cfg, flip)
            rc = C._L.ovis_split_gemm_pair_gated_ws(ap.data_ptr(), 2 * ap.stride(0), wp.data_ptr(), 2 * wp.stride(0), c.data_ptr(), n,
                                                    cp.data_ptr(), 4 * n, gp.data_ptr(), 2 * gp.stride(0), m, n, ch, kh, kw, h, w,
                                                    flip, 0, 0, cfg, C._stream())
            assert rc == OVIS_EINVAL, (cfg, flip, "gated")
    torch.cuda.synchronize()
    assert bool((slabs == 7.0).all()) and bool((c == 7.0).all()) and not cp.any()
