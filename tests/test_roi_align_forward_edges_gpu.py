"""GPU: every form of the RoIAlign forward -- the exact NCHW kernel (csrc/roi_align.hip ``roi_align_fwd_kernel``), the
matrix-core kernel (csrc/roi_align_fwd_mfma.hip) and the strided NHWC poolers (``roi_align_fwd_nhwc_in_strided_lds_kernel``,
``roi_align_fwd_nhwc_in_strided_kernel``) -- against the independent fp64 reference tests/roi_align_reference.py
(``roi_align_forward_ref``, pinned by tests/test_roi_align_reference.py), elementwise and without a floor:

    |got - ref| <= TOL * mag + slack            exact zeros wherever mag == 0 and slack == 0

``mag`` = sum weight * |x| / count, ``slack`` = what K_ULPS = 3 float32 ulps on every sample coordinate may move.  Exact forms:
(terms + 5) * 2^-24 * mag + slack (derived at ``FWD_C``), and bit-equal to the oracle's float32 restatement of the reference
CPU kernel.  Matrix-core form: TOL_MFMA = 4e-5 (two chained split products, V re-split in between).  Strided poolers: the
oracle's bins (s i, s j) bit for bit, pair rows equal to bf16 hi | lo rows built in NumPy from the oracle's bins.

Every table is built on the host (NumPy, nothing at import) and held to three conditions before anything is launched, all
of them checked without a GPU by tests/test_roi_align_reference.py as well: no finite RoI has a sampling grid above 16 per
axis, every RoI with a non-finite coordinate is one ``make_geom`` declares empty, and every sample is >= 4 d clear of the
validity boundaries.  The dispatch classes a table claims (``claims``: table / per-lane / tail batches, the power-of-two flag,
window budgets, block shapes, strided window classes, shared-tap states) are computed with the float32 twin ``geom32``.

  A  exact kernel: channel batches C = 31, 33, 1, 2, 3, 5 (tab16/8/4 + tail2/1, a second 32-channel tile); sampling ratios
     0 .. 4 with adaptive grids 3 and 5 (FAST and division paths); tables that do not fit (14 x 14 at ratio 5: 70 entries;
     17 x 17: 289 bins, two passes); poolers (1,16), (16,1), (3,5), (7,14); windows of exactly 272, 544, 1088, 2176 and 4352
     cells on a 64 x 68 map (and one cell class above each) and the 4420-cell whole map of 65 x 68 (global gathers); scales
     1/4, 1/32, 1 and 0.3; the edge RoIs, image ids -1 and n, NaN / +Inf / -Inf coordinates in every table; NaN written
     everywhere more than one cell outside every window changes no bit.
  B  matrix-core kernel: PW in {1 .. 8, 13, 16} x PH in {1, 7, 16} (every ``PW % 4`` tail store, PW < 4, both NST); windows of
     1x1, 1x2, 2x1, 2x2, 3x2, 2x3 and 4x6 blocks incl. pulled-back last blocks; maps 16x16, 16x84, 50x16, 17x33; the
     unsupported 20x9 map and 17x17 pooler bit-equal to the exact kernel; C = 1, 3, 4, 5, 63, 64, 65, 130; sentinel bands
     around the output; one-hot maps.  Finite maps only (the 16-cell block footprints multiply zero weights with whatever
     lies in the block), so no NaN-immunity test on this form.
  C  strided NHWC poolers on channels-last maps: C = 32, 64, 96 (LDS kernel), 8, 36 (direct kernel); all four window classes;
     all 25 (row state, column state) pairs of the shared-tap path at sampling ratio 2; ratios 0, 1, 3; strides 1, 2, 3, 14;
     poolers 14, 7 and (7,14); foreign-id and NaN RoIs; the C entry point's refusals.

Largest measured error / bound per section on an MI355X (every test prints its own; run with ``-s``):
  A  exact kernel               0.235  (channels-c31-p14; bit-equal to the oracle, whose own float32 forward measures the same
                                       0.235 on the CPU; the other tables 0.08 .. 0.21, the NaN-immunity table 0.165)
  B  tail stores                0.323  (PW = 13; PW = 1 0.167, the others 0.22 .. 0.30)
     block shapes / one-hot     0.250 / 0.165
     maps                       0.453  (17 x 33; 16 x 16 0.401, 50 x 16 0.358, 16 x 84 0.328)
     channels                   0.437  (C = 130; the others 0.26 .. 0.37)
  C  strided poolers            0.240  (C = 36; the others 0.22 .. 0.24; bins and pair rows bit for bit)
The matrix-core figures are the hi/lo algorithm's share, not the kernel's: ``split_form_emulation_forward`` on the reference's
own weights gives 0.452 on the 17 x 33 map, 0.323 on the 7 x 13 pooler and 0.405 at C = 130 on the CPU
(tests/test_roi_align_reference.py prints the largest).
"""
import collections
import functools

import numpy as np
import pytest
import torch

from tests import roi_align_reference as R

pytestmark = pytest.mark.gpu

S = R.SCALE
_REF = {}
_f = np.float32

Case = collections.namedtuple("Case", "name n c h w scale ph pw srs rois claims cells")


# ------------------------------------------------------------------ host helpers (NumPy only)
def box(b, y0, y1, x0, x1, scale=S):
    """A RoI given in feature cells"""
    return [b, x0 / scale, y0 / scale, x1 / scale, y1 / scale]


def win_roi(b, oy, ny, ox, nx, scale=S):
    """A RoI whose window is exactly rows oy .. oy + ny - 1, columns ox .. ox + nx - 1: the first sample lies less than half
    a cell (bin / 2 grid <= 0.5) above oy + 0.2, the last less than half a cell below oy + ny - 1.1."""
    return box(b, oy + 0.2, oy + ny - 1.1, ox + 0.2, ox + nx - 1.1, scale)


def limit_grid(rois, scale, ph, pw):
    """No side above 15.5 cells per bin: the adaptive grid ceil(side / P) stays <= 16."""
    rois = np.array(rois, dtype=_f)
    finite = np.all(np.isfinite(rois), axis=1)
    for k, p in ((3, pw), (4, ph)):
        rois[finite, k] = np.minimum(rois[finite, k], rois[finite, k - 2] + _f(15.5 * p / scale))
    return rois


def base_rois(seed, n, h, w, r_random, scale=S):
    """Random RoIs and the edge RoIs, in the pixels of ``scale``"""
    rois = np.concatenate([R.random_rois(seed, r_random, n, h, w), R.edge_rois(h, w)])
    rois[:, 0] = np.minimum(rois[:, 0], n - 1)
    rois[:, 1:] *= _f(S / scale)
    return rois


def special_rois(n, h, w, scale=S):
    """Foreign image ids and non-finite coordinates of the kind ``make_geom`` rejects: exact zeros in every form."""
    iw, ih, nan, inf = w / scale, h / scale, float("nan"), float("inf")
    return np.array([[-1, 0.2 * iw, 0.2 * ih, 0.6 * iw, 0.7 * ih], [n, 0.2 * iw, 0.2 * ih, 0.6 * iw, 0.7 * ih],
                     [0, nan, 0.2 * ih, 0.6 * iw, 0.7 * ih], [n - 1, 0.2 * iw, 0.2 * ih, inf, 0.7 * ih],
                     [0, 0.2 * iw, -inf, 0.6 * iw, 0.7 * ih], [0, inf, 0.1 * ih, inf, 0.5 * ih]], dtype=_f)


def make_case(name, n, c, h, w, ph, pw, srs, rois, claims, scale=S, cells=()):
    """Limits the grids, clears the samples for every sampling ratio of the case, appends the special RoIs."""
    rois = R.cleared(limit_grid(rois, scale, ph, pw), ph, pw, n, h, w, srs, scale)
    rois = np.concatenate([rois, limit_grid(special_rois(n, h, w, scale), scale, ph, pw)])
    if not isinstance(claims, dict):
        claims = {sr: claims for sr in srs}
    return Case(name, n, c, h, w, scale, ph, pw, tuple(srs), rois, claims, frozenset(cells))


def check_safe(case):
    """The safety condition of every table: grids <= 16 on finite RoIs, non-finite RoIs are empty for ``make_geom``."""
    for sr in case.srs:
        assert R.max_grid(case.rois, case.scale, case.ph, case.pw, sr) <= 16, (case.name, sr)
        for roi in case.rois:
            if not np.all(np.isfinite(roi)):
                assert R.roi_window(roi, case.scale, case.n, case.h, case.w, case.ph, case.pw, sr) is None, (case.name, roi)


@functools.lru_cache(maxsize=None)
def feature_map(seed, n, c, h, w):
    x = np.random.default_rng(seed).standard_normal((n, c, h, w)).astype(_f)
    x.setflags(write=False)
    return x


def case_map(case):
    return feature_map(len(case.name) + case.c, case.n, case.c, case.h, case.w)


def kept(case):
    """RoIs the oracle may be given: finite, image id in [0, n) (it checks neither)."""
    rois = case.rois
    return np.all(np.isfinite(rois), axis=1) & (rois[:, 0] >= 0) & (rois[:, 0] < case.n)


def oracle_bins(oracle_mod, case, x, sr):
    """The oracle's float32 forward on the kept RoIs, exact zeros for the others: [R, C, PH, PW] float32."""
    keep = kept(case)
    out = np.zeros((case.rois.shape[0], x.shape[1], case.ph, case.pw), dtype=_f)
    out[keep] = oracle_mod.roi_align_forward(torch.tensor(x), torch.from_numpy(case.rois[keep]), case.scale, case.ph, case.pw,
                                             sr).numpy()
    return out


def reference(case, sr, stride=1, x=None, key=None):
    """The fp64 reference of a case, computed once and shared (never modified)."""
    key = (case.name, case.c, sr, stride, key)
    if key not in _REF:
        _REF[key] = R.roi_align_forward_ref(case_map(case) if x is None else x, case.rois, case.scale, case.ph, case.pw, sr, stride)
        assert _REF[key].clearance >= 4.0, (key, _REF[key].clearance)
    return _REF[key]


def pair_rows(bins_nhwc):
    """[rows, C] float32 -> the pair rows as uint16 bit patterns: per 32 channels bf16_rne(v) x 32 | bf16_rne(v - hi) x 32."""
    v = np.ascontiguousarray(bins_nhwc, dtype=_f).reshape(-1, bins_nhwc.shape[-1])
    hi = R._bf16(v)
    lo = R._bf16(v - hi)
    bits = lambda a: (a.view(np.uint32) >> 16).astype(np.uint16).reshape(v.shape[0], -1, 32)
    return np.concatenate([bits(hi), bits(lo)], axis=2).reshape(v.shape[0], -1)


# ------------------------------------------------------------------ A: case tables of the exact kernel
BATCHES = {31: {"tab16", "tab8", "tab4", "tail2", "tail1"}, 33: {"tab16", "tail1"}, 1: {"tail1"}, 2: {"tail2"},
           3: {"tail2", "tail1"}, 5: {"tab4", "tail1"}, 7: {"tab4", "tail2", "tail1"}}
BUDGET_WINDOWS = [(16, 17), (17, 17), (16, 34), (17, 34), (32, 34), (33, 34), (64, 34), (64, 35), (64, 68)]
EXACT = ([f"channels-c{c}-p{p}" for c in (31, 33, 1, 2, 3, 5) for p in (14, 7)] +
         ["grids", "p14-sr5", "p17x17", "p1x16", "p16x1", "p3x5", "p7x14", "budget-64x68-c3", "budget-64x68-c19", "budget-65x68-c3",
          "scale-1/4", "scale-1/32", "scale-1", "scale-0.3"])


@functools.lru_cache(maxsize=None)
def exact_case(name):
    kind = name.split("-")[0]
    if kind == "channels":
        c, p = int(name.split("-")[1][1:]), int(name.split("-")[2][1:])
        claims = BATCHES[c] | {"empty"} | ({"pow2", "div"} if c >= 4 else set())
        return make_case(name, 2, c, 25, 42, p, p, (0,), base_rois(100 * c + p, 2, 25, 42, 12), claims)
    if kind == "grids":  # a RoI of 2.6 x 4.5 cells per bin: adaptive grids 3 and 5
        rois = np.concatenate([base_rois(7, 2, 25, 42, 12), np.array([box(0, 2.7, 2.7 + 2.6 * 7, 3.3, 3.3 + 4.5 * 7)], dtype=_f)])
        claims = {0: {"grid3", "grid5", "pow2", "div", "tab4", "tail1"}, 1: {"pow2", "grid1"}, 2: {"pow2", "grid2"},
                  3: {"div", "grid3"}, 4: {"pow2", "grid4"}}
        return make_case(name, 2, 5, 25, 42, 7, 7, (0, 1, 2, 3, 4), rois, claims)
    if kind == "p14":    # 14 * 5 = 70 table entries > 64: the per-lane forms
        return make_case(name, 2, 31, 25, 42, 14, 14, (5,), base_rois(145, 2, 25, 42, 12), {"lane16", "lane8", "lane4", "tail2", "tail1", "div"})
    if kind == "p17x17":  # 289 bins > 256: no tables, two passes of the bin loop
        return make_case(name, 2, 7, 25, 42, 17, 17, (0, 2), base_rois(17, 2, 25, 42, 12),
                         {0: {"lane4", "tail2", "tail1", "pow2", "div"}, 2: {"lane4", "tail2", "tail1", "pow2"}})
    if kind in ("p1x16", "p16x1", "p3x5", "p7x14"):
        ph, pw = map(int, kind[1:].split("x"))
        return make_case(name, 2, 7, 25, 42, ph, pw, (0, 2), base_rois(16 * ph + pw, 2, 25, 42, 12), {0: BATCHES[7], 2: BATCHES[7] | {"pow2"}})
    if kind == "budget":
        h, w = map(int, name.split("-")[1].split("x"))
        c = int(name.split("-")[2][1:])
        rois = [win_roi(0, (3 * k) % (h - ny + 1), ny, (5 * k) % (w - nx + 1), nx) for k, (ny, nx) in enumerate(BUDGET_WINDOWS)]
        rois = np.concatenate([np.array(rois + [win_roi(0, 0, h, 0, w)], dtype=_f), base_rois(h, 1, h, w, 4)])
        if h == 64:
            claims = {"budget16", "budget8", "budget4", "budget2", "budget1", "tail2", "tail1"} | ({"tab16", "tab8", "tab4"} if c == 19 else set())
            cells = (272, 544, 1088, 2176, 4352)
        else:
            claims, cells = {"budget0", "global", "budget1"}, (4420, 4352)
        return make_case(name, 1, c, h, w, 14, 14, (0,), rois, claims, cells=cells)
    if kind == "scale":
        scale = {"1/4": 0.25, "1/32": 1.0 / 32, "1": 1.0, "0.3": 0.3}[name.split("-")[1]]
        return make_case(name, 2, 5, 25, 42, 7, 7, (0, 2), base_rois(int(1000 * scale), 2, 25, 42, 12, scale), {0: BATCHES[5], 2: BATCHES[5]}, scale)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def immunity_case():
    """RoIs of 2 .. 8 cells a side inside the 25 x 42 map: most of the map lies outside every window."""
    g = np.random.default_rng(11)
    r = 10
    sw, sh = g.random(r) * 6 + 2, g.random(r) * 6 + 2
    x1, y1 = g.random(r) * (42 - 9), g.random(r) * (25 - 9)
    rois = np.array([box(k % 2, y1[k], y1[k] + sh[k], x1[k], x1[k] + sw[k]) for k in range(r)], dtype=_f)
    return make_case("nan-outside-windows", 2, 5, 25, 42, 7, 7, (0, 2), rois, {0: {"tab4", "tail1"}, 2: {"tab4", "tail1"}})


def outside_windows(case):
    """[n, h, w] bool: cells lying more than one cell outside every RoI's window (any sampling ratio of the case)"""
    far = np.ones((case.n, case.h, case.w), dtype=bool)
    for roi in case.rois:
        for sr in case.srs:
            win = R.roi_window(roi, case.scale, case.n, case.h, case.w, case.ph, case.pw, sr)
            if win is not None:
                far[int(roi[0]), max(win[0] - 1, 0):win[1] + 2, max(win[2] - 1, 0):win[3] + 2] = False
    return far


# ------------------------------------------------------------------ B: case tables of the matrix-core kernel
TAIL_PW = (1, 2, 3, 4, 5, 6, 7, 8, 13, 16)
TAIL_PH = (1, 7, 16)
BLOCK_SHAPES = {(1, 1), (1, 2), (2, 1), (2, 2), (3, 2), (2, 3), (4, 6)}
MFMA_MAPS = [(16, 16), (16, 84), (50, 16), (17, 33)]
MFMA_CHANNELS = (1, 3, 4, 5, 63, 64, 65, 130)
SENTINEL_PW = (1, 3, 5, 6, 13)


@functools.lru_cache(maxsize=None)
def tail_case(ph, pw):
    return make_case(f"tail-{ph}x{pw}", 2, 5, 50, 84, ph, pw, (0, 2), base_rois(50 * ph + pw, 2, 50, 84, 8), set())


@functools.lru_cache(maxsize=None)
def block_case():
    h, w = 50, 84
    rois = np.array([box(0, 20.3, 30.1, 17.2, 26.9), box(1, 5.3, 14.9, 30.2, 50.7), box(0, 10.4, 31.2, 60.3, 70.1),
                     box(1, 3.2, 23.9, 8.4, 29.1), box(0, 1.2, h - 8.5, 40.4, 60.7), box(1, 12.3, 33.1, 20.2, 61.6),
                     box(0, 0.0, h - 1.0 / 16, 0.0, w - 1.0 / 16),                      # the whole map: 4 x 6 blocks
                     box(1, h - 12.3, h + 2.0, w - 20.6, w + 3.0),                      # 1 x 2, both last blocks pulled back
                     box(0, h - 30.4, h - 0.5, w - 40.3, w - 0.5)], dtype=_f)           # 2 x 3 ending on the last row and column
    return make_case("blocks", 2, 5, h, w, 14, 14, (0, 2), rois, BLOCK_SHAPES | {"pulled-back-rows", "pulled-back-columns"})


def block_forms(case, sr):
    forms = set()
    for roi in case.rois:
        win = R.roi_window(roi, case.scale, case.n, case.h, case.w, case.ph, case.pw, sr)
        if win is None:
            continue
        nyb, nxb = R.block_shape(win)
        forms.add((nyb, nxb))
        if win[1] == case.h - 1 and win[0] + 16 * nyb > case.h:
            forms.add("pulled-back-rows")
        if win[3] == case.w - 1 and win[2] + 16 * nxb > case.w:
            forms.add("pulled-back-columns")
    return forms


@functools.lru_cache(maxsize=None)
def map_case(h, w, ph=14, pw=14):
    return make_case(f"map-{h}x{w}-p{ph}x{pw}", 2, 5, h, w, ph, pw, (0, 2), base_rois(h * w, 2, h, w, 8), set())


@functools.lru_cache(maxsize=None)
def channel_case(c):
    return make_case(f"mfma-channels-{c}", 2, c, 25, 42, 7, 7, (0,), base_rois(c, 2, 25, 42, 8), set())


ONEHOT_CELLS = [(0, 24, 21), (1, 9, 40), (0, 0, 0), (1, 49, 83), (0, 15, 16), (1, 16, 47)]   # (image, row, column) on 50 x 84


# ------------------------------------------------------------------ C: case tables of the strided poolers
STATES = ("none", "first", "last", "same", "diff")
# ((ph, pw), bin stride, sampling ratio)
STRIDED_ALL = [((14, 14), 2, 2), ((14, 14), 2, 0), ((14, 14), 2, 1), ((14, 14), 2, 3), ((14, 14), 1, 2), ((14, 14), 3, 2),
               ((7, 7), 2, 2), ((14, 14), 14, 2), ((7, 14), 2, 2)]
STRIDED_FEW = [((14, 14), 2, 2), ((14, 14), 2, 0), ((7, 14), 2, 2)]
STRIDED_CHANNELS = {32: STRIDED_ALL, 64: STRIDED_FEW, 96: STRIDED_FEW, 8: STRIDED_ALL, 36: STRIDED_FEW}
WINDOW_CLASSES = ("empty", "<= 136", "137-272", "> 272")


def _axis_recipes(p, size):
    """(start, end) in cells of six RoI extents along one axis of ``p`` bins: bins of 0.37 cells (both samples of a bin in one
    cell pair almost everywhere) and of 1.5 cells (mixed), hanging over the low border (the border -1 between the two
    samples of bin 2: bins 0, 1 are outside, bin 2 has only its last sample), hanging over the high border (the border
    ``size`` between the two samples of the last even bin before p - 1), and inside the map."""
    hi = (p - 2) // 2 * 2
    out = []
    for b in (0.37, 1.5):
        for start in (-1.0 - 2.5 * b, size - (2 * hi + 1) * b / 2, 0.4 * size + 0.13):
            out.append((start, start + p * b))
    return out


@functools.lru_cache(maxsize=None)
def strided_case(ph, pw):
    h, w = 50, 84
    rois = [box((i + j) % 2, y0, y1, x0, x1) for i, (y0, y1) in enumerate(_axis_recipes(ph, h)) for j, (x0, x1) in enumerate(_axis_recipes(pw, w))]
    rois += [win_roi(0, 7, 10, 30, 20), win_roi(1, 20, 14, 11, 19), win_roi(0, 3, 30, 6, 40),   # 200 and 266 cells; 1200
             box(1, h + 300.0, h + 310.0, w + 300.0, w + 310.0)]                                  # outside the map: empty
    return make_case(f"strided-{ph}x{pw}", 2, 0, h, w, ph, pw, (0, 1, 2, 3), np.array(rois, dtype=_f), set())


def window_classes(case, sr):
    cells = R._window_cells(case.rois, case.scale, case.n, case.h, case.w, (case.ph, case.pw), sr)
    return {"empty": int((cells == 0).sum()), "<= 136": int(((cells > 0) & (cells <= 136)).sum()),
            "137-272": int(((cells > 136) & (cells <= 272)).sum()), "> 272": int((cells > 272).sum())}


def all_cases():
    """(section, case) of every table of this file, for the host checks of tests/test_roi_align_reference.py"""
    for name in EXACT:
        yield "A", exact_case(name)
    yield "A", immunity_case()
    for pw in TAIL_PW:
        for ph in TAIL_PH:
            if ph != pw:
                yield "B", tail_case(ph, pw)
    yield "B", block_case()
    for h, w in MFMA_MAPS:
        yield "B", map_case(h, w)
    yield "B", map_case(20, 9)
    yield "B", map_case(25, 42, 17, 17)
    for c in MFMA_CHANNELS:
        yield "B", channel_case(c)
    for p in sorted({p for combos in STRIDED_CHANNELS.values() for p, _, _ in combos}):
        yield "C", strided_case(*p)


# ------------------------------------------------------------------ device helpers
def _dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


def _channels_last(x):
    """Same values and shape, NHWC memory: what the trunk hands to the poolers."""
    return x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _lib():
    from cvpr22_cross_modal_pseudo_labeling_amd import _lib

    return _lib


def _report(section, name, ratio):
    print(f"roi_align_forward {section} {name}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0, (section, name, ratio)


def _check_exact(oracle_mod, case, sr):
    """Bit-equal to the oracle (exact zeros for foreign ids and non-finite RoIs), within the fp32 bound of the reference."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    x = case_map(case)
    want = oracle_bins(oracle_mod, case, x, sr)
    got = _C.roi_align_forward(_dev(x), _dev(case.rois), case.scale, case.ph, case.pw, sr).cpu().numpy()
    assert np.array_equal(got, want), (case.name, sr, np.argwhere(got != want)[:6])
    assert not got[~kept(case)].any()
    res = reference(case, sr)
    return R.worst_ratio(got, res, R.f32_forward_bound(res))


def _check_mfma(case, sr, x=None, key=None):
    """Within TOL_MFMA * mag + slack element by element (exact zeros where there is no bound), two runs bit-identical."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    assert _lib().load().ovis_roi_align_forward_mfma_supported(case.h, case.w, case.ph, case.pw) == 1
    x = case_map(case) if x is None else x
    got = _C.roi_align_forward_mfma(_dev(x), _dev(case.rois), case.scale, case.ph, case.pw, sr)
    assert torch.equal(got, _C.roi_align_forward_mfma(_dev(x), _dev(case.rois), case.scale, case.ph, case.pw, sr)), "not reproducible"
    got = got.cpu().numpy()
    empty = [R.roi_window(roi, case.scale, case.n, case.h, case.w, case.ph, case.pw, sr) is None for roi in case.rois]
    assert not got[np.array(empty)].any(), "foreign-id, non-finite and out-of-map RoIs pool to exact zeros"
    res = reference(case, sr, x=x, key=key)
    return R.worst_ratio(got, res, R.mfma_forward_bound(res)), got


# ------------------------------------------------------------------ A: exact kernel
@pytest.mark.parametrize("name", EXACT)
def test_exact_kernel_forms(oracle_mod, name):
    """Every dispatch form of ``roi_align_fwd_kernel`` its table claims (checked on the host first)."""
    case = exact_case(name)
    check_safe(case)
    worst = 0.0
    for sr in case.srs:
        forms = R.exact_forms(case.rois, case.scale, case.n, case.c, case.h, case.w, case.ph, case.pw, sr)
        assert case.claims[sr] <= forms, (name, sr, case.claims[sr] - forms)
        worst = max(worst, _check_exact(oracle_mod, case, sr))
    _report("A", name, worst)


def test_exact_kernel_reads_only_its_windows(oracle_mod):
    """NaN in every cell more than one cell outside every RoI's window of that image: no bit of the result changes (a tap
    address off by more than the window's rim would fetch one)."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    case = immunity_case()
    check_safe(case)
    far = outside_windows(case)
    assert far.sum() > far.size // 4, "most of the map must lie outside the windows"
    x = case_map(case)
    poisoned = x.copy()
    poisoned[np.broadcast_to(far[:, None], x.shape)] = np.nan
    worst = 0.0
    for sr in case.srs:
        worst = max(worst, _check_exact(oracle_mod, case, sr))
        clean = _C.roi_align_forward(_dev(x), _dev(case.rois), case.scale, case.ph, case.pw, sr)
        got = _C.roi_align_forward(_dev(poisoned), _dev(case.rois), case.scale, case.ph, case.pw, sr)
        assert not torch.isnan(got).any() and torch.equal(got, clean), sr
    _report("A", case.name, worst)


# ------------------------------------------------------------------ B: matrix-core kernel
@pytest.mark.parametrize("pw", TAIL_PW)
def test_mfma_tail_stores(pw):
    """PW % 4 = 0 (no tail), 1 (dword), 2 (dwordx2), 3 (dwordx3), PW < 4 (tail only); NST = 2 for PW = 5, 6, 7, 13, else 1."""
    worst = 0.0
    for ph in TAIL_PH:
        if ph == pw:
            continue
        case = tail_case(ph, pw)
        check_safe(case)
        for sr in case.srs:
            ratio, _ = _check_mfma(case, sr)
            assert ratio <= 1.0, (ph, pw, sr, ratio)
            worst = max(worst, ratio)
    _report("B", f"tail stores PW = {pw}, PH in {[ph for ph in TAIL_PH if ph != pw]}", worst)


def test_mfma_block_shapes():
    case = block_case()
    check_safe(case)
    worst = 0.0
    for sr in case.srs:
        forms = block_forms(case, sr)
        assert case.claims[sr] <= forms, (sr, case.claims[sr] - forms)
        worst = max(worst, _check_mfma(case, sr)[0])
    _report("B", "block shapes 1x1 .. 4x6", worst)


@pytest.mark.parametrize("hw", MFMA_MAPS, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_mfma_maps(hw):
    """Maps of exactly one block a side (every block origin is 0), one block in one direction, and sizes that are no multiple
    of 16 (17 x 33: the last blocks are pulled back by 15)."""
    case = map_case(*hw)
    check_safe(case)
    _report("B", case.name, max(_check_mfma(case, sr)[0] for sr in case.srs))


@pytest.mark.parametrize("shape", [(20, 9, 14, 14), (25, 42, 17, 17)], ids=["20x9", "p17x17"])
def test_mfma_unsupported_shapes_fall_back_to_the_exact_kernel(shape):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    case = map_case(*shape)
    check_safe(case)
    assert _lib().load().ovis_roi_align_forward_mfma_supported(case.h, case.w, case.ph, case.pw) == 0
    x, rois = _dev(case_map(case)), _dev(case.rois)
    for sr in case.srs:
        assert torch.equal(_C.roi_align_forward_mfma(x, rois, case.scale, case.ph, case.pw, sr),
                           _C.roi_align_forward(x, rois, case.scale, case.ph, case.pw, sr)), sr


@pytest.mark.parametrize("c", MFMA_CHANNELS)
def test_mfma_channels(c):
    """Waves without a channel (C < 4), a partial slab (63, 65 - 64, 130 - 128) and three slabs."""
    case = channel_case(c)
    check_safe(case)
    _report("B", case.name, _check_mfma(case, 0)[0])


@pytest.mark.parametrize("pw", SENTINEL_PW)
def test_mfma_writes_only_its_tiles(pw):
    """The C entry point on an output placed inside a larger tensor the test owns: 64 sentinel floats before it and 64 after it
    stay untouched, and the tiles equal the wrapper's."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    case = tail_case(7, pw)
    check_safe(case)
    L = _lib().load()
    x, rois = _dev(case_map(case)), _dev(case.rois)
    r, numel = case.rois.shape[0], case.rois.shape[0] * case.c * case.ph * case.pw
    nbytes = L.ovis_roi_align_forward_workspace_bytes(r, case.h, case.w)
    ws = torch.empty((max(nbytes, 1),), dtype=torch.uint8, device="cuda")
    for sr in case.srs:
        want = _C.roi_align_forward_mfma(x, rois, case.scale, case.ph, case.pw, sr)
        buf = torch.full((numel + 128,), -7777.0, dtype=torch.float32, device="cuda")
        rc = L.ovis_roi_align_forward_ws_f32(x.data_ptr(), rois.data_ptr(), buf.data_ptr() + 64 * 4, r, case.n, case.c, case.h, case.w,
                                             case.ph, case.pw, case.scale, sr, ws.data_ptr(), nbytes,
                                             torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert bool((buf[:64] == -7777.0).all()) and bool((buf[-64:] == -7777.0).all()), (pw, sr)
        assert torch.equal(buf[64:-64].view_as(want), want), (pw, sr)


def test_mfma_onehot_maps():
    """x = 1.0 (exact in bf16) at one cell of channel 1: the output is that cell's weight in every bin that reaches it, within
    the bound, and exactly zero in every bin without a bound (the other channels, the other image's RoIs, far bins)."""
    case = block_case()
    check_safe(case)
    worst = 0.0
    for b, y, xc in ONEHOT_CELLS:
        x = np.zeros((case.n, 3, case.h, case.w), dtype=_f)
        x[b, 1, y, xc] = 1.0
        ratio, got = _check_mfma(case, 0, x=x, key=(b, y, xc))
        res = reference(case, 0, x=x, key=(b, y, xc))
        assert ratio <= 1.0, ((b, y, xc), ratio)
        assert res.mag.max() > 0 and not got[:, [0, 2]].any() and not got[case.rois[:, 0] != b].any()
        assert np.count_nonzero(R.mfma_forward_bound(res) == 0) > res.mag.size // 2
        worst = max(worst, ratio)
    _report("B", "one-hot maps", worst)


# ------------------------------------------------------------------ C: strided NHWC poolers
@pytest.mark.parametrize("c", list(STRIDED_CHANNELS))
def test_strided_nhwc_poolers(oracle_mod, c):
    """fp32 bins bit-equal to the oracle's bins (s i, s j) and within the fp32 bound of the reference at that stride; pair rows
    (C % 32 == 0) equal to bf16 hi | lo rows built in NumPy from the oracle's bins."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    worst = 0.0
    for (ph, pw), s, sr in STRIDED_CHANNELS[c]:
        case = strided_case(ph, pw)._replace(c=c)
        check_safe(case)
        classes = window_classes(case, sr)
        assert all(classes.values()), (ph, pw, sr, classes)
        if (ph, pw, sr) == (14, 14, 2) and s in (1, 2):
            states = R.shared_tap_states(case.rois, case.scale, case.n, case.h, case.w, ph, pw, s)
            assert states == {(a, b) for a in STATES for b in STATES}, (s, sorted(states))
        x = case_map(case)
        x_cl = _channels_last(_dev(x))
        assert not x_cl.is_contiguous() or c == 1
        rois = _dev(case.rois)
        want = np.ascontiguousarray(oracle_bins(oracle_mod, case, x, sr)[:, :, ::s, ::s].transpose(0, 2, 3, 1))
        got = _C.roi_align_forward_strided_nhwc(x_cl, rois, case.scale, ph, pw, sr, s).cpu().numpy()
        assert np.array_equal(got, want), ((ph, pw), s, sr, np.argwhere(got != want)[:6])
        assert not got[~kept(case)].any()
        res = reference(case, sr, s)
        ratio = R.worst_ratio(got.transpose(0, 3, 1, 2), res, R.f32_forward_bound(res))
        assert ratio <= 1.0, ((ph, pw), s, sr, ratio)
        worst = max(worst, ratio)
        if c % 32 == 0:
            pair, shp = _C.roi_align_forward_strided_pair(x_cl, rois, case.scale, ph, pw, sr, s)
            assert shp == want.shape[1:3]
            rows = pair.view(torch.int16).cpu().numpy().view(np.uint16)
            expect = pair_rows(want)
            assert rows.shape == expect.shape and np.array_equal(rows, expect), ((ph, pw), s, sr, np.argwhere(rows != expect)[:6])
            dead = np.repeat(~kept(case), want.shape[1] * want.shape[2])
            assert not rows[dead].any(), "foreign-id and NaN RoIs: zeros in both halves of a pair row"
    _report("C", f"strided poolers C = {c}", worst)


def test_strided_entry_point_refusals():
    """A base pointer that is not 16-byte aligned, and pair rows with C % 32 != 0: OVIS_ERANGE, nothing launched."""
    lib = _lib()
    L = lib.load()
    x = torch.zeros((2 * 8 * 8 * 8 + 4,), dtype=torch.float32, device="cuda")
    rois = _dev(np.array([box(0, 1.0, 5.0, 1.0, 5.0)], dtype=_f))
    out = torch.zeros((7 * 7 * 8 * 2,), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    args = (1, 2, 8, 8, 8, 14, 14, 2, S, 2)
    assert L.ovis_roi_align_forward_strided_from_nhwc_f32(x.data_ptr(), rois.data_ptr(), out.data_ptr(), *args, 0, stream) == 0
    assert L.ovis_roi_align_forward_strided_from_nhwc_f32(x.data_ptr() + 4, rois.data_ptr(), out.data_ptr(), *args, 0, stream) == lib.OVIS_ERANGE
    assert L.ovis_roi_align_forward_strided_from_nhwc_f32(x.data_ptr(), rois.data_ptr(), out.data_ptr() + 4, *args, 0, stream) == lib.OVIS_ERANGE
    assert L.ovis_roi_align_forward_strided_from_nhwc_f32(x.data_ptr(), rois.data_ptr(), out.data_ptr(), *args, 1, stream) == lib.OVIS_ERANGE
    torch.cuda.synchronize()
