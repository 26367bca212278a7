"""GPU: every form of the RoIAlign backward (csrc/roi_align_bwd_plane.hip: plan kernel, tile re-layout kernel, the seven
``roi_bwd_mfma_kernel`` instantiations; csrc/roi_align.hip: the two atomic fallbacks) against the independent fp64
reference tests/roi_align_reference.py (pinned by tests/test_roi_align_reference.py), elementwise and without a floor:

    |got - ref| <= TOL * mag + slack            exact zeros wherever mag == 0 and slack == 0

``mag`` = sum weight * |grad|, ``slack`` = what K_ULPS = 3 float32 ulps on every sample coordinate may move (derived in the
reference's docstring from ``sample_coord`` / ``axis_weight``).  Matrix-core forms: TOL = 4e-5 = 2 x the single-product constant
2e-5 (``split_bf16`` keeps a value to 2^-16, ``mfma3`` drops lo.lo <= 2^-16 |a||b|: three sources per product plus its fp32
accumulation; two chained products with T re-split in between -- written out at ``TOL_MFMA``).  Atomic forms: fp32 summation,
(terms + 4) * 2^-24 * mag + slack (derived at ``ATOMIC_C``).  Every case asserts ``clearance >= 4`` on the host before it
launches anything (tests/test_roi_align_reference.py checks the whole case table without a GPU); no case is skipped.

Which kernel a case reaches (``plane_waves``: 8 planes if 8 * 4HW <= 160 KB - 24 KB = 139264 B, i.e. HW <= 4352 cells, else 4
if 4 * 4HW <= 139264, HW <= 8704; FIT = both sides >= 16; WC = 84 only for width 84):
  A  50x84 (4200) <8,true,84>;  40x56 (2240) <8,true,0>
  B  50x84 <8,true,84>;  40x56 <8,true,0>;  13x17 (221, height < 16) and 20x9 (180, width < 16) <8,false,0>;  5x7 <8,false,0>
     masked in both directions;  70x100 = 7000 cells, 28000 B a plane: 8 planes 224000 B > 139264, 4 planes 112000 B fit:
     <4,true,0>;  12x400 = 4800 cells, 19200 B: 8 planes 153600 B > 139264, 4 planes 76800 B, height 12 < 16: <4,false,0>
  C, D  50x84 <8,true,84>
  E  strided: tiles of ceil(P / s) >= 4 columns on 50x84 <8,true,84> and 25x42 <8,true,0>; NHWC: tiles <= 8x8 on maps >= 16x16
     with HW <= 4352: <8,true,84,SMALL> (width 84) / <8,true,0,SMALL> (30x40, 16x16)
  F  LDS atomic form needs PH*H + PW*W + 2(H+W) + 16*PH*PW <= 16384 floats (64 KB): (2,2) on 25x42: 50+84+134+64 = 332;
     (7,3) on 25x42: 175+126+134+336 = 771 (both refused by the plane kernel: pooled_w < 4); 14x14 on 120x100 (12000 cells
     > 8704): 1680+1400+440+3136 = 6656.  Scatter form: 32x32 on 20x24: 640+768+88+16384 = 17880 > 16384; 28x28 on 50x84:
     1400+2352+268+12544 = 16564 > 16384 (poolers above 16 are refused by the plane kernel).

Coverage before this file: no test reached ``roi_bwd_mfma_kernel<4, true, 0>`` or ``<4, false, 0>`` -- every backward
shape in tests/ was 50x84 (4200 cells) or smaller, except 120x100 which the plane kernel refuses -- and none reached
``roi_align_bwd_scatter_kernel`` (the one fallback test, 14x14 on 120x100, is the LDS form) or a pooler narrower than 4.

The strided NCHW form (three hi/lo terms, gradient split in the kernel) and the NHWC form (four terms, gradient pre-split)
are not defined to agree bit for bit: both are compared to the reference.

Largest measured error / bound per section on an MI355X (every test prints its own; run with ``-s``):
  A  one-hot footprints          0.21   (both maps; every cell outside the footprint exactly zero)
  B  plane-kernel instantiations 0.51   (20x9; 70x100 <4,true,0> 0.35, 12x400 <4,false,0> 0.21, the others 0.18 .. 0.35)
  C  pooler shapes               0.47   (2x5; the others 0.38 .. 0.47)
  D  list shapes                 0.26   (257 RoIs; foreign ids only: exactly zero; all bit-reproducible and exact under 2^+-20)
  E  strided NCHW tiles          0.69   (8x5 tiles on the 16x16 map; 4x4 tiles 0.57, 7x7 0.49, the others 0.19 .. 0.44)
     strided NHWC tiles (SMALL)  0.40   (4x4 and 8x5 tiles; the others 0.23 .. 0.33)
  F  atomic LDS form             0.26   (7x3; 2x2 0.09, 14x14 on 120x100 0.16)
     atomic scatter form         0.14   (28x28 on 50x84; 32x32 on 20x24 0.04)
Three figures lie above one half (B 20x9 0.51, E 4x4 tiles 0.57, E 8x5 tiles 0.69), all of the three-term form and all on cells
that one to six terms reach (clamped border cells, tiles of a few bins): nothing averages there.  They are the hi/lo
algorithm, not the kernel: ``roi_align_reference.split_form_emulation`` -- bf16 hi + lo operands, three terms, T re-split,
on the reference's own weights -- gives 0.508 / 0.569 / 0.686 on the same cases on the CPU (printed by
tests/test_roi_align_reference.py), the kernels measure 0.509 / 0.569 / 0.686 with the same worst cells, and the four-term
emulation gives the SMALL form's 0.40.  The re-derivation at ``TOL_MFMA``: bf16's unit roundoff is 2^-8, one error source is
at most 2^-16 = 1.5e-5, six sources in the chain, worst case 9.2e-5; TOL = 4e-5 is the project's constant for independent
roundings, and 0.69 of it is 0.30 of the worst case.
"""
import functools

import numpy as np
import pytest
import torch

from tests import roi_align_reference as R

pytestmark = pytest.mark.gpu

S = R.SCALE
_REF = {}


def _px(cells):
    return [16.0 * v for v in cells]


def _ref(name, grad, rois, ph, pw, n, c, h, w, sr, stride=1):
    """The reference of a case, computed once and shared (never modified)."""
    if name not in _REF:
        _REF[name] = R.roi_align_backward_ref(grad, rois, S, ph, pw, n, c, h, w, sr, stride)
        assert _REF[name].clearance >= 4.0, (name, _REF[name].clearance)
    return _REF[name]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _lib():
    from cvpr22_cross_modal_pseudo_labeling_amd import _lib

    return _lib.load()


def _backward(grad, rois, ph, pw, n, c, h, w, sr):
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    return _C.roi_align_backward(_dev(grad), _dev(rois), S, ph, pw, n, c, h, w, sr)


def _report(section, name, form, ratio):
    print(f"roi_align_backward {section} {name} [{form}]: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0, (section, name, ratio)


# ------------------------------------------------------------------ case tables (host only: NumPy, no GPU at import)
@functools.lru_cache(maxsize=None)
def onehot_rois(h, w):
    """One RoI inside a single 16-cell block, one spanning 3 x 2 blocks (3 row blocks: the reuse flag is on), one whose
    window ends at the map's last row and column (its last blocks' origins are pulled back)."""
    rois = np.array([[0] + _px([20.3, 17.2, 30.1, 26.9]),
                     [1] + _px([10.4, 1.2, 36.7, h - 1.5]),
                     [1] + _px([w - 20.6, h - 12.3, w + 3.0, h + 2.0])], dtype=np.float32)
    return R.cleared(rois, 14, 14, 2, h, w)


ONEHOT_BINS = [(0, 0), (0, 13), (13, 0), (13, 13), (13, 9), (13, 10), (7, 7)]
ONEHOT_MAPS = {(50, 84): "<8,true,84>", (40, 56): "<8,true,0>"}

PLANE_MAPS = [((50, 84), "<8,true,84>"), ((40, 56), "<8,true,0>"), ((13, 17), "<8,false,0> low"), ((20, 9), "<8,false,0> narrow"),
              ((5, 7), "<8,false,0> both"), ((70, 100), "<4,true,0>"), ((12, 400), "<4,false,0>")]


@functools.lru_cache(maxsize=None)
def plane_case(h, w):
    rois = np.concatenate([R.random_rois(100 + h, 24, 2, h, w, 4.0, 16.0 * max(min(h, w), min(max(h, w), 100))),
                           R.edge_rois(h, w)])
    return R.cleared(rois, 14, 14, 2, h, w), R.dense_grad(200 + w, 31, 9, 14, 14)


POOLERS = [(1, 4), (16, 16), (14, 14), (7, 7), (5, 6), (3, 13), (2, 5)]
RATIOS = (0, 1, 2, 3)


@functools.lru_cache(maxsize=None)
def pooler_case(ph, pw):
    big = [0] + _px([3.3, 2.7, 3.3 + 2.6 * pw, 2.7 + 2.6 * ph])  # ceil(2.6) = 3: the division path of make_geom
    rois = R.recipe(300 + 16 * ph + pw, 2, 50, 84, ph, pw, 16, RATIOS, [big])
    return rois, R.dense_grad(400 + ph, rois.shape[0], 3, ph, pw)


def small_rois(seed, ids):
    """RoIs of 2 .. 12 cells a side anywhere inside the 50 x 84 map: a window of at most 14 cells, one block, one item."""
    g = np.random.default_rng(seed)
    r = len(ids)
    sw, sh = g.random(r) * 10 + 2, g.random(r) * 10 + 2
    x1, y1 = g.random(r) * (84 - 13), g.random(r) * (50 - 13)
    rois = np.stack([np.asarray(ids, dtype=np.float64), 16 * x1, 16 * y1, 16 * (x1 + sw), 16 * (y1 + sh)], 1).astype(np.float32)
    return R.cleared(rois, 14, 14, 1 << 20, 50, 84)  # every id counts as in range here: foreign RoIs are cleared too


@functools.lru_cache(maxsize=None)
def list_cases():
    counts = [9, 0, 17, 1, 8, 16, 7]
    by_count = [i for i, k in enumerate(counts) for _ in range(k)]
    np.random.default_rng(5).shuffle(by_count)
    whole = np.array([[0, 0.0, 0.0, 16.0 * 84 - 1.0, 16.0 * 50 - 1.0]] * 9, dtype=np.float32)
    return {"counts-9-0-17-1-8-16-7": (7, small_rois(1, by_count)),
            "middle-image-empty": (3, small_rois(2, [2, 0, 0, 2, 2, 0, 2, 0, 0])),
            "foreign-ids-only": (2, small_rois(3, [2, -1, 7, 2, 300])),
            "257-unsorted": (3, small_rois(4, [(7 * i + i // 5) % 3 for i in range(257)])),
            "513-unsorted": (3, small_rois(5, [(5 * i + i // 7) % 3 for i in range(513)])),
            "whole-map-x9": (1, R.cleared(whole, 14, 14, 1, 50, 84))}


# (name, (h, w), pooler, stride, channels, expected: True = accepted, False = None)
STRIDED = [("p14-s2", (50, 84), 14, 2, 5, True), ("p14-s3", (50, 84), 14, 3, 5, True), ("p28-s2", (50, 84), 28, 2, 5, True),
           ("p7-s2", (25, 42), 7, 2, 5, True), ("p28-s2-small-map", (25, 42), 28, 2, 3, True), ("p6-s2", (50, 84), 6, 2, 5, False)]
# (name, (h, w), (ph, pw), stride, channels, accepted)
NHWC = [("8x8-c63", (50, 84), (8, 8), 1, 63, True), ("7x7-c65", (50, 84), (14, 14), 2, 65, True),
        ("1x4-c1", (30, 40), (1, 4), 1, 1, True), ("4x4-c64", (30, 40), (7, 7), 2, 64, True),
        ("8x5-c130", (16, 16), (16, 10), 2, 130, True), ("7x7-c3-w40", (30, 40), (14, 14), 2, 3, True),
        ("low-map", (15, 40), (14, 14), 2, 8, False), ("9x9", (50, 84), (9, 9), 1, 8, False)]


@functools.lru_cache(maxsize=None)
def strided_case(name, h, w, ph, pw, stride, c):
    rois = R.recipe(sum(map(ord, name)), 2, h, w, ph, pw, 12)
    return rois, R.dense_grad(len(name), rois.shape[0], c, -(-ph // stride), -(-pw // stride))


# (name, (n, c, h, w), (ph, pw), sampling ratio, form)
ATOMIC = [("lds-2x2", (2, 3, 25, 42), (2, 2), 0, "lds"), ("lds-7x3", (2, 3, 25, 42), (7, 3), 2, "lds"),
          ("lds-14x14-120x100", (2, 4, 120, 100), (14, 14), 0, "lds"),
          ("scatter-32x32-20x24", (2, 3, 20, 24), (32, 32), 0, "scatter"), ("scatter-28x28-50x84", (2, 3, 50, 84), (28, 28), 0, "scatter")]


@functools.lru_cache(maxsize=None)
def atomic_case(name, n, h, w, ph, pw, c, sr):
    rois = R.recipe(sum(map(ord, name)), n, h, w, ph, pw, 12, (sr,))
    return rois, R.dense_grad(len(name), rois.shape[0], c, ph, pw)


def clearances():
    """(case, clearance) of every case of this file: checked on the CPU by tests/test_roi_align_reference.py."""
    for (h, w) in ONEHOT_MAPS:
        yield f"A-{h}x{w}", R.clearance_of(onehot_rois(h, w), S, 14, 14, 2, h, w, 0)
    for (h, w), _ in PLANE_MAPS:
        yield f"B-{h}x{w}", R.clearance_of(plane_case(h, w)[0], S, 14, 14, 2, h, w, 0)
    for ph, pw in POOLERS:
        for sr in RATIOS:
            yield f"C-{ph}x{pw}-sr{sr}", R.clearance_of(pooler_case(ph, pw)[0], S, ph, pw, 2, 50, 84, sr)
    for name, (n, rois) in list_cases().items():
        yield f"D-{name}", R.clearance_of(rois, S, 14, 14, n, 50, 84, 0)
    for name, (h, w), p, s, c, ok in STRIDED:
        yield f"E-{name}", R.clearance_of(strided_case(name, h, w, p, p, s, c)[0], S, p, p, 2, h, w, 0)
    for name, (h, w), (ph, pw), s, c, ok in NHWC:
        yield f"E-nhwc-{name}", R.clearance_of(strided_case(name, h, w, ph, pw, s, c)[0], S, ph, pw, 2, h, w, 0)
    for name, (n, c, h, w), (ph, pw), sr, _ in ATOMIC:
        yield f"F-{name}", R.clearance_of(atomic_case(name, n, h, w, ph, pw, c, sr)[0], S, ph, pw, n, h, w, sr)


# ------------------------------------------------------------------ A: one-hot gradients pin the enumeration
@pytest.mark.parametrize("hw", list(ONEHOT_MAPS), ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_onehot_footprints(hw):
    """G = 1.0 (exact in bf16) at one (RoI, channel 1, bin): the result is that bin's weight footprint, within the bound
    cell by cell and exactly zero everywhere else -- the other channels, the other image, the other RoIs' windows."""
    h, w = hw
    rois = onehot_rois(h, w)
    assert _lib().ovis_roi_align_backward_plane_supported(h, w, 14, 14) == 1
    worst = 0.0
    for r in range(3):
        for (i, j) in ONEHOT_BINS:
            grad = np.zeros((3, 3, 14, 14), dtype=np.float32)
            grad[r, 1, i, j] = 1.0
            res = _ref(f"A-{h}x{w}-r{r}-{i}-{j}", grad, rois, 14, 14, 2, 3, h, w, 0)
            assert np.count_nonzero(res.mag[:, [0, 2]]) == 0 and np.count_nonzero(res.mag[1 - int(rois[r, 0])]) == 0
            got = _backward(grad, rois, 14, 14, 2, 3, h, w, 0).cpu().numpy()
            ratio = R.worst_ratio(got, res, R.mfma_bound(res))
            assert ratio <= 1.0, (hw, r, (i, j), ratio, np.argwhere(np.abs(got - res.ref) > R.mfma_bound(res))[:6])
            worst = max(worst, ratio)
    _report("A", f"{h}x{w} 3 RoIs x 7 bins", ONEHOT_MAPS[hw], worst)


# ------------------------------------------------------------------ B: every instantiation of the plane kernel
@pytest.mark.parametrize("hw,form", PLANE_MAPS, ids=[f"{h}x{w}" for (h, w), _ in PLANE_MAPS])
def test_plane_kernel_instantiations(hw, form):
    """Dense random G, random RoIs plus the edge RoIs, 9 channels (a partial last channel group for both group sizes)."""
    h, w = hw
    rois, grad = plane_case(h, w)
    assert _lib().ovis_roi_align_backward_plane_supported(h, w, 14, 14) == 1
    res = _ref(f"B-{h}x{w}", grad, rois, 14, 14, 2, 9, h, w, 0)
    got = _backward(grad, rois, 14, 14, 2, 9, h, w, 0).cpu().numpy()
    _report("B", f"{h}x{w}", form, R.worst_ratio(got, res, R.mfma_bound(res)))


# ------------------------------------------------------------------ C: pooler shapes and sampling grids
@pytest.mark.parametrize("pooler", POOLERS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_pooler_shapes(pooler):
    """PW 4 / 5 / 6 (the pulled-back last k-group at every offset), PH 1 and 16, sampling ratios 0 .. 3 and a RoI of 2.6 bins
    per cell whose adaptive grid is 3."""
    ph, pw = pooler
    rois, grad = pooler_case(ph, pw)
    assert _lib().ovis_roi_align_backward_plane_supported(50, 84, ph, pw) == 1
    worst = 0.0
    for sr in RATIOS:
        res = _ref(f"C-{ph}x{pw}-sr{sr}", grad, rois, ph, pw, 2, 3, 50, 84, sr)
        got = _backward(grad, rois, ph, pw, 2, 3, 50, 84, sr).cpu().numpy()
        ratio = R.worst_ratio(got, res, R.mfma_bound(res))
        assert ratio <= 1.0, (pooler, sr, ratio)
        worst = max(worst, ratio)
    _report("C", f"{ph}x{pw} sampling 0-3", "<8,true,84>", worst)


# ------------------------------------------------------------------ D: list shapes
@pytest.mark.parametrize("name", list(list_cases()))
def test_list_shapes(name):
    """One item per RoI: per-image item counts 0, 1, 7, 8, 9, 16, 17 around the rounds of 8, an empty image between two
    others, foreign ids only (every plane exactly zero), 257 / 513 RoIs in unsorted image order (the plan's prefix sum carries
    a base across its chunks of 256), 9 whole-map RoIs of 24 items.  No atomics: two runs are bit-identical, and scaling G by
    2^-20 / 2^20 scales the result exactly (a power of two commutes with the hi/lo split and every fp32 operation)."""
    n, rois = list_cases()[name]
    grad = R.dense_grad(len(name), rois.shape[0], 3, 14, 14)
    res = _ref(f"D-{name}", grad, rois, 14, 14, n, 3, 50, 84, 0)
    if name == "foreign-ids-only":
        assert np.count_nonzero(res.mag) == 0 and np.count_nonzero(res.slack) == 0
    got = _backward(grad, rois, 14, 14, n, 3, 50, 84, 0)
    _report("D", name, "<8,true,84>", R.worst_ratio(got.cpu().numpy(), res, R.mfma_bound(res)))
    assert torch.equal(got, _backward(grad, rois, 14, 14, n, 3, 50, 84, 0)), "not reproducible"
    for k in (-20, 20):
        scaled = _backward(grad * np.float32(2.0 ** k), rois, 14, 14, n, 3, 50, 84, 0)
        assert torch.equal(scaled, got * 2.0 ** k), f"2^{k} * G"


# ------------------------------------------------------------------ E: strided forms
@pytest.mark.parametrize("case", STRIDED, ids=lambda c: c[0])
def test_strided_tiles(case):
    """``roi_align_backward_strided``: [R, C, ceil(P / s), ceil(P / s)] tiles of the bins (s i, s j).  Pooler 28 at stride 2 is
    legal only through its 14 x 14 tiles; pooler 7 at stride 2 has the minimum tile width 4; 3 columns are refused."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    name, (h, w), p, s, c, ok = case
    rois, grad = strided_case(name, h, w, p, p, s, c)
    got = _C.roi_align_backward_strided(_dev(grad), _dev(rois), S, p, p, 2, c, h, w, 0, s)
    if not ok:
        assert got is None
        return
    assert got is not None
    res = _ref(f"E-{name}", grad, rois, p, p, 2, c, h, w, 0, s)
    _report("E", f"strided {name} {h}x{w}", "<8,true,84>" if w == 84 else "<8,true,0>", R.worst_ratio(got.cpu().numpy(), res, R.mfma_bound(res)))


@pytest.mark.parametrize("case", NHWC, ids=lambda c: c[0])
def test_strided_nhwc_small_tiles(case):
    """``roi_align_backward_strided_nhwc`` (pre-split tiles, SMALL kernel): tiles 8x8, 7x7, 1x4, 4x4, 8x5; channels 1, 63, 64, 65,
    130 around the 64-channel groups of the re-layout kernel; widths 84 and 40 and a 16 x 16 map; refused: a 15 x 40 map,
    9 x 9 tiles.  Where the NCHW strided form accepts the shape too, it is held to the same reference."""
    from cvpr22_cross_modal_pseudo_labeling_amd import _C

    name, (h, w), (ph, pw), s, c, ok = case
    rois, grad = strided_case(name, h, w, ph, pw, s, c)
    nhwc = np.ascontiguousarray(grad.transpose(0, 2, 3, 1))
    got = _C.roi_align_backward_strided_nhwc(_dev(nhwc), _dev(rois), S, ph, pw, 2, c, h, w, 0, s)
    if not ok:
        assert got is None
        return
    assert got is not None
    res = _ref(f"E-nhwc-{name}", grad, rois, ph, pw, 2, c, h, w, 0, s)
    form = "<8,true,84,SMALL>" if w == 84 else "<8,true,0,SMALL>"
    _report("E", f"nhwc {name} {h}x{w}", form, R.worst_ratio(got.cpu().numpy(), res, R.mfma_bound(res)))
    assert torch.equal(got, _C.roi_align_backward_strided_nhwc(_dev(nhwc), _dev(rois), S, ph, pw, 2, c, h, w, 0, s))
    nchw = _C.roi_align_backward_strided(_dev(grad), _dev(rois), S, ph, pw, 2, c, h, w, 0, s)
    assert nchw is not None
    _report("E", f"nchw {name} {h}x{w}", form.replace(",SMALL", ""), R.worst_ratio(nchw.cpu().numpy(), res, R.mfma_bound(res)))


# ------------------------------------------------------------------ F: atomic fallbacks
@pytest.mark.parametrize("case", ATOMIC, ids=lambda c: c[0])
def test_atomic_fallbacks(case):
    """Shapes the plane kernel refuses (pooled_w < 4, a plane above 8704 cells, a pooler above 16): the LDS form while its
    tables fit 64 KB, the scatter form otherwise.  fp32 summation bound; atomics, so no bit-reproducibility is asserted."""
    name, (n, c, h, w), (ph, pw), sr, form = case
    rois, grad = atomic_case(name, n, h, w, ph, pw, c, sr)
    assert _lib().ovis_roi_align_backward_plane_supported(h, w, ph, pw) == 0
    floats = ph * h + pw * w + 2 * (h + w) + 16 * ph * pw
    assert (floats <= 16384) == (form == "lds"), floats
    res = _ref(f"F-{name}", grad, rois, ph, pw, n, c, h, w, sr)
    got = _backward(grad, rois, ph, pw, n, c, h, w, sr).cpu().numpy()
    _report("F", name, f"atomic {form}, {floats} floats", R.worst_ratio(got, res, R.f32_bound(res)))
