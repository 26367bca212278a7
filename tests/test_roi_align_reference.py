"""CPU: pins tests/roi_align_reference.py (the fp64 RoIAlign-backward reference of the GPU edge tests) -- against the
oracle's non-separable fp64 scatter form on inputs whose geometry is exact in float32, against the fp32 oracle within the
fp32 budget, and by hand on one RoI, one bin, one sample.  Also checks, without a GPU, that every case of
tests/test_roi_align_backward_edges_gpu.py keeps its samples clear of the validity boundaries.

The forward reference of the same module is pinned the same way further down: against a plain scalar fp64 loop written
here, by hand on one sample, and -- on every case table of tests/test_roi_align_forward_edges_gpu.py -- by the oracle's
float32 forward staying inside the derived fp32 budget; the tables themselves are held to their safety condition, their
clearance and the dispatch classes they claim to reach."""
import numpy as np
import pytest
import torch

from tests import roi_align_reference as R

S = R.SCALE


def _oracle(oracle_mod, grad, rois, ph, pw, n, c, h, w, sr, stride=1, dtype=torch.float64):
    """The oracle on the RoIs of images in [0, n) (it has no image-id check), bins (s i, s j) zero-scattered into a full tile."""
    keep = (rois[:, 0] >= 0) & (rois[:, 0] < n)
    full = np.zeros((rois.shape[0], c, ph, pw), dtype=np.float64)
    full[:, :, ::stride, ::stride] = grad
    return oracle_mod.roi_align_backward(torch.from_numpy(full[keep]), torch.from_numpy(rois[keep].astype(np.float64)), S, ph, pw,
                                         n, c, h, w, sr, dtype=dtype).numpy().astype(np.float64)


def _dyadic_rois(seed, r, n, h, w):
    """Corners on multiples of 0.5 px (exact x 1/16 in float32; sides divide exactly by 4, 8, 16): inside, clipped at every
    border, out of the map, malformed (x2 < x1), zero size, foreign image ids."""
    g = np.random.default_rng(seed)
    x1 = g.integers(-64, 32 * w, r) * 0.5
    y1 = g.integers(-64, 32 * h, r) * 0.5
    rois = np.stack([g.integers(0, n, r), x1, y1, x1 + g.integers(0, 24 * w, r) * 0.5, y1 + g.integers(0, 24 * h, r) * 0.5], 1)
    fixed = np.array([[0, -48.0, -40.0, 32.0, 24.0], [1, 16.0 * w - 40, 16.0 * h - 24, 16.0 * w + 80, 16.0 * h + 64],
                      [0, 16.0 * w + 512, 16.0 * h + 512, 16.0 * w + 640, 16.0 * h + 640], [1, -900.0, -900.0, -700.0, -800.0],
                      [1, 200.0, 120.0, 136.0, 96.0], [0, 80.0, 64.0, 80.0, 64.0], [n, 32.0, 32.0, 96.0, 96.0],
                      [-1, 32.0, 32.0, 96.0, 96.0], [n + 5, 0.0, 0.0, 64.0, 64.0], [0, 0.0, 0.0, 16.0 * w, 16.0 * h]])
    return np.concatenate([rois, fixed]).astype(np.float32)


@pytest.mark.parametrize("pooler", [(4, 4), (8, 8), (16, 16), (4, 16), (8, 4)], ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("sr", [0, 1, 2, 3])
def test_reference_equals_fp64_scatter_on_exact_geometry(oracle_mod, pooler, sr):
    ph, pw = pooler
    n, c, h, w = 2, 3, 25, 42
    rois = _dyadic_rois(10 * ph + sr, 30, n, h, w)
    grad = R.dense_grad(ph + pw + sr, rois.shape[0], c, ph, pw)
    res = R.roi_align_backward_ref(grad, rois, S, ph, pw, n, c, h, w, sr)
    want = _oracle(oracle_mod, grad, rois, ph, pw, n, c, h, w, sr)
    assert res.mag.max() > 0 and np.all(np.abs(res.ref - want) <= 1e-12 * res.mag)
    assert np.all(res.mag >= np.abs(res.ref) * (1 - 1e-12)) and np.all(res.slack >= 0)
    assert np.all((res.terms > 0) == (res.mag > 0))


@pytest.mark.parametrize("stride", [2, 3])
@pytest.mark.parametrize("pooler", [(8, 8), (16, 16), (16, 4)], ids=lambda p: f"{p[0]}x{p[1]}")
def test_reference_bin_stride_equals_zero_scattered_tile(oracle_mod, pooler, stride):
    ph, pw = pooler
    n, c, h, w = 2, 2, 20, 31
    rois = _dyadic_rois(7 * ph + stride, 20, n, h, w)
    grad = R.dense_grad(stride, rois.shape[0], c, -(-ph // stride), -(-pw // stride))
    for sr in (0, 3):
        res = R.roi_align_backward_ref(grad, rois, S, ph, pw, n, c, h, w, sr, stride)
        want = _oracle(oracle_mod, grad, rois, ph, pw, n, c, h, w, sr, stride)
        assert res.mag.max() > 0 and np.all(np.abs(res.ref - want) <= 1e-12 * res.mag)


@pytest.mark.parametrize("p,sr", [(7, 0), (7, 2), (14, 0), (14, 3)])
def test_fp32_oracle_within_the_fp32_budget(oracle_mod, p, sr):
    """The reference's own float32 arithmetic (sequential sums, ``sample_coord``'s five roundings) stays inside
    (terms + ATOMIC_C) * 2^-24 * mag + slack: the budget the atomic kernels are held to is wide enough for the reference op."""
    n, c, h, w = 2, 3, 25, 42
    rois = R.recipe(p + sr, n, h, w, p, p, 30, (sr,))
    grad = R.dense_grad(p, rois.shape[0], c, p, p)
    res = R.roi_align_backward_ref(grad, rois, S, p, p, n, c, h, w, sr)
    assert res.clearance >= 4.0
    got = _oracle(oracle_mod, grad, rois, p, p, n, c, h, w, sr, dtype=torch.float32)
    ratio = R.worst_ratio(got, res, R.f32_bound(res))
    print(f"fp32 oracle {p}x{p} sampling {sr}: worst error / bound = {ratio:.3f}")
    assert ratio <= 1.0


def test_one_roi_one_bin_one_sample_by_hand():
    """RoI [2, 5] x [3, 5.5] cells, 1 x 1 pooler, one sample at (x, y) = (3.5, 4.25): weights (.5, .5) on columns 3, 4 and
    (.75, .25) on rows 4, 5; d = 3 ulp(3.5) = 3 * 2^-22 in x and 3 ulp(4.25) = 3 * 2^-21 in y, spread over cells lo - 1 .. hi + 1."""
    rois = np.array([[1, 32.0, 48.0, 80.0, 88.0]], dtype=np.float32)
    grad = np.full((1, 2, 1, 1), -2.0, dtype=np.float32)
    grad[0, 1] = 0.0
    res = R.roi_align_backward_ref(grad, rois, S, 1, 1, 2, 2, 8, 9, 1)
    want = np.zeros((8, 9))
    want[4, 3], want[4, 4], want[5, 3], want[5, 4] = 0.375, 0.375, 0.125, 0.125
    assert np.array_equal(res.ref[1, 0], -2.0 * want) and np.array_equal(res.mag[1, 0], 2.0 * want)
    assert np.array_equal(res.terms[1, 0], (want > 0).astype(np.int64))
    assert not res.ref[0].any() and not res.mag[0].any() and not res.slack[0].any() and not res.terms[0].any()
    assert not res.ref[1, 1].any() and not res.slack[1, 1].any() and not res.terms[1, 1].any()  # zero gradient: no slack
    dx, dy = 3 * 2.0 ** -22, 3 * 2.0 ** -21
    wy, wx = np.zeros(8), np.zeros(9)
    wy[4], wy[5], wx[3], wx[4] = 0.75, 0.25, 0.5, 0.5
    sy, sx = np.zeros(8), np.zeros(9)
    sy[3:7], sx[2:6] = dy, dx
    slack = 2.0 * (np.outer(wy + sy, wx + sx) - np.outer(wy, wx))
    assert np.allclose(res.slack[1, 0], slack, rtol=1e-9, atol=0) and np.array_equal(res.slack[1, 0] > 0, slack > 0)
    assert res.slack[1, 0, 3, 3] == pytest.approx(2.0 * dy * (0.5 + dx)) and res.slack[1, 0, 2, 3] == 0.0
    assert res.clearance == pytest.approx(min(4.5 / dx, 3.75 / dy)) and R.clearance_of(rois, S, 1, 1, 2, 8, 9, 1) == res.clearance
    # a sample exactly on the boundary (x = -1): clearance 0, which the GPU cases must never have
    assert R.clearance_of(np.array([[0, -32.0, 16.0, 0.0, 48.0]], dtype=np.float32), S, 1, 1, 1, 8, 9, 1) == 0.0


def test_gpu_case_tables_are_clear_of_the_validity_boundaries():
    from tests import test_roi_align_backward_edges_gpu as E

    cases = list(E.clearances())
    assert len(cases) >= 60
    low = [(name, c) for name, c in cases if not c >= 4.0]
    assert not low, low


def test_split_algorithm_share_of_the_matrix_core_bound():
    """The hi/lo algorithm of the matrix-core kernels, emulated on the reference's own weights, on the cases of the GPU file
    whose cells few terms reach: it stays inside TOL_MFMA * mag + slack, and the share it uses (printed) is what a correct
    kernel measures there -- 0.51 (20 x 9 map), 0.57 (4 x 4 tiles), 0.69 (8 x 5 tiles on the 16 x 16 map) with three terms,
    0.40 with four."""
    from tests import test_roi_align_backward_edges_gpu as E

    rois, grad = E.plane_case(20, 9)
    todo = [("B-20x9", rois, grad, (14, 14), 9, (20, 9), 1)]
    for name, hw, pooler, s, c, ok in E.NHWC:
        if name in ("4x4-c64", "8x5-c130"):
            rois, grad = E.strided_case(name, *hw, *pooler, s, c)
            todo.append((name, rois, grad, pooler, c, hw, s))
    for name, rois, grad, (ph, pw), c, (h, w), s in todo:
        res = R.roi_align_backward_ref(grad, rois, S, ph, pw, 2, c, h, w, 0, s)
        for four in (False, True):
            ratio = R.worst_ratio(R.split_form_emulation(grad, rois, S, ph, pw, 2, c, h, w, 0, s, four), res, R.mfma_bound(res))
            print(f"hi/lo algorithm {name} {'four' if four else 'three'} terms: worst error / bound = {ratio:.3f}")
            assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# The forward reference (``roi_align_forward_ref``) and the case tables of tests/test_roi_align_forward_edges_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
def _forward_scalar(x, rois, scale, ph, pw, sr, n, stride):
    """The operation as the reference kernel states it, a plain fp64 loop over (RoI, bin, sample, four taps): no weight
    matrices, no separability.  start, bin and the grid are float32 (they are decisions both sides share), the rest fp64.
    Returns the bins (s i, s j) and the same sum over |x|."""
    f = np.float32
    _, c, h, w = x.shape
    th, tw = -(-ph // stride), -(-pw // stride)
    out, mag = np.zeros((rois.shape[0], c, th, tw)), np.zeros((rois.shape[0], c, th, tw))

    def taps(v, size):
        if v < -1.0 or v > size:
            return None
        v = max(v, 0.0)
        lo = int(v)
        if lo >= size - 1:
            return size - 1, size - 1, 1.0, 0.0
        return lo, lo + 1, 1.0 - (v - lo), v - lo

    for r, roi in enumerate(rois.astype(f)):
        b = int(roi[0])
        if b < 0 or b >= n:
            continue
        sw, sh = f(roi[1] * f(scale)), f(roi[2] * f(scale))
        bw = f(max(f(f(roi[3] * f(scale)) - sw), f(1)) / f(pw))
        bh = f(max(f(f(roi[4] * f(scale)) - sh), f(1)) / f(ph))
        gh, gw = (sr, sr) if sr > 0 else (int(np.ceil(bh)), int(np.ceil(bw)))
        sw, sh, bw, bh = float(sw), float(sh), float(bw), float(bh)
        for i in range(0, ph, stride):
            for j in range(0, pw, stride):
                acc, acc_abs = np.zeros(c), np.zeros(c)
                for iy in range(gh):
                    ty = taps(sh + i * bh + (iy + .5) * bh / gh, h)
                    if ty is None:
                        continue
                    for ix in range(gw):
                        tx = taps(sw + j * bw + (ix + .5) * bw / gw, w)
                        if tx is None:
                            continue
                        for yy, wy in ((ty[0], ty[2]), (ty[1], ty[3])):
                            for xx, wx in ((tx[0], tx[2]), (tx[1], tx[3])):
                                acc += wy * wx * x[b, :, yy, xx]
                                acc_abs += wy * wx * np.abs(x[b, :, yy, xx])
                out[r, :, i // stride, j // stride] = acc / (gh * gw)
                mag[r, :, i // stride, j // stride] = acc_abs / (gh * gw)
    return out, mag


@pytest.mark.parametrize("pooler", [(14, 14), (7, 7), (3, 5)], ids=lambda p: f"{p[0]}x{p[1]}")
@pytest.mark.parametrize("sr", [0, 2, 3])
def test_forward_reference_equals_a_scalar_loop(pooler, sr):
    ph, pw = pooler
    n, c, h, w = 2, 3, 13, 17
    rois = _dyadic_rois(10 * ph + sr, 8, n, h, w)
    x = np.random.default_rng(ph + sr).standard_normal((n, c, h, w))
    for stride in (1, 2, 3):
        res = R.roi_align_forward_ref(x, rois, S, ph, pw, sr, stride)
        want, mag = _forward_scalar(x, rois, S, ph, pw, sr, n, stride)
        assert res.mag.max() > 0 and np.all(np.abs(res.ref - want) <= 1e-12 * res.mag)
        assert np.all(np.abs(res.mag - mag) <= 1e-12 * mag) and np.all(res.slack >= 0)
        assert np.all((res.terms > 0) | (res.mag == 0))
        foreign = (rois[:, 0] < 0) | (rois[:, 0] >= n)
        assert foreign.sum() == 3 and not res.ref[foreign].any() and not res.slack[foreign].any() and not res.terms[foreign].any()


def test_forward_one_roi_one_bin_one_sample_by_hand():
    """The RoI of the backward's hand case: one sample at (x, y) = (3.5, 4.25), weights (.5, .5) on columns 3, 4 and (.75, .25)
    on rows 4, 5.  x = 2, -4, 8, 16 on those cells: .375 * 2 - .375 * 4 + .125 * 8 + .125 * 16 = 2.25, mag 5.25."""
    rois = np.array([[1, 32.0, 48.0, 80.0, 88.0], [0, np.nan, 48.0, 80.0, 88.0], [1, 32.0, 48.0, np.inf, 88.0], [2, 32.0, 48.0, 80.0, 88.0]],
                    dtype=np.float32)
    x = np.zeros((2, 2, 8, 9))
    x[1, 0, 4, 3], x[1, 0, 4, 4], x[1, 0, 5, 3], x[1, 0, 5, 4] = 2.0, -4.0, 8.0, 16.0
    x[0] = 1.0
    res = R.roi_align_forward_ref(x, rois, S, 1, 1, 1)
    assert res.ref.shape == (4, 2, 1, 1)
    assert res.ref[0, 0, 0, 0] == 2.25 and res.mag[0, 0, 0, 0] == 5.25 and res.terms[0, 0, 0, 0] == 4 and res.terms[0, 1, 0, 0] == 4
    assert res.ref[0, 1, 0, 0] == 0.0 and res.mag[0, 1, 0, 0] == 0.0 and res.slack[0, 1, 0, 0] == 0.0   # a zero map: no slack
    dx, dy = 3 * 2.0 ** -22, 3 * 2.0 ** -21
    wy, wx = np.zeros(8), np.zeros(9)
    wy[4], wy[5], wx[3], wx[4] = 0.75, 0.25, 0.5, 0.5
    sy, sx = np.zeros(8), np.zeros(9)
    sy[3:7], sx[2:6] = dy, dx
    slack = (wy + sy) @ np.abs(x[1, 0]) @ (wx + sx) - 5.25
    assert slack > 0 and res.slack[0, 0, 0, 0] == pytest.approx(slack, rel=1e-6)
    for r in (1, 2, 3):   # NaN, +Inf, a foreign image id: exact zeros and no bound
        assert not res.ref[r].any() and not res.mag[r].any() and not res.slack[r].any() and not res.terms[r].any()
    assert res.clearance == pytest.approx(min(4.5 / dx, 3.75 / dy))
    assert R.f32_forward_bound(res)[0, 0, 0, 0] == pytest.approx(9 * 2.0 ** -24 * 5.25 + slack, rel=1e-6)
    # the float32 twin: the window of that sample, one block, an empty RoI for each of the others
    assert R.roi_window(rois[0], S, 2, 8, 9, 1, 1, 1) == (4, 5, 3, 4) and R.block_shape((4, 5, 3, 4)) == (1, 1)
    assert R.block_shape((0, 49, 0, 83)) == (4, 6) and R.block_shape((3, 18, 7, 23)) == (1, 2)
    assert all(R.roi_window(rois[r], S, 2, 8, 9, 1, 1, sr) is None for r in (1, 2, 3) for sr in (0, 1))
    assert list(R._window_cells(rois, S, 2, 8, 9, 1, 1)) == [4, 0, 0, 0]


def _forward_cases(section):
    from tests import test_roi_align_forward_edges_gpu as F

    return F, [case._replace(c=8) if case.c == 0 else case for sec, case in F.all_cases() if sec == section]


@pytest.mark.parametrize("section", ["A", "B", "C"])
def test_fp32_oracle_forward_within_the_fp32_forward_budget(oracle_mod, section):
    """On every case table of the GPU file the oracle's own float32 forward (the pinned restatement of the reference CPU
    kernel: sequential sums, ``sample_coord``'s five roundings) stays inside (terms + FWD_C) * 2^-24 * mag + slack: the
    budget the exact kernels are held to is wide enough for the reference operation itself."""
    F, cases = _forward_cases(section)
    worst = (0.0, None)
    for case in cases:
        x = F.case_map(case)
        for sr in case.srs:
            res = F.reference(case, sr)
            ratio = R.worst_ratio(F.oracle_bins(oracle_mod, case, x, sr), res, R.f32_forward_bound(res))
            assert ratio <= 1.0, (case.name, sr, ratio)
            worst = max(worst, (ratio, f"{case.name} sampling {sr}"))
    print(f"fp32 oracle forward, section {section}: worst error / bound = {worst[0]:.3f} ({worst[1]})")


def test_forward_gpu_case_tables_are_safe_clear_and_reach_what_they_claim():
    """Without a GPU: grids <= 16 and non-finite RoIs empty (``check_safe``), clearance >= 4 for every sampling ratio, and every
    dispatch class a table claims is present in its RoI set -- a table that silently stops reaching a form fails here."""
    from tests import test_roi_align_forward_edges_gpu as F

    count = 0
    for section, case in F.all_cases():
        F.check_safe(case)
        for sr in case.srs:
            count += 1
            assert R.clearance_of(case.rois, case.scale, case.ph, case.pw, case.n, case.h, case.w, sr) >= 4.0, (case.name, sr)
            if section == "A":
                forms = R.exact_forms(case.rois, case.scale, case.n, case.c, case.h, case.w, case.ph, case.pw, sr)
                assert case.claims[sr] <= forms, (case.name, sr, case.claims[sr] - forms)
                cells = set(R._window_cells(case.rois, case.scale, case.n, case.h, case.w, (case.ph, case.pw), sr))
                assert case.cells <= cells, (case.name, sorted(case.cells - cells))
            elif case.name == "blocks":
                assert case.claims[sr] <= F.block_forms(case, sr), (sr, case.claims[sr] - F.block_forms(case, sr))
            elif section == "C":
                assert all(F.window_classes(case, sr).values()), (case.name, sr, F.window_classes(case, sr))
    assert count >= 100
    # tail stores: every PW % 4 class, PW < 4 and both store counts; supported / unsupported shapes as the kernel decides them
    assert {pw % 4 for pw in F.TAIL_PW if pw >= 4} == {0, 1, 2, 3} and {1, 2, 3} <= set(F.TAIL_PW)
    assert {(pw >= 4) + (pw % 4 != 0) for pw in F.TAIL_PW} == {1, 2}
    assert set(F.SENTINEL_PW) <= set(F.TAIL_PW) and 7 in F.TAIL_PH
    # the shared-tap path: all 25 (row state, column state) pairs at the strides that visit the constructed bins
    case = F.strided_case(14, 14)
    for s in (1, 2):
        states = R.shared_tap_states(case.rois, case.scale, case.n, case.h, case.w, 14, 14, s)
        assert states == {(a, b) for a in F.STATES for b in F.STATES}, (s, sorted(states))
    # the immunity case leaves most of the map outside every window
    far = F.outside_windows(F.immunity_case())
    assert far.sum() > far.size // 4


def test_forward_split_algorithm_share_of_the_matrix_core_bound():
    """The forward's hi/lo algorithm (three terms per product, V rounded to float32 and re-split), emulated on the
    reference's own weights on every table of section B: it stays inside TOL_MFMA * mag + slack; the share it uses (printed)
    is what a correct kernel measures there."""
    F, cases = _forward_cases("B")
    worst = (0.0, None)
    for case in cases:
        x = F.case_map(case)
        for sr in case.srs:
            res = F.reference(case, sr)
            ratio = R.worst_ratio(R.split_form_emulation_forward(x, case.rois, case.scale, case.ph, case.pw, sr), res, R.mfma_forward_bound(res))
            assert ratio <= 1.0, (case.name, sr, ratio)
            worst = max(worst, (ratio, f"{case.name} sampling {sr}"))
    print(f"forward hi/lo algorithm: worst error / bound = {worst[0]:.3f} ({worst[1]})")


def test_forward_elementwise_bound_sees_what_a_whole_tensor_tolerance_cannot():
    """Two mistakes a kernel could make, applied on the host to the emulated matrix-core result of the block-shape table with
    one image scaled by 2^-16: every weight of that image's RoIs off by 2^-10, and one window-corner cell of one of its RoIs
    lost.  Both stay far below 4e-5 * max |x| over the tensor (the tolerance the forward had before); both are outside
    TOL_MFMA * mag + slack in the bins they touch."""
    from tests import test_roi_align_forward_edges_gpu as F

    case = F.block_case()
    x = F.case_map(case).copy()
    x[1] *= np.float32(2.0 ** -16)
    res = R.roi_align_forward_ref(x, case.rois, case.scale, case.ph, case.pw, 0)
    good = R.split_form_emulation_forward(x, case.rois, case.scale, case.ph, case.pw, 0)
    assert R.worst_ratio(good, res, R.mfma_forward_bound(res)) <= 1.0
    small = case.rois[:, 0] == 1
    wrong = good.copy()
    wrong[small] *= 1.0 + 2.0 ** -10
    lost = x.copy()
    r = int(np.flatnonzero(small)[0])
    wy0, wy1, wx0, wx1 = R.roi_window(case.rois[r], case.scale, case.n, case.h, case.w, case.ph, case.pw, 0)
    lost[1, :, wy1 - 1, wx1 - 1] = 0.0
    dropped = R.split_form_emulation_forward(lost, case.rois, case.scale, case.ph, case.pw, 0)
    for bad in (wrong, dropped):
        assert np.abs(bad - res.ref).max() <= 4e-5 * np.abs(x).max()
        assert R.worst_ratio(bad, res, R.mfma_forward_bound(res)) > 10.0
