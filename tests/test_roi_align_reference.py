"""CPU: pins tests/roi_align_reference.py (the fp64 RoIAlign-backward reference of the GPU edge tests) -- against the
oracle's non-separable fp64 scatter form on inputs whose geometry is exact in float32, against the fp32 oracle within the
fp32 budget, and by hand on one RoI, one bin, one sample.  Also checks, without a GPU, that every case of
tests/test_roi_align_backward_edges_gpu.py keeps its samples clear of the validity boundaries."""
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
