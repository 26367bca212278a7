"""GPU: the 3x3 weight gradient on maps of at most 64 pixels contracts over the in-map rows of every tap only
(csrc/split_gemm.hip, the SMALL form of split_gemm_tn_kernel): the row enumeration is pinned exactly with one-hot
operands, the sums against an fp64 reference of the hi + lo operands, on 7x7 and on the edge shapes of the form."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 2e-5


def _C():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C as c
    return c


def _unpair64(p):
    """pair layout [rows, 2K] bf16 -> hi + lo as fp64 [rows, K]: the values the kernel multiplies."""
    rows, k2 = p.shape
    v = p.view(rows, k2 // 64, 2, 32).double()
    return (v[:, :, 0, :] + v[:, :, 1, :]).reshape(rows, -1)


def _operands(r, h, w, n, ch, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    m = r * h * w
    C = _C()
    return C.split_pair(torch.randn(m, n, device="cuda", generator=g)), C.split_pair(torch.randn(m, ch, device="cuda", generator=g))


def _tap_rows(x64, r, h, w, kh, kw):
    """[m, ch] fp64 -> tap-major im2col rows [m, kh*kw*ch], zeros outside the map."""
    ch = x64.shape[1]
    cols = F.unfold(x64.view(r, h, w, ch).permute(0, 3, 1, 2), (kh, kw), padding=(kh // 2, kw // 2))
    return cols.view(r, ch, kh * kw, h * w).permute(0, 3, 2, 1).reshape(r * h * w, kh * kw * ch)


def _skip_unsupported(n, ch, conv):
    if not _C().split_gemm_pair_tn_supported(n, ch, conv):
        pytest.skip("split_gemm_pair_tn does not serve this shape")


HOT = [(0, 0), (0, 6), (6, 0), (6, 6), (0, 3), (3, 0), (3, 6), (6, 3), (3, 3)]  # corners, edge middles, centre


@pytest.mark.parametrize("py,px", HOT)
@pytest.mark.parametrize("last_map", [False, True])
def test_one_hot_input_pins_the_row_of_every_tap(py, px, last_map):
    """X = one pixel of one map, one channel, 1.0; G = small integers: dW[n, (tap, c)] is the G value of the output pixel
    whose tap reads the hot pixel -- an integer, reproduced exactly by a gather."""
    C = _C()
    r, h, w, n, ch, kh, kw = 70, 7, 7, 128, 128, 3, 3   # 3430 rows: several slices, a tail in every tap class
    _skip_unsupported(n, ch, (h, w, kh, kw))
    m = r * h * w
    hot_map, hot_c = (r - 1 if last_map else 0), 37
    gi = (np.arange(m)[:, None] * 37 + np.arange(n)[None, :] * 11) % 199 - 99      # exact in bf16
    x = torch.zeros(m, ch, device="cuda")
    x[hot_map * h * w + py * w + px, hot_c] = 1.0
    dw = C.split_gemm_pair_tn(C.split_pair(torch.from_numpy(gi).float().cuda()), C.split_pair(x), (h, w, kh, kw))
    want = np.zeros((n, kh * kw, ch), dtype=np.float32)
    for tap in range(kh * kw):
        oy, ox = py - (tap // kw - kh // 2), px - (tap % kw - kw // 2)            # output pixel that reads the hot one
        if 0 <= oy < h and 0 <= ox < w:
            want[:, tap, hot_c] = gi[hot_map * h * w + oy * w + ox]
    assert np.array_equal(dw.cpu().numpy(), want.reshape(n, kh * kw * ch))


SHAPES = [(r, 7, 7, n, ch) for r in (1, 3, 70) for n, ch in ((128, 128), (256, 256))] + [
    (5, 8, 8, 128, 128),     # the 64-pixel limit of the form
    (7, 5, 3, 128, 128),     # non-square: four tap classes
    (9, 1, 7, 128, 128), (9, 7, 1, 128, 128),   # taps without any in-map row
    (33, 2, 2, 128, 128), (33, 1, 1, 128, 128),
]


@pytest.mark.parametrize("r,h,w,n,ch", SHAPES)
def test_in_map_rows_vs_fp64_of_the_pair_operands(r, h, w, n, ch):
    C = _C()
    conv = (h, w, 3, 3)
    _skip_unsupported(n, ch, conv)
    gp, xp = _operands(r, h, w, n, ch, seed=r * 1000 + h * 10 + w + n)
    dw = C.split_gemm_pair_tn(gp, xp, conv)
    g64, cols = _unpair64(gp), _tap_rows(_unpair64(xp), r, h, w, 3, 3)
    ref = g64.t() @ cols
    bound = g64.abs().t() @ cols.abs()
    err = (dw.double() - ref).abs()
    print(f"max err / bound = {(err / bound.clamp(min=1e-300)).max().item():.3e}")
    assert bool((err <= TOL * bound).all())
    # a tap none of whose rows lies inside the map leaves exact zeros in all its columns
    dwt = dw.view(n, 9, ch)
    for tap in range(9):
        dy, dx = tap // 3 - 1, tap % 3 - 1
        if abs(dy) >= h or abs(dx) >= w:
            assert dwt[:, tap].count_nonzero().item() == 0, tap
    # two launches on the same operands: the same bits
    assert torch.equal(dw, C.split_gemm_pair_tn(gp, xp, conv))


@pytest.mark.parametrize("r,h,w,n,ch", [(70, 7, 7, 128, 256), (7, 5, 3, 128, 128)])
def test_column_slices_of_wider_pair_tensors_equal_contiguous_copies(r, h, w, n, ch):
    C = _C()
    conv = (h, w, 3, 3)
    _skip_unsupported(n, ch, conv)
    gw, xw = _operands(r, h, w, n + 64, ch + 96, seed=5)                 # pair tensors of wider matrices
    gs, xs = gw[:, 64:64 + 2 * n], xw[:, 128:128 + 2 * ch]               # whole (hi32 | lo32) groups: still pair layout
    assert gs.stride(0) > gs.shape[1] and xs.stride(0) > xs.shape[1]
    assert torch.equal(C.split_gemm_pair_tn(gs, xs, conv), C.split_gemm_pair_tn(gs.contiguous(), xs.contiguous(), conv))


@pytest.mark.parametrize("r,h,w,n,ch", [(5, 8, 8, 128, 128), (70, 7, 7, 256, 256)])
def test_fused_reduce_equals_the_plain_result_relaid_and_scaled(r, h, w, n, ch):
    C = _C()
    conv = (h, w, 3, 3)
    _skip_unsupported(n, ch, conv)
    gp, xp = _operands(r, h, w, n, ch, seed=9)
    sc = torch.rand(n, device="cuda") + 0.5
    plain = C.split_gemm_pair_tn(gp, xp, conv)                                            # [n, 9*ch] tap-major
    got = C.split_gemm_pair_tn(gp, xp, conv, scale=sc, weight_shape=(n, ch, 3, 3))
    want = plain.view(n, 3, 3, ch).permute(0, 3, 1, 2) * sc.view(-1, 1, 1, 1)
    assert got.shape == (n, ch, 3, 3) and (got - want).abs().max().item() <= 1e-6 * want.abs().max().item()


def test_all_maps_in_one_call_equal_the_sum_over_two_halves():
    C = _C()
    r, h, w, n, ch = 70, 7, 7, 256, 256
    conv = (h, w, 3, 3)
    _skip_unsupported(n, ch, conv)
    gp, xp = _operands(r, h, w, n, ch, seed=11)
    half = (r // 2) * h * w                                                               # a map boundary
    dw = C.split_gemm_pair_tn(gp, xp, conv)
    dw2 = C.split_gemm_pair_tn(gp[:half], xp[:half], conv) + C.split_gemm_pair_tn(gp[half:], xp[half:], conv)
    assert (dw - dw2).abs().max().item() <= 1e-5 * dw.abs().max().item()


@pytest.mark.parametrize("h,w,kh,kw", [(1, 64, 1, 19), (64, 1, 25, 1), (7, 7, 5, 5)])
def test_long_and_5x5_kernels_on_small_maps_vs_fp64(h, w, kh, kw):
    """More than five taps a side have more in-map row counts than the small-map form keeps classes for: they are served
    by the general form; 5 x 5 (nine classes) is the largest kernel of the small-map form."""
    C = _C()
    r, n, ch, conv = 3, 128, 128, (h, w, kh, kw)
    _skip_unsupported(n, ch, conv)
    gp, xp = _operands(r, h, w, n, ch, seed=kh * 100 + kw)
    dw = C.split_gemm_pair_tn(gp, xp, conv)
    g64, cols = _unpair64(gp), _tap_rows(_unpair64(xp), r, h, w, kh, kw)
    err = (dw.double() - g64.t() @ cols).abs()
    assert bool((err <= TOL * (g64.abs().t() @ cols.abs())).all())
