"""GPU: the kernels that WRITE pair-layout operands (csrc/split_gemm.hip: split_pair, gate_split_pair, im2col_nchw_pair,
weight_prep_pair, im2col_pair; csrc/weight_prep_multi.hip) and slab_reduce, which closes every weight gradient, held BIT FOR
BIT to tests/pair_layout_reference.py computed on the host from the same inputs.  No tolerance anywhere, except the derived
fp64 bound of slab_reduce, which stands beside the exact comparison with the kernel's own summation tree.

Elements whose reference is a NaN are exempt from the bit comparison: there the device must give a NaN too, whatever its
payload.  Inputs come from the reference module's generators (ties, subnormals, signed zeros, overflow to infinity, inf, NaN:
tests/test_pair_layout_reference.py shows that they tell the listed wrong kernels from the right one).

ONE GRID PASS.  Every launcher clamps its grid to a multiple of OVIS_NUM_CU (csrc/ovis_common.h) workgroups of 256 threads and
the kernel strides over the rest; the capacities below restate those clamps (``blocks < 8L * OVIS_NUM_CU ? ...``) and each
kernel gets one shape beyond its capacity whose work-item count is no multiple of it:
  split_pair, gate_split_pair, weight_prep_pair: 8 * OVIS_NUM_CU * 256 groups of 8 values;
  slab_reduce: 8 * OVIS_NUM_CU * 256 lanes, four lanes per group of 4 channels;
  im2col_nchw_pair: 16 * OVIS_NUM_CU * 256 groups of 8 values;  im2col_pair: 16 * OVIS_NUM_CU * 256 16-byte slots.
"""
import os
import re

import numpy as np
import pytest
import torch

from tests import pair_layout_reference as R

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

OVIS_OK, OVIS_EINVAL, OVIS_ERANGE = 0, -1, -3

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(_ROOT, "cvpr22_cross_modal_pseudo_labeling_amd", "csrc", "ovis_common.h")) as _f:
    NUM_CU = int(re.search(r"#define\s+OVIS_NUM_CU\s+(\d+)", _f.read()).group(1))
PASS_8 = 8 * NUM_CU * 256      # split_pair / gate_split_pair / weight_prep_pair (groups of 8), slab_reduce (lanes)
PASS_16 = 16 * NUM_CU * 256    # im2col_nchw_pair (groups of 8), im2col_pair (16-byte slots)


def _beyond(items, capacity):
    """The shape runs the grid-stride loop a second time, and the last pass is a partial one."""
    return capacity < items < 2 * capacity and items % capacity != 0


def C():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C
    return _C


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def dev_pair(bits):
    """uint16 pair rows -> the bfloat16 device tensor the package hands around."""
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).cuda().view(torch.bfloat16)


def host_bits16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def host_bits32(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _report(bad, got, want, what):
    idx = np.argwhere(bad)[:8]
    lines = [f"{tuple(int(v) for v in i)}: got {int(got[tuple(i)]):#x} want {int(want[tuple(i)]):#x}" for i in idx]
    return f"{what}: {int(bad.sum())} of {bad.size} differ; " + "; ".join(lines)


def assert_pair_bits(got_t, want, what):
    """bf16 bits of a device pair tensor == the reference's, NaN where (and only where the comparison is waived) it has NaN."""
    got = host_bits16(got_t)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = R.bf16_is_nan(want)
    assert R.bf16_is_nan(got[nan]).all(), f"{what}: a NaN of the reference is no NaN on the device"
    bad = (got != want) & ~nan
    assert not bad.any(), _report(bad, got, want, what)


def assert_f32_bits(got_t, want, what):
    got = host_bits32(got_t).reshape(want.shape)
    wb = np.ascontiguousarray(want, dtype=np.float32).view(np.uint32)
    nan = np.isnan(want)
    assert np.isnan(got.view(np.float32)[nan]).all(), f"{what}: a NaN of the reference is no NaN on the device"
    bad = (got != wb) & ~nan
    assert not bad.any(), _report(bad, got, wb, what)


def _stream():
    return C()._stream()


# ------------------------------------------------------------------ split_pair
def _split_raw(x):
    """ovis_split_pair_f32 on the tensor AS IT IS (the Python shim copies views it deems unfit)."""
    out = torch.full((x.shape[0], 2 * x.shape[1]), -1.0, dtype=torch.bfloat16, device="cuda")
    rc = C()._L.ovis_split_pair_f32(x.data_ptr(), x.stride(0), out.data_ptr(), x.shape[0], x.shape[1], _stream())
    assert rc == OVIS_OK
    return out


@pytest.mark.parametrize("cols", [32, 64, 96, 1056])
@pytest.mark.parametrize("rows", [1, 37])
def test_split_pair_bits(rows, cols):
    x = R.edge_values(rows, cols, 100 + rows + cols)
    want = R.pair_rows(x)
    assert_pair_bits(C().split_pair(dev(x)), want, "split_pair")
    assert_pair_bits(_split_raw(dev(x)), want, "ovis_split_pair_f32")


def test_split_pair_bits_beyond_one_grid_pass():
    rows, cols = 4099, 1056
    assert _beyond(rows * (cols // 8), PASS_8)
    x = R.edge_values(rows, cols, 101)
    assert_pair_bits(_split_raw(dev(x)), R.pair_rows(x), "split_pair, second pass")


def test_split_pair_strided_and_offset_views():
    big = R.edge_values(37, 192, 102)
    bd = dev(big)
    for c0, c1 in ((32, 128), (4, 68), (0, 64), (92, 188)):      # 16-byte-aligned column offsets, row stride 192
        view = bd[:, c0:c1]
        assert view.data_ptr() % 16 == 0 and view.stride(0) == 192
        assert_pair_bits(_split_raw(view), R.pair_rows(big[:, c0:c1]), f"split_pair view {c0}:{c1}")
    every_other = bd.view(-1)[: 18 * 384].view(18, 384)[:, :96]   # row stride 384: every second row's first 96 columns
    assert_pair_bits(_split_raw(every_other), R.pair_rows(big[0:36:2, :96]), "split_pair, row stride 2 rows")


def test_split_pair_refusals():
    L = C()._L
    x = torch.zeros(8, 64, device="cuda")
    out = torch.full((8, 128), 7.0, dtype=torch.bfloat16, device="cuda")
    before = host_bits16(out).copy()
    s = _stream()
    assert x.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    assert L.ovis_split_pair_f32(x.data_ptr(), 64, out.data_ptr(), 8, 40, s) == OVIS_ERANGE      # cols % 32
    assert L.ovis_split_pair_f32(x.data_ptr(), 34, out.data_ptr(), 8, 32, s) == OVIS_ERANGE      # row stride % 4
    assert L.ovis_split_pair_f32(x.data_ptr() + 4, 64, out.data_ptr(), 7, 32, s) == OVIS_ERANGE  # source 4 bytes off
    assert L.ovis_split_pair_f32(x.data_ptr(), 64, out.data_ptr() + 8, 7, 32, s) == OVIS_ERANGE  # destination 8 bytes off
    assert L.ovis_split_pair_f32(0, 64, out.data_ptr(), 8, 64, s) == OVIS_EINVAL
    assert L.ovis_split_pair_f32(x.data_ptr(), 64, 0, 8, 64, s) == OVIS_EINVAL
    assert L.ovis_split_pair_f32(x.data_ptr(), 64, out.data_ptr(), -1, 64, s) == OVIS_EINVAL
    assert L.ovis_split_pair_f32(x.data_ptr(), 64, out.data_ptr(), 0, 64, s) == OVIS_OK          # nothing to do
    torch.cuda.synchronize()
    assert np.array_equal(host_bits16(out), before)
    with pytest.raises(RuntimeError):
        C().split_pair(torch.zeros(4, 40, device="cuda"))


# ------------------------------------------------------------------ gate_split_pair
def _gate_raw(dy, gate, gate_is_pair, want_f32, rows, cols, pooled=None, pool_rows=0, selected=None, slot=None):
    """ovis_gate_split_pair_rows_f32 on device tensors as they are -> (pair tensor, fp32 tensor or None)."""
    out = torch.full((rows, 2 * cols), -1.0, dtype=torch.bfloat16, device="cuda")
    g32 = torch.full((rows, cols), -1.0, device="cuda") if want_f32 else None
    p = C()._ptr
    rc = C()._L.ovis_gate_split_pair_rows_f32(p(dy), 0 if dy is None else dy.stride(0), p(gate), int(gate_is_pair),
                                             out.data_ptr(), p(g32), rows, cols, p(pooled), pool_rows, p(selected), p(slot),
                                             _stream())
    assert rc == OVIS_OK
    return out, g32


# operands: (dy, pooled, selected)
OPERANDS = {"dy": (True, False, False), "dy+pooled": (True, True, False), "pooled": (False, True, False),
            "dy+pooled+selected": (True, True, True), "pooled+selected": (False, True, True)}


def _gate_case(rows, cols, pool_rows, operands, seed):
    """Host inputs of one case.  Operands that are summed stay finite (special=False) so that most sums are comparable; a
    lone dy carries inf and NaN too."""
    has_dy, has_pool, has_sel = OPERANDS[operands]
    groups = rows // pool_rows
    lone = has_dy and not has_pool
    dy = R.edge_values(rows, cols, seed, special=lone) if has_dy else None
    pooled = R.edge_values(groups, cols, seed + 1, special=False) if has_pool else None
    selected = slot = None
    if has_sel:
        nsel = 4                                              # slot 1 stays unused; first and last slot are used, once each
        selected = R.edge_values(nsel * pool_rows, cols, seed + 2, special=False)
        slot = np.full(groups, -1, dtype=np.int32)
        slot[1], slot[groups - 1], slot[groups // 2] = 0, nsel - 1, 2
    y = R.gate_values(rows, cols, seed + 3)
    return dy, pooled, selected, slot, y


def _gate_check(rows, cols, pool_rows, operands, gate_form, want_f32, seed, dy_stride=None):
    dy, pooled, selected, slot, y = _gate_case(rows, cols, pool_rows, operands, seed)
    gate_h = {"none": None, "f32": y, "pair": R.pair_rows(y)}[gate_form]
    want_p, want_v = R.gate_split(dy, gate_h, gate_form == "pair", pooled, pool_rows, selected, slot, rows=rows)
    gate_d = {"none": None, "f32": dev(y), "pair": dev_pair(R.pair_rows(y))}[gate_form]
    dy_d = None
    if dy is not None:
        if dy_stride is None:
            dy_d = dev(dy)
        else:
            wide = torch.full((rows, dy_stride), 3.0e38, device="cuda")
            wide[:, :cols] = dev(dy)
            dy_d = wide[:, :cols]
            assert dy_d.stride(0) == dy_stride and not dy_d.is_contiguous()
    got_p, got_v = _gate_raw(dy_d, gate_d, gate_form == "pair", want_f32, rows, cols,
                             None if pooled is None else dev(pooled), pool_rows if (pooled is not None) else 0,
                             None if selected is None else dev(selected), None if slot is None else dev(slot))
    what = f"gate_split_pair[{gate_form}, f32={want_f32}, {operands}, pool_rows={pool_rows}]"
    assert_pair_bits(got_p, want_p, what)
    if want_f32:
        assert_f32_bits(got_v, want_v, what + " fp32 copy")
    return y, want_v, got_p


@pytest.mark.parametrize("pool_rows", [1, 49])
@pytest.mark.parametrize("operands", list(OPERANDS))
@pytest.mark.parametrize("want_f32", [False, True])
@pytest.mark.parametrize("gate_form", ["none", "f32", "pair"])
def test_gate_split_pair_bits(gate_form, want_f32, operands, pool_rows):
    groups = 37 if pool_rows == 1 else 6
    _gate_check(groups * pool_rows, 96, pool_rows, operands, gate_form, want_f32, 200 + pool_rows)


@pytest.mark.parametrize("gate_form", ["f32", "pair"])
def test_gate_split_pair_row_strided_dy(gate_form):
    _gate_check(6 * 49, 64, 49, "dy+pooled+selected", gate_form, True, 210, dy_stride=100)
    _gate_check(37, 32, 1, "dy", gate_form, False, 211, dy_stride=36)


@pytest.mark.parametrize("gate_form", ["f32", "pair"])
def test_gate_split_pair_bits_beyond_one_grid_pass(gate_form):
    rows, cols = 86 * 49, 1024
    assert _beyond(rows * (cols // 8), PASS_8)
    _gate_check(rows, cols, 49, "dy+pooled+selected", gate_form, True, 220)


def test_gate_forms_agree_on_positive_normals_and_differ_below():
    """The pair gate reads bf16(y): it equals the fp32 gate for every positive NORMAL y (rounding keeps the sign and maps no
    normal to zero); for 0 < y <= 2^-134 bf16(y) is 0, the pair gate is shut and the fp32 gate open.  Each against its own
    reference (above); here the two device results against each other."""
    rows, cols = 74, 96
    dy = R.edge_values(rows, cols, 230, special=False)
    y = R.gate_values(rows, cols, 231)
    f_p, f_v = _gate_raw(dev(dy), dev(y), False, True, rows, cols)
    p_p, p_v = _gate_raw(dev(dy), dev_pair(R.pair_rows(y)), True, True, rows, cols)
    fv, pv = host_bits32(f_v), host_bits32(p_v)
    normal = y >= np.float32(2.0 ** -126)
    tiny = (y > 0) & (y <= np.float32(2.0 ** -134))
    assert normal.any() and tiny.any()
    assert np.array_equal(fv[normal], pv[normal]) and np.array_equal(fv[normal], dy.view(np.uint32)[normal])
    assert np.array_equal(fv[~tiny], pv[~tiny])
    assert not pv[tiny].any() and np.array_equal(fv[tiny], dy.view(np.uint32)[tiny]) and fv[tiny].any()
    fh, fl = R.unpair(host_bits16(f_p))
    ph, pl = R.unpair(host_bits16(p_p))
    assert np.array_equal(fh[~tiny], ph[~tiny]) and np.array_equal(fl[~tiny], pl[~tiny])


# ------------------------------------------------------------------ im2col_nchw_pair
def _nchw_raw(x, kh, kw, stride, pad, kp):
    n, c, h, w = x.shape
    ho, wo = R.conv_out_size(h, kh, stride, pad), R.conv_out_size(w, kw, stride, pad)
    out = torch.full((n * ho * wo, 2 * kp), -1.0, dtype=torch.bfloat16, device="cuda")
    rc = C()._L.ovis_im2col_nchw_pair_f32(x.data_ptr(), out.data_ptr(), n, c, h, w, kh, kw, stride, pad, kp, _stream())
    return rc, out


def _image(shape, seed):
    n, c, h, w = shape
    return R.edge_values(n * c * h, w, seed).reshape(shape)


@pytest.mark.parametrize("shape,kh,kw,stride,pad", [((2, 3, 67, 93), 7, 7, 2, 3), ((1, 3, 7, 5), 7, 7, 2, 3),
                                                      ((2, 4, 6, 9), 3, 3, 1, 0), ((1, 3, 2, 9), 5, 5, 1, 2),
                                                      ((2, 2, 11, 13), 3, 3, 3, 1), ((1, 1, 9, 9), 3, 3, 2, 1),
                                                      ((2, 1, 8, 35), 1, 1, 1, 0)])
def test_im2col_nchw_pair_bits(shape, kh, kw, stride, pad):
    x = _image(shape, 300 + shape[2])
    want, (ho, wo) = R.im2col_nchw_pair(x, kh, kw, stride, pad)
    got, hw = C().im2col_nchw_pair(dev(x), kh, kw, stride, pad)
    assert hw == (ho, wo)
    assert_pair_bits(got, want, "im2col_nchw_pair")                  # hi AND lo, everywhere
    k = kh * kw * shape[1]
    hi, lo = R.unpair(host_bits16(got))
    assert not hi[:, k:].any() and not lo[:, k:].any()


def test_im2col_nchw_pair_wider_padding_and_refusals():
    x = _image((2, 3, 23, 17), 310)
    xd = dev(x)
    for kp in (160, 192):                                            # 147 columns of the stem's 7x7 on 3 channels
        rc, got = _nchw_raw(xd, 7, 7, 2, 3, kp)
        assert rc == OVIS_OK
        assert_pair_bits(got, R.im2col_nchw_pair(x, 7, 7, 2, 3, kp)[0], f"im2col_nchw_pair k_padded={kp}")
        hi, lo = R.unpair(host_bits16(got))
        assert not hi[:, 147:].any() and not lo[:, 147:].any()
    assert _nchw_raw(xd, 7, 7, 2, 3, 152)[0] == OVIS_ERANGE          # no multiple of 32
    rc, out = _nchw_raw(xd, 7, 7, 2, 3, 128)                         # too small
    torch.cuda.synchronize()
    assert rc == OVIS_ERANGE and (host_bits16(out) == 0xBF80).all()  # the pre-filled -1 is untouched


def test_im2col_nchw_pair_bits_beyond_one_grid_pass():
    shape = (1, 3, 460, 461)                                          # the stem on one image: 230 x 231 rows of 160 columns
    ho, wo = R.conv_out_size(460, 7, 2, 3), R.conv_out_size(461, 7, 2, 3)
    assert _beyond(ho * wo * (160 // 8), PASS_16)
    x = _image(shape, 320)
    got, _ = C().im2col_nchw_pair(dev(x), 7, 7, 2, 3)
    assert_pair_bits(got, R.im2col_nchw_pair(x, 7, 7, 2, 3)[0], "im2col_nchw_pair, second pass")


# ------------------------------------------------------------------ weight_prep_pair
def _weight(shape, seed):
    n, c, kh, kw = shape
    return R.edge_values(n * c, kh * kw, seed, special=False).reshape(shape) if kh * kw > 1 else \
        R.edge_values(n, c, seed, special=False).reshape(shape)


def _scale(n, seed):
    """Folded FrozenBN scales: powers of two (the product is exact), 1, and values that make the product round."""
    sc = np.random.default_rng(seed).uniform(0.5, 1.5, size=n).astype(np.float32)
    sc[0::7], sc[1::7], sc[2::7], sc[3::7] = 2.0, 0.5, 1.0, -0.75
    return sc


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("shape", [(32, 32, 1, 1), (64, 32, 3, 3), (32, 96, 3, 5), (128, 64, 1, 1)])
def test_weight_prep_pair_bits(shape, scaled, transposed):
    w = _weight(shape, 400 + shape[0] + shape[1])
    sc = _scale(shape[0], 401) if scaled else None
    want_f, want_b = R.weight_prep(w, sc, transposed)
    f, b = C().weight_prep_pair(dev(w), None if sc is None else dev(sc), transposed)
    assert_pair_bits(f, want_f, "weight_prep_pair forward")
    assert (b is None) == (not transposed)
    if transposed:
        assert_pair_bits(b, want_b, "weight_prep_pair transposed")
    if scaled:  # the scale rounds some products: the unscaled operand differs
        assert not np.array_equal(want_f, R.weight_prep(w, None, False)[0])


def test_weight_prep_pair_bits_beyond_one_grid_pass():
    shape = (512, 512, 3, 3)                                          # res5's 3x3: forward + transposed groups of 8
    assert _beyond(2 * 512 * 9 * (512 // 8), PASS_8)
    w = _weight(shape, 410)
    sc = _scale(512, 411)
    want_f, want_b = R.weight_prep(w, sc, True)
    f, b = C().weight_prep_pair(dev(w), dev(sc), True)
    assert_pair_bits(f, want_f, "weight_prep_pair forward, res5")
    assert_pair_bits(b, want_b, "weight_prep_pair transposed, second pass")


def test_weight_prep_pair_refusals():
    L = C()._L
    s = _stream()
    w = torch.zeros(48 * 48 * 9, device="cuda")
    f = torch.zeros(48 * 48 * 9 * 2, dtype=torch.bfloat16, device="cuda")
    b = torch.zeros(48 * 48 * 9 * 2, dtype=torch.bfloat16, device="cuda")
    assert L.ovis_weight_prep_pair_f32(w.data_ptr(), 0, f.data_ptr(), 0, 32, 48, 9, s) == OVIS_ERANGE             # C % 32
    assert L.ovis_weight_prep_pair_f32(w.data_ptr(), 0, f.data_ptr(), b.data_ptr(), 32, 48, 9, s) == OVIS_ERANGE
    assert L.ovis_weight_prep_pair_f32(w.data_ptr(), 0, f.data_ptr(), b.data_ptr(), 48, 32, 9, s) == OVIS_ERANGE  # N % 32, transposed
    assert L.ovis_weight_prep_pair_f32(0, 0, f.data_ptr(), 0, 32, 32, 1, s) == OVIS_EINVAL
    assert L.ovis_weight_prep_pair_f32(w.data_ptr(), 0, 0, 0, 32, 32, 1, s) == OVIS_EINVAL
    # N % 32 != 0 is fine without the transposed form
    wh = _weight((48, 32, 3, 3), 420)
    got, none = C().weight_prep_pair(dev(wh), None, False)
    assert none is None
    assert_pair_bits(got, R.weight_prep(wh, None, False)[0], "weight_prep_pair N = 48")


# ------------------------------------------------------------------ weight_prep_pair_multi
def _conv(n, c, kh, kw, seed, scaled=True):
    w = _weight((n, c, kh, kw), seed)
    return w, (_scale(n, seed + 1) if scaled else None)


def test_weight_prep_plan_bits():
    """Every buffer WeightPrepPlan.run() fills against the host reference: a projection block ([w3 | wd] side by side), an
    identity block with mixed scales, res5 sizes, and lone convolutions with 15 taps (the LDS maximum) and 32 x 32 x 1 x 1."""
    from cvpr22_cross_modal_pseudo_labeling_amd.layers.pair_bottleneck import ConvWeights, PairWeights, WeightPrepPlan
    host = {
        "a": [_conv(64, 256, 1, 1, 500), _conv(64, 64, 3, 3, 502), _conv(256, 64, 1, 1, 504), _conv(256, 256, 1, 1, 506)],
        "b": [_conv(128, 512, 1, 1, 510, False), _conv(128, 128, 3, 3, 512), _conv(512, 128, 1, 1, 514, False)],
        "c": [_conv(512, 2048, 1, 1, 520), _conv(512, 512, 3, 3, 522), _conv(2048, 512, 1, 1, 524)],
        "d": [_conv(32, 96, 3, 5, 530)],
        "e": [_conv(32, 32, 1, 1, 532, False)],
    }
    onto = {k: [(dev(w), None if s is None else dev(s)) for w, s in v] for k, v in host.items()}
    plan = WeightPrepPlan(list(onto.items()))
    assert plan.max_taps == 15
    plan.run()
    for key, convs in host.items():
        got = plan.lookup(key, tuple(s for _, s in onto[key]))
        want = [R.weight_prep(w, s, True) for w, s in convs]
        if len(convs) == 1:
            assert isinstance(got, ConvWeights)
            assert_pair_bits(got.w, want[0][0], f"plan {key} forward")
            assert_pair_bits(got.wt, want[0][1], f"plan {key} transposed")
            continue
        assert isinstance(got, PairWeights)
        for i, name in enumerate(("w1", "w2", "w3", "wd")[:len(convs)]):
            assert_pair_bits(getattr(got, name), want[i][0], f"plan {key} {name}")
            assert_pair_bits(got.wts[i], want[i][1], f"plan {key} {name} transposed")
        if len(convs) == 4:
            assert_pair_bits(got.w3d, np.concatenate([want[2][0], want[3][0]], 1), f"plan {key} [w3 | wd]")
        else:
            assert got.wd is None and got.w3d is None and got.wts[3] is None


def _prep_table(records):
    """The 64-byte item records of ovis_weight_prep_pair_multi_f32 (include/ovis_hip.h) and one block per 32 x 32 tile."""
    table = np.zeros((len(records), 8), dtype=np.int64)
    blocks = []
    for i, (w, sc, fwd, bwd, frb, brb, n, c, t) in enumerate(records):
        table[i] = (w, sc, fwd, bwd, frb, brb, n | (c << 32), t)
        blocks += [(i, tile) for tile in range((n // 32) * (c // 32))]
    return dev(table.view(np.uint8).reshape(-1)), dev(np.array(blocks, dtype=np.int32).reshape(-1, 2))


@pytest.mark.parametrize("which", ["w3", "wd"])
def test_weight_prep_multi_writes_only_its_half_of_a_wider_matrix(which):
    """[w3 | wd] of a projection block is ONE matrix written by two items, each with the row stride of the whole: a table with
    only one of them leaves the other half's bytes alone."""
    assert C().weight_prep_tile() == 32
    n, c3, cd = 64, 32, 96
    w3, s3 = _conv(n, c3, 1, 1, 540)
    wd, sd = _conv(n, cd, 1, 1, 542)
    w, sc, k, off = (w3, s3, c3, 0) if which == "w3" else (wd, sd, cd, c3)
    fill = 0x1234
    both = dev_pair(np.full((n, 2 * (c3 + cd)), fill, dtype=np.uint16))
    tb = dev_pair(np.full((k, 2 * n), fill, dtype=np.uint16))
    wdev, sdev = dev(w), dev(sc)
    items, blocks = _prep_table([(wdev.data_ptr(), sdev.data_ptr(), both.data_ptr() + 4 * off, tb.data_ptr(),
                                  4 * (c3 + cd), 4 * n, n, k, 1)])
    C().weight_prep_pair_multi(items, blocks, 1)
    want_f, want_b = R.weight_prep(w, sc, True)
    got = host_bits16(both)
    assert_pair_bits(both[:, 2 * off:2 * (off + k)], want_f, f"[w3 | wd]: the {which} item")
    other = np.ones(2 * (c3 + cd), dtype=bool)
    other[2 * off:2 * (off + k)] = False
    assert (got[:, other] == fill).all()
    assert_pair_bits(tb, want_b, f"{which} transposed")


def test_weight_prep_multi_refuses_sixteen_taps():
    items = torch.zeros(64, dtype=torch.uint8, device="cuda")
    blocks = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
    L = C()._L
    assert L.ovis_weight_prep_pair_multi_f32(items.data_ptr(), blocks.data_ptr(), 1, 16, _stream()) == OVIS_ERANGE
    assert L.ovis_weight_prep_pair_multi_f32(items.data_ptr(), blocks.data_ptr(), 0, 15, _stream()) == OVIS_OK   # no block
    assert L.ovis_weight_prep_pair_multi_f32(0, blocks.data_ptr(), 1, 15, _stream()) == OVIS_EINVAL


# ------------------------------------------------------------------ im2col_pair
def _maps(num, h, w, c, seed):
    """Pair rows of `num` NHWC maps, map r filled from [2^(2r), 1.9 * 2^(2r)): a tap that reaches into a neighbouring map
    shows in the exponent of its hi halves."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(1.0, 1.9, size=(num, h * w, c)) * np.exp2(2.0 * np.arange(num)).reshape(num, 1, 1)
    return R.pair_rows(x.astype(np.float32).reshape(num * h * w, c))


IM2COL_CASES = [(2, 1, 1, 32, 3, 3), (3, 1, 5, 32, 3, 3), (2, 7, 7, 64, 3, 3), (2, 2, 3, 32, 5, 5), (1, 4, 4, 32, 1, 3),
                (2, 3, 4, 32, 1, 1)]


@pytest.mark.parametrize("num,h,w,c,kh,kw", IM2COL_CASES)
def test_im2col_pair_bits(num, h, w, c, kh, kw):
    xp = _maps(num, h, w, c, 600 + h * w)
    got = C().im2col_pair(dev_pair(xp), h, w, kh, kw)
    want = R.im2col_pair(xp, num, h, w, kh, kw)
    assert np.array_equal(host_bits16(got), want)
    # no tap carries another map's values: every non-zero hi of map r has map r's exponent
    hi, _ = R.unpair(want)
    expo = (hi.reshape(num, -1) >> 7) & 0xFF
    for r in range(num):
        assert set(np.unique(expo[r])) <= {0, 127 + 2 * r}


def test_im2col_pair_bits_beyond_one_grid_pass():
    num, h, w, c = 3, 70, 70, 32
    assert _beyond(num * h * w * 9 * (c // 4), PASS_16)
    xp = _maps(num, h, w, c, 610)
    got = C().im2col_pair(dev_pair(xp), h, w, 3, 3)
    assert np.array_equal(host_bits16(got), R.im2col_pair(xp, num, h, w, 3, 3))


def test_im2col_pair_refusals():
    L = C()._L
    s = _stream()
    src = torch.zeros((12, 128), dtype=torch.bfloat16, device="cuda")
    dst = torch.zeros((12, 9 * 128), dtype=torch.bfloat16, device="cuda")
    assert L.ovis_im2col_pair(src.data_ptr(), dst.data_ptr(), 1, 3, 4, 64, 2, 3, s) == OVIS_EINVAL     # even kh
    assert L.ovis_im2col_pair(src.data_ptr(), dst.data_ptr(), 1, 3, 4, 64, 3, 2, s) == OVIS_EINVAL     # even kw
    assert L.ovis_im2col_pair(src.data_ptr(), dst.data_ptr(), 1, 3, 4, 48, 3, 3, s) == OVIS_ERANGE     # C % 32
    assert L.ovis_im2col_pair(src.data_ptr() + 8, dst.data_ptr(), 1, 3, 4, 32, 3, 3, s) == OVIS_ERANGE
    assert L.ovis_im2col_pair(0, dst.data_ptr(), 1, 3, 4, 64, 3, 3, s) == OVIS_EINVAL
    assert L.ovis_im2col_pair(src.data_ptr(), dst.data_ptr(), 0, 3, 4, 64, 3, 3, s) == OVIS_OK
    torch.cuda.synchronize()
    assert not host_bits16(dst).any()


# ------------------------------------------------------------------ slab_reduce
SENTINEL = 3.0e37


def _slab_check(s, n, c, t, scaled, seed):
    """Slabs beyond S in the same allocation hold a large sentinel: the predicated loads of the last group of 8 read none."""
    slabs = R.slab_values(s, n, t * c, seed)
    sc = np.random.default_rng(seed + 1).uniform(-2.0, 2.0, size=n).astype(np.float32) if scaled else None
    if sc is not None:
        sc[0], sc[n - 1] = 0.5, 1.0
    extra = 8
    alloc = torch.full((s + extra, n, t * c), SENTINEL, device="cuda")
    alloc[:s] = dev(slabs)
    dw = torch.full((n, c, t), -1.0, device="cuda")
    scd = None if sc is None else dev(sc)
    rc = C()._L.ovis_slab_reduce_f32(alloc.data_ptr(), C()._ptr(scd), dw.data_ptr(), s, n, c, t, _stream())
    assert rc == OVIS_OK
    got = dw.cpu().numpy()
    want = R.slab_reduce(slabs, sc, n, c, t)
    bad = got != want                                                  # as values: -0 == +0; no NaN in these inputs
    assert not bad.any(), _report(bad, got.view(np.uint32), want.view(np.uint32), f"slab_reduce S={s}")
    val, bound = R.slab_reduce_bound(slabs, sc, n, c, t)
    assert (np.abs(got.astype(np.float64) - val) <= bound).all()


@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("n,c,t", [(8, 8, 1), (4, 12, 9)])
@pytest.mark.parametrize("s", [1, 2, 3, 4, 5, 8, 31, 32, 33, 36, 64, 65, 256])
def test_slab_reduce_equals_the_fixed_tree(s, n, c, t, scaled):
    _slab_check(s, n, c, t, scaled, 700 + s)


def test_slab_reduce_beyond_one_grid_pass():
    n, c, t = 128, 512, 9
    assert _beyond(4 * n * t * (c // 4), PASS_8)
    _slab_check(3, n, c, t, True, 710)


def test_slab_reduce_refusals():
    L = C()._L
    s = _stream()
    slabs = torch.zeros(4 * 8 * 8 + 4, device="cuda")
    dw = torch.full((8, 8, 1), 5.0, device="cuda")
    assert L.ovis_slab_reduce_f32(slabs.data_ptr() + 4, 0, dw.data_ptr(), 4, 8, 8, 1, s) == OVIS_ERANGE   # slabs misaligned
    assert L.ovis_slab_reduce_f32(slabs.data_ptr(), 0, dw.data_ptr(), 4, 8, 6, 1, s) == OVIS_ERANGE       # C % 4
    assert L.ovis_slab_reduce_f32(slabs.data_ptr(), 0, dw.data_ptr(), 0, 8, 8, 1, s) == OVIS_EINVAL
    assert L.ovis_slab_reduce_f32(0, 0, dw.data_ptr(), 4, 8, 8, 1, s) == OVIS_EINVAL
    assert L.ovis_slab_reduce_f32(slabs.data_ptr(), 0, 0, 4, 8, 8, 1, s) == OVIS_EINVAL
    torch.cuda.synchronize()
    assert (dw == 5.0).all()


# ------------------------------------------------------------------ closing the chain
@pytest.mark.parametrize("m,k,n", [(300, 64, 64), (777, 128, 256)])
def test_gemm_pair_epilogue_is_the_reference_split_of_its_fp32_output(m, k, n):
    """The fused pair output of a GEMM epilogue equals the HOST split of the fp32 output of the same launch: the existing
    ``torch.equal(cp, C.split_pair(c))`` assertions, and split_pair itself (above), end on the same reference."""
    rng = np.random.default_rng(800 + m)
    a = rng.standard_normal((m, k)).astype(np.float32)
    b = (rng.standard_normal((n, k)) * 0.1).astype(np.float32)
    bias = rng.standard_normal(n).astype(np.float32)
    c, cp = C().split_gemm_pair(dev_pair(R.pair_rows(a)), dev_pair(R.pair_rows(b)), dev(bias), None, True, True, True)
    ch = c.cpu().numpy()
    assert (ch == 0).any() and (ch > 0).any()                          # the ReLU is at work
    assert_pair_bits(cp, R.pair_rows(ch), "split_gemm_pair pair epilogue")
