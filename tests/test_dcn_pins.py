"""CPU pins of oracle/dcn.py: the vectorised fp64 oracle (forward, and autograd of it as the backward) against the scalar
restatement of the reference's CUDA kernels in tests/dcn_scalar_reference.py, whose backward restates the hand-written
col2im / col2im_coord / PS-RoI accumulation kernels.  Two offset families per case: smooth (N(0, 1.5^2)) and grid (multiples
of 0.25 in [-4, 4]: every sampling position is exactly representable, many lie on integer rows / columns and some exactly
on the border lines -1, H, W of the inside rule).  Both sides are fp64 sums of at most a few hundred terms of order one:
the bound is 1e-10 of the maximum of the expected tensor, as in tests/test_dcn.py; sample counts must match exactly."""
import numpy as np
import pytest
import torch

from oracle import dcn as O

from . import dcn_scalar_reference as R

TOL = 1e-10

CASES = {
    # the parameter sets of the GPU tests in tests/test_dcn.py, scaled down
    "default": dict(),
    "stride2_pad2_dil2": dict(H=8, W=9, stride=2, pad=2, dil=2),
    "groups2_dg2": dict(C=8, Cout=4, H=5, W=6, groups=2, dg=2),
    "b3_1x1": dict(B=3, C=4, Cout=5, H=7, W=6, k=1, pad=0),
    "b4_dg3": dict(B=4, C=6, Cout=6, H=6, W=5, dg=3),
    "dg2_stride2_pad2_dil2": dict(C=8, Cout=4, H=8, W=9, dg=2, stride=2, pad=2, dil=2),
    "b3_1x1_dg3": dict(B=3, C=6, Cout=4, H=7, W=6, k=1, pad=0, dg=3),
    "b1_wide_out": dict(B=1, C=2, Cout=7, H=8, W=9),
    "dg2_stride2": dict(C=8, Cout=4, H=6, W=7, dg=2, stride=2),
    # further shapes
    "k3x5_unequal_pad": dict(H=6, W=8, k=(3, 5), pad=(2, 1)),
    "groups2_dg1": dict(C=4, Cout=6, H=5, W=6, groups=2),
    "b3": dict(B=3, C=2, Cout=2, H=5, W=5),
}


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _make(seed, family, B=2, C=4, Cout=3, H=6, W=7, k=3, stride=1, pad=1, dil=1, groups=1, dg=1):
    g = torch.Generator().manual_seed(seed)
    (kh, kw), st, pd, dl = _pair(k), _pair(stride), _pair(pad), _pair(dil)
    Ho = (H + 2 * pd[0] - (dl[0] * (kh - 1) + 1)) // st[0] + 1
    Wo = (W + 2 * pd[1] - (dl[1] * (kw - 1) + 1)) // st[1] + 1
    f64 = torch.float64
    x = torch.randn(B, C, H, W, generator=g, dtype=f64)
    w = torch.randn(Cout, C // groups, kh, kw, generator=g, dtype=f64) * 0.2
    if family == "grid":
        off = torch.randint(-16, 17, (B, dg * 2 * kh * kw, Ho, Wo), generator=g).to(f64) * 0.25
    else:
        off = torch.randn(B, dg * 2 * kh * kw, Ho, Wo, generator=g, dtype=f64) * 1.5
    mask = torch.sigmoid(torch.randn(B, dg * kh * kw, Ho, Wo, generator=g, dtype=f64))
    bias = torch.randn(Cout, generator=g, dtype=f64)
    go = torch.randn(B, Cout, Ho, Wo, generator=g, dtype=f64)
    return dict(x=x, w=w, off=off, mask=mask, bias=bias, go=go, args=dict(stride=st, padding=pd, dilation=dl, groups=groups,
                                                                         deformable_groups=dg))


def _close(name, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, name
    err, scale = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert err <= TOL * scale, f"{name}: |oracle - scalar reference| = {err:.3e} > {TOL:g} * {scale:.3e}"


def _check_conv(c, modulated):
    """Oracle forward + autograd against the scalar forward + hand-written backward; `want` is the scalar reference."""
    a = c["args"]
    leaves = {n: c[n].clone().requires_grad_(True) for n in ("x", "w", "off", "mask", "bias")}
    out = O.deform_conv2d(leaves["x"], leaves["off"], leaves["w"], leaves["mask"] if modulated else None,
                          leaves["bias"] if modulated else None, a["stride"], a["padding"], a["dilation"], a["groups"],
                          a["deformable_groups"])
    out.backward(c["go"])
    np_ = {n: c[n].numpy() for n in ("x", "w", "off", "mask", "bias", "go")}
    want, _ = R.deform_conv_forward(np_["x"], np_["off"], np_["w"], np_["mask"] if modulated else None,
                                    np_["bias"] if modulated else None, **a)
    grads = R.deform_conv_backward(np_["x"], np_["off"], np_["w"], np_["go"], np_["mask"] if modulated else None, **a)
    _close("forward", out.detach().numpy(), want)
    _close("dX", leaves["x"].grad.numpy(), grads["x"])
    _close("dWeight", leaves["w"].grad.numpy(), grads["weight"])
    _close("dOffset", leaves["off"].grad.numpy(), grads["offset"])
    if modulated:
        _close("dMask", leaves["mask"].grad.numpy(), grads["mask"])
        _close("dBias", leaves["bias"].grad.numpy(), grads["bias"])
    return want, grads


def _edge_counts(c):
    """(samples with an integer row or column coordinate, samples exactly on one of the lines -1, H, W)."""
    H, W = c["x"].shape[2:]
    a = c["args"]
    hs, ws = R.sample_positions(c["off"].numpy(), c["w"].shape, c["x"].shape, a["stride"], a["padding"], a["dilation"],
                                a["deformable_groups"])
    on_line = (hs == np.floor(hs)) | (ws == np.floor(ws))
    on_border = (hs == -1) | (hs == H) | (ws == -1) | (ws == W)
    return int(on_line.sum()), int(on_border.sum())


@pytest.mark.parametrize("modulated", [False, True], ids=["v1", "v2"])
@pytest.mark.parametrize("family", ["smooth", "grid"])
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_deform_conv_vs_scalar_reference(name, family, modulated):
    c = _make(100 + list(CASES).index(name), family, **CASES[name])
    if family == "grid":
        on_line, on_border = _edge_counts(c)
        assert on_line > 0 and on_border > 0, (on_line, on_border)   # the grid family must keep exercising the edges
    _check_conv(c, modulated)


def test_grid_family_reaches_every_border_line():
    """Across the grid cases, samples sit exactly on each of the four lines of the inside rule (-1 and H for rows, -1 and W
    for columns) and exactly on the last row / column H - 1 / W - 1 and on 0, where the per-corner rule decides."""
    hit = dict(h_m1=0, h_H=0, w_m1=0, w_W=0, h_0=0, h_last=0, w_0=0, w_last=0)
    for i, (name, kw) in enumerate(CASES.items()):
        c = _make(100 + i, "grid", **kw)
        H, W = c["x"].shape[2:]
        a = c["args"]
        hs, ws = R.sample_positions(c["off"].numpy(), c["w"].shape, c["x"].shape, a["stride"], a["padding"], a["dilation"],
                                    a["deformable_groups"])
        for key, n in (("h_m1", hs == -1), ("h_H", hs == H), ("w_m1", ws == -1), ("w_W", ws == W), ("h_0", hs == 0),
                       ("h_last", hs == H - 1), ("w_0", ws == 0), ("w_last", ws == W - 1)):
            hit[key] += int(n.sum())
    assert all(v > 0 for v in hit.values()), hit


@pytest.mark.parametrize("family", ["smooth", "grid"])
def test_oracle_mask_with_exact_zeros(family):
    """Taps whose mask is exactly 0: no contribution to the output, to dX or to dOffset (the reference multiplies the
    column gradient by the mask), while dMask there is still the sampled value times the column gradient."""
    c = _make(7, family, C=4, Cout=3, H=5, W=6, dg=2)
    g = torch.Generator().manual_seed(8)
    zero = torch.rand(c["mask"].shape, generator=g) < 0.4
    c["mask"] = torch.where(zero, torch.zeros_like(c["mask"]), c["mask"])
    assert int(zero.sum()) > 0
    _, grads = _check_conv(c, True)
    B, _, Ho, Wo = c["mask"].shape
    doff = grads["offset"].reshape(B, 2, 9, 2, Ho, Wo)
    z = zero.numpy().reshape(B, 2, 9, Ho, Wo)
    assert float(np.abs(doff[:, :, :, 0][z]).max()) == 0.0 and float(np.abs(doff[:, :, :, 1][z]).max()) == 0.0
    assert float(np.abs(grads["mask"].reshape(B, 2, 9, Ho, Wo)[z]).max()) > 0.0


@pytest.mark.parametrize("modulated", [False, True], ids=["v1", "v2"])
def test_oracle_image_with_every_sample_outside(modulated):
    """Offsets that push every sample of image 1 outside the map (exactly representable: +/- 64 plus the grid family):
    its output is the bias (0 for v1) and its dX, dOffset and dMask are zero, in the scalar reference and in the oracle."""
    c = _make(9, "grid", B=3, C=4, Cout=3, H=5, W=6, dg=2)
    sign = torch.where(torch.rand(c["off"][1].shape, generator=torch.Generator().manual_seed(10)) < 0.5, -1.0, 1.0)
    c["off"][1] = c["off"][1] + 64.0 * sign.to(torch.float64)
    want, grads = _check_conv(c, modulated)
    expect = c["bias"].numpy().reshape(-1, 1, 1) if modulated else 0.0
    assert float(np.abs(want[1] - expect).max()) == 0.0
    for n in ("x", "offset") + (("mask",) if modulated else ()):
        assert float(np.abs(grads[n][1]).max()) == 0.0, n
        assert float(np.abs(grads[n][0]).max()) > 0.0 and float(np.abs(grads[n][2]).max()) > 0.0, n


# ---------------------------------------------------------------- deformable position-sensitive RoI pooling
def _check_pool(data, rois, trans, scale, P, od, no_trans, gs, ps, spp, std, seed=5):
    part = P if ps is None else ps
    d0 = data.clone().requires_grad_(True)
    t0 = None if no_trans else trans.clone().requires_grad_(True)
    out, cnt = O.deform_psroi_pool(d0, rois, t0, scale, P, od, no_trans, gs, ps, spp, std)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    got = torch.autograd.grad(out, [d0] if no_trans else [d0, t0], go)
    tn = None if no_trans else trans.numpy()
    want, want_cnt = R.psroi_forward(data.numpy(), rois.numpy(), tn, scale, P, od, no_trans, gs, part, spp, std)
    dd, dt = R.psroi_backward(go.numpy(), want_cnt, data.numpy(), rois.numpy(), tn, scale, P, od, no_trans, gs, part, spp, std)
    assert np.array_equal(cnt.numpy(), want_cnt), "sample counts"
    _close("pooled", out.detach().numpy(), want)
    _close("dData", got[0].numpy(), dd)
    if not no_trans:
        assert got[1].dtype == torch.float64
        _close("dTrans", got[1].numpy(), dt)
    return want, want_cnt, dd, dt


def _pool_case(seed, n, od, gs, P, ps=None, H=7, W=9, classes=1, B=2):
    g = torch.Generator().manual_seed(seed)
    data = torch.randn(B, od * gs * gs, H, W, generator=g, dtype=torch.float64)
    xy = torch.rand(n, 2, generator=g) * torch.tensor([W * 8.0, H * 8.0])
    wh = torch.rand(n, 2, generator=g) * 40 + 10
    rois = torch.cat([torch.randint(0, B, (n, 1), generator=g).float(), xy, xy + wh], 1)
    ps = P if ps is None else ps
    trans = (torch.randn(n, 2 * classes, ps, ps, generator=g) * 0.5).double()   # float32 values: the geometry is float32
    return data, rois, trans


@pytest.mark.parametrize("kw", [dict(no_trans=True, gs=1, P=3, od=3), dict(no_trans=False, gs=2, P=4, od=4, classes=2),
                                dict(no_trans=False, gs=1, P=6, od=3, classes=3, ps=3, spp=2),
                                dict(no_trans=False, gs=3, P=3, od=2, classes=1, std=1.0, far=True)],
                         ids=["no_trans", "gs2_classes2", "part3_spp2", "gs3_std1_far"])
def test_oracle_psroi_pool_vs_scalar_reference(kw):
    """The parameter sets of test_deform_psroi_pooling_vs_oracle at smaller sizes; with `far`, RoIs wholly and partly
    outside the map (count 0 -> output 0 and no gradient)."""
    no_trans, gs, P, od = kw["no_trans"], kw["gs"], kw["P"], kw["od"]
    classes, ps, spp, std = kw.get("classes", 1), kw.get("ps"), kw.get("spp", 4), kw.get("std", 0.1)
    data, rois, trans = _pool_case(od + P, 5, od, gs, P, ps, classes=classes)
    if kw.get("far"):
        rois[0, 1:] = torch.tensor([900.0, 900.0, 980.0, 990.0])   # wholly outside the 9x7 map (scale 1/8)
        rois[1, 1:] = torch.tensor([-60.0, -40.0, 30.0, 20.0])     # partly outside
        rois[2, 1:] = torch.tensor([40.0, 30.0, 130.0, 90.0])      # partly outside, the far side
    want, cnt, dd, dt = _check_pool(data, rois, trans, 0.125, P, od, no_trans, gs, ps, spp, std)
    if kw.get("far"):
        assert cnt[0].sum() == 0 and float(np.abs(want[0]).max()) == 0.0 and float(np.abs(dt[0]).max()) == 0.0
        assert 0 < cnt[1].sum() < cnt[1].size * spp * spp and 0 < cnt[2].sum() < cnt[2].size * spp * spp
    else:
        assert cnt.max() == spp * spp


def _boundary_pool_case():
    """RoIs of exactly the map's extent (start -0.5, width 8 = W, height 4 = H at scale 1/4) with P = 2, 4 samples per
    part (sub-bin 1 cell in x, 0.5 in y) and trans_std 1/8, so that a trans of t shifts a bin by exactly t cells in x and
    0.5 t in y: with t a multiple of 0.5 every position is exact in float32, and samples land exactly on -0.5 and W - 0.5
    (the inside test), on 0 and W - 1 (the clamp), and beyond both."""
    g = torch.Generator().manual_seed(21)
    H, W, n = 4, 8, 6
    data = torch.randn(2, 3 * 2 * 2, H, W, generator=g, dtype=torch.float64)
    rois = torch.tensor([[0, 0.0, 0.0, 31.0, 15.0]]).repeat(n, 1)
    rois[:, 0] = torch.randint(0, 2, (n,), generator=g).float()
    trans = torch.randint(-4, 5, (n, 2 * 3, 2, 2), generator=g).double() * 0.5
    trans[0] = 0.0                                         # the unshifted RoI: first samples exactly on -0.5
    return data, rois, trans, dict(scale=0.25, P=2, od=3, gs=2, spp=4, std=0.125)


def test_oracle_psroi_pool_on_the_boundary():
    data, rois, trans, p = _boundary_pool_case()
    H, W = data.shape[2:]
    ws, hs = R.psroi_positions(data.shape, rois.numpy(), trans.numpy(), p["scale"], p["P"], p["od"], False, p["gs"], p["P"],
                               p["spp"], p["std"])
    hits = {"-0.5": int((ws == -0.5).sum()), "W-0.5": int((ws == W - 0.5).sum()), "0": int((ws == 0).sum()),
            "W-1": int((ws == W - 1).sum()), "below": int((ws < -0.5).sum()), "above": int((ws > W - 0.5).sum()),
            "h=-0.5": int((hs == -0.5).sum()), "H-0.5": int((hs == H - 0.5).sum()), "h=0": int((hs == 0).sum()),
            "H-1": int((hs == H - 1).sum())}
    assert all(v > 0 for v in hits.values()), hits
    _, cnt, _, _ = _check_pool(data, rois, trans, p["scale"], p["P"], p["od"], False, p["gs"], None, p["spp"], p["std"])
    assert cnt.min() < cnt.max() == p["spp"] ** 2   # bins with every sample counted, and bins that lost some
