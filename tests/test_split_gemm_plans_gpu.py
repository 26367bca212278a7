"""GPU: every way ``split_gemm_plan`` (csrc/split_gemm.hip) cuts K into slices, and the sliced epilogue of
``split_gemm_finish_kernel``, against fp64 -- the under-filled-grid rule, the co-scheduled rule (config bit 16, what
``_C.co_scheduled()`` turns on), the fitted cost model, forced slice counts (config bits 8..15), each with one and two LDS
stages on the PLAIN, SHIFTED, HALO and narrow kernels; the no-workspace fallback of the launcher; exactness under a
power-of-two scaling of the operands; row-strided operands.

The slice count of a launch is READ from the library (``slices``: the workspace query is the only window onto the plan);
nothing here restates the plan.  The fp64 bound has NO floor:

    |got - ref| <= TOL * (sum_k |a_k||b_k| + |bias| + |residual|)     elementwise, TOL = 2e-5

(the constant derived in tests/test_split_gemm_pair.py: the three-term bf16 hi/lo product drops lo.lo and rounds lo to 8
bits, ~4e-6 per term), so a kernel that is wrong by an absolute amount, or on small magnitudes, fails.  The 1e-30 in the
printed ratio only keeps 0 / 0 (exact-zero operand rows) finite.  Every test prints case, config, slice count and its worst
error / bound (run with ``-s``).

Largest measured error / bound per section on an MI355X (fp64 reference, floor-free bound):
  1  forced slice counts                 0.113  (PLAIN with a2_pair, 3 slices across the A | A2 seam; the others 0.04 .. 0.08)
  2  the plan's own choices              0.080  (1100 x 512 x 2048, un-sliced, also the dual rp_gated kernel; sliced cases 0.02 .. 0.05)
  2  identity backward, co-scheduled     0.672  (dw3, one product: conv2 output channels that are almost never positive leave
                                                 sums of a few terms, where the per-term error does not average out: the worst
                                                 entry has 11 non-zero rows of 8400, the kernel is within 0.008 of the three-term
                                                 hi/lo sum there, and channels with > 2100 non-zero rows stay below 0.053); relative
                                                 L2 error of gx / dw1 / dw2 / dw3 = 0.24 / 0.39 / 0.30 / 0.22 of TOL
  3  no-workspace fallback               bit-identical to config 8; sliced run with the full workspace 0.039
  4  power-of-two scaling                bit-identical at 2^-20 and 2^20, all six forms; zero rows give exactly
                                         act(bias + residual), the other entries 0.038
  5  row-strided operands                bit-identical to contiguous copies; 0.044 against fp64
One and two LDS stages were bit-identical wherever compared.  No kernel missed a check.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 2e-5
CO = 0x10000      # config bit 16: what ``_C.co_scheduled()`` ORs in
OVIS_OK = 0


def _C():
    from cvpr22_cross_modal_pseudo_labeling_amd import _C as c
    return c


def slices(m, n, ch, ch2, kh, kw, w, cfg):
    """The number of K slices the library's plan gives this launch (1: un-sliced)."""
    nbytes = int(_C()._L.ovis_split_gemm_pair_workspace_bytes_ex(m, n, ch, ch2, kh, kw, w, cfg))
    return nbytes // (4 * m * n) if nbytes else 1


def _recut(units, s):
    """min(s, units) slices re-cut the library's way: slices of ceil(units / s) units, the last one shorter or dropped."""
    s = min(s, units)
    return -(-units // -(-units // s))


def _rec(pair):
    """hi + lo of pair rows as fp32 (exact)."""
    rows, c2 = pair.shape
    v = pair.reshape(rows, c2 // 64, 2, 32).float()
    return (v[:, :, 0] + v[:, :, 1]).reshape(rows, c2 // 2).contiguous()


def _cols64(x, geom):
    """Tap-major fp64 patch rows [m, 9 * c] of the NHWC rows x [r * h * w, c] (3x3, zero padding)."""
    r, h, w = geom
    c = x.shape[1]
    cols = F.unfold(x.view(r, h, w, c).permute(0, 3, 1, 2).double(), (3, 3), padding=1)
    return cols.view(r, c, 9, h * w).permute(0, 3, 2, 1).reshape(r * h * w, 9 * c)


class _Problem:
    """Operands of one product (fp32 values, pair forms) with its fp64 value and its fp64 magnitude sum_k |a_k||b_k|."""

    def __init__(self, name, m, ch, n, seed, geom=None, flip=False, ch2=0, b_scale=1.0):
        C = _C()
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.name, self.m, self.ch, self.n, self.ch2, self.geom, self.flip = name, m, ch, n, ch2, geom, flip
        taps = 1 if geom is None else 9
        self.a = torch.randn(m, ch, device="cuda", generator=g)
        self.a2 = torch.randn(m, ch2, device="cuda", generator=g) if ch2 else None
        self.b = torch.randn(n, taps * ch + ch2, device="cuda", generator=g) * b_scale
        self.bias = torch.randn(n, device="cuda", generator=g)
        self.res = torch.randn(m, n, device="cuda", generator=g)
        self.y = torch.randn(m, n, device="cuda", generator=g).clamp(min=0)   # a forward activation: the gate
        self.ap, self.bp = C.split_pair(self.a), C.split_pair(self.b)
        self.a2p = C.split_pair(self.a2) if ch2 else None
        self.conv = None if geom is None else (geom[1], geom[2], 3, 3, flip)
        self.units = taps * ch // 32 + ch2 // 32                               # SHIFTED / PLAIN; the HALO form counts ch / 32
        self._ref = None

    def reference(self):
        if self._ref is None:
            if self.geom is None:
                lhs = self.a.double() if self.a2 is None else torch.cat([self.a, self.a2], 1).double()
                rhs = self.b.double()
            else:
                lhs = _cols64(self.a, self.geom)
                # flip negates the tap offsets: the taps of the weight matrix in reverse order
                rhs = (self.b.view(self.n, 9, self.ch).flip(1).reshape(self.n, -1) if self.flip else self.b).double()
            self._ref = (lhs @ rhs.t(), lhs.abs() @ rhs.abs().t())
        return self._ref

    def width(self):
        return 0 if self.geom is None else self.geom[2]

    def slices(self, cfg):
        return slices(self.m, self.n, self.ch, self.ch2, 1 if self.geom is None else 3, 1 if self.geom is None else 3,
                      self.width(), cfg)

    def run(self, cfg, bias=False, res=None, relu=False, out_f32=True, out_pair=True, co=False):
        """res: None, "f32" or "pair"."""
        C = _C()
        kw = {}
        if res == "pair":
            kw["residual_pair"] = C.split_pair(self.res)
        with C.co_scheduled(co):
            return C.split_gemm_pair(self.ap, self.bp, self.bias if bias else None, self.res if res == "f32" else None, relu,
                                     out_f32, out_pair and self.n % 32 == 0, conv=self.conv, config=cfg, a2_pair=self.a2p, **kw)

    def run_gated(self, cfg, out_f32=True, out_pair=True, co=False):
        C = _C()
        with C.co_scheduled(co):
            return C.split_gemm_pair_gated(self.ap, self.bp, C.split_pair(self.y), conv=self.conv, out_f32=out_f32,
                                           out_pair=out_pair, config=cfg)

    def ratio(self, got, bias=False, res=None, relu=False, gated=False):
        """Largest |got - ref| / (TOL * bound) of the floor-free bound."""
        ref, bound = (t.clone() for t in self.reference())
        if bias:
            ref += self.bias.double()
            bound += self.bias.abs().double()
        if res is not None:
            r = self.res if res == "f32" else _rec(_C().split_pair(self.res))
            ref += r.double()
            bound += r.abs().double()
        if relu:
            ref.clamp_(min=0)
        if gated:
            ref *= self.y > 0
        return ((got.double() - ref).abs() / (TOL * bound + 1e-30)).max().item()


@functools.lru_cache(maxsize=None)
def _problem(*args, **kw):
    return _Problem(*args, **kw)


_WORST = {}


def _epi_name(epi):
    parts = (["bias"] if epi.get("bias") else []) + ([epi["res"] + " residual"] if epi.get("res") else []) + (["relu"] if epi.get("relu") else [])
    return " + ".join(parts) or "no epilogue operand"


def _note(section, label, cfg, ns, ratio):
    _WORST[section] = max(_WORST.get(section, 0.0), ratio)
    print(f"[{section}] {label} config={cfg:#x} slices={ns} err/bound={ratio:.3f}  (worst of section {section} so far "
          f"{_WORST[section]:.3f})")


# ---------------------------------------------------------------------------------------------------------------------
# 1. forced slice counts (config bits 8..15), with bits 1 / 2 (one / two LDS stages) ORed in
# ---------------------------------------------------------------------------------------------------------------------
_FORCED = {
    # name: (problem arguments, config bits ORed into every launch, units a slice is counted in, forced counts, epilogue)
    "plain-333x1024x192": (dict(m=333, ch=1024, n=192, seed=11), 0, 32, (2, 3, 5, 7, 32, 200), dict(bias=True, res="f32", relu=True)),
    "plain-a2-490x(160+96)x256": (dict(m=490, ch=160, n=256, seed=12, ch2=96), 0, 8, (3,), dict(bias=True, relu=True)),
    "shifted-5x7x7x96-128": (dict(m=245, ch=96, n=128, seed=13, geom=(5, 7, 7)), 4, 27, (2, 4, 5, 27), dict(bias=True, relu=True)),
    "shifted-flip-5x7x7x96-128": (dict(m=245, ch=96, n=128, seed=14, geom=(5, 7, 7), flip=True), 4, 27, (2, 4, 5, 27), dict()),
    "halo-37x7x7x160-192": (dict(m=37 * 49, ch=160, n=192, seed=15, geom=(37, 7, 7)), 0, 5, (2, 3, 5, 9), dict(bias=True, relu=True)),
}


@pytest.mark.parametrize("name", list(_FORCED))
def test_forced_slice_counts_vs_fp64(name):
    """``config = s << 8`` cuts K into min(s, units) slices re-cut to equal length (s above units is clamped; the SHIFTED
    slices start mid-tap, 3 channel blocks per tap; the HALO slices count channel blocks and walk every tap; the a2 case has
    a slice across the A | A2 seam): each within the floor-free fp64 bound, within the sliced-equals-un-sliced margin
    1e-5 * max|y| of the ``config = 8`` result, pair output == split_pair(fp32 output), and -- same k order per workgroup --
    one and two LDS stages bit-identical."""
    C = _C()
    args, base, units, counts, epi = _FORCED[name]
    P = _problem(name, **args)
    assert units == (P.ch // 32 if name.startswith("halo") else P.units)
    y8, _ = P.run(8 | base, **epi)
    scale8 = y8.abs().max().item()
    assert P.ratio(y8, **epi) <= 1.0
    for s in counts:
        ns = P.slices((s << 8) | base)
        assert ns == _recut(units, s), (name, s, ns)
        outs = []
        for stage in (0, 1, 2):
            cfg = (s << 8) | base | stage
            assert P.slices(cfg) == ns
            y, yp = P.run(cfg, **epi)
            ratio = P.ratio(y, **epi)
            _note(1, name, cfg, ns, ratio)
            assert ratio <= 1.0, (name, hex(cfg), ratio)
            assert (y - y8).abs().max().item() <= 1e-5 * scale8, (name, hex(cfg))
            assert torch.equal(yp, C.split_pair(y)), (name, hex(cfg))
            outs.append(y)
        assert torch.equal(outs[1], outs[2]), (name, s, "one stage != two stages")


def test_forced_slice_counts_ignored_by_the_narrow_kernel():
    """n = 64 runs the 64-column kernels, which have no sliced form: the plan ignores bits 8..15."""
    P = _problem("narrow-300x256x64", m=300, ch=256, n=64, seed=16)
    assert P.units == 8 and P.slices(4 << 8) == 1 and P.slices(0) == 1
    epi = dict(bias=True, res="f32", relu=True)
    y8, y8p = P.run(8, **epi)
    y, yp = P.run(4 << 8, **epi)
    ratio = P.ratio(y, **epi)
    _note(1, P.name, 4 << 8, 1, ratio)
    assert ratio <= 1.0
    assert torch.equal(y, y8) and torch.equal(yp, y8p) and torch.equal(yp, _C().split_pair(y))


def test_finish_kernel_epilogues_at_a_ragged_forced_count():
    """Every epilogue of ``split_gemm_finish_kernel`` on slices of 11, 11 and 10 units (PLAIN) or 7, 7, 7 and 6 (SHIFTED):
    bias + fp32 residual + ReLU, the residual in pair layout, the ReLU gate of a data gradient, and pair-only output."""
    C = _C()
    P = _problem("plain-333x1024x192", **_FORCED["plain-333x1024x192"][0])
    cfg = 3 << 8
    assert P.slices(cfg) == 3 and P.units % 11 != 0
    for epi in (dict(bias=True, res="f32", relu=True), dict(bias=True, res="pair", relu=True), dict(res="pair")):
        y, yp = P.run(cfg, **epi)
        ratio = P.ratio(y, **epi)
        _note(1, f"{P.name} {_epi_name(epi)}", cfg, 3, ratio)
        assert ratio <= 1.0, epi
        assert torch.equal(yp, C.split_pair(y))
        none, only_p = P.run(cfg, out_f32=False, **epi)
        assert none is None and torch.equal(only_p, yp)
        y8, _ = P.run(8, **epi)
        assert (y - y8).abs().max().item() <= 1e-5 * y8.abs().max().item()
    for Q, cfg, ns in ((P, 3 << 8, 3), (_problem("shifted-flip-5x7x7x96-128", **_FORCED["shifted-flip-5x7x7x96-128"][0]), (4 << 8) | 4, 4)):
        assert Q.slices(cfg) == ns
        y, yp = Q.run_gated(cfg)
        ratio = Q.ratio(y, gated=True)
        _note(1, f"{Q.name} gate", cfg, ns, ratio)
        assert ratio <= 1.0
        assert torch.equal(yp, C.split_pair(y)) and not y[Q.y == 0].any()
        none, only_p = Q.run_gated(cfg, out_f32=False)
        assert none is None and torch.equal(only_p, yp)
        # the gate applied by the finish kernel == the plain sliced product gated afterwards
        d, _ = Q.run(cfg, out_pair=False)
        want_p, want = C.gate_split_pair(d, C.split_pair(Q.y), want_f32=True)
        assert torch.equal(y, want) and torch.equal(yp, want_p)


# ---------------------------------------------------------------------------------------------------------------------
# 2. the plan's own choices, co-scheduled and not
# ---------------------------------------------------------------------------------------------------------------------
_CHOICES = {
    "plain-1100x512x2048": dict(m=1100, ch=512, n=2048, seed=21),
    "plain-1100x1024x2048": dict(m=1100, ch=1024, n=2048, seed=22),
    "plain-1100x2048x2048": dict(m=1100, ch=2048, n=2048, seed=23),
    "plain-1357x1536x2048": dict(m=1357, ch=1536, n=2048, seed=24),
    "plain-5453x768x384": dict(m=5453, ch=768, n=384, seed=25),
    "3x3-flip-2x50x84x256-256": dict(m=2 * 50 * 84, ch=256, n=256, seed=26, geom=(2, 50, 84), flip=True, b_scale=0.05),
    "3x3-1x50x84x128-512": dict(m=50 * 84, ch=128, n=512, seed=27, geom=(1, 50, 84), b_scale=0.05),
    "3x3-15x20x24x768-384": dict(m=15 * 480, ch=768, n=384, seed=28, geom=(15, 20, 24), b_scale=0.05),
    "3x3-15x20x24x1024-384": dict(m=15 * 480, ch=1024, n=384, seed=29, geom=(15, 20, 24), b_scale=0.05),
    "plain-4200x4096x1024": dict(m=4200, ch=4096, n=1024, seed=30),
}


def _choice_counts(cfg):
    """(slice count, the last slice is shorter than the others) per case, read from the library."""
    out = {}
    for name, args in _CHOICES.items():
        taps = 1 if args.get("geom") is None else 3
        ns = slices(args["m"], args["n"], args["ch"], 0, taps, taps, args["geom"][2] if taps == 3 else 0, cfg)
        units = taps * taps * args["ch"] // 32
        out[name] = (ns, ns > 1 and units % -(-units // ns) != 0)
    return out


def test_plan_choices_cover_every_slice_count():
    """Coverage of the cases below, not a measurement: the plan's own choice (config 0) reaches 1, 2, 3, 4 and 8 slices with
    at least one ragged cut, the co-scheduled rule 1, 2 and 4."""
    own, co = _choice_counts(0), _choice_counts(CO)
    for name in _CHOICES:
        print(f"[2] {name}: config 0 -> {own[name][0]} slices{' (ragged)' if own[name][1] else ''}, co-scheduled -> "
              f"{co[name][0]}{' (ragged)' if co[name][1] else ''}")
    hint = "the cost model was retuned: re-pick shapes so every slice count is exercised"
    assert {1, 2, 3, 4, 8} <= {ns for ns, _ in own.values()}, (hint, own)
    assert any(ragged for _, ragged in own.values()), (hint, own)
    assert {1, 2, 4} <= {ns for ns, _ in co.values()}, (hint, co)


@pytest.mark.parametrize("name", list(_CHOICES))
def test_plan_choices_vs_fp64(name):
    """``config = 0`` and the same launch inside ``_C.co_scheduled()`` (bit 16 through ``_gemm_cfg``), each within the
    floor-free fp64 bound and of the un-sliced order's result; with the stage count forced (bits 1 / 2) the slice count
    stays and one and two LDS stages are bit-identical, sliced and un-sliced."""
    C = _C()
    P = _problem(name, **_CHOICES[name])
    epi = dict(bias=True, res="f32", relu=True) if P.geom is None else dict(bias=True, relu=True)
    y8, _ = P.run(8, **epi)
    scale8 = y8.abs().max().item()
    for co in (False, True):
        bit = CO if co else 0
        ns = P.slices(bit)
        y, yp = P.run(0, co=co, **epi)
        ratio = P.ratio(y, **epi)
        _note(2, name, bit, ns, ratio)
        assert ratio <= 1.0, (name, co, ratio)
        assert torch.equal(yp, C.split_pair(y))
        assert (y - y8).abs().max().item() <= 1e-5 * scale8
        assert P.slices(bit | 1) == ns and P.slices(bit | 2) == ns
        one, _ = P.run(1, co=co, **epi)
        two, _ = P.run(2, co=co, **epi)
        assert torch.equal(one, two), (name, co, "one stage != two stages")
        assert torch.equal(y, one) or torch.equal(y, two)
        if ns == 1:
            assert torch.equal(y, y8)
    one, _ = P.run(8 | 1, **epi)
    two, _ = P.run(8 | 2, **epi)
    assert torch.equal(one, two) and torch.equal(one, y8), (name, "un-sliced: one stage != two stages")
    if P.flip:  # the data gradient this shape stands for: gated, co-scheduled
        for co in (False, True):
            y, yp = P.run_gated(0, co=co)
            ratio = P.ratio(y, gated=True)
            _note(2, name + " gate", CO if co else 0, P.slices(CO if co else 0), ratio)
            assert ratio <= 1.0 and torch.equal(yp, C.split_pair(y))


def test_dual_rp_gated_one_and_two_stages_bit_identical():
    """The DUAL kernel (pair shortcut + gate, never sliced): one and two LDS stages give the same bits, and the fp64 value."""
    C = _C()
    P = _problem("plain-1100x512x2048", **_CHOICES["plain-1100x512x2048"])
    rp, xp = C.split_pair(P.res), C.split_pair(P.y)
    outs = [C.split_gemm_pair_rp_gated(P.ap, P.bp, rp, xp, out_f32=True, out_pair=True, config=cfg) for cfg in (0, 1, 2)]
    for (y, yp), cfg in zip(outs, (0, 1, 2)):
        ratio = P.ratio(y, res="pair", gated=True)
        _note(2, P.name + " rp_gated", cfg, 1, ratio)
        assert ratio <= 1.0 and torch.equal(yp, C.split_pair(y))
    assert torch.equal(outs[1][0], outs[2][0]) and torch.equal(outs[0][0], outs[1][0])


def test_identity_backward_co_scheduled_vs_fp64_autograd():
    """``_C.bottleneck_identity_backward`` on 2 maps of 50 x 84, 1024 -> 256 -> 1024, inside ``co_scheduled()`` (the frozen
    half of the student-teacher step): bit-equal to the separate launches, which pick up bit 16 the same way (two K slices
    on the 1x1 data gradient, four on the 3x3 one), and gx, dw1, dw2, dw3 against fp64 autograd of the same block.

    Bounds.  L2: |got - ref| <= TOL |ref| per gradient.  Elementwise, floor-free: every product is within TOL of its own
    sum |a||b| and every hand-over in pair layout rounds to 2^-17 <= TOL of the value, and magnitudes propagate through the
    chain as sums of absolute values, so with mag = the same backward chain run on absolute values (gates kept)
    dw3 (one product) is within 1 TOL mag, g2 within 2 (product + hand-over), dw2 within 3, g1 within 4, dw1 within 5, and gx
    (product + the pair output itself) within 6."""
    C = _C()
    r, h, w, cin, mid = 2, 50, 84, 1024, 256
    m = r * h * w
    g = torch.Generator(device="cuda").manual_seed(31)
    z = torch.randn(m, cin, device="cuda", generator=g)              # the pre-activation of the block below
    w1 = torch.randn(mid, cin, 1, 1, device="cuda", generator=g) / cin ** 0.5
    w2 = torch.randn(mid, mid, 3, 3, device="cuda", generator=g) / (9 * mid) ** 0.5
    w3 = torch.randn(cin, mid, 1, 1, device="cuda", generator=g) / mid ** 0.5
    ss = tuple(torch.rand(n, device="cuda", generator=g) + 0.5 for n in (mid, mid, cin))
    gout = torch.randn(m, cin, device="cuda", generator=g) * 1e-3

    def mat(wt, s):  # folded weight as the forward GEMM's [N, taps * C] tap-major matrix
        return (wt * s.view(-1, 1, 1, 1)).permute(0, 2, 3, 1).reshape(wt.shape[0], -1)

    zd = z.double().requires_grad_(True)
    wd = [t.double().requires_grad_(True) for t in (w1, w2, w3)]
    sd = [s.double() for s in ss]
    xd = zd.clamp(min=0)
    o1 = (xd @ mat(wd[0], sd[0]).t()).clamp(min=0)
    o2 = (_cols64(o1, (r, h, w)) @ mat(wd[1], sd[1]).t()).clamp(min=0)
    y3 = o2 @ mat(wd[2], sd[2]).t() + xd
    rgx, rdw1, rdw2, rdw3 = torch.autograd.grad((y3.clamp(min=0) * gout.double()).sum(), [zd] + wd)
    g3 = gout * (y3.detach() > 0)                                    # the gated gradient the block receives: exact in fp32
    x32, o1_32, o2_32 = xd.detach().float(), o1.detach().float(), o2.detach().float()

    with torch.no_grad():  # the chain on absolute values, gates kept
        a1, a2, a3 = (mat(t.detach(), s).abs() for t, s in zip(wd, sd))
        mg2 = (g3.abs().double() @ a3) * (o2 > 0)
        mdw3 = (g3.abs().double().t() @ o2) * sd[2].view(-1, 1)
        mdw2 = (mg2.t() @ _cols64(o1_32, (r, h, w))) * sd[1].view(-1, 1)
    with torch.enable_grad():
        probe = torch.zeros(m, mid, dtype=torch.float64, device="cuda", requires_grad=True)
        mg1 = torch.autograd.grad(_cols64(probe, (r, h, w)) @ a2.t(), probe, mg2)[0] * (o1.detach() > 0)
    with torch.no_grad():
        mdw1 = (mg1.t() @ xd) * sd[0].view(-1, 1)
        mgx = (mg1 @ a1 + g3.abs().double()) * (zd > 0)
        mdw2 = mdw2.view(mid, 9, mid).permute(0, 2, 1).reshape(mid, mid, 3, 3)

    g3p, xp, o1p, o2p = (C.split_pair(t) for t in (g3, x32, o1_32, o2_32))
    t1, t2, t3 = (C.weight_prep_pair(wt, sc, True)[1] for wt, sc in zip((w1, w2, w3), ss))
    with C.co_scheduled():
        assert C._gemm_cfg(0) == CO
        dw3 = C.split_gemm_pair_tn(g3p, o2p, None, scale=ss[2], weight_shape=tuple(w3.shape))
        _, g2p = C.split_gemm_pair_gated(g3p, t3, o2p)
        dw2 = C.split_gemm_pair_tn(g2p, o1p, (h, w, 3, 3), scale=ss[1], weight_shape=tuple(w2.shape))
        _, g1p = C.split_gemm_pair_gated(g2p, t2, o1p, conv=(h, w, 3, 3, True))
        dw1 = C.split_gemm_pair_tn(g1p, xp, None, scale=ss[0], weight_shape=tuple(w1.shape))
        _, gx = C.split_gemm_pair_rp_gated(g1p, t1, g3p, xp)
        for second in (torch.cuda.Stream(), None):
            got = C.bottleneck_identity_backward(g3p, xp, o1p, o2p, t1, t2, t3, ss, (h, w, 3, 3),
                                                 (w1.shape, w2.shape, w3.shape), second)
            torch.cuda.synchronize()
            assert torch.equal(got[0].view(torch.int16), gx.view(torch.int16))
            for a, b, name in zip(got[1:], (dw1, dw2, dw3), ("dw1", "dw2", "dw3")):
                assert a.shape == b.shape and torch.equal(a, b), (name, second is not None)
    ns = (slices(m, mid, cin, 0, 1, 1, 0, CO), slices(m, mid, mid, 0, 3, 3, w, CO), slices(m, cin, mid, 0, 1, 1, 0, CO))
    print(f"[2b] identity backward {r}x{h}x{w} {cin}->{mid}: co-scheduled slices of the data gradients (conv3, conv2, conv1) = {ns}")
    assert max(ns) > 1
    for name, a, ref, mag, depth in (("gx", _rec(got[0]), rgx, mgx, 6), ("dw1", got[1], rdw1.view_as(got[1]), mdw1.view_as(got[1]), 5),
                                     ("dw2", got[2], rdw2, mdw2, 3), ("dw3", got[3], rdw3.view_as(got[3]), mdw3.view_as(got[3]), 1)):
        err = (a.double() - ref).abs()
        ratio = (err / (depth * TOL * mag + 1e-30)).max().item()
        l2 = err.norm().item() / ref.norm().item()
        _WORST["2b"] = max(_WORST.get("2b", 0.0), ratio, l2 / TOL)
        print(f"[2b] {name}: config={CO:#x} slices={ns} err/bound={ratio:.2e} of {depth} x TOL x magnitude; relative L2 error {l2:.3e} "
              f"= {l2 / TOL:.3f} of TOL")
        assert ratio <= 1.0, (name, ratio)
        assert l2 <= TOL, (name, l2)


# ---------------------------------------------------------------------------------------------------------------------
# 3. the no-workspace fallback of the launcher
# ---------------------------------------------------------------------------------------------------------------------
def test_missing_or_short_workspace_falls_back_to_the_unsliced_grid():
    """``ovis_split_gemm_pair`` with a NULL workspace, or one a byte too small, for a plan that slices: OVIS_OK and the bits
    of ``config = 8`` (the launcher re-plans un-sliced); with the full workspace the sliced plan runs."""
    C = _C()
    m, k, n = 513, 2048, 2048
    P = _problem("plain-513x2048x2048", m=m, ch=k, n=n, seed=41)
    ns = P.slices(0)
    assert ns > 1
    need = 4 * m * n * ns
    want, want_p = P.run(8, bias=True, relu=True)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(ws_ptr, ws_bytes):
        c = torch.full((m, n), float("nan"), device="cuda")
        cp = torch.zeros(m, 2 * n, dtype=torch.bfloat16, device="cuda")
        rc = C._L.ovis_split_gemm_pair(P.ap.data_ptr(), 2 * P.ap.stride(0), 0, 0, P.bp.data_ptr(), 2 * P.bp.stride(0),
                                       c.data_ptr(), n, cp.data_ptr(), 4 * n, P.bias.data_ptr(), 0, 0, m, n, k, 0, 1, 1, 0, 0, 0,
                                       1, ws_ptr, ws_bytes, 0, C._stream())
        torch.cuda.synchronize()
        return rc, c, cp

    for label, ptr, nbytes in (("NULL workspace", 0, 0), ("NULL workspace, size given", 0, need), ("one byte short", ws.data_ptr(), need - 1)):
        rc, c, cp = call(ptr, nbytes)
        assert rc == OVIS_OK, label
        assert torch.equal(c, want) and torch.equal(cp, want_p), label
        print(f"[3] {P.name} {label}: config=0x0 slices={ns} planned, un-sliced run, bit-identical to config 8")
    rc, c, cp = call(ws.data_ptr(), need)
    sliced, sliced_p = P.run(0, bias=True, relu=True)
    assert rc == OVIS_OK and torch.equal(c, sliced) and torch.equal(cp, sliced_p)
    assert not torch.equal(sliced, want)   # (another summation order: the full workspace did select the sliced plan)
    ratio = P.ratio(c, bias=True, relu=True)
    _note(3, P.name + " full workspace", 0, ns, ratio)
    assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------------------------------
# 4. magnitude: power-of-two scaling is exact
# ---------------------------------------------------------------------------------------------------------------------
_SCALED = {
    # name: (problem arguments, config, sliced?)
    "plain-unsliced-1000x512x192": (dict(m=1000, ch=512, n=192, seed=51), 8, False),
    "plain-sliced-513x2048x256": (dict(m=513, ch=2048, n=256, seed=52), 0, True),
    "shifted-5x7x7x96-128": (dict(m=245, ch=96, n=128, seed=53, geom=(5, 7, 7)), 4 | 8, False),
    "shifted-sliced-flip-5x7x7x96-128": (dict(m=245, ch=96, n=128, seed=54, geom=(5, 7, 7), flip=True), 4, True),
    "halo-37x7x7x160-192": (dict(m=37 * 49, ch=160, n=192, seed=55, geom=(37, 7, 7)), 0, True),
    "narrow-300x256x64": (dict(m=300, ch=256, n=64, seed=56), 0, False),
}


@pytest.mark.parametrize("shift", [-20, 20])
@pytest.mark.parametrize("name", list(_SCALED))
def test_power_of_two_scaling_is_exact(name, shift):
    """The hi/lo split, the bf16 products and the fp32 accumulation commute with a scaling by 2^s while nothing leaves the
    normal range (unit-normal operands: the smallest surviving term is ~1e-27), so act(2^s A B^T + 2^s bias + 2^s residual)
    must be 2^s act(A B^T + bias + residual) BIT FOR BIT, in fp32 and in pair layout: no absolute epsilon, no flush, no
    lane that holds anything but products."""
    C = _C()
    args, cfg, sliced = _SCALED[name]
    P = _problem(name, **args)
    assert (P.slices(cfg) > 1) == sliced
    f = 2.0 ** shift
    conv = P.conv
    res = None if conv is not None else P.res

    def run(scale):
        return C.split_gemm_pair(C.split_pair(P.a * scale), P.bp, P.bias * scale, None if res is None else res * scale, True, True, True,
                                 conv=conv, config=cfg)

    y, yp = run(1.0)
    ys, ysp = run(f)
    assert y.abs().max().item() > 1.0 and torch.isfinite(ys).all()
    assert torch.equal(ys, y * f), name
    assert torch.equal(ysp, C.split_pair(ys)) and torch.equal(ysp, C.split_pair(y * f))
    # and on the B side
    yb, _ = C.split_gemm_pair(P.ap, C.split_pair(P.b * f), P.bias * f, None if res is None else res * f, True, True, False,
                              conv=conv, config=cfg)
    assert torch.equal(yb, ys)
    print(f"[4] {name} config={cfg:#x} slices={P.slices(cfg)} 2^{shift}: bit-identical (err/bound 0)")


@pytest.mark.parametrize("shift", [-20, 20])
@pytest.mark.parametrize("conv", [None, (7, 7, 3, 3)])
def test_power_of_two_scaling_is_exact_weight_gradient(conv, shift):
    """The same for the transpose-read weight gradient ``split_gemm_pair_tn`` (row slices + slab sum)."""
    C = _C()
    g = torch.Generator(device="cuda").manual_seed(57)
    m, n, ch = 49 * 37, 256, 128
    dy = torch.randn(m, n, device="cuda", generator=g)
    x = torch.randn(m, ch, device="cuda", generator=g)
    f = 2.0 ** shift
    dw = C.split_gemm_pair_tn(C.split_pair(dy), C.split_pair(x), conv)
    dws = C.split_gemm_pair_tn(C.split_pair(dy * f), C.split_pair(x), conv)
    dwx = C.split_gemm_pair_tn(C.split_pair(dy), C.split_pair(x * f), conv)
    assert dw.abs().max().item() > 1.0
    assert torch.equal(dws, dw * f) and torch.equal(dwx, dw * f)
    print(f"[4] tn {'plain' if conv is None else '3x3'} {m}x{n}x{ch} 2^{shift}: bit-identical (err/bound 0)")


@pytest.mark.parametrize("cfg", [0, 8, 5 << 8])
def test_zero_rows_give_exactly_the_epilogue_operands(cfg):
    """A third of A's rows and a third of B's rows exactly zero: those outputs are exactly act(bias + residual) -- sliced
    (the plan's choice, a forced ragged count) and un-sliced -- and everything stays within the floor-free bound, which is
    |bias| + |residual| alone there."""
    C = _C()
    P = _Problem("zero-rows-513x2048x256", m=513, ch=2048, n=256, seed=58)
    P.a[::3] = 0.0
    P.b[1::3] = 0.0
    P.ap, P.bp = C.split_pair(P.a), C.split_pair(P.b)
    ns = P.slices(cfg)
    assert (ns > 1) == (cfg != 8)
    for epi in (dict(bias=True, res="f32", relu=True), dict(bias=True, res="f32"), dict(res="pair"), dict()):
        y, yp = P.run(cfg, **epi)
        want = torch.zeros_like(y)
        if epi.get("bias"):
            want = want + P.bias
        if epi.get("res"):
            want = want + (P.res if epi["res"] == "f32" else _rec(C.split_pair(P.res)))
        if epi.get("relu"):
            want = want.clamp(min=0)
        assert torch.equal(y[::3], want[::3]) and torch.equal(y[:, 1::3], want[:, 1::3]), epi
        assert torch.equal(yp, C.split_pair(y))
        ratio = P.ratio(y, **epi)
        _note(4, f"{P.name} {_epi_name(epi)}", cfg, ns, ratio)
        assert ratio <= 1.0, epi


# ---------------------------------------------------------------------------------------------------------------------
# 5. row-strided operands
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [0, 8, 3 << 8])
def test_row_strided_operands_equal_contiguous_copies(cfg):
    """A as a 64-column-aligned column slice of a wider pair tensor, the fp32 residual as a row-strided view, the pair
    residual as a column slice of wider pair rows: bit-identical to contiguous copies, un-sliced and sliced (the finish
    kernel addresses the epilogue operands on its own)."""
    C = _C()
    g = torch.Generator(device="cuda").manual_seed(61)
    m, k, n = 333, 512, 192
    ns = slices(m, n, k, 0, 1, 1, 0, cfg)
    assert (ns > 1) == (cfg != 8)
    wide = C.split_pair(torch.randn(m, 64 + k + 32, device="cuda", generator=g))       # pair rows of 64 + k + 32 values
    a_view = wide[:, 2 * 64:2 * (64 + k)]                                             # values 64 .. 64 + k
    bp = C.split_pair(torch.randn(n, k, device="cuda", generator=g))
    bias = torch.randn(n, device="cuda", generator=g)
    big = torch.randn(m, n + 24, device="cuda", generator=g)
    r_view = big[:, 8:8 + n]
    rp_wide = C.split_pair(torch.randn(m, 32 + n + 64, device="cuda", generator=g))
    rp_view = rp_wide[:, 64:64 + 2 * n]
    assert not a_view.is_contiguous() and not r_view.is_contiguous() and not rp_view.is_contiguous()
    a_copy, r_copy, rp_copy = a_view.contiguous(), r_view.contiguous(), rp_view.contiguous()
    want, want_p = C.split_gemm_pair(a_copy, bp, bias, r_copy, True, True, True, config=cfg)
    got, got_p = C.split_gemm_pair(a_view, bp, bias, r_view, True, True, True, config=cfg)
    assert torch.equal(got, want) and torch.equal(got_p, want_p)
    want, want_p = C.split_gemm_pair(a_copy, bp, bias, None, True, True, True, config=cfg, residual_pair=rp_copy)
    got, got_p = C.split_gemm_pair(a_view, bp, bias, None, True, True, True, config=cfg, residual_pair=rp_view)
    assert torch.equal(got, want) and torch.equal(got_p, want_p)
    # the views were read where they lie: against fp64 of the sliced-out values
    ref = _rec(a_copy).double() @ _rec(bp).double().t() + bias.double() + _rec(rp_copy).double()
    bound = _rec(a_copy).abs().double() @ _rec(bp).abs().double().t() + bias.abs().double() + _rec(rp_copy).abs().double()
    ratio = ((got.double() - ref.clamp(min=0)).abs() / (TOL * bound + 1e-30)).max().item()
    _note(5, f"strided-{m}x{k}x{n}", cfg, ns, ratio)
    assert ratio <= 1.0
