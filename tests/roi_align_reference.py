"""An independent fp64 reference of the RoIAlign backward and forward, with elementwise error budgets (host only, NumPy).

The operation (the formulas ``csrc/roi_geom.h`` cites: ROIAlign_cuda.cu:16-62 the bilinear set-up, :86-113 the RoI
geometry, :178-254 the backward): bin (i, j) of RoI r averages ``gh x gw`` bilinear samples at

    y = start_h + i * bin_h + (iy + .5) * bin_h / gh,        x likewise,

a sample outside [-1, size] is dropped, one inside is clamped to [0, size - 1] and splits between the two cells around
it with weights (1 - l, l).  The backward sends ``grad[r, c, i, j] / (gh * gw)`` back along every weight.  The weight of a
sample is a product of a row part and a column part, so the gradient of a RoI is ``Ay^T . G_c . Ax / count`` with
``Ay[i, y]`` the summed row weights of bin-row i's samples -- a property of the operation, used here only to keep the
reference fast (two fp64 matrix products per RoI).  ``Ay`` / ``Ax`` are filled by scalar loops over (RoI, bin, sample) on
the WHOLE map axis: no windows, blocks, tables, origins or k-groups.

Geometry.  ``start``, ``roi_w``, ``roi_h``, ``bin`` and the adaptive grid ``ceil(roi / P)`` are evaluated in float32, operation
by operation as ``make_geom`` does (plain IEEE operations, the library is built with ``-ffp-contract=off``, the reference
op does the same): they decide discrete things (the grid) that both sides must agree on.  From the sample coordinate on
everything is fp64.  RoIs whose image id ``(int)roi[0]`` lies outside [0, n) contribute nothing.  ``bin_stride = s > 1``:
``grad`` is [R, C, ceil(PH / s), ceil(PW / s)] and holds bins (s * i, s * j); every other bin's gradient is zero.

What comes back, each [n, c, h, w] float64 (``terms`` int64) plus a scalar:

``ref``     the gradient.
``mag``     sum of weight * |grad| over the same terms.  All weights are >= 0, so a backward-stable kernel errs by a
            multiple of ``mag`` per cell -- the multiple is the kernel's own (``TOL_MFMA``, ``f32_bound`` below).
``slack``   what the kernels' float32 sample coordinates may move.  A coordinate off by d moves the weights of its two
            cells by at most d each, and when it crosses an integer it moves at most d onto the next cell.  So with
            ``Dy[i, y]`` = the sum of d over bin-row i's samples whose cells lo - 1 .. hi + 1 include y (and Dx likewise)
                slack = sum |g| / count * ((Ay + Dy) (x) (Ax + Dx) - Ay (x) Ax)
            = sum (|g| / count) (dx * wy + dy * wx) + the second-order term.  It scales with |g|: it is no floor.
``terms``   per cell, the number of (RoI, bin, sample pair, corner) contributions with a non-zero weight and a non-zero
            gradient: the length of the fp32 sum the reference's atomic formulation (and the atomic kernels) build.
``clearance`` the smallest distance of any sample coordinate (RoIs of images in [0, n)) from the validity boundaries -1
            and ``size``, in units of that sample's d.  The operation is discontinuous there (a sample is kept with
            weight 1 on the border cell or dropped), no bound covers a flip, so the GPU tests require >= 4.

The coordinate error d = ``K_ULPS`` float32 ulps of the largest intermediate M of that coordinate
(M = max |start|, |p * bin|, |start + p * bin|, |(i + .5) * bin|, |v|), counted in roundings of half an ulp(M) each:

  ``sample_coord`` (roi_geom.h, the atomic kernels and the window):  v = (start + p * bin) + ((i + .5) * bin) / g
      p * bin, the first sum, (i + .5) * bin, the quotient, the last sum: 5 roundings (i + .5 and the conversions are exact).
  ``axis_weight`` (roi_mfma.h, the matrix-core tables):  v = (start + p * bin) + (i + .5) * step, step = fl(bin / g)
      p * bin, the sum, the product, the last sum: 4 roundings; the rounding of ``step`` itself is half an ulp(step),
      multiplied by i + .5 -- at most one ulp of the product (ulps double at a power of two), counted as 2.  6 roundings.

6 half-ulps = ``K_ULPS = 3``.  Past the coordinate a kernel's weight arithmetic is exact or relative: l = v - lo is exact
(Sterbenz), 1 - l and the sums over a bin's samples carry relative roundings of 2^-24 that the kernels' ``mag`` multiples
absorb.

The forward (``roi_align_forward_ref``) is the same operation read the other way: with the same float32 geometry and the
same fp64 ``Ay`` / ``Ax``,  out[r, c, i, j] = Ay[i, :] . x[b, c] . Ax[j, :]^T / count.  Its ``Result`` fields are
[R, C, th, tw]: ``mag`` the same sum with |x|, ``slack`` as above with |x| in place of |g|, ``terms`` the number of
(sample pair, corner) taps of the bin whose weight is non-zero (the same for every channel).  A RoI with a foreign image
id gives exact zeros with no bound, and so does a RoI with a non-finite coordinate: the project's rule (``make_geom``'s
``empty``: a non-finite sample coordinate pools nothing).  ``make_geom`` reaches that verdict for a NaN or an infinity in
x1 / y1 and for +Inf in x2 / y2; a NaN or -Inf in x2 / y2 alone is, in the kernels as in the reference operation, a RoI of
size 1 (``fmaxf(NaN, 1) = 1``) -- the GPU case tables use only the former kind and check that on the host (``geom32``).
"""
import collections

import numpy as np

K_ULPS = 3.0
# Matrix-core forms (roi_mfma.h).  ``split_bf16`` keeps v as bf16 hi + bf16 lo of the exact remainder; bf16 has 8 significand
# bits, unit roundoff u = 2^-8, so |v - hi - lo| <= u^2 |v| = 2^-16 |v| in the worst case.
# ``mfma3`` adds hi.hi + hi.lo + lo.hi in fp32 and drops lo.lo <= u^2 |a||b|.  One product therefore has three error sources
# of at most 2^-16 = 1.5e-5 of sum |a||b| each (two operand representations, the dropped term) plus the fp32 accumulation
# of at most 16 terms (1e-6).  The project's single-product constant is 2e-5 (tests/test_split_gemm_pair.py): more than any
# one source, less than the three at their worst together (4.6e-5), which independent roundings do not reach.  The backward
# chains two such products, T = G . Ax and dW = Ay^T . T, with T re-split in between (the second product's operand
# representation): twice the constant, against a worst case of 6 * 2^-16 = 9.2e-5.  All weights are >= 0, so sum |a||b|
# through both stages is ``mag``.  The pre-split small-tile form issues all four hi/lo terms (four sources instead of six).
# Cells that few terms reach (a clamped border cell of one RoI, 4 x 4 tiles) have nothing to average over and come
# closest: ``split_form_emulation`` below restates the algorithm on this module's fp64 weights so that the share of the
# bound the ALGORITHM uses can be told from a kernel's mistake (tests/test_roi_align_reference.py prints it per case).
TOL_MFMA = 4e-5
# Atomic kernels (roi_align.hip).  Scatter form, per contribution top * (hy * hx) / count: 1 - l, the product, the
# multiplication by top, the division = 4 relative roundings of 2^-24, and a sum of ``terms`` contributions adds
# terms - 1: (terms + 3) * 2^-24.  LDS form, per RoI and cell sum_bins (Ay[i] * Ax[j]) * g / count: Ay[i] is a sum of Ny
# weights (Ny roundings with the 1 - l), Ax[j] of Nx, the product, the multiplication, the division, nb - 1 additions over
# the bins, one atomic per RoI: max(Ny + Nx) + nb + 2 + RoIs <= terms + 4 because sum Ny * Nx >= max(Ny + Nx) - 1 + nb - 1.
ATOMIC_C = 4
# Exact forward forms (``fwd_pool`` and its LDS / table / strided variants, roi_align.hip; the reference CPU kernel has the same
# sequence).  Per tap w * v with w = hy * hx: l = v - lo is exact, 1 - ly and 1 - lx are one rounding each, their product
# one (the worst of the four corner weights: 3), w * v one: 4 per tap.  The taps of a sample are added left to right and the
# sample to the accumulator; a tap whose weight is zero contributes an exact zero whose addition is exact, so a bin of
# ``terms`` non-zero taps sees at most terms - 1 rounded additions on any one path.  The division by ``count`` (or the exact
# multiplication by 1 / count on power-of-two grids) is one more: 4 + (terms - 1) + 1 = terms + 4 relative roundings of
# 2^-24 of the tap's |w v|, i.e. of ``mag``.  That is the first-order count k * u; the exact factor (1 + u)^k - 1 <=
# k u / (1 - k u) exceeds it by about (k u)^2, less than one u while k^2 u <= 1 (k <= 4096; 16 x 16 samples of four taps and
# the four above are 1028), which one further unit covers: terms + 5.
FWD_C = 5
U32 = 2.0 ** -24

Result = collections.namedtuple("Result", "ref mag slack terms clearance")
_f = np.float32


def _geometry(roi, scale, ph, pw, sampling_ratio):
    """float32, operation by operation as ``make_geom``: image id, (start, bin, grid) per axis (y first)."""
    roi = np.asarray(roi, dtype=_f)
    sc = _f(scale)
    axes = []
    for lo, hi, p in ((roi[2], roi[4], ph), (roi[1], roi[3], pw)):
        start = _f(lo * sc)
        end = _f(hi * sc)
        size = max(_f(end - start), _f(1.0))
        bin_ = _f(size / _f(p))
        grid = sampling_ratio if sampling_ratio > 0 else int(np.ceil(bin_))
        axes.append((float(start), float(bin_), grid))
    return int(roi[0]), axes


def _axis(start, bin_, grid, bins, size):
    """fp64 weights A[t, cell] of the bins ``bins`` along one axis, their coordinate slack D, the count of non-zero
    weights N, and the clearance of the samples."""
    A = np.zeros((len(bins), size))
    D = np.zeros((len(bins), size))
    N = np.zeros((len(bins), size))
    clear = np.inf
    for t, p in enumerate(bins):
        for i in range(grid):
            off, part = p * bin_, (i + .5) * bin_
            v = start + off + part / grid
            big = max(abs(start), abs(off), abs(start + off), abs(part), abs(v))
            d = K_ULPS * float(np.spacing(_f(big)))
            clear = min(clear, abs(v + 1.0) / d, abs(v - size) / d)
            if v < -1.0 or v > size:
                continue
            v = max(v, 0.0)
            lo = int(v)
            if lo >= size - 1:
                lo = hi = size - 1
                v = float(lo)
            else:
                hi = lo + 1
            l = v - lo
            h = 1.0 - l
            A[t, lo] += h
            A[t, hi] += l
            N[t, lo] += h != 0.0
            N[t, hi] += l != 0.0
            D[t, max(lo - 1, 0):min(hi + 1, size - 1) + 1] += d
    return A, D, N, clear


def _rows(T, Ly):
    """sum_i T[c, i, x] Ly[i, y]"""
    return np.einsum("iy,cix->cyx", Ly, T)


def _fold(G, Ly, Lx):
    """sum_ij G[c, i, j] Ly[i, y] Lx[j, x]"""
    return _rows(G @ Lx, Ly)


def roi_align_backward_ref(grad, rois, scale, ph, pw, n, c, h, w, sampling_ratio, bin_stride=1):
    grad = np.asarray(grad, dtype=np.float64)
    rois = np.asarray(rois, dtype=_f).reshape(-1, 5)
    th, tw = -(-ph // bin_stride), -(-pw // bin_stride)
    assert grad.shape == (rois.shape[0], c, th, tw), (grad.shape, (rois.shape[0], c, th, tw))
    ref, mag, slack = (np.zeros((n, c, h, w)) for _ in range(3))
    terms = np.zeros((n, c, h, w))
    clearance = np.inf
    for r in range(rois.shape[0]):
        b, ((sy, by, gy), (sx, bx, gx)) = _geometry(rois[r], scale, ph, pw, sampling_ratio)
        if b < 0 or b >= n:
            continue
        Ay, Dy, Ny, cy = _axis(sy, by, gy, [bin_stride * i for i in range(th)], h)
        Ax, Dx, Nx, cx = _axis(sx, bx, gx, [bin_stride * j for j in range(tw)], w)
        clearance = min(clearance, cy, cx)
        count = float(gy * gx)
        G = grad[r]
        ref[b] += _fold(G, Ay, Ax) / count
        m = _fold(np.abs(G), Ay, Ax) / count
        mag[b] += m
        slack[b] += _fold(np.abs(G), Ay + Dy, Ax + Dx) / count - m
        terms[b] += _fold((G != 0.0).astype(np.float64), Ny, Nx)
    return Result(ref, mag, np.maximum(slack, 0.0), np.rint(terms).astype(np.int64), clearance)


def clearance_of(rois, scale, ph, pw, n, h, w, sampling_ratio):
    """``clearance`` alone (every bin, so it covers any ``bin_stride``)."""
    clear = np.inf
    for roi in np.asarray(rois, dtype=_f).reshape(-1, 5):
        if not np.all(np.isfinite(roi)):
            continue
        b, ((sy, by, gy), (sx, bx, gx)) = _geometry(roi, scale, ph, pw, sampling_ratio)
        if 0 <= b < n:
            clear = min(clear, _axis(sy, by, gy, range(ph), h)[3], _axis(sx, bx, gx, range(pw), w)[3])
    return clear


def _pool(X, Ly, Lx):
    """sum_yx Ly[i, y] X[c, y, x] Lx[j, x]"""
    return (Ly @ X) @ Lx.T


def roi_align_forward_ref(x, rois, scale, ph, pw, sampling_ratio, bin_stride=1):
    x = np.asarray(x, dtype=np.float64)
    rois = np.asarray(rois, dtype=_f).reshape(-1, 5)
    n, c, h, w = x.shape
    th, tw = -(-ph // bin_stride), -(-pw // bin_stride)
    ref, mag, slack, terms = (np.zeros((rois.shape[0], c, th, tw)) for _ in range(4))
    clearance = np.inf
    for r in range(rois.shape[0]):
        if not np.all(np.isfinite(rois[r])):
            continue
        b, ((sy, by, gy), (sx, bx, gx)) = _geometry(rois[r], scale, ph, pw, sampling_ratio)
        if b < 0 or b >= n:
            continue
        Ay, Dy, Ny, cy = _axis(sy, by, gy, [bin_stride * i for i in range(th)], h)
        Ax, Dx, Nx, cx = _axis(sx, bx, gx, [bin_stride * j for j in range(tw)], w)
        clearance = min(clearance, cy, cx)
        count = float(gy * gx)
        X = np.abs(x[b])
        ref[r] = _pool(x[b], Ay, Ax) / count
        mag[r] = _pool(X, Ay, Ax) / count
        slack[r] = _pool(X, Ay + Dy, Ax + Dx) / count - mag[r]
        terms[r] = np.outer(Ny.sum(1), Nx.sum(1))[None]
    return Result(ref, mag, np.maximum(slack, 0.0), np.rint(terms).astype(np.int64), clearance)


def _bf16(v):
    """float32 -> bf16 (round to nearest even), as float32"""
    u = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) & 0xffff0000).astype(np.uint32).view(np.float32)


def _split(v):
    v = np.asarray(v, dtype=np.float32)
    hi = _bf16(v)
    return hi.astype(np.float64), _bf16(v - hi).astype(np.float64)


def split_form_emulation(grad, rois, scale, ph, pw, n, c, h, w, sampling_ratio, bin_stride=1, four_terms=False):
    """What the matrix-core algorithm itself computes -- both operands of both products as bf16 hi + lo, three (or four)
    of the hi/lo terms, T rounded to float32 and re-split -- on this module's weights rounded to float32, sums in fp64."""
    grad = np.asarray(grad, dtype=_f)
    rois = np.asarray(rois, dtype=_f).reshape(-1, 5)
    th, tw = -(-ph // bin_stride), -(-pw // bin_stride)
    out = np.zeros((n, c, h, w))
    for r in range(rois.shape[0]):
        b, ((sy, by, gy), (sx, bx, gx)) = _geometry(rois[r], scale, ph, pw, sampling_ratio)
        if b < 0 or b >= n:
            continue
        Ay = _axis(sy, by, gy, [bin_stride * i for i in range(th)], h)[0].astype(_f) / _f(gy * gx)
        Ax = _axis(sx, bx, gx, [bin_stride * j for j in range(tw)], w)[0].astype(_f)
        (g_hi, g_lo), (x_hi, x_lo), (y_hi, y_lo) = _split(grad[r]), _split(Ax), _split(Ay)
        T = g_hi @ x_hi + g_hi @ x_lo + g_lo @ x_hi + (g_lo @ x_lo if four_terms else 0.0)
        t_hi, t_lo = _split(T.astype(_f))
        out[b] += _rows(t_hi, y_hi) + _rows(t_lo, y_hi) + _rows(t_hi, y_lo) + (_rows(t_lo, y_lo) if four_terms else 0.0)
    return out


def split_form_emulation_forward(x, rois, scale, ph, pw, sampling_ratio, bin_stride=1):
    """The forward's matrix-core algorithm (roi_align_fwd_mfma.hip): V = (Ay / count) . x[b, c] with both operands as bf16
    hi + lo and three of the hi/lo terms, V rounded to float32 and re-split, out = V . Ax^T the same way -- on this module's
    weights rounded to float32, sums in fp64."""
    x = np.asarray(x, dtype=_f)
    rois = np.asarray(rois, dtype=_f).reshape(-1, 5)
    n, c, h, w = x.shape
    th, tw = -(-ph // bin_stride), -(-pw // bin_stride)
    out = np.zeros((rois.shape[0], c, th, tw))
    for r in range(rois.shape[0]):
        if not np.all(np.isfinite(rois[r])):
            continue
        b, ((sy, by, gy), (sx, bx, gx)) = _geometry(rois[r], scale, ph, pw, sampling_ratio)
        if b < 0 or b >= n:
            continue
        Ay = _axis(sy, by, gy, [bin_stride * i for i in range(th)], h)[0].astype(_f) / _f(gy * gx)
        Ax = _axis(sx, bx, gx, [bin_stride * j for j in range(tw)], w)[0].astype(_f)
        (f_hi, f_lo), (x_hi, x_lo), (y_hi, y_lo) = _split(x[b]), _split(Ax), _split(Ay)
        V = y_hi @ f_hi + y_hi @ f_lo + y_lo @ f_hi
        v_hi, v_lo = _split(V.astype(_f))
        out[r] = v_hi @ x_hi.T + v_hi @ x_lo.T + v_lo @ x_hi.T
    return out


def mfma_bound(res):
    return TOL_MFMA * res.mag + res.slack


def mfma_forward_bound(res):
    """The forward chains two split products with a re-split in between, as the backward does: the same constant."""
    return TOL_MFMA * res.mag + res.slack


def f32_bound(res):
    return (res.terms + ATOMIC_C) * U32 * res.mag + res.slack


def f32_forward_bound(res):
    return (res.terms + FWD_C) * U32 * res.mag + res.slack


def worst_ratio(got, res, bound):
    """max |got - ref| / bound over the cells with a bound; a cell without one (mag == 0 and slack == 0: outside every
    window, other channels, images without RoIs) must be exactly zero and counts as inf otherwise."""
    err = np.abs(np.asarray(got, dtype=np.float64) - res.ref)
    free = bound == 0.0
    if np.any(err[free] != 0.0):
        return np.inf
    return float((err[~free] / bound[~free]).max()) if np.any(~free) else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# The float32 twin of ``make_geom`` (csrc/roi_geom.h) and of the forward kernels' dispatch decisions: which form a RoI
# reaches is computed on the host, so that a case table can be held to what it claims to cover without a GPU.
# ---------------------------------------------------------------------------------------------------------------------
Geom32 = collections.namedtuple("Geom32", "b gh gw pow2 window start bin")


def _coord32(start, p, bin_, i, g):
    """``sample_coord``: start + p * bin + (i + .5) * bin / g, every operation in float32"""
    return _f(_f(start + _f(_f(p) * bin_)) + _f(_f(_f(i) + _f(0.5)) * bin_) / _f(g))


def _low32(v, size):
    return 0 if v <= 0 else min(int(v), size - 1)


def geom32(roi, scale, n_img, h, w, ph, pw, sampling_ratio):
    """``make_geom`` in float32: grids, the power-of-two flag, (start, bin) per axis (y first) and the inclusive window
    (wy0, wy1, wx0, wx1) -- None when the RoI is ``empty`` (foreign image id, non-finite sample coordinates, every sample
    outside the map)."""
    roi = np.asarray(roi, dtype=_f)
    sc = _f(scale)
    grids, spans, starts, bins = [], [], [], []
    with np.errstate(all="ignore"):
        for lo, hi, p, size in ((roi[2], roi[4], ph, h), (roi[1], roi[3], pw, w)):
            start = _f(lo * sc)
            side = _f(_f(hi * sc) - start)
            side = side if side > 1 else _f(1)      # fmaxf: a NaN gives 1
            bin_ = _f(side / _f(p))
            starts.append(start)
            bins.append(bin_)
            if sampling_ratio <= 0 and not np.isfinite(bin_):
                grids.append(0)                      # (int)ceilf of a non-finite value: the coordinates below are not finite either
                spans.append(None)
                continue
            grid = sampling_ratio if sampling_ratio > 0 else int(np.ceil(bin_))
            grids.append(grid)
            first, last = _coord32(start, 0, bin_, 0, grid), _coord32(start, p - 1, bin_, grid - 1, grid)
            if not (np.isfinite(first) and np.isfinite(last)) or last < -1 or first > size:
                spans.append(None)
            else:
                spans.append((_low32(max(first, _f(-1)), size), min(_low32(min(last, _f(size)), size) + 1, size - 1)))
    gh, gw = grids
    pow2 = gh > 0 and gw > 0 and gh & (gh - 1) == 0 and gw & (gw - 1) == 0 and gh <= 1024 and gw <= 1024
    b = int(roi[0]) if np.isfinite(roi[0]) else -1
    ok = 0 <= b < n_img and spans[0] is not None and spans[1] is not None
    return Geom32(b, gh, gw, pow2, spans[0] + spans[1] if ok else None, tuple(starts), tuple(bins))


def roi_window(roi, scale, n_img, h, w, ph, pw, sampling_ratio):
    """(wy0, wy1, wx0, wx1) of a RoI's feature-map window, or None for an empty RoI"""
    return geom32(roi, scale, n_img, h, w, ph, pw, sampling_ratio).window


def _window_cells(rois, scale, n_img, h, w, p, sampling_ratio):
    """Cells of each RoI's feature-map window (0: no sample inside the map) -- the host twin of ``make_geom`` in
    csrc/roi_geom.h, in float32 like the kernel.  ``p``: the pooler, one number or (ph, pw)."""
    ph, pw = (p, p) if np.isscalar(p) else p
    cells = []
    for roi in np.asarray(rois, dtype=_f).reshape(-1, 5):
        win = roi_window(roi, scale, n_img, h, w, ph, pw, sampling_ratio)
        cells.append(0 if win is None else (win[1] - win[0] + 1) * (win[3] - win[2] + 1))
    return np.array(cells)


def block_shape(window):
    """(nyb, nxb): the 16-cell blocks the matrix-core forward cuts a window into"""
    wy0, wy1, wx0, wx1 = window
    return (wy1 - wy0 + 16) // 16, (wx1 - wx0 + 16) // 16


def max_grid(rois, scale, ph, pw, sampling_ratio):
    """The largest sampling grid per axis over the RoIs with finite coordinates (the kernels loop over it)."""
    worst = 0
    for roi in np.asarray(rois, dtype=_f).reshape(-1, 5):
        if np.all(np.isfinite(roi)):
            _, ((_, _, gy), (_, _, gx)) = _geometry(roi, scale, ph, pw, sampling_ratio)
            worst = max(worst, gy, gx)
    return worst


def exact_forms(rois, scale, n_img, c, h, w, ph, pw, sampling_ratio):
    """The forms of ``roi_align_fwd_kernel`` (csrc/roi_align.hip) a RoI list reaches with ``c`` channels, as a set of
    names: 'empty'; 'tab<16|8|4>' (table-driven batches), 'lane<16|8|4>' (``fwd_batch_lds4``), 'tail<2|1>'
    (``fwd_batch_lds``), 'global'; 'pow2' / 'div' (the FAST flag of the RoIs that run a 4-channel form); 'budget<16|8|4|2|1|0>'
    (the channels per batch the window leaves room for: 4352 // cells, capped at 16 and rounded down to a batch size; 0 =
    the global path); 'grid<g>' per axis grid."""
    forms = set()
    for roi in np.asarray(rois, dtype=_f).reshape(-1, 5):
        g = geom32(roi, scale, n_img, h, w, ph, pw, sampling_ratio)
        if g.window is None:
            forms.add("empty")
            continue
        cells = (g.window[1] - g.window[0] + 1) * (g.window[3] - g.window[2] + 1)
        cs_max = min(16, 4352 // cells)
        forms.add("budget%d" % max([k for k in (16, 8, 4, 2, 1, 0) if k <= cs_max]))
        forms.update(("grid%d" % g.gh, "grid%d" % g.gw))
        tables = ph * g.gh <= 64 and pw * g.gw <= 64 and ph * pw <= 256 and cells <= 4352
        for c0 in range(0, c, 32):
            left = min(c, c0 + 32) - c0
            while left > 0:
                k = min(left, cs_max)
                if k >= 4:
                    k = 16 if k >= 16 else 8 if k >= 8 else 4
                    forms.update((("tab%d" if tables else "lane%d") % k, "pow2" if g.pow2 else "div"))
                elif k >= 1:
                    k = 2 if k >= 2 else 1
                    forms.add("tail%d" % k)
                else:
                    k = 1
                    forms.add("global")
                left -= k
    return forms


def _axis_state32(start, bin_, p, size):
    """The shared-tap path's view of one axis of a bin at a 2-sample grid: 'none' (both samples invalid), 'first' / 'last'
    (only that sample valid), 'same' (both in one cell pair), 'diff'."""
    taps = []
    for i in range(2):
        v = _coord32(start, p, bin_, i, 2)
        if v < -1 or v > size:
            taps.append(None)
            continue
        lo = _low32(v, size)
        taps.append((lo, min(lo + 1, size - 1)))
    if taps[0] is None or taps[1] is None:
        return "none" if taps[0] is None and taps[1] is None else "first" if taps[1] is None else "last"
    return "same" if taps[0] == taps[1] else "diff"


def shared_tap_states(rois, scale, n_img, h, w, ph, pw, bin_stride):
    """The (row state, column state) pairs that the bins (s i, s j) of the RoIs take in the ``gh == gw == 2`` path of
    ``pool_nhwc_strided`` at sampling ratio 2 (``same_rows`` / ``same_cols`` / ``oky`` / ``okx`` per bin)."""
    states = set()
    for roi in np.asarray(rois, dtype=_f).reshape(-1, 5):
        g = geom32(roi, scale, n_img, h, w, ph, pw, 2)
        if g.window is None:
            continue
        rows = {_axis_state32(g.start[0], g.bin[0], p, h) for p in range(0, ph, bin_stride)}
        cols = {_axis_state32(g.start[1], g.bin[1], p, w) for p in range(0, pw, bin_stride)}
        states.update((a, b) for a in rows for b in cols)
    return states


# ---------------------------------------------------------------------------------------------------------------------
# RoI recipes shared by the CPU and the GPU tests (image pixels; the maps are ``scale`` = 1/16 of the image)
# ---------------------------------------------------------------------------------------------------------------------
SCALE = 1.0 / 16


def random_rois(seed, r, n, h, w, smin=4.0, smax=None):
    """r RoIs with corners anywhere in the 16h x 16w image, sides smin .. smax pixels, clamped to the image."""
    g = np.random.default_rng(seed)
    iw, ih = 16.0 * w, 16.0 * h
    smax = 16.0 * min(h, w) if smax is None else smax
    b = g.integers(0, n, r)
    x1, y1 = g.random(r) * iw * 0.8, g.random(r) * ih * 0.8
    sw, sh = g.random(r) * (smax - smin) + smin, g.random(r) * (smax - smin) + smin
    return np.stack([b, x1, y1, np.minimum(x1 + sw, iw - 1), np.minimum(y1 + sh, ih - 1)], 1).astype(_f)


def edge_rois(h, w):
    """The RoIs of tests/test_ops_gpu.py::test_roi_align_backward_edge_rois, placed relative to an h x w map."""
    iw, ih = 16.0 * w, 16.0 * h
    return np.array([[0, -50.0, -40.0, 30.0, 20.0],                                # hangs over the top-left corner
                     [1, 0.6 * iw + 0.3, 0.5 * ih + 0.7, 0.6 * iw + 0.3, 0.5 * ih + 0.7],  # zero size -> one cell
                     [0, 0.8 * iw + 3.3, 0.8 * ih + 5.1, 3.0 * iw, 2.2 * ih],       # runs past the bottom-right corner
                     [1, iw + 5000.0, ih + 5000.0, iw + 5100.0, ih + 5100.0],       # entirely outside
                     [0, 0.0, 0.0, iw - 1.0, ih - 1.0],                             # the whole map
                     [1, 0.4 * iw + 0.3, 0.3 * ih + 0.7, 0.4 * iw + 1.9, 0.3 * ih + 2.2],  # sub-cell
                     [0, 0.5 * iw, 0.5 * ih, 0.5 * iw - 40.0, 0.5 * ih + 33.0]], dtype=_f)  # malformed: x2 < x1


def cleared(rois, ph, pw, n, h, w, sampling_ratios=(0,), scale=SCALE):
    """The same RoIs, any whose samples sit within 4 d of a validity boundary shifted by 0.37 px steps (at the scale 1/16;
    the same fraction of a cell at another) until none does."""
    rois = np.array(rois, dtype=_f)
    for r in range(rois.shape[0]):
        for _ in range(8):
            if all(clearance_of(rois[r], scale, ph, pw, n, h, w, sr) >= 4.0 for sr in sampling_ratios):
                break
            rois[r, 1:] += _f(0.37 * SCALE / scale)
        else:
            raise AssertionError(("no clear placement", r, rois[r]))
    return rois


def recipe(seed, n, h, w, ph, pw, r_random=24, sampling_ratios=(0,), extra=()):
    """Random RoIs + the edge RoIs (+ ``extra``), cleared for every sampling ratio it will be run with."""
    rois = np.concatenate([random_rois(seed, r_random, n, h, w), edge_rois(h, w)] +
                          [np.asarray(e, dtype=_f).reshape(-1, 5) for e in extra])
    rois[:, 0] = np.minimum(rois[:, 0], n - 1)
    return cleared(rois, ph, pw, n, h, w, sampling_ratios)


def dense_grad(seed, r, c, th, tw):
    return np.random.default_rng(seed).standard_normal((r, c, th, tw)).astype(_f)
