"""Autograd wrappers of the cross-modal head kernels (include/ovis_hip.h, csrc/gemm_f32.hip, csrc/losses.hip).

* ``linear_mfma`` / ``text_logits`` -- the two products of FastRCNNPredictor.forward
  (maskrcnn_benchmark/modeling/roi_heads/box_head/roi_box_predictors.py:66-71) on the fp32 matrix cores,
  forward and both backward products through the same strided GEMM kernel;
* ``weighted_cross_entropy`` -- box_head/loss.py:172-174, loss and d/dlogits in one pass;
* ``stochastic_mask_bce`` -- roi_mask_predictors.py:41-65 + mask_head/loss.py:139-142, loss and the
  gradients w.r.t. the mask logits and the predicted std-dev in one pass.
"""
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import _C
from .derived import derived


class _LinearMFMA(Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return _C.gemm_nt(x, weight, bias)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = _C.gemm_nt(dy, weight.t()) if ctx.needs_input_grad[0] else None          # [M,N] x [K,N]^T
        dw = _C.gemm_nt(dy.t(), x.t()) if ctx.needs_input_grad[1] else None          # [N,M] x [K,M]^T
        db = dy.sum(0) if (ctx.has_bias and ctx.needs_input_grad[2]) else None
        return dx, dw, db


def _pair_weight_padded(weight, n_pad, transposed=False):
    """[N, K] f32 -> pair layout [n_pad, 2K] (zero rows behind N), or of its transpose [K, 2 * n_pad] (the data-gradient
    operand); computed once for a tensor that does not require grad (the class / vocabulary matrices, frozen emb_pred)."""
    def build():
        import torch.nn.functional as F
        w = weight.detach()
        if transposed:
            w = w.t()
            if w.shape[1] != n_pad:
                w = F.pad(w, (0, n_pad - w.shape[1]))
        elif w.shape[0] != n_pad:
            w = F.pad(w, (0, 0, 0, n_pad - w.shape[0]))
        return _C.split_pair(w.contiguous())
    return derived((weight,), ("pair", n_pad, transposed), build)


class _LinearPair(Function):
    """y = x @ weight^T + bias on the pair-layout split GEMM (csrc/split_gemm.hip): the region x text products of the
    cross-modal head (roi_box_predictors.py:62-81) as fp32-accurate three-term bf16 hi/lo products on the bf16 matrix
    cores -- several times the rate of the fp32-input MFMA GEMM they replace, and deterministic (small-M problems are cut
    into K slices whose slabs one kernel reduces; no atomics).  N is padded to a multiple of 128 with zero rows."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        """Returns [M, N] -- a column slice (view) of the padded [M, n_pad] product when N is not a multiple of 128; a
        caller that can build its weight already padded (zero rows) avoids the pad launches."""
        import torch.nn.functional as F
        n = weight.shape[0]
        n_pad = -(-n // 128) * 128
        xp = _C.split_pair(x.detach())   # row-strided views (column slices of a padded product) are read in place
        wp = _pair_weight_padded(weight, n_pad)
        b = None
        if bias is not None:
            b = bias.detach() if n == n_pad else F.pad(bias.detach(), (0, n_pad - n))
        y, _ = _C.split_gemm_pair(xp, wp, b)
        ctx.save_for_backward(xp, weight)
        ctx.has_bias = bias is not None
        ctx.n_pad = n_pad
        return y if n == n_pad else y[:, :n]

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        import torch.nn.functional as F
        xp, weight = ctx.saved_tensors
        n, n_pad = weight.shape[0], ctx.n_pad
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dx = dw = db = None
        if need_x or need_w:
            g = dy if n == n_pad else F.pad(dy, (0, n_pad - n))
            gp = _C.split_pair(g.contiguous())                                  # [M, 2 n_pad]
            if need_x:
                dx, _ = _C.split_gemm_pair(gp, _pair_weight_padded(weight, n_pad, transposed=True))  # dY W
            if need_w:
                dw = _C.split_gemm_pair_tn(gp, xp)[:n]                          # dY^T X over the rows
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.sum(0)
        return dx, dw, db


def _pair_ok(x, weight):
    return (x.is_cuda and x.dim() == 2 and weight.dim() == 2 and x.dtype == torch.float32 and weight.shape[1] % 128 == 0
            and weight.shape[0] >= 32 and x.shape[0] > 0)


def linear_mfma(x, weight, bias=None):
    """y = x @ weight^T + bias with x [M,K], weight [N,K] (nn.Linear layout): split GEMM on the bf16 matrix cores when
    the shape allows (K % 128 == 0, N >= 32), else the exact-fp32 MFMA GEMM (``_C.gemm_nt``: the mask predictor's
    1- and 2-channel 1x1 heads)."""
    if _pair_ok(x, weight):
        return _LinearPair.apply(x, weight, bias)
    return _LinearMFMA.apply(x, weight, bias)


def text_logits(region_emb, class_emb):
    """einsum('pe,ce->pc'): region embeddings [P,E] against the class / vocabulary matrix [C,E]."""
    return linear_mfma(region_emb, class_emb, None)


class _WeightedCE(Function):
    @staticmethod
    def forward(ctx, logits, labels, bg_weight):
        loss, dlogits = _C.weighted_ce_fwd_bwd(logits, labels, bg_weight, need_grad=logits.requires_grad)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None, None


def weighted_cross_entropy(logits, labels, bg_weight):
    """sum_p w[label_p] * CE_p / P with w[0] = bg_weight, w[c>0] = 1 (scalar)."""
    return _WeightedCE.apply(logits, labels, bg_weight)


class _SmoothL1Picked(Function):
    @staticmethod
    def forward(ctx, box_regression, regression_targets, positives, labels, column0, beta, denominator):
        loss, grad = _C.smooth_l1_picked_fwd_bwd(box_regression, regression_targets, positives, labels, column0, beta,
                                                 denominator, need_grad=box_regression.requires_grad)
        ctx.save_for_backward(grad)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return grad * g, None, None, None, None, None, None


def smooth_l1_picked(box_regression, regression_targets, positives, labels, column0, beta, denominator):
    """sum over the rows ``positives`` of smooth_l1(box_regression[p, col0:col0 + 4] - regression_targets[p]; beta) /
    denominator, col0 = 4 * labels[p] or ``column0`` (labels None) -- box_head/loss.py:147-170 as one fused op."""
    return _SmoothL1Picked.apply(box_regression, regression_targets, positives, labels, column0, beta, denominator)


class _StochasticMaskBCE(Function):
    @staticmethod
    def forward(ctx, mu, sigma, eps, pos_index, targets, channel):
        need = mu.requires_grad or (sigma is not None and sigma.requires_grad)
        loss, dmu, dsigma = _C.mask_bce_stochastic_fwd_bwd(mu, sigma, eps, pos_index, targets, channel, need_grad=need)
        ctx.has_sigma = sigma is not None
        ctx.save_for_backward(dmu, dsigma)
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        dmu, dsigma = ctx.saved_tensors
        return (dmu * g if dmu is not None else None, dsigma * g if (ctx.has_sigma and dsigma is not None) else None,
                None, None, None, None)


def stochastic_mask_bce(mu, sigma, eps, pos_index, targets, channel=1):
    """mean BCEWithLogits(mu[pos, channel] + eps[pos, channel] * sigma[pos], targets); sigma / eps may be None."""
    return _StochasticMaskBCE.apply(mu, sigma, eps, pos_index, targets, channel)
