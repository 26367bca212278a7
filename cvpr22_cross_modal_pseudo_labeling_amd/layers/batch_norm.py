"""``FrozenBatchNorm2d`` -- maskrcnn_benchmark/layers/batch_norm.py:6-31 (note: no epsilon).

Same four buffers (``weight, bias, running_mean, running_var``) so reference checkpoints load
unchanged.  ``fold()`` returns the per-channel (scale, shift) pair so a caller can fold the
affine into the preceding convolution at load time instead of running it as a separate
memory-bound pass."""
import torch
from torch import nn

from .derived import derived


class FrozenBatchNorm2d(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.register_buffer("weight", torch.ones(n))
        self.register_buffer("bias", torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))

    def sources(self):
        """The four buffers: the sources of ``fold()`` and of every value derived from it (layers/derived.py)."""
        return tuple(self._buffers.values())  # weight, bias, running_mean, running_var

    def fold(self):
        # computed once per state of the buffers: the SAME two tensors until then (``WeightPrepPlan.lookup`` compares by identity)
        return derived(self.sources(), "fold", self._fold)

    def _fold(self):
        scale = self.weight * self.running_var.rsqrt()
        return scale, self.bias - self.running_mean * scale

    def forward(self, x):
        scale, shift = self.fold()
        if x.dtype != scale.dtype:
            scale, shift = scale.to(x.dtype), shift.to(x.dtype)
        return x * scale.reshape(1, -1, 1, 1) + shift.reshape(1, -1, 1, 1)
