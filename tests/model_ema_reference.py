"""NumPy fp32 restatement of SGD with momentum + the weight EMA + its decay schedule (include/ovis_hip.h states the rule).
It shares only the formulas with the product code: every line below is one fp32 operation with one rounding (NumPy does not
contract a multiply and an add), on arrays the caller owns."""
import numpy as np

F = np.float32


def decay_at(decay, t):
    """d_t = min(DECAY, (1 + t) / (10 + t)), in Python doubles."""
    return min(float(decay), (1.0 + t) / (10.0 + t))


def weight_at(decay, t):
    """w = float32(1 - d_t)."""
    return F(1.0 - decay_at(decay, t))


class SgdEma:
    """``params`` / ``emas``: lists of float32 arrays (the averages start as copies); ``lrs`` / ``wds``: per-parameter Python
    floats, read at every step (the caller's schedule moves them); one momentum for all."""

    def __init__(self, params, lrs, wds, momentum, decay):
        self.params = [np.array(p, dtype=F) for p in params]
        self.emas = [p.copy() for p in self.params]
        self.bufs = [None] * len(self.params)
        self.lrs, self.wds, self.momentum, self.decay = list(lrs), list(wds), float(momentum), float(decay)
        self.t = 0

    def step(self, grads):
        """``grads[i]`` None: parameter i is skipped -- no SGD update, no momentum update, no EMA update."""
        w = weight_at(self.decay, self.t)
        any_decay = any(wd != 0 for wd in self.wds)  # torch's multi-tensor form decays all or none (g + p * 0 = g)
        for i, g in enumerate(grads):
            if g is None:
                continue
            p = self.params[i]
            g = np.asarray(g, dtype=F)
            d = g + p * F(self.wds[i]) if any_decay else g
            if self.momentum != 0:
                self.bufs[i] = d.copy() if self.bufs[i] is None else self.bufs[i] * F(self.momentum) + d
                upd = self.bufs[i]
            else:
                upd = d
            p = p + upd * F(-self.lrs[i])
            diff = p - self.emas[i]
            self.emas[i] = self.emas[i] + diff * w
            self.params[i] = p
        self.t += 1
