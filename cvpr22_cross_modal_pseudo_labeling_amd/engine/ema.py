"""Exponential moving average (EMA) of the trained weights: the weights that get evaluated and shipped when the student learns
from noisy pseudo labels (``tools/train_net.py --ema DECAY``, ``tools/infer_net.py --ema``).

The rule is stated in full in include/ovis_hip.h next to ``ovis_sgd_momentum_ema_multi_f32``.  In brief: one fp32 average per
parameter with ``requires_grad``, keyed by its name, started as a copy of the parameters when the object is made; at optimizer
step t (counted from 0) behind the SGD update,  d_t = min(DECAY, (1 + t) / (10 + t)),  w = float32(1 - d_t),
diff = p_new - e;  e = e + diff * w  in fp32 with three roundings.  The update itself belongs to the optimizer
(``engine/solver.py::GroupFusedSGD.ema``: inside the fused SGD launch on the device, three multi-tensor ops elsewhere); this
module holds the tensors, the count, the checkpoint entry and the exchange that lets a model compute with the averages.
"""
import contextlib
from collections import OrderedDict

import numpy as np
import torch


def decay_at(decay, t):
    """d_t of the rule, in Python doubles: the warm-up (1 + t) / (10 + t) until it crosses ``decay``."""
    return min(float(decay), (1 + t) / (10 + t))


def weight_at(decay, t):
    """w = float32(1 - d_t), as the Python float that holds exactly that float32."""
    return float(np.float32(1.0 - decay_at(decay, t)))


class ModelEma:
    """``tensors`` {name: fp32 tensor on the parameter's device} over ``model.named_parameters()`` with ``requires_grad``,
    ``decay`` and ``num_updates`` (t).  Attach it to the optimizer (``optimizer.ema = ema``): every optimizer step then moves
    the averages of the parameters it updates and counts one update."""

    def __init__(self, model, decay):
        decay = float(decay)
        if not 0.0 < decay < 1.0:
            raise ValueError(f"ModelEma: decay must be a float in (0, 1), got {decay}")
        self.decay = decay
        self.num_updates = 0
        self.tensors = OrderedDict()
        self._names = {}  # id(parameter) -> name; the parameters are kept alive by ``_params``
        self._params = OrderedDict()
        self._swap_table = None
        for name, p in model.named_parameters():
            if not p.requires_grad:
                continue
            if p.dtype != torch.float32:
                raise ValueError(f"ModelEma: {name} is {p.dtype}; the average is kept for float32 parameters")
            self.tensors[name] = p.detach().clone(memory_format=torch.contiguous_format)
            self._names[id(p)] = name
            self._params[name] = p

    def weight(self):
        """w of the NEXT update (the optimizer reads it, updates, then counts)."""
        return weight_at(self.decay, self.num_updates)

    def tensor_of(self, param):
        """The average of a parameter object of the model this was made from."""
        name = self._names.get(id(param))
        if name is None:
            raise ValueError("ModelEma: the optimizer updates a parameter that is no trainable parameter of the averaged model")
        return self.tensors[name]

    # ---- checkpoint entry ---------------------------------------------------------------------------------------------------
    def state_dict(self):
        """{"num_updates": t, "params": {name: tensor}} -- the tensors themselves, as ``Module.state_dict`` hands out."""
        return {"num_updates": self.num_updates, "params": OrderedDict(self.tensors)}

    def load_state_dict(self, state):
        """Restores the averages (as NEW tensors: the optimizer's cached tables notice) and ``num_updates``; ``decay`` stays
        the caller's.  A key or a shape that does not match the model's trainable parameters is a ValueError naming the key."""
        params = check_ema_entry(state, self._params)
        fresh = OrderedDict()
        for name, p in self._params.items():
            fresh[name] = params[name].detach().to(device=p.device, dtype=torch.float32).clone(memory_format=torch.contiguous_format)
        self.tensors = fresh
        self.num_updates = int(state["num_updates"])
        self._swap_table = None

    # ---- computing with the averages ----------------------------------------------------------------------------------------
    @torch.no_grad()
    def swap(self, model):
        """Exchange every trainable parameter of ``model`` with its average, bit for bit and in place: values move, pointers
        stay (the optimizer's tables, the reducer's gradient views and every Parameter object stay valid).  Device tensors:
        ONE launch (``_C.swap_multi``); host tensors: a three-assignment exchange.  Everything prepared from the weights
        before is stale afterwards (``note_weights_written``)."""
        from ..layers.pair_bottleneck import note_weights_written

        live = dict(model.named_parameters())
        pairs = []
        for name, e in self.tensors.items():
            p = live.get(name)
            if p is None or p.shape != e.shape or p.device != e.device or p.dtype != e.dtype:
                raise ValueError(f"ModelEma: {name} of the model does not match its average (missing, or another shape, "
                                 "device or dtype)")
            pairs.append((p, e))
        if pairs and all(p.is_cuda for p, _ in pairs):
            self._swap_native(pairs)
        else:
            for p, e in pairs:
                held = p.detach().clone()
                p.detach().copy_(e)
                e.copy_(held)
        note_weights_written()

    def _swap_native(self, pairs):
        from .. import _C

        if not all(p.is_contiguous() and e.is_contiguous() and p.device == pairs[0][0].device for p, e in pairs):
            raise RuntimeError("ModelEma: the swap launch takes contiguous tensors on one HIP device")
        sig = tuple((p.data_ptr(), e.data_ptr(), p.numel()) for p, e in pairs)
        if self._swap_table is None or self._swap_table[0] != sig:
            chunk = _C.sgd_chunk_elements()
            dev = pairs[0][0].device
            items = np.array(sig, dtype=np.int64).reshape(-1, 3)
            blocks = [(j, c) for j, (_, _, n) in enumerate(sig) for c in range((n + chunk - 1) // chunk)]
            self._swap_table = (sig, torch.from_numpy(items.view(np.uint8).reshape(-1)).to(dev),
                                torch.tensor(blocks, dtype=torch.int32, device=dev).reshape(-1, 2))
        _C.swap_multi(self._swap_table[1], self._swap_table[2])

    @contextlib.contextmanager
    def applied(self, model):
        """Inside the context ``model`` computes with the averaged weights on every route (the raw weights rest in
        ``tensors``); on exit the exchange is undone and, where the trainer prepares the pair-layout operands behind the
        optimizer step (modeling/backbone.py::prepare_weights_ahead), they are prepared again from the raw weights: the next
        training step sees exactly what it would have seen."""
        self.swap(model)
        try:
            yield self
        finally:
            self.swap(model)
            from ..layers.pair_bottleneck import WeightPrepPlan
            if isinstance(model.__dict__.get("_ovis_prep_plan"), WeightPrepPlan):
                from ..modeling.backbone import prepare_weights_ahead
                prepare_weights_ahead(model)


def check_ema_entry(state, trainable):
    """The ``params`` of a checkpoint's ``"ema"`` entry, checked against ``trainable`` {name: parameter}: a missing key, an
    unknown key or another shape is a ValueError naming the key."""
    if not isinstance(state, dict) or "params" not in state or "num_updates" not in state:
        raise ValueError("ModelEma: an entry {'num_updates', 'params'} expected (key 'params' or 'num_updates' is missing)")
    params = state["params"]
    for name, p in trainable.items():
        if name not in params:
            raise ValueError(f"ModelEma: the entry has no average for the trainable parameter {name}")
        if tuple(params[name].shape) != tuple(p.shape):
            raise ValueError(f"ModelEma: the average of {name} has shape {tuple(params[name].shape)}, the parameter "
                             f"{tuple(p.shape)}")
    for name in params:
        if name not in trainable:
            raise ValueError(f"ModelEma: the entry's key {name} is no trainable parameter of the model")
    return params


@torch.no_grad()
def load_ema_weights(model, state):
    """``tools/infer_net.py --ema``: the averages of a checkpoint's ``"ema"`` entry over the model's trainable parameters."""
    trainable = OrderedDict((name, p) for name, p in model.named_parameters() if p.requires_grad)
    params = check_ema_entry(state, trainable)
    for name, p in trainable.items():
        p.copy_(params[name].to(device=p.device, dtype=p.dtype))
