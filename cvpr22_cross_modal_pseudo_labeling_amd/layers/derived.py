"""Values computed from weights (folded FrozenBN affines, folded convolution weights, pair-layout GEMM operands) and the
ONE rule for when such a value may be served again: ``derived(sources, slot, build)``.
* A stored value is served, as the very object that was stored, while every tensor of ``sources`` is the same object with the
  same ``_version``, ``data_ptr()``, device and dtype as when ``build()`` made it (``module.to()`` and ``p.data = other`` keep a
  Parameter and its version: only pointer, device or dtype move).  Anything else rebuilds.
* When any source requires grad nothing is stored or served: ``build()`` runs, in the caller's grad mode, on every call.  The
  fused SGD launch and ``.data`` writes go through raw pointers, so no key sees them (for a source that does NOT require grad
  that is the known limit); training prepares its operands behind the optimizer step (pair_bottleneck.py::WeightPrepPlan).
* Values live in one weak dictionary keyed on the first source, ``{slot: (key, value, other sources)}``, and die with that
  tensor.  The entry holds the other sources, so no ``id`` in its key can be a dead tensor's.  No lock: a lookup or a store
  is one dictionary operation, and two threads that both miss both build."""
from torch.utils.weak import WeakIdKeyDictionary

_STORE = WeakIdKeyDictionary()


def derived(sources, slot, build):
    key = []
    for t in sources:
        if t.requires_grad:
            return build()
        key.append((id(t), t._version, t.data_ptr(), t.device, t.dtype))
    slots = _STORE.setdefault(sources[0], {})
    hit = slots.get(slot)
    if hit is None or hit[0] != key:
        hit = slots[slot] = (key, build(), tuple(sources[1:]))
    return hit[1]
