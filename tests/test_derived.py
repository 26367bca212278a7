"""Host: the one rule for values derived from weights (layers/derived.py) -- when a stored value is served, when it is
rebuilt, that nothing is kept for trainable sources and that entries die with their source -- on the helper itself and on its
two host-reachable users, ``FrozenBatchNorm2d.fold`` and ``ConvBN.folded``."""
import gc

import pytest
import torch
from torch import nn

from cvpr22_cross_modal_pseudo_labeling_amd.layers import FrozenBatchNorm2d
from cvpr22_cross_modal_pseudo_labeling_amd.layers.derived import _STORE, derived
from cvpr22_cross_modal_pseudo_labeling_amd.modeling.backbone import ConvBN


class Doubled:
    """``build`` of 2 * (a + b) that counts its runs."""

    def __init__(self, *sources):
        self.sources, self.runs = sources, 0

    def build(self):
        self.runs += 1
        return 2 * sum(self.sources)

    def __call__(self):
        return derived(self.sources, "doubled", self.build)


def _conv_bn(seed=0):
    g = torch.Generator().manual_seed(seed)
    conv = nn.Conv2d(3, 4, 3, bias=False)
    conv.weight.requires_grad = False
    bn = FrozenBatchNorm2d(4)
    for b in bn.buffers():
        b.copy_(torch.rand(4, generator=g) + 0.5)
    return ConvBN(conv, bn)


def _fold_formula(bn):
    scale = bn.weight * bn.running_var.rsqrt()
    return scale, bn.bias - bn.running_mean * scale


def test_second_call_returns_the_stored_object():
    d = Doubled(torch.ones(3), torch.ones(3))
    first = d()
    assert d() is first and d.runs == 1
    assert torch.equal(first, torch.full((3,), 4.0))
    assert derived(d.sources, "other slot", lambda: "x") == "x" and d() is first  # slots of one tensor do not collide


@pytest.mark.parametrize("which", [0, 1])
def test_copy_under_no_grad_on_any_source_rebuilds(which):
    d = Doubled(torch.ones(3), torch.ones(3))
    first = d()
    with torch.no_grad():
        d.sources[which].copy_(torch.full((3,), 5.0))
    second = d()
    assert d.runs == 2 and second is not first and torch.equal(second, torch.full((3,), 12.0))


def test_inplace_write_on_data_is_not_seen():
    """The known limit for sources that do not require grad: ``.data`` carries its own version counter."""
    d = Doubled(torch.ones(3), torch.ones(3))
    first = d()
    d.sources[0].data.fill_(7.0)
    assert d() is first and d.runs == 1


def test_data_swap_rebuilds():
    p = nn.Parameter(torch.ones(3), requires_grad=False)
    d = Doubled(p, torch.ones(3))
    d()
    version = p._version
    p.data = torch.full((3,), 2.0)
    assert p._version == version  # the swap moves the pointer only
    assert torch.equal(d(), torch.full((3,), 6.0)) and d.runs == 2


def test_module_double_rebuilds_in_the_new_dtype():
    m = _conv_bn()
    w32, b32 = m.folded()
    assert w32.dtype == torch.float32 and m.folded()[0] is w32
    m.double()
    w64, b64 = m.folded()
    assert w64.dtype == torch.float64 and b64.dtype == torch.float64
    scale, shift = _fold_formula(m.bn)
    assert torch.equal(w64, m.conv.weight * scale.reshape(-1, 1, 1, 1)) and torch.equal(b64, shift)


def test_trainable_source_builds_every_call_and_stores_nothing():
    p = nn.Parameter(torch.ones(3))
    d = Doubled(torch.ones(3), p)
    before = len(_STORE)
    a, b = d(), d()
    assert d.runs == 2 and a is not b
    assert a.requires_grad  # built in the caller's grad mode
    with torch.no_grad():
        assert not d().requires_grad
    assert len(_STORE) == before and d.sources[0] not in _STORE


def test_entries_die_with_their_source():
    gc.collect()
    before = len(_STORE)
    d = Doubled(torch.ones(3), torch.ones(3))
    d()
    assert len(_STORE) == before + 1
    del d
    gc.collect()
    assert len(_STORE) == before
    kept = []
    for i in range(200):
        t = torch.full((3,), float(i))
        assert torch.equal(derived((t,), "doubled", lambda: 2 * t), torch.full((3,), 2.0 * i))
        if i % 50 == 0:
            kept.append(t)
    del t
    gc.collect()
    assert len(_STORE) <= before + len(kept)


def test_fold_returns_identical_tensors_until_the_buffers_change():
    bn = _conv_bn().bn
    scale, shift = bn.fold()
    for _ in range(3):
        again = bn.fold()
        assert again[0] is scale and again[1] is shift
    want = _fold_formula(bn)
    assert torch.equal(scale, want[0]) and torch.equal(shift, want[1])


def test_fold_follows_load_state_dict():
    bn = _conv_bn(0).bn
    scale, shift = bn.fold()
    bn.load_state_dict(_conv_bn(1).bn.state_dict())
    new_scale, new_shift = bn.fold()
    assert new_scale is not scale and new_shift is not shift
    want = _fold_formula(bn)
    assert torch.equal(new_scale, want[0]) and torch.equal(new_shift, want[1])
    assert not torch.equal(new_scale, scale)


def test_folded_conv_follows_weight_and_buffers():
    m = _conv_bn()
    w, b = m.folded()
    assert m.folded()[0] is w and m.folded()[1] is b
    with torch.no_grad():
        m.bn.running_var.copy_(torch.full((4,), 4.0))  # a buffer is a source of the folded weight
    w2, b2 = m.folded()
    scale, shift = _fold_formula(m.bn)
    assert w2 is not w and torch.equal(w2, m.conv.weight * scale.reshape(-1, 1, 1, 1)) and torch.equal(b2, shift)
    m.conv.weight.data = torch.ones_like(m.conv.weight)
    assert torch.equal(m.folded()[0], scale.reshape(-1, 1, 1, 1).expand_as(m.conv.weight))
    m.conv.weight.requires_grad = True  # a trainable convolution: folded in the graph, on every call
    w3 = m.folded()[0]
    assert w3.requires_grad and m.folded()[0] is not w3
