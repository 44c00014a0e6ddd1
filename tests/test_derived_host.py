"""`dualfusion.derived`: the one keyed cache of everything derived from parameters and buffers, on CPU tensors.  Each case
uses a counting `build`: a hit returns the same object without calling it, every supported state change calls it once."""
import gc
import weakref

import pytest
import torch
from torch import nn

from dualfusion.derived import derived, slot_tensors, state_slots


class _Build(object):
    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return [self.calls]                       # a fresh object per build


def _linear_pack(lin, build, extra=()):
    return derived(lin.__dict__, "_pack", (lin.weight, lin.bias), build, extra)


def test_hit_returns_the_same_object_without_building():
    lin, build = nn.Linear(3, 2), _Build()
    a = _linear_pack(lin, build)
    assert _linear_pack(lin, build) is a and build.calls == 1
    assert lin.__dict__["_pack"][1] is a          # the slot layout: (key, value)


def test_in_place_edit_rebuilds():
    lin, build = nn.Linear(3, 2), _Build()
    a = _linear_pack(lin, build)
    with torch.no_grad():
        lin.weight.add_(1)
    b = _linear_pack(lin, build)
    assert b is not a and build.calls == 2
    assert _linear_pack(lin, build) is b and build.calls == 2


def test_load_state_dict_rebuilds():
    lin, build = nn.Linear(3, 2), _Build()
    _linear_pack(lin, build)
    lin.load_state_dict({k: v + 1 for k, v in lin.state_dict().items()})
    _linear_pack(lin, build)
    assert build.calls == 2


def test_double_float_replaces_buffers_and_later_edits_are_seen():
    bn, build = nn.BatchNorm1d(4).eval(), _Build()
    slots = state_slots(bn)                        # collected once, as the modules do

    def get():
        return derived(bn.__dict__, "_fold", slot_tensors(slots), build)
    get()
    old_mean = bn.running_mean
    bn.double().float()
    assert bn.running_mean is not old_mean         # nn.Module._apply: new buffer objects
    get()
    assert build.calls == 2
    with torch.no_grad():
        bn.running_mean.add_(0.5)                  # the live buffer: a list of the tensors collected before would miss it
    get()
    assert build.calls == 3
    get()
    assert build.calls == 3


def test_new_parameter_in_the_second_tensor_rebuilds():
    a, b, build = nn.Linear(3, 3), nn.Linear(3, 3), _Build()

    def get():
        return derived(a.__dict__, "_ffn", (a.weight, b.weight), build)
    get()
    b.weight = nn.Parameter(b.weight.detach().clone())         # same values and version, another address
    get()
    assert build.calls == 2


def test_none_is_accepted_and_none_to_tensor_rebuilds():
    lin, build = nn.Linear(3, 2, bias=False), _Build()
    a = _linear_pack(lin, build)
    assert _linear_pack(lin, build) is a and build.calls == 1
    lin.bias = nn.Parameter(torch.zeros(2))
    assert _linear_pack(lin, build) is not a and build.calls == 2


def test_extra_rebuilds():
    lin, build = nn.Linear(3, 2), _Build()
    a = _linear_pack(lin, build, ("split",))
    assert _linear_pack(lin, build, ("split",)) is a
    assert _linear_pack(lin, build, ("split3",)) is not a and build.calls == 2


def test_two_names_in_one_dict_are_independent():
    lin, b1, b2 = nn.Linear(3, 2), _Build(), _Build()
    x = derived(lin.__dict__, "_a", (lin.weight,), b1)
    y = derived(lin.__dict__, "_b", (lin.bias,), b2)
    with torch.no_grad():
        lin.bias.add_(1)
    assert derived(lin.__dict__, "_a", (lin.weight,), b1) is x and b1.calls == 1
    assert derived(lin.__dict__, "_b", (lin.bias,), b2) is not y and b2.calls == 2


def test_the_value_dies_with_its_owner():
    class Value(object):
        pass
    lin = nn.Linear(3, 2)
    ref = weakref.ref(_linear_pack(lin, Value))
    assert ref() is not None
    del lin
    gc.collect()
    assert ref() is None                           # nothing global holds it


def test_fold_batchnorm_on_cpu():
    try:
        from dualfusion.spconv.modules import fold_batchnorm
    except (ImportError, OSError) as e:            # the package wants the native library on this box
        pytest.skip("dualfusion.spconv.modules: %s" % e)
    torch.manual_seed(0)
    bn = nn.BatchNorm1d(5, eps=1e-3).eval()
    with torch.no_grad():
        for t in (bn.weight, bn.bias, bn.running_mean):
            t.copy_(torch.randn(5))
        bn.running_var.copy_(torch.rand(5) + 0.5)
    pair = fold_batchnorm(bn)
    assert fold_batchnorm(bn) is pair
    for t in (bn.weight, bn.bias, bn.running_mean, bn.running_var):
        with torch.no_grad():
            t.mul_(1.25)
        new = fold_batchnorm(bn)
        assert new is not pair and fold_batchnorm(bn) is new
        pair = new
        scale = bn.weight * torch.rsqrt(bn.running_var + bn.eps)
        assert torch.equal(pair[0], scale) and torch.equal(pair[1], bn.bias - bn.running_mean * scale)
