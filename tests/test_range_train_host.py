"""`ops.with_range_fallback_training` on the host: what it saves before the first attempt (BatchNorm running statistics and
counters, the generator state) and puts back before the rerun, on a CPU nn.Sequential with two BatchNorm layers -- no device:
`ops.split_overflow` and `ops.CONV_PRECISION` are patched.  The device side is tests/test_gpu_range_train.py."""
import copy

import pytest
import torch
from torch import nn


def _net(dtype=torch.float32):
    gen = torch.Generator().manual_seed(5)
    net = nn.Sequential(nn.Linear(8, 8), nn.BatchNorm1d(8), nn.ReLU(), nn.Dropout(0.25), nn.Linear(8, 4), nn.BatchNorm1d(4))
    with torch.no_grad():
        for p in net.parameters():
            p.copy_(torch.randn(p.shape, generator=gen))
        for bn in (net[1], net[5]):
            bn.running_mean.copy_(torch.randn(bn.running_mean.shape, generator=gen))
            bn.running_var.copy_(torch.rand(bn.running_var.shape, generator=gen) + 0.5)
    x = torch.randn((12, 8), generator=gen)
    return net.to(dtype).train(), x.to(dtype)


def _buffers(net):
    return {k: v.clone() for k, v in net.named_buffers()}


@pytest.fixture
def host_ops(monkeypatch):
    from dualfusion import ops
    monkeypatch.setattr(ops, "split_overflow", lambda reset=True: (False, ""))
    monkeypatch.setattr(ops, "CONV_PRECISION", "split")
    monkeypatch.setattr(ops, "_RANGE_WARNED", [True])
    monkeypatch.setitem(ops.RANGE_STATS, "range_fallbacks", ops.RANGE_STATS["range_fallbacks"])
    rng = torch.get_rng_state()
    yield ops
    torch.set_rng_state(rng)


def _plain_call(net, x, seed):
    """One forward of a copy of `net` from the generator state `seed` selects: (buffers, generator state, output)."""
    ref = copy.deepcopy(net)
    torch.manual_seed(seed)
    y = ref(x)
    return _buffers(ref), torch.get_rng_state(), y.detach()


def _leaves_range_once(ops, net, x, calls):
    def fn(inp):
        calls.append(ops.CONV_PRECISION)
        if len(calls) == 1:
            # the attempt that leaves the range: its rows hold inf / NaN, the BatchNorm layers take them into their statistics
            net(inp * float("inf"))
            raise ops.SplitRangeError("left the range")
        return net(inp)
    return fn


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_rerun_starts_from_the_saved_batchnorm_and_generator_state(host_ops, dtype):
    ops = host_ops
    net, x = _net(dtype)
    want, want_rng, want_y = _plain_call(net, x, 11)
    calls = []
    before = ops.RANGE_STATS["range_fallbacks"]
    torch.manual_seed(11)
    y = ops.with_range_fallback_training(net, _leaves_range_once(ops, net, x, calls), x)
    assert calls == ["split", "split3"]                                    # fn ran twice, the rerun on three parts
    assert ops.CONV_PRECISION == "split"
    assert ops.RANGE_STATS["range_fallbacks"] == before + 1
    got = _buffers(net)
    assert sorted(got) == sorted(want) and len(got) == 6
    for k in want:
        assert torch.isfinite(got[k].double()).all() and torch.equal(got[k], want[k]), k
    assert int(net[1].num_batches_tracked) == int(net[5].num_batches_tracked) == 1
    assert torch.equal(torch.get_rng_state(), want_rng)
    assert torch.equal(y.detach(), want_y)                                 # (the same dropout mask as the plain call)


def test_plain_form_restores_nothing(host_ops):
    """`with_range_fallback` is the inference form: a train() forward through it keeps the first attempt's update."""
    ops = host_ops
    net, x = _net()
    calls = []
    ops.with_range_fallback(_leaves_range_once(ops, net, x, calls), x)
    assert calls == ["split", "split3"]
    assert int(net[1].num_batches_tracked) == 2 and not torch.isfinite(net[1].running_var).all()


def test_saved_copies_follow_replaced_buffers_and_a_list_of_modules(host_ops):
    ops = host_ops
    net, x = _net()
    ops.with_range_fallback_training(net, net, x)                          # in range: builds the copies' storage
    assert int(net[1].num_batches_tracked) == 1
    net = net.double()                                                     # new buffer tensors
    x = x.double()
    want, want_rng, _ = _plain_call(net, x, 3)
    torch.manual_seed(3)
    ops.with_range_fallback_training([net[:4], net[4:]], _leaves_range_once(ops, net, x, []), x)
    got = _buffers(net)
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert int(net[5].num_batches_tracked) == 2 and torch.equal(torch.get_rng_state(), want_rng)


def test_other_exceptions_pass_with_the_state_as_fn_left_it(host_ops):
    ops = host_ops
    net, x = _net()
    want, want_rng, _ = _plain_call(net, x, 7)
    calls = []

    def fn(inp):
        calls.append(1)
        net(inp)
        raise ValueError("unrelated")

    before = ops.RANGE_STATS["range_fallbacks"]
    torch.manual_seed(7)
    with pytest.raises(ValueError, match="unrelated"):
        ops.with_range_fallback_training(net, fn, x)
    assert len(calls) == 1 and ops.RANGE_STATS["range_fallbacks"] == before
    got = _buffers(net)
    for k in want:
        assert torch.equal(got[k], want[k]), k                            # one update: nothing was rolled back
    assert torch.equal(torch.get_rng_state(), want_rng)
    # outside the two-part mode a SplitRangeError is nobody's to rerun either
    ops.CONV_PRECISION = "split3"
    with pytest.raises(ops.SplitRangeError):
        ops.with_range_fallback_training(net, _leaves_range_once(ops, net, x, []), x)
    assert int(net[1].num_batches_tracked) == 2
