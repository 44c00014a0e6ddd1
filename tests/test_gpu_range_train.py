"""The fp16 operand format's range fallback under a TRAINING forward (`ops.with_range_fallback_training`, used by
`TransFusionDetector.training_step`): the attempt that leaves the range has already updated every BatchNorm's running
statistics (from rows that hold inf / NaN), counted a batch and drawn dropout seeds when the flag is read.  The rerun on three
bf16 parts must start from the state the step began with: ONE momentum update, one count, one forward's worth of the device
generator -- pinned to the same chain / the same step on the host in float64, evaluated once."""
import copy
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P_DROP = 0.1
SEED = 1234


class _Saved(object):
    """CONV_PRECISION, the once-only warning and both generators as the test found them."""

    def __enter__(self):
        from dualfusion import ops
        self.ops = ops
        self.state = (ops.CONV_PRECISION, ops._RANGE_WARNED[0], torch.get_rng_state(), torch.cuda.get_rng_state(DEV))
        ops.CONV_PRECISION = "split"
        ops.split_overflow(reset=True)
        return ops

    def __exit__(self, *exc):
        ops = self.ops
        ops.CONV_PRECISION, ops._RANGE_WARNED[0] = self.state[:2]
        torch.set_rng_state(self.state[2])
        torch.cuda.set_rng_state(self.state[3], DEV)
        ops.split_overflow(reset=True)                       # the flag these tests raise on purpose
        return False


# ------------------------------------------------------------------------------------------------ a. one chain of row kernels
_cases = {}


def _case(n, c, big):
    """Rows x [n, cc] (cc = the narrowest convolution that serves c channels), a cc -> cc filter, BatchNorm1d(c) buffers, and
    the chain conv -> [:, :c] -> BatchNorm(train) -> ReLU in float64: (running_mean, running_var, rectified output)."""
    key = (n, c, big)
    if key not in _cases:
        cc = max(c, 32)
        gen = torch.Generator().manual_seed(1000 * n + c)
        x = torch.randn((n, cc), generator=gen)
        if big:
            k = min(40, n * cc // 4)                          # a few dozen entries beyond the two-part format's |x| < 2047
            at = torch.randperm(n * cc, generator=gen)[:k]
            x.view(-1)[at] = (2047.0 + 2000.0 * torch.rand(k, generator=gen)) * torch.sign(torch.randn(k, generator=gen))
            assert int((x.abs() >= 2047).sum()) == k
        w = torch.randn((1, cc, cc), generator=gen) * (0.5 / np.sqrt(cc))
        bn = torch.nn.BatchNorm1d(c, eps=1e-3, momentum=0.1).train()
        with torch.no_grad():
            bn.weight.copy_(torch.randn(c, generator=gen))
            bn.bias.copy_(torch.randn(c, generator=gen))
            bn.running_mean.copy_(torch.randn(c, generator=gen))
            bn.running_var.copy_(torch.rand(c, generator=gen) + 0.5)
        ref = copy.deepcopy(bn).double()
        with torch.no_grad():
            y = (x.double() @ w[0].double())[:, :c]
            h = torch.relu(ref(y))
            # What the rows' own rounding may move in the output.  The device's rows y are of fp32 grade: within 4e-6 of
            # their largest entry (the bound test_gpu_ops grants the two-part kernel against float64).  BatchNorm over batch
            # statistics passes a perturbation of its input rows on with sum_j |d xhat_i / d y_j| = rstd * sum_j |delta_ij -
            # 1 / n - xhat_i xhat_j / n| <= rstd * (2 + |xhat_i|) (mean |xhat| <= 1), times |weight|: next to nothing in a
            # channel of ordinary spread, everything in one whose rows nearly coincide (n = 2: xhat = +-1 by cancellation).
            rstd = (y.var(0, unbiased=False) + ref.eps).rsqrt()
            xhat = (y - y.mean(0)) * rstd
            slack = ref.weight.abs() * rstd * (2.0 + xhat.abs()) * (4e-6 * float(y.abs().max()))
        assert int(ref.num_batches_tracked) == 1
        _cases[key] = dict(x=x, w=w, bn=bn, mean=ref.running_mean.clone(), var=ref.running_var.clone(), h=h, c=c, slack=slack)
    return _cases[key]


def _chain(ops, case, bn, x, w):
    n = x.shape[0]
    y, _ = ops.conv(ops.ConvFilters(w), ops.identity_table(n, x.device), n, rows=x, want_operand=False)
    if case["c"] != y.shape[1]:
        y = y[:, :case["c"]].contiguous()
    h = ops.batch_norm_rows(bn, y, relu=True)
    h = ops.relu_dropout_(h, P_DROP, ops._dropout_seed(h.device))
    ops.read_with_range_flag(torch.zeros((1,), dtype=torch.int32, device=x.device))
    return h.detach()


def _rel(a, b):
    return float((a.detach().cpu().double() - b).abs().max() / max(1e-9, float(b.abs().max())))


def _run(ops, case, how):
    """The chain on a fresh copy of the case's BatchNorm after torch.manual_seed(SEED): how = "fallback" (the training
    entry), "split3" (the three-part mode outright).  -> (bn, output, offset of the device generator after the call)."""
    bn = copy.deepcopy(case["bn"]).to(DEV)
    x, w = case["x"].to(DEV), case["w"].to(DEV)
    gen = torch.cuda.default_generators[0]
    torch.manual_seed(SEED)
    assert gen.get_offset() == 0
    if how == "fallback":
        h = ops.with_range_fallback_training(bn, _chain, ops, case, bn, x, w)
    else:
        with ops.precision(how):
            h = _chain(ops, case, bn, x, w)
    return bn, h, gen.get_offset()


def _buffers_hold_one_update(bn, case):
    assert int(bn.num_batches_tracked) == 1
    assert torch.isfinite(bn.running_mean).all() and torch.isfinite(bn.running_var).all()
    err = _rel(bn.running_mean, case["mean"]), _rel(bn.running_var, case["var"])
    print("running_mean / running_var against float64:", err)
    assert err[0] < 1e-5 and err[1] < 1e-5, err


def _output_is_the_dropped_out_reference(ops, h, case):
    """Kept entries = the float64 chain's / (1 - p), to 1e-5 of the largest (the output bound of
    test_batch_norm_rows_kernels_vs_float64) plus what the rows' rounding moves (`_case`: slack); of the reference's positive
    entries the share p is zero."""
    keep = 1.0 - ops._dropout_threshold(P_DROP) / 16777216.0
    want = case["h"] / keep
    got = h.cpu().double()
    kept = got != 0
    excess = ((got - want).abs() - case["slack"] / keep) * kept
    print("output against float64 beyond the rows' rounding: %.3g of the largest" % (float(excess.max()) / float(want.abs().max())))
    assert float(excess.max()) <= 1e-5 * float(want.abs().max())
    positive = want > 1e-4 * float(want.abs().max())         # (clear of the rectifier's edge)
    m = int(positive.sum())
    dropped = int((positive & ~kept).sum())
    if m >= 2000:                                            # 6 standard deviations of a binomial share
        assert abs(dropped / m - P_DROP) <= 6.0 * np.sqrt(P_DROP * (1 - P_DROP) / m), (dropped, m)
    else:
        assert dropped <= m // 2


@pytest.mark.parametrize("n,c", [(300, 64), (300, 16), (2, 64)])
def test_chain_out_of_range_leaves_one_batchnorm_update_and_one_seed(n, c):
    with _Saved() as ops:
        assert ops.bn_rows_supported(c) and ops.conv_kind(1, max(c, 32), max(c, 32)) == "split"
        case, small = _case(n, c, True), _case(n, c, False)
        _, _, plain_offset = _run(ops, small, "fallback")                      # one in-range call: what one forward draws
        assert plain_offset > 0
        before = ops.RANGE_STATS["range_fallbacks"]
        bn, h, offset = _run(ops, case, "fallback")
        assert ops.RANGE_STATS["range_fallbacks"] == before + 1
        _buffers_hold_one_update(bn, case)
        assert offset == plain_offset, (offset, plain_offset)
        _output_is_the_dropped_out_reference(ops, h, case)
        # the rerun IS a three-part forward from the seed the step began with: the same mask, the same values
        _, again, _ = _run(ops, case, "fallback")
        bn3, want, offset3 = _run(ops, case, "split3")
        assert ops.RANGE_STATS["range_fallbacks"] == before + 2
        assert offset3 == plain_offset
        assert torch.equal(again == 0, want == 0) and torch.equal(again, want) and torch.equal(h, want)
        assert torch.equal(bn.running_var, bn3.running_var) and torch.equal(bn.running_mean, bn3.running_mean)


@pytest.mark.parametrize("n,c", [(300, 64), (300, 16), (2, 64)])
def test_chain_in_range_takes_no_fallback_and_one_update(n, c):
    with _Saved() as ops:
        case = _case(n, c, False)
        before = ops.RANGE_STATS["range_fallbacks"]
        bn, h, _ = _run(ops, case, "fallback")
        assert ops.RANGE_STATS["range_fallbacks"] == before
        assert not ops.split_overflow(reset=True)[0]
        _buffers_hold_one_update(bn, case)
        _output_is_the_dropped_out_reference(ops, h, case)


# ------------------------------------------------------------------------------------------------ b. the reduced TransFusion step
SCALED = ["pts_middle_encoder.conv_input.1"] + ["pts_middle_encoder.encoder_layers.encoder_layer%d.2.1" % i for i in (1, 2, 3)]


def _batchnorms(det):
    return [(k, m) for k, m in det.named_modules() if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)]


def test_training_step_out_of_range_updates_every_batchnorm_once():
    """One `training_step` of the reduced TransFusion-L + 3D-DF detector from a checkpoint whose BatchNorm scales behind the
    stem and the strided stages are x 400 (the recipe of test_gpu_range._detector): the forward leaves the two-part format's
    range, is rerun on three bf16 parts, and the step leaves what one float64 forward leaves -- in every BatchNorm's buffers
    and counter, in the losses and in the gradients (the statements of test_training_step_gradients_vs_float64_composition)."""
    import test_gpu_tftrain as tt
    from dualfusion.spconv.conv import SparseConvolution
    seen = dict(peak=0.0, layers=0)

    def hook(conv, inputs, output):
        rows = inputs[0].features
        if rows.dtype == torch.float64 and seen["ops"].conv_kind(int(np.prod(conv.kernel_size)), conv.in_channels,
                                                                  conv.out_channels) == "split":
            seen["layers"] += 1
            seen["peak"] = max(seen["peak"], float(rows.detach().abs().max()))

    def prepare(det):
        with torch.no_grad():
            for name in SCALED:
                bn = det.get_submodule(name)
                assert isinstance(bn, torch.nn.BatchNorm1d)
                bn.weight.mul_(400.0)
        seen["counts"] = {k: int(m.num_batches_tracked) for k, m in _batchnorms(det)}
        for m in det.modules():
            if isinstance(m, SparseConvolution):
                m.register_forward_hook(hook)

    with _Saved() as ops:
        seen["ops"] = ops
        ops._RANGE_WARNED[0] = False
        before = ops.RANGE_STATS["range_fallbacks"]
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            logs, logs64, rows, (det, d64, d32) = tt._step_three_ways(smooth=False, prepare=prepare)
        # the float64 model's rows do leave |x| < 2047 in front of a convolution the two-part kernels serve
        assert seen["layers"] > 0 and seen["peak"] > 2047.0, seen["peak"]
        assert np.isfinite(logs64["loss"])
        assert ops.RANGE_STATS["range_fallbacks"] == before + 1
        assert sum("three-part" in str(w.message) for w in caught) == 1
        names = [k for k, _ in _batchnorms(det)]
        assert len(names) == 38 and names == [k for k, _ in _batchnorms(d64)]
        got, want, plain = dict(det.named_buffers()), dict(d64.named_buffers()), dict(d32.named_buffers())
        worst = (0.0, 0.0, None)
        for k in names:
            assert int(got[k + ".num_batches_tracked"]) == int(want[k + ".num_batches_tracked"]) == seen["counts"][k] + 1, k
            for stat in (".running_mean", ".running_var"):
                a, b = got[k + stat].double().cpu(), want[k + stat]
                assert torch.isfinite(a).all(), k + stat
                bound = 1e-5 * max(1.0, float(b.abs().max()))
                err = float((a - b).abs().max()) / bound
                worst = max(worst, (err, float((plain[k + stat].double() - b).abs().max()) / bound, k + stat))
        print("BatchNorm buffers, worst error / bound: ours %.3g, plain fp32 torch %.3g (%s)" % worst)
        assert worst[0] <= 1.0, worst
        tt._losses_agree(logs, logs64)
        l2 = np.array([r[2] for r in rows])
        direct = [r for r in rows if r[3].startswith(("pts_bbox_head.decoder", "pts_bbox_head.prediction_heads",
                                                      "pts_bbox_head.class_encoding"))]
        print("gradients: L2-relative max %.3g median %.3g; direct max %.3g (plain fp32 torch %.3g)"
              % (l2.max(), np.median(l2), max(r[0] for r in direct), max(r[1] for r in direct)))
        assert len(rows) > 200 and l2.max() <= 0.15 and np.median(l2) <= 2e-2, (l2.max(), np.median(l2),
                                                                                 sorted((r[2], r[3]) for r in rows)[-5:])
        assert len(direct) > 40 and max(r[0] for r in direct) <= 5e-5, sorted(direct, reverse=True)[:4]
        # the rerun and ITS backward stayed inside the three-part format: no kernel behind the fallback raised the flag
        hit, where = ops.split_overflow(reset=True)
        assert not hit, where
        # a second step on the same inputs: one more update everywhere, again through the fallback
        counts = {k: int(m.num_batches_tracked) for k, m in _batchnorms(det)}
        points, img, metas, gts, labels = tt._device_inputs(2, seed=0)
        feats, coors = det.voxelize(points)
        loss, _ = det.training_step(None, [img], [dict(m) for m in metas], gts, labels, voxels=(feats, coors))
        assert torch.isfinite(loss) and ops.RANGE_STATS["range_fallbacks"] == before + 2
        for k, m in _batchnorms(det):
            assert int(m.num_batches_tracked) == counts[k] + 1, k
            assert torch.isfinite(m.running_mean).all() and torch.isfinite(m.running_var).all(), k


# ------------------------------------------------------------------------------------------------ c. what the step test found
@pytest.mark.parametrize("cout", [16, 1])
@pytest.mark.parametrize("entry", ["linear_rows.linear", "ops.linear_rows_autograd"])
def test_row_linear_weight_gradient_follows_the_forward_into_the_three_part_mode(entry, cout):
    """The weight gradient of a linear layer over >= 2048 rows runs on two-part operands with the ACTIVATION at the fixed scale
    (|x| < 2047).  A forward in the three-part mode -- the rerun of a step that left that range -- must get a three-part
    gradient, whatever the mode is when the backward runs: NaN otherwise (three parameters of the fusion layer in the step
    above).  Against float64, to the bound of the existing row-linear gradient tests (4e-6 of the largest entry)."""
    from dualfusion import linear_rows
    with _Saved() as ops:
        fn = linear_rows.linear if entry == "linear_rows.linear" else ops.linear_rows_autograd
        n, cin = 2051, 64
        gen = torch.Generator().manual_seed(77 + cout)
        x = torch.randn((n, cin), generator=gen)
        at = torch.randperm(n * cin, generator=gen)[:40]
        x.view(-1)[at] = (2047.0 + 2000.0 * torch.rand(40, generator=gen)) * torch.sign(torch.randn(40, generator=gen))
        w, b = torch.randn((cout, cin), generator=gen) * 0.1, torch.randn((cout,), generator=gen)
        g = torch.randn((n, cout), generator=gen) * 1e-3
        wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
        xr = x.double().requires_grad_(True)
        torch.nn.functional.linear(xr, wr, br).backward(g.double())
        for mode_at_backward in ("split3", "split"):
            wd, bd = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
            xd = x.to(DEV).requires_grad_(True)
            with ops.precision("split3"):
                y = fn(xd, wd, bd)
            assert type(y.grad_fn).__name__ in ("_LinearFunctionBackward", "_LinearRowsBackward")
            with ops.precision(mode_at_backward):
                y.backward(g.to(DEV))
            for got, want in ((wd.grad, wr.grad), (bd.grad, br.grad), (xd.grad, xr.grad)):
                assert torch.isfinite(got).all()
                assert float((got.cpu().double() - want).abs().max()) <= 4e-6 * float(want.abs().max())
            assert not ops.split_overflow(reset=True)[0]
