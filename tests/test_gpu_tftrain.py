"""TransFusion-L + 3D-DF as a TRAINING step (BASELINE configs[3]'s per-rank body):
`TransFusionDetector.training_step` -- voxelise -> SparseEncoderFusion (21 rulebook'd convolutions through
`SparseConvFunction`, BatchNorm rows, the ACTR fusion layer's differentiable composition over the native integer work,
MSDA forward / backward kernels) -> SECOND / SECONDFPN on the row kernels -> TransFusionHead -> `loss_device` (matching
costs, heat-map targets, losses and their gradients on csrc/tfloss.hip) -> backward -> clip -> AdamW.

Reference: TF/mmdet3d/models/detectors/transfusion.py:110-199, dense_heads/transfusion_head.py:1218-1283,
ops/spconv/include/spconv/spconv_ops.h:363-456 (indice_conv_backward), TF/configs/transfusion_nusc_voxel_F.py:302-303."""
import copy
import types

import numpy as np
import pytest
import torch

import detgen
import f64_reference as fr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _loaded(det, tag):
    """Deterministic weights for every parameter / buffer (numpy MT19937 by name: the same on every box)."""
    sd = detgen.det_state_dict({k: tuple(v.shape) for k, v in det.state_dict().items()})
    det.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return det


def _device_inputs(B, seed=0):
    points, img, metas, gts, labels = fr.small_inputs(B, seed=seed)
    return ([torch.from_numpy(p).to(DEV) for p in points], torch.from_numpy(img).to(DEV), metas,
            [torch.from_numpy(g) for g in gts], [torch.from_numpy(l) for l in labels])


def _with_precision(mode):
    from dualfusion import ops
    old = ops.CONV_PRECISION
    ops.CONV_PRECISION = mode
    return old


def _step_three_ways(smooth, seed=0, prepare=None):
    """One training step at reduced size (160 x 160 x 40 grid, 2 samples x 6 cameras, 24 proposals) on the GPU, and the same
    detector on the host in float64 and in float32 with every HIP kernel replaced by an independent torch composition
    (tests/f64_reference.py: convolutions on the ORACLE's rulebooks, grid_sample for the deformable sampling, torch BatchNorm /
    conv2d / attention, the plain-torch `loss` with its own Hungarian matching).  smooth: without rectifiers (see
    f64_reference.without_relu).  -> (device log_vars, float64 log_vars, rows (our error, plain fp32 torch's error, L2-relative
    error, name) per parameter -- errors against float64 relative to the gradient's largest entry --, the three detectors).
    prepare(det): changes the freshly loaded host detector in place before it is copied three ways (another checkpoint, hooks)."""
    import contextlib
    from dualfusion.transfusion import parse_losses
    B = 2
    det = _loaded(fr.small_transfusion_detector(), "tftrain")
    if prepare is not None:
        prepare(det)
    d64, d32 = copy.deepcopy(det).double().train(), copy.deepcopy(det).train()
    det = det.to(DEV).train()
    points, img, metas, gts, labels = _device_inputs(B, seed=seed)
    with (fr.without_relu(det, d64, d32) if smooth else contextlib.nullcontext()):
        feats, coors = det.voxelize(points)
        # the projection (camera assignment, pixel // 4: integer-valued downstream, no learnable input) of THIS run is handed
        # to the host runs -- see f64_reference.patched
        layer = det.pts_middle_encoder.fusion_layer
        seen = {}
        plain = layer.project
        layer.project = lambda pts, metas_: seen.setdefault("p", (pts,) + tuple(plain(pts, metas_)))[1:]
        loss, logs = det.training_step(None, [img], [dict(m) for m in metas], gts, labels, voxels=(feats, coors))
        del layer.project
        assert "p" in seen and torch.isfinite(loss)

        def host_run(model, dtype):
            with fr.patched(projection=seen["p"]):
                out = model.forward_train_voxels(feats.cpu().to(dtype), coors.cpu(), B, [img.cpu().to(dtype)],
                                                 [dict(m) for m in metas], [g.to(dtype) for g in gts], labels)
                total, lv = parse_losses(out)
                total.backward()
            return {k: float(v.detach()) for k, v in lv.items()}

        logs64 = host_run(d64, torch.float64)
        host_run(d32, torch.float32)
    want, plain32 = dict(d64.named_parameters()), dict(d32.named_parameters())
    rows = []
    for k, p in det.named_parameters():
        w = want[k].grad
        if w is None:
            # parameters the configuration never reaches, in the reference as here (one image level: no level embedding;
            # nobody reads the LAST dual-query layer's image stream: the image half of its gate)
            assert p.grad is None or float(p.grad.abs().max()) == 0, k
            assert "level_embed" in k or "fusion_layer.a_conv1d" in k, k
            continue
        assert p.grad is not None, k
        scale = float(w.abs().max())
        if scale < 1e-12:                                       # exactly-cancelling sums (a bias in front of a BatchNorm): noise
            assert float(p.grad.abs().max()) < 1e-6, k
            continue
        g = p.grad.double().cpu()
        rows.append((float((g - w).abs().max()) / scale, float((plain32[k].grad.double() - w).abs().max()) / scale,
                     float((g - w).norm() / w.norm()), k))
    return {k: float(v) for k, v in logs.items()}, logs64, rows, (det, d64, d32)


def _losses_agree(logs, logs64):
    for k in ("loss_heatmap", "layer_-1_loss_cls", "layer_-1_loss_bbox", "loss"):
        assert abs(logs[k] - logs64[k]) <= 1e-5 * max(1.0, abs(logs64[k])), (k, logs[k], logs64[k])
    assert abs(logs["matched_ious"] - logs64["matched_ious"]) <= 1e-5


def test_training_step_gradients_vs_float64_without_rectifiers():
    """The precision statement: with the rectifiers taken out (the step is smooth; every convolution, BatchNorm, sampling and
    loss kernel with its backward is still in it) EVERY parameter gradient of the step is of fp32 grade against float64 --
    measured against the same yardstick as plain fp32 torch arithmetic on the host."""
    from dualfusion import ops
    old = _with_precision("split")
    try:
        logs, logs64, rows, _ = _step_three_ways(smooth=True)
        _losses_agree(logs, logs64)
        ours, torch32 = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
        assert len(rows) > 200
        worst = sorted(rows, reverse=True)[:6]
        # BatchNorm's backward over batch statistics cancels (it removes the mean and the normalised-input component of a
        # gradient that is nearly constant over a heat map: tools/debug/bn_backward_precision.py, every 24-bit implementation
        # loses 2-3 digits there), so the bound is the fp32 yardstick, not an absolute 1e-6
        assert ours.max() <= 4.0 * torch32.max() + 2e-5, (ours.max(), torch32.max(), worst)
        assert np.median(ours) <= 4.0 * np.median(torch32) + 2e-6, (np.median(ours), np.median(torch32))
        assert ours.max() <= 2e-3 and np.median(ours) <= 5e-5, (ours.max(), np.median(ours), worst)
    finally:
        ops.CONV_PRECISION = old


def test_training_step_gradients_vs_float64_composition():
    """The real step (rectifiers in).  Two correct 24-bit evaluations differ here by which side of zero a handful of
    pre-activations land on (~20 of 2 M units at the 1e-6 forward agreement measured below), which moves gradients by ~1e-3:
    losses and forward agree with float64 to 1e-5, the parameters with no rectifier between them and the loss (decoder,
    prediction heads) to 5e-5 outright, every other gradient in direction and size (L2-relative error; a wrong kernel, a
    missing term or a transposed operand is an error of order 1)."""
    from dualfusion import ops
    old = _with_precision("split")
    try:
        logs, logs64, rows, (det, d64, d32) = _step_three_ways(smooth=False)
        _losses_agree(logs, logs64)
        l2 = np.array([r[2] for r in rows])
        assert len(rows) > 200 and l2.max() <= 0.15 and np.median(l2) <= 2e-2, (l2.max(), np.median(l2),
                                                                                 sorted((r[2], r[3]) for r in rows)[-5:])
        direct = [r for r in rows if r[3].startswith(("pts_bbox_head.decoder", "pts_bbox_head.prediction_heads",
                                                      "pts_bbox_head.class_encoding"))]
        assert len(direct) > 40 and max(r[0] for r in direct) <= 5e-5, sorted(direct, reverse=True)[:4]
        # BatchNorm running statistics moved the way torch's moved
        for name in ("pts_middle_encoder.conv_input.1", "pts_middle_encoder.encoder_layers.encoder_layer3.0.bn2",
                     "pts_backbone.blocks.1.1", "pts_neck.deblocks.0.1"):
            a = dict(det.named_buffers())[name + ".running_var"].double().cpu()
            b = dict(d64.named_buffers())[name + ".running_var"]
            assert float((a - b).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max())), name
    finally:
        ops.CONV_PRECISION = old


def test_fusion_layer_training_formulation_equals_inference_kernels():
    """`ACTRFusionLayer._forward_autograd` (native integer work + differentiable composition) against `_forward_native`
    (assembly / fused dual-query / write-back kernels, pinned to the reference golden `tf_fusion.npz`): same rows."""
    from dualfusion import ops
    old = _with_precision("split")
    try:
        B = 2
        det = _loaded(fr.small_transfusion_detector(), "tftrain").to(DEV).eval()
        points, img, metas, gts, labels = _device_inputs(B, seed=1)
        enc = det.pts_middle_encoder
        layer = enc.fusion_layer
        feats, coors = det.voxelize(points)
        with torch.no_grad():
            # rows of the stage the layer reads (fusion_pos = 3): any rows on a plausible index set do
            n = 3000
            idx = torch.from_numpy(detgen.clustered_voxels("tffus", B, [5, 20, 20], 4, 400)[:n]).to(DEV)
            idx = idx[torch.argsort(idx[:, 0], stable=True)].contiguous()
            from dualfusion import spconv
            x = spconv.SparseConvTensor(torch.from_numpy(detgen.randn("tffus_rows", (idx.shape[0], 128))).to(DEV), idx,
                                        [5, 20, 20], B)
            pts = enc.coor2pts(x, 0.5)
            want = layer([img], pts, x.features, [dict(m) for m in metas])
        rows = x.features.clone().requires_grad_(True)
        got = layer([img], pts, rows, [dict(m) for m in metas])
        assert got.requires_grad
        err = float((got.detach() - want).abs().max() / want.abs().max())
        assert err <= 1e-4, err
        got.square().sum().backward()
        assert torch.isfinite(rows.grad).all() and float(rows.grad.abs().sum()) > 0
    finally:
        ops.CONV_PRECISION = old


@pytest.mark.parametrize("precision", ["bf16", "split"])
def test_full_size_training_steps_are_finite_and_move_the_weights(precision):
    """BASELINE configs[3]'s per-rank body at full size (0.075 m nuScenes grid, 6 x [256, 112, 200] camera maps per sweep;
    two sweeps here to bound the test's time): two iterations of `bench.py --workload tf_fusion --stage train`'s step --
    losses and the clipped gradient norm finite, every trainable parameter that received a gradient moved, the bucketed
    reducer holds every gradient."""
    from dualfusion import ops, workloads
    old = _with_precision(precision)
    try:
        args = types.SimpleNamespace(batch=2, frames=2, prefetch=False)
        wl = workloads.TransFusionWorkload(args, 0, 1, DEV)
        before = {k: p.detach().clone() for k, p in wl.detector.named_parameters()}
        outs = [wl.step(i, "train") for i in range(2)]
        torch.cuda.synchronize()
        for out in outs:
            wl.check(out, "train")
        assert float(outs[-1]["grad_norm"]) > 0
        moved = sum(int(not torch.equal(before[k], p.detach())) for k, p in wl.detector.named_parameters())
        assert moved >= len(before) - 3, (moved, len(before))        # all but the three parameters the config never reaches
        assert all(p.grad is not None and p.grad.data_ptr() == wl.reducer._view(p._df3d_bucket, p).data_ptr()
                   for p in wl.reducer.params)
        wl.close()
    finally:
        ops.CONV_PRECISION = old
