"""The CenterPoint fusion adapter as a TRAINING stage: `VoxelWithPointProjection.forward_autograd` (native integer work,
the image gate -- factored out of input_proj and computed from voxel rows by default --, `_TallMatmul`,
`channel_first_linear` on df3d_chanfirst_dot, the ACTR module path over the binned MSDA backward, the additive write-back
in camera order) against a float64 evaluation of the reference's own order of operations: `oracle_models.
centerpoint_fusion_torch`, pinned to the reference module's output by tests/golden/fusion_cp.npz and checked on its own in
tests/test_cptrain_host.py.  The yardstick of every bound is the same port in plain float32 on the host.

Reference: CP/det3d/models/fusion/voxel_with_point_projection.py:131-385, point_to_image_projection.py:63-231,
model_utils/attention.py:31-61, model_utils/actr.py:131-187."""
import contextlib

import numpy as np
import pytest
import torch

import f64_reference as fr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

# the three formulations of the product's training path (fusion.py, forward_autograd)
FORMULATIONS = {"factored_sparse": {},                                   # default: att * (W img) + b, gate from voxel rows
                "factored_canvas": {"DF3D_TRAIN_GATE_SPARSE": "0"},      # factored gate over dense canvases
                "gated": {"DF3D_TRAIN_GATED": "1"}}                      # the reference's order: input_proj(img * att)
UNREACHED = ["ifat.reduced_dim.1.bias", "ifat.reduced_dim.1.weight",
             "pfat.transformer.encoder.layers.1.fusion_layer.a_conv1d.bias",
             "pfat.transformer.encoder.layers.1.fusion_layer.a_conv1d.weight", "pfat.transformer.level_embed"]


@pytest.fixture(autouse=True)
def _split_precision():
    from dualfusion import ops
    old, ops.CONV_PRECISION = ops.CONV_PRECISION, "split"
    yield
    ops.CONV_PRECISION = old


def _formulation(monkeypatch, name):
    for k in ("DF3D_TRAIN_GATE_SPARSE", "DF3D_TRAIN_GATED"):
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMULATIONS[name].items():
        monkeypatch.setenv(k, v)


def _device_step(case, work, smooth, blind=False):
    """The module of test_centerpoint_fusion_adapter_training_path (same fixture, construction and weights, dropout 0) ->
    forward and backward of sum(out.features * w) on the GPU.  Before anything floating-point is looked at, its `_project`
    has to give the port's pixel grid and mask (`work`) for every scale and camera, row for row.
    -> (out [n, 128], {parameter name | 'leaf<i>': gradient}) as float64 host tensors."""
    from dualfusion import fusion as fz, spconv, synth
    from make_golden import ACTR_CFG, FUS, FUS_IFAT, FUS_LT
    mod = fz.VoxelWithPointProjection(fuse_mode='pfat', interpolate=False, voxel_size=FUS["voxel_size"],
                                      pc_range=FUS["pc_range"], image_list=synth.NUSC_CAMS, image_scale=FUS["image_scale"],
                                      depth_thres=fr.cp_depth_thres(blind), pfat_cfg=dict(ACTR_CFG), lt_cfg=dict(FUS_LT),
                                      ifat_cfg=dict(FUS_IFAT), model_name='ACTR')
    assert {k: tuple(v.shape) for k, v in mod.state_dict().items()} == case["shapes"]
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in case["sd"].items()})
    mod = mod.to(DEV).train()
    for m in mod.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    B = FUS["batch"]
    H, W = FUS["img_hw"]
    batch_dict = {'image_shape': {}, 'img_feat': {'layer1_ori_feat2d': {}}, 'calib': {}}
    for n in synth.NUSC_CAMS:
        key = n.lower()
        batch_dict['image_shape'][key] = torch.tensor([[H, W, 3]] * B)
        batch_dict['img_feat']['layer1_ori_feat2d'][key] = torch.from_numpy(case["img"][n]).to(DEV)
        T, K = case["cams"][n]
        batch_dict['calib']['lidar2cam_' + key.lstrip('cam_')] = torch.from_numpy(np.stack([T] * B)).to(DEV)
        batch_dict['calib']['cam_intrinsic_' + key.lstrip('cam_')] = torch.from_numpy(np.stack([K] * B)).to(DEV)
    shapes = [[21, 128, 128], [11, 64, 64], [5, 32, 32]]
    leaves = [torch.from_numpy(f).to(DEV).requires_grad_(True) for f in case["feats"]]
    xs = [spconv.SparseConvTensor(f, torch.from_numpy(i).to(DEV), shp, B) for f, i, shp in zip(leaves, case["sets"], shapes)]
    # ---- integer work first: a voxel on a truncation boundary shows up HERE, not as a gradient mismatch
    inp = mod._gather_inputs(batch_dict, 'layer1_ori', DEV)
    for s, d_factor in enumerate([2, 4, 8]):
        grid, mask, _ = mod._project(xs[s], d_factor, inp)
        grid, mask = grid.cpu().long(), mask.cpu().bool()
        for ci, cam in enumerate(synth.NUSC_CAMS):
            g_ref, m_ref = work[(s, ci)]
            off = torch.nonzero(mask[ci] != m_ref).flatten()
            assert off.numel() == 0, "scale %d, %s: mask differs at rows %s" % (s, cam, off[:8].tolist())
            # (the kernel writes pixel (0, 0) for a row it masks out, the reference whatever the truncation gave: nobody
            # reads either)
            off = torch.nonzero((grid[ci] != g_ref).any(1) & m_ref).flatten()
            assert off.numel() == 0, "scale %d, %s: pixel differs at rows %s" % (s, cam, off[:8].tolist())
            if blind and cam == fr.CP_BLIND_CAMERA:
                assert int(mask[ci].sum()) == 0
            else:
                assert int(mask[ci].sum()) > 0
    with (fr.without_relu(mod) if smooth else contextlib.nullcontext()):
        out = mod(batch_dict, {}, encoded_voxel_list=xs, layer_name='layer1_ori', fuse_mode='pfat', d_factor_list=[2, 4, 8])
        assert out.features.requires_grad
        (out.features * torch.from_numpy(case["w"]).to(DEV)).sum().backward()
    got = {k: p.grad for k, p in mod.named_parameters()}
    got.update({"leaf%d" % i: f.grad for i, f in enumerate(leaves)})
    return out.features.detach().double().cpu(), {k: None if g is None else g.double().cpu() for k, g in got.items()}


def _compare(case, monkeypatch, formulation, smooth, blind=False):
    """-> rows (our entry-wise error, plain fp32's, our L2-relative error, plain fp32's, name) per tensor with a gradient,
    errors against float64, entry-wise ones relative to that gradient's largest entry.  Asserts the integer work, the
    forward (1e-5 of the output scale) and that what float64 does not reach has no gradient here either."""
    ref64 = fr.cp_fusion_gradients(case, torch.float64, relu=not smooth, blind=blind)
    ref32 = fr.cp_fusion_gradients(case, torch.float32, relu=not smooth, blind=blind)
    _formulation(monkeypatch, formulation)
    out, got = _device_step(case, ref64["work"], smooth, blind)
    scale = float(ref64["out"].abs().max())
    err, err32 = float((out - ref64["out"]).abs().max()), float((ref32["out"].double() - ref64["out"]).abs().max())
    print("%s%s%s: forward max abs %.3g (plain fp32 %.3g) at scale %.4g" % (
        formulation, ", no rectifiers" if smooth else "", ", blind camera" if blind else "", err, err32, scale))
    assert err <= 1e-5 * scale, (err, scale)
    assert ref64["unreached"] == sorted(UNREACHED + ["leaf1"]) and set(got) == set(ref64["grads"]) | set(ref64["unreached"])
    for k in ref64["unreached"]:
        assert got[k] is None or float(got[k].abs().max()) == 0, k
    rows = []
    for k, w in ref64["grads"].items():
        assert got[k] is not None and got[k].shape == w.shape and torch.isfinite(got[k]).all(), k
        top, d, d32 = float(w.abs().max()), got[k] - w, ref32["grads"][k].double() - w
        rows.append((float(d.abs().max()) / top, float(d32.abs().max()) / top, float(d.norm() / w.norm()),
                     float(d32.norm() / w.norm()), k))
    assert len(rows) >= 68, len(rows)
    e = np.array([r[:4] for r in rows])
    print("  entry-wise: ours max %.3g median %.3g | plain fp32 max %.3g median %.3g" % (
        e[:, 0].max(), np.median(e[:, 0]), e[:, 1].max(), np.median(e[:, 1])))
    print("  L2-relative: ours max %.3g median %.3g | plain fp32 max %.3g median %.3g" % (
        e[:, 2].max(), np.median(e[:, 2]), e[:, 3].max(), np.median(e[:, 3])))
    for r in sorted(rows, reverse=True)[:4]:
        print("  worst: %.3g (fp32 %.3g, L2 %.3g / %.3g) %s" % r)
    return rows


def _assert_fp32_grade(rows):
    """The bounds of test_gpu_tftrain.test_training_step_gradients_vs_float64_without_rectifiers."""
    ours, torch32 = np.array([r[0] for r in rows]), np.array([r[1] for r in rows])
    worst = sorted(rows, reverse=True)[:6]
    assert ours.max() <= 4.0 * torch32.max() + 2e-5, (ours.max(), torch32.max(), worst)
    assert np.median(ours) <= 4.0 * np.median(torch32) + 2e-6, (np.median(ours), np.median(torch32), worst)


@pytest.mark.parametrize("formulation", sorted(FORMULATIONS))
def test_adapter_gradients_vs_float64_without_rectifiers(golden, monkeypatch, formulation):
    """With the rectifiers out the adapter is smooth, every kernel and its backward is still in it, and each of the 68
    gradients (66 parameters, the voxel features of scales 0 and 2) is compared entry by entry with float64, relative to
    its largest entry, against what plain fp32 torch arithmetic on the host makes of the same function.  Every formulation
    has to pass on its own: they share the projection, winner and slot glue, the scatters, ACTR and the write-back, so a
    comparison between them says nothing about those.
    Measured on the MI355X, entry-wise max / median (the plain-fp32 yardstick of that run: 7.5e-4 / 4.7e-7, its largest
    on ifat.reduced_dim3.bias, a cancelling sum over all pixels, then 4.9e-5 on ifat.spatial_basic.bias, the rest <= 1.5e-5):
      factored_sparse 1.5e-4 / 6.1e-7,  factored_canvas 1.1e-3 / 7.0e-7,  gated 9.3e-4 / 6.8e-7
    -- each one's largest on ifat.reduced_dim3.bias too, next ifat.spatial_basic.bias (1.5e-5 / 1.0e-4 / 8.8e-5), everything
    else <= 1.9e-5; the L2-relative figures have the same maxima and medians 6.0e-7 / 6.3e-7 / 6.0e-7 (fp32: 5.0e-7).
    Forward: 4.4e-6 .. 4.8e-6 absolute at scale 15.07 (plain fp32: 5.9e-6)."""
    _assert_fp32_grade(_compare(fr.cp_fusion_case(golden("fusion_cp.npz")), monkeypatch, formulation, smooth=True))


def test_adapter_gradients_vs_float64_with_a_camera_that_sees_nothing(golden, monkeypatch):
    """The same comparison (default formulation, no rectifiers) with one camera's depth threshold beyond every voxel, in the
    product and in the port alike: its mask is empty, its slot count zero, its range in the camera-ordered write-back loop
    empty -- and it sits in the middle of the camera order.
    Measured on the MI355X: entry-wise max 9.5e-6, median 6.1e-7 (plain fp32: 1.1e-5 / 5.1e-7), L2-relative max 9.5e-6
    (1.3e-5); forward 4.3e-6 at scale 13.33."""
    _assert_fp32_grade(_compare(fr.cp_fusion_case(golden("fusion_cp.npz")), monkeypatch, "factored_sparse", smooth=True,
                                blind=True))


def test_adapter_gradients_vs_float64_composition(golden, monkeypatch):
    """The real path (rectifiers in, default formulation).  A pre-activation within rounding of zero lands on either side
    of it in two correct 24-bit evaluations, and that one unit then moves the gradients upstream of it by ~1e-3 (the plain
    fp32 port against float64: 5.4e-3 entry-wise, 1.8e-3 L2-relative at the worst, both on layers.1.self_attn.
    sampling_offsets.*).  So per-tensor L2-relative errors, bounded by ten times the largest of the fp32 yardstick's from
    the same run: which units flip is chance, and the per-tensor sizes spread over an order of magnitude; a wrong kernel,
    a dropped term or a transposed operand is an error of order one.
    Measured on the MI355X: L2-relative max 1.76e-3, median 4.9e-5 -- the fp32 yardstick's figures to three digits (the
    same units flip in both 24-bit evaluations); entry-wise max 5.4e-3 (5.4e-3); forward 4.8e-6 at scale 14.57."""
    rows = _compare(fr.cp_fusion_case(golden("fusion_cp.npz")), monkeypatch, "factored_sparse", smooth=False)
    ours, torch32 = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])
    assert ours.max() <= 10.0 * torch32.max(), (ours.max(), torch32.max(), sorted((r[2], r[3], r[4]) for r in rows)[-5:])
