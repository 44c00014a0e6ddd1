"""TransFusion and Voxel-RCNN flavours of the hot path (BASELINE configs 3-5 shapes, reduced grids):
sparse encoders vs the oracle compositions; fusion-layer glue vs loop restatements of the reference code."""
import os

import numpy as np
import pytest

import detgen
import oracle_models as om
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TF_CH = ((16, 16, 32), (32, 32, 64), (64, 64, 128), (128, 128))
TF_PAD = ((0, 0, 1), (0, 0, 1), (0, 0, [0, 1, 1]), (0, 0))


def _voxels(seed, rng, dev, feat_c=5, batch=1):
    from dualfusion import ops, synth
    feats, coors, of, oc_ = [], [], [], []
    for b in range(batch):
        pts = synth.nusc_sweep(seed=seed + b)[:, :feat_c].copy()
        v, c, n, mean = ops.hard_voxelize(torch.from_numpy(pts).to(dev), synth.NUSC_VOXEL, rng, 10, 120000)
        ov, oc, on = orc.hard_voxelize(pts, synth.NUSC_VOXEL, rng, 10, 120000)
        feats.append(mean)
        coors.append(torch.cat([torch.full((c.shape[0], 1), b, dtype=torch.int32, device=dev), c], 1))
        of.append(orc.mean_vfe(ov, on))
        oc_.append(np.concatenate([np.full((len(oc), 1), b, np.int32), oc], 1))
    return torch.cat(feats), torch.cat(coors), np.concatenate(of), np.concatenate(oc_)


def _load_det(model, dev):
    sd = detgen.det_state_dict({k: tuple(v.shape) for k, v in model.state_dict().items()})
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.to(dev).eval(), sd


def test_transfusion_sparse_encoder_vs_oracle():
    from dualfusion.backbones import SparseEncoder
    dev = torch.device("cuda:0")
    shape = [41, 256, 256]
    m = SparseEncoder(in_channels=5, sparse_shape=shape, output_channels=128, encoder_channels=TF_CH,
                      encoder_paddings=TF_PAD, block_type='basicblock')
    # checkpoint layout of SURVEY.md Appendix B
    keys = set(m.state_dict())
    assert {"conv_input.0.weight", "encoder_layers.encoder_layer1.0.conv1.weight", "encoder_layers.encoder_layer1.0.bn2.weight",
            "encoder_layers.encoder_layer3.2.0.weight", "encoder_layers.encoder_layer4.1.conv2.weight",
            "conv_out.0.weight"} <= keys
    assert not any(k.endswith("conv1.bias") for k in keys)
    m, sd = _load_det(m, dev)
    f, c, of, oc = _voxels(60, [-9.6, -9.6, -5.0, 9.6, 9.6, 3.0], dev, batch=2)
    with torch.no_grad():
        assert m._runner() is not None, "the native executor must serve this module tree"
        y = m(f, c, 2)
    ref, _ = om.transfusion_encoder(sd, of, oc, 2, shape, TF_CH, TF_PAD)
    assert tuple(y.shape) == ref.shape == (2, 256, 32, 32)
    np.testing.assert_allclose(y.cpu().numpy(), ref, rtol=1e-3, atol=1e-3 * max(1.0, np.abs(ref).max()))


def test_transfusion_encoder_accepts_bf16_features():
    """BASELINE configs[2] feeds bf16 activations: the encoder takes them (computing in fp32 / split precision) and
    stays within bf16 input rounding (2^-8 relative per feature) of the fp32-input result."""
    from dualfusion.backbones import SparseEncoder
    dev = torch.device("cuda:0")
    m = SparseEncoder(in_channels=5, sparse_shape=[41, 256, 256], output_channels=128, encoder_channels=TF_CH,
                      encoder_paddings=TF_PAD, block_type='basicblock')
    m, _ = _load_det(m, dev)
    f, c, _, _ = _voxels(61, [-9.6, -9.6, -5.0, 9.6, 9.6, 3.0], dev, batch=2)
    with torch.no_grad():
        y32 = m(f, c, 2)
        y16 = m(f.to(torch.bfloat16), c, 2)
    assert y16.dtype == torch.float32 and tuple(y16.shape) == tuple(y32.shape)
    err = float((y16 - y32).abs().max() / y32.abs().max())
    assert err < 3e-2, err


def test_bf16_conv_mode_encoder_and_centerpoint_backbone():
    """DF3D_CONV_PRECISION=bf16 (BASELINE configs[2]: bf16, fp32 accumulate): every C >= 32 sparse conv runs on the bf16
    kernel (bf16 rows handed from layer to layer, fp32 epilogue); results stay within accumulated bf16 rounding of the
    split-precision path, index sets are identical."""
    from dualfusion import ops
    from dualfusion.backbones import SparseEncoder
    from dualfusion.pipeline import CenterPointHotPath
    from dualfusion import synth
    dev = torch.device("cuda:0")
    m = SparseEncoder(in_channels=5, sparse_shape=[41, 256, 256], output_channels=128, encoder_channels=TF_CH,
                      encoder_paddings=TF_PAD, block_type='basicblock')
    m, _ = _load_det(m, dev)
    f, c, _, _ = _voxels(61, [-9.6, -9.6, -5.0, 9.6, 9.6, 3.0], dev, batch=2)
    hp = CenterPointHotPath().eval().to(dev)
    pts = [torch.from_numpy(synth.nusc_sweep(seed=4)).to(dev)]
    with torch.no_grad():
        y32 = m(f, c, 2)
        d32, multi32 = hp(pts)
        old = ops.CONV_PRECISION
        ops.CONV_PRECISION = "bf16"
        try:
            y16 = m(f, c, 2)
            d16, multi16 = hp(pts)
        finally:
            ops.CONV_PRECISION = old
    assert y16.dtype == torch.float32 and tuple(y16.shape) == tuple(y32.shape)
    assert float((y16 - y32).abs().max() / y32.abs().max()) < 5e-2
    assert float((y16 - y32).abs().mean() / y32.abs().mean()) < 1e-2
    for k in ("conv1", "conv2", "conv3", "conv4"):
        assert torch.equal(multi16[k].indices, multi32[k].indices)
    assert getattr(multi16["conv4"], "_bf16", None) is not None          # the bf16 kernel served the 128-channel stage
    assert float((d16 - d32).abs().max() / d32.abs().max()) < 5e-2
    assert float((d16 - d32).abs().mean() / d32.abs().mean()) < 1e-2


def _tf_metas(B, cams, ori_hw, in_hw):
    sf = [in_hw[1] / ori_hw[1], in_hw[0] / ori_hw[0]]
    from dualfusion import synth
    return [dict(lidar2cam=np.stack([cams[n][0] for n in synth.NUSC_CAMS]),
                 cam_intrinsic=np.stack([cams[n][1] for n in synth.NUSC_CAMS]),
                 ori_shape=(ori_hw[0], ori_hw[1], 3), img_shape=(in_hw[0], in_hw[1], 3),
                 input_shape=(in_hw[0], in_hw[1]), scale_factor=sf, flip=False) for _ in range(B)]


def test_transfusion_fusion_layer_glue_and_encoder_fusion():
    """ACTRFusionLayer.project/assemble vs a loop restatement of point_fusion.py:342-382,509-549,612-617
    (projection through lidar2cam + intrinsics instead of the nuScenes DB)."""
    from dualfusion import synth
    from dualfusion.backbones import SparseEncoderFusion
    from dualfusion.fusion_tf import ACTRFusionLayer
    from make_golden import ACTR_CFG
    dev = torch.device("cuda:0")
    B, ori_hw, in_hw, fh, fw = 2, (225, 400), (112, 200), 28, 50
    cams = synth.nusc_cameras(image_hw=ori_hw, focal=316.0)
    metas = _tf_metas(B, cams, ori_hw, in_hw)
    layer = ACTRFusionLayer(pfat_cfg=dict(ACTR_CFG)).to(dev).eval()
    gen = np.random.RandomState(0)
    n = 700
    pts = np.concatenate([np.repeat(np.arange(B), n // B)[:, None].astype(np.float32),
                          gen.uniform(-25, 25, (n, 2)).astype(np.float32), gen.uniform(-3, 1, (n, 1)).astype(np.float32)], 1)
    feats = gen.standard_normal((n, 128)).astype(np.float32)
    img = gen.standard_normal((B * 6, 256, fh, fw)).astype(np.float32)
    cam_id, norm, pix = layer.project(torch.from_numpy(pts).to(dev), metas)
    # ---- loop restatement
    exp_cam = np.zeros(n, np.int64)
    exp_pix = np.zeros((n, 2), np.float32)
    for i in range(n):
        b = int(pts[i, 0])
        for ci, name in enumerate(synth.NUSC_CAMS):
            T, K = cams[name]
            pc = T[:3, :3].astype(np.float64) @ pts[i, 1:4].astype(np.float64) + T[:3, 3]
            if pc[2] <= 1.0:
                continue
            u = (K[0, 0] * pc[0] + K[0, 2] * pc[2]) / pc[2]
            v = (K[1, 1] * pc[1] + K[1, 2] * pc[2]) / pc[2]
            if 1 < u < ori_hw[1] - 1 and 1 < v < ori_hw[0] - 1:
                exp_cam[i] = ci
                exp_pix[i] = [u * metas[b]['scale_factor'][0], v * metas[b]['scale_factor'][1]]
    assert (cam_id.cpu().numpy() == exp_cam).mean() > 0.999          # fp32 vs fp64 borderline pixels
    same = cam_id.cpu().numpy() == exp_cam
    np.testing.assert_allclose(pix.cpu().numpy()[same], exp_pix[same], rtol=1e-3, atol=2e-2)
    v_feat, v_i_feat, grid, qpts, seg, slot = layer.assemble([torch.from_numpy(img).to(dev)], torch.from_numpy(pts).to(dev),
                                                             torch.from_numpy(feats).to(dev), cam_id, norm, pix, B)
    cid, px = cam_id.cpu().numpy(), pix.cpu().numpy()
    for b in range(B):
        for c in range(6):
            rows = [i for i in range(n) if int(pts[i, 0]) == b and cid[i] == c]
            got = v_feat[b * 6 + c].cpu().numpy()
            np.testing.assert_array_equal(got[:len(rows)], feats[rows])
            assert not got[len(rows):].any()
            if rows:
                ic = px[rows].astype(np.int64) // 4
                np.testing.assert_array_equal(v_i_feat[b * 6 + c, :len(rows)].cpu().numpy(),
                                              img[b * 6 + c][:, ic[:, 1], ic[:, 0]].T)
    # ---- the encoder with the fusion layer mounted (configs[2] module tree), reduced grid
    enc = SparseEncoderFusion(in_channels=5, sparse_shape=[41, 256, 256], output_channels=128, encoder_channels=TF_CH,
                              encoder_paddings=TF_PAD, block_type='basicblock', fusion_pos=[3],
                              voxel_size=[0.075, 0.075, 0.2], point_cloud_range=[-9.6, -9.6, -5.0, 9.6, 9.6, 3.0],
                              fusion_layer=dict(type='ACTR', pfat_cfg=dict(ACTR_CFG)))
    assert "fusion_layer.actr.transformer.encoder.layers.1.linear3.weight" in enc.state_dict()
    enc = enc.to(dev).eval()
    f, c, _, _ = _voxels(70, [-9.6, -9.6, -5.0, 9.6, 9.6, 3.0], dev, batch=B)
    with torch.no_grad():
        assert enc._runner([4]) is not None          # fusion after the LAST encoder layer: one segment, hook at its end
        y = enc(f, c, B, img_feats=[torch.from_numpy(img).to(dev)], img_metas=metas)
        # the executor segments launch the same kernels as the per-module path
        import os
        os.environ["DF3D_EXECUTOR"] = "0"
        try:
            y_slow = enc(f, c, B, img_feats=[torch.from_numpy(img).to(dev)], img_metas=metas)
        finally:
            os.environ["DF3D_EXECUTOR"] = "1"
    assert tuple(y.shape) == (B, 256, 32, 32) and bool(torch.isfinite(y).all())
    torch.testing.assert_close(y, y_slow, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("tag,aug", [("plain", False), ("aug", True)])
def test_transfusion_fusion_layer_vs_reference_golden(golden, tag, aug):
    """The whole fusion layer -- projection, last-camera-wins assignment, per-camera query sets, image features at
    pixel // 4, ACTR, additive write-back -- against the output of the reference's own point_fusion.ACTR.forward on the
    same weights and inputs (golden tf_fusion.npz from tests/golden/make_golden.py gen_tf_fusion; nuScenes records
    composed into the per-camera lidar2cam the layer takes).  `aug`: with a 3-D augmentation flow to undo."""
    import detgen
    from dualfusion.fusion_tf import ACTRFusionLayer
    from make_golden import ACTR_CFG, tff_inputs, tff_metas
    dev = torch.device("cuda:0")
    g = golden("tf_fusion.npz")
    layer = ACTRFusionLayer(pfat_cfg=dict(ACTR_CFG))
    shapes = {k: tuple(v.shape) for k, v in layer.state_dict().items()}
    assert sorted(shapes) == list(g["param_names"])                    # same parameter names as the reference module
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in detgen.det_state_dict(shapes).items()})
    layer = layer.to(dev).eval()
    pts, feats, img = tff_inputs()
    metas, _, _, _ = tff_metas(aug)
    ours = []
    for b, m in enumerate(metas):
        mm = {k: v for k, v in m.items() if k not in ("sample_idx", "filename")}
        mm["lidar2cam"], mm["cam_intrinsic"] = g[tag + "_lidar2cam"][b], g[tag + "_intrinsic"][b]
        ours.append(mm)
    with torch.no_grad():
        fused = layer([torch.from_numpy(img).to(dev)], [torch.from_numpy(p).to(dev) for p in pts],
                      torch.from_numpy(feats).to(dev), ours)
        # ... and through the module composition instead of the fold-through image path
        import os
        os.environ["DF3D_IMGPROJ"] = "0"
        try:
            fused_mod = layer([torch.from_numpy(img).to(dev)], [torch.from_numpy(p).to(dev) for p in pts],
                              torch.from_numpy(feats).to(dev), ours)
        finally:
            os.environ["DF3D_IMGPROJ"] = "1"
    want = g[tag + "_fused"]
    scale = np.abs(want).max()
    for name, got in (("fold-through", fused), ("module composition", fused_mod)):
        err = np.abs(got.cpu().numpy() - want).max(1) / scale
        assert err.max() <= 1e-3, (name, err.max(), int((err > 1e-3).sum()))


@pytest.mark.parametrize("tag,with_aug", [("plain", False), ("aug", True)])
def test_voxel_rcnn_fusion_glue_vs_reference_golden(golden, tag, with_aug):
    """The Voxel-RCNN camera glue -- voxel corner -> image pixel through the KITTI calibration, bilinear upsample +
    truncated-pixel gather, (a) MVX sum at stride 1, (b) ACTRv2 (d_model 64, 4 encoder layers, 3-D local self-attention
    per layer) dual-query fusion at stride 8 -- against the outputs of the reference's own
    VoxelBackBone8xFusion.point_fusion (golden vr_fusion.npz, tests/golden/make_golden.py gen_vr_fusion), without and
    with augmentation records (noise_scale, noise_rot, flip_x) to undo."""
    import detgen
    from dualfusion import spconv as sp
    from dualfusion.backbones import VoxelBackBone8xFusion
    from make_golden import VRF, vrf_inputs
    dev = torch.device("cuda:0")
    g = golden("vr_fusion.npz")
    cfg = dict(NAME='VoxelBackBone8xFusion', USE_IMG=True, FUSION_POS=[1, 4], FUSION_METHOD='MVX+ACTRv2', FEATURE_LEVELS=[0],
               LT_CFG=dict(VRF["lt"]), ACTR_CFG=dict(VRF["actr"]), HYBRID_CFG=dict(VRF["hybrid"]))
    m = VoxelBackBone8xFusion(cfg, 4, [1408, 1600, 40])
    shapes = {k: tuple(v.shape) for k, v in m.actr.state_dict().items()}
    assert sorted(shapes) == list(g["param_names"])                    # same parameter names as the reference's ACTRv2
    m.actr.load_state_dict({k: torch.from_numpy(v) for k, v in detgen.det_state_dict(shapes).items()})
    m = m.to(dev).eval()
    ind1, f1, ind4, f4, mvx, img, aug = vrf_inputs()
    B, (H, W) = VRF["batch"], VRF["hw"]
    bd = dict(batch_size=B, lidar2img=torch.from_numpy(g["lidar2img"][:, :3].astype(np.float32)).to(dev), image_hw=(H, W),
              img_dict={"mvx_layer1_feat2d": torch.from_numpy(mvx).to(dev), "layer1_feat2d": torch.from_numpy(img).to(dev)})
    if with_aug:
        bd.update(noise_scale=torch.from_numpy(aug["noise_scale"]).to(dev), noise_rot=torch.from_numpy(aug["noise_rot"]).to(dev),
                  flip_x=torch.from_numpy(aug["flip_x"]).to(dev))
    x1 = sp.SparseConvTensor(torch.from_numpy(f1).to(dev), torch.from_numpy(ind1).to(dev), [41, 1600, 1408], B)
    x4 = sp.SparseConvTensor(torch.from_numpy(f4).to(dev), torch.from_numpy(ind4).to(dev), [5, 200, 176], B)
    stages, hooks = {}, []
    enc = m.actr.transformer.encoder
    for nm, mod in (("lt0", enc.lidar_attns[0]), ("layer0", enc.layers[0]), ("lt1", enc.lidar_attns[1])):
        hooks.append(mod.register_forward_hook(
            lambda m_, i_, o_, nm=nm: stages.__setitem__(nm, (o_[0] if isinstance(o_, tuple) else o_).detach().cpu().numpy().copy())))
    def grab(m_, args, kwargs):
        stages["in_ref"] = args[2].detach().cpu().numpy().copy()
        stages["in_qpos"] = kwargs["q_pos"].detach().cpu().numpy().copy()
        stages["in_qi"] = kwargs["q_i_feat"].detach().cpu().numpy().copy()
    hooks.append(enc.layers[0].register_forward_pre_hook(grab, with_kwargs=True))
    with torch.no_grad():
        y1 = m._fuse1(x1, bd).features.cpu().numpy()
        y4 = m._fuse4(None, None, x4, bd).features.cpu().numpy()
    for h_ in hooks:
        h_.remove()
    for nm in ("in_ref", "in_qpos", "in_qi", "lt0", "layer0", "lt1"):                 # intermediate LiDAR queries of the reference: localises a deviation
        want = g[tag + "_stage_" + nm]
        got = stages[nm].reshape(want.shape)
        e = np.abs(got - want).max() / np.abs(want).max()
        assert e <= 1e-3, (nm, e)
    want1, want4 = g[tag + "_mvx"], g[tag + "_actr"]
    # MVX: the gathered pixel is a truncation of a projected coordinate -- a voxel within 1e-3 px of a pixel boundary may
    # land on either side in fp32 vs the reference's float64 numpy projection; everything else must agree to 1e-4
    bad = np.abs(y1 - want1).max(1) > 1e-4 * np.abs(want1).max()
    assert bad.sum() <= 2, int(bad.sum())
    err = np.abs(y4 - want4).max(1) / np.abs(want4).max()
    assert (err > 1e-3).sum() <= 1 and np.median(err) < 1e-4, (err.max(), int((err > 1e-3).sum()))
    # round 6: with the reference's own batch_dict key -- `calib` objects, projected on the host the way the devkit does
    # (`KittiCalibration`) -- every voxel lands in the reference's pixel: no row may differ
    from dualfusion.backbones import KittiCalibration
    from make_golden import vrf_calib
    bdc = {k: v for k, v in bd.items() if k != "lidar2img"}
    bdc["calib"] = [KittiCalibration(*vrf_calib(b)) for b in range(B)]
    with torch.no_grad():
        y1c = m._fuse1(x1, bdc).features.cpu().numpy()
        y4c = m._fuse4(None, None, x4, bdc).features.cpu().numpy()
    assert np.abs(y1c - want1).max() <= 1e-5 * np.abs(want1).max()
    assert (np.abs(y4c - want4).max(1) / np.abs(want4).max()).max() <= 1e-3


VR_CFG = dict(NAME='VoxelBackBone8xFusion', USE_IMG=True, FUSION_POS=[1, 4], FUSION_METHOD='MVX+ACTRv2',
              FEATURE_LEVELS=[0], LT_CFG=dict(npoint=256, radius=2.0, nsample=16, num_layers=2),
              ACTR_CFG=dict(fusion_method='sum', feature_modal='hybrid', num_bins=80, num_channels=[256],
                            query_num_feat=64, num_enc_layers=4, max_num_ne_voxel=20000, pos_encode_method='depth'),
              HYBRID_CFG=dict(attn_layer='BiGateSum1D_2', q_method='sum', q_rep_place=['weight']))


def _kitti_voxels(dev, batch):
    from dualfusion import ops, synth
    rng = [0.0, -12.8, -3.0, 25.6, 12.8, 1.0]         # reduced KITTI range: grid 512 x 512 x 40
    feats, coors, of, oc_ = [], [], [], []
    for b in range(batch):
        pts = synth.kitti_sweep(seed=80 + b)
        v, c, n, mean = ops.hard_voxelize(torch.from_numpy(pts).to(dev), synth.KITTI_VOXEL, rng, 5, 40000)
        ov, oc, on = orc.hard_voxelize(pts, synth.KITTI_VOXEL, rng, 5, 40000)
        assert np.array_equal(c.cpu().numpy(), oc)
        feats.append(mean)
        coors.append(torch.cat([torch.full((c.shape[0], 1), b, dtype=torch.int32, device=dev), c], 1))
        of.append(orc.mean_vfe(ov, on, clamp_min=1.0))
        oc_.append(np.concatenate([np.full((len(oc), 1), b, np.int32), oc], 1))
    return torch.cat(feats), torch.cat(coors), np.concatenate(of), np.concatenate(oc_)


def test_voxel_rcnn_backbone_vs_oracle_and_fusion_runs():
    from dualfusion.backbones import VoxelBackBone8x, VoxelBackBone8xFusion
    dev = torch.device("cuda:0")
    B = 2
    f, c, of, oc = _kitti_voxels(dev, B)
    m = VoxelBackBone8x(dict(NAME='VoxelBackBone8x'), 4, [512, 512, 40])
    assert {"conv_input.0.weight", "conv1.0.0.weight", "conv4.2.1.running_var", "conv_out.0.weight"} <= set(m.state_dict())
    m, sd = _load_det(m, dev)
    with torch.no_grad():
        assert m._runner() is not None and len(m._runner().segments) == 1
        bd = m(dict(voxel_features=f, voxel_coords=c, batch_size=B))
    o_out, o_ms = om.voxel_backbone8x(sd, of, oc, B, [41, 512, 512])
    got = bd["encoded_spconv_tensor"]
    assert got.spatial_shape == o_out.shape == [2, 64, 64] and bd["multi_scale_3d_strides"]["x_conv4"] == 8
    gi, gf = om.sort_rows(got.indices.cpu().numpy(), got.features.cpu().numpy())
    oi, of_ = om.sort_rows(o_out.indices, o_out.features)
    assert np.array_equal(gi, oi)
    np.testing.assert_allclose(gf, of_, rtol=1e-3, atol=1e-3 * max(1.0, np.abs(of_).max()))
    # fusion variant (BASELINE config 5 module tree: MVX at stride 1 + ACTRv2 at stride 8, one camera)
    mf = VoxelBackBone8xFusion(dict(VR_CFG), 4, [512, 512, 40]).to(dev).eval()
    assert "actr.transformer.encoder.lidar_attns.3.chunk.layers.1.linear2.weight" in mf.state_dict()
    H, W = 96, 320
    K = np.array([[180., 0, W / 2, 0], [0, 180., H / 2, 0], [0, 0, 1, 0]], np.float32)
    Tr = np.array([[0, -1, 0, 0], [0, 0, -1, -0.08], [1, 0, 0, -0.27], [0, 0, 0, 1]], np.float32)   # velo -> cam
    l2i = torch.from_numpy(np.stack([K @ Tr] * B)).to(dev)
    gen = torch.Generator().manual_seed(0)
    bd = dict(voxel_features=f, voxel_coords=c, batch_size=B, lidar2img=l2i, image_hw=(H, W),
              img_dict={"mvx_layer1_feat2d": torch.randn(B, 16, H // 4, W // 4, generator=gen).to(dev),
                        "layer1_feat2d": torch.randn(B, 256, H // 4, W // 4, generator=gen).to(dev)})
    with torch.no_grad():
        assert mf._runner() is not None and len(mf._runner().segments) == 2          # cut after conv1 (MVX fusion)
        out = mf(bd)
    x4 = out["multi_scale_3d_features"]["x_conv4"]
    assert x4.features.shape[1] == 64 and bool(torch.isfinite(x4.features).all())
    # MVX glue vs loop restatement (spconv_backbone.py:672-675,717-748)
    x1 = out["multi_scale_3d_features"]["x_conv1"]
    with torch.no_grad():
        plain = mf.conv1(mf.conv_input(__import__("dualfusion").spconv.SparseConvTensor(f, c, mf.sparse_shape, B)))
    up = torch.nn.functional.interpolate(bd["img_dict"]["mvx_layer1_feat2d"], (H, W), mode="bilinear").cpu().numpy()
    ind = plain.indices.cpu().numpy()
    vs, pr = np.array([0.1, 0.05, 0.05], np.float32), np.array([-3., -40., 0.], np.float32)
    P = (K @ Tr).astype(np.float32)
    exp = plain.features.cpu().numpy().copy()
    for i in range(0, len(ind), 37):
        zyx = ind[i, 1:].astype(np.float32) * vs + pr
        hcoord = P @ np.array([zyx[2], zyx[1], zyx[0], 1.0], np.float32)
        u, v = int(hcoord[0] / hcoord[2]), int(hcoord[1] / hcoord[2])
        if 0 <= u < W and 0 <= v < H:
            exp[i] += up[ind[i, 0], :, v, u]
        np.testing.assert_allclose(x1.features[i].cpu().numpy(), exp[i], rtol=1e-3, atol=1e-3)


def test_two_frames_in_flight_equal_sequential():
    """A serving process may keep two frames in flight per GPU (one host thread + HIP stream + model replica each).
    Frames are independent: concurrent execution must give every frame exactly the result of a sequential run
    (per-thread geometry stream / ordering events in the native executor, no shared scratch)."""
    import threading
    import types
    from dualfusion import synth
    from dualfusion.fusion import build_centerpoint_fusion, synthetic_camera_inputs
    from dualfusion.pipeline import CenterPointHotPath
    dev = torch.device("cuda:0")
    bench = types.SimpleNamespace(run_step=lambda m, p, e: m(p, batch_dict=e[0], example=e[1]))
    slots = []
    for i in range(2):
        torch.manual_seed(0)
        m = CenterPointHotPath(fusion=build_centerpoint_fusion()).eval().to(dev)
        pts = [torch.from_numpy(synth.nusc_sweep(seed=i * 1000)).to(dev)]   # different sweeps / cameras per slot
        extra = synthetic_camera_inputs(1, dev, seed=1234 + i)
        slots.append((m, pts, extra, torch.cuda.Stream()))
    want = []
    for m, pts, extra, _ in slots:
        dense, multi = bench.run_step(m, pts, extra)
        want.append((dense.clone(), [multi[k].indices.clone() for k in ("conv1", "conv2", "conv3", "conv4")]))
    torch.cuda.synchronize()
    got = [[], []]

    def work(i):
        m, pts, extra, st = slots[i]
        with torch.cuda.stream(st):
            for _ in range(6):
                dense, multi = bench.run_step(m, pts, extra)
                got[i].append((dense.clone(), [multi[k].indices.clone() for k in ("conv1", "conv2", "conv3", "conv4")]))
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    torch.cuda.synchronize()
    for i in range(2):
        for dense, idx in got[i]:
            for a, b in zip(idx, want[i][1]):
                assert torch.equal(a, b)
            assert float((dense - want[i][0]).abs().max()) <= 1e-5 * float(want[i][0].abs().max())


@pytest.mark.parametrize("aug", [False, True])
def test_voxel_image_sample_kernel_equals_the_torch_composition(aug):
    """df3d_voxel_image_sample (csrc/mvx.hip: voxel -> augmentation inverse -> pixel -> bilinear upsample tap at the
    truncated pixel -> sum / padded scatter in one launch) against the torch composition it replaces
    (`_project` + `_sample_int`, pinned to the reference's point_fusion by tests/golden/vr_fusion.npz): same operations
    in the same order, so the pixels and features agree BIT FOR BIT, incl. voxels that project outside the image,
    behind the camera and onto the image border."""
    from dualfusion import ops
    from dualfusion.backbones import VoxelBackBone8xFusion
    dev = torch.device("cuda:0")
    B, H, W = 3, 96, 320
    m = VoxelBackBone8xFusion(dict(VR_CFG), 4, [512, 512, 40]).to(dev).eval()
    g = torch.Generator().manual_seed(5 + int(aug))
    n = 60000
    ind = torch.stack([torch.randint(0, B, (n,), generator=g), torch.randint(0, 41, (n,), generator=g),
                       torch.randint(0, 512, (n,), generator=g), torch.randint(0, 512, (n,), generator=g)], 1).int()
    ind = ind[torch.argsort(ind[:, 0], stable=True)].contiguous().to(dev)
    K = np.array([[180., 0, W / 2, 0.3], [0, 180., H / 2, -0.2], [0, 0, 1, 0.002]], np.float32)
    Tr = np.array([[0, -1, 0, 0.01], [0, 0, -1, -0.08], [1, 0, 0, -0.27], [0, 0, 0, 1]], np.float32)
    l2i = torch.from_numpy(np.stack([K @ Tr] * B)).to(dev)
    bd = dict(batch_size=B, lidar2img=l2i, image_hw=(H, W))
    if aug:
        bd.update(noise_scale=[1.03, 0.97, 1.0], noise_rot=[0.31, -0.2, 0.0], flip_x=[True, False, False], flip_y=[False, True, False])

    class X(object):
        pass
    for C, stride in ((16, 1), (256, 8)):
        fmap = torch.randn(B, C, H // 4, W // 4, generator=g).to(dev)
        feats = torch.randn(n, C, generator=g).to(dev)
        x = X()
        x.indices, x.features = ind, feats
        with torch.no_grad():
            xyz, uv = m._project(x, stride, bd)
            want = m._sample_int(fmap, ind[:, 0].long(), uv, (H, W))
            vs, r0 = m._geometry_floats()
            got, guv = ops.voxel_image_sample(ind, B, float(stride), vs, r0, m._aug_params(dict(bd), B, dev), l2i, fmap, (H, W),
                                              want_uv=True)
            assert torch.equal(guv, uv)
            inside = ((uv[:, 0] >= 0) & (uv[:, 0] < W) & (uv[:, 1] >= 0) & (uv[:, 1] < H)).float().mean().item()
            assert 0.02 < inside < 0.98                                   # both cases are exercised
            assert torch.equal(got, want)
            # sum with the voxel features and the padded scatter + normalised grid
            got2, _ = ops.voxel_image_sample(ind, B, float(stride), vs, r0, m._aug_params(dict(bd), B, dev), l2i, fmap, (H, W),
                                             add=feats)
            assert torch.equal(got2, feats + want)
            b, slot, n_max = m._query_slots(ind, B)
            rows = b * n_max + slot
            out = torch.zeros(B * n_max, C, device=dev)
            grid = torch.zeros(B * n_max, 2, device=dev)
            ops.voxel_image_sample(ind, B, float(stride), vs, r0, m._aug_params(dict(bd), B, dev), l2i, fmap, (H, W), rows=rows,
                                   out=out, grid=grid)
            ref = torch.zeros(B, n_max, C, device=dev)
            ref[b, slot] = want
            rg = torch.zeros(B, n_max, 2, device=dev)
            rg[b, slot] = uv / torch.tensor([W, H], dtype=torch.float32, device=dev)
            assert torch.equal(out.view(B, n_max, C), ref) and torch.equal(grid.view(B, n_max, 2), rg)


def test_pipelined_frames_equal_isolated_frames():
    """bench.py's mode of the Voxel-RCNN tree and of the CenterPoint detector: resident point clouds voxelised on the voxel
    stream (`hard_voxelize_clouds(resident_inputs=True)`), the stride-8 query geometry on a side stream that waits for the
    voxeliser's event only, the native executor's geometry stream likewise (three persistent arenas in rotation), two to three
    frames in flight at most, NO synchronisation between frames -- against the same frames run
    one at a time with a device synchronisation after each and everything on the current stream.  Outputs must be
    identical, frame by frame, over several rounds (buffers of frame k are released while frame k + 1 / k + 2 run)."""
    import types
    from dualfusion import ops, synth, workloads
    from dualfusion.fusion import build_centerpoint_fusion, synthetic_camera_inputs
    from dualfusion.pipeline import CenterPointHotPath
    dev = torch.device("cuda:0")
    args = types.SimpleNamespace(workload="vr_fusion", frames=3, batch=2, inflight=1)
    wl = workloads.make(args, 0, 1, dev)
    old = os.environ.get("DF3D_VOXEL_STREAM")
    try:
        os.environ["DF3D_VOXEL_STREAM"] = "0"
        assert wl.prefetch
        wl.prefetch = False                                       # isolated frames: nothing of a batch starts before its step
        want = []
        for k in range(3):
            out = wl.step(k, "detect")
            torch.cuda.synchronize()
            want.append((out["encoded_spconv_tensor"].features.clone(), out["encoded_spconv_tensor"].indices.clone()))
        os.environ["DF3D_VOXEL_STREAM"] = "1"
        wl.prefetch = True              # round 5: batch k + 1's voxelisation, index sets, FPS and ball query beside batch k
        got = []
        for k in range(18):                                       # six rounds over the frames, back to back
            out = wl.step(k, "detect")
            got.append((out["encoded_spconv_tensor"].features.clone(), out["encoded_spconv_tensor"].indices.clone()))
        torch.cuda.synchronize()
    finally:
        if old is None:
            os.environ.pop("DF3D_VOXEL_STREAM", None)
        else:
            os.environ["DF3D_VOXEL_STREAM"] = old
    for k, (f, i) in enumerate(got):
        assert torch.equal(i, want[k % 3][1]) and torch.equal(f, want[k % 3][0]), k
    # CenterPoint hot path with the camera fusion: resident inputs on / off
    torch.manual_seed(0)
    m = CenterPointHotPath(fusion=build_centerpoint_fusion()).eval().to(dev)
    frames = [([torch.from_numpy(synth.nusc_sweep(seed=40 + j)).to(dev)], synthetic_camera_inputs(1, dev, seed=j)) for j in range(3)]
    torch.cuda.synchronize()
    with torch.no_grad():
        want = []
        for pts, (bd, ex) in frames:
            want.append(m(pts, batch_dict=dict(bd), example=dict(ex))[0].clone())
            torch.cuda.synchronize()
        m.resident_inputs = m.fusion.resident_inputs = True
        for decouple in ("1", "0"):          # the executor's geometry stream waits for the voxeliser's event only / for the stream
            os.environ["DF3D_EXEC_DECOUPLE"] = decouple
            try:
                got = [m(pts, batch_dict=dict(bd), example=dict(ex))[0].clone() for _ in range(8) for pts, (bd, ex) in frames]
                torch.cuda.synchronize()
            finally:
                os.environ.pop("DF3D_EXEC_DECOUPLE", None)
            for k, y in enumerate(got):
                assert torch.equal(y, want[k % 3]), (decouple, k)


def test_prefetched_geometry_equals_isolated_frames():
    """Round 4: the head of frame k + 1 (voxelisation, every rulebook of the backbone, the fusion adapter's projection and
    query slots -- with all count round trips) built on the detector's helper thread while frame k is queued
    (`CenterPointHotPath.prefetch`, dualfusion/prefetch.py, `df3d_backbone_geometry` + `df3d_backbone_convs`), then TWO
    detector replicas alternating over two streams from one host thread (bench.py's `in_flight` pass) -- against the same
    frames run one at a time with a device synchronisation after each.  Bit-identical, frame by frame, over several rounds
    (frame slots of the executor's arenas are rewritten while later frames run)."""
    from dualfusion import synth
    from dualfusion.fusion import build_centerpoint_fusion, synthetic_camera_inputs
    from dualfusion.pipeline import CenterPointHotPath
    dev = torch.device("cuda:0")
    frames = [([torch.from_numpy(synth.nusc_sweep(seed=70 + j)).to(dev)], synthetic_camera_inputs(1, dev, seed=20 + j)) for j in range(3)]

    def model():
        torch.manual_seed(0)
        return CenterPointHotPath(fusion=build_centerpoint_fusion()).eval().to(dev)
    m = model()
    torch.cuda.synchronize()
    with torch.no_grad():
        want = []
        for pts, (bd, ex) in frames:
            y, multi = m(pts, batch_dict=dict(bd), example=dict(ex))
            want.append((y.clone(), [multi[k].indices.clone() for k in ("conv1", "conv2", "conv3", "conv4")],
                         multi["conv4"].features.clone()))
            torch.cuda.synchronize()
        m.resident_inputs = m.fusion.resident_inputs = True
        # (1) one replica, the next frame prefetched while the current one is queued
        nf, rounds = len(frames), 8
        staged = dict(frames[0][1][0])
        assert m.prefetch(frames[0][0], staged)
        got = []
        for k in range(rounds * nf):
            pts, (bd, ex) = frames[k % nf]
            cur, staged = staged, dict(frames[(k + 1) % nf][1][0])
            m.prefetch(frames[(k + 1) % nf][0], staged)
            y, multi = m(pts, batch_dict=cur, example=dict(ex))
            got.append((y.clone(), [multi[n].indices.clone() for n in ("conv1", "conv2", "conv3", "conv4")],
                        multi["conv4"].features.clone()))
        torch.cuda.synchronize()
        for k, (y, idx, f4) in enumerate(got):
            w = want[k % nf]
            assert all(torch.equal(a, b) for a, b in zip(idx, w[1])), k
            assert torch.equal(f4, w[2]) and torch.equal(y, w[0]), k
        # a frame that was NOT prefetched takes the in-line path; a prefetched one that is never consumed is dropped
        y = m(frames[1][0], batch_dict=dict(frames[1][1][0]), example={})[0]
        assert torch.equal(y, want[1][0])
        # (2) two replicas / two streams / one host thread, each replica prefetching its own next frame (stride 2)
        ms = [m, model()]
        ms[1].resident_inputs = ms[1].fusion.resident_inputs = True
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        staged = [None, None]
        for r in range(2):
            staged[r] = dict(frames[r % nf][1][0])
            ms[r].prefetch(frames[r % nf][0], staged[r])
        got = []
        for k in range(rounds * nf):
            r = k % 2
            with torch.cuda.stream(streams[r]):
                cur, staged[r] = staged[r], dict(frames[(k + 2) % nf][1][0])
                ms[r].prefetch(frames[(k + 2) % nf][0], staged[r])
                y, multi = ms[r](frames[k % nf][0], batch_dict=cur, example={})
                got.append((y.clone(), multi["conv4"].indices.clone()))
                y.record_stream(streams[r])
        torch.cuda.synchronize()
        for k, (y, i4) in enumerate(got):
            assert torch.equal(i4, want[k % nf][1][3]) and torch.equal(y, want[k % nf][0]), k
    for mm in ms:
        mm.close()


def test_transfusion_encoder_frame_head_equals_inline():
    """The TransFusion encoder with its frame head (voxelisation of the batch + every rulebook) built ahead on the module's
    worker thread (`SparseEncoderFusion.prefetch` / `take_head`, bench.py's tf_fusion step) against the in-line path:
    bit-identical dense maps, frame by frame, in split precision and in the bf16 mode of configs[2]."""
    from dualfusion import ops, synth
    from dualfusion.backbones import SparseEncoderFusion
    from make_golden import ACTR_CFG
    dev = torch.device("cuda:0")
    B, ori_hw, in_hw, fh, fw = 2, (225, 400), (112, 200), 28, 50
    rng = [-9.6, -9.6, -5.0, 9.6, 9.6, 3.0]
    enc = SparseEncoderFusion(in_channels=5, sparse_shape=[41, 256, 256], output_channels=128, encoder_channels=TF_CH,
                              encoder_paddings=TF_PAD, block_type='basicblock', fusion_pos=[3], voxel_size=[0.075, 0.075, 0.2],
                              point_cloud_range=rng, fusion_layer=dict(type='ACTR', pfat_cfg=dict(ACTR_CFG)))
    enc, _ = _load_det(enc, dev)
    cams = synth.nusc_cameras(image_hw=ori_hw, focal=316.0)
    metas = _tf_metas(B, cams, ori_hw, in_hw)
    img = torch.from_numpy(np.random.RandomState(0).standard_normal((B * 6, 256, fh, fw)).astype(np.float32)).to(dev)
    frames = [[torch.from_numpy(synth.nusc_sweep(seed=90 + 7 * j + b)).to(dev) for b in range(B)] for j in range(3)]
    old = ops.CONV_PRECISION
    try:
        for mode in ("split", "bf16"):
            ops.CONV_PRECISION = mode
            with torch.no_grad():
                want = []
                for pts in frames:
                    f, c = ops.hard_voxelize_clouds(pts, synth.NUSC_VOXEL, rng, 10, 120000)
                    want.append(enc(f, c, B, img_feats=[img], img_metas=[dict(m) for m in metas]).clone())
                    torch.cuda.synchronize()
                assert enc.prefetch(frames[0], synth.NUSC_VOXEL, rng, 10, 120000)
                for k in range(9):
                    head = enc.take_head(frames[k % 3])
                    assert head is not None
                    enc.prefetch(frames[(k + 1) % 3], synth.NUSC_VOXEL, rng, 10, 120000)
                    f, c, prepared = head
                    y = enc(f, c, B, img_feats=[img], img_metas=[dict(m) for m in metas], prepared=prepared)
                    assert torch.equal(y, want[k % 3]), (mode, k)
                torch.cuda.synchronize()
    finally:
        ops.CONV_PRECISION = old
        enc.close()


@pytest.mark.parametrize("tag,with_aug", [("plain", False), ("aug", True)])
def test_voxel_rcnn_basic_gate_vs_reference_golden(golden, tag, with_aug):
    """`I_FUSION_METHOD: BasicGate` of the Voxel-RCNN tree (round 4) against the reference's own class
    (VR/pcdet/models/model_utils/attention.py:88-177; golden vr_gate.npz, make_golden.py gen_vr_gate): stride-2 voxels
    projected through the KITTI calibration, `pts2img` (clamped pixels, last writer wins, cropped canvas), two 3 x 3
    convolutions, sigmoid, product with the image features -- without and with augmentation records.
    Round 6: (1) with the reference's own batch_dict key -- `calib` objects, projected on the host in numpy the way the devkit
    does (`KittiCalibration`) -- EVERY pixel is within 1e-3; (2) with the composed `lidar2img` on the device (the fast path) a
    voxel within fp32 rounding of a canvas-cell boundary may land in the neighbouring cell: every voxel that does is within
    2e-2 px of such a boundary, and every pixel that differs from (1) lies in the 5 x 5 neighbourhood (two 3 x 3
    convolutions) of a cell such a voxel left or entered -- nothing else differs."""
    import detgen
    from dualfusion import spconv as sp
    from dualfusion.backbones import KittiCalibration, VoxelBackBone8xFusion
    from make_golden import VRF, vrf_calib
    dev = torch.device("cuda:0")
    g = golden("vr_gate.npz")
    cfg = dict(NAME='VoxelBackBone8xFusion', USE_IMG=True, FUSION_POS=[1, 4], FUSION_METHOD='MVX+ACTRv2', FEATURE_LEVELS=[0],
               LT_CFG=dict(VRF["lt"]), ACTR_CFG=dict(VRF["actr"]), HYBRID_CFG=dict(VRF["hybrid"]),
               I_FUSION_METHOD="BasicGate", IFAT_CFG=dict(img_num_channels=[256, 512, 1024], pts_num_channels=[32, 64, 64]))
    m = VoxelBackBone8xFusion(cfg, 4, [1408, 1600, 40]).to(dev).eval()
    assert m.ifat is not None and not any(k.startswith("ifat") for k in m.state_dict())     # unregistered, as in the reference
    stack = m.ifat.spatial_basic_list[0].eval()
    stack.load_state_dict({k[len("stack_"):]: torch.from_numpy(g[k]) for k in g.files if k.startswith("stack_")})
    B, (H, W) = VRF["batch"], VRF["hw"]
    ind2 = g["ind2"]
    f2 = detgen.randn("vrg_f2", (len(ind2), 32))
    img = detgen.randn("vrg_img", (B, 256, H // 4, W // 4))
    aug = {}
    if with_aug:
        aug = dict(noise_scale=torch.tensor([1.03, 0.96]).to(dev), noise_rot=torch.tensor([0.21, -0.33]).to(dev),
                   flip_x=torch.tensor([True, False]).to(dev))
    bd_calib = dict(batch_size=B, calib=[KittiCalibration(*vrf_calib(b)) for b in range(B)], image_hw=(H, W), **aug)
    bd_matrix = dict(batch_size=B, lidar2img=torch.from_numpy(g["lidar2img"][:, :3].astype(np.float32)).to(dev), image_hw=(H, W), **aug)
    x2 = sp.SparseConvTensor(torch.from_numpy(f2).to(dev), torch.from_numpy(ind2).to(dev), [21, 800, 704], B)
    with torch.no_grad():
        y = m._gate_images([torch.from_numpy(img).to(dev)], [x2, None, None], bd_calib)[0]
        y_dev = m._gate_images([torch.from_numpy(img).to(dev)], [x2, None, None], bd_matrix)[0]
        uv_host = m._project(x2, 2, bd_calib)[1].cpu().numpy().astype(np.float64)
        uv_dev = m._project(x2, 2, bd_matrix)[1].cpu().numpy().astype(np.float64)
    want = g[tag + "_gated"]
    scale = np.abs(want).max()
    err = np.abs(y[:, :4].cpu().numpy() - want).max(1)                # per pixel: (1) every one of them
    assert err.max() <= 1e-3 * scale, (tag, float(err.max() / scale), int((err > 1e-3 * scale).sum()))
    assert np.median(err) < 1e-5
    # (2) the device projection
    assert (np.abs(uv_dev - uv_host) <= 1e-2 + 2e-5 * np.abs(uv_host)).all()      # (points near the camera plane project far out)
    Hf, Wf = H // 4, W // 4

    def cell(uv):
        n = np.clip(uv.astype(np.float32) / np.array([W, H], np.float32), 0.0, 1.0)
        return (n[:, 1] * np.float32(Hf)).astype(np.int64), (n[:, 0] * np.float32(Wf)).astype(np.int64)
    (ya, xa), (yb, xb) = cell(uv_host), cell(uv_dev)
    moved = (ya != yb) | (xa != xb)
    frac = np.abs(uv_host / 4.0 - np.round(uv_host / 4.0)) * 4.0                      # distance to a canvas-cell boundary, px
    assert (frac[moved].min(1) <= 2e-2).all() and moved.sum() <= 0.01 * len(moved), int(moved.sum())
    diff = np.abs((y_dev - y)[:, :4].cpu().numpy()).max(1) > 1e-3 * scale           # [B, Hf, Wf]
    near = np.zeros_like(diff)
    bcol = ind2[:, 0]
    for i in np.nonzero(moved)[0]:
        for cy, cx in ((ya[i], xa[i]), (yb[i], xb[i])):
            near[bcol[i], max(cy - 2, 0):cy + 3, max(cx - 2, 0):cx + 3] = True
    assert not (diff & ~near).any(), int((diff & ~near).sum())


def test_launch_tape_over_neck_and_head_equals_plain_detector():
    """Round 4: neck + head of the CenterPoint detector re-issued from a launch tape (dualfusion/tape.py: the recorded C-ABI
    calls with the stream and the input address rewritten, buffers from the tape's private pool) -- bit-identical head maps
    and losses to the plain module path for every frame, through the warm-up / record / replay sequence, on a second stream,
    and again after an in-place parameter update (which must re-record)."""
    from dualfusion import synth
    from dualfusion.pipeline import NUSC_TASKS, CenterPointDetector
    dev = torch.device("cuda:0")
    ncls = [t["num_class"] for t in NUSC_TASKS]
    frames = []
    for j in range(3):
        tg = synth.centerhead_targets(1, ncls, seed=40 + j)
        frames.append(([torch.from_numpy(synth.nusc_sweep(seed=90 + j)).to(dev)],
                       {k: [torch.from_numpy(a).to(dev) for a in v] for k, v in tg.items()}))
    torch.manual_seed(0)
    plain = CenterPointDetector().eval().to(dev)
    torch.manual_seed(0)
    taped = CenterPointDetector().eval().to(dev)
    taped.launch_tape = True

    def run(m, pts, ex, loss):
        out = m(pts, example=ex, return_loss=loss)
        if loss:
            return [torch.stack([v.float().reshape(()) for v in out[k]]).clone() for k in ("loss", "hm_loss", "loc_loss")]
        return [t.clone() for t in out]                      # predict_device: (boxes, scores, labels, counts)

    def maps(m, pts):
        x, _ = m.hot_path(pts)
        return [v.clone() for d in m.bbox_head(x) for _, v in sorted(d.items())]

    with torch.no_grad():
        want_maps = [maps(plain, pts) for pts, _ in frames]
        for rnd in range(3):
            for j, (pts, ex) in enumerate(frames):
                for a, b in zip(run(taped, pts, ex, True), run(plain, pts, ex, True)):
                    assert torch.equal(a, b), (rnd, j)
        st = taped._tail_tape.stats
        assert st["plain"] == 1 and st["recorded"] == 1 and st["replayed"] == 7, (st, taped._tail_tape.refused_ops)
        # the head maps themselves (the tape's result object), and detections decoded from them
        for j, (pts, ex) in enumerate(frames):
            hp = taped.hot_path
            hp.defer_neck = True
            try:
                bev, _ = hp(pts)
            finally:
                hp.defer_neck = False
            preds = taped._taped_tail(bev)
            got = [v.clone() for d in preds for _, v in sorted(d.items())]
            assert len(got) == len(want_maps[j]) and all(torch.equal(a, b) for a, b in zip(got, want_maps[j])), j
            for a, b in zip(run(taped, pts, ex, False), run(plain, pts, ex, False)):
                assert torch.equal(a, b), j
        # another stream: the replay follows torch's current stream
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            got = run(taped, frames[1][0], frames[1][1], True)
        side.synchronize()
        for a, b in zip(got, run(plain, frames[1][0], frames[1][1], True)):
            assert torch.equal(a, b)
        # an in-place update of a parameter: the tape is stale, the next frames warm up / record / replay again
        for m in (plain, taped):
            bn = m.bbox_head.shared_conv[1]
            bn.bias.add_(0.125)
            m.hot_path.neck.blocks[0][1].weight.mul_(1.5)
        before = dict(st)
        for rnd in range(2):
            for j, (pts, ex) in enumerate(frames):
                for a, b in zip(run(taped, pts, ex, True), run(plain, pts, ex, True)):
                    assert torch.equal(a, b), ("updated", rnd, j)
        assert st["plain"] == before["plain"] + 1 and st["recorded"] == before["recorded"] + 1, st
        # a precision round trip (split -> split3 -> split): the modules replace their packed filters / plans when the mode
        # changes, so the tape of the returning mode must be recorded again instead of replayed with the old addresses
        from dualfusion import ops as _ops
        old_mode = _ops.CONV_PRECISION
        before = dict(st)
        try:
            for mode in ("split3", old_mode):
                _ops.CONV_PRECISION = mode
                for rnd in range(2):
                    for j, (pts, ex) in enumerate(frames):
                        for a, b in zip(run(taped, pts, ex, True), run(plain, pts, ex, True)):
                            assert torch.equal(a, b), (mode, rnd, j)
        finally:
            _ops.CONV_PRECISION = old_mode
        assert st["plain"] == before["plain"] + 2 and st["recorded"] == before["recorded"] + 2, st
        # modes whose neck ends in launches torch dispatches itself (bf16 / exact fp32: torch.cat of the upsampled
        # maps, a .contiguous() copy) are NOT pure C-ABI sections -- a replay would skip those launches and hand the head the
        # recording frame's map.  The recording notices the foreign operators and the key runs the module path from then on:
        # every frame its own result, nothing replayed.
        for mode in ("bf16", "fp32"):
            before = dict(st)
            try:
                _ops.CONV_PRECISION = mode
                for rnd in range(3):
                    for j, (pts, ex) in enumerate(frames):
                        for a, b in zip(run(taped, pts, ex, True), run(plain, pts, ex, True)):
                            assert torch.equal(a, b), (mode, rnd, j)
            finally:
                _ops.CONV_PRECISION = old_mode
            assert st["refused"] == before["refused"] + 1 and st["replayed"] == before["replayed"], (mode, st)
            assert st["recorded"] == before["recorded"] and taped._tail_tape.refused_ops, (mode, st)
        _ops.CONV_PRECISION = old_mode
        for rnd in range(2):                                  # back in the taped mode
            for j, (pts, ex) in enumerate(frames):
                for a, b in zip(run(taped, pts, ex, True), run(plain, pts, ex, True)):
                    assert torch.equal(a, b), ("back", rnd, j)
        # round 5 (found by bench.py's precision probe: memory fault): a precision switch OUTSIDE the detector's forward -- the
        # neck and the head called directly in another mode and back -- makes the modules replace their packed filters / plans
        # without the taped section ever seeing another key.  The tape keeps every tensor whose address it recorded, so the
        # replay that follows reads live memory with the right contents.
        assert taped._tail_tape.stats["replayed"] > 0 and isinstance(next(iter(taped._tail_tape.tapes.values())), object)
        for mode in ("fp32", "split3", old_mode):
            _ops.CONV_PRECISION = mode
            try:
                for m_ in (plain, taped):
                    x, _ = m_.hot_path(frames[0][0])
                    m_.bbox_head(x)
            finally:
                _ops.CONV_PRECISION = old_mode
        import gc
        gc.collect()
        torch.cuda.synchronize()
        junk = [torch.full((1 << 22,), float("nan"), device=dev) for _ in range(8)]      # recycle whatever was freed
        before = dict(st)
        for rnd in range(2):
            for j, (pts, ex) in enumerate(frames):
                for a, b in zip(run(taped, pts, ex, True), run(plain, pts, ex, True)):
                    assert torch.equal(a, b), ("after an outside switch", rnd, j)
        assert st["replayed"] > before["replayed"], st
        del junk
        # `.double().float()` replaces every buffer OBJECT (nn.Module._apply), then in-place edits of the new running
        # statistics: the tape key reads the modules' own slots, so it follows the live buffers and records again
        for m in (plain, taped):
            m.double().float()
            m.bbox_head.shared_conv[1].running_mean.add_(0.125)
            m.hot_path.neck.blocks[0][2].running_var.mul_(1.5)
        before = dict(st)
        for rnd in range(2):
            for j, (pts, ex) in enumerate(frames):
                for a, b in zip(run(taped, pts, ex, True), run(plain, pts, ex, True)):
                    assert torch.equal(a, b), ("converted", rnd, j)
        assert st["recorded"] == before["recorded"] + 1, st
    torch.cuda.synchronize()
