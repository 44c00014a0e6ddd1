"""The PV-RCNN point branch on the GPU (csrc/stackpool.hip, dualfusion/pointnet2_stack.py, pfe.py, roi_heads.PVRCNNHead) against
the host restatement (tests/stacksa_reference.py) and the reference's own outputs (tests/golden/vsa.npz).

Index results are compared with array_equal under a precondition asserted on the reference alone: no (centre, row) pair
within 8 ulps of radius^2 (256 ulps where the centres are RoI grid points, computed in float32 on either side).

Feature results have no bound fixed in advance.  Each test measures the composed float32 path (the torch formulation the
module takes with DF3D_STACK_SA_FUSED=0) against float64 on the same inputs; the fused kernel may be at most 4 x that error
away from float64, in units of the output's largest magnitude -- the margin the project gives matrix-core arithmetic over plain
fp32.  Every figure is printed before it is asserted (pytest -s shows them; DESIGN section 7.16 records them)."""
import copy

import numpy as np
import pytest
import torch

import stacksa_reference as sr

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = 4.0


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def counts(c):
    return torch.tensor(c, dtype=torch.int32, device=DEV)


def rel(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def composed_only(monkeypatch):
    """DF3D_STACK_SA_FUSED=0, and the fused op raises if it is reached anyway"""
    from dualfusion import ops
    monkeypatch.setenv("DF3D_STACK_SA_FUSED", "0")

    def refuse(*a, **k):
        raise AssertionError("the fused kernel was called with DF3D_STACK_SA_FUSED=0")
    monkeypatch.setattr(ops, "stack_sa_fused", refuse)


def count_fused(monkeypatch):
    from dualfusion import ops
    calls, real = [], ops.stack_sa_fused
    monkeypatch.setenv("DF3D_STACK_SA_FUSED", "1")

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "stack_sa_fused", counted)
    return calls


# ---------------------------------------------------------------------------------------------------------------- ball query
@pytest.mark.parametrize("nsample", [16, 32])
def test_ball_query_equals_the_restatement(nsample):
    from dualfusion import ext, ops
    from dualfusion import pointnet2_stack as ps
    fx = sr.ball_fixture()
    assert sr.near_boundary(fx["radius"], fx["xyz"], fx["xyz_cnt"], fx["new_xyz"], fx["new_cnt"]) == 0
    raw, found = sr.ball_query_kernel(fx["radius"], nsample, fx["xyz"], fx["xyz_cnt"], fx["new_xyz"], fx["new_cnt"])
    assert found[fx["far"]] == 0 and found[fx["dense"]] > nsample and ((found > 0) & (found < nsample)).any() and (found[5:8] == 0).all()
    args = (T(fx["xyz"]), counts(fx["xyz_cnt"]), T(fx["new_xyz"]), counts(fx["new_cnt"]))
    assert np.array_equal(ops.ball_query_stack(fx["radius"], nsample, *args).cpu().numpy(), raw)
    idx, mask = ps.ball_query_stack(fx["radius"], nsample, *args)
    want_idx, want_mask = sr.ball_query_stack(fx["radius"], nsample, fx["xyz"], fx["xyz_cnt"], fx["new_xyz"], fx["new_cnt"])
    assert idx.dtype == torch.int32 and mask.dtype == torch.bool
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(mask.cpu().numpy(), want_mask)
    # the pybind-name entry, over an allocation of the caller's: an empty ball touches slot 0 alone
    out = torch.full((19, nsample), 9, dtype=torch.int32, device=DEV)
    want, _ = sr.ball_query_kernel(fx["radius"], nsample, fx["xyz"], fx["xyz_cnt"], fx["new_xyz"], fx["new_cnt"],
                                   idx=np.full((19, nsample), 9, np.int32))
    assert ext.load("pointnet2_stack_cuda").ball_query_wrapper(3, 19, fx["radius"], nsample, args[2], args[3], args[0], args[1], out) == 1
    assert np.array_equal(out.cpu().numpy(), want) and (want[fx["far"], 1:] == 9).all()


def test_ball_query_over_a_long_frame():
    """5 000 rows: 79 steps of 64 rows; interior balls stop early at 16 hits, corner balls read the whole frame"""
    from dualfusion import ops
    fx = sr.big_ball_fixture()
    assert sr.near_boundary(fx["radius"], fx["xyz"], fx["xyz_cnt"], fx["new_xyz"], fx["new_cnt"]) == 0
    args = (T(fx["xyz"]), counts(fx["xyz_cnt"]), T(fx["new_xyz"]), counts(fx["new_cnt"]))
    for nsample in (16, 32, 64):
        want, found = sr.ball_query_kernel(fx["radius"], nsample, fx["xyz"], fx["xyz_cnt"], fx["new_xyz"], fx["new_cnt"])
        assert np.array_equal(ops.ball_query_stack(fx["radius"], nsample, *args).cpu().numpy(), want)
    assert (found > 16).sum() >= 20 and (found < 16).sum() >= 10


# --------------------------------------------------------------------------------------------------------------- fused scale
def _layer(c_in, c1, c2, nsample, radius, seed=7):
    from dualfusion import pointnet2_stack as ps
    layer = ps.StackSAModuleMSG(radii=[radius], nsamples=[nsample], mlps=[[c_in, c1, c2]])
    sd = sr.random_sa_state([[c_in, c1, c2]], seed)
    layer.load_state_dict(sr.torch_state(sd), strict=True)
    return layer.to(DEV).eval(), sd


@pytest.mark.parametrize("c_in,c1,c2,nsample", sr.SCALE_CLASSES)
def test_fused_scale_against_float64_and_the_composed_path(c_in, c1, c2, nsample, monkeypatch):
    from dualfusion import ops
    fx = sr.scale_fixture(c_in)
    assert sr.near_boundary(fx["radius"], fx["xyz"], fx["xyz_cnt"], fx["new_xyz"], fx["new_cnt"]) == 0
    layer, sd = _layer(c_in, c1, c2, nsample, fx["radius"])
    feats64 = torch.from_numpy(fx["features"]) if c_in else None
    want = sr.sa_scale(sr.torch_state(sd), 0, fx["radius"], nsample, fx["xyz"], fx["xyz_cnt"], fx["new_xyz"], fx["new_cnt"],
                       feats64).numpy()
    want_idx, want_empty = sr.ball_query_stack(fx["radius"], nsample, fx["xyz"], fx["xyz_cnt"], fx["new_xyz"], fx["new_cnt"])
    assert want_empty[0] and not want_empty[1:].all()
    args = (T(fx["xyz"]), counts(fx["xyz_cnt"]), T(fx["new_xyz"]), counts(fx["new_cnt"]))
    feats = T(fx["features"]) if c_in else None
    with torch.no_grad():
        rows_in, w_pos, w2, b2 = layer.fused_operands(0, feats)
        assert (rows_in is None) == (c_in == 0)
        pooled, idx, empty = ops.stack_sa_fused(rows_in, *args, fx["radius"], nsample, w_pos, w2, b2, want_idx=True)
        assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(empty.cpu().numpy(), want_empty)
        calls = count_fused(monkeypatch)
        _, fused = layer(*args, features=feats)
        assert len(calls) == 1 and torch.equal(fused, pooled)
        composed_only(monkeypatch)
        _, composed = layer(*args, features=feats)
    e32 = rel(composed.cpu().numpy(), want)
    ef = rel(fused.cpu().numpy(), want)
    efc = rel(fused.cpu().numpy(), composed.cpu().numpy())
    print("scale %3d -> %2d -> %2d, nsample %2d: composed fp32 %.3e, fused %.3e, fused vs composed %.3e (of max |out| = %.3f)"
          % (c_in, c1, c2, nsample, e32, ef, efc, np.abs(want).max()))
    assert 0 < e32 < 1e-5
    assert ef <= MARGIN * e32 and efc <= MARGIN * e32


def test_composed_path_serves_what_the_kernel_does_not(monkeypatch):
    """avg_pool and a 3-layer MLP never reach the kernel, and agree with float64"""
    from dualfusion import pointnet2_stack as ps
    fx = sr.scale_fixture(16)
    args = (T(fx["xyz"]), counts(fx["xyz_cnt"]), T(fx["new_xyz"]), counts(fx["new_cnt"]))
    calls = count_fused(monkeypatch)
    for mlps, pool in (([[16, 16, 16]], "avg_pool"), ([[16, 16, 32, 16]], "max_pool"), ([[16, 24, 16]], "max_pool")):
        layer = ps.StackSAModuleMSG(radii=[fx["radius"]], nsamples=[16], mlps=mlps, pool_method=pool)
        sd = sr.random_sa_state(mlps, 11)
        layer.load_state_dict(sr.torch_state(sd), strict=True)
        layer = layer.to(DEV).eval()
        with torch.no_grad():
            _, got = layer(*args, features=T(fx["features"]))
        want = sr.sa_scale(sr.torch_state(sd), 0, fx["radius"], 16, fx["xyz"], fx["xyz_cnt"], fx["new_xyz"], fx["new_cnt"],
                           torch.from_numpy(fx["features"]), pool_method=pool).numpy()
        assert rel(got.cpu().numpy(), want) < 1e-5
    assert calls == []


# ------------------------------------------------------------------------------------------------------------------ training
def test_composed_path_trains():
    """16 -> 16 -> 16, M = 20, N = 60, batch statistics: the gradients to the features and to every parameter against float64
    autograd of the restatement; the yardstick is float32 autograd of the same restatement (torch, CPU), margin 4 x"""
    from dualfusion import pointnet2_stack as ps
    rs = np.random.RandomState(5)
    xyz, new_xyz = rs.uniform(0, 3, (60, 3)).astype(np.float32), rs.uniform(0, 3, (20, 3)).astype(np.float32)
    new_xyz[3] = (30, 30, 30)                                                            # an empty ball
    xyz_cnt, new_cnt, radius, ns = [35, 25], [12, 8], 1.0, 16
    assert sr.near_boundary(radius, xyz, xyz_cnt, new_xyz, new_cnt) == 0
    feats = rs.standard_normal((60, 16)).astype(np.float32)
    weight = rs.standard_normal((20, 16)).astype(np.float32)
    sd = {k: v for k, v in sr.random_sa_state([[16, 16, 16]], 13).items()}
    names = [k for k in sd if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]

    def restated(dtype):
        p = {k: (torch.from_numpy(v).to(dtype).requires_grad_() if k in names else torch.from_numpy(np.asarray(v))) for k, v in sd.items()}
        f = torch.from_numpy(feats).to(dtype).requires_grad_()
        out = sr.sa_scale(p, 0, radius, ns, xyz, xyz_cnt, new_xyz, new_cnt, f, dtype=dtype, training=True)
        (out * torch.from_numpy(weight).to(dtype)).sum().backward()
        return out.detach().numpy(), dict({k: p[k].grad.numpy() for k in names}, features=f.grad.numpy())

    out64, g64 = restated(torch.float64)
    out32, g32 = restated(torch.float32)
    layer = ps.StackSAModuleMSG(radii=[radius], nsamples=[ns], mlps=[[16, 16, 16]])
    layer.load_state_dict(sr.torch_state(sd), strict=True)
    layer = layer.to(DEV).train()
    f = T(feats).requires_grad_()
    _, out = layer(T(xyz), counts(xyz_cnt), T(new_xyz), counts(new_cnt), features=f)
    (out * T(weight)).sum().backward()
    got = dict({k: p.grad.cpu().numpy() for k, p in layer.named_parameters()}, features=f.grad.cpu().numpy())
    assert sorted(got) == sorted(g64)
    e_out = rel(out32, out64)
    print("training forward: torch fp32 %.3e, composed path %.3e" % (e_out, rel(out.detach().cpu().numpy(), out64)))
    assert rel(out.detach().cpu().numpy(), out64) <= MARGIN * e_out
    for k in sorted(g64):
        e32, e = rel(g32[k], g64[k]), rel(got[k], g64[k])
        print("grad %-20s torch fp32 %.3e, composed path %.3e" % (k, e32, e))
        assert 0 < e32 < 1e-4 and e <= MARGIN * e32, k
    # the running statistics moved (batch statistics were used and recorded)
    assert not np.array_equal(layer.mlps[0][1].running_mean.cpu().numpy(), sd["mlps.0.1.running_mean"])


# ----------------------------------------------------------------------------------------------------------- BEV interpolation
BEV_RANGE, BEV_VOXEL, BEV_STRIDE = [0.0, -4.0, -2.0, 10.0, 10.0, 2.0], [0.25, 0.25, 0.5], 8        # one BEV pixel = 2 m


def _bev_keypoints():
    rs = np.random.RandomState(21)
    kp = np.concatenate([rs.randint(0, 2, (40, 1)), rs.uniform(0.2, 9.6, (40, 1)), rs.uniform(-3.8, 9.6, (40, 1)),
                         rs.uniform(-1, 1, (40, 1))], 1).astype(np.float32)
    kp[0, 1:3] = (-0.7, 1.3)              # left of column 0
    kp[1, 1:3] = (3.3, 11.1)              # beyond the last row (H = 7: y index 7.55)
    kp[2, 1:3] = (4.0, 2.0)               # exactly on the centre of pixel (x 2, y 3)
    kp[3, 1:3] = (9.9, 9.99)              # past the last column and the last row
    return kp


def _bev_magnitudes(kp, grad_out, shape):
    """per element of grad_bev: the sum of |grad_out| * |weight| over its contributions, and their number"""
    B, C, H, W = shape
    x, y = [v.double().numpy() for v in sr.bev_coords(torch.from_numpy(kp), BEV_RANGE, BEV_VOXEL, BEV_STRIDE)]
    mag, n = np.zeros(shape), np.zeros(shape)
    for m in range(len(kp)):
        x0, x1 = np.clip([np.floor(x[m]), np.floor(x[m]) + 1], 0, W - 1)
        y0, y1 = np.clip([np.floor(y[m]), np.floor(y[m]) + 1], 0, H - 1)
        for xi, yi, w in ((x0, y0, (x1 - x[m]) * (y1 - y[m])), (x0, y1, (x1 - x[m]) * (y[m] - y0)),
                          (x1, y0, (x[m] - x0) * (y1 - y[m])), (x1, y1, (x[m] - x0) * (y[m] - y0))):
            mag[int(kp[m, 0]), :, int(yi), int(xi)] += np.abs(grad_out[m]) * abs(w)
            n[int(kp[m, 0]), :, int(yi), int(xi)] += 1
    return mag, n


@pytest.mark.parametrize("C", [8, 256])
def test_bev_interpolate_forward_and_ordered_backward(C):
    from dualfusion import ops
    H, W = 7, 5
    rs = np.random.RandomState(22)
    kp, bev = _bev_keypoints(), rs.standard_normal((2, C, H, W)).astype(np.float32)
    x, y = sr.bev_coords(torch.from_numpy(kp), BEV_RANGE, BEV_VOXEL, BEV_STRIDE)
    assert float(x[0]) < 0 and float(y[1]) > H - 1 and float(x[2]) == 2.0 and float(y[2]) == 3.0 and float(x[3]) > W - 1
    want = sr.bev_interpolate(torch.from_numpy(kp), torch.from_numpy(bev), BEV_RANGE, BEV_VOXEL, BEV_STRIDE).numpy()
    assert np.array_equal(want[2], bev[int(kp[2, 0]), :, 3, 2])                         # the pixel itself
    got = ops.bev_interpolate(T(kp), T(bev), BEV_RANGE, BEV_VOXEL, BEV_STRIDE).cpu().numpy()
    ulps = np.abs(got.astype(np.float64) - want) / np.spacing(np.maximum(np.abs(want), np.float32(1e-30)))
    print("bev forward, C = %d: max %.1f ulps of the float32 restatement" % (C, ulps.max()))
    assert ulps.max() <= 2
    # backward: the same bits twice, through autograd as well, and float64
    grad_out = rs.standard_normal((40, C)).astype(np.float32)
    g1 = ops.bev_interpolate_backward(T(grad_out), T(kp), (2, C, H, W), BEV_RANGE, BEV_VOXEL, BEV_STRIDE)
    g2 = ops.bev_interpolate_backward(T(grad_out), T(kp), (2, C, H, W), BEV_RANGE, BEV_VOXEL, BEV_STRIDE)
    b = T(bev).requires_grad_()
    ops.bev_interpolate(T(kp), b, BEV_RANGE, BEV_VOXEL, BEV_STRIDE).backward(T(grad_out))
    assert torch.equal(g1, g2) and torch.equal(g1, b.grad)
    b64 = torch.from_numpy(bev).double().requires_grad_()
    sr.bev_interpolate(torch.from_numpy(kp), b64, BEV_RANGE, BEV_VOXEL, BEV_STRIDE, dtype=torch.float64,
                       coord_dtype=torch.float32).backward(torch.from_numpy(grad_out).double())
    # every pixel's sum of n products against float64 on the same float32 pixel coordinates: (n + 8) * 2^-23 of the sum of the
    # products' magnitudes (the float32 weights: two roundings; one per product and per addition)
    mag, n = _bev_magnitudes(kp, grad_out, (2, C, H, W))
    err = np.abs(g1.cpu().numpy().astype(np.float64) - b64.grad.numpy())
    print("bev backward, C = %d: max error %.3e against float64, largest sum of magnitudes %.3e, up to %d terms"
          % (C, err.max(), mag.max(), n.max()))
    assert (err <= (n + 8) * 2.0 ** -23 * mag).all()
    assert 0 < (n[:, 0] == 0).sum() < 2 * H * W and (g1.cpu().numpy()[n == 0] == 0).all()          # untouched pixels: exactly 0


# -------------------------------------------------------------------------------------------------------- VoxelSetAbstraction
def _vsa_batch(inputs):
    from dualfusion.spconv import SparseConvTensor
    levels = {}
    for stride, (name, (ind, feats)) in zip((1, 2, 4, 8), inputs["levels"].items()):
        levels[name] = SparseConvTensor(T(feats), T(ind), [s // stride for s in sr.VSA_GRID], 2)
    return {"batch_size": 2, "points": T(inputs["points"]), "voxel_coords": T(inputs["voxel_coords"]),
            "spatial_features": T(inputs["bev"]), "spatial_features_stride": inputs["bev_stride"], "multi_scale_3d_features": levels}


@pytest.mark.parametrize("point_source", ["raw_points", "voxel_centers"])
def test_voxel_set_abstraction_against_the_reference(point_source, golden, monkeypatch):
    from dualfusion import pfe
    g = golden("vsa.npz")
    cfg, inputs = sr.vsa_cfg(point_source), sr.vsa_inputs()
    sd = sr.vsa_state(cfg)
    vsa = pfe.VoxelSetAbstraction(cfg, sr.VSA_VOXEL, sr.VSA_RANGE, num_bev_features=sr.VSA_BEV[0], num_rawpoint_features=4)
    vsa.load_state_dict(sr.torch_state(sd), strict=True)
    vsa = vsa.to(DEV).eval()
    want_kp, want_before, want_fused = sr.vsa_forward(sr.torch_state(sd), cfg, inputs)           # float64
    want_before, want_fused = want_before.numpy(), want_fused.numpy()
    assert np.array_equal(want_kp, g["vsa__%s__keypoints" % point_source])
    assert rel(want_fused, g["vsa__%s__point_features" % point_source]) < 1e-10
    with torch.no_grad():
        calls = count_fused(monkeypatch)
        fused = vsa(_vsa_batch(inputs))
        assert len(calls) == 10                                                                  # 5 sources x 2 scales
        composed_only(monkeypatch)
        composed = vsa(_vsa_batch(inputs))
    assert vsa.num_point_features == 32 and vsa.num_point_features_before_fusion == 400
    for out in (fused, composed):
        assert np.array_equal(out["point_coords"].cpu().numpy(), g["vsa__%s__keypoints" % point_source])
    for key, want in (("point_features_before_fusion", want_before), ("point_features", want_fused)):
        if point_source == "raw_points" or key == "point_features":
            stored = g["vsa__%s__%s" % (point_source, "before_fusion" if key.endswith("fusion") else "point_features")]
            want = stored                                                                        # the reference's own output
        e32, ef = rel(composed[key].cpu().numpy(), want), rel(fused[key].cpu().numpy(), want)
        efc = rel(fused[key].cpu().numpy(), composed[key].cpu().numpy())
        print("VoxelSetAbstraction (%s) %s: composed fp32 %.3e, fused %.3e, fused vs composed %.3e" % (point_source, key, e32, ef, efc))
        assert tuple(fused[key].shape) == want.shape and 0 < e32 < 1e-5
        assert ef <= MARGIN * e32 and efc <= MARGIN * e32


# ------------------------------------------------------------------------------------------------------------------ PVRCNNHead
def _head():
    from dualfusion import roi_heads
    torch.manual_seed(3)
    cfg = sr.head_cfg()
    head = roi_heads.PVRCNNHead(32, cfg, num_class=1)
    missing = head.load_state_dict(sr.torch_state(sr.head_pool_state(cfg)), strict=False)
    assert not missing.unexpected_keys and not any(k.startswith("roi_grid_pool_layer") for k in missing.missing_keys)
    for m in head.modules():                                     # non-trivial statistics in the FC layers as well
        if isinstance(m, torch.nn.BatchNorm1d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    return head, cfg


def _head_batch(h, dtype=torch.float32, device=DEV):
    return {"batch_size": 2, "rois": torch.from_numpy(h["rois"]).to(device=device, dtype=dtype),
            "point_coords": torch.from_numpy(h["point_coords"]).to(device=device, dtype=dtype),
            "point_features": torch.from_numpy(h["point_features"]).to(device=device, dtype=dtype),
            "point_cls_scores": torch.from_numpy(h["point_cls_scores"]).to(device=device, dtype=dtype)}


def test_pvrcnn_head_pool_and_eval_forward(golden, monkeypatch):
    g = golden("vsa.npz")
    h = sr.head_inputs()
    head, cfg = _head()
    pool = cfg["ROI_GRID_POOL"]
    grid = sr.global_grid_points(h["rois"], pool["GRID_SIZE"])
    for radius in pool["POOL_RADIUS"]:
        assert sr.near_boundary(radius, h["point_coords"][:, 1:4], [64, 64], grid.reshape(-1, 3), [648, 648], ulps=256) == 0
    # float64 forward: the restated pool under a float64 copy of the head's layers
    head64 = copy.deepcopy(head).double().eval()
    head64.roi_grid_pool = lambda bd: torch.from_numpy(g["head__pooled"])
    with torch.no_grad():
        want = head64(_head_batch(h, torch.float64, "cpu"))
    head = head.to(DEV).eval()
    # the grid points of the product are the restatement's up to float32 rounding of the rotation
    got_grid, _ = head.get_global_grid_points_of_roi(T(h["rois"]), pool["GRID_SIZE"])
    assert np.abs(got_grid.cpu().numpy() - grid).max() < 8e-6
    with torch.no_grad():
        calls = count_fused(monkeypatch)
        fused_pool = head.roi_grid_pool(_head_batch(h))
        fused = head(_head_batch(h))
        assert len(calls) == 4
        composed_only(monkeypatch)
        composed_pool = head.roi_grid_pool(_head_batch(h))
        composed = head(_head_batch(h))
    assert tuple(fused_pool.shape) == (6, 216, 32)
    e32, ef = rel(composed_pool.cpu().numpy(), g["head__pooled"]), rel(fused_pool.cpu().numpy(), g["head__pooled"])
    efc = rel(fused_pool.cpu().numpy(), composed_pool.cpu().numpy())
    print("PVRCNNHead.roi_grid_pool: composed fp32 %.3e, fused %.3e, fused vs composed %.3e" % (e32, ef, efc))
    assert 0 < e32 < 1e-5 and ef <= MARGIN * e32 and efc <= MARGIN * e32
    assert tuple(fused["batch_box_preds"].shape) == (2, 3, 7) and tuple(fused["batch_cls_preds"].shape) == (2, 3, 1)
    assert fused["cls_preds_normalized"] is False
    for key in ("batch_box_preds", "batch_cls_preds"):
        e32, ef = rel(composed[key].cpu().numpy(), want[key].numpy()), rel(fused[key].cpu().numpy(), want[key].numpy())
        efc = rel(fused[key].cpu().numpy(), composed[key].cpu().numpy())
        print("PVRCNNHead.forward %s: composed fp32 %.3e, fused %.3e, fused vs composed %.3e" % (key, e32, ef, efc))
        assert 0 < e32 < 1e-5 and ef <= MARGIN * e32 and efc <= MARGIN * e32


def test_pvrcnn_head_trains():
    h = sr.head_inputs()
    head, cfg = _head()
    head = head.to(DEV).train()
    bd = _head_batch(h)
    gt = torch.zeros((2, 2, 8), device=DEV)
    gt[:, 0, :7] = bd["rois"][:, 0] + torch.tensor([0.1, -0.1, 0.05, 0.1, 0.0, 0.1, 0.05], device=DEV)   # overlaps RoI 0 of each frame
    gt[:, 0, 7] = 1
    bd["gt_boxes"] = gt
    out = head(bd)                                               # train mode: forward_train
    assert tuple(out["rcnn_cls"].shape) == (12, 1) and tuple(out["rcnn_reg"].shape) == (12, 7) and tuple(out["rois"].shape) == (2, 6, 7)
    loss, tb = head.get_loss()
    assert sorted(tb) == ["rcnn_loss", "rcnn_loss_cls", "rcnn_loss_corner", "rcnn_loss_reg"]
    assert all(bool(torch.isfinite(v)) for v in tb.values()) and float(tb["rcnn_loss"]) > 0
    loss.backward()
    grads = {k: p.grad for k, p in head.roi_grid_pool_layer.named_parameters()}
    assert len(grads) == 12 and all(v is not None and bool(torch.isfinite(v).all()) for v in grads.values())
    assert float(grads["mlps.0.0.weight"].abs().max()) > 0 and float(grads["mlps.1.3.weight"].abs().max()) > 0
