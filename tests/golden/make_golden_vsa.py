#!/usr/bin/env python3
"""Generate tests/golden/vsa.npz FROM THE REFERENCE ITSELF: the PV-RCNN point branch.

Runs only where the reference checkout exists.  The reference's own StackSAModuleMSG (through build_local_aggregation_module),
VoxelSetAbstraction.forward and PVRCNNHead.roi_grid_pool run on the CPU in float64: their packages are stubbed in sys.modules
the way make_golden_vrtail does it (the stubs only satisfy `import`), `torch.cuda.IntTensor / FloatTensor` allocate host
tensors, and the compiled module `pointnet2_stack_cuda` is replaced by the host restatement of its kernels
(tests/stacksa_reference.py: ball query and furthest point sampling on float32 coordinates; the stack gather).  The modules'
parameters and inputs are the seeded float32 values of tests/stacksa_reference.py (vsa_state, head_pool_state, vsa_inputs,
head_inputs, scale_fixture), which the tests rebuild from the same seeds; the fixture stores the reference's OUTPUTS and the
names and shapes of its state dicts.

Every output is also computed by the restatement alone and must agree with the reference's to 1e-10 of its scale; the stored
arrays are the reference's.  Seeds are searched until no (centre, row) pair of any ball query lies within the margins the
tests assert (8 ulps of radius^2; 256 ulps for the RoI grid points, which the product computes in float32), so that an index
mismatch in a test is a bug and not rounding."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (paths, _stub, save)
import make_golden_vrtail as mv  # noqa: E402  (attr, import_reference_vr_tail)
import stacksa_reference as sr  # noqa: E402

R = mv.R


# ---- pointnet2_stack_cuda on the host
def ball_query_wrapper(B, M, radius, nsample, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, idx):
    out, _ = sr.ball_query_kernel(radius, nsample, xyz.numpy().astype(np.float32), xyz_batch_cnt.tolist(),
                                  new_xyz.numpy().astype(np.float32), new_xyz_batch_cnt.tolist(), idx=idx.numpy().copy())
    idx.copy_(torch.from_numpy(out))
    return 1


def group_points_wrapper(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, out):
    rows = torch.from_numpy(sr.global_rows(idx.numpy(), idx_batch_cnt.tolist(), features_batch_cnt.tolist()))
    out.copy_(features[rows].permute(0, 2, 1))
    return 1


def farthest_point_sampling_wrapper(B, N, npoint, xyz, temp, output):
    for b in range(B):
        picks = sr.furthest_point_sample(xyz[b].numpy().astype(np.float32), min(N, npoint))
        output[b] = 0                                    # the picks past N are overwritten by the caller's padding
        output[b, :len(picks)] = torch.from_numpy(picks).int()
    return 1


def import_reference():
    mv.import_reference_vr_tail()
    for pkg, path in [("pcdet.ops.pointnet2", R + "/ops/pointnet2"), ("pcdet.ops.pointnet2.pointnet2_stack", R + "/ops/pointnet2/pointnet2_stack"),
                      ("pcdet.models.backbones_3d", R + "/models/backbones_3d"), ("pcdet.models.backbones_3d.pfe", R + "/models/backbones_3d/pfe")]:
        mg._stub(pkg).__path__ = [path]
    cuda = mg._stub("pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda", ball_query_wrapper=ball_query_wrapper,
                    group_points_wrapper=group_points_wrapper, farthest_point_sampling_wrapper=farthest_point_sampling_wrapper)
    sys.modules["pcdet.ops.pointnet2.pointnet2_stack"].pointnet2_stack_cuda = cuda
    torch.cuda.IntTensor = lambda *s: torch.empty(*s, dtype=torch.int32)
    torch.cuda.FloatTensor = lambda *s: torch.empty(*s, dtype=torch.float64)          # the modules run in float64 here
    return {"modules": importlib.import_module("pcdet.ops.pointnet2.pointnet2_stack.pointnet2_modules"),
            "vsa": importlib.import_module("pcdet.models.backbones_3d.pfe.voxel_set_abstraction"),
            "head": importlib.import_module("pcdet.models.roi_heads.pvrcnn_head")}


def copy_cfg(c):
    return {k: copy_cfg(v) for k, v in c.items()} if isinstance(c, dict) else ([copy_cfg(v) for v in c] if isinstance(c, list) else c)


def load(module, sd):
    missing = module.load_state_dict(sr.torch_state(sd), strict=True)
    return module.double().eval()


def vsa_margin(cfg, inputs, keypoints):
    """pairs within 8 ulps of a radius^2 over every ball query of the forward"""
    B, K = inputs["batch_size"], cfg["NUM_KEYPOINTS"]
    n = 0
    sources = [("raw_points", inputs["points"][:, 1:4], inputs["points"][:, 0])]
    for name, (ind, _) in inputs["levels"].items():
        c = cfg["SA_LAYER"][name]
        sources.append((name, sr.voxel_centers(ind[:, 1:4], c["DOWNSAMPLE_FACTOR"], cfg["VOXEL_SIZE"], cfg["POINT_CLOUD_RANGE"]), ind[:, 0]))
    for name, xyz, bidx in sources:
        cnt = [int((bidx == b).sum()) for b in range(B)]
        for radius in cfg["SA_LAYER"][name]["POOL_RADIUS"]:
            n += sr.near_boundary(radius, xyz, cnt, keypoints[:, 1:4], [K] * B)
    return n


def close(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)
    assert err < 1e-10, (what, err)


def main():
    if not os.path.isdir(R):
        raise SystemExit("the reference checkout is needed to generate vsa.npz")
    ref = import_reference()
    out = {}
    # ---- VoxelSetAbstraction, raw_points and voxel_centers
    seed = sr.VSA_SEED
    inputs = sr.vsa_inputs(seed)
    for tag in ("raw_points", "voxel_centers"):
        cfg = sr.vsa_cfg(tag)
        sd = sr.vsa_state(cfg)
        kp, before, fused = sr.vsa_forward(sr.torch_state(sd), cfg, inputs)
        assert vsa_margin(cfg, inputs, kp) == 0, "pick another VSA_SEED"
        module = ref["vsa"].VoxelSetAbstraction(mv.attr(copy_cfg(cfg)), cfg["VOXEL_SIZE"], cfg["POINT_CLOUD_RANGE"],
                                                num_bev_features=sr.VSA_BEV[0], num_rawpoint_features=4)
        assert module.num_point_features_before_fusion == before.shape[1]
        load(module, sd)
        levels = {k: mv.attr({"indices": torch.from_numpy(i), "features": torch.from_numpy(f).double()})
                  for k, (i, f) in inputs["levels"].items()}
        bd = {"batch_size": 2, "points": torch.from_numpy(inputs["points"]).double(),
              "voxel_coords": torch.from_numpy(inputs["voxel_coords"]), "spatial_features": torch.from_numpy(inputs["bev"]).double(),
              "spatial_features_stride": inputs["bev_stride"], "multi_scale_3d_features": levels}
        with torch.no_grad():
            bd = module(bd)
        assert np.array_equal(bd["point_coords"].numpy().astype(np.float32), kp), "keypoints"
        close(before, bd["point_features_before_fusion"], tag + " before fusion")
        close(fused, bd["point_features"], tag + " fused")
        out["vsa__%s__keypoints" % tag] = kp
        out["vsa__%s__point_features" % tag] = bd["point_features"].numpy()
        if tag == "raw_points":                          # (the other variant differs in the keypoints alone)
            out["vsa__%s__before_fusion" % tag] = bd["point_features_before_fusion"].numpy()
            out["vsa__sd_shapes"] = np.asarray(["%s %s" % (k, tuple(v.shape)) for k, v in sorted(module.state_dict().items())])
    # ---- one StackSAModuleMSG of the reference per served class, against the restatement
    for c_in, c1, c2, ns in sr.SCALE_CLASSES:
        fx = sr.scale_fixture(c_in)
        sd = sr.random_sa_state([[c_in, c1, c2]], 7)
        layer, c_out = ref["modules"].build_local_aggregation_module(
            c_in, mv.attr({"MLPS": [[c1, c2]], "POOL_RADIUS": [fx["radius"]], "NSAMPLE": [ns]}))
        load(layer, sd)
        feats = torch.from_numpy(fx["features"]).double() if c_in else None
        with torch.no_grad():
            _, got = layer(torch.from_numpy(fx["xyz"]).double(), torch.tensor(fx["xyz_cnt"]).int(),
                           torch.from_numpy(fx["new_xyz"]).double(), torch.tensor(fx["new_cnt"]).int(), features=feats)
        want = sr.sa_scale(sr.torch_state(sd), 0, fx["radius"], ns, fx["xyz"], fx["xyz_cnt"], fx["new_xyz"], fx["new_cnt"],
                           torch.from_numpy(fx["features"]) if c_in else None)
        close(want, got, "scale %s" % ((c_in, c1, c2, ns),))
    # ---- PVRCNNHead.roi_grid_pool
    hin = sr.head_inputs(sr.HEAD_SEED)
    cfg = sr.head_cfg()
    pool = cfg["ROI_GRID_POOL"]
    sd = sr.head_pool_state(cfg)
    grid = sr.global_grid_points(hin["rois"], pool["GRID_SIZE"]).reshape(-1, 3)
    cnt = [64, 64]
    for radius in pool["POOL_RADIUS"]:
        assert sr.near_boundary(radius, hin["point_coords"][:, 1:4], cnt, grid, [3 * 216] * 2, ulps=256) == 0, "pick another HEAD_SEED"
    head = ref["head"].PVRCNNHead(32, mv.attr(copy_cfg(cfg)), num_class=1)
    full = {k: v.numpy() for k, v in head.state_dict().items()}
    full.update(sd)
    load(head, full)
    with torch.no_grad():
        got = head.roi_grid_pool({"batch_size": 2, "rois": torch.from_numpy(hin["rois"]),       # (rotate_points_along_z is float32 anyway)
                                  "point_coords": torch.from_numpy(hin["point_coords"]).double(),
                                  "point_features": torch.from_numpy(hin["point_features"]).double(),
                                  "point_cls_scores": torch.from_numpy(hin["point_cls_scores"]).double()})
    want = sr.pvrcnn_grid_pool(sr.torch_state(sd), pool, hin["rois"], hin["point_coords"], hin["point_features"], hin["point_cls_scores"])
    close(want, got, "roi_grid_pool")
    out["head__pooled"] = got.numpy()
    out["head__sd_shapes"] = np.asarray(["%s %s" % (k, tuple(v.shape)) for k, v in sorted(head.state_dict().items())])
    mg.save("vsa.npz", **out)
    print("vsa.npz:", {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    main()
