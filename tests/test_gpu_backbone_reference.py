"""dualfusion.backbones.{SpMiddleResNetFHD, SparseEncoderFusion without a fusion layer, VoxelBackBone8x} on the device
against what the reference's own backbone classes computed (tests/golden/backbone_{cp,tf,vr}.npz, recorded by
tests/golden/make_golden_backbones.py from the reference's modules on its own spconv Python layer and compiled CPU ops).
Same detgen state dict, same voxels (a batch of 3 whose middle sample is empty, voxels on the grid's corners and faces).

Eval, in every arithmetic mode that promises fp32 grade ("fp32", "split", "split3" under `ops.precision`; the bf16 mode stays
with tests/test_gpu_bf16train.py), by the native executor and by the module path (DF3D_EXECUTOR=0):
    every stage's index set (rows sorted by (b, z, y, x)) and spatial_shape exactly; its features and the final map within
    1e-3 of the stage's max |golden| (the parity bar of DESIGN.md section 4).

One training step with loss = (out * c).sum(), same modes -- the bars of test_training_step_gradients_vs_dense_torch
(tests/test_gpu_backbone.py) for the same quantities:
    training-mode output                     max |got - golden| <= 1e-4
    input gradient, parameter gradients      max |got - golden| <= 2e-4 max(1, max |golden|); a gradient of more than 4096
                                             elements through its 8 probe contractions, |<g, r> - golden| <= 2e-4 |g| |r|, and
                                             its L2 norm per kernel offset, <= 2e-4 max(1, max golden norm)
    num_batches_tracked                      exactly
    running_mean / running_var               no bar in that test: the reference's own fp32 step lies D from the dense float64
                                             network of tests/backbone_reference.py (recorded in the golden, `f64dist__*`:
                                             8e-8 .. 9e-8 of the buffer's max); allowed 4 D + 1e-6 of the buffer's max |golden|

Measured on the MI355X, largest over modes and routes (cp / tf / vr; DESIGN.md section 4, "Backbones against the reference's
classes"): eval 6.7e-7 / 9.1e-7 / 8.4e-7 of the stage's max; training output 1.1e-5 / 1.4e-5 / 1.1e-5; input gradient 2.4e-6 /
2.8e-6 / 1.8e-6; parameter gradients 2.7e-5 / 4.0e-6 / 4.6e-6; running_mean 9.7e-8 / 7.2e-8 / 8.1e-8 and running_var 8.1e-8 /
8.3e-8 / 8.2e-8 of the buffer's max against an allowance of 1.3e-6 .. 1.4e-6.  The executor and the module path give the same
bits.  Every test runs in well under a second."""
import os

import numpy as np
import pytest

import backbone_reference as br

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

MODES = ("fp32", "split", "split3")
PARITY = 1e-3
TRAIN_OUT = 1e-4            # test_training_step_gradients_vs_dense_torch
TRAIN_GRAD = 2e-4


def build(tree, g, dev):
    from dualfusion import backbones as bb
    if tree == "cp":
        m = bb.SpMiddleResNetFHD(num_input_features=br.C_IN["cp"])
    elif tree == "tf":
        m = bb.SparseEncoderFusion(**br.TF_KW)
    else:
        m = bb.VoxelBackBone8x({}, br.C_IN["vr"], br.GRID_XYZ)
    shapes = br.shapes_of(g)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == shapes          # the reference module's layout
    m.load_state_dict({k: torch.from_numpy(v) for k, v in br.state(tree, shapes).items()}, strict=True)
    return m.to(dev)


def run(tree, m, feats, coors):
    """-> ({stage: sparse tensor}, output: the dense map, or the last sparse tensor for vr)"""
    if tree == "cp":
        out, ms = m(feats, coors, br.BATCH, br.GRID_XYZ)
        return ms, out
    if tree == "tf":
        out, last, _ = m(feats, coors, br.BATCH, ret_lidar_features=True)
        return {"enc": last}, out
    bd = m({"voxel_features": feats, "voxel_coords": coors, "batch_size": br.BATCH})
    return bd["multi_scale_3d_features"], bd["encoded_spconv_tensor"]


def inputs(tree, g, dev):
    coors = br.voxels(tree)
    assert np.array_equal(coors, g["coors"])
    return torch.from_numpy(br.features(tree, len(coors))).to(dev), torch.from_numpy(coors).to(dev)


@pytest.mark.parametrize("route", ["executor", "modules"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tree", br.TREES)
def test_eval_forward_against_the_reference_module(golden, tree, mode, route):
    from dualfusion import ops
    dev = torch.device("cuda:0")
    g = golden("backbone_%s.npz" % tree)
    m = build(tree, g, dev).eval()
    feats, coors = inputs(tree, g, dev)
    os.environ["DF3D_EXECUTOR"] = "1" if route == "executor" else "0"
    try:
        with torch.no_grad(), ops.precision(mode):
            if route == "executor":
                assert (m._plan() if tree == "cp" else m._runner()) is not None
            stages, out = run(tree, m, feats, coors)
    finally:
        os.environ["DF3D_EXECUTOR"] = "1"
    if tree == "vr":
        stages = dict(stages, out=out)
    assert sorted(stages) == sorted(br.STAGES[tree] + (("out",) if tree == "vr" else ()))
    fig = {}
    for name, t in stages.items():
        ind, f = br.sort_rows(t.indices.cpu().numpy(), t.features.float().cpu().numpy())
        assert [int(v) for v in t.spatial_shape] == g["eval__%s__shape" % name].tolist(), name
        assert np.array_equal(ind, g["eval__%s__indices" % name]), name
        want = g["eval__%s__features" % name]
        fig[name] = float(np.abs(f - want).max() / np.abs(want).max())
    if tree != "vr":
        want = g["eval__dense"]
        got = out.float().cpu().numpy()
        assert got.shape == want.shape
        fig["dense"] = float(np.abs(got - want).max() / np.abs(want).max())
    print("eval %s %s %s: %s" % (tree, mode, route, {k: "%.2e" % v for k, v in fig.items()}))
    assert max(fig.values()) <= PARITY, fig


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tree", br.TREES)
def test_training_step_against_the_reference_module(golden, tree, mode):
    from dualfusion import ops
    dev = torch.device("cuda:0")
    g = golden("backbone_%s.npz" % tree)
    m = build(tree, g, dev).train()
    feats, coors = inputs(tree, g, dev)
    feats.requires_grad_(True)
    cot = br.cotangent(tree, g["train__out"].shape)
    with ops.precision(mode):
        _, out = run(tree, m, feats, coors)
        if tree == "vr":
            order = np.lexsort(tuple(out.indices.cpu().numpy()[:, k] for k in (3, 2, 1, 0)))
            assert np.array_equal(out.indices.cpu().numpy()[order], g["eval__out__indices"])
            out = out.features[torch.from_numpy(order).to(dev)]
        (out * torch.from_numpy(cot).to(dev)).sum().backward()
    fig, bad = {}, []

    def hold(what, err, bound):
        fig[what] = max(fig.get(what, 0.0), err / bound)
        if not err <= bound:
            bad.append("%s: %.3e > %.3e" % (what, err, bound))

    hold("out", float(np.abs(out.detach().float().cpu().numpy() - g["train__out"]).max()), TRAIN_OUT)
    want = g["train__dx"]
    hold("dx", float(np.abs(feats.grad.cpu().numpy() - want).max() / max(1.0, np.abs(want).max())), TRAIN_GRAD)
    raw = {}
    for k, v in m.state_dict().items():
        kind = k.split(".")[-1]
        want = g["train__bn__" + k] if kind in ("running_mean", "running_var", "num_batches_tracked") else None
        if kind == "num_batches_tracked":
            assert int(v) == int(want) == 1, k
        elif want is not None:
            err = float(np.abs(v.cpu().numpy() - want).max() / np.abs(want).max())
            raw[kind] = max(raw.get(kind, 0.0), err)
            hold(kind, err, 4 * float(g["f64dist__" + kind]) + 1e-6)
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        for suffix, rec in br.grad_record(k, p.grad.cpu().numpy()).items():
            want = g["train__dp__" + k + suffix]
            if suffix == "__probes":
                scale = float(g["train__dp__" + k + "__norm"]) * br.probe_norms(k, tuple(p.shape))
                hold("dp probes", float((np.abs(rec - want) / scale).max()), TRAIN_GRAD)
            else:
                hold("dp" + suffix.replace("__", " "), float(np.abs(rec - want).max() / max(1.0, np.abs(want).max())), TRAIN_GRAD)
    print("train %s %s: fraction of the bound %s; running statistics %s of the buffer's max" % (
        tree, mode, {k: "%.3f" % v for k, v in fig.items()}, {k: "%.2e" % v for k, v in raw.items()}))
    assert not bad, bad
