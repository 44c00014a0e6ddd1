#!/usr/bin/env python3
"""Generate tests/golden/backbone_{cp,tf,vr}.npz FROM THE REFERENCE ITSELF: the three sparse backbones.

Runs only where the reference checkout and oracle/_ref exist, on the CPU.  The reference's own backbone classes

    CP/det3d/models/backbones/scn.py                        SpMiddleResNetFHD(num_input_features=5)
    TF/mmdet3d/models/middle_encoders/sparse_encoder.py     SparseEncoder as configs/transfusion_nusc_voxel_L.py builds it
                                                            (block_type='basicblock' over TF/mmdet3d/ops/sparse_block.py)
    VR/pcdet/models/backbones_3d/spconv_backbone.py         VoxelBackBone8x(input_channels=4)

run on the reference's own spconv Python layer (TF/mmdet3d/ops/spconv/{conv, modules, structure, functional, ops}.py, imported
under the module name `spconv` and as `mmdet3d.ops.spconv`) over its compiled CPU ops (oracle/_ref/sparse_conv_ext.so, seated
as `spconv.sparse_conv_ext`): SparseConvolution.forward with its output-shape arithmetic and rulebook reuse by indice_key,
SparseSequential, SparseConvTensor.dense() and the autograd Functions all execute.  What is stubbed only satisfies `import`
(registries with a register_module() decorator, `auto_fp16` as an identity decorator, det3d's `dist_common`) or is restated
from a published definition (tests/golden/mmdet_restated.py: mmcv's build_conv_layer / build_norm_layer, mmdet 2.10's
BasicBlock constructor, which the reference's SparseBasicBlock inherits).

The case of every tree (tests/backbone_reference.py): the grid 48 x 48 x 40, a batch of 3 whose middle sample is empty, ~250
voxels with the grid's corners and face centres among them, detgen features and weights.  Recorded: the eval forward (every
stage the class returns, rows sorted by (b, z, y, x), and the final dense map / last sparse tensor) and one training step with
loss = (out * c).sum(): the output, every BatchNorm buffer after the step, the input gradient, every parameter gradient (in
full up to 4096 elements, else 8 probe contractions, its norm and the per-offset norms).  The weights are not stored.

Beside the recorded results every file holds `f64dist__*`: the distance of the reference's fp32 training step from the dense
float64 network of tests/backbone_reference.py (`dense_f64_step`), relative to the quantity's largest magnitude -- the rounding
floor the tests derive the bounds of the BatchNorm running statistics from.

The files are written with fixed zip timestamps: a second run gives the same bytes."""
import contextlib
import importlib
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import make_golden as mg  # noqa: E402  (_stub, Cfg, import_reference_vr_backbone, paths)
import mmdet_restated as mr  # noqa: E402
import backbone_reference as br  # noqa: E402
from oracle import ref  # noqa: E402

REF = "/root/reference"
SPCONV = REF + "/TransFusion/mmdet3d/ops/spconv"
LIMIT = 1000 * 1000


def available():
    return os.path.isdir(SPCONV) and ref.available("sparse_conv_ext")


@contextlib.contextmanager
def clean_modules():
    """sys.modules and sys.path as they were: the stubs of this generator (cv2, torchvision, mmcv, ...)
    do not outlive the block -- a test process that regenerates the cases goes on with its own modules."""
    mods, path = dict(sys.modules), list(sys.path)
    try:
        yield
    finally:
        for k in list(sys.modules):
            if k not in mods:
                del sys.modules[k]
        sys.modules.update(mods)
        sys.path[:] = path


def _mmcv():
    mmcv = mg._stub("mmcv")
    mmcv.cnn = mg._stub("mmcv.cnn", CONV_LAYERS=mr.CONV_LAYERS, build_conv_layer=mr.build_conv_layer,
                        build_norm_layer=mr.build_norm_layer)
    mmcv.runner = mg._stub("mmcv.runner", auto_fp16=lambda *a, **k: (lambda f: f))


def import_spconv():
    """the reference's vendored spconv package under the name `spconv`, its compiled ops pre-seated"""
    _mmcv()
    sys.modules["spconv.sparse_conv_ext"] = ref.load("sparse_conv_ext")
    spec = importlib.util.spec_from_file_location("spconv", SPCONV + "/__init__.py", submodule_search_locations=[SPCONV])
    m = importlib.util.module_from_spec(spec)
    sys.modules["spconv"] = m
    spec.loader.exec_module(m)
    return m


class _Registry(object):
    def register_module(self, *a, **k):
        return a[0] if a and isinstance(a[0], type) else (lambda cls: cls)


def import_cp(sp):
    R = REF + "/CenterPoint/det3d"
    for pkg, path in [("det3d", R), ("det3d.models", R + "/models"), ("det3d.models.backbones", R + "/models/backbones"),
                      ("det3d.models.utils", R + "/models/utils"), ("det3d.utils", R + "/utils"), ("det3d.utils.dist", None)]:
        mg._stub(pkg).__path__ = [path] if path else []
    mg._stub("det3d.models.registry", BACKBONES=_Registry())
    sys.modules["det3d.utils.dist"].dist_common = mg._stub("det3d.utils.dist.dist_common")
    norm = importlib.import_module("det3d.models.utils.norm")                  # the reference's own build_norm_layer
    sys.modules["det3d.models.utils"].build_norm_layer = norm.build_norm_layer
    scn = importlib.import_module("det3d.models.backbones.scn")
    assert scn.spconv is sp
    return scn


def import_tf(sp):
    R = REF + "/TransFusion/mmdet3d"
    for pkg, path in [("mmdet3d", R), ("mmdet3d.ops", R + "/ops"), ("mmdet3d.models", R + "/models"),
                      ("mmdet3d.models.middle_encoders", R + "/models/middle_encoders"), ("mmdet", None), ("mmdet.models", None),
                      ("mmdet.models.backbones", None)]:
        mg._stub(pkg).__path__ = [path] if path else []
    sys.modules["mmdet3d.ops.spconv"] = sys.modules["mmdet3d.ops"].spconv = sp
    mg._stub("mmdet.models.backbones.resnet", BasicBlock=mr.BasicBlock, Bottleneck=mr.Bottleneck)
    blk = importlib.import_module("mmdet3d.ops.sparse_block")
    ops = sys.modules["mmdet3d.ops"]
    ops.SparseBasicBlock, ops.make_sparse_convmodule = blk.SparseBasicBlock, blk.make_sparse_convmodule
    models = sys.modules["mmdet3d.models"]
    models.registry = mg._stub("mmdet3d.models.registry", MIDDLE_ENCODERS=_Registry())
    models.builder = mg._stub("mmdet3d.models.builder")
    return importlib.import_module("mmdet3d.models.middle_encoders.sparse_encoder")


def import_vr(sp):
    bb = mg.import_reference_vr_backbone()[0]
    bb.spconv = sp                                  # (make_golden's stand-in had torch.nn.Module for SparseModule)

    def replace_feature(out, new_features):
        out.features = new_features
        return out

    bb.replace_feature = replace_feature
    return bb


def build(tree):
    """-> (the reference's module, run(module, features, coors) -> (stages {name: sparse tensor}, output))"""
    sp = import_spconv()
    if tree == "cp":
        m = import_cp(sp).SpMiddleResNetFHD(num_input_features=br.C_IN["cp"])

        def run(m, f, c):
            out, ms = m(f, c, br.BATCH, br.GRID_XYZ)
            return ms, out
    elif tree == "tf":
        m = import_tf(sp).SparseEncoder(**br.TF_KW)

        def run(m, f, c):
            keep = []
            hooks = [layer.register_forward_hook(lambda mod, i, o: keep.append(o)) for layer in m.encoder_layers]
            try:
                out = m(f, c, br.BATCH)
            finally:
                for h in hooks:
                    h.remove()
            return {"enc": keep[-1]}, out
    else:
        m = import_vr(sp).VoxelBackBone8x(mg.Cfg(), br.C_IN["vr"], np.asarray(br.GRID_XYZ))

        def run(m, f, c):
            bd = m({"voxel_features": f, "voxel_coords": c, "batch_size": br.BATCH})
            return bd["multi_scale_3d_features"], bd["encoded_spconv_tensor"]
    return m, run


def _rel(a, b, floor=1.0):
    """max |a - b| / max(floor, max |b|): the scale test_training_step_gradients_vs_dense_torch divides by (a conv bias in
    front of a training-mode BatchNorm has a gradient of exactly zero: rounding noise alone, no scale of its own)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), floor))


def generate(tree, with_f64=True):
    """-> {name: array}: the golden of one tree"""
    with clean_modules():
        module, run = build(tree)
        shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
        sd = br.state(tree, shapes)
        module.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
        coors = br.voxels(tree)
        feats = br.features(tree, len(coors))
        out = {"sd_shapes": np.asarray(["%s %s" % (k, shapes[k]) for k in sorted(shapes)]), "coors": coors,
               "note": np.asarray("the reference's own classes on its own spconv Python layer and compiled CPU ops; tf: "
                                  "block_type='basicblock' as configs/transfusion_nusc_voxel_L.py has it")}
        # ---- eval forward
        module.eval()
        with torch.no_grad():
            stages, y = run(module, torch.from_numpy(feats), torch.from_numpy(coors))
        assert tuple(stages) == br.STAGES[tree]
        last = dict(stages)
        if tree == "vr":
            last["out"] = y
            cot_shape = tuple(y.features.shape)
        else:
            out["eval__dense"] = y.numpy()
            cot_shape = tuple(y.shape)
        lively = {}                                      # stage: (max |features|, fraction of non-zero entries)
        for name, t in last.items():
            ind, f = br.sort_rows(t.indices.numpy().astype(np.int32), t.features.numpy())
            lively[name] = (float(np.abs(f).max()), float((f != 0).mean()))
            out["eval__%s__indices" % name], out["eval__%s__features" % name] = ind, f
            out["eval__%s__shape" % name] = np.asarray([int(v) for v in t.spatial_shape], np.int64)
        assert all(0.1 <= top <= 100 and live >= 0.25 for top, live in lively.values()), (tree, lively)
        # ---- one training step
        cot = br.cotangent(tree, cot_shape)
        module.train()
        x = torch.from_numpy(feats).requires_grad_(True)
        _, y = run(module, x, torch.from_numpy(coors))
        if tree == "vr":
            order = np.lexsort(tuple(y.indices.numpy()[:, k] for k in (3, 2, 1, 0)))
            assert np.array_equal(y.indices.numpy()[order], out["eval__out__indices"])
            y = y.features[torch.from_numpy(order)]
        (y * torch.from_numpy(cot)).sum().backward()
        out["train__out"] = y.detach().numpy()
        buffers = {k: v.numpy().copy() for k, v in module.state_dict().items() if k.split(".")[-1] in
                   ("running_mean", "running_var", "num_batches_tracked")}
        for k, v in buffers.items():
            out["train__bn__" + k] = v
        out["train__dx"] = x.grad.numpy()
        grads = {k: p.grad.numpy() for k, p in module.named_parameters()}
        assert sorted(grads) == sorted(k for k in shapes if k not in buffers)
        for k, g in grads.items():
            for suffix, v in br.grad_record(k, g).items():
                out["train__dp__" + k + suffix] = v.astype(np.float32) if suffix == "" else v
        # ---- the reference's fp32 step against dense float64
        if with_f64:
            o64, s64, dx64, g64 = br.dense_f64_step(tree, sd, feats, coors, cot)
            dist = {"out": _rel(out["train__out"], o64), "dx": _rel(out["train__dx"], dx64),
                    "dp": max(_rel(grads[k], g64[k]) for k in grads),
                    "running_mean": max(_rel(buffers[k], s64[k], 1e-300) for k in s64 if k.endswith("running_mean")),
                    "running_var": max(_rel(buffers[k], s64[k], 1e-300) for k in s64 if k.endswith("running_var"))}
            for k, v in dist.items():
                assert v < 1e-4, (tree, k, v)           # the same network: fp32 rounding apart
                out["f64dist__" + k] = np.asarray(v)
    return out


def write(path, arrs):
    """np.savez_compressed with fixed member timestamps"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrs[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def main():
    if not available():
        raise SystemExit("the reference checkout and oracle/_ref are needed to generate the backbone goldens")
    for tree in br.TREES:
        arrs = generate(tree)
        path = os.path.join(HERE, "backbone_%s.npz" % tree)
        write(path, arrs)
        size = os.path.getsize(path)
        print("backbone_%s.npz: %.1f KB, %d voxels, rows %s, f64 distances %s" % (
            tree, size / 1024, len(arrs["coors"]), {k.split("__")[1]: len(v) for k, v in arrs.items() if k.endswith("__indices")},
            {k[9:]: "%.2e" % float(v) for k, v in arrs.items() if k.startswith("f64dist__")}))
        assert size < LIMIT, size


if __name__ == "__main__":
    main()
