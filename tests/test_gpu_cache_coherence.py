"""Every cached weight pack follows the tensors it was built from.

Almost every fast path keeps something derived from module state (packed filters, folded BatchNorm scale / shift,
concatenated weights, executor tables) under a key of its tensors (`dualfusion.derived`).  A key that leaves one tensor
out makes the module compute with old weights after that tensor changes, and a suite that builds a module and runs it once
cannot notice.  The invariant checked here, for a module instance `m` that has already run (caches warm):

    after any supported state change, the next output of `m` equals the output of a FRESH TWIN -- a new instance from the
    same constructor arguments with load_state_dict(m.state_dict(), strict=True), which has never run and has no caches --
    on the same input in the same arithmetic mode.

The twin is the reference; the cached instance is never compared with itself.  The comparison is bit for bit; a path that is
not reproducible run to run gets the noise floor MEASURED inside the test (largest difference between two fresh twins of
identical state; printed) as its bound, and an edit then has to move the twin's output by 100 floors.

Two conditions keep a case from passing vacuously: every compared run must have called the native entries the case names
(`_Names` recorder: no silent plain-torch path) and left the named cache slots behind, and every edit must change the twin's
output unless the tensor is listed in the case's `no_effect` with the reason.

Writes through `.data` bypass the version counters by PyTorch's design and are not supported."""
import os

import numpy as np
import pytest

import detgen

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"

# the library entries that ARE the convolution of a mode (ops.FORMATS / ops.sparse_conv_fused / sparse_conv_grouped)
CONV_ENTRIES = {"split": ("df3d_sparse_conv_split", "df3d_conv_rows_split"), "split3": ("df3d_conv_rows_split3",),
                "bf16": ("df3d_sparse_conv_bf16",), "fp32": ("df3d_sparse_conv_fused_tiled", "df3d_sparse_conv_grouped")}
MODE_CYCLE = ("split", "split3", "bf16", "fp32", "split")


# ------------------------------------------------------------------------------------------------ the harness
class Case(object):
    """One cached module: how to construct it, its deterministic state, its inputs per geometry and how to run it."""
    mode = "split"              # the arithmetic mode the state changes are made in
    modes = ("split", "split3", "bf16", "fp32")
    groups = ("",)              # name prefixes: the one-tensor sweep is one test per prefix (keeps each at a few seconds)
    only = None                 # name prefixes the one-tensor sweep is limited to (None: every floating tensor)
    no_effect = {}              # tensor name -> why an edit cannot move the output
    slots = ()                  # (submodule path, __dict__ key) that a run on the native path leaves behind
    geoms = ("B",)              # the geometries the geometry test visits between two runs of A
    env = {}

    def new(self):
        """A fresh case object for one test: the inputs it builds (device tensors, calibration edited in place) die with it.
        The objects in CASES only parametrize; they never run."""
        return type(self)(*getattr(self, "args", ()))

    def cache_slots(self, mode):
        return self.slots

    def construct(self):
        raise NotImplementedError

    def state(self, shapes):
        return detgen.det_state_dict(shapes)

    def inputs(self, geom):
        raise NotImplementedError

    def enter(self, geom):
        """Called when the geometry test moves to `geom`: for inputs that change IN PLACE (calibration tensors)."""

    def run(self, m, inp):
        raise NotImplementedError

    def entries(self, mode):
        """Groups of entry names; a run must have called at least one name of every group."""
        return (CONV_ENTRIES[mode],)

    # ---- derived
    def fresh(self):
        return self.construct().to(DEV).eval()

    def base(self):
        m = self.construct()
        shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in self.state(shapes).items()}, strict=True)
        return m.to(DEV).eval()

    def twin(self, m):
        t = self.fresh()
        t.load_state_dict(m.state_dict(), strict=True)
        return t

    def cached_input(self, geom):
        cache = self.__dict__.setdefault("_inputs", {})
        if geom not in cache:
            cache[geom] = self.inputs(geom)
        return cache[geom]


def _flat(out):
    """Any nesting of dicts / lists / tuples of tensors -> [detached clones], in a fixed order."""
    if torch.is_tensor(out):
        return [out.detach().clone()]
    if isinstance(out, dict):
        return [t for k in sorted(out) for t in _flat(out[k])]
    if isinstance(out, (list, tuple)):
        return [t for v in out for t in _flat(v)]
    if out is None:
        return []
    raise TypeError(type(out))


def _maxdiff(a, b):
    """Largest |a - b| over two output lists; inf when they differ in structure or hold a NaN on one side only."""
    if len(a) != len(b):
        return float("inf")
    worst = 0.0
    for x, y in zip(a, b):
        if x.shape != y.shape or x.dtype != y.dtype:
            return float("inf")
        if x.numel() == 0 or torch.equal(x, y):
            continue
        d = float((x.double() - y.double()).abs().max())
        worst = max(worst, d if d == d else float("inf"))
    return worst


def _execute(case, m, geom="A"):
    """One recorded run under the case's environment -> (outputs, names of the df3d entries called)."""
    from dualfusion import _lib
    from test_gpu_head_loss_sites import _Names
    real, names = _lib.load(), []
    saved = {k: os.environ.get(k) for k in case.env}
    os.environ.update(case.env)
    _lib._lib = _Names(real, names)
    try:
        with torch.no_grad():
            out = _flat(case.run(m, case.cached_input(geom)))
    finally:
        _lib._lib = real
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return out, names


def _native(case, m, names, mode, who):
    """No vacuous pass: the run called the native entries of the case and left its cache slots behind."""
    for group in case.entries(mode):
        assert any(n in names for n in group), "%s (%s, %s mode): none of %s was called" % (case.name, who, mode, group)
    for path, key in case.cache_slots(mode):
        sub = m.get_submodule(path) if path else m
        assert sub.__dict__.get(key) is not None, "%s (%s, %s mode): cache slot %s.%s is empty after the run" % (
            case.name, who, mode, path, key)


def _pair(case, m, mode, geom="A"):
    """(output of the cached instance, output of its fresh twin), both checked to have run natively."""
    got, names = _execute(case, m, geom)
    _native(case, m, names, mode, "cached instance")
    t = case.twin(m)
    want, names = _execute(case, t, geom)
    _native(case, t, names, mode, "fresh twin")
    return got, want


def _floor(case, m, mode, geom="A"):
    """The noise floor of the path: largest difference between two fresh twins of identical state (0: reproducible)."""
    a, _ = _execute(case, case.twin(m), geom)
    b, _ = _execute(case, case.twin(m), geom)
    fl = _maxdiff(a, b)
    print("noise floor %-22s mode %-6s geometry %s: %.3e" % (case.name, mode, geom, fl))
    assert fl != float("inf")
    return fl


def _delta(t, name):
    """The in-place edit of one tensor: running_var * 1.5, else + a quarter of the mean magnitude (at least 0.1) shaped
    by a ramp over [0.5, 1.5] -- a constant added to a bias in front of a LayerNorm would cancel exactly."""
    if name.endswith("running_var"):
        t.mul_(1.5)
        return
    amp = max(0.1, 0.25 * float(t.detach().abs().mean()))
    ramp = torch.linspace(0.5, 1.5, max(t.numel(), 1), device=t.device, dtype=torch.float64)[:t.numel()]
    t.add_((amp * ramp).to(t.dtype).view(t.shape))


def _floating(m, case, prefix=""):
    out = []
    for k, t in m.state_dict(keep_vars=True).items():
        if not t.is_floating_point() or not k.startswith(prefix):
            continue
        if case.only is not None and not any(k.startswith(p) for p in case.only):
            continue
        out.append((k, t))
    return out


def _judge(case, what, got, want, before, floor, failures, listed=False):
    """The two assertions of every change: cached == twin (within the floor), and the change moved the twin's output."""
    d = _maxdiff(got, want)
    if d > floor:
        failures.append("%s: STALE after %s: max |cached - fresh twin| = %.3e (floor %.1e)" % (case.name, what, d, floor))
    moved = _maxdiff(want, before)
    if listed:
        if moved > 100 * floor:
            failures.append("%s: %s is listed as without effect but moved the output by %.3e" % (case.name, what, moved))
    elif moved == 0 or moved < 100 * floor:
        failures.append("%s: %s had no effect on the fresh twin (moved %.3e, floor %.1e): the edit proves nothing"
                        % (case.name, what, moved, floor))


def _perturbed_state(m):
    """A perturbed copy of the whole state (3 % + 2 % of the mean magnitude; running_var * 1.5): every tensor moves, a deep
    stack stays inside the range of the fp16 operand format."""
    sd = {}
    for k, v in m.state_dict().items():
        v = v.detach().clone()
        if v.is_floating_point():
            v = v * 1.5 if k.endswith("running_var") else v * 1.03 + 0.02 * v.abs().mean()
        sd[k] = v
    return sd


def _synthetic_grads(m):
    g = torch.Generator(device="cpu").manual_seed(11)
    for p in m.parameters():
        p.grad = (torch.randn(p.shape, generator=g) * float(p.detach().abs().mean())).to(p.device, p.dtype)


def _route_load_state_dict(case, m):
    m.load_state_dict(_perturbed_state(m), strict=True)


def _route_sgd(foreach):
    def route(case, m):
        _synthetic_grads(m)
        torch.optim.SGD(list(m.parameters()), lr=0.1, foreach=foreach).step()
    return route


def _route_bucket_adamw(case, m):
    from dualfusion import dist
    reducer = dist.GradBucketReducer(list(m.parameters()))
    opt = dist.BucketAdamW(reducer, lr=2e-3)
    g = torch.Generator(device="cpu").manual_seed(12)
    for b in reducer.buckets:                              # the reduced gradients, as `finish()` leaves them
        b["flat"].copy_(torch.randn(b["flat"].shape, generator=g))
    opt.step()
    reducer.remove()


ROUTES = {"load_state_dict": _route_load_state_dict, "sgd_foreach": _route_sgd(True), "sgd_loop": _route_sgd(False),
          "bucket_adamw": _route_bucket_adamw}


# ------------------------------------------------------------------------------------------------ the cases
class _Neck(Case):
    slots = (("", "_row_plan"),)

    def inputs(self, geom):
        B, H, W = (1, 12, 14) if geom == "A" else (2, 9, 10)
        return torch.from_numpy(detgen.randn("coh_neck_%s" % geom, (B, 32, H, W))).to(DEV)

    def run(self, m, x):
        return m(x)


class RpnCase(_Neck):
    """One layer per block, the narrowest channels the row kernels serve (32 / 64); strides [2, 1] + deconvs x2 keep both
    upsampled maps the same size at 12 x 14 and at 9 x 10; the two deblocks write the concatenated rows in place."""
    name = "RPN"

    def construct(self):
        from dualfusion.necks import RPN
        return RPN(layer_nums=[1, 1], ds_layer_strides=[2, 1], ds_num_filters=[32, 64], us_layer_strides=[2, 2],
                   us_num_filters=[32, 32], num_input_features=32)


class SecondCase(_Neck):
    name = "SECOND"

    def construct(self):
        from dualfusion.necks import SECOND
        return SECOND(in_channels=32, out_channels=[32, 64], layer_nums=[1, 1], layer_strides=[2, 1],
                      conv_cfg=dict(type="Conv2d", bias=True))


class SecondFpnCase(_Neck):
    name = "SECONDFPN"

    def construct(self):
        from dualfusion.necks import SECONDFPN
        return SECONDFPN(in_channels=[32, 64], out_channels=[32, 32], upsample_strides=[2, 2],
                         upsample_cfg=dict(type="deconv", bias=True))

    def inputs(self, geom):
        B, H, W = (1, 6, 7) if geom == "A" else (2, 5, 5)
        return [torch.from_numpy(detgen.randn("coh_fpn_%s_%d" % (geom, c), (B, c, H, W))).to(DEV) for c in (32, 64)]


class SparseSeqCase(Case):
    """SubM conv + BN + ReLU and a strided conv + BN + ReLU, both with the fused epilogue (`fold_batchnorm`,
    `ops.conv_filters`), on ~2 000 clustered voxels."""
    name = "SparseSequential"
    slots = (("0", "_conv_filters"), ("1", "_df3d_fold"), ("3", "_conv_filters"), ("4", "_df3d_fold"))

    def construct(self):
        from torch import nn
        from dualfusion import spconv
        return spconv.SparseSequential(spconv.SubMConv3d(32, 32, 3, bias=True, indice_key="coh0"),
                                       nn.BatchNorm1d(32, eps=1e-3, momentum=0.01), nn.ReLU(),
                                       spconv.SparseConv3d(32, 64, 3, 2, padding=1, bias=True),
                                       nn.BatchNorm1d(64, eps=1e-3, momentum=0.01), nn.ReLU())

    def inputs(self, geom):
        batch, shape, seeds = (1, [16, 48, 48], 22) if geom == "A" else (2, [12, 40, 56], 9)
        ind = detgen.clustered_voxels("coh_seq_%s" % geom, batch, shape, seeds, 120)
        feats = detgen.randn("coh_seq_f_%s" % geom, (len(ind), 32))
        return torch.from_numpy(feats).to(DEV), torch.from_numpy(ind).to(DEV), shape, batch

    def run(self, m, inp):
        from dualfusion import spconv
        feats, ind, shape, batch = inp
        y = m(spconv.SparseConvTensor(feats, ind, shape, batch))
        return [y.features, y.indices]


class CenterHeadCase(Case):
    """The golden mirror head (6 tasks, 36 branches) on a 512-channel map: the dense maps of `forward` (row plan; the fp32
    plan under precision("fp32")), the boxes of `predict_device`, and in the two-part mode the loss-sites path."""
    name = "CenterHead"
    groups = ("shared_conv.",) + tuple("tasks.%d." % t for t in range(6))

    def construct(self):
        from dualfusion.heads import CenterHead
        from make_golden import HEAD_COMMON, HEAD_TASKS
        return CenterHead(in_channels=512, tasks=HEAD_TASKS, dataset='nuscenes', weight=0.25,
                          code_weights=[1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0], common_heads=dict(HEAD_COMMON),
                          share_conv_channel=64, dcn_head=False)

    def state(self, shapes):
        from make_golden import head_bias_shift
        return head_bias_shift(detgen.det_state_dict(shapes))

    def inputs(self, geom):
        from test_gpu_head_loss_sites import _targets, _to_dev
        B, H, W = (1, 12, 14) if geom == "A" else (2, 9, 10)
        x = torch.from_numpy(detgen.randn("coh_head_%s" % geom, (B, 512, H, W))).to(DEV)
        return x, _to_dev(_targets(B, H, W, [1, 2, 2, 1, 2, 2]))

    def entries(self, mode):
        if mode == "fp32":
            return (("df3d_sparse_conv_fused_tiled",), ("df3d_sparse_conv_grouped",), ("df3d_centerhead_predict",))
        if mode == "split3":
            return (("df3d_conv_rows_split3",), ("df3d_centerhead_predict",))
        sites = (("df3d_head_regress_at",), ("df3d_centerhead_loss_slots",)) if mode == "split" else ()
        return (("df3d_conv_rows_split",), ("df3d_head_final_conv_packed", "df3d_head_final_conv"),
                ("df3d_centerhead_predict",)) + sites

    def run(self, m, inp):
        from make_golden import HEAD_TEST_CFG
        from dualfusion import ops
        x, ex = inp
        preds = m(x)
        out = [preds]
        boxes, scores, labels, counts = m.predict_device(preds, HEAD_TEST_CFG)
        live = torch.arange(boxes.shape[1], device=boxes.device)[None, :] < counts[:, None].long()
        out += [counts, torch.where(live[..., None], boxes, torch.zeros((), device=boxes.device)),
                torch.where(live, scores, torch.zeros((), device=boxes.device)),
                torch.where(live, labels, torch.zeros((), dtype=labels.dtype, device=boxes.device))]
        if ops.CONV_PRECISION == "split":
            assert m.loss_sites_wanted(ex) and m.loss_sites_fit(x)
            out.append(m.loss_sites(ex, m.forward_loss_dense(x)))
        return out


class CenterHeadFp32Case(CenterHeadCase):
    """The same head with every state change made under precision("fp32"): the plan of `forward_rows_fp32`
    (`_row_plan_fp32`), swept over the shared conv and the first and the last task."""
    name = "CenterHead-fp32plan"
    mode = "fp32"
    modes = ("fp32",)
    only = groups = ("shared_conv.", "tasks.0.", "tasks.5.")
    slots = (("", "_row_plan_fp32"),)


class TransFusionHeadCase(Case):
    """The device path of the TransFusion head (row-kernel convolutions, proposals, decoder, decode) on the 20 x 20 map of
    the loss golden.  precision("fp32") selects the module's plain-torch path, so the fp32 mode is not one it serves."""
    name = "TransFusionHead"
    modes = ("split", "split3", "bf16")
    groups = ("shared_conv.", "heatmap_head.", "class_encoding.", "decoder.", "prediction_heads.")
    slots = (("", "_row_plan"),)

    def construct(self):
        from make_golden import TFH_KW, TFL_CODER, TFL_LOSSES, TFL_TEST_CFG, TFL_TRAIN_CFG
        from dualfusion.transfusion_head import TransFusionHead
        return TransFusionHead(train_cfg=dict(TFL_TRAIN_CFG), test_cfg=dict(TFL_TEST_CFG), loss_iou=dict(type='VarifocalLoss'),
                               bbox_coder=dict(type='TransFusionBBoxCoder', **TFL_CODER), **TFL_LOSSES, **TFH_KW)

    def state(self, shapes):
        from make_golden import tfh_weight_shift
        return tfh_weight_shift(detgen.det_state_dict(shapes))

    def inputs(self, geom):
        B = 2 if geom == "A" else 1                 # (the map size is a constructor argument of this head: bev_pos)
        return torch.from_numpy(detgen.randn("coh_tfh_%s" % geom, (B, 512, 20, 20))).to(DEV)

    def entries(self, mode):
        conv = ("df3d_conv_rows_split3",) if mode == "split3" else ("df3d_conv_rows_split",)
        return (conv, ("df3d_heatmap_proposals",), ("df3d_cross_attention",), ("df3d_transfusion_decode",))

    def run(self, m, x):
        res = m([x], None, [{}])
        return [res[0][0], m.query_labels, [list(d) for d in m.get_bboxes(res)]]


class BackboneCase(Case):
    """SpMiddleResNetFHD on ~2 000 clustered voxels: the native executor's table (`BackbonePlan._signature`)."""
    name = "SpMiddleResNetFHD-executor"
    only = ("conv_input.", "conv1.")
    env = {"DF3D_EXECUTOR": "1"}

    def construct(self):
        from dualfusion.backbones import SpMiddleResNetFHD
        return SpMiddleResNetFHD(num_input_features=5)

    def inputs(self, geom):
        batch, grid, seeds = (1, [64, 64, 40], 22) if geom == "A" else (2, [80, 48, 40], 9)
        ind = detgen.clustered_voxels("coh_bb_%s" % geom, batch, [41, grid[1], grid[0]], seeds, 120)
        feats = detgen.randn("coh_bb_f_%s" % geom, (len(ind), 5))
        return torch.from_numpy(feats).to(DEV), torch.from_numpy(ind).to(DEV), batch, grid

    def entries(self, mode):
        return (("df3d_backbone_run",),)

    def run(self, m, inp):
        feats, ind, batch, grid = inp
        return [[t.features, t.indices] for t in m._stem(feats, ind, batch, grid)]


class BackboneModulesCase(BackboneCase):
    """The same backbone on the per-module path (`fold_batchnorm`, `ops.conv_filters` of every convolution)."""
    name = "SpMiddleResNetFHD-modules"
    env = {"DF3D_EXECUTOR": "0"}
    slots = (("conv_input.0", "_conv_filters"), ("conv_input.1", "_df3d_fold"), ("conv1.0.bn1", "_df3d_fold"),
             ("conv4.4.conv2", "_conv_filters"))

    def entries(self, mode):
        # (channels <= 16 have no matrix-core kernel: those layers run the exact-fp32 entry in every mode)
        return (("df3d_sparse_conv_fused_tiled",),) + ((CONV_ENTRIES[mode],) if mode != "fp32" else ())


class FusionCpCase(Case):
    """The CenterPoint fusion adapter (VoxelWithPointProjection: image gate, image projection, query assembly, ACTR, write-back)
    on the inputs of tests/golden/fusion_cp.npz: `_folded`, `_wcat`, `_wpack`, `_ffn_i`, `_ffn_p`, `_vcat`,
    `rows_linear_pack`, the calibration cache and the shape caches (`fusion._shape_cache`, `actr._shape_cache`).
    Geometry B is another frame altogether: batch 1 (sample 0 of every voxel set), camera maps of 32 x 48 instead of 40 x 54,
    another `image_shape`, its own calibration tensors.  Geometry C is geometry A seen through calibration matrices that were
    edited IN PLACE (the same tensor objects the calibration cache holds by identity).  The camera list is a constructor
    argument (`image_list`)."""
    name = "CenterPointFusionAdapter"
    modes = ("split", "bf16", "fp32")           # (the adapter's own kernels have no three-part form)
    geoms = ("B", "C")
    slots = (("", "_wcat"), ("", "_wpack"), ("", "_shape_cache"), ("", "_calib_cache"), ("ifat", "_folded"),
             ("pfat", "_vcat"), ("pfat", "_shape_cache"))
    groups = ("ifat.", "pfat.input_proj.", "pfat.i_input_proj.", "pfat.transformer.level_embed",
              "pfat.transformer.encoder.layers.0.", "pfat.transformer.encoder.layers.1.")
    no_effect = {
        "ifat.reduced_dim.1.weight": "the gate reads scales 0 and 2: the reference builds the mixer of scale 1 and never calls it",
        "ifat.reduced_dim.1.bias": "the gate reads scales 0 and 2: the reference builds the mixer of scale 1 and never calls it",
        "pfat.transformer.level_embed": "one image level: the folded image path never forms the level position encoding",
        "pfat.transformer.encoder.layers.1.fusion_layer.a_conv1d.weight":
            "gates the image-query stream of the LAST layer, which the encoder's output drops",
        "pfat.transformer.encoder.layers.1.fusion_layer.a_conv1d.bias":
            "gates the image-query stream of the LAST layer, which the encoder's output drops"}

    def construct(self):
        from dualfusion import fusion as fz, synth
        from make_golden import ACTR_CFG, FUS, FUS_IFAT, FUS_LT
        return fz.VoxelWithPointProjection(fuse_mode='pfat', interpolate=False, voxel_size=FUS["voxel_size"],
                                           pc_range=FUS["pc_range"], image_list=synth.NUSC_CAMS,
                                           image_scale=FUS["image_scale"], depth_thres=FUS["depth_thres"],
                                           pfat_cfg=dict(ACTR_CFG), lt_cfg=dict(FUS_LT), ifat_cfg=dict(FUS_IFAT),
                                           model_name='ACTR')

    def _frame(self, geom):
        """(batch_dict, pristine copies of its calibration) of a geometry.  A and C are ONE set of tensor objects."""
        geom = "A" if geom == "C" else geom
        hit = self.__dict__.setdefault("_frames", {}).get(geom)
        if hit is None:
            from dualfusion import synth
            from make_golden import FUS
            B, (H, W), fhw = (FUS["batch"], FUS["img_hw"], tuple(FUS["feat_hw"])) if geom == "A" else (1, (144, 200), (32, 48))
            cams = synth.nusc_cameras(image_hw=FUS["raw_hw"], focal=FUS["focal"], yaw_offset_deg=FUS["yaw_offset_deg"])
            bd = {'image_shape': {}, 'img_feat': {'layer1_ori_feat2d': {}}, 'calib': {}}
            for n in synth.NUSC_CAMS:
                key = n.lower()
                bd['image_shape'][key] = torch.tensor([[H, W, 3]] * B)
                bd['img_feat']['layer1_ori_feat2d'][key] = torch.from_numpy(
                    detgen.randn("fus_img_%s_%s" % (geom, n) if geom != "A" else "fus_img_" + n, (B, 256) + fhw)).to(DEV)
                T, K = cams[n]
                bd['calib']['lidar2cam_' + key.lstrip('cam_')] = torch.from_numpy(np.stack([T] * B)).to(DEV)
                bd['calib']['cam_intrinsic_' + key.lstrip('cam_')] = torch.from_numpy(np.stack([K] * B)).to(DEV)
            hit = self._frames[geom] = (bd, {k: v.clone() for k, v in bd['calib'].items()})
        return hit

    def inputs(self, geom):
        from make_golden import FUS
        g = self.golden("fusion_cp.npz")
        sets = [g["coords2"].astype(np.int32), g["coords3"].astype(np.int32), g["coords4"].astype(np.int32)]
        feats = [detgen.randn("fus_feat%d" % i, (len(s), c)) for i, (s, c) in enumerate(zip(sets, [32, 64, 128]))]
        B = FUS["batch"]
        if geom == "B":                                              # sample 0 alone
            rows = [s[:, 0] == 0 for s in sets]
            sets, feats, B = [s[r] for s, r in zip(sets, rows)], [f[r] for f, r in zip(feats, rows)], 1
        shapes = [[21, 128, 128], [11, 64, 64], [5, 32, 32]]
        return ([(torch.from_numpy(np.ascontiguousarray(f)).to(DEV), torch.from_numpy(np.ascontiguousarray(i)).to(DEV), shp)
                 for f, i, shp in zip(feats, sets, shapes)], B, self._frame(geom)[0])

    def enter(self, geom):
        bd, original = self._frame("A")
        with torch.no_grad():
            for k, t in bd['calib'].items():
                t.copy_(original[k])
                if geom == "C" and k.startswith("lidar2cam"):
                    t[:, :3, 3] += 0.4                           # the sensor moved: other pixels, other visible voxels

    def entries(self, mode):
        if mode == "fp32":
            return (("df3d_project_voxels",), ("df3d_imgproj_split", "df3d_imgproj_split_compact"),
                    ("df3d_gate_finish_bias", "df3d_gate_finish"), ("df3d_fusion_writeback_split",))
        return (("df3d_imgproj_split", "df3d_imgproj_split_compact"), ("df3d_gate_finish_bias", "df3d_gate_finish"),
                ("df3d_ffn_fused_jobs", "df3d_ffn_fused"), ("df3d_rows_linear",), ("df3d_fusion_writeback_split",))

    def run(self, m, inp):
        from dualfusion import spconv
        levels, B, bd = inp
        batch_dict = {k: (dict(v) if isinstance(v, dict) else v) for k, v in bd.items()}     # a new frame, the same tensors
        xs = [spconv.SparseConvTensor(f, i, shp, B) for f, i, shp in levels]
        out = m(batch_dict, {}, encoded_voxel_list=xs, layer_name='layer1_ori', fuse_mode='pfat', d_factor_list=[2, 4, 8])
        return [out.features, out.indices]


class FusionTfCase(Case):
    """The TransFusion fusion layer (`fusion_tf.ACTRFusionLayer`) on the inputs of tests/golden/tf_fusion.npz: `fusion_tf._wpack`,
    the dual-query layers' `_ffn_i` / `_ffn_p`, `_vcat`, `rows_linear_pack`, `actr._shape_cache`.  Geometry B: batch 1
    (sample 0), camera maps of 32 x 56 instead of 28 x 50 (the layer takes any map of at least input / 4), the golden's
    second calibration with 3-D augmentation records to undo."""
    name = "TransFusionFusionLayer"
    modes = ("split", "bf16", "fp32")
    slots = (("", "_wpack"), ("actr", "_vcat"), ("actr", "_shape_cache"))
    groups = ("actr.input_proj.", "actr.i_input_proj.", "actr.transformer.level_embed", "actr.transformer.encoder.layers.0.",
              "actr.transformer.encoder.layers.1.")
    no_effect = {
        "actr.transformer.level_embed": "one image level: the folded image path never forms the level position encoding",
        "actr.transformer.encoder.layers.1.fusion_layer.a_conv1d.weight":
            "gates the image-query stream of the LAST layer, which the encoder's output drops",
        "actr.transformer.encoder.layers.1.fusion_layer.a_conv1d.bias":
            "gates the image-query stream of the LAST layer, which the encoder's output drops"}

    def construct(self):
        from dualfusion.fusion_tf import ACTRFusionLayer
        from make_golden import ACTR_CFG
        return ACTRFusionLayer(pfat_cfg=dict(ACTR_CFG))

    def inputs(self, geom):
        from make_golden import tff_inputs, tff_metas
        g = self.golden("tf_fusion.npz")
        tag = "plain" if geom == "A" else "aug"
        pts, feats, img = tff_inputs()
        metas = []
        for b, m in enumerate(tff_metas(geom == "B")[0]):
            mm = {k: v for k, v in m.items() if k not in ("sample_idx", "filename")}
            mm["lidar2cam"], mm["cam_intrinsic"] = g[tag + "_lidar2cam"][b], g[tag + "_intrinsic"][b]
            metas.append(mm)
        if geom == "B":
            pts, feats, metas = pts[:1], feats[:len(pts[0])], metas[:1]
            img = detgen.randn("coh_tff_img_B", (6, 256, 32, 56))
        return (torch.from_numpy(img).to(DEV), [torch.from_numpy(p).to(DEV) for p in pts], torch.from_numpy(feats).to(DEV),
                metas)

    def entries(self, mode):
        if mode == "fp32":
            return (("df3d_ms_deform_attn_fused", "df3d_ms_deform_attn_fused_bf16", "df3d_ms_deform_attn_forward"),)
        return (("df3d_imgproj_split", "df3d_imgproj_split_compact"), ("df3d_ffn_fused_jobs", "df3d_ffn_fused"),
                ("df3d_rows_linear",))

    def run(self, m, inp):
        img, pts, feats, metas = inp
        return m([img], pts, feats, metas)


class FusionVrCase(Case):
    """The Voxel-RCNN camera glue of `VoxelBackBone8xFusion` (MVX sum at stride 1, ACTRv2 with a 3-D `LocalTransformer` per
    layer at stride 8) on the inputs of tests/golden/vr_fusion.npz: `_lt_packed`, `_ffn_packed`, `_pe_packed`,
    `ops.packed_linear`, the dual-query layers' packs.  Only the tensors of `actr` are on this path (the sparse convolutions
    of the backbone are the executor cases' subject).  Geometry B: batch 1 (sample 0), camera maps of 20 x 72 instead of
    24 x 80 (they are resampled to the image size), with the augmentation records to undo."""
    modes = ("split", "bf16", "fp32")
    slots = (("actr.transformer", "_level_cache"),)     # (ACTRv2 runs the module composition: no folded image path)

    def __init__(self, name, nsample, lt_entries, lt_slots):
        # 8 neighbours (the golden's LocalTransformer) run the layer on the row kernels (`_ffn_packed`, `packed_linear`);
        # groups of 32 are what the one-kernel layer of csrc/ltlayer.hip serves (`_lt_packed`, `_pe_packed`)
        self.args = (name, nsample, lt_entries, lt_slots)
        self.name, self.nsample, self.lt_entries, self.lt_slots = name, nsample, lt_entries, lt_slots

    def cache_slots(self, mode):
        # (the LocalTransformer's row / fused kernels serve the two-part mode; the other modes take its library path)
        return self.slots + (self.lt_slots if mode == "split" else ())
    only = ("actr.",)
    groups = ("actr.input_proj.", "actr.i_input_proj.", "actr.transformer.level_embed") + \
        tuple("actr.transformer.encoder.%s.%d." % (k, i) for k in ("layers", "lidar_attns") for i in range(4))
    no_effect = {
        "actr.transformer.level_embed": "one image level: the folded image path never forms the level position encoding",
        "actr.transformer.encoder.layers.3.fusion_layer.a_conv1d.weight":
            "gates the image-query stream of the LAST layer, which the encoder's output drops",
        "actr.transformer.encoder.layers.3.fusion_layer.a_conv1d.bias":
            "gates the image-query stream of the LAST layer, which the encoder's output drops"}
    # (this configuration gates before the feed-forward blocks: the image-query block of the last layer is dead as well)
    no_effect.update({"actr.transformer.encoder.layers.3.%s" % k:
                      "feed-forward block of the image-query stream of the LAST layer, which the encoder's output drops"
                      for k in ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm2.weight", "norm2.bias")})

    def construct(self):
        from dualfusion.backbones import VoxelBackBone8xFusion
        from make_golden import VRF
        cfg = dict(NAME='VoxelBackBone8xFusion', USE_IMG=True, FUSION_POS=[1, 4], FUSION_METHOD='MVX+ACTRv2',
                   FEATURE_LEVELS=[0], LT_CFG=dict(VRF["lt"], nsample=self.nsample), ACTR_CFG=dict(VRF["actr"]),
                   HYBRID_CFG=dict(VRF["hybrid"]))
        return VoxelBackBone8xFusion(cfg, 4, [1408, 1600, 40])

    def inputs(self, geom):
        from make_golden import VRF, vrf_inputs
        g = self.golden("vr_fusion.npz")
        ind1, f1, ind4, f4, mvx, img, aug = vrf_inputs()
        B, (H, W) = VRF["batch"], VRF["hw"]
        bd = dict(batch_size=B, lidar2img=torch.from_numpy(g["lidar2img"][:, :3].astype(np.float32)).to(DEV), image_hw=(H, W),
                  img_dict={"mvx_layer1_feat2d": torch.from_numpy(mvx).to(DEV), "layer1_feat2d": torch.from_numpy(img).to(DEV)})
        if geom == "B":
            (ind1, f1), (ind4, f4) = [(i[i[:, 0] == 0], f[i[:, 0] == 0]) for i, f in ((ind1, f1), (ind4, f4))]
            bd.update({k: torch.from_numpy(aug[k][:1]).to(DEV) for k in ("noise_scale", "noise_rot", "flip_x")})
            bd.update(batch_size=1, lidar2img=bd["lidar2img"][:1].contiguous(), img_dict={
                "mvx_layer1_feat2d": torch.from_numpy(detgen.randn("coh_vrf_mvx_B", (1, 16, 20, 72))).to(DEV),
                "layer1_feat2d": torch.from_numpy(detgen.randn("coh_vrf_img_B", (1, 256, 20, 72))).to(DEV)})
            B = 1
        lv = [(torch.from_numpy(np.ascontiguousarray(f)).to(DEV), torch.from_numpy(np.ascontiguousarray(i)).to(DEV))
              for f, i in ((f1, ind1), (f4, ind4))]
        return lv, bd, B

    def entries(self, mode):
        if mode == "fp32":
            return (("df3d_ms_deform_attn_fused", "df3d_ms_deform_attn_fused_bf16", "df3d_ms_deform_attn_forward"),)
        return (self.lt_entries if mode == "split" else ()) + (("df3d_ffn_fused_jobs", "df3d_ffn_fused"),)

    def run(self, m, inp):
        from dualfusion import spconv
        (f1, i1), (f4, i4) = inp[0]
        bd, B = dict(inp[1]), inp[2]
        x1 = spconv.SparseConvTensor(f1, i1, [41, 1600, 1408], B)
        x4 = spconv.SparseConvTensor(f4, i4, [5, 200, 176], B)
        return [m._fuse1(x1, bd).features, m._fuse4(None, None, x4, bd).features]


CASES = [RpnCase(), SecondCase(), SecondFpnCase(), SparseSeqCase(), CenterHeadCase(), CenterHeadFp32Case(),
         TransFusionHeadCase(), BackboneCase(), BackboneModulesCase(), FusionCpCase(), FusionTfCase(),
         FusionVrCase("VoxelRCNN-MVX-ACTRv2-rows", 8, (("df3d_group_attention_split",), ("df3d_ffn_fused",)),
                      tuple(("actr.transformer.encoder.lidar_attns.%d.chunk.layers.%d" % (i, j), "_ffn_packed")
                            for i in (0, 3) for j in (0, 1))),
         FusionVrCase("VoxelRCNN-MVX-ACTRv2-fused", 32, (("df3d_lt_layer_gather",), ("df3d_lt_layer_scatter",)),
                      tuple(("actr.transformer.encoder.lidar_attns.%d.chunk.layers.%d" % (i, j), "_lt_packed")
                            for i in (0, 3) for j in (0, 1))
                      + tuple(("actr.transformer.encoder.lidar_attns.%d" % i, "_pe_packed") for i in (0, 3)))]
_ids = lambda c: c.name if isinstance(c, Case) else str(c)          # noqa: E731


def _warm(case, mode="split"):
    """A base instance that has run (caches warm) and agrees with its twin, the twin's output, the path's noise floor."""
    m = case.base()
    floor = _floor(case, m, mode)
    got, want = _pair(case, m, mode)
    assert _maxdiff(got, want) <= floor, "%s: cached instance and fresh twin differ before any change" % case.name
    return m, want, floor


# ------------------------------------------------------------------------------------------------ 1. one tensor at a time
@pytest.mark.parametrize("case,prefix", [(c, p) for c in CASES for p in c.groups],
                         ids=["%s-%s" % (c.name, p.rstrip(".") or "all") for c in CASES for p in c.groups])
def test_one_tensor_at_a_time(case, prefix, golden):
    """Every floating tensor of state_dict(keep_vars=True), edited in place under no_grad, alone; restored (in place, bit for
    bit) before the next one, so every edit starts from the same state and is judged against the same `before`."""
    from dualfusion import ops
    case = case.new()
    case.golden, failures = golden, []
    with ops.precision(case.mode):
        m, before, floor = _warm(case, case.mode)
        tensors = _floating(m, case, prefix)
        assert tensors, "no floating tensor under %r" % prefix
        assert all(any(k.startswith(p) for p in case.groups) for k, _ in _floating(m, case)), "a tensor outside every group"
        for name, t in tensors:
            saved = t.detach().clone()
            with torch.no_grad():
                _delta(t, name)
            got, want = _pair(case, m, case.mode)
            _judge(case, "an in-place edit of %s" % name, got, want, before, floor, failures, listed=name in case.no_effect)
            with torch.no_grad():
                t.copy_(saved)
            # run the restored state: the restore moved this tensor's version, and the next edit has to meet WARM caches (a
            # rebuild it triggers would hide a key that misses the next tensor); it must give the first output again
            again, _ = _execute(case, m)
            if _maxdiff(again, before) > floor:
                failures.append("%s: STALE after %s was restored" % (case.name, name))
    print("%s %s: %d tensors edited" % (case.name, prefix, len(tensors)))
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ 2. whole-model routes
@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_whole_model_route(case, route, golden):
    """load_state_dict of a perturbed copy, SGD.step() (foreach and the loop) and dist.BucketAdamW.step() with synthetic
    gradients, on an instance whose caches are warm."""
    from dualfusion import ops
    case = case.new()
    case.golden, failures = golden, []
    with ops.precision(case.mode):
        m, before, floor = _warm(case, case.mode)
        ROUTES[route](case, m)
        got, want = _pair(case, m, case.mode)
        _judge(case, route, got, want, before, floor, failures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_double_float_round_trip_then_one_buffer(case, golden):
    """m.double().float() replaces the parameters' storage and the buffer OBJECTS; the values survive it exactly.  The edit
    of one buffer alone afterwards must still be seen (a tensor list collected before the round trip watches dead objects)."""
    from dualfusion import ops
    case = case.new()
    case.golden, failures = golden, []
    with ops.precision(case.mode):
        m, before, floor = _warm(case, case.mode)
        m.double().float()
        got, want = _pair(case, m, case.mode)
        if _maxdiff(got, want) > floor or _maxdiff(want, before) > floor:
            failures.append("%s: output changed over .double().float()" % case.name)
        named = [(k, t) for k, t in _floating(m, case) if k in dict(m.named_buffers()) and k not in case.no_effect]
        if not named:                                               # a module without buffers: one parameter alone
            named = [(k, t) for k, t in _floating(m, case) if k not in case.no_effect][:1]
        name, t = next(((k, t) for k, t in named if k.endswith("running_mean")), named[0])
        with torch.no_grad():
            _delta(t, name)
        got, want = _pair(case, m, case.mode)
        _judge(case, ".double().float() + an edit of %s" % name, got, want, before, floor, failures)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ 3. arithmetic mode
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_arithmetic_mode_cycle(case, golden):
    """split -> split3 -> bf16 -> fp32 -> split on ONE instance (the modes the module serves): every run equals a fresh twin
    run in that mode, and the last split run equals the first."""
    from dualfusion import ops
    case = case.new()
    case.golden = golden
    m = case.base()
    first = None
    for mode in [md for md in (MODE_CYCLE if case.mode == "split" else (case.mode,)) if md in case.modes]:
        with ops.precision(mode):
            floor = _floor(case, m, mode)
            got, want = _pair(case, m, mode)
            d = _maxdiff(got, want)
            assert d <= floor, "%s: STALE in the %s mode: max |cached - fresh twin| = %.3e (floor %.1e)" % (case.name, mode, d, floor)
            if mode == case.mode:
                if first is None:
                    first = got
                else:
                    assert _maxdiff(got, first) <= floor, "%s: the split run after the cycle differs from the first" % case.name


# ------------------------------------------------------------------------------------------------ 4. input geometry
@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_input_geometry_cycle(case, golden):
    """Shape A, then every other geometry of the case (B: another map size and batch; the fusion adapter's C: the calibration
    tensors of A edited in place), then A again: each equals a fresh twin on that geometry and differs from A, and the second A
    equals the first."""
    from dualfusion import ops
    case = case.new()
    case.golden = golden
    with ops.precision(case.mode):
        m, _, floor_a = _warm(case, case.mode)
        first, _ = _execute(case, m, "A")
        for geom in case.geoms:
            case.enter(geom)
            try:
                floor_b = _floor(case, m, case.mode, geom)
                got, want = _pair(case, m, case.mode, geom)
            finally:
                case.enter("A")
            assert _maxdiff(got, want) <= floor_b, "%s: STALE on geometry %s after geometry A" % (case.name, geom)
            assert _maxdiff(got, first) > 100 * floor_b, "%s: geometry %s gave the output of geometry A" % (case.name, geom)
        again, names = _execute(case, m, "A")
        _native(case, m, names, case.mode, "cached instance")
        assert _maxdiff(again, first) <= floor_a, "%s: the second run of geometry A differs from the first" % case.name
