"""The three sparse backbones against the reference's own backbone classes: what the generator
(tests/golden/make_golden_backbones.py, which runs the reference's modules), the host test and the device test share.

  * the case of every tree -- `voxels`, `features`, `state`, `cotangent`: functions of detgen names, so a golden stores
    recorded results only;
  * how a parameter gradient is recorded (`grad_record`) and how a stage's rows are ordered (`sort_rows`);
  * `dense_f64_step`: the three layer lists once more as a dense float64 network of torch.nn.functional ops
    (tests/spconv_dense_reference.py), training mode.  Nothing is held to it: the generator measures the distance of the
    reference's fp32 training step from it, and that distance is the rounding floor from which the bounds of the quantities
    without an older bar (the BatchNorm running statistics) are derived."""
import numpy as np

import detgen

GRID_XYZ = [48, 48, 40]                       # (x, y, z) as the detectors' configs give it
SPARSE_SHAPE = [41, 48, 48]                   # (z, y, x): grid[::-1] + [1, 0, 0]
BATCH = 3                                     # the middle sample is empty
TREES = ("cp", "tf", "vr")
C_IN = {"cp": 5, "tf": 5, "vr": 4}
BN_EPS, BN_MOMENTUM = 1e-3, 0.01              # (of the dense float64 network; the modules carry their own)
N_PROBES = 8
FULL_NUMEL = 4096

# TransFusion: configs/transfusion_nusc_voxel_L.py `pts_middle_encoder`, sparse_shape reduced to this grid
TF_KW = dict(in_channels=5, sparse_shape=SPARSE_SHAPE, output_channels=128, order=('conv', 'norm', 'act'),
             encoder_channels=((16, 16, 32), (32, 32, 64), (64, 64, 128), (128, 128)),
             encoder_paddings=((0, 0, 1), (0, 0, 1), (0, 0, [0, 1, 1]), (0, 0)), block_type='basicblock')

# weight gains per tree: detgen.det_state_dict draws a [*k, cin, cout] filter with sigma 0.5 / sqrt(k_y k_x cin cout); times
# GAIN sqrt(cout) that is GAIN / (6 sqrt(cin)) per tap, chosen so that every recorded stage lies in [0.1, 100] and at least a
# quarter of its entries survive the ReLU (asserted by the generator)
GAIN = {"cp": 1.5, "tf": 1.5, "vr": 2.0}
SEEDS_WALK = {"cp": (3, 42), "tf": (3, 42), "vr": (3, 42)}      # clustered_voxels(n_seeds per sample, walk)

STAGES = {"cp": ("conv1", "conv2", "conv3", "conv4"), "tf": ("enc",), "vr": ("x_conv1", "x_conv2", "x_conv3", "x_conv4")}


def voxels(tree):
    """[n, 4] (b, z, y, x) int32, distinct, in a shuffled order: random walks in samples 0 and 2 plus the eight corners of
    the voxelised grid (four in each sample) and one voxel in the middle of each of its six faces."""
    D, H, W = GRID_XYZ[2], GRID_XYZ[1], GRID_XYZ[0]
    n_seeds, walk = SEEDS_WALK[tree]
    walks = detgen.clustered_voxels("backbone_" + tree, 2, [D, H, W], n_seeds, walk)
    walks[:, 0] *= 2
    corners = [((0, 2)[i % 2], z, y, x) for i, (z, y, x) in
               enumerate((z, y, x) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1))]
    faces = [(0, 0, H // 2, W // 2), (2, D - 1, H // 2, W // 2), (0, D // 2, 0, W // 2), (2, D // 2, H - 1, W // 2),
             (0, D // 2, H // 2, 0), (2, D // 2, H // 2, W - 1)]
    rows = np.concatenate([walks, np.asarray(corners + faces, np.int32)])
    rows = rows[np.sort(np.unique(rows, axis=0, return_index=True)[1])]
    np.random.RandomState(detgen._seed("backbone_order_" + tree)).shuffle(rows)
    return np.ascontiguousarray(rows, np.int32)


def features(tree, n):
    return detgen.randn("backbone_features_" + tree, (n, C_IN[tree]))


def state(tree, shapes):
    """{name: array} for a state dict of these shapes: detgen.det_state_dict with the tree's gain on the filters"""
    sd = detgen.det_state_dict(shapes)
    for k, v in sd.items():
        if v.ndim >= 2:
            sd[k] = (v * np.float32(GAIN[tree] * np.sqrt(v.shape[-1]))).astype(np.float32)
    return sd


def cotangent(tree, shape):
    return detgen.randn("backbone_cotangent_" + tree, tuple(shape))


def sort_rows(indices, feats):
    o = np.lexsort((indices[:, 3], indices[:, 2], indices[:, 1], indices[:, 0]))
    return np.ascontiguousarray(indices[o]), np.ascontiguousarray(feats[o])


def shapes_of(g):
    """the reference module's state dict layout as the golden stores it -> {name: shape}"""
    out = {}
    for line in g["sd_shapes"]:
        name, shp = str(line).split(" ", 1)
        out[name] = tuple(int(v) for v in shp.strip("(),").replace(",", " ").split())
    return out


def probes(name, shape):
    return [detgen.randn("backbone_probe%d_%s" % (j, name), shape).astype(np.float64) for j in range(N_PROBES)]


def grad_record(name, g):
    """A parameter gradient as the goldens hold it: in full up to 4096 elements, else its contraction with 8 detgen normal
    probes, its L2 norm, and for a filter [*k, cin, cout] the L2 norm per kernel offset.  -> {suffix: array} (float64)"""
    g = np.asarray(g, np.float64)
    if g.size <= FULL_NUMEL:
        return {"": g}
    out = {"__probes": np.asarray([float((g * r).sum()) for r in probes(name, g.shape)]),
           "__norm": np.asarray(np.sqrt((g * g).sum()))}
    if g.ndim == 5:
        out["__offsets"] = np.sqrt((g.reshape(-1, g.shape[3], g.shape[4]) ** 2).sum((1, 2)))
    return out


def probe_norms(name, shape):
    return np.asarray([np.sqrt((r * r).sum()) for r in probes(name, shape)])


# ------------------------------------------------------------------------------------------- dense float64, training mode
class _F64Net(object):
    def __init__(self, sd):
        import torch
        self.P = {k: torch.tensor(np.asarray(v), dtype=torch.float64).requires_grad_(True)
                  for k, v in sd.items() if np.asarray(v).dtype.kind == "f" and not k.split(".")[-1].startswith("running")}
        self.stats = {k: torch.tensor(np.asarray(v), dtype=torch.float64) for k, v in sd.items()
                      if k.split(".")[-1].startswith("running")}

    def conv(self, p, t, stride=None, padding=0):
        import spconv_dense_reference as sdr
        rows, coords, shape = t
        w, b = self.P[p + ".weight"], self.P.get(p + ".bias")
        if stride is None:
            c, s, y = sdr.subm(rows, coords, shape, BATCH, w, b)
        else:
            c, s, y = sdr.conv(rows, coords, shape, BATCH, w, b, stride, padding)
        return y, c, s

    def bn(self, p, t, relu=True):
        import torch
        import torch.nn.functional as F
        y = F.batch_norm(t[0], self.stats[p + ".running_mean"], self.stats[p + ".running_var"], self.P[p + ".weight"],
                         self.P[p + ".bias"], True, BN_MOMENTUM, BN_EPS)
        return (torch.relu(y) if relu else y), t[1], t[2]

    def cbr(self, pc, pb, t, stride=None, padding=0):
        return self.bn(pb, self.conv(pc, t, stride, padding))

    def block(self, p, t):
        import torch
        o = self.cbr(p + ".conv1", p + ".bn1", t)
        o = self.bn(p + ".bn2", self.conv(p + ".conv2", o), relu=False)
        return torch.relu(o[0] + t[0]), o[1], o[2]


def _cp(n, t):
    t = n.cbr("conv_input.0", "conv_input.1", t)
    t = n.block("conv1.1", n.block("conv1.0", t))
    for s, pad in ((2, 1), (3, 1), (4, [0, 1, 1])):
        t = n.cbr("conv%d.0" % s, "conv%d.1" % s, t, 2, pad)
        t = n.block("conv%d.4" % s, n.block("conv%d.3" % s, t))
    return n.cbr("extra_conv.0", "extra_conv.1", t, [2, 1, 1], 0)


def _tf(n, t):
    t = n.cbr("conv_input.0", "conv_input.1", t)
    ch, pads = TF_KW["encoder_channels"], TF_KW["encoder_paddings"]
    for i, blocks in enumerate(ch):
        for j in range(len(blocks)):
            p = "encoder_layers.encoder_layer%d.%d" % (i + 1, j)
            if j == len(blocks) - 1 and i != len(ch) - 1:
                t = n.cbr(p + ".0", p + ".1", t, 2, pads[i][j])
            else:
                t = n.block(p, t)
    return n.cbr("conv_out.0", "conv_out.1", t, [2, 1, 1], 0)


def _vr(n, t):
    t = n.cbr("conv_input.0", "conv_input.1", t)
    t = n.cbr("conv1.0.0", "conv1.0.1", t)
    for s, pad in ((2, 1), (3, 1), (4, [0, 1, 1])):
        t = n.cbr("conv%d.0.0" % s, "conv%d.0.1" % s, t, 2, pad)
        for j in (1, 2):
            t = n.cbr("conv%d.%d.0" % (s, j), "conv%d.%d.1" % (s, j), t)
    return n.cbr("conv_out.0", "conv_out.1", t, [2, 1, 1], 0)


def dense_f64_step(tree, sd, feats, coors, cot):
    """One training step of the tree's layer list in float64 from dense torch ops.  cot: the cotangent of the output (the
    dense map [B, C D, H, W] for cp / tf, the rows of the last sparse tensor in (b, z, y, x) order for vr).
    -> (output, {BatchNorm buffer: value after the step}, d features, {parameter: gradient}), numpy float64."""
    import torch
    import spconv_dense_reference as sdr
    n = _F64Net(sd)
    x = torch.tensor(np.asarray(feats), dtype=torch.float64).requires_grad_(True)
    rows, coords, shape = {"cp": _cp, "tf": _tf, "vr": _vr}[tree](n, (x, torch.tensor(np.asarray(coors), dtype=torch.int64),
                                                                      list(SPARSE_SHAPE)))
    if tree == "vr":
        out = rows                            # (strided outputs come in ascending (b, z, y, x) order)
    else:
        d = sdr.dense(rows, coords, shape, BATCH)
        out = d.reshape(BATCH, d.shape[1] * d.shape[2], d.shape[3], d.shape[4])
    (out * torch.tensor(np.asarray(cot), dtype=torch.float64)).sum().backward()
    return (out.detach().numpy(), {k: v.numpy() for k, v in n.stats.items()}, x.grad.numpy(),
            {k: v.grad.numpy() for k, v in n.P.items()})
