"""The layer lists of the three sparse backbones against the reference's own backbone classes (CPU suite).

tests/golden/backbone_{cp,tf,vr}.npz hold what the reference's SpMiddleResNetFHD, SparseEncoder (block_type='basicblock')
and VoxelBackBone8x computed on the reference's own spconv Python layer and compiled CPU ops
(tests/golden/make_golden_backbones.py).  Here:

  * the restatements every device test of the backbones compares with -- oracle_models.centerpoint_backbone /
    transfusion_encoder / voxel_backbone8x -- run on the golden's inputs and must reproduce the recorded eval forward: index
    sets and spatial shapes exactly, features within 2e-5 of the stage's max |golden| (the bound tests/test_oracle_golden.py
    holds oracle == golden floats to).  A stride, a padding, an eps, a bias or an order of operations stated wrongly there no
    longer passes, so a device test against these compositions is a test against the reference's modules;
  * the goldens are lively (every stage within [0.1, 100], a quarter of its entries non-zero) and below the size limit;
  * the dense float64 network of tests/backbone_reference.py stays at the recorded distance from the reference's training
    step (the rounding floor DESIGN.md section 4 derives the running-statistics bound from);
  * where the reference checkout and oracle/_ref are present: the three cases regenerated in memory equal the committed files
    -- integers bit for bit, floats within 1e-6 of their scale (the CPU thread count can reorder torch.mm).  Skipped elsewhere.

Measured (max |restatement - golden| / max |golden| over the stages): cp 2.9e-7, tf 3.1e-7, vr 3.4e-7.  Each of these,
changed alone in oracle_models.py, fails the first test: the last strided layer's padding [0,1,1] -> [1,1,1] (cp, vr; the
TransFusion paddings come from the config), BN eps 1e-3 -> 1e-5 (all), the residual add dropped (cp, tf), the ReLU in front
of the add (cp, tf), the output layer's stride (2,1,1) -> (1,1,1) (all), the CenterPoint block convs' bias dropped (cp)."""
import os

import numpy as np
import pytest

import backbone_reference as br
import oracle_models as om

FLOAT_BOUND = 2e-5          # tests/test_oracle_golden.py: oracle == golden floats
REGEN_BOUND = 1e-6


def _inputs(g, tree):
    coors = br.voxels(tree)
    assert np.array_equal(coors, g["coors"])
    assert set(coors[:, 0]) == {0, 2}                                          # the middle sample is empty
    return br.state(tree, br.shapes_of(g)), br.features(tree, len(coors)), coors


def _restatement(tree, sd, feats, coors):
    """-> ({stage: (indices, features, shape)}, dense map or None)"""
    if tree == "cp":
        dense, ms = om.centerpoint_backbone(sd, feats, coors, br.BATCH, br.GRID_XYZ)
    elif tree == "tf":
        dense, last = om.transfusion_encoder(sd, feats, coors, br.BATCH, br.SPARSE_SHAPE, br.TF_KW["encoder_channels"],
                                             br.TF_KW["encoder_paddings"])
        ms = {"enc": last}
    else:
        out, ms = om.voxel_backbone8x(sd, feats, coors, br.BATCH, br.SPARSE_SHAPE)
        ms, dense = dict(ms, out=out), None
    return {k: (t.indices, t.features, t.shape) for k, t in ms.items()}, dense


@pytest.mark.parametrize("tree", br.TREES)
def test_restatement_reproduces_the_reference_module(golden, tree):
    g = golden("backbone_%s.npz" % tree)
    stages, dense = _restatement(tree, *_inputs(g, tree))
    names = br.STAGES[tree] + (("out",) if tree == "vr" else ())
    assert sorted(stages) == sorted(names)
    worst = 0.0
    for name in names:
        ind, f = br.sort_rows(np.asarray(stages[name][0]), np.asarray(stages[name][1]))
        assert [int(v) for v in stages[name][2]] == g["eval__%s__shape" % name].tolist(), name
        assert np.array_equal(ind, g["eval__%s__indices" % name]), name
        want = g["eval__%s__features" % name]
        err = float(np.abs(f - want).max() / np.abs(want).max())
        worst = max(worst, err)
        assert err <= FLOAT_BOUND, (tree, name, err)
    if dense is not None:
        want = g["eval__dense"]
        assert dense.shape == want.shape
        err = float(np.abs(dense - want).max() / np.abs(want).max())
        worst = max(worst, err)
        assert err <= FLOAT_BOUND, (tree, "dense", err)
    print("%s: restatement within %.2e of the reference module" % (tree, worst))


@pytest.mark.parametrize("tree", br.TREES)
def test_goldens_are_lively_and_small(golden, tree):
    g = golden("backbone_%s.npz" % tree)
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backbone_%s.npz" % tree)) < 1000 * 1000
    for k in g.files:
        if k.endswith("__features"):
            f = g[k]
            assert 0.1 <= np.abs(f).max() <= 100 and (f != 0).mean() >= 0.25, k
        if k.endswith("num_batches_tracked"):
            assert int(g[k]) == 1, k
    W, H, D = br.GRID_XYZ
    for corner in [(z, y, x) for z in (0, D - 1) for y in (0, H - 1) for x in (0, W - 1)]:      # the voxelised grid's corners
        assert (g["coors"][:, 1:] == np.asarray(corner)).all(1).any(), corner


@pytest.mark.parametrize("tree", br.TREES)
def test_dense_float64_network_stays_at_the_recorded_distance(golden, tree):
    """The training half of the golden, on any machine: the float64 network of dense torch ops gives the recorded output,
    running statistics, input gradient and parameter gradients to within the distance the generator measured (4 x, plus 1e-6
    of scale for a different thread count)."""
    g = golden("backbone_%s.npz" % tree)
    sd, feats, coors = _inputs(g, tree)
    out, stats, dx, grads = br.dense_f64_step(tree, sd, feats, coors, br.cotangent(tree, g["train__out"].shape))

    def close(got, want, what, dist, floor):
        err = float(np.abs(np.asarray(want, np.float64) - got).max() / max(float(np.abs(got).max()), floor))
        assert err <= 4 * float(g["f64dist__" + dist]) + 1e-6, (tree, what, err)

    close(out, g["train__out"], "out", "out", 1.0)
    close(dx, g["train__dx"], "dx", "dx", 1.0)
    for k, v in stats.items():
        close(v, g["train__bn__" + k], k, k.split(".")[-1], 1e-300)
    for k, v in grads.items():
        for suffix, rec in br.grad_record(k, v).items():
            want = g["train__dp__" + k + suffix]
            if suffix == "__probes":
                err = float(np.abs(rec - want).max() / (float(g["train__dp__" + k + "__norm"]) * br.probe_norms(k, v.shape).min()))
                assert err <= 4 * float(g["f64dist__dp"]) + 1e-6, (tree, k, suffix, err)
            else:
                close(rec, want, k + suffix, "dp", 1.0)


def _generator():
    import make_golden_backbones as mb
    return mb


def _reference_present():
    return os.path.isdir("/root/reference/TransFusion/mmdet3d/ops/spconv") and \
        os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref", "sparse_conv_ext.so"))


@pytest.mark.skipif(not _reference_present(), reason="needs the reference checkout and oracle/_ref")
@pytest.mark.parametrize("tree", br.TREES)
def test_committed_golden_is_what_the_reference_computes(golden, tree):
    g = golden("backbone_%s.npz" % tree)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        new = _generator().generate(tree, with_f64=False)
    assert sorted(k for k in g.files if not k.startswith("f64dist__")) == sorted(new)
    for k, v in new.items():
        v, old = np.asarray(v), g[k]
        assert v.shape == old.shape and v.dtype == old.dtype, k
        if v.dtype.kind in "fc":
            scale = max(float(np.abs(old).max()), 1.0 if k.startswith("train__dp__") else 1e-300)
            assert float(np.abs(v - old).max()) <= REGEN_BOUND * scale, k
        else:
            assert np.array_equal(v, old), k
