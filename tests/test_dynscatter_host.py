"""Dynamic scatter without a GPU: the C entries are declared, exported and bound; the dynamic encoders are registered with
the reference's parameter names; refusals; and the host reference of tests/dynscatter_reference.py against a brute-force
mask loop."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import dynscatter_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["df3d_dynamic_scatter_plan_workspace_bytes", "df3d_dynamic_scatter_plan", "df3d_dynamic_scatter_reduce",
           "df3d_voxel_to_point", "df3d_dynamic_scatter_max_backward"]


def test_symbols_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge._load(os.path.join(ge.PKG, "csrc", "build.py"), "df3d_build").build()
    from dualfusion import _lib
    header = open(os.path.join(ROOT, "include", "df3d_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, header), s
        assert hasattr(lib, s), s
        assert s in _lib.SIGNATURES, s
    # argument errors are reported without a GPU
    bound = _lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False)
    assert bound.df3d_dynamic_scatter_plan(None, 10, 3, None, None, None, None, None, None, None, 0, None) == -1
    assert bound.df3d_dynamic_scatter_reduce(None, 0, 4, None, None, 3, 7, None, None) == -1
    assert b"reduce" in bound.df3d_last_error()


def test_dynamic_encoders_are_registered():
    from dualfusion import voxel
    from dualfusion.registry import VOXEL_ENCODERS
    assert VOXEL_ENCODERS.get("DynamicSimpleVFE") is voxel.DynamicSimpleVFE
    assert VOXEL_ENCODERS.get("DynamicVFE") is voxel.DynamicVFE
    assert callable(voxel.dynamic_scatter) and issubclass(voxel.DynamicScatter, torch.nn.Module)
    enc = VOXEL_ENCODERS.build(dict(type="DynamicSimpleVFE", voxel_size=(0.2, 0.2, 4), point_cloud_range=(0, -40, -3, 70.4, 40, 1)))
    assert isinstance(enc.scatter, voxel.DynamicScatter) and enc.scatter.average_points is True
    assert repr(enc.scatter) == ("DynamicScatter(voxel_size=(0.2, 0.2, 4), point_cloud_range=(0, -40, -3, 70.4, 40, 1), "
                                 "average_points=True)")


def test_dynamic_vfe_state_dict_keys_are_the_references():
    from dualfusion.voxel import DynamicVFE
    vfe = DynamicVFE(in_channels=4, feat_channels=[16, 32], with_cluster_center=True, with_voxel_center=True)
    assert list(vfe.state_dict().keys()) == [
        "vfe_layers.0.0.weight",
        "vfe_layers.0.1.weight", "vfe_layers.0.1.bias", "vfe_layers.0.1.running_mean", "vfe_layers.0.1.running_var",
        "vfe_layers.0.1.num_batches_tracked",
        "vfe_layers.1.0.weight",
        "vfe_layers.1.1.weight", "vfe_layers.1.1.bias", "vfe_layers.1.1.running_mean", "vfe_layers.1.1.running_var",
        "vfe_layers.1.1.num_batches_tracked",
    ]
    assert tuple(vfe.vfe_layers[0][0].weight.shape) == (16, 10)
    assert tuple(vfe.vfe_layers[1][0].weight.shape) == (32, 32)
    assert vfe.vfe_layers[0][1].eps == 1e-3 and vfe.vfe_layers[0][1].momentum == 0.01
    assert vfe.vfe_scatter.average_points is False and vfe.cluster_scatter.average_points is True
    assert DynamicVFE(feat_channels=[8], mode="avg").vfe_scatter.average_points is True


def test_dynamic_vfe_constructor_refusals():
    from dualfusion.voxel import DynamicVFE
    with pytest.raises(NotImplementedError, match="fusion_layer"):
        DynamicVFE(feat_channels=[16], fusion_layer=dict(type="PointFusion"))
    with pytest.raises(AssertionError):
        DynamicVFE(feat_channels=[])
    with pytest.raises(AssertionError):
        DynamicVFE(feat_channels=[16], mode="sum")


def test_ops_refuse_cpu_tensors():
    from dualfusion import _lib, ops
    from dualfusion.voxel import DynamicScatter, DynamicSimpleVFE
    feats, coors = torch.zeros(6, 4), torch.zeros(6, 3, dtype=torch.int32)
    with pytest.raises(_lib.Df3dError):
        ops.dynamic_scatter_plan(coors)
    with pytest.raises(_lib.Df3dError):
        ops.dynamic_scatter(feats, coors, "mean")
    with pytest.raises(_lib.Df3dError):
        ops.voxel_to_point(feats, coors)
    with pytest.raises(_lib.Df3dError):
        DynamicScatter([0.1, 0.1, 0.1], [0, 0, 0, 1, 1, 1], True)(feats, coors)
    with pytest.raises(_lib.Df3dError):
        DynamicSimpleVFE()(feats, coors)


def test_unknown_reduce_type_is_a_runtime_error():
    from dualfusion import ext, ops
    feats, coors = torch.zeros(6, 4), torch.zeros(6, 3, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="reduce"):
        ops.dynamic_scatter(feats, coors, "min")
    vl = ext.load("voxel_layer")
    with pytest.raises(RuntimeError):
        vl.dynamic_point_to_voxel_forward(feats, coors, "mean")             # CPU tensors
    with pytest.raises(RuntimeError):
        vl.dynamic_point_to_voxel_backward(feats, feats, feats, feats, coors[:, 0], coors[:, 0], "mean")
    with pytest.raises(RuntimeError, match="reduce"):
        ops._reduce_code("median")


def _brute_force(feats, coors, reduce_type):
    """every distinct valid row by a mask over all points, rows sorted as tuples"""
    rows = sorted(set(tuple(int(x) for x in r) for r in coors if min(r) >= 0))
    vf, cnt = [], []
    p2v = np.full((len(coors),), -1, np.int32)
    for v, r in enumerate(rows):
        mask = np.array([tuple(int(x) for x in c) == r for c in coors])
        p2v[mask] = v
        seg = feats[mask].astype(np.float64)
        cnt.append(mask.sum())
        vf.append({"sum": seg.sum(0), "mean": seg.sum(0) / mask.sum(), "max": seg.max(0)}[reduce_type])
    return np.array(vf).reshape(len(rows), feats.shape[1]), np.array(rows, np.int32).reshape(len(rows), coors.shape[1]), \
        p2v, np.array(cnt, np.int32)


@pytest.mark.parametrize("reduce_type", ["sum", "mean", "max"])
def test_host_reference_agrees_with_a_mask_loop(reduce_type):
    rs = np.random.RandomState(3)
    coors = rs.randint(-1, 3, (60, 3)).astype(np.int32)
    coors[5] = (3, -7, 2)
    coors[9] = (-1, 2, 2)
    feats = rs.randint(0, 4, (60, 5)).astype(np.float64)
    vf, vc, p2v, cnt = ref.reduce(feats, coors, reduce_type)
    bf, bc, bp, bn = _brute_force(feats, coors, reduce_type)
    assert np.array_equal(vc, bc) and np.array_equal(p2v, bp) and np.array_equal(cnt, bn)
    assert p2v[5] == -1 and p2v[9] == -1
    np.testing.assert_allclose(vf, bf, rtol=0, atol=1e-12)
    # backward: the gradient of sum_v,c g[v, c] * out[v, c]
    g = rs.standard_normal(vf.shape)
    grad = ref.reduce_backward(g, feats, coors, reduce_type)
    want = np.zeros_like(feats)
    for v in range(len(vc)):
        pts = np.nonzero(p2v == v)[0]
        for c in range(feats.shape[1]):
            if reduce_type == "max":
                want[pts[np.nonzero(feats[pts, c] == bf[v, c])[0][0]], c] = g[v, c]
            else:
                want[pts, c] = g[v, c] / (len(pts) if reduce_type == "mean" else 1)
    assert np.array_equal(grad, want)


def test_host_reference_batched_loop_and_vfe_composition():
    rs = np.random.RandomState(4)
    coors = np.concatenate([np.sort(rs.randint(0, 3, (50, 1)), axis=0), rs.randint(-1, 3, (50, 3))], 1).astype(np.int32)
    feats = rs.uniform(-1, 1, (50, 4))
    vf, vc = ref.batched_loop(feats, coors, "mean")
    wf, wc, _, _ = ref.reduce(feats, coors, "mean")
    assert np.array_equal(vc, wc)
    np.testing.assert_allclose(vf, wf, rtol=0, atol=1e-15)
    torch.manual_seed(0)
    m = ref.DynamicVFERef(4, [16, 32], (0.5, 0.5, 1.0), (0, 0, 0, 2, 2, 2), "max")
    assert [k for k in m.state_dict()][:2] == ["vfe_layers.0.0.weight", "vfe_layers.0.1.weight"]
    out, oc = m(torch.from_numpy(feats), torch.from_numpy(coors))
    assert out.shape == (len(wc), 32) and out.dtype == torch.float64 and np.array_equal(oc.numpy(), wc)
