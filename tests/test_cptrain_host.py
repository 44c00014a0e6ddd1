"""The float64 reference of the CenterPoint fusion adapter's gradients, checked on its own (CPU only): before
tests/test_gpu_cptrain.py measures `VoxelWithPointProjection.forward_autograd` against it, the differentiable port
(`oracle_models.centerpoint_fusion_torch` in float64, sampling by `f64_reference.msda_core_f64`) has to reproduce the
reference module's recorded output, reach every parameter the configuration reaches, and carry a gradient that is the
derivative of its own values."""
import numpy as np
import torch

import detgen
import f64_reference as fr

UNREACHED = ["ifat.reduced_dim.1.bias", "ifat.reduced_dim.1.weight",
             "pfat.transformer.encoder.layers.1.fusion_layer.a_conv1d.bias",
             "pfat.transformer.encoder.layers.1.fusion_layer.a_conv1d.weight", "pfat.transformer.level_embed"]


def test_float64_port_reproduces_reference_golden(golden):
    """`out` of fusion_cp.npz is the reference module's fp32 output, so what is left against float64 is the reference's own
    rounding: 5.3e-6 absolute measured (output scale 14.57; the fp32 port is at 4.3e-6).  Bound: 2e-5, four times that for
    another host BLAS and a fifth of what the fp32 oracle's golden test allows."""
    case = fr.cp_fusion_case(golden("fusion_cp.npz"))
    got = fr.cp_fusion_gradients(case, torch.float64)["out"].numpy()
    err = float(np.abs(got - case["out"]).max())
    print("float64 port vs golden: max abs %.3g at scale %.4g" % (err, np.abs(case["out"]).max()))
    assert err <= 2e-5, err


def test_float64_port_reaches_every_parameter_the_reference_reaches(golden):
    """No gradient arrives at exactly the five tensors the configuration never reads (the gate's reduction of a scale that
    is not in voxel_idx, the image half of the LAST layer's gate, the level embedding of a single level) and at the
    features of scale 1; every other parameter and the features of scales 0 and 2 take a non-zero one: 68 tensors."""
    case = fr.cp_fusion_case(golden("fusion_cp.npz"))
    ref = fr.cp_fusion_gradients(case, torch.float64)
    assert ref["unreached"] == sorted(UNREACHED + ["leaf1"]), ref["unreached"]
    zero = [k for k, v in ref["grads"].items() if not torch.isfinite(v).all() or float(v.abs().max()) == 0]
    assert not zero, zero
    assert len(ref["grads"]) == 68 and set(ref["grads"]) | set(UNREACHED) == set(case["shapes"]) | {"leaf0", "leaf2"}


def test_float64_port_gradient_is_the_derivative_of_its_values(golden):
    """<grad, direction> over all parameters and both feature leaves (direction: detgen's unit normals) against the central
    difference of the float64 loss `sum(out * w)` along that direction, rectifiers out.  The loss is then smooth up to the
    kinks of bilinear sampling (a sampling point that crosses a line of pixel centres changes slope), and those, not
    rounding, are what a central difference has left: the share of sampling points that cross inside +-h grows with h.
    Measured, relative difference: 1.9e-3 at h = 1e-5, 5.9e-4 at h = 1e-6, 2.4e-10 at h = 1e-7, 4.8e-9 at h = 1e-8 (a
    second, torch-seeded direction: 1.3e-3, 7.4e-4, 3.4e-10, 1.7e-9).  So h = 1e-7: no kink inside the step here, and the
    rounding of the difference stays far away -- the loss (1.7e3, a sum of 5e5 terms of size <= 50) carries ~5e-10 of
    float64 rounding, over 2h that is 3e-3 against a derivative of 7e3, 4e-7 relative.  Bound 2e-4: a branch detached inside
    the port is an error of the size of that branch's share, at any h."""
    case = fr.cp_fusion_case(golden("fusion_cp.npz"))
    grads = fr.cp_fusion_gradients(case, torch.float64, relu=False)["grads"]
    w = torch.from_numpy(case["w"]).double()
    P, feats = fr.cp_fusion_leaves(case, torch.float64)
    leaves = dict(P, **{"leaf%d" % i: f for i, f in enumerate(feats)})
    direction = {k: torch.from_numpy(detgen.randn("fus_dir_" + k, tuple(v.shape))).double() for k, v in leaves.items()}
    analytic = sum(float((g * direction[k]).sum()) for k, g in grads.items())

    def loss(step):
        with torch.no_grad():
            moved = {k: v + step * direction[k] for k, v in leaves.items()}
            out, _ = fr.cp_fusion_port(case, moved, [moved["leaf%d" % i] for i in range(3)], relu=False)
            return float((out * w).sum())

    h = 1e-7
    numeric = (loss(h) - loss(-h)) / (2 * h)
    rel = abs(numeric - analytic) / abs(numeric)
    print("directional derivative: analytic %.9g, central difference %.9g, relative difference %.3g" % (analytic, numeric, rel))
    assert rel <= 2e-4, (analytic, numeric, rel)
