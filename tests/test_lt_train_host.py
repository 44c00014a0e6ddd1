"""Training of the LocalTransformer (ACTRv2), the parts that need no GPU: the ABI of the attention backward, its argument
contract, and the float64 yardstick of tests/test_gpu_lt_train.py (tests/lt_f64_reference.py) checked against the
reference's golden output and against torch.autograd on the product's own layer."""
import copy
import ctypes
import os
import re

import numpy as np
import torch

import detgen
import lt_f64_reference as ltr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "df3d_group_attention_backward"


def test_group_attention_backward_is_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge._load(os.path.join(ge.PKG, "csrc", "build.py"), "df3d_build").build()
    from dualfusion import _lib
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "df3d_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % SYMBOL, txt)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), SYMBOL)
    assert SYMBOL in _lib.SIGNATURES and len(_lib.SIGNATURES[SYMBOL][1]) == 8
    assert hasattr(_lib.load(), SYMBOL)


def test_group_attention_backward_argument_errors_without_a_gpu():
    from dualfusion import _lib
    lib = _lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False)
    fn = getattr(lib, SYMBOL)
    one = ctypes.c_void_p(16)                                  # a non-null address nobody dereferences: the checks come first
    assert fn(one, one, 32, 4, 4, 8, one, None) == -1 and b"16 channels" in lib.df3d_last_error()
    assert fn(one, one, 512, 4, 4, 16, one, None) == -1 and b"does not fit" in lib.df3d_last_error()
    assert fn(one, one, 32, 4, 4, 16, None, None) == -1 and b"null" in lib.df3d_last_error()
    assert fn(None, None, 32, 0, 4, 16, None, None) == 0       # no groups: nothing to do, empty tensors carry null pointers


def test_float64_yardstick_reproduces_the_reference_golden(golden):
    """lt_f64_reference.local_transformer in float64 on the oracle's geometry against the output the reference's own
    LocalTransformer stored (tests/golden/local_transformer.npz, eval mode), to the atol of
    test_local_transformer_oracle_vs_reference_golden."""
    from make_golden import LT_DIMS, lt_inputs
    from oracle import oracle as orc
    g = golden("local_transformer.npz")
    shapes = {str(k): eval(str(s)) for k, s in zip(g["param_names"], g["param_shapes"])}
    p = {k: torch.from_numpy(v).double() for k, v in detgen.det_state_dict(shapes).items()}
    xyz, feat = lt_inputs()
    d = LT_DIMS
    fps = orc.furthest_point_sample(xyz, d["npoint"])
    new_xyz = np.stack([xyz[b][fps[b]] for b in range(d["B"])])
    idx = orc.ball_query(0.0, d["radius"], d["nsample"], xyz, new_xyz)
    gx = np.stack([xyz[b][idx[b]] for b in range(d["B"])]).transpose(0, 3, 1, 2)               # [B, 3, np, ns]
    rows = torch.from_numpy(np.ascontiguousarray(feat.transpose(0, 2, 1))).double()
    y = ltr.local_transformer(p, idx, torch.from_numpy(np.ascontiguousarray(gx)).double(), rows, 4, d["num_layers"], False)
    np.testing.assert_allclose(y.numpy(), g["out"], atol=2e-5)


def test_float64_yardstick_layer_gradients_equal_autograd_of_the_module():
    """lt_f64_reference.encoder_layer against torch.autograd on TransformerEncoderLayerPreNorm(...).double() on the CPU (the
    module's torch composition: nn.LayerNorm, nn.MultiheadAttention, nn.Linear): output, input gradient and the gradients
    of all 12 parameters to 1e-10 of scale."""
    from dualfusion.pointformer import TransformerEncoderLayerPreNorm
    m = TransformerEncoderLayerPreNorm(64, 4, 128, dropout=0.0).train()
    sd = detgen.det_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.double()
    ours = copy.deepcopy(m)
    L, G = 32, 11
    x = torch.from_numpy(detgen.randn("lth_x", (L, G, 64))).double()
    w = torch.from_numpy(detgen.randn("lth_g", (L, G, 64))).double()
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ya = m(xa)
    yb = ltr.encoder_layer(ltr.module_tensors(ours), xb, 4)
    assert float((ya - yb).detach().abs().max()) <= 1e-10 * float(ya.detach().abs().max())
    (ya * w).sum().backward()
    (yb * w).sum().backward()
    want, got = dict(m.named_parameters()), dict(ours.named_parameters())
    assert len(want) == 12
    for name, a, b in [("input", xa.grad, xb.grad)] + [(k, want[k].grad, got[k].grad) for k in sorted(want)]:
        assert a is not None and b is not None, name
        assert float((a - b).abs().max()) <= 1e-10 * float(a.abs().max()), name
    # the module's own method for the torch composition is what `forward` runs off the GPU
    assert torch.equal(m._forward_torch(x), m(x))
