"""The C-ABI library loads (no GPU needed) and exports every symbol include/df3d_hip.h declares;
the Python binding table matches the header."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, "include", "df3d_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(df3d_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    import __graft_entry__ as ge
    ge._load(os.path.join(ge.PKG, "csrc", "build.py"), "df3d_build").build()
    from dualfusion import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    syms = declared_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(lib, s), "libdf3d_hip.so does not export %s" % s
    assert sorted(_lib.SIGNATURES) == syms, set(_lib.SIGNATURES) ^ set(syms)
    assert _lib.load().df3d_version() >= 100


def test_argument_errors_are_reported_without_a_gpu():
    from dualfusion import _lib
    lib = _lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False)
    rc = lib.df3d_sparse_conv_fused(None, 0, 16, None, 27, 16, None, 10, None, None, None, None, 0, None, None)
    assert rc == -1 and b"null" in lib.df3d_last_error()
    assert lib.df3d_hard_voxelize_workspace_bytes(60000, 10, 120000) > 0


def test_product_path_refuses_cpu_tensors():
    import pytest
    import torch
    from dualfusion import _lib, ops
    with pytest.raises(_lib.Df3dError):
        ops.ms_deform_attn_forward(torch.zeros(1, 4, 1, 4), torch.tensor([[2, 2]]), torch.tensor([0]),
                                   torch.zeros(1, 1, 1, 1, 1, 2), torch.zeros(1, 1, 1, 1, 1))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "3d-dual-fusion_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle", src, flags=re.M), f


def test_binding_table_is_read_from_the_header():
    """One prototype per kind the type rule distinguishes, spelled out by hand from include/df3d_hip.h."""
    from ctypes import (c_char_p, c_float, c_int, c_longlong, c_size_t, c_uint, c_ulonglong, c_void_p)
    from dualfusion import _lib
    p, i = c_void_p, c_int
    want = {
        "df3d_device_arch": (i, [c_char_p, i]),                                             # a `char *` out-buffer
        "df3d_last_error": (c_char_p, []),                                                  # a `const char *` return, (void)
        "df3d_grid_bytes": (c_size_t, [i, p]),                                              # a size_t return
        "df3d_lt_layer_packed_bytes": (c_longlong, []),                                     # a long long return
        "df3d_head_worker_create": (p, [i]),                                                # a `void *` return
        "df3d_ball_query": (i, [p, p, i, i, i, c_float, c_float, i, p, p]),                 # float parameters
        "df3d_heatmap_proposals": (i, [p, i, i, i, i, i, i, c_uint, i, p, i, i, p, p, p, p, p, p, p, p, c_size_t, p]),
        "df3d_relu_dropout": (i, [p, c_longlong, c_float, c_ulonglong, p]),                 # an unsigned long long seed
        "df3d_frame_head_submit": (i, [p, p, p, c_size_t, p]),                              # a struct pointer, a `void **`
        "df3d_backbone_geometry": (i, [p, i, p, i, i, i, p, p, c_size_t, p, p, p, p]),      # `size_t *`, `void **`, host int[3]
    }
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, (name, _lib.SIGNATURES[name])
    assert os.path.samefile(_lib.HEADER_PATH, os.path.join(ROOT, "include", "df3d_hip.h"))


def test_header_parser_refuses_what_it_cannot_bind():
    import pytest
    from dualfusion import _lib
    ok = _lib.parse_header("/* c */\n#define X 1\nint df3d_a(const float *x, unsigned n, double y[3]);  // t\nsize_t df3d_b(void);")
    assert ok == {"df3d_a": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p]), "df3d_b": (ctypes.c_size_t, [])}
    for bad, word in (("int df3d_x(short n);", "short n"), ("df3d_layer df3d_x(int n);", "df3d_layer"),
                      ("int df3d_x(df3d_layer by_value);", "df3d_layer by_value"), ("int other(int n);", "other"),
                      ("int df3d_x(int (*callback)(int));", "callback")):
        with pytest.raises(_lib.Df3dError) as e:
            _lib.parse_header(bad)
        assert word in str(e.value) and bad.rstrip(";") in str(e.value), (bad, str(e.value))        # the declaration is named


def test_checked_handle_raises_on_negative_and_passes_values():
    import pytest
    from dualfusion import _lib
    lib = _lib.load()
    with pytest.raises(_lib.Df3dError) as e:
        lib.df3d_sparse_conv_fused(None, 0, 16, None, 27, 16, None, 10, None, None, None, None, 0, None, None)
    assert e.value.rc == -1 and e.value.entry == "df3d_sparse_conv_fused" and "null" in str(e.value)
    assert str(e.value).startswith("df3d_sparse_conv_fused failed (rc=-1): ")
    assert lib.df3d_version() >= 100
    assert lib.df3d_conv_tile_count(0, 64, 128, 27) == 0
    _lib.check(0, "anything")                                   # still there for callers that hold a raw status
    with pytest.raises(_lib.Df3dError):
        _lib.check(-1, "df3d_x")
