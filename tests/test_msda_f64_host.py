"""The float64 MSDA entries (csrc/msda_f64.hip) as far as a machine without a GPU can check them: the workspace size function is
host-only, and bad arguments are refused before any device call (the contract tests/test_abi.py pins for the other entries)."""
import ctypes


def _lib():
    from dualfusion import _lib
    return _lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False)


def test_workspace_size_is_nonzero_and_monotone():
    lib = _lib()
    small = int(lib.df3d_ms_deform_attn_backward_f64_workspace_bytes(1, 30, 2, 2, 2, 2))
    large = int(lib.df3d_ms_deform_attn_backward_f64_workspace_bytes(2, 2240, 8, 3000, 1, 4))
    assert 0 < small < large
    # at least the ids and their sorting copy (4 bytes each per corner) and three counters per value row
    assert large >= 2 * 4 * (2 * 3000 * 8 * 1 * 4 * 4) + 3 * 4 * (2 * 2240 * 8)
    assert int(lib.df3d_ms_deform_attn_backward_f64_workspace_bytes(2, 2240, 8, 6000, 1, 4)) > large        # more points
    assert int(lib.df3d_ms_deform_attn_backward_f64_workspace_bytes(2, 4480, 8, 3000, 1, 4)) > large        # more rows


def test_a_shape_beyond_the_id_and_counter_types_names_the_limit():
    lib = _lib()
    # 6 x 40 000 x 8 x 4 x 16 x 4 = 4.9e8 x ... contributions: beyond 2^31 - 1
    assert int(lib.df3d_ms_deform_attn_backward_f64_workspace_bytes(64, 1000, 8, 1 << 20, 4, 4)) == 0
    assert b"contributions" in lib.df3d_last_error()
    assert int(lib.df3d_ms_deform_attn_backward_f64_workspace_bytes(1 << 12, 1 << 18, 8, 1, 1, 1)) == 0
    assert b"value rows" in lib.df3d_last_error()


def test_bad_arguments_are_reported_without_a_gpu():
    lib = _lib()
    buf = (ctypes.c_double * 64)()
    idx = (ctypes.c_int64 * 4)(2, 2, 0, 0)
    p, i, null = ctypes.cast(buf, ctypes.c_void_p), ctypes.cast(idx, ctypes.c_void_p), ctypes.c_void_p(0)
    # forward: null value, then D = 0
    assert lib.df3d_ms_deform_attn_forward_f64(null, i, i, p, p, 1, 4, 1, 4, 1, 1, 1, p, null) != 0
    assert b"ms_deform_attn_forward_f64" in lib.df3d_last_error()
    assert lib.df3d_ms_deform_attn_forward_f64(p, i, i, p, p, 1, 4, 1, 0, 1, 1, 1, p, null) != 0
    assert b"ms_deform_attn_forward_f64" in lib.df3d_last_error()
    # backward: null grad_output, null workspace, D = 0, a workspace that is too small
    assert lib.df3d_ms_deform_attn_backward_f64(p, i, i, p, p, null, 1, 4, 1, 4, 1, 1, 1, p, p, p, p, 1 << 20, null) != 0
    assert b"ms_deform_attn_backward_f64" in lib.df3d_last_error()
    assert lib.df3d_ms_deform_attn_backward_f64(p, i, i, p, p, p, 1, 4, 1, 4, 1, 1, 1, p, p, p, null, 1 << 20, null) != 0
    assert b"ms_deform_attn_backward_f64" in lib.df3d_last_error()
    assert lib.df3d_ms_deform_attn_backward_f64(p, i, i, p, p, p, 1, 4, 1, 0, 1, 1, 1, p, p, p, p, 1 << 20, null) != 0
    assert b"ms_deform_attn_backward_f64" in lib.df3d_last_error()
    assert lib.df3d_ms_deform_attn_backward_f64(p, i, i, p, p, p, 1, 4, 1, 4, 1, 1, 1, p, p, p, p, 16, null) != 0
    assert b"workspace" in lib.df3d_last_error()
