"""Where the arithmetic of a convolution's gradients is decided is pinned without a GPU: the kernel a filter gradient runs on
(df3d_grad_filters_kernel, the choice function of csrc/spconv_bwd.hip) and the plan of the input gradient
(`ops.conv_grad_plan`).  All filter-gradient kernels are fp32-grade or better, so a shape that silently changed kernel would
pass every numerical test."""
import ctypes
import itertools
import os

CHANNELS = (4, 12, 16, 20, 32, 48, 64, 128, 132, 256, 1024)
ROWS = (1000, 16383, 16384)
PLAIN, BF16, SCALED = 0, 1, 2
DIRECT, STAGED, MATRIX1, MATRIX2, MATRIX3, REFUSED = 0, 1, 11, 12, 13, -1


def _lib():
    import __graft_entry__ as ge
    ge._load(os.path.join(ge.PKG, "csrc", "build.py"), "df3d_build").build()
    from dualfusion import _lib
    return _lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False)        # REFUSED (-1) is an answer here


class _Env(object):
    """`with _Env(name, value):` -- the variable set (None: unset) inside, restored on the way out."""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.old = os.environ.get(self.name)
        os.environ.pop(self.name, None)
        if self.value is not None:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        os.environ.pop(self.name, None)
        if self.old is not None:
            os.environ[self.name] = self.old
        return False


def _unscaled_entry(cin, cout, n_out, wgrad):
    """df3d_sparse_conv_grad_filters as it stood before the entries shared a launcher."""
    quads = cin % 4 == 0 and cout % 4 == 0
    wide = (cin >= 128 and cout >= 128 and n_out >= 16384) or cout >= 1024
    choice = int(wgrad) if wgrad is not None else (3 if wide else 1)
    if choice == 3 and quads:
        return MATRIX3
    if choice and quads:
        return STAGED
    return DIRECT if cout <= 128 else REFUSED


def _parent_kernel(form, kvol, cin, cout, n_out, wgrad):
    """The five entries of the parent commit, one branch each."""
    quads = cin % 4 == 0 and cout % 4 == 0
    if kvol == 0:                                   # df3d_rows_grad_weights / _scaled: multiples of 4 or refused; no bf16 entry
        if form == BF16 or not quads:
            return REFUSED
        return MATRIX2 if form == SCALED else MATRIX3
    if form == BF16:                                # DF3D_WGRAD is not read unless the layer is narrow
        if not quads or cin < 64 or cout < 64:
            return _unscaled_entry(cin, cout, n_out, wgrad)
        return MATRIX1
    if form == SCALED:
        if wgrad is not None or not (quads and cin >= 64 and cout >= 64):
            return _unscaled_entry(cin, cout, n_out, wgrad)
        return MATRIX2
    return _unscaled_entry(cin, cout, n_out, wgrad)


# (form, kvol, cin, cout, n_out, DF3D_WGRAD) -> kernel: the layers of the training step and the corners of the rules, by hand
SPOT = {
    (PLAIN, 27, 128, 128, 16384, None): MATRIX3, (PLAIN, 27, 128, 128, 16383, None): STAGED,
    (PLAIN, 27, 64, 64, 16384, None): STAGED, (PLAIN, 9, 64, 1024, 1000, None): MATRIX3,
    (PLAIN, 27, 132, 132, 16384, None): MATRIX3, (PLAIN, 27, 16, 16, 1000, None): STAGED,
    (PLAIN, 27, 16, 16, 1000, "0"): DIRECT, (PLAIN, 27, 16, 16, 1000, "3"): MATRIX3, (PLAIN, 27, 4, 1024, 1000, "0"): REFUSED,
    (PLAIN, 1, 256, 132, 1000, "0"): REFUSED, (PLAIN, 27, 128, 128, 16384, "1"): STAGED, (PLAIN, 27, 4, 128, 1000, "0"): DIRECT,
    (BF16, 27, 64, 64, 1000, None): MATRIX1, (BF16, 27, 64, 64, 1000, "0"): MATRIX1, (BF16, 27, 48, 64, 1000, None): STAGED,
    (BF16, 27, 48, 64, 1000, "0"): DIRECT, (BF16, 27, 32, 256, 16384, "3"): MATRIX3, (BF16, 1, 1024, 1024, 1000, "1"): MATRIX1,
    (SCALED, 27, 64, 64, 1000, None): MATRIX2, (SCALED, 27, 64, 64, 1000, "1"): STAGED, (SCALED, 27, 64, 64, 1000, "3"): MATRIX3,
    (SCALED, 27, 128, 128, 16384, "0"): DIRECT, (SCALED, 27, 32, 32, 16384, None): STAGED,
    (SCALED, 9, 64, 1152, 1000, None): MATRIX2, (SCALED, 27, 48, 1024, 1000, None): MATRIX3,
    (PLAIN, 0, 64, 64, 1000, None): MATRIX3, (PLAIN, 0, 4, 1024, 1000, "0"): MATRIX3, (SCALED, 0, 4, 4, 1000, "1"): MATRIX2,
    (PLAIN, 0, 132, 64, 16384, "1"): MATRIX3, (BF16, 0, 64, 64, 1000, None): REFUSED,
}


def test_filter_gradient_kernel_choice_is_pinned():
    query = _lib().df3d_grad_filters_kernel
    for wgrad in (None, "0", "1", "3"):
        with _Env("DF3D_WGRAD", wgrad):
            for form, kvol, cin, cout, n_out in itertools.product((PLAIN, BF16, SCALED), (0, 1, 27), CHANNELS, CHANNELS, ROWS):
                want = _parent_kernel(form, kvol, cin, cout, n_out, wgrad)
                assert query(form, kvol, cin, cout, n_out) == want, (form, kvol, cin, cout, n_out, wgrad)
            for (form, kvol, cin, cout, n_out, env), want in SPOT.items():
                if env == wgrad:
                    assert _parent_kernel(form, kvol, cin, cout, n_out, env) == want, (form, kvol, cin, cout, n_out, env)
                    assert query(form, kvol, cin, cout, n_out) == want, (form, kvol, cin, cout, n_out, env)
    # channel counts that are no multiples of 4: the direct kernel or nothing
    assert query(PLAIN, 27, 5, 16, 1000) == DIRECT and query(PLAIN, 27, 5, 130, 1000) == REFUSED
    assert query(PLAIN, 0, 5, 16, 1000) == REFUSED and query(SCALED, 0, 16, 130, 1000) == REFUSED
    for bad in ((3, 27, 16, 16, 10), (-1, 27, 16, 16, 10), (PLAIN, 33, 16, 16, 10), (PLAIN, -1, 16, 16, 10), (PLAIN, 27, 0, 16, 10),
                (PLAIN, 27, 16, 0, 10), (PLAIN, 27, 16, 16, -1)):
        assert query(*bad) < 0, bad


# Forward shapes (cin, cout); the input gradient convolves the transposed shape (cout, cin).
SHAPES = ((16, 16), (32, 64), (64, 64), (64, 128), (64, 60), (128, 32), (256, 64), (512, 64), (512, 128))
TRANSPOSE_SERVED = ((32, 64), (64, 64), (64, 128))          # by the two- and three-part formats and by bf16
IN_BLOCKS = ((256, 64), (512, 64), (512, 128))              # transposed shape unserved; (cout, 128) served, cin % 128 == 0
UNSERVED = ((16, 16), (64, 60), (128, 32))                  # (64, 60): cout % 8 != 0 as well; (128, 32): no 32 -> 128 kernel


def _plans(served, in_blocks, unserved):
    out = {}
    for shapes, plan in ((TRANSPOSE_SERVED, served), (IN_BLOCKS, in_blocks), (UNSERVED, unserved)):
        for s in shapes:
            out[s] = plan + (False,)                         # fixed_scale: grouped plans only
    return out


# (mode, amp, DF3D_GRAD_SCALED on) -> {shape: (mode, scaled, blocks, wgrad_bf16, fixed_scale)}
_THREE_PART = _plans(("split3", False, False, False), ("split3", False, True, False), ("split3", False, False, False))
_THREE_PART_AMP = _plans(("bf16", False, False, True), ("split3", False, True, True), ("split3", False, False, True))
_FP32 = _plans(("fp32", False, False, False), ("fp32", False, False, False), ("fp32", False, False, False))
_FP32_AMP = _plans(("bf16", False, False, True), ("fp32", False, False, True), ("fp32", False, False, True))
PLANS = {
    ("split", False, True): _plans(("split", True, False, False), ("split", True, True, False), ("split3", False, False, False)),
    ("split", False, False): _THREE_PART, ("split", True, True): _THREE_PART_AMP, ("split", True, False): _THREE_PART_AMP,
    ("split3", False, True): _THREE_PART, ("split3", False, False): _THREE_PART,
    ("split3", True, True): _THREE_PART_AMP, ("split3", True, False): _THREE_PART_AMP,
    ("bf16", False, True): _FP32, ("bf16", False, False): _FP32, ("bf16", True, True): _FP32_AMP, ("bf16", True, False): _FP32_AMP,
    ("fp32", False, True): _FP32, ("fp32", False, False): _FP32, ("fp32", True, True): _FP32_AMP, ("fp32", True, False): _FP32_AMP,
}
# the CenterPoint head's grouped 64 -> 64 branch convolutions (K = 9): (mode, DF3D_GRAD_SCALED on) -> plan
GROUPED_PLANS = {
    ("split", True): ("split", True, False, False, False), ("split", False): ("split3", False, False, False, False),
    ("split3", True): ("split3", False, False, False, False), ("split3", False): ("split3", False, False, False, False),
    # two-part rows at the forward's fixed activation scale: what the parent did, written down
    ("bf16", True): ("split", False, False, False, True), ("bf16", False): ("split", False, False, False, True),
    ("fp32", True): ("split", False, False, False, True), ("fp32", False): ("split", False, False, False, True),
}


def test_gradient_plan_is_pinned():
    _lib()
    from dualfusion import ops
    assert set(SHAPES) == set(TRANSPOSE_SERVED + IN_BLOCKS + UNSERVED)
    old = ops.CONV_PRECISION
    try:
        for (mode, amp, scaled_on), want in sorted(PLANS.items()):
            ops.CONV_PRECISION = mode
            with _Env("DF3D_GRAD_SCALED", None if scaled_on else "0"):
                assert ops.grad_scaled() == scaled_on
                for kvol, (cin, cout) in itertools.product((27, 9), SHAPES):
                    got = ops.conv_grad_plan(kvol, cin, cout, amp)
                    assert tuple(got) == want[(cin, cout)], (mode, amp, scaled_on, kvol, cin, cout, got)
                    assert ops.CONV_PRECISION == mode
        for (mode, scaled_on), want in sorted(GROUPED_PLANS.items()):
            ops.CONV_PRECISION = mode
            with _Env("DF3D_GRAD_SCALED", None if scaled_on else "0"):
                got = ops.conv_grad_plan(9, 64, 64, False, grouped=True)
                assert tuple(got) == want and got._fields == ("mode", "scaled", "blocks", "wgrad_bf16", "fixed_scale"), (mode, got)
    finally:
        ops.CONV_PRECISION = old


def test_gradient_switches_are_read_in_one_place():
    """DF3D_GRAD_SCALED through `ops.grad_scaled` alone; DF3D_WGRAD_SCALED is gone."""
    import __graft_entry__ as ge
    hits = []
    for dp, _, fs in os.walk(ge.PKG):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert "DF3D_WGRAD_SCALED" not in src, f
                hits += [f] * src.count('"DF3D_GRAD_SCALED"')
    assert hits == ["ops.py"], hits
