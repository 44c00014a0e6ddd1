"""Which instantiation a matrix-core convolution runs on is pinned without a GPU: df3d_conv_launch_plan (the function the five
launchers of csrc/spconv_split.hip take their decision from) against a restatement of the rules, at every threshold and one row
below it; the set of plans a scan over the row counts reaches, written out per (format, shape); and, from the same scan, the
smallest row count that selects each plan -- `plan_runs`, where tests/test_gpu_conv_configs.py takes its row counts from.  All
kernels of the family are fp32-grade, so a threshold that moved would pass every numerical test and only leave a configuration
without one.  num_cu = 256 throughout: the answer needs no device."""
import ctypes
import functools
import itertools
import os

NUM_CU = 256
SCAN_ROWS = 60000
FIELDS = ("family", "rt", "nw", "kps", "ks", "masked", "cbw", "tile_rows")
PARTS = {"bf16": 1, "split": 2, "split3": 3}
OS, WIDE = "os", "wide"
# DF3D_CONV_SHAPES of csrc/spconv_split.hip: (cin, cout) -> (launch family of the two-part format, served by bf16)
SHAPES = {
    (256, 256): (WIDE, True), (256, 128): (WIDE, True), (128, 256): (WIDE, True), (512, 64): (WIDE, False),
    (512, 128): (WIDE, False), (128, 32): (OS, False), (128, 64): (OS, True), (128, 128): (OS, True), (64, 128): (OS, True),
    (64, 64): (OS, True), (32, 64): (OS, True), (64, 32): (OS, True), (32, 32): (OS, True),
}
TUNING_AIDS = ("DF3D_OS_CFG", "DF3D_OS_WIDE", "DF3D_LC_CBW")        # read once per process: must be unset here
SWITCHES = ("DF3D_OS_LC", "DF3D_OS_KSPLIT", "DF3D_OS_MASKED")       # read per call


def served(kind):
    return [s for s in SHAPES if kind != "bf16" or SHAPES[s][1]]


# the plans, as the record of df3d_conv_launch_plan: (family, RT, NW, KPS, KS, masked, cbw, tile rows)
OS2, OS4, OS8 = (0, 1, 2, 1, 1, 0, 0, 32), (0, 1, 4, 1, 1, 0, 0, 64), (0, 1, 8, 1, 1, 0, 0, 128)
OS8_MASKED = (0, 1, 8, 1, 1, 1, 0, 128)
OS4_KS3 = (0, 1, 4, 1, 3, 0, 0, 64)
LC1, LC2 = (1, 2, 4, 1, 1, 0, 1, 128), (1, 2, 4, 1, 1, 0, 2, 128)


def _cdiv(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def _lib_handle():
    import __graft_entry__ as ge
    ge._load(os.path.join(ge.PKG, "csrc", "build.py"), "df3d_build").build()
    from dualfusion import _lib
    return _lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False)        # a negative status is an answer here


def assert_default_environment():
    """The plans of this file are the defaults: no tuning aid, no A/B switch."""
    for name in TUNING_AIDS + SWITCHES:
        assert name not in os.environ, "%s is set: the launch plans pinned here are the defaults" % name


@functools.lru_cache(maxsize=None)
def _query():
    fn = _lib_handle().df3d_conv_launch_plan
    rec = (ctypes.c_int * len(FIELDS))()

    def query(kind, kvol, cin, cout, groups, n_out, compact_cols=0, num_cu=NUM_CU):
        """-> the plan record as a tuple, or the negative status"""
        rc = fn(PARTS[kind], kvol, cin, cout, groups, n_out, compact_cols, num_cu, rec)
        return tuple(rec) if rc == 0 else rc
    return query


# ---- the rules, restated ---------------------------------------------------------------------------------------------------
def _lc_plan(n_out, gy, ncu):
    """Column blocks per workgroup of the loader / consumer kernel: the number ny of workgroups per row tile with the fewest
    (rounds over the CUs) x (blocks walked + half a block of prologue and drain); the first ny wins a tie."""
    tiles = _cdiv(n_out, 128)
    best_ny = min(range(1, gy + 1), key=lambda ny: (_cdiv(tiles * ny, ncu) * (2 * _cdiv(gy, ny) + 1), ny))
    return (1, 2, 4, 1, 1, 0, _cdiv(gy, best_ny), 128)


def _os(nw, ks=1, masked=0):
    return (0, 1, nw, 1, ks, masked, 0, 16 * nw)


def restated_plan(kind, kvol, cin, cout, groups, n_out, compact_cols=0, ncu=NUM_CU):
    fam = SHAPES[(cin, cout)][0]
    gy = groups * (cout // 128 if cout > 128 else 1)
    work = n_out * gy
    if kind == "bf16":
        return _os(8 if work >= 16384 else 2)
    if kind == "split3":
        return _os(8 if work >= 32768 else 4 if work >= 12288 else 2)
    lc = not compact_cols and kvol > 1 and _cdiv(n_out, 128) * gy >= 190
    if fam == OS:
        if cout == 128 and lc:
            return _lc_plan(n_out, gy, ncu)
        if n_out < 16384:
            return _os(2)
        return _os(8, masked=int(kvol == 27 and cin == 32 and not compact_cols))
    if cout % 128 == 0 and lc:
        return _lc_plan(n_out, gy, ncu)
    nw = 8 if work >= 49152 else 4 if work >= 12288 else 2
    if cin <= 256 and cout % 128 == 0 and nw == 4 and kvol >= 3 and _cdiv(n_out, 64) * gy * 4 <= 6 * ncu:
        return _os(4, ks=3)
    return _os(nw)


def _threshold_rows(gy):
    """Every row count at which a rule of restated_plan changes its answer for gridDim.y = gy (the first row count on the far
    side), for each the row below, and the small counts around the 32- and 128-row tiles."""
    firsts = {_cdiv(t, gy) for t in (12288, 16384, 32768, 49152)} | {16384}
    firsts.add(128 * (_cdiv(190, gy) - 1) + 1)                       # loader / consumer from 190 workgroups on
    firsts.add(64 * (6 * NUM_CU // (4 * gy)) + 1)                    # three wave groups up to 6 waves per CU
    firsts |= {128 * t + 1 for t in range(1, _cdiv(SCAN_ROWS, 128))}  # (its column blocks per workgroup change at tile counts)
    rows = {1, 31, 32, 33, 127, 128, 129}
    for f in firsts:
        rows |= {f - 1, f}
    return sorted(r for r in rows if r >= 1)


def test_launch_plan_equals_the_restated_rules_at_every_threshold():
    assert_default_environment()
    query = _query()
    seen = set()
    for kind in PARTS:
        for (cin, cout), kvol, groups in itertools.product(served(kind), (1, 4, 9, 27), (1, 6)):
            gy = groups * (cout // 128 if cout > 128 else 1)
            for n_out in _threshold_rows(gy):
                want = restated_plan(kind, kvol, cin, cout, groups, n_out)
                got = query(kind, kvol, cin, cout, groups, n_out)
                assert got == want, (kind, kvol, cin, cout, groups, n_out, got, want)
                assert got[7] == (128 if got[0] else 16 * got[1] * got[2])
                seen.add(got)
            if cout == 32:                                           # compact output columns: no masked gathers
                for n_out in (1, 16383, 16384, 30000):
                    want = restated_plan(kind, kvol, cin, cout, groups, n_out, compact_cols=1)
                    assert query(kind, kvol, cin, cout, groups, n_out, 1) == want and not want[5]
    assert {OS2, OS4, OS8, OS8_MASKED, OS4_KS3, LC1, LC2} <= seen
    # what no format serves, and arguments the entries refuse
    assert query("bf16", 27, 512, 64, 1, 1000) < 0 and query("bf16", 27, 128, 32, 1, 1000) < 0
    for bad in (("split", 27, 16, 16, 1, 1000), ("split", 27, 32, 128, 1, 1000), ("split3", 0, 64, 64, 1, 1000),
                ("split", 33, 64, 64, 1, 1000), ("split", 27, 64, 64, 0, 1000), ("split", 27, 64, 64, 1, 0),
                ("split", 27, 64, 64, 1, 1000, 1), ("split", 27, 64, 64, 1, 1000, 0, -1)):
        assert query(*bad) < 0, bad
    fn = _lib_handle().df3d_conv_launch_plan
    assert fn(0, 27, 64, 64, 1, 1000, 0, NUM_CU, (ctypes.c_int * 8)()) < 0 and fn(4, 27, 64, 64, 1, 1000, 0, NUM_CU, (ctypes.c_int * 8)()) < 0
    assert fn(2, 27, 64, 64, 1, 1000, 0, NUM_CU, None) < 0


def test_per_call_switches_reach_the_plan():
    """DF3D_OS_LC, DF3D_OS_KSPLIT and DF3D_OS_MASKED are read per call by the query as by the launchers."""
    assert_default_environment()
    query = _query()
    try:
        os.environ["DF3D_OS_LC"] = "1"
        assert query("split", 27, 128, 128, 1, 5) == LC1 and query("split", 1, 256, 256, 1, 5)[0] == 1
        assert query("split", 27, 32, 32, 1, 5, 1) == OS2                # compact columns: never
        assert query("split", 27, 64, 64, 1, 5) == OS2 and query("split3", 27, 128, 128, 1, 5) == OS2
        os.environ["DF3D_OS_LC"] = "0"
        assert query("split", 27, 128, 128, 1, 30000) == OS8 and query("split", 9, 256, 256, 1, 30000) == OS8
        # the upper end of the three wave groups (6 waves per CU) lies behind the loader / consumer kernel's 190 workgroups on
        # 256 CUs: without that kernel, and on a smaller device, it is the rule that decides
        assert query("split", 9, 256, 256, 1, 12288) == OS4_KS3 and query("split", 9, 256, 256, 1, 12289) == OS4
        assert query("split", 9, 256, 128, 1, 24576) == OS4_KS3 and query("split", 9, 256, 128, 1, 24577) == OS4
        os.environ.pop("DF3D_OS_LC")
        assert query("split", 9, 256, 256, 1, 6144, 0, 128) == OS4_KS3 and query("split", 9, 256, 256, 1, 6145, 0, 128) == OS4
        assert query("split", 9, 256, 256, 1, 12033, 0, 128) == LC2 and query("split", 9, 256, 256, 1, 12033) == LC1
        assert query("split", 9, 256, 256, 1, 8000) == OS4_KS3
        os.environ["DF3D_OS_KSPLIT"] = "0"
        assert query("split", 9, 256, 256, 1, 8000) == OS4
        os.environ.pop("DF3D_OS_KSPLIT")
        os.environ["DF3D_OS_MASKED"] = "1"
        assert query("split", 27, 64, 64, 1, 20000) == OS8_MASKED and query("split", 27, 64, 64, 1, 20) == OS2
        os.environ["DF3D_OS_MASKED"] = "0"
        assert query("split", 27, 32, 32, 1, 20000) == OS8
    finally:
        for name in SWITCHES:
            os.environ.pop(name, None)
    assert query("split", 27, 32, 32, 1, 20000) == OS8_MASKED


def test_ops_wrapper_names_the_record():
    assert_default_environment()
    _lib_handle()
    from dualfusion import _lib as binding, ops
    assert ops.ConvLaunchPlan._fields == FIELDS and ops.CONV_PLAN_FIELDS == len(FIELDS)
    got = ops.conv_launch_plan("split", 9, 256, 256, 13000, num_cu=NUM_CU)
    assert got == ("lc", 2, 4, 1, 1, False, 1, 128) and got.family == "lc" and got.tile_rows == 128
    assert ops.conv_launch_plan("split", 27, 32, 64, 16384, num_cu=NUM_CU) == ("os", 1, 8, 1, 1, True, 0, 128)
    assert ops.conv_launch_plan("split3", 27, 64, 64, 2048, groups=6, num_cu=NUM_CU).nw == 4
    try:
        ops.conv_launch_plan("bf16", 27, 512, 64, 100, num_cu=NUM_CU)
        raise AssertionError("an unserved shape must raise")
    except binding.Df3dError as e:
        assert e.entry == "df3d_conv_launch_plan"


# ---- the plans a scan reaches ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plan_runs(kind, cin, cout, kvol, groups=1):
    """One scan of n_out = 1 .. SCAN_ROWS -> [(plan, first, last)] in the order the plans are first selected: `first` is the
    smallest n_out that selects the plan, `last` the end of the run of row counts that starts there (SCAN_ROWS: no threshold
    above it inside the scan)."""
    assert_default_environment()
    fn, rec, parts = _lib_handle().df3d_conv_launch_plan, (ctypes.c_int * len(FIELDS))(), PARTS[kind]
    runs, order, prev = {}, [], None
    for n_out in range(1, SCAN_ROWS + 1):
        assert fn(parts, kvol, cin, cout, groups, n_out, 0, NUM_CU, rec) == 0, (kind, cin, cout, kvol, n_out)
        raw = bytes(rec)
        if raw == prev:
            continue
        prev = raw
        plan = tuple(rec)
        if plan not in runs:
            runs[plan] = [n_out, None]
            order.append(plan)
        for other in runs.values():                                  # the plan changed here: the run that was open ends
            if other[1] is None and other is not runs[plan]:
                other[1] = n_out - 1
    for run in runs.values():
        if run[1] is None:
            run[1] = SCAN_ROWS
    return [(plan, runs[plan][0], runs[plan][1]) for plan in order]


def plan_named(plan):
    """The record as `ops.conv_launch_plan` returns it."""
    from dualfusion import ops
    return ops.ConvLaunchPlan(ops.CONV_PLAN_FAMILIES[plan[0]], *plan[1:5], bool(plan[5]), *plan[6:])


def query_named(kind, kvol, cin, cout, groups, n_out):
    return plan_named(_query()(kind, kvol, cin, cout, groups, n_out))


# kernel volumes of the scans: the sparse 3 x 3 x 3 layers for the `os` family (the masked gathers need 27), 3 x 3 and 2 x 2 maps
# for the wide one (three wave groups with shares of 3 / 3 / 3 and 2 / 2 / 0), and one offset -- a linear layer over rows, which
# neither the loader / consumer kernel nor the wave groups take, so the plain 4- and 8-wave kernels of the wide shapes show
# (the one- and three-part launches do not look at the kernel volume -- the rules test above holds them to that --: one scan)
SCAN_KVOLS = {OS: (27, 1), WIDE: (9, 4, 1)}


def scan_kvols(kind, cin, cout):
    kvols = SCAN_KVOLS[SHAPES[(cin, cout)][0]]
    return kvols if kind == "split" else kvols[:1]


# (format, cin, cout, kvol) -> the plans a scan reaches, in the order of their smallest row count
_TWO_WAVES_THEN_EIGHT = [OS2, OS8]
_P3 = [OS2, OS4, OS8]
EXPECTED = {}
for _s in served("bf16"):
    for _k in scan_kvols("bf16", *_s):
        EXPECTED[("bf16",) + _s + (_k,)] = _TWO_WAVES_THEN_EIGHT
for _s in served("split3"):
    for _k in scan_kvols("split3", *_s):
        EXPECTED[("split3",) + _s + (_k,)] = _P3
for _s in ((128, 32), (128, 64), (64, 64), (64, 32)):
    EXPECTED[("split",) + _s + (27,)] = EXPECTED[("split",) + _s + (1,)] = _TWO_WAVES_THEN_EIGHT
for _s in ((32, 64), (32, 32)):                                      # masked gathers: 32 input channels, 27 offsets
    EXPECTED[("split",) + _s + (27,)] = [OS2, OS8_MASKED]
    EXPECTED[("split",) + _s + (1,)] = _TWO_WAVES_THEN_EIGHT
for _s in ((128, 128), (64, 128)):                                   # loader / consumer from 190 row tiles on
    EXPECTED[("split",) + _s + (27,)] = [OS2, OS8, LC1]
    EXPECTED[("split",) + _s + (1,)] = _TWO_WAVES_THEN_EIGHT
for _k in (9, 4):
    # two column blocks: 95 row tiles are 190 workgroups, before the plain 4-wave kernel would leave the wave groups' range
    EXPECTED[("split", 256, 256, _k)] = EXPECTED[("split", 128, 256, _k)] = [OS2, OS4_KS3, LC1, LC2]
    EXPECTED[("split", 256, 128, _k)] = [OS2, OS4_KS3, LC1]
    EXPECTED[("split", 512, 128, _k)] = [OS2, OS4, LC1]              # (no three-group kernel above 256 input channels)
    EXPECTED[("split", 512, 64, _k)] = _P3
for _s in (s for s in SHAPES if SHAPES[s][0] == WIDE):
    EXPECTED[("split",) + _s + (1,)] = _P3
# ... and the smallest row count of each, where it is not 1
FIRST_ROWS = {
    ("bf16", OS8): {1: 16384, 2: 8192}, ("split3", OS4): {1: 12288, 2: 6144}, ("split3", OS8): {1: 32768, 2: 16384},
    ("split", OS8): {1: 16384}, ("split", OS8_MASKED): {1: 16384}, ("split", LC1): {1: 24193, 2: 12033}, ("split", LC2): {2: 16385},
    ("split", OS4_KS3): {1: 12288, 2: 6144}, ("split", OS4): {1: 12288, 2: 6144}, ("wide1", OS8): {1: 49152, 2: 24576},
}


def test_reachable_plans_are_the_expected_set():
    """A configuration that became unreachable fails here, and so does one that appeared without a test: the GPU test loops
    over exactly these."""
    keys = [(kind,) + s + (k,) for kind in PARTS for s in served(kind) for k in scan_kvols(kind, *s)]
    assert sorted(keys) == sorted(EXPECTED) and len(served("split")) == len(served("split3")) == 13 and len(served("bf16")) == 10
    for key in keys:
        kind, cin, cout, kvol = key
        runs = plan_runs(kind, cin, cout, kvol)
        assert [r[0] for r in runs] == EXPECTED[key], (key, runs)
        gy = cout // 128 if cout > 128 else 1
        for plan, first, last in runs:
            wide_plain = kind == "split" and SHAPES[(cin, cout)][0] == WIDE and plan == OS8
            want = 1 if plan == OS2 else FIRST_ROWS[("wide1" if wide_plain else kind, plan)][gy]
            assert first == want and last >= first, (key, plan, first, last)
            assert restated_plan(kind, kvol, cin, cout, 1, first) == plan == restated_plan(kind, kvol, cin, cout, 1, last)
            if first > 1:
                assert restated_plan(kind, kvol, cin, cout, 1, first - 1) != plan
            if last < SCAN_ROWS:
                assert restated_plan(kind, kvol, cin, cout, 1, last + 1) != plan
