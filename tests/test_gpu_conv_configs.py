"""Every launch configuration of the matrix-core convolutions (csrc/spconv_split.hip) against float64.

One (format, cin, cout) does not run as one kernel: the launchers pick 2, 4 or 8 waves, the masked-gather variant, three wave
groups per tile or the loader / consumer kernel from the row count.  tests/test_conv_plan_host.py pins which, and exports the
smallest row count that selects each plan; this file runs every plan there (and one row above, and at the last ragged row
count before the next threshold) and compares with tests/conv_f64_reference.py -- the default configurations, which the
parity tests on a [9, 48, 48] grid never reach.  `ops.conv_launch_plan` says before each launch which kernel the case is about
to run, so a threshold that moves fails here instead of silently testing another kernel.

Neighbour tables are built directly (no rulebook): n_in != n_out, density 0.5, and planted in them a tile of rows without any
neighbour (its output is the epilogue of zero), a tile with exactly one active offset and one with exactly two (fewer steps
than stages of the weight ring), an offset that is empty everywhere, the indices 0 and n_in - 1, a ragged last tile.  Rows
carry scales spread over 2^+-6, inside the fp16 operand range (the flag must stay clear).

Bounds, each the one the project states for the kernel class: two- and three-part 4e-6 of the output scale against float64 on
the fp32 operands (README round 5, test_sparse_conv_split_precision / _three_part_precision); bf16 2e-5 against float64 on the
bf16-rounded operands, weights and residual (test_conv_bf16_equals_fp32_kernel_on_rounded_operands).  The exact-fp32 kernel
(`ops.sparse_conv_fused`) runs on the same inputs as the yardstick, and both errors are printed (pytest -s)."""
import pytest

import conv_f64_reference as cref
import test_conv_plan_host as plans

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BOUND = {"split": 4e-6, "split3": 4e-6, "bf16": 2e-5}
INDEXING_BUG = 1e-3                 # an error of this size is a wrong index or a wrong operand layout, whatever the yardstick says
CASES = [(kind,) + s for kind in ("split", "split3", "bf16") for s in plans.served(kind)]
GROUPS = 6
# grouped launches (`ops.conv_rows_split`: the heads' branch convolutions), one shape per launch family -- where n_out * gy
# crosses the thresholds: (cin, cout) -> (kvol, input columns between groups; 0 = every group reads the same columns)
GROUPED = {(64, 64): (9, 64), (512, 64): (9, 0), (128, 128): (9, 0)}
GROUPED_MAX_ROWS = 20000


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    plans.assert_default_environment()
    return torch.device("cuda:0")


def _table(K, n_in, n_out, tile, empty_offset, seed):
    """int32 [K, n_out] on the host, with the planted features that fit into n_out rows of `tile`-row tiles."""
    gen = torch.Generator().manual_seed(seed)
    nbr = torch.randint(0, n_in, (K, n_out), generator=gen, dtype=torch.int32)
    nbr[torch.rand((K, n_out), generator=gen) >= 0.5] = -1
    if empty_offset and K > 2:
        nbr[1] = -1
    tiles = -(-n_out // tile)
    live = [k for k in range(K) if not (empty_offset and K > 2 and k == 1)]
    planted = []
    for t, offsets in ((1, ()), (2, live[-1:]), (3, (live[0], live[-1]) if len(live) > 1 else ())):
        if t > tiles - 2 or (t > 1 and not offsets):          # (tile 0 and the last, ragged one stay as they are)
            continue
        rows = slice(t * tile, (t + 1) * tile)
        keep = nbr[:, rows].clone()
        nbr[:, rows] = -1
        for k in offsets:
            nbr[k, rows] = keep[k]
            nbr[k, t * tile] = (t * 7919 + k) % n_in          # at least one pair at the offset
        planted.append(t)
    nbr[live[0], 0] = 0
    nbr[live[-1], min(1, n_out - 1) if len(live) == 1 else 0] = n_in - 1
    return nbr, planted


def _rows(n, c, seed, dev):
    """randn rows under per-row scales spread over 2^+-6, |x| < 2000"""
    gen = torch.Generator(device=dev).manual_seed(seed)
    x = torch.randn((n, c), generator=gen, device=dev)
    x = x * torch.exp2(torch.rand((n, 1), generator=gen, device=dev) * 12 - 6)
    return x.clamp_(-2000.0, 2000.0)


def _row_counts(first, last, tile):
    """smallest selecting count; one more row (a last tile of one row where the smallest is a tile multiple); the largest count
    below the next threshold that is no multiple of the tile (none where the scan met no threshold above)."""
    counts = [first]
    if first + 1 <= last:
        counts.append(first + 1)
    if last < plans.SCAN_ROWS:
        ragged = last if last % tile else last - 1
        if ragged > counts[-1]:
            counts.append(ragged)
    return counts


class _Shape(object):
    """The operands of one (format, cin, cout, K) that do not depend on the row count."""

    def __init__(self, kind, cin, cout, K, dev, groups=1):
        from dualfusion import ops
        self.kind, self.cin, self.cout, self.K, self.groups = kind, cin, cout, K, groups
        gen = torch.Generator(device=dev).manual_seed(cin * 1000 + cout * 10 + K + groups)
        shape = (groups, K, cin, cout) if groups > 1 else (K, cin, cout)
        self.filt = torch.randn(shape, generator=gen, device=dev) * (0.5 / cin ** 0.5)
        C = groups * cout
        self.bias, self.shift = (torch.randn((C,), generator=gen, device=dev) * 0.1 for _ in range(2))
        self.scale = 1 + torch.randn((C,), generator=gen, device=dev) * 0.1
        if kind == "bf16":
            self.packed = ops.conv_pack_weights_bf16(self.filt)
            self.filt_ref = self.filt.bfloat16().float()               # what the reference multiplies: the rounded weights
        else:
            with ops.precision(kind):
                self.packed = ops.conv_pack_weights_groups(self.filt) if groups > 1 else ops.conv_pack_weights(self.filt)
            self.filt_ref = self.filt


def _err(got, ref):
    return float((got.double() - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def _check_three_part_rows(rows, y):
    """hi + mid + lo of the emitted three-part rows == the fp32 rows, exactly"""
    n, c = y.shape
    parts = rows.view(n, c // 8, 3, 8, 2).view(torch.int16).reshape(n, c // 8, 3, 8).to(torch.int32)
    recon = sum((parts[:, :, p] << 16).view(torch.float32).double() for p in range(3))
    assert torch.equal(recon.reshape(n, c).float(), y)


def _run_case(sh, plan, n_out, which, dev, worst, order=False):
    """One row count under both epilogues; -> nothing, asserts.  worst: {(plan, epilogue): (err, yardstick err)} of the shape."""
    from dualfusion import ops
    kind, cin, cout, K = sh.kind, sh.cin, sh.cout, sh.K
    tile = plan[7]
    n_in = n_out * 7 // 8 + 3
    fam = plans.SHAPES[(cin, cout)][0]
    empty_offset = fam == plans.OS or which == "last"            # (wide: 3 / 3 / 3 and 2 / 2 / 0 shares need every offset)
    nbr_h, planted = _table(K, n_in, n_out, tile, empty_offset, n_out * 31 + K)
    assert int(nbr_h.max()) == n_in - 1 and (bool((nbr_h == 0).any()) or K * n_out == 1)
    if which != "first":
        assert n_out % tile, (plan, n_out)                       # the last tile is ragged
    if n_out >= 5 * tile:
        assert planted == ([1, 2, 3] if K > 1 else [1, 2]) and bool((nbr_h[:, tile:2 * tile] < 0).all())
        assert int((nbr_h[:, 2 * tile:3 * tile] >= 0).any(1).sum()) == 1
        assert K == 1 or int((nbr_h[:, 3 * tile:4 * tile] >= 0).any(1).sum()) == 2
        assert not empty_offset or K <= 2 or bool((nbr_h[1] < 0).all())
    nbr = nbr_h.to(dev)
    x = _rows(n_in, cin, n_out + 1, dev)
    res = _rows(n_out, cout, n_out + 2, dev)
    want_plan = plans.plan_named(plan)
    got_plan = ops.conv_launch_plan(kind, K, cin, cout, n_out)
    assert got_plan == want_plan, (kind, cin, cout, K, n_out, got_plan, want_plan)
    if kind == "bf16":
        xb, rb = ops.rows_to_bf16(x), ops.rows_to_bf16(res)
        assert torch.equal(xb, x.to(torch.bfloat16))
        x_ref, res_ref = xb.float(), rb.float()
        operand = xb
    else:
        with ops.precision(kind):
            operand = ops.split_rows(x)
        x_ref, res_ref = x, res
    acc = cref.conv_acc_f64(x_ref, sh.filt_ref, nbr, n_out)
    perm = torch.randperm(n_out, device=dev).to(torch.int32) if order else None
    for tag, kw in (("none", {}), ("all", dict(bias=sh.bias, scale=sh.scale, shift=sh.shift, relu=True))):
        ref = cref.epilogue_f64(acc, residual=res_ref if kw else None, **kw)
        if kind == "bf16":
            y, yrows = ops.sparse_conv_bf16(operand, sh.packed, nbr, n_out, cin, cout, residual=rb if kw else None, want_f32=True,
                                            want_bf16=True, **kw)
            assert torch.equal(yrows, y.to(torch.bfloat16)), (plan, n_out, tag)
        else:
            with ops.precision(kind):
                y, yrows = ops.sparse_conv_split(operand, sh.packed, nbr, n_out, cin, cout, residual=res if kw else None,
                                                 emit_split=True, order=perm, **kw)
                assert torch.equal(yrows, ops.split_rows(y)), (plan, n_out, tag)
            if kind == "split3":
                _check_three_part_rows(yrows, y)
        y32 = ops.sparse_conv_fused(x_ref, sh.filt_ref, nbr, n_out, residual=res_ref if kw else None, **kw)
        err, yard = _err(y, ref), _err(y32, ref)
        print("conv-config %s %d->%d K=%d %s n_out=%d (%s) epilogue=%s: err %.3g  exact-fp32 %.3g"
              % (kind, cin, cout, K, want_plan, n_out, which, tag, err, yard))
        key = (plan, tag)
        if key not in worst or err > worst[key][0]:
            worst[key] = (err, yard)
        assert err < INDEXING_BUG, (kind, cin, cout, K, plan, n_out, tag, err)
        assert err < BOUND[kind], (kind, cin, cout, K, plan, n_out, tag, err, yard)
        if planted and not kw:                                   # the tile without a neighbour: exact zeros
            assert not bool(y[tile:2 * tile].any()), (plan, n_out)
    hit, where = ops.split_overflow(reset=True)
    assert not hit, where


def _run_grouped(kind, cin, cout, dev):
    """`groups` convolutions over one table in one launch (gridDim.y = groups), at the first row count of every plan the grouped
    scan reaches and one row below it: the thresholds that n_out * gy crosses."""
    from dualfusion import ops
    K, stride = GROUPED[(cin, cout)]
    sh = _Shape(kind, cin, cout, K, dev, groups=GROUPS)
    for plan, first, last in plans.plan_runs(kind, cin, cout, K, GROUPS):
        if first > GROUPED_MAX_ROWS:
            continue
        for n_out in sorted({max(first - 1, 1), first}):
            n_in = n_out * 7 // 8 + 3
            want_plan = plans.query_named(kind, K, cin, cout, GROUPS, n_out)
            assert want_plan == ops.conv_launch_plan(kind, K, cin, cout, n_out, groups=GROUPS)
            nbr = _table(K, n_in, n_out, want_plan.tile_rows, True, n_out * 17 + K)[0].to(dev)
            x = _rows(n_in, stride * (GROUPS - 1) + cin, n_out + 3, dev)
            ref = cref.conv_rows_f64(x, sh.filt, nbr, n_out, sh.bias, sh.scale, sh.shift, None, True, GROUPS, stride)
            with ops.precision(kind):
                y, yrows = ops.conv_rows_split(ops.split_rows(x), cin, stride, sh.packed, cout, GROUPS, nbr, n_out, sh.bias, sh.scale,
                                               sh.shift, relu=True, want_split=True)
                assert torch.equal(yrows, ops.split_rows(y))
            err = _err(y, ref)
            print("conv-config %s %d->%d K=%d groups=%d %s n_out=%d: err %.3g" % (kind, cin, cout, K, GROUPS, want_plan, n_out, err))
            assert err < BOUND[kind], (kind, cin, cout, GROUPS, want_plan, n_out, err)
    hit, where = ops.split_overflow(reset=True)
    assert not hit, where


@pytest.mark.parametrize("kind,cin,cout", CASES)
def test_every_launch_plan_against_float64(dev, kind, cin, cout):
    from dualfusion import ops
    ops.split_overflow(reset=True)
    done, worst = set(), {}
    for K in plans.scan_kvols(kind, cin, cout):
        sh = None
        for plan, first, last in plans.plan_runs(kind, cin, cout, K):
            if K == 1 and plan in done:
                continue                                         # one offset: only the plans no other kernel volume reaches
            sh = sh or _Shape(kind, cin, cout, K, dev)
            counts = _row_counts(first, last, plan[7])
            for i, n_out in enumerate(counts):
                _run_case(sh, plan, n_out, "last" if i == 2 else ("first", "first+1")[i], dev, worst)
            done.add(plan)
    assert done == {p for K in plans.scan_kvols(kind, cin, cout) for p, _, _ in plans.plan_runs(kind, cin, cout, K)}
    if kind == "split":                                          # a tiling order (two-part entry): the top plan's first row count
        K = plans.scan_kvols(kind, cin, cout)[0]
        plan, first, _ = plans.plan_runs(kind, cin, cout, K)[-1]
        _run_case(_Shape(kind, cin, cout, K, dev), plan, first + 1, "order", dev, worst, order=True)
    if kind != "bf16" and (cin, cout) in GROUPED:
        _run_grouped(kind, cin, cout, dev)
    for (plan, tag), (err, yard) in sorted(worst.items()):
        print("conv-config-worst %s %d->%d %s epilogue=%s: %.3g (exact fp32 %.3g)" % (kind, cin, cout, plans.plan_named(plan), tag, err, yard))
