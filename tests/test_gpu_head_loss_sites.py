"""Loss-only path of the CenterPoint head: heat maps densely, the regression branches only at the object centres
(csrc/headloss.hip `df3d_head_regress_at`), the loss on slot rows (`df3d_centerhead_loss_slots`).

1. the kernel against the float64 composition of the same module, on targets that hold every edge case of the slot list;
2. the slot-indexed loss entry against the pixel-indexed one, bit for bit;
3. the head's new path against `loss_device(head(x))`;
4. the switch: DF3D_HEAD_LOSS_SITES=0 is the previous call sequence, and only a loss-mode forward takes the new path."""
import copy

import numpy as np
import pytest

import detgen

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
DEV = "cuda:0"
M = 11                       # object slots per sample: no multiple of the kernel's slots per workgroup (7)
NCODES = 10
CODE_COLS = (("reg", 0, 2), ("height", 2, 1), ("dim", 3, 3), ("vel", 6, 2), ("rot", 8, 2))


def _split_only():
    from dualfusion import ops
    if ops.CONV_PRECISION != "split":
        pytest.skip("the loss-only head path serves the two-part split mode")


def _head():
    from test_oracle_golden import _mirror_head
    return _mirror_head()[0]


def _targets(B, H, W, ncls):
    """Hand-made slot lists ([B, M] per task).  Sample 0 of task 0: the four corners (the last one is pixel H*W-1), an edge
    pixel, one pixel P in two slots, a masked-out slot at ind 0, ind = -1 / H*W with mask 0 and ind = -1 with mask 1.
    Task 1: P again (another task), ind = H*W with mask 1, live slots that are no prefix.  Task 2: no live slot."""
    hw = H * W
    P = (H // 2) * W + W // 2
    rs = np.random.RandomState(7)
    ex = dict(hm=[], ind=[], mask=[], cat=[], anno_box=[])
    for t, nc in enumerate(ncls):
        ind = rs.randint(0, hw, size=(B, M)).astype(np.int64)
        mask = (rs.uniform(size=(B, M)) < 0.6).astype(np.uint8)
        if t == 0:
            ind[0] = [0, W - 1, (H - 1) * W, hw - 1, W // 2, P, P, 0, -1, hw, -1]
            mask[0] = [1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 1]
        elif t == 1:
            ind[0] = [P, hw, 3, 5, 7, 2, 1, hw - 1, 0, 4, 6]
            mask[0] = [1, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1]
        elif t == 2:
            mask[:] = 0
        ex["ind"].append(ind), ex["mask"].append(mask)
        ex["cat"].append(rs.randint(0, nc, size=(B, M)).astype(np.int64))
        ex["hm"].append((rs.uniform(0, 1, size=(B, nc, H, W)) ** 6).astype(np.float32))
        ex["anno_box"].append(rs.normal(size=(B, M, NCODES)).astype(np.float32))
    return ex


def _to_dev(ex):
    return {k: [torch.from_numpy(a).to(DEV) for a in v] for k, v in ex.items()}


def _live(ind, mask, hw):
    return (mask != 0) & (ind >= 0) & (ind < hw)


@pytest.fixture(scope="module")
def head64():
    """(the fp32 head on the CPU, its float64 copy): one reference module for the tests below."""
    head = _head()
    return head, copy.deepcopy(head).double()


@pytest.mark.parametrize("shape", [(2, 512, 12, 14), (1, 512, 3, 4)])
def test_regress_at_equals_float64_maps_at_the_centres(head64, shape):
    """`df3d_head_regress_at` against `forward_reference` in float64, gathered at ind: max |pred - ref| / max |ref map| per
    branch < 1e-5 (the bar of test_forward_rows_vs_torch_cpu_and_end_to_end for the same maps); dead slots exactly 0; a
    second call bit-identical.  The second shape is a map smaller than the kernel's 5 x 5 halo."""
    _split_only()
    from dualfusion import ops
    head, ref_head = head64
    B, _, H, W = shape
    hw = H * W
    x = torch.from_numpy(detgen.randn("head_sites_x_%dx%d" % (H, W), shape))
    with torch.no_grad():
        ref = ref_head.forward_reference(x.double())
    ncls = [r["hm"].shape[1] for r in ref]
    ex = _targets(B, H, W, ncls)
    exd = _to_dev(ex)
    hd = copy.deepcopy(head).to(DEV)
    xd = x.to(DEV)
    with torch.no_grad():
        assert hd.loss_sites_fit(xd)
        _, s1, geom = hd.forward_loss_dense(xd)
        assert geom == (B, H, W)
        sites = hd._sites_plan(hd._plan())
        args = (s1, B, H, W, exd["ind"], exd["mask"], sites["w1"], sites["bias1"], sites["scale1"], sites["shift1"],
                sites["w2"], sites["b2"], sites["cols"])
        pred = ops.head_regress_at(*args)
        again = ops.head_regress_at(*args)
    torch.cuda.synchronize()
    assert tuple(pred.shape) == (len(ncls), B * M, NCODES)
    assert torch.equal(pred, again)
    got = pred.cpu().numpy()
    assert np.isfinite(got).all()
    for t in range(len(ncls)):
        ind, mask = ex["ind"][t].reshape(-1), ex["mask"][t].reshape(-1)
        live = _live(ind, mask, hw)
        assert (got[t][~live] == 0).all(), t
        if t == 2:
            assert not live.any()
        b = np.arange(B * M) // M
        for name, c0, k in CODE_COLS:
            rmap = ref[t][name].numpy()                                      # [B, k, H, W] float64
            want = rmap.transpose(0, 2, 3, 1).reshape(B * hw, k)[(b * hw + np.clip(ind, 0, hw - 1))[live]]
            err = np.abs(got[t][live, c0:c0 + k] - want).max() / np.abs(rmap).max() if live.any() else 0.0
            print("regress_at %dx%d task %d %-6s live %2d  err / scale %.3e" % (H, W, t, name, int(live.sum()), err))
            assert err < 1e-5, (t, name, err)


def test_loss_slots_equals_loss_on_full_maps(head64):
    """`ops.centerhead_loss(..., reg_by_slot=True)` on the maps of `forward_rows` gathered at ind (zeros at dead slots) is
    bit-identical to `ops.centerhead_loss` on the full maps."""
    _split_only()
    from dualfusion import ops
    head, _ = head64
    shape = (2, 512, 12, 14)
    B, _, H, W = shape
    hw = H * W
    hd = copy.deepcopy(head).to(DEV)
    x = torch.from_numpy(detgen.randn("head_sites_x_%dx%d" % (H, W), shape)).to(DEV)
    with torch.no_grad():
        preds = hd.forward_rows(x)
    ncls = [p["hm"].shape[1] for p in preds]
    exd = _to_dev(_targets(B, H, W, ncls))
    full, slot = [], []
    for t, pd in enumerate(preds):
        d = {k: hd._rows(pd[k]) for k in ("hm", "reg", "height", "dim", "rot", "vel")}
        full.append(d)
        ind, mask = exd["ind"][t].reshape(-1), exd["mask"][t].reshape(-1)
        live = (mask != 0) & (ind >= 0) & (ind < hw)
        r = torch.arange(B * M, device=DEV) // M * hw + ind.clamp(0, hw - 1)
        buf = torch.zeros((B * M, NCODES), dtype=torch.float32, device=DEV)
        for name, c0, k in CODE_COLS:
            buf[:, c0:c0 + k] = torch.where(live[:, None], d[name][r], torch.zeros((), device=DEV))
        s = {name: buf[:, c0:c0 + k] for name, c0, k in CODE_COLS}
        s["hm"] = d["hm"]
        slot.append(s)
    targets = [dict(hm=exd["hm"][t], ind=exd["ind"][t], mask=exd["mask"][t], cat=exd["cat"][t], anno_box=exd["anno_box"][t])
               for t in range(len(preds))]
    cw = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0]
    a = ops.centerhead_loss(full, targets, B, H, W, cw, 0.25)
    b = ops.centerhead_loss(slot, targets, B, H, W, cw, 0.25, reg_by_slot=True)
    assert tuple(a.shape) == (len(preds), ops.LOSS_FIELDS) and bool(torch.isfinite(a).all())
    assert torch.equal(a, b)


def test_head_loss_sites_equals_loss_device():
    """Both parts of the new path against `loss_device(ex, head(x))` on the golden map and targets, and again with one task's
    mask zeroed: every loss field within rtol 2e-5 / atol 1e-6 (the tolerance of
    test_loss_rows_values_and_gradients_equal_the_autograd_loss for the same scalars)."""
    _split_only()
    from make_golden import HEAD_SHAPE, head_loss_example
    hd = _head().to(DEV)
    hd.code_weights = [1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.2, 0.2, 1.0, 1.0]
    x = torch.from_numpy(detgen.randn("head_loss_x", HEAD_SHAPE)).to(DEV)
    ex = head_loss_example()
    for zeroed in (None, 3):
        if zeroed is not None:
            ex["mask"][zeroed][:] = 0
        exd = _to_dev(ex)
        with torch.no_grad():
            assert hd.loss_sites_wanted(exd) and hd.loss_sites_fit(x)
            got = hd.loss_sites(exd, hd.forward_loss_dense(x))
            want = hd.loss_device(exd, hd(x))
        assert set(got) == set(want)
        for k in want:
            g, w = got[k].cpu().numpy(), want[k].cpu().numpy()
            print("head loss sites (zeroed task: %s) %-14s bit-identical: %s  max |diff| %.3e"
                  % (zeroed, k, bool(np.array_equal(g, w)), float(np.abs(g - w).max())))
            assert g.shape == w.shape and np.isfinite(g).all()
            np.testing.assert_allclose(g, w, rtol=2e-5, atol=1e-6, err_msg=k)
        if zeroed is not None:
            assert float(got["num_positive"][zeroed]) == 0.0 and float(got["loc_loss"][zeroed]) == 0.0


class _Names(object):
    """Stands in for the ctypes library and notes the name of every entry that is called."""

    def __init__(self, real, names):
        self.__dict__["_real"], self.__dict__["_names"] = real, names

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("df3d_"):
            return fn
        names = self._names

        def call(*args):
            names.append(name)
            return fn(*args)
        return call


def test_switch_keeps_the_previous_call_sequence(monkeypatch):
    """DF3D_HEAD_LOSS_SITES=0: `CenterPointDetector.forward(return_loss=True)` issues the C-ABI calls of hot path ->
    `bbox_head(x)` -> `loss_device`, name for name.  Switch on: a loss-mode forward calls each new entry once and the
    pixel-indexed loss never; `return_loss=False` and `bbox_head(x)` call neither new entry."""
    _split_only()
    from dualfusion import _lib, synth
    from dualfusion.pipeline import NUSC_TASKS, CenterPointDetector
    new = ("df3d_head_regress_at", "df3d_centerhead_loss_slots")
    ncls = [t["num_class"] for t in NUSC_TASKS]
    pts = [torch.from_numpy(synth.nusc_sweep(seed=91)).to(DEV)]
    ex = _to_dev(synth.centerhead_targets(1, ncls, seed=41))
    torch.manual_seed(0)
    model = CenterPointDetector().eval().to(DEV)
    assert not model.launch_tape
    real = _lib.load()

    def record(fn):
        names = []
        monkeypatch.setattr(_lib, "_lib", _Names(real, names))
        try:
            with torch.no_grad():
                out = fn()
        finally:
            monkeypatch.setattr(_lib, "_lib", real)
        return names, out

    def by_hand():
        x, _ = model.hot_path(pts, example=ex)
        return model.bbox_head.loss_device(ex, model.bbox_head(x))

    record(lambda: model(pts, example=ex, return_loss=True))                 # lazily built plans and tables
    record(by_hand)
    monkeypatch.setenv("DF3D_HEAD_LOSS_SITES", "0")
    off, loss_off = record(lambda: model(pts, example=ex, return_loss=True))
    hand, loss_hand = record(by_hand)
    assert off == hand and not set(new) & set(off) and off.count("df3d_centerhead_loss") == 1
    assert torch.equal(loss_off["loss"], loss_hand["loss"])
    monkeypatch.setenv("DF3D_HEAD_LOSS_SITES", "1")
    on, loss_on = record(lambda: model(pts, example=ex, return_loss=True))
    assert [on.count(n) for n in new] == [1, 1] and "df3d_centerhead_loss" not in on
    np.testing.assert_allclose(loss_on["loss"].cpu().numpy(), loss_off["loss"].cpu().numpy(), rtol=2e-5, atol=1e-6)
    boxes, _ = record(lambda: model(pts, example=ex, return_loss=False))
    maps, _ = record(lambda: model.bbox_head(model.hot_path(pts, example=ex)[0]))
    assert not set(new) & set(boxes) and not set(new) & set(maps)
    model.close()
