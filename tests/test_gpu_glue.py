"""The camera-fusion glue of csrc/fusion.hip, entry point by entry point through the C ABI, against the host reference
tests/glue_reference.py (plain numpy written from the contract text of include/df3d_hip.h; checked on its own and against the
port of the adapter in tests/test_glue_host.py).  Integers and copies are exact; a floating result may be at most four times
as far from the float64 reference as the same formula in numpy float32 is, plus 1e-6 of the tensor's scale.

The inputs are the ones no other test produces: samples without voxels inside and at the end of the batch, lists that cross
the 1024-row pass of the slot scan, an empty list and an all-visible one, max_ne below the list lengths, channel counts
outside the by-slot kernel's registers and off the 8-channel write-back, winners on the map's corners, calibration, image
size and feature scale per (sample, camera), a per-sample augmentation, the requested depth.

Pixels of visible rows handed to the assembly entries and to df3d_query_pixel_rows lie inside the map (the contract: the
projection emits no other); the scatter entries are also given pixels outside it, which they drop."""
import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":                     # the child of test_assemble_queries2_with_the_kernel_forced
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "3d-dual-fusion_amd"), os.path.join(_root, "tests", "golden")]

import glue_reference as gr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda:0"
MAP_H, MAP_W, SLOT_NCAM, SLOT_DENSITY = 20, 36, 3, 0.3
CHANNEL_PAIRS = [(128, 256), (32, 80), (24, 256), (320, 576)]          # the last pair is past the by-slot kernel's 256 / 512
FILL = -3.0


def P(x):
    return ctypes.c_void_p(x.data_ptr()) if x is not None else ctypes.c_void_p(0)


def D(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _lib():
    from dualfusion import _lib as L, ops
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    return L.load(), L.check, ops._stream


@functools.lru_cache(maxsize=None)
def slot_case(C, Ci, out_of_map=False):
    """The slot case at one channel pair: host arrays, the reference's slots, and the inputs on the device."""
    c = gr.glue_case(5, gr.SLOT_ROWS, SLOT_NCAM, MAP_H, MAP_W, C, Ci, SLOT_DENSITY, out_of_map=out_of_map)
    c["pos"], c["counts"] = gr.slots(c["mask"], c["ind"], c["B"], c["ncam"])
    c["dev"] = {k: D(c[k]) for k in ("ind", "mask", "grid", "feat", "pinv", "img", "att", "pos", "counts")}
    seen = c["mask"].astype(int).sum(0)
    assert {0, 1, 3} <= set(seen.tolist())                               # a voxel seen by no, one and every camera
    assert 0 in c["counts"].tolist() and int(c["counts"].max()) == 1025  # an empty list, and every row of the 1025-row sample
    return c


def ulp_distance(a, b):
    """Largest distance in units of the last place between two non-negative fp32 tensors."""
    return int((a.contiguous().view(torch.int32).long() - b.contiguous().view(torch.int32).long()).abs().max()) if a.numel() else 0


# ---------------------------------------------------------------------------------------------------------- slots
def test_query_slots_across_passes_and_empty_samples():
    """df3d_query_slots on rows per sample (1, 0, 1024, 1025, 2500, 0), three cameras: pos equal on every row (the contract
    defines it on invisible rows too, and the lanes-over-queries assembly searches them) and counts equal, with an empty
    list, a 1025-row all-visible list (a full 1024-row pass and a carry) and invisible runs at a sample's start and end."""
    lib, check, stream = _lib()
    c = slot_case(32, 80)
    d = c["dev"]
    pos = torch.full((c["ncam"], c["n"]), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((c["B"] * c["ncam"],), -7, dtype=torch.int32, device=DEV)
    check(lib.df3d_query_slots(P(d["mask"]), P(d["ind"]), c["n"], c["B"], c["ncam"], P(pos), P(counts), stream()))
    assert np.array_equal(counts.cpu().numpy(), c["counts"])
    got = pos.cpu().numpy()
    vis = c["mask"] != 0
    assert np.array_equal(got[vis], c["pos"][vis])
    assert np.array_equal(got, c["pos"])


# ------------------------------------------------------------------------------------------------------- assembly
def assembly_reference(c, max_ne, use_att):
    """The padded query tensors of the reference on the device: the fp32 evaluation (v_feat, qpts, v_i_feat are a copy, a copy
    and one multiply: the kernel's bits) and the float64 one for qgrid and qpos."""
    args = (c["feat"], c["pinv"], c["ind"], c["grid"], c["mask"], c["pos"], c["img"], c["B"], c["ncam"], c["H"], c["W"], max_ne)
    r32 = gr.assemble(*args, att=c["att"] if use_att else None, want_qpos=True, fp32=True)
    r64 = gr.assemble(*args, att=None, want_qpos=True)
    ref = {k: D(v) for k, v in r32.items()}
    ref["qpos64"], ref["qgrid64"] = D(r64["qpos"]), D(r64["qgrid"])
    ref["qpos_yard"] = float(np.abs(r32["qpos"] - r64["qpos"]).max())
    return ref


def compact_rows(c):
    """pixrow of the reference and the pixel-major rows compact[rank] = the image column of that pixel, built on the host."""
    pixrow, total = gr.pixel_rows(c["ind"], c["grid"], c["mask"], c["B"], c["ncam"], c["H"], c["W"])
    cols = c["img"].transpose(0, 2, 3, 1).reshape(-1, c["Ci"])
    compact = cols[pixrow >= 0]
    assert len(compact) == total
    return D(pixrow), D(compact)


ENTRIES = ("queries", "queries2", "queries2_counts", "slots", "slots_table", "slots_compact", "compact")


def run_assembly(entry, c, max_ne, use_att, use_qpos, extra):
    """One assembly entry into tensors prefilled with -3 -> [v_feat, v_i_feat, qgrid, qpts, qpos]."""
    lib, check, stream = _lib()
    d = c["dev"]
    NI, C, Ci = c["B"] * c["ncam"], c["C"], c["Ci"]
    outs = [torch.full((NI, max_ne, k), FILL, device=DEV) for k in (C, Ci, 2, 3, C)]
    att = P(d["att"]) if use_att else None
    qpos = P(outs[4]) if use_qpos else None
    head = (P(d["feat"]), P(d["pinv"]), P(d["ind"]), P(d["grid"]), P(d["mask"]), P(extra["pos"]))
    dims = (c["n"], C, Ci, c["B"], c["ncam"], c["H"], c["W"], max_ne)
    o4 = (P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]))
    if entry == "queries":
        check(lib.df3d_assemble_queries(*head, P(d["img"]), *dims, *o4, stream()), entry)
    elif entry in ("queries2", "queries2_counts"):
        check(lib.df3d_assemble_queries2(*head, P(d["img"]), None, att, *dims, *o4, qpos,
                                         P(extra["counts"]) if entry == "queries2_counts" else None, stream()), entry)
    elif entry in ("slots", "slots_table", "slots_compact"):
        table = torch.full((NI * max(max_ne, 1), 4), -9, dtype=torch.int32, device=DEV)
        use_c = entry == "slots_compact"
        check(lib.df3d_assemble_queries2_slots(*head, P(d["img"]) if entry == "slots" else None,
                                               P(extra["ptrs"]) if entry == "slots_table" else None, att, *dims, *o4, qpos,
                                               P(extra["counts"]), P(table), P(extra["pixrow"]) if use_c else None,
                                               P(extra["compact"]) if use_c else None, stream()), entry)
    else:
        check(lib.df3d_assemble_queries2_compact(*head, P(extra["pixrow"]), P(extra["compact"]), att, *dims, *o4, qpos,
                                                 P(extra["counts"]), stream()), entry)
    return outs


def check_assembly(tag, outs, ref, use_qpos, worst):
    v_feat, v_i, qgrid, qpts, qpos = outs
    assert torch.equal(v_feat, ref["v_feat"]), tag
    assert torch.equal(qpts, ref["qpts"]), tag
    assert torch.equal(v_i, ref["v_i_feat"]), tag
    assert ulp_distance(qgrid, ref["qgrid"]) <= 2, tag
    assert float((qgrid.double() - ref["qgrid64"]).abs().max()) <= 2.0 ** -22, tag
    if use_qpos:
        err = float((qpos.double() - ref["qpos64"]).abs().max()) if qpos.numel() else 0.0
        worst["qpos"], worst["yard"] = max(worst["qpos"], err), max(worst["yard"], ref["qpos_yard"])
        assert err <= 4.0 * ref["qpos_yard"] + 1e-6, (tag, err, ref["qpos_yard"])
    else:
        assert bool((qpos == FILL).all()), tag                           # not requested: not touched


def assembly_sweep(C, Ci, entries, combos):
    """Every entry in `entries` at the channel pair, for (att, qpos) in `combos` and max_ne = the longest list, half of it
    and 1 -> the worst qpos error and its yardstick."""
    c = slot_case(C, Ci)
    d = c["dev"]
    lib, check, stream = _lib()
    pos = torch.full((c["ncam"], c["n"]), -7, dtype=torch.int32, device=DEV)
    counts = torch.full((c["B"] * c["ncam"],), -7, dtype=torch.int32, device=DEV)
    check(lib.df3d_query_slots(P(d["mask"]), P(d["ind"]), c["n"], c["B"], c["ncam"], P(pos), P(counts), stream()))
    assert torch.equal(counts, d["counts"])                              # the kernels read the slots the slot kernel wrote
    extra = dict(pos=pos, counts=counts)
    extra["pixrow"], extra["compact"] = compact_rows(c)
    extra["ptrs"] = torch.tensor([d["img"][i].data_ptr() for i in range(c["B"] * c["ncam"])], dtype=torch.int64, device=DEV)
    full = int(c["counts"].max())
    worst = dict(qpos=0.0, yard=0.0)
    for max_ne in (full, full // 2, 1):
        for use_att in sorted({a for a, _ in combos}):
            ref = assembly_reference(c, max_ne, use_att)
            for use_qpos in sorted({q for a, q in combos if a == use_att}):
                for entry in entries:
                    if entry == "queries" and (use_att or use_qpos):
                        continue                                         # df3d_assemble_queries has neither
                    outs = run_assembly(entry, c, max_ne, use_att, use_qpos, extra)
                    check_assembly((entry, C, Ci, max_ne, use_att, use_qpos), outs, ref, use_qpos, worst)
            del ref
    torch.cuda.synchronize()
    print("assembly C=%d Ci=%d: qpos kernel %.3g, fp32 yardstick %.3g" % (C, Ci, worst["qpos"], worst["yard"]))
    return worst


@pytest.mark.parametrize("C,Ci", CHANNEL_PAIRS)
def test_assembly_entries_against_the_reference(C, Ci):
    """df3d_assemble_queries, _queries2 (without and with list lengths), _queries2_slots (one tensor / pointer table / pixrow +
    compact) and _queries2_compact on the slot case, map 20 x 36, with and without att and qpos, outputs prefilled with -3,
    max_ne = 1025 (the longest list), 512 and 1: v_feat, qpts and v_i_feat bit-equal to numpy float32, qgrid within 2 ulp, qpos
    within the yardstick; padding rows zero (qpos 0 / 1), slots >= max_ne dropped, nothing left unwritten.
    Measured on the MI355X, qpos (kernel / fp32 yardstick; both carry the rounding of the shared depth argument): 7.9e-7 / 7.9e-7
    at (128, 256), 5.1e-7 / 5.1e-7 at (32, 80) and (24, 256), 8.1e-7 / 8.1e-7 at (320, 576); every other tensor exact."""
    assembly_sweep(C, Ci, ENTRIES, [(True, True), (True, False), (False, True), (False, False)])


@pytest.mark.parametrize("mode", ["1", "2"])
def test_assemble_queries2_with_the_kernel_forced(mode):
    """df3d_assemble_queries2 with list lengths under DF3D_ASSEMBLE=1 (lanes over queries: the slot's row by binary search
    over pos) and DF3D_ASSEMBLE=2 (a wave per candidate).  The variable is read once per process, so each setting runs the
    sweep of the test above (all channel pairs; att + qpos, neither) in a fresh child process.
    Measured on the MI355X: the figures of the test above under both settings, 3.2 s per child."""
    env = dict(os.environ, DF3D_ASSEMBLE=mode)
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable] + flags + [os.path.abspath(__file__), "assemble"], env=env, timeout=300, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, universal_newlines=True)
    print(r.stdout)
    assert r.returncode == 0 and "assembly child ok" in r.stdout, r.stdout[-4000:]


# ------------------------------------------------------------------------------------------------------ write-back
@pytest.mark.parametrize("C", [128, 20])
def test_writeback_against_the_reference(C):
    """df3d_fusion_writeback at C = 128 (16-byte path) and C = 20 (the one-channel kernel), df3d_fusion_writeback_split
    without and with the split rows (C = 128), on the slot case -- voxels seen by 0, 1 and all 3 cameras -- with max_ne = the
    longest list and half of it (slots past it add nothing): bit-equal to the reference's fp32 adds in camera order, the split
    rows bit-equal to ops.split_rows(out)."""
    from dualfusion import ops
    lib, check, stream = _lib()
    c = slot_case(C, 8)
    d = c["dev"]
    n, NI, ncam = c["n"], c["B"] * c["ncam"], c["ncam"]
    rs = np.random.RandomState(C)
    for max_ne in (int(c["counts"].max()), int(c["counts"].max()) // 2):
        enh = rs.standard_normal((NI, max_ne, C)).astype(np.float32)
        want = D(gr.writeback(c["feat"], enh, c["ind"], c["mask"], c["pos"], max_ne))
        assert not torch.equal(want, d["feat"])
        enh_d = D(enh)
        out = torch.full((n, C), FILL, device=DEV)
        check(lib.df3d_fusion_writeback(P(d["feat"]), P(enh_d), P(d["ind"]), P(d["mask"]), P(d["pos"]), n, C, ncam, max_ne, P(out),
                                        stream()))
        assert torch.equal(out, want), max_ne
        if C % 8:
            continue
        for with_split in (False, True):
            out = torch.full((n, C), FILL, device=DEV)
            split = torch.zeros((n, 4 * C), dtype=torch.uint8, device=DEV) if with_split else None
            check(lib.df3d_fusion_writeback_split(P(d["feat"]), P(enh_d), P(d["ind"]), P(d["mask"]), P(d["pos"]), n, C, ncam, max_ne,
                                                  P(out), P(split), stream()))
            assert torch.equal(out, want), (max_ne, with_split)
            if with_split:
                assert torch.equal(split, ops.split_rows(want)), max_ne


# ------------------------------------------------------------------------------------------------- winner and gate
def test_winner_canvas_and_gate_scatter_with_pixels_outside_the_map():
    """df3d_scatter_winner, df3d_scatter_to_image and df3d_gate_scatter on the slot case with three entries in ten outside the
    map (-3 .. W + 2): the winner map equals the reference's (highest row per pixel, outside pixels dropped, -1 where
    empty); the canvas holds exactly the winners' (features | xyz) and zeros elsewhere; S, from s9 = rows @ T.T evaluated in
    float64 and rounded, equals the reference bit for bit (one fp32 add per winner), over two scales with clear on the first."""
    lib, check, stream = _lib()
    C = 32
    c, c2 = slot_case(C, 80, True), gr.glue_case(6, gr.SLOT_ROWS, SLOT_NCAM, MAP_H, MAP_W, C, 8, 0.5, out_of_map=True)
    B, ncam, H, W, n = c["B"], c["ncam"], c["H"], c["W"], c["n"]
    NI = B * ncam
    d = c["dev"]
    win_ref = gr.winner(c["ind"], c["grid"], c["mask"], B, ncam, H, W)
    assert (win_ref >= 0).sum() > 500 and all(win_ref[4 * ncam, y, x] >= 0 for y in (0, H - 1) for x in (0, W - 1))
    outside = (c["grid"][:, :, 0] < 0) | (c["grid"][:, :, 0] >= W) | (c["grid"][:, :, 1] < 0) | (c["grid"][:, :, 1] >= H)
    assert (outside & (c["mask"] != 0)).sum() > 100
    win = torch.full((NI, H, W), -5, dtype=torch.int32, device=DEV)
    check(lib.df3d_scatter_winner(P(d["ind"]), P(d["grid"]), P(d["mask"]), n, B, ncam, H, W, P(win), stream()))
    assert np.array_equal(win.cpu().numpy(), win_ref)
    # pts2img canvas
    win.fill_(-5)
    canvas = torch.full((NI, C + 3, H, W), FILL, device=DEV)
    check(lib.df3d_scatter_to_image(P(d["feat"]), P(d["pinv"]), P(d["ind"]), P(d["grid"]), P(d["mask"]), n, C, B, ncam, H, W, P(win),
                                    P(canvas), stream()))
    want = np.zeros((NI, C + 3, H, W), np.float32)
    im, y, x = np.nonzero(win_ref >= 0)
    want[im, :, y, x] = np.concatenate([c["feat"], c["pinv"]], 1)[win_ref[im, y, x]]
    assert np.array_equal(win.cpu().numpy(), win_ref) and np.array_equal(canvas.cpu().numpy(), want)
    # gate scatter, two scales into one S
    rs = np.random.RandomState(2)
    S = torch.full((NI, 9, H, W), 7.0, device=DEV)
    S_ref = None
    for k, cc in enumerate((c, c2)):
        T = rs.standard_normal((9, C + 3)) * 0.2
        s9 = (np.concatenate([cc["feat"], cc["pinv"]], 1).astype(np.float64) @ T.T).astype(np.float32)
        wr = gr.winner(cc["ind"], cc["grid"], cc["mask"], B, ncam, H, W)
        S_ref = gr.gate_S(None, None, None, wr, k == 0, S_ref, s9=s9, fp32=True)
        dv = [D(a) for a in (s9, cc["ind"], cc["grid"], cc["mask"])]      # held until the results are read
        check(lib.df3d_gate_scatter(P(dv[0]), P(dv[1]), P(dv[2]), P(dv[3]), cc["n"], B, ncam, H, W, P(win), P(S), int(k == 0),
                                    stream()))
        assert np.array_equal(win.cpu().numpy(), wr)
    assert np.array_equal(S.cpu().numpy(), S_ref) and float(np.abs(S_ref).max()) > 1.0


@pytest.mark.parametrize("C", [4, 32, 36, 128])
def test_gate_rows_against_the_reference(C):
    """df3d_gate_scatter_rows and df3d_gate_rows (on the winner map of df3d_scatter_winner) at C = 4, 32, 36 (not a multiple of
    the 32-channel pass: its guarded tail) and 128: two scales accumulate into one S prefilled with 7, clear on the first only;
    the winner map is exact, S within the yardstick of the float64 row responses.
    Measured on the MI355X (kernel / fp32 yardstick, both entries alike, S of size 43-66: the rounding of the stored sum):
    C=4 5.7e-6 / 5.7e-6, C=32 5.4e-6 / 5.4e-6, C=36 3.9e-6 / 3.9e-6, C=128 4.4e-6 / 4.4e-6."""
    lib, check, stream = _lib()
    rows = (1, 0, 700, 1300, 0)
    cases = [gr.glue_case(10 + C + k, rows, SLOT_NCAM, MAP_H, MAP_W, C, 8, 0.5, out_of_map=True) for k in range(2)]
    B, ncam, H, W = cases[0]["B"], SLOT_NCAM, MAP_H, MAP_W
    NI = B * ncam
    rs = np.random.RandomState(C)
    Ts = [(rs.standard_normal((9, C + 3)) * 0.2).astype(np.float32) for _ in cases]
    S64 = S32 = None
    S_a, S_b = [torch.full((NI, 9, H, W), 7.0, device=DEV) for _ in range(2)]
    for k, (cc, T) in enumerate(zip(cases, Ts)):
        wr = gr.winner(cc["ind"], cc["grid"], cc["mask"], B, ncam, H, W)
        S64 = gr.gate_S(cc["feat"], cc["pinv"], T, wr, k == 0, S64)
        S32 = gr.gate_S(cc["feat"], cc["pinv"], T, wr, k == 0, S32, fp32=True)
        dv = [D(cc[key]) for key in ("feat", "pinv", "ind", "grid", "mask")]
        Td = D(T)
        win = torch.full((NI, H, W), -5, dtype=torch.int32, device=DEV)
        check(lib.df3d_gate_scatter_rows(P(dv[0]), C, P(dv[1]), P(Td), P(dv[2]), P(dv[3]), P(dv[4]), cc["n"], B, ncam, H, W, P(win),
                                         P(S_a), int(k == 0), stream()))
        assert np.array_equal(win.cpu().numpy(), wr)
        win.fill_(-5)
        check(lib.df3d_scatter_winner(P(dv[2]), P(dv[3]), P(dv[4]), cc["n"], B, ncam, H, W, P(win), stream()))
        check(lib.df3d_gate_rows(P(dv[0]), C, P(dv[1]), P(Td), P(win), NI, H, W, P(S_b), int(k == 0), stream()))
    assert float(np.abs(S64).max()) > 1.0 and (S64 == 0).any()
    gr.assert_within_yardstick("gate_scatter_rows C=%d" % C, S_a.cpu().numpy(), S64, S32)
    gr.assert_within_yardstick("gate_rows C=%d" % C, S_b.cpu().numpy(), S64, S32)


@pytest.mark.parametrize("H,W", [(1, 1), (1, 7), (3, 3), (20, 36)])
def test_gate_finish_zero_padding_with_winners_on_the_border(H, W):
    """df3d_scatter_winner -> df3d_gate_rows -> df3d_gate_finish / df3d_gate_finish_bias on maps 1 x 1, 1 x 7, 3 x 3 and 20 x 36
    with a winner on every border pixel (corners included; on 20 x 36 the interior is filled at random): S and the attention
    map within the yardstick of the float64 reference -- a tap that reads across the border, or a border tap left out, is
    an error of the size of a term.
    Measured on the MI355X (kernel / fp32 yardstick): S 3.0e-8 .. 8.3e-8, equal to the yardstick on every map; att without / with
    the bias 1 x 1 2.4e-8 / 2.1e-8 and 3.5e-8 / 3.5e-8, 1 x 7 4.6e-8 / 6.2e-8 and 4.4e-8 / 6.0e-8, 3 x 3 5.0e-8 / 5.0e-8 and
    5.1e-8 / 7.7e-8, 20 x 36 8.5e-8 / 9.3e-8 and 9.4e-8 / 9.4e-8."""
    lib, check, stream = _lib()
    B, ncam, C = 2, 2, 8
    NI = B * ncam
    rs = np.random.RandomState(H * 100 + W)
    border = [(y, x) for y in range(H) for x in range(W) if y in (0, H - 1) or x in (0, W - 1)]
    inner = [(int(rs.randint(H)), int(rs.randint(W))) for _ in range(H * W // 3)] if H * W > 9 else []
    pix = np.array((border + inner) * 2)                                 # every pixel twice: the later row wins
    n_b = len(pix)
    ind = np.zeros((B * n_b, 4), np.int32)
    ind[:, 0] = np.repeat(np.arange(B), n_b)
    grid = np.zeros((ncam, B * n_b, 2), np.int32)
    grid[:, :, 0], grid[:, :, 1] = np.tile(pix[:, 1], B), np.tile(pix[:, 0], B)
    mask = np.ones((ncam, B * n_b), np.uint8)
    feat, pinv = rs.standard_normal((B * n_b, C)).astype(np.float32), rs.uniform(-1, 1, (B * n_b, 3)).astype(np.float32)
    T = (rs.standard_normal((9, C + 3)) * 0.05).astype(np.float32)
    kg = (rs.standard_normal(19) * 0.2).astype(np.float32)
    gate, b3 = rs.standard_normal((NI, H, W)).astype(np.float32), np.array([0.37], np.float32)
    wr = gr.winner(ind, grid, mask, B, ncam, H, W)
    assert all(wr[i, y, x] >= n_b // 2 + (i // ncam) * n_b for i in range(NI) for y, x in border)      # the second copy won
    S64, S32 = gr.gate_S(feat, pinv, T, wr, True, None), gr.gate_S(feat, pinv, T, wr, True, None, fp32=True)
    win = torch.full((NI, H, W), -5, dtype=torch.int32, device=DEV)
    S = torch.full((NI, 9, H, W), 7.0, device=DEV)
    dv = [D(a) for a in (ind, grid, mask, feat, pinv, T, b3)]             # held until the results are read
    check(lib.df3d_scatter_winner(P(dv[0]), P(dv[1]), P(dv[2]), B * n_b, B, ncam, H, W, P(win), stream()))
    assert np.array_equal(win.cpu().numpy(), wr)
    check(lib.df3d_gate_rows(P(dv[3]), C, P(dv[4]), P(dv[5]), P(win), NI, H, W, P(S), 1, stream()))
    gr.assert_within_yardstick("S %dx%d" % (H, W), S.cpu().numpy(), S64, S32)
    # the finish on the REFERENCE's fp32 S, so that its error is its own
    Sd, gd, kd = D(S32.astype(np.float32)), D(gate), D(kg)
    for bias in (None, b3):
        a64 = gr.gate_att(gate, bias, S32.astype(np.float32), kg)
        a32 = gr.gate_att(gate, bias, S32.astype(np.float32), kg, fp32=True)
        att = torch.full((NI, H, W), FILL, device=DEV)
        if bias is None:
            check(lib.df3d_gate_finish(P(gd), P(Sd), P(kd), NI, H, W, P(att), stream()))
        else:
            check(lib.df3d_gate_finish_bias(P(gd), P(dv[6]), P(Sd), P(kd), NI, H, W, P(att), stream()))
        gr.assert_within_yardstick("att %dx%d%s" % (H, W, " +bias" if bias is not None else ""), att.cpu().numpy(), a64, a32)
        assert ((a64 > 0.05) & (a64 < 0.95)).mean() >= 0.75                     # the sigmoid is not saturated: every term counts


def test_gate_module_fold_through_the_kernels():
    """`Basicgate_patch_iv_multivoxel` with voxel_idx (0, 2) and random weights: its folded() matrices through
    df3d_scatter_winner / df3d_gate_rows (both scales into one S) / df3d_gate_finish_bias, against its own forward_batched on
    dense canvases evaluated in float64 on the host; the yardstick is the same dense forward in float32.  Pins the fold
    (tap order, the constant term of the biases, the image summary's weight), not only the kernels that consume it.
    Measured on the MI355X: gated image kernel 1.7e-7, fp32 yardstick 2.5e-7, scale 2.7."""
    from dualfusion.fusion import Basicgate_patch_iv_multivoxel
    lib, check, stream = _lib()
    torch.manual_seed(3)
    chans, Cimg, B, ncam, H, W = [8, 16, 12], 16, 2, 2, 6, 9
    NI = B * ncam
    mod = Basicgate_patch_iv_multivoxel(img_num_channel=Cimg, pts_num_channel=chans[2], voxel_feat_channel=chans, voxel_idx=(0, 2))
    with torch.no_grad():
        for p in mod.parameters():
            p.copy_(torch.randn_like(p) * 0.15)
    T, kg, w3, b3 = mod.folded()
    cases = {idx: gr.glue_case(40 + idx, (60, 45), ncam, H, W, chans[idx], 4, 0.5, out_of_map=True) for idx in (0, 2)}
    for cc in cases.values():
        cc["pinv"] = cc["pinv"] * np.float32(0.02)                       # coordinates of the size of the features
    img = np.random.RandomState(9).standard_normal((NI, Cimg, H, W)).astype(np.float32)
    canv = {}
    S = torch.full((NI, 9, H, W), 7.0, device=DEV)
    for k, (idx, cc) in enumerate(cases.items()):
        wr = gr.winner(cc["ind"], cc["grid"], cc["mask"], B, ncam, H, W)
        assert (wr >= 0).any() and (wr < 0).any()
        canv[idx] = np.zeros((NI, chans[idx] + 3, H, W), np.float32)
        im, y, x = np.nonzero(wr >= 0)
        canv[idx][im, :, y, x] = np.concatenate([cc["feat"], cc["pinv"]], 1)[wr[im, y, x]]
        win = torch.full((NI, H, W), -5, dtype=torch.int32, device=DEV)
        dv = [D(cc[key]) for key in ("ind", "grid", "mask", "feat", "pinv")] + [T[idx].to(DEV).contiguous()]
        check(lib.df3d_scatter_winner(P(dv[0]), P(dv[1]), P(dv[2]), cc["n"], B, ncam, H, W, P(win), stream()))
        assert np.array_equal(win.cpu().numpy(), wr)
        check(lib.df3d_gate_rows(P(dv[3]), chans[idx], P(dv[4]), P(dv[5]), P(win), NI, H, W, P(S), int(k == 0), stream()))
        torch.cuda.synchronize()
    gate = np.einsum("c,nchw->nhw", w3[0].detach().double().numpy(), img.astype(np.float64)).astype(np.float32)   # the summary, bias apart
    att = torch.full((NI, H, W), FILL, device=DEV)
    dv = [D(gate), b3.detach().to(DEV).contiguous(), kg.to(DEV).contiguous()]
    check(lib.df3d_gate_finish_bias(P(dv[0]), P(dv[1]), P(S), P(dv[2]), NI, H, W, P(att), stream()))
    got = img.astype(np.float64) * att.cpu().numpy().astype(np.float64)[:, None]
    with torch.no_grad():
        want32 = mod.forward_batched(torch.from_numpy(img), {i: torch.from_numpy(v) for i, v in canv.items()}).numpy()
        want64 = mod.double().forward_batched(torch.from_numpy(img).double(), {i: torch.from_numpy(v).double() for i, v in canv.items()}).numpy()
    ratio = want64 / np.where(img == 0, 1, img)
    assert ((ratio > 0.05) & (ratio < 0.95)).mean() >= 0.75                  # the sigmoid is not saturated
    gr.assert_within_yardstick("gated image through the fold", got, want64, want32)


# ------------------------------------------------------------------------------------------------------ pixel rows
def run_pixel_rows(ind, grid, mask, n, B, ncam, H, W):
    lib, check, stream = _lib()
    nws = int(lib.df3d_query_pixel_rows_workspace_bytes(B, ncam, H, W))
    ws = torch.empty((nws,), dtype=torch.uint8, device=DEV)
    pixrow = torch.full((B * ncam * H * W,), -5, dtype=torch.int32, device=DEV)
    total = torch.full((1,), -5, dtype=torch.int32, device=DEV)
    check(lib.df3d_query_pixel_rows(P(ind), P(grid), P(mask), n, B, ncam, H, W, P(pixrow), P(total), P(ws), nws, stream()))
    return pixrow.cpu().numpy(), int(total)


def test_query_pixel_rows_against_the_reference():
    """df3d_query_pixel_rows on the slot case (pixels inside the map) and on n = 0: pixrow and total equal -- the rank in
    image-major, row-major order, -1 elsewhere; images of the empty samples carry no pixel."""
    c = slot_case(32, 80)
    d = c["dev"]
    want, total = gr.pixel_rows(c["ind"], c["grid"], c["mask"], c["B"], c["ncam"], c["H"], c["W"])
    got, gtotal = run_pixel_rows(d["ind"], d["grid"], d["mask"], c["n"], c["B"], c["ncam"], c["H"], c["W"])
    assert gtotal == total and 0 < total < want.size and np.array_equal(got, want)
    got, gtotal = run_pixel_rows(None, None, None, 0, 2, 3, 5, 7)
    assert gtotal == 0 and (got == -1).all()


# ------------------------------------------------------------------------------------------------------ projection
def run_project(args, want_depth=True):
    lib, check, stream = _lib()
    n, B, ncam = len(args["indices"]), args["batch"], args["ncam"]
    grid = torch.full((ncam, n, 2), -5, dtype=torch.int32, device=DEV)      # at n = 0: tensors without storage, null pointers
    mask = torch.full((ncam, n), 9, dtype=torch.uint8, device=DEV)
    pinv = torch.full((n, 3), FILL, device=DEV)
    depth = torch.full((ncam, n), FILL, device=DEV) if want_depth else None
    ind = D(args["indices"])
    sp = (ctypes.c_float * 3)(*[float(v) for v in args["scale_xyz"]])
    mp = (ctypes.c_float * 3)(*[float(v) for v in args["pc_min"]])
    aug = D(args["aug_inv"]) if args["aug_inv"] is not None else None
    dv = [D(args[key]) for key in ("lidar2cam", "intrinsic", "raw_hw", "depth_thres", "feat_scale")]    # held until the results are read
    check(lib.df3d_project_voxels(P(ind), n, B, ncam, ctypes.cast(sp, ctypes.c_void_p), ctypes.cast(mp, ctypes.c_void_p),
                                  P(dv[0]), P(dv[1]), P(dv[2]), P(dv[3]), float(args["image_scale"]), P(dv[4]), P(grid), P(mask),
                                  P(pinv), P(depth), P(aug), stream()))
    torch.cuda.synchronize()
    return grid.cpu().numpy(), mask.cpu().numpy(), pinv.cpu().numpy(), depth.cpu().numpy() if want_depth else None


_proj_cache = {}


def _projection_cases(golden):
    if not _proj_cache:
        g = golden("fusion_cp.npz")
        _proj_cache.update(gr.projection_cases([g["coords%d" % i].astype(np.int32) for i in (2, 3, 4)]))
    return _proj_cache


@pytest.mark.parametrize("name", ["level0", "level0_aug", "level1", "level1_aug", "level2", "level2_aug", "empty_middle_aug"])
def test_project_voxels_against_the_reference(golden, name):
    """df3d_project_voxels with depth requested on the golden voxel sets, the second sample's cameras aimed with a yaw offset
    and a focal length of their own, image size and feature scale per (sample, camera), a depth threshold per camera, without
    and with a per-sample inverse augmentation; and three samples with an empty one in the middle.  On the decided pairs
    (tests/test_glue_host.py: >= 97.8 % of them, on which fp32 and float64 agree): mask equal, grid equal where visible,
    depth within the yardstick; grid (0, 0) and depth 0 wherever the kernel masks a pair; point_inv within the yardstick.
    Measured on the MI355X (kernel / fp32 yardstick, scale 10-15): point_inv 8.3e-7 / 8.3e-7 .. 8.6e-7 / 8.6e-7 plain (the same
    two operations) and 1.9e-6 / 1.9e-6 .. 2.1e-6 / 1.6e-6 augmented; depth 1.4e-6 / 1.7e-6 .. 2.5e-6 / 2.5e-6; 97.9-98.2 % of the
    pairs decided, no mask or grid mismatch on any of them."""
    pc = _projection_cases(golden)[name]
    args = gr.project_args(pc)
    g64, m64, p64, d64, decided = gr.project(**args)
    _, _, p32, d32, _ = gr.project(fp32=True, **args)
    grid, mask, pinv, depth = run_project(args)
    assert set(np.unique(mask).tolist()) <= {0, 1}
    assert np.array_equal(mask[decided], m64[decided])
    vis = decided & (m64 != 0)
    assert vis.sum() > 1000 and np.array_equal(grid[vis], g64[vis])
    off = mask == 0
    assert not grid[off].any() and not depth[off].any()
    print("%s: %d pairs, %d decided, %d visible" % (name, decided.size, decided.sum(), vis.sum()))
    gr.assert_within_yardstick(name + " point_inv", pinv, p64, p32)
    gr.assert_within_yardstick(name + " depth", depth[vis], d64[vis], d32[vis])
    # without the depth output the rest is unchanged
    grid2, mask2, pinv2, _ = run_project(args, want_depth=False)
    assert np.array_equal(grid2, grid) and np.array_equal(mask2, mask) and np.array_equal(pinv2, pinv)


def test_project_voxels_strict_inequalities_on_exact_values():
    """Power-of-two focal length, principal point, voxel size and coordinates: u lands exactly on 0, 1, W_raw - 1 and W_raw, v on
    0, 1, H_raw - 1 and H_raw, the depth exactly on its threshold.  Every value is representable, so every pair counts and
    nothing has a margin: 0 < x < W_raw, 0 < y < H_raw and depth > thres are strict."""
    args, want = gr.exact_projection_case()
    g64, m64, p64, d64, _ = gr.project(**args)
    grid, mask, pinv, depth = run_project(args)
    assert np.array_equal(mask[0], want) and np.array_equal(m64[0], want)
    assert np.array_equal(grid, g64) and np.array_equal(pinv, p64.astype(np.float32)) and np.array_equal(depth, d64.astype(np.float32))


# ---------------------------------------------------------------------------------------------------- empty inputs
def test_every_entry_on_an_empty_voxel_set():
    """n = 0 through every entry that accepts it: winner maps -1, canvas and (cleared) S zero, an uncleared S untouched,
    counts zero, query tensors all padding (zeros, qpos 0 / 1), pixrow -1 and total 0, the projection (given the null
    pointers that the tensors of an empty level have) and the write-backs return without a launch."""
    lib, check, stream = _lib()
    B, ncam, H, W, C, Ci, max_ne = 2, 3, 5, 7, 16, 24, 4
    NI = B * ncam
    nul = None
    win = torch.full((NI, H, W), -5, dtype=torch.int32, device=DEV)
    check(lib.df3d_scatter_winner(nul, nul, nul, 0, B, ncam, H, W, P(win), stream()))
    assert bool((win == -1).all())
    win.fill_(-5)
    canvas = torch.full((NI, C + 3, H, W), FILL, device=DEV)
    check(lib.df3d_scatter_to_image(nul, nul, nul, nul, nul, 0, C, B, ncam, H, W, P(win), P(canvas), stream()))
    assert bool((win == -1).all()) and not bool(canvas.any())
    T = torch.zeros((9, C + 3), device=DEV)
    for entry in ("scatter", "rows"):
        for clear in (1, 0):
            S = torch.full((NI, 9, H, W), 7.0, device=DEV)
            win.fill_(-5)
            if entry == "scatter":
                check(lib.df3d_gate_scatter(nul, nul, nul, nul, 0, B, ncam, H, W, P(win), P(S), clear, stream()))
            else:
                check(lib.df3d_gate_scatter_rows(nul, C, nul, P(T), nul, nul, nul, 0, B, ncam, H, W, P(win), P(S), clear, stream()))
            assert bool((win == -1).all()) and bool((S == (0.0 if clear else 7.0)).all()), (entry, clear)
    counts = torch.full((NI,), -7, dtype=torch.int32, device=DEV)
    check(lib.df3d_query_slots(nul, nul, 0, B, ncam, nul, P(counts), stream()))
    assert not bool(counts.any())
    pad = np.zeros((NI, max_ne, C), np.float32)
    pad[:, :, 1::2] = 1
    pad = D(pad)
    pixrow = torch.full((NI * H * W,), -1, dtype=torch.int32, device=DEV)
    compact = torch.zeros((1, Ci), device=DEV)
    table = torch.zeros((NI * max_ne, 4), dtype=torch.int32, device=DEV)
    img = torch.zeros((NI, Ci, H, W), device=DEV)
    dims = (0, C, Ci, B, ncam, H, W, max_ne)
    six = (nul,) * 6
    for entry in ("queries", "queries2", "queries2_counts", "slots", "compact"):
        for use_qpos in (False, True):
            outs = [torch.full((NI, max_ne, k), FILL, device=DEV) for k in (C, Ci, 2, 3, C)]
            o4 = tuple(P(o) for o in outs[:4])
            qpos = P(outs[4]) if use_qpos else None
            if entry == "queries":
                check(lib.df3d_assemble_queries(*six, P(img), *dims, *o4, stream()))
            elif entry in ("queries2", "queries2_counts"):
                check(lib.df3d_assemble_queries2(*six, P(img), nul, nul, *dims, *o4, qpos,
                                                 P(counts) if entry == "queries2_counts" else None, stream()))
            elif entry == "slots":
                check(lib.df3d_assemble_queries2_slots(*six, P(img), nul, nul, *dims, *o4, qpos, P(counts), P(table), nul, nul,
                                                       stream()))
            else:
                check(lib.df3d_assemble_queries2_compact(*six, P(pixrow), P(compact), nul, *dims, *o4, qpos, P(counts), stream()))
            assert not any(bool(o.any()) for o in outs[:4]), entry
            if use_qpos and entry != "queries":
                assert torch.equal(outs[4], pad), entry
    got, total = run_pixel_rows(None, None, None, 0, B, ncam, H, W)
    assert total == 0 and (got == -1).all()
    out = torch.full((1, C), FILL, device=DEV)
    check(lib.df3d_fusion_writeback(nul, nul, nul, nul, nul, 0, C, ncam, max_ne, P(out), stream()))
    check(lib.df3d_fusion_writeback_split(nul, nul, nul, nul, nul, 0, C, ncam, max_ne, P(out), nul, stream()))
    assert bool((out == FILL).all())
    args, _ = gr.exact_projection_case()
    args["indices"] = args["indices"][:0]
    grid, mask, pinv, depth = run_project(args)                             # the null pointers an empty level's tensors have
    assert grid.shape == (1, 0, 2) and mask.size == 0 and pinv.size == 0 and depth.size == 0
    torch.cuda.synchronize()


if __name__ == "__main__":
    assert sys.argv[1:] == ["assemble"], sys.argv
    for _C, _Ci in CHANNEL_PAIRS:
        assembly_sweep(_C, _Ci, ("queries2_counts",), [(True, True), (False, False)])
    print("assembly child ok (DF3D_ASSEMBLE=%s)" % os.environ.get("DF3D_ASSEMBLE"))
