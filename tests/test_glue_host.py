"""The host reference of the camera-fusion glue (tests/glue_reference.py) checked on its own, CPU only: before
tests/test_gpu_glue.py measures the kernels of csrc/fusion.hip against it, it has to reproduce what the port of the adapter
(`oracle_models.centerpoint_fusion_torch`, pinned to the reference module by tests/golden/fusion_cp.npz) holds per sample and
camera on the golden inputs, and the projection cases of the GPU test have to stay inside the conditions their comparison
rests on: few undecided (camera, voxel) pairs, and an fp32 evaluation that agrees with float64 on every decided one."""
import numpy as np
import pytest
import torch

import f64_reference as fr
import glue_reference as gr
import oracle_models as om

UNDECIDED_CAP = 0.05


@pytest.fixture(scope="module")
def case(golden):
    return fr.cp_fusion_case(golden("fusion_cp.npz"))


def golden_project_args(case, level):
    """df3d_project_voxels' arguments for one level of the golden geometry, as the adapter builds them."""
    from dualfusion import synth
    from make_golden import FUS
    cams, B = synth.NUSC_CAMS, FUS["batch"]
    (H, W), (h, w) = FUS["img_hw"], FUS["feat_hw"]
    return dict(indices=case["sets"][level], batch=B, ncam=len(cams),
                scale_xyz=np.asarray(FUS["voxel_size"], np.float32) * np.float32((2, 4, 8)[level]),
                pc_min=np.asarray(FUS["pc_range"][:3], np.float32),
                lidar2cam=np.stack([case["calib"][c][0] for c in cams], 1), intrinsic=np.stack([case["calib"][c][1] for c in cams], 1),
                raw_hw=np.tile(np.array([H, W], np.int32), (B, len(cams), 1)),
                depth_thres=np.asarray([FUS["depth_thres"][c] for c in cams], np.float32),
                image_scale=np.float32(FUS["image_scale"]), feat_scale=np.tile(np.float32([w / W, h / H]), (B, len(cams), 1)))


@pytest.fixture(scope="module")
def ports(case):
    """The port in float32 and in float64 on the golden inputs: what it holds per (sample, camera) (`debug`), the rows its
    encoder returned and its output.  The encoder runs in the float32 evaluation only (the float64 one is here for the
    gated image features, which lie in front of it)."""
    from dualfusion import synth
    from make_golden import FUS
    real = om.actr_forward_torch
    runs = {}
    for dt in (torch.float32, torch.float64):
        seen = {}

        def spy(P, v_feat, grid, imgs, pts, v_i, **kw):
            enh = real(P, v_feat, grid, imgs, pts, v_i, **kw) if v_feat.dtype == torch.float32 else torch.zeros_like(v_feat)
            seen.update(enh=enh, v_feat=v_feat, v_i=v_i, grid=grid, pts=pts)
            return enh
        om.actr_forward_torch = spy
        try:
            with torch.no_grad():
                P = {k: torch.from_numpy(v).to(dt) for k, v in case["sd"].items()}
                levels = [(s, torch.from_numpy(f).to(dt)) for s, f in zip(case["sets"], case["feats"])]
                img = {n: torch.from_numpy(v).to(dt) for n, v in case["img"].items()}
                dbg = {}
                out, _ = om.centerpoint_fusion_torch(P, levels, img, case["calib"], FUS["img_hw"], synth.NUSC_CAMS, FUS["voxel_size"],
                                                     FUS["pc_range"], FUS["image_scale"], fr.cp_depth_thres(), debug=dbg)
        finally:
            om.actr_forward_torch = real
        runs[dt] = dict(per=dbg["per"], out=out.numpy(), **{k: v.numpy() for k, v in seen.items()})
    return runs


def fold64(sd, voxel_idx=(0, 2)):
    """`Basicgate_patch_iv_multivoxel._fold` restated in float64 on the state dict: T {scale: [9, C_s + 3]}, kg [19]
    (k_t, g_t, bias), the image summary's weight [Cimg] and bias."""
    f = lambda k: np.asarray(sd["ifat." + k], np.float64)                            # noqa: E731
    last = voxel_idx[-1]
    R2 = f("reduced_dim2.weight")[:, :, 0, 0]
    Wsb = f("spatial_basic.weight")[0].transpose(1, 2, 0).reshape(9, -1)              # [tap, channel]
    const = f("reduced_dim2.bias").copy()
    T = {}
    for idx in voxel_idx:
        if len(voxel_idx) > 1 and idx != last:
            T[idx] = Wsb @ (R2 @ f("reduced_dim.%d.weight" % idx)[:, :, 0, 0])
            const = const + R2 @ f("reduced_dim.%d.bias" % idx)
        else:
            T[idx] = Wsb @ R2
    kg = np.concatenate([Wsb @ const, Wsb.sum(1), f("spatial_basic.bias").reshape(1)])
    return T, kg, f("reduced_dim3.weight")[0, :, 0, 0], f("reduced_dim3.bias")[0]


def test_reference_reproduces_the_port_on_the_golden_inputs(case, ports):
    """Per (sample, camera) of fusion_cp.npz the reference holds what the port holds: grid, mask and corner points of the
    visible rows and the assembled voxel rows equal; the gated image features at the query pixels (gate_S -> gate_att ->
    assemble, float64, the fold restated here) within four times the gap between the port's own float32 and float64
    evaluations (measured: 3.0e-8 against a gap of 5.1e-7); the write-back of the port's encoder rows bit-equal to its output."""
    from dualfusion import synth
    from make_golden import FUS
    B, ncam = FUS["batch"], len(synth.NUSC_CAMS)
    h, w = FUS["feat_hw"]
    p32, p64 = ports[torch.float32], ports[torch.float64]
    ind = case["sets"][2]
    proj = {li: gr.project(**golden_project_args(case, li)) for li in (0, 2)}
    grid, mask, pinv, _, _ = proj[2]
    pinv32 = gr.project(fp32=True, **golden_project_args(case, 2))[2]
    pos, counts = gr.slots(mask, ind, B, ncam)
    max_ne = int(counts.max())
    # the gate: both scales into one S, the image summary with its bias, the sigmoid
    T, kg, w3, b3 = fold64(case["sd"])
    img = np.stack([case["img"][c][b] for b in range(B) for c in synth.NUSC_CAMS])           # image index = b * ncam + cam
    S = None
    for li in (0, 2):
        g_l, m_l, p_l = proj[li][:3]
        win = gr.winner(case["sets"][li], g_l, m_l, B, ncam, h, w)
        S = gr.gate_S(case["feats"][li], p_l, T[li], win, S is None, S)
    gate = np.einsum("c,nchw->nhw", w3, img.astype(np.float64))
    att = gr.gate_att(gate, np.array([b3]), S, kg)
    q = gr.assemble(case["feats"][2], pinv, ind, grid, mask, pos, img, B, ncam, h, w, max_ne, att=att)
    assert max_ne == p32["v_feat"].shape[1]
    worst = gap = 0.0
    for b in range(B):
        rows = np.nonzero(ind[:, 0] == b)[0]
        for ci in range(ncam):
            per, i = p32["per"][(b, ci)], b * ncam + ci
            m = mask[ci, rows] != 0
            k = int(m.sum())
            assert k == counts[i] and np.array_equal(m, per["mask"].numpy())
            assert np.array_equal(grid[ci, rows][m], per["grid"].numpy())
            assert np.array_equal(pinv32[rows][m], per["pts"].numpy())
            assert np.array_equal(q["v_feat"][i, :k], per["feat"].numpy()) and not q["v_feat"][i, k:].any()
            want = p64["per"][(b, ci)]["ifeat"].numpy()
            worst = max(worst, float(np.abs(q["v_i_feat"][i, :k] - want).max()))
            gap = max(gap, float(np.abs(per["ifeat"].numpy().astype(np.float64) - want).max()))
            assert not q["v_i_feat"][i, k:].any() and not q["qgrid"][i, k:].any()
    print("gated image features at the query pixels: reference %.3g off the float64 port, the port's fp32 gap %.3g" % (worst, gap))
    assert worst <= 4.0 * gap, (worst, gap)
    # the padded tensors as the port stacks them (its grid is the float32 division)
    q32 = gr.assemble(case["feats"][2], pinv32, ind, grid, mask, pos, img, B, ncam, h, w, max_ne, fp32=True)
    assert np.array_equal(q32["qgrid"], p32["grid"]) and np.array_equal(q32["qpts"], p32["pts"])
    assert np.array_equal(q32["v_feat"], p32["v_feat"])
    # the write-back of the rows the port's encoder returned
    assert float(np.abs(p32["enh"]).max()) > 0.1
    assert np.array_equal(gr.writeback(case["feats"][2], p32["enh"], ind, mask, pos, max_ne), p32["out"])


def _decided_share(name, res):
    decided = res[4]
    share = 1.0 - float(decided.mean()) if decided.size else 0.0
    print("%s: %d pairs, %.2f %% undecided" % (name, decided.size, 100 * share))
    assert share <= UNDECIDED_CAP, (name, share)
    return decided


def test_golden_geometry_is_decided_and_fp32_agrees(case):
    """The golden geometry, all three levels: 2.07 % of the 324,258 (camera, voxel) pairs are undecided under the 64-ulp
    rule, and the fp32 port `centerpoint_projection` equals the float64 evaluation on every decided pair (measured: on
    every pair), as does the reference's own fp32 evaluation."""
    from dualfusion import synth
    from make_golden import FUS
    disagree = 0
    for li, d in enumerate((2, 4, 8)):
        args = golden_project_args(case, li)
        ind = args["indices"]
        g64, g32 = gr.project(**args), gr.project(fp32=True, **args)
        decided = _decided_share("golden level %d" % li, g64)
        port = om.centerpoint_projection([(ind, None)], case["calib"], FUS["img_hw"], FUS["feat_hw"], synth.NUSC_CAMS,
                                         FUS["voxel_size"], FUS["pc_range"], FUS["image_scale"], fr.cp_depth_thres(), d_factors=(d,))
        for ci in range(args["ncam"]):
            for b in range(args["batch"]):
                sel = ind[:, 0] == b
                gp, mp, _ = [t.numpy() for t in port[(0, ci)][b]]
                for grid, mask in (g64[:2], g32[:2]):
                    m = mask[ci, sel] != 0
                    bad = (m != mp) | (mp & (grid[ci, sel] != gp).any(1))
                    disagree += int((bad & decided[ci, sel]).sum())
    print("golden geometry: %d disagreements on decided pairs" % disagree)
    assert disagree == 0


def test_projection_cases_are_decided_and_fp32_agrees(case):
    """The conditions of tests/test_gpu_glue.py's projection cases, asserted before a GPU is involved: at most 5 % of the
    pairs undecided (measured 1.8-2.0 %), and zero disagreements between an fp32 evaluation and float64 on the decided pairs.
    The fp32 evaluation is the port `centerpoint_projection`, called per (sample, camera) because it takes one image size and
    no augmentation -- and, on the augmented cases, the reference's own float32 evaluation of the same formula, which the
    cases without augmentation tie to the port (equal on every decided pair).  No seed or angle had to be changed."""
    for name, pc in gr.projection_cases(case["sets"]).items():
        args = gr.project_args(pc)
        ind = args["indices"]
        g64, g32 = gr.project(**args), gr.project(fp32=True, **args)
        decided = _decided_share(name, g64)
        assert g64[1].any(axis=1).all(), name                               # every camera sees something
        bad = (g64[1] != g32[1]) | ((g64[1] != 0) & (g64[0] != g32[0]).any(2))
        disagree = int((bad & decided).sum())
        if args["aug_inv"] is None:
            d = int(round(float(args["scale_xyz"][0]) / gr.PROJ_VOXEL[0]))
            for b in range(args["batch"]):
                sel = ind[:, 0] == b
                ind_b = ind[sel].copy()
                ind_b[:, 0] = 0
                for ci in range(args["ncam"]):
                    port = om.centerpoint_projection([(ind_b, None)], {ci: (args["lidar2cam"][b:b + 1, ci], args["intrinsic"][b:b + 1, ci])},
                                                     tuple(args["raw_hw"][b, ci]), tuple(pc["feat_hw"][b, ci]), [ci], gr.PROJ_VOXEL,
                                                     gr.PROJ_RANGE, gr.PROJ_IMAGE_SCALE, {ci: float(args["depth_thres"][ci])},
                                                     d_factors=(d,))
                    gp, mp, _ = [t.numpy() for t in port[(0, 0)][0]]
                    m = g64[1][ci, sel] != 0
                    bad = (m != mp) | (mp & (g64[0][ci, sel] != gp).any(1))
                    disagree += int((bad & decided[ci, sel]).sum())
        print("%s: %d fp32-versus-float64 disagreements on decided pairs" % (name, disagree))
        assert disagree == 0, name


def test_exact_projection_case_is_exact():
    """The power-of-two case: float64 and float32 evaluate it to the same integers and the expected visibility, with u, v on
    0, 1, size - 1 and size and the depth on its threshold."""
    args, want = gr.exact_projection_case()
    for fp32 in (False, True):
        grid, mask, _, depth, _ = gr.project(fp32=fp32, **args)
        assert np.array_equal(mask[0], want), mask
        assert np.array_equal(grid[0][want == 1], [[0, 8], [31, 8], [16, 0], [16, 15], [16, 8]])
        assert not grid[0][want == 0].any() and not depth[0][want == 0].any()


def test_reference_pieces_agree_with_brute_force():
    """winner / slots / pixel_rows / writeback / gate_att against loops written from the contract's sentences, on a slot
    case small enough to loop over (and with out-of-map pixels for the winner map)."""
    c = gr.glue_case(3, (5, 0, 70, 33), 3, 4, 6, 8, 8, 0.5, out_of_map=True)
    B, ncam, H, W, n = c["B"], c["ncam"], c["H"], c["W"], c["n"]
    win = np.full((B * ncam, H, W), -1)
    pos, counts = np.zeros((ncam, n), np.int64), np.zeros(B * ncam, np.int64)
    for cam in range(ncam):
        for i in range(n):
            b = c["ind"][i, 0]
            pos[cam, i] = counts[b * ncam + cam]
            if c["mask"][cam, i]:
                counts[b * ncam + cam] += 1
                x, y = c["grid"][cam, i]
                if 0 <= x < W and 0 <= y < H:
                    win[b * ncam + cam, y, x] = i                          # rows in order: the last writer stays
    assert np.array_equal(gr.winner(c["ind"], c["grid"], c["mask"], B, ncam, H, W), win) and (win >= 0).any()
    rpos, rcounts = gr.slots(c["mask"], c["ind"], B, ncam)
    assert np.array_equal(rpos, pos) and np.array_equal(rcounts, counts)
    c = gr.glue_case(3, (5, 0, 70, 33), 3, 4, 6, 8, 8, 0.5)
    pixrow, total = gr.pixel_rows(c["ind"], c["grid"], c["mask"], B, ncam, H, W)
    seen = sorted({(int(c["ind"][i, 0]) * ncam + cam, int(c["grid"][cam, i, 1]), int(c["grid"][cam, i, 0]))
                   for cam in range(ncam) for i in range(n) if c["mask"][cam, i]})
    assert total == len(seen) and (pixrow >= 0).sum() == total
    assert all(pixrow[(im * H + y) * W + x] == r for r, (im, y, x) in enumerate(seen))
    rpos, rcounts = gr.slots(c["mask"], c["ind"], B, ncam)
    max_ne = int(rcounts.max()) // 2
    enh = np.random.RandomState(0).standard_normal((B * ncam, max_ne, 8)).astype(np.float32)
    out = c["feat"].copy()
    for i in range(n):
        for cam in range(ncam):
            if c["mask"][cam, i] and rpos[cam, i] < max_ne:
                out[i] = out[i] + enh[c["ind"][i, 0] * ncam + cam, rpos[cam, i]]
    assert np.array_equal(gr.writeback(c["feat"], enh, c["ind"], c["mask"], rpos, max_ne), out)
    rs = np.random.RandomState(1)
    gate, S, kg = rs.standard_normal((2, 3, 3)), rs.standard_normal((2, 9, 3, 3)), rs.standard_normal(19)
    att = gr.gate_att(gate, np.array([0.25]), S, kg)
    for y in range(3):
        for x in range(3):
            acc = kg[18]
            for ty in range(3):
                for tx in range(3):
                    yy, xx = y + ty - 1, x + tx - 1
                    if 0 <= yy < 3 and 0 <= xx < 3:
                        acc += kg[ty * 3 + tx] + kg[9 + ty * 3 + tx] * (gate[1, yy, xx] + 0.25) + S[1, ty * 3 + tx, yy, xx]
            assert abs(att[1, y, x] - 1 / (1 + np.exp(-acc))) < 1e-14
