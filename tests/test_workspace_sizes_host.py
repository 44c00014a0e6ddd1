"""The workspace sizes of the detection tails and losses without a GPU.  The ..._workspace_bytes entries are host code; their
layouts went from one hand-written carving per unit to `WsLayout` (csrc/common.h) and `partials_bytes` (csrc/loss_terms.h).
Every size below is a literal recorded from the library built at commit ecb63a2 ("Train the Voxel-RCNN RoI head: proposal
targets, RCNN losses on device"), the last one with the hand-written carvings; the configurations it refused (size 0) are
still refused."""
import ctypes

TABLE = [[-1.0, 3.9, 1.6, 1.56, 0.0], [-1.0, 3.9, 1.6, 1.56, 1.57]]
SAMPLER = {"ROI_PER_IMAGE": 16, "FG_RATIO": 0.5, "REG_FG_THRESH": 0.55, "CLS_FG_THRESH": 0.75, "CLS_BG_THRESH": 0.25,
           "CLS_BG_THRESH_LO": 0.1, "HARD_BG_RATIO": 0.8, "CLS_SCORE_TYPE": "roi_iou"}


def sizes(lib):
    """name of the case -> the size the entry returns"""
    from dualfusion import ops
    ref = ctypes.byref
    out = {}

    def anchors(B, sets, pre, H=4, W=6):
        return ops.anchor_cfg(B, H, W, 1, 2, sets, TABLE, max(sets) + 1, 0.78539, 0.0, 0.7, pre, 32)
    for name, cfg in (("b1_1set_pre5", anchors(1, [0, 0], 5)), ("b3_2sets_pre4096", anchors(3, [0, 1], 4096)),
                      ("b3_25x22_pre256", anchors(3, [0, 0], 256, 25, 22)), ("refused_pre4097", anchors(1, [0, 0], 4097)),
                      ("refused_pre0", anchors(1, [0, 0], 0)), ("refused_b0", anchors(0, [0, 0], 5))):
        out["anchor_proposals " + name] = lib.df3d_anchor_proposals_workspace_bytes(ref(cfg))

    for name, args in (("b1_n7_pre5", (1, 7, 5)), ("b3_n300_pre4096", (3, 300, 4096)), ("b3_n300_pre5", (3, 300, 5)),
                       ("refused_n4097", (1, 4097, 5)), ("refused_pre0", (1, 7, 0)), ("refused_pre4097", (1, 7, 4097))):
        B, N, pre = args
        out["roi_decode_select " + name] = lib.df3d_roi_decode_select_workspace_bytes(ref(ops._RoiDecodeCfg(B, N, 1, 0.3, 0.1, pre, 100, 0)))

    def assign(B, M, sets):
        n = max(sets) + 1
        return ops.anchor_assign_cfg(B, 4, 6, M, sets, TABLE, [1] * n, [0.6] * n, [0.45] * n)
    for name, cfg in (("b1_m1_1set", assign(1, 1, [0, 0])), ("b3_m129_2sets", assign(3, 129, [0, 1])), ("b3_m129_1set", assign(3, 129, [0, 0])),
                      ("refused_m1025", assign(1, 1025, [0, 0])), ("refused_m0", assign(1, 0, [0, 0])), ("refused_b0", assign(0, 1, [0, 0]))):
        out["anchor_assign " + name] = lib.df3d_anchor_assign_workspace_bytes(ref(cfg))

    def loss(B, H, W):
        return ops.anchor_loss_cfg(B, H, W, 15, 1, 2, [0, 0], TABLE, 1, 1.0, 2.0, 0.2, [1.0] * 7)
    for name, cfg in (("b1_4x6", loss(1, 4, 6)), ("b3_4x6", loss(3, 4, 6)), ("b3_25x22", loss(3, 25, 22)), ("refused_h0", loss(1, 0, 6)),
                      ("refused_b0", loss(0, 4, 6))):
        out["anchor_loss " + name] = lib.df3d_anchor_loss_workspace_bytes(ref(cfg))

    for name, (B, R) in (("b1_r7", (1, 7)), ("b3_r300", (3, 300)), ("b3_r4096", (3, 4096)), ("refused_b0", (0, 7)), ("refused_r0", (1, 0))):
        out["roi_targets " + name] = lib.df3d_roi_targets_workspace_bytes(ref(ops.roi_target_cfg(B, R, 8, SAMPLER)))
    big = ops.roi_target_cfg(1, 7, 8, SAMPLER)
    big.num_rois = 4097                                            # (roi_target_cfg itself refuses it by name)
    out["roi_targets refused_r4097"] = lib.df3d_roi_targets_workspace_bytes(ref(big))

    spec = ops.RcnnLossSpec(1.0, 1.0, 1.0, [1.0] * 7)
    for name, rows in (("n7", 7), ("n300", 300), ("n3000", 3000), ("refused_n0", 0)):
        out["rcnn_loss " + name] = lib.df3d_rcnn_loss_workspace_bytes(ref(spec.cfg(rows)))

    def head(B, pre, H=4, W=6):
        cfg = ops._HeadCfg()
        cfg.batch, cfg.H, cfg.W, cfg.pre_max, cfg.post_max = B, H, W, pre, 83
        return cfg
    for name, (n, cfg) in (("t1_b1_pre5", (1, head(1, 5))), ("t2_b3_pre4096", (2, head(3, 4096))), ("t6_b3_pre300", (6, head(3, 300))),
                           ("refused_t0", (0, head(1, 5))), ("refused_pre0", (1, head(1, 0))), ("refused_w0", (1, head(1, 5, 4, 0)))):
        out["centerhead_predict " + name] = lib.df3d_centerhead_predict_workspace_bytes(n, ref(cfg))

    for name, args in (("b1_c2_4x6", (1, 2, 4, 6)), ("b3_c10_4x6", (3, 10, 4, 6)), ("b3_c10_25x22", (3, 10, 25, 22)),
                       ("refused_b256", (256, 2, 4, 6)), ("refused_c33", (1, 33, 4, 6)), ("refused_h0", (1, 2, 0, 6))):
        out["heatmap_proposals " + name] = lib.df3d_heatmap_proposals_workspace_bytes(*args)

    for name, args in (("s1_n24_k5", (1, 24, 5)), ("s3_n48_k4096", (3, 48, 4096)), ("s3_n300_k7", (3, 300, 7)),
                       ("refused_k4097", (1, 24, 4097)), ("refused_s0", (0, 24, 5)), ("refused_n0", (1, 0, 5))):
        out["topk_keys " + name] = lib.df3d_topk_keys_workspace_bytes(*args)
    return out


WANT = {
    "anchor_proposals b1_1set_pre5": 68352,
    "anchor_proposals b3_2sets_pre4096": 208640,
    "anchor_proposals b3_25x22_pre256": 291328,
    "anchor_proposals refused_pre4097": 0,
    "anchor_proposals refused_pre0": 0,
    "anchor_proposals refused_b0": 0,
    "roi_decode_select b1_n7_pre5": 68100,
    "roi_decode_select b3_n300_pre4096": 292364,
    "roi_decode_select b3_n300_pre5": 206604,
    "roi_decode_select refused_n4097": 0,
    "roi_decode_select refused_pre0": 0,
    "roi_decode_select refused_pre4097": 0,
    "anchor_assign b1_m1_1set": 1024,
    "anchor_assign b3_m129_2sets": 13312,
    "anchor_assign b3_m129_1set": 11776,
    "anchor_assign refused_m1025": 0,
    "anchor_assign refused_m0": 0,
    "anchor_assign refused_b0": 0,
    "anchor_loss b1_4x6": 256,
    "anchor_loss b3_4x6": 256,
    "anchor_loss b3_25x22": 512,
    "anchor_loss refused_h0": 0,
    "anchor_loss refused_b0": 0,
    "roi_targets b1_r7": 1024,
    "roi_targets b3_r300": 15360,
    "roi_targets b3_r4096": 196608,
    "roi_targets refused_b0": 0,
    "roi_targets refused_r0": 0,
    "roi_targets refused_r4097": 0,
    "rcnn_loss n7": 256,
    "rcnn_loss n300": 256,
    "rcnn_loss n3000": 512,
    "rcnn_loss refused_n0": 0,
    "centerhead_predict t1_b1_pre5": 68608,
    "centerhead_predict t2_b3_pre4096": 15239168,
    "centerhead_predict t6_b3_pre300": 1897728,
    "centerhead_predict refused_t0": 0,
    "centerhead_predict refused_pre0": 0,
    "centerhead_predict refused_w0": 0,
    "heatmap_proposals b1_c2_4x6": 132096,
    "heatmap_proposals b3_c10_4x6": 399616,
    "heatmap_proposals b3_c10_25x22": 525824,
    "heatmap_proposals refused_b256": 0,
    "heatmap_proposals refused_c33": 0,
    "heatmap_proposals refused_h0": 0,
    "topk_keys s1_n24_k5": 66304,
    "topk_keys s3_n48_k4096": 295424,
    "topk_keys s3_n300_k7": 197376,
    "topk_keys refused_k4097": 0,
    "topk_keys refused_s0": 0,
    "topk_keys refused_n0": 0,
}


def test_workspace_sizes_are_those_of_the_hand_written_layouts():
    from dualfusion import _lib
    got = sizes(_lib.bind(ctypes.CDLL(_lib.LIB_PATH), check=False))
    assert sorted(got) == sorted(WANT)
    for name in sorted(WANT):
        assert got[name] == WANT[name], (name, got[name], WANT[name])
        assert (WANT[name] == 0) == ("refused" in name), name
