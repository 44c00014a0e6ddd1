"""The Voxel-RCNN detector for inference (VR/pcdet/models/detectors/voxel_rcnn.py over detector3d_template.py):
backbone_3d -> map_to_bev -> backbone_2d -> dense_head -> roi_head -> post_processing, on a batch dict that already holds
voxels (as VoxelBackBone8xFusion takes it).  Recall records, training and the losses are not here.

The PV-RCNN detector (VR/pcdet/models/detectors/pv_rcnn.py): backbone_3d -> map_to_bev -> pfe -> backbone_2d -> dense_head ->
point_head -> roi_head, on a batch dict that also holds `points`; eval returns boxes through the same `post_processing`,
training returns the sum of the three heads' losses (get_training_loss, pv_rcnn.py:57-62).

`post_processing` is the class-agnostic branch of Detector3DTemplate.post_processing (detector3d_template.py:251-269).  In
the fused mode (DF3D_VR_TAIL_FUSED, default 1) the RoI decode and the selection of ALL frames are one call with no host round
trip (ops.roi_decode_select, csrc/proposals.hip); the per-frame counts are read back in ONE copy to cut the padded results
into the reference's list of dicts.  The composed mode is the reference's per-frame loop on iou3d_nms.nms_gpu."""
import torch
import torch.nn as nn

from . import backbones, ops, pfe  # noqa: F401 (backbones and pfe register the 3-D backbones and VoxelSetAbstraction)
from .dense_heads import _get, tail_fused
from .registry import BACKBONES_2D, BACKBONES_3D, DENSE_HEADS, DETECTORS_PCDET, MAP_TO_BEV, PFE, ROI_HEADS
from .roi_heads import VoxelRCNNHead, class_agnostic_nms


def _need(cfg, key):
    v = _get(cfg, key)
    if v is None:
        raise KeyError("post_processing: the config has no %s" % key)
    return v


def _selection_args(cfg):
    nms = _need(cfg, "NMS_CONFIG")
    pre, post, thresh = VoxelRCNNHead.check_nms_config(nms, "post_processing")
    return float(_need(cfg, "SCORE_THRESH")), thresh, pre, post, bool(_get(cfg, "OUTPUT_RAW_SCORE", False))


def final_selection(batch_dict, cfg):
    """One ops.roi_decode_select call on rois / rcnn_cls / rcnn_reg: returns batch_box_preds [B, N, 7] and leaves the padded
    results in batch_dict['final_selection'] = (settings, pred_boxes, pred_scores, pred_labels, counts)."""
    args = _selection_args(cfg)
    rois = batch_dict["rois"]
    if rois.shape[1] > ops.TAIL_MAX_CANDIDATES:
        raise NotImplementedError("post_processing: %d RoIs per frame exceed %d, the cap of the top-k select and the NMS"
                                  % (rois.shape[1], ops.TAIL_MAX_CANDIDATES))
    labels = batch_dict["roi_labels"] if batch_dict.get("has_class_labels", False) else None
    box_preds, boxes, scores, out_labels, counts = ops.roi_decode_select(
        rois.contiguous(), batch_dict["rcnn_cls"], batch_dict["rcnn_reg"], labels, args[0], args[1], args[2], args[3], args[4])
    batch_dict["final_selection"] = (args, boxes, scores, out_labels, counts)
    return box_preds


@torch.no_grad()
def post_processing(batch_dict, cfg):
    """-> pred_dicts: one {'pred_boxes' [n, 7], 'pred_scores' [n], 'pred_labels' [n]} per frame."""
    args = _selection_args(cfg)
    score_thresh, thresh, pre, post, raw = args
    batch_size = batch_dict["batch_size"]
    if tail_fused() and "rcnn_reg" in batch_dict and batch_dict["rcnn_reg"].is_cuda:
        hit = batch_dict.get("final_selection")
        if hit is None or hit[0] != args:
            final_selection(batch_dict, cfg)
            hit = batch_dict["final_selection"]
        _, boxes, scores, labels, counts = hit
        counts = counts.tolist()                                              # the one copy of the whole batch
        return [{"pred_boxes": boxes[b, :n], "pred_scores": scores[b, :n], "pred_labels": labels[b, :n]}
                for b, n in enumerate(counts)]
    if batch_dict.get("batch_index", None) is not None:
        raise NotImplementedError("post_processing: stacked predictions (batch_index) are not supported")
    pred_dicts = []
    for index in range(batch_size):
        box_preds = batch_dict["batch_box_preds"][index]
        src_cls_preds = cls_preds = batch_dict["batch_cls_preds"][index]
        if not batch_dict["cls_preds_normalized"]:
            cls_preds = torch.sigmoid(cls_preds)
        cls_preds, label_preds = torch.max(cls_preds, dim=-1)
        if batch_dict.get("has_class_labels", False):
            label_preds = batch_dict["roi_labels" if "roi_labels" in batch_dict else "batch_pred_labels"][index]
        else:
            label_preds = label_preds + 1
        selected = class_agnostic_nms(cls_preds, box_preds, pre, post, thresh, score_thresh=score_thresh)
        final_scores = torch.max(src_cls_preds, dim=-1)[0][selected] if raw else cls_preds[selected]
        pred_dicts.append({"pred_boxes": box_preds[selected], "pred_scores": final_scores, "pred_labels": label_preds[selected]})
    return pred_dicts


def _build_module(model_cfg, registry, key, **kwargs):
    """the module model_cfg[key].NAME names in `registry`, built from that node (pcdet's `__all__[cfg.NAME](model_cfg=cfg, ..)`)"""
    cfg = _need(model_cfg, key)
    cls = registry.get(_need(cfg, "NAME"))
    if cls is None:
        raise KeyError("%s is not in the %s registry" % (_get(cfg, "NAME"), registry.name))
    return cls(model_cfg=cfg, **kwargs)


@DETECTORS_PCDET.register_module
class VoxelRCNN(nn.Module):
    """model_cfg: BACKBONE_3D, MAP_TO_BEV, BACKBONE_2D, DENSE_HEAD, ROI_HEAD (each with its NAME) and POST_PROCESSING."""

    def __init__(self, model_cfg, num_class, class_names, grid_size, point_cloud_range, voxel_size, input_channels=4):
        super().__init__()
        self.model_cfg, self.num_class, self.class_names = model_cfg, num_class, class_names

        def build(registry, key, **kwargs):
            return _build_module(model_cfg, registry, key, **kwargs)

        self.backbone_3d = build(BACKBONES_3D, "BACKBONE_3D", input_channels=input_channels, grid_size=grid_size,
                                 voxel_size=voxel_size, point_cloud_range=point_cloud_range)
        self.map_to_bev_module = build(MAP_TO_BEV, "MAP_TO_BEV", grid_size=grid_size)
        self.backbone_2d = build(BACKBONES_2D, "BACKBONE_2D", input_channels=self.map_to_bev_module.num_bev_features)
        dense_cfg = _need(model_cfg, "DENSE_HEAD")
        self.dense_head = build(DENSE_HEADS, "DENSE_HEAD", input_channels=self.backbone_2d.num_bev_features,
                                num_class=num_class if not _get(dense_cfg, "CLASS_AGNOSTIC", False) else 1,
                                class_names=class_names, grid_size=grid_size, point_cloud_range=point_cloud_range,
                                predict_boxes_when_training=True)
        roi_cfg = _need(model_cfg, "ROI_HEAD")
        self.roi_head = build(ROI_HEADS, "ROI_HEAD", input_channels=self.backbone_3d.num_point_features,
                              backbone_channels=self.backbone_3d.backbone_channels, point_cloud_range=point_cloud_range,
                              voxel_size=voxel_size, num_class=num_class if not _get(roi_cfg, "CLASS_AGNOSTIC", False) else 1)
        self.roi_head.post_process_cfg = _need(model_cfg, "POST_PROCESSING")
        self.module_list = [self.backbone_3d, self.map_to_bev_module, self.backbone_2d, self.dense_head, self.roi_head]

    def forward(self, batch_dict):
        if self.training:
            raise NotImplementedError("VoxelRCNN: the losses of this tail are not implemented; the detector runs in eval mode only")
        for module in self.module_list:
            batch_dict = module(batch_dict)
        return post_processing(batch_dict, self.roi_head.post_process_cfg), {}


@DETECTORS_PCDET.register_module
class PVRCNN(nn.Module):
    """VR/pcdet/models/detectors/pv_rcnn.py.  model_cfg: BACKBONE_3D, MAP_TO_BEV, PFE, BACKBONE_2D, DENSE_HEAD, POINT_HEAD,
    ROI_HEAD (each with its NAME) and POST_PROCESSING; the channel hand-offs are detector3d_template.py:100-173.  The batch
    dict holds voxel_features, voxel_coords, points [N, 1 + input_channels] (b, x, y, z, ..) and batch_size; training adds
    gt_boxes [B, G, 8].

    Eval: `forward` -> (pred_dicts, {}).  Training: `forward` -> ({'loss': loss}, tb_dict, {}) with loss = rpn + point + rcnn.
    The first stage trains through AnchorHeadSingle.forward_train; the RoI head makes its TRAIN proposals from that pass's
    DETACHED predictions (NMS_CONFIG.TRAIN.NMS_PRE_MAXSIZE inside the 4096-candidate cap).  Not provided, refused by name:
    DENSE_HEAD_3D and the auxiliary losses of this fork's backbone (BACKBONE_3D.SEG_LOSS, AUX_PTS_LOSS, AUX_CNS_LOSS)."""

    def __init__(self, model_cfg, num_class, class_names, grid_size, point_cloud_range, voxel_size, input_channels=4):
        super().__init__()
        self.model_cfg, self.num_class, self.class_names = model_cfg, num_class, class_names
        if _get(model_cfg, "DENSE_HEAD_3D", None) is not None:
            raise NotImplementedError("PVRCNN: DENSE_HEAD_3D is not provided")
        for key in ("SEG_LOSS", "AUX_PTS_LOSS", "AUX_CNS_LOSS"):
            if _get(_need(model_cfg, "BACKBONE_3D"), key, None):
                raise NotImplementedError("PVRCNN: BACKBONE_3D.%s is not provided (the auxiliary heads of the backbone have no "
                                          "counterpart here)" % key)

        def build(registry, key, **kwargs):
            return _build_module(model_cfg, registry, key, **kwargs)

        def classes(key):
            return 1 if _get(_need(model_cfg, key), "CLASS_AGNOSTIC", False) else num_class

        self.backbone_3d = build(BACKBONES_3D, "BACKBONE_3D", input_channels=input_channels, grid_size=grid_size,
                                 voxel_size=voxel_size, point_cloud_range=point_cloud_range)
        self.map_to_bev_module = build(MAP_TO_BEV, "MAP_TO_BEV", grid_size=grid_size)
        self.pfe = build(PFE, "PFE", voxel_size=voxel_size, point_cloud_range=point_cloud_range,
                         num_bev_features=self.map_to_bev_module.num_bev_features, num_rawpoint_features=input_channels)
        self.backbone_2d = build(BACKBONES_2D, "BACKBONE_2D", input_channels=self.map_to_bev_module.num_bev_features)
        self.dense_head = build(DENSE_HEADS, "DENSE_HEAD", input_channels=self.backbone_2d.num_bev_features,
                                num_class=classes("DENSE_HEAD"), class_names=class_names, grid_size=grid_size,
                                point_cloud_range=point_cloud_range, predict_boxes_when_training=True)
        before_fusion = _get(_need(model_cfg, "POINT_HEAD"), "USE_POINT_FEATURES_BEFORE_FUSION", False)
        self.point_head = build(DENSE_HEADS, "POINT_HEAD", num_class=classes("POINT_HEAD"), predict_boxes_when_training=True,
                                input_channels=self.pfe.num_point_features_before_fusion if before_fusion
                                else self.pfe.num_point_features)
        self.roi_head = build(ROI_HEADS, "ROI_HEAD", input_channels=self.pfe.num_point_features,
                              backbone_channels=getattr(self.backbone_3d, "backbone_channels", None),
                              point_cloud_range=point_cloud_range, voxel_size=voxel_size, num_class=classes("ROI_HEAD"))
        self.roi_head.post_process_cfg = _need(model_cfg, "POST_PROCESSING")
        self.module_list = [self.backbone_3d, self.map_to_bev_module, self.pfe, self.backbone_2d, self.dense_head,
                            self.point_head, self.roi_head]

    def get_training_loss(self):
        """pv_rcnn.py:57-62 -> (loss, tb_dict, disp_dict); the tb_dict values are detached device tensors"""
        loss_rpn, tb_dict = self.dense_head.get_loss()
        loss_point, tb_dict = self.point_head.get_loss(tb_dict)
        loss_rcnn, tb_dict = self.roi_head.get_loss(tb_dict)
        return loss_rpn + loss_point + loss_rcnn, tb_dict, {}

    def forward(self, batch_dict):
        if not self.training:
            for module in self.module_list:
                batch_dict = module(batch_dict)
            return post_processing(batch_dict, self.roi_head.post_process_cfg), {}
        for module in self.module_list[:4]:
            batch_dict = module(batch_dict)
        batch_dict = self.dense_head.forward_train(batch_dict)
        self.dense_head.write_train_predictions(batch_dict)
        batch_dict = self.point_head(batch_dict)
        self.roi_head.forward_train(batch_dict)
        loss, tb_dict, disp_dict = self.get_training_loss()
        return {"loss": loss}, tb_dict, disp_dict
