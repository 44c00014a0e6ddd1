"""Pieces of mmdetection 2.10.0 (the version TF/README.md:56 pins; the package itself is a pip dependency that is
not vendored under /root/reference and not installed here) which TransFusionHead.loss calls, restated from their
published definitions so that the reference's OWN loss / target-assignment code (transfusion_head.py:1048-1283,
hungarian_assigner.py:100-160) can be imported and run by make_golden.py.  GENERATOR-SIDE ONLY: the fixture holds
the reference module's outputs; nothing here is imported by the product package.

  mmdet/models/losses/utils.py            reduce_loss / weight_reduce_loss / weighted_loss
  mmdet/models/losses/focal_loss.py       FocalLoss (sigmoid form; mmcv's sigmoid_focal_loss op, restated as the
                                          formula its CUDA kernel evaluates: mmcv/ops/csrc/sigmoid_focal_loss_cuda_kernel.cuh)
  mmdet/models/losses/smooth_l1_loss.py   L1Loss
  mmdet/models/losses/gaussian_focal_loss.py  GaussianFocalLoss
  mmdet/core/bbox/match_costs/match_cost.py   FocalLossCost
  mmdet/core/bbox/assigners/assign_result.py  AssignResult (fields only)
  mmdet/core/bbox/samplers/pseudo_sampler.py, sampling_result.py   PseudoSampler / SamplingResult

and, for make_golden_backbones.py (the reference's own SparseEncoder over its own spconv layer):

  mmcv/utils/registry.py                  Registry: register_module() as a decorator, get()
  mmcv/cnn/bricks/conv.py, norm.py        build_conv_layer / build_norm_layer (the 'BN1d' entry)
  mmdet/models/backbones/resnet.py        BasicBlock: the constructor and the norm1 / norm2 properties (the forward is the
                                          reference's own, TF/mmdet3d/ops/sparse_block.py)"""
import torch


def weight_reduce_loss(loss, weight=None, reduction='mean', avg_factor=None):
    if weight is not None:
        loss = loss * weight
    if avg_factor is None:
        return {'none': loss, 'mean': loss.mean(), 'sum': loss.sum()}[reduction]
    if reduction == 'mean':
        return loss.sum() / avg_factor
    if reduction != 'none':
        raise ValueError('avg_factor can not be used with reduction="sum"')
    return loss


def sigmoid_focal_loss_elements(pred, target, gamma, alpha):
    """mmcv SigmoidFocalLoss forward: target [N] class index (== C: background row of zeros)."""
    p = pred.sigmoid()
    flt_min = torch.finfo(torch.float32).tiny
    onehot = torch.zeros_like(pred)
    valid = target < pred.shape[1]
    onehot[valid, target[valid]] = 1.0
    pos = -alpha * (1 - p).pow(gamma) * torch.log(p.clamp(min=flt_min))
    neg = -(1 - alpha) * p.pow(gamma) * torch.log((1 - p).clamp(min=flt_min))
    return onehot * pos + (1 - onehot) * neg


class FocalLoss(torch.nn.Module):
    def __init__(self, use_sigmoid=True, gamma=2.0, alpha=0.25, reduction='mean', loss_weight=1.0):
        super().__init__()
        assert use_sigmoid
        self.use_sigmoid, self.gamma, self.alpha, self.reduction, self.loss_weight = use_sigmoid, gamma, alpha, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        loss = sigmoid_focal_loss_elements(pred.contiguous(), target, self.gamma, self.alpha)
        if weight is not None and weight.shape != loss.shape:
            weight = weight.view(-1, 1) if weight.size(0) == loss.size(0) else weight.view(loss.size(0), -1)
        return self.loss_weight * weight_reduce_loss(loss, weight, reduction_override or self.reduction, avg_factor)


class L1Loss(torch.nn.Module):
    def __init__(self, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.reduction, self.loss_weight = reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        assert pred.size() == target.size() and target.numel() > 0
        return self.loss_weight * weight_reduce_loss(torch.abs(pred - target), weight,
                                                     reduction_override or self.reduction, avg_factor)


class GaussianFocalLoss(torch.nn.Module):
    def __init__(self, alpha=2.0, gamma=4.0, reduction='mean', loss_weight=1.0):
        super().__init__()
        self.alpha, self.gamma, self.reduction, self.loss_weight = alpha, gamma, reduction, loss_weight

    def forward(self, pred, target, weight=None, avg_factor=None, reduction_override=None):
        eps = 1e-12
        pos_weights = target.eq(1)
        neg_weights = (1 - target).pow(self.gamma)
        pos_loss = -(pred + eps).log() * (1 - pred).pow(self.alpha) * pos_weights
        neg_loss = -(1 - pred + eps).log() * pred.pow(self.alpha) * neg_weights
        return self.loss_weight * weight_reduce_loss(pos_loss + neg_loss, weight, reduction_override or self.reduction,
                                                     avg_factor)


class VarifocalLoss(torch.nn.Module):
    """Constructed by the head (loss_iou) but never called (transfusion_head.py:1273-1279 are comments)."""

    def __init__(self, **kw):
        super().__init__()


LOSSES = dict(FocalLoss=FocalLoss, L1Loss=L1Loss, GaussianFocalLoss=GaussianFocalLoss, VarifocalLoss=VarifocalLoss,
              CrossEntropyLoss=VarifocalLoss)


def build_loss(cfg):
    cfg = dict(cfg)
    return LOSSES[cfg.pop('type')](**cfg)


class FocalLossCost(object):
    def __init__(self, weight=1., alpha=0.25, gamma=2, eps=1e-12):
        self.weight, self.alpha, self.gamma, self.eps = weight, alpha, gamma, eps

    def __call__(self, cls_pred, gt_labels):
        cls_pred = cls_pred.sigmoid()
        neg_cost = -(1 - cls_pred + self.eps).log() * (1 - self.alpha) * cls_pred.pow(self.gamma)
        pos_cost = -(cls_pred + self.eps).log() * self.alpha * (1 - cls_pred).pow(self.gamma)
        return (pos_cost[:, gt_labels] - neg_cost[:, gt_labels]) * self.weight


class AssignResult(object):
    def __init__(self, num_gts, gt_inds, max_overlaps, labels=None):
        self.num_gts, self.gt_inds, self.max_overlaps, self.labels = num_gts, gt_inds, max_overlaps, labels


class SamplingResult(object):
    def __init__(self, pos_inds, neg_inds, bboxes, gt_bboxes, assign_result, gt_flags):
        self.pos_inds, self.neg_inds = pos_inds, neg_inds
        self.pos_bboxes, self.neg_bboxes = bboxes[pos_inds], bboxes[neg_inds]
        self.pos_is_gt = gt_flags[pos_inds]
        self.num_gts = gt_bboxes.shape[0]
        self.pos_assigned_gt_inds = assign_result.gt_inds[pos_inds] - 1
        if gt_bboxes.numel() == 0:
            self.pos_gt_bboxes = torch.empty_like(gt_bboxes).view(-1, 4)
        else:
            if len(gt_bboxes.shape) < 2:
                gt_bboxes = gt_bboxes.view(-1, 4)
            self.pos_gt_bboxes = gt_bboxes[self.pos_assigned_gt_inds, :]
        self.pos_gt_labels = assign_result.labels[pos_inds] if assign_result.labels is not None else None


class PseudoSampler(object):
    def __init__(self, **kwargs):
        pass

    def sample(self, assign_result, bboxes, gt_bboxes, **kwargs):
        pos_inds = torch.nonzero(assign_result.gt_inds > 0, as_tuple=False).squeeze(-1).unique()
        neg_inds = torch.nonzero(assign_result.gt_inds == 0, as_tuple=False).squeeze(-1).unique()
        gt_flags = bboxes.new_zeros(bboxes.shape[0], dtype=torch.uint8)
        return SamplingResult(pos_inds, neg_inds, bboxes, gt_bboxes, assign_result, gt_flags)


# ------------------------------------------------------------------------------------------- mmcv builders, mmdet BasicBlock
class Registry(object):
    def __init__(self, name):
        self.name, self.module_dict = name, {}

    def get(self, key):
        return self.module_dict.get(key)

    def register_module(self, name=None, force=False, module=None):
        def _register(cls):
            self.module_dict[name or cls.__name__] = cls
            return cls
        return _register if module is None else _register(module)


CONV_LAYERS = Registry('conv layer')
CONV_LAYERS.register_module('Conv2d', module=torch.nn.Conv2d)
NORM_LAYERS = Registry('norm layer')
NORM_LAYERS.register_module('BN1d', module=torch.nn.BatchNorm1d)     # abbreviation 'bn' (infer_abbr of a _BatchNorm)


def build_conv_layer(cfg, *args, **kwargs):
    cfg_ = dict(type='Conv2d') if cfg is None else cfg.copy()
    layer_type = cfg_.pop('type')
    conv_layer = CONV_LAYERS.get(layer_type)
    if conv_layer is None:
        raise KeyError('Unrecognized norm type %s' % layer_type)
    return conv_layer(*args, **kwargs, **cfg_)


def build_norm_layer(cfg, num_features, postfix=''):
    cfg_ = cfg.copy()
    layer_type = cfg_.pop('type')
    norm_layer = NORM_LAYERS.get(layer_type)
    if norm_layer is None:
        raise KeyError('Unrecognized norm type %s' % layer_type)
    name = 'bn' + str(postfix)
    requires_grad = cfg_.pop('requires_grad', True)
    cfg_.setdefault('eps', 1e-5)
    layer = norm_layer(num_features, **cfg_)
    for param in layer.parameters():
        param.requires_grad = requires_grad
    return name, layer


class BasicBlock(torch.nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, style='pytorch', with_cp=False,
                 conv_cfg=None, norm_cfg=dict(type='BN'), dcn=None, plugins=None):
        super(BasicBlock, self).__init__()
        assert dcn is None and plugins is None
        self.norm1_name, norm1 = build_norm_layer(norm_cfg, planes, postfix=1)
        self.norm2_name, norm2 = build_norm_layer(norm_cfg, planes, postfix=2)
        self.conv1 = build_conv_layer(conv_cfg, inplanes, planes, 3, stride=stride, padding=dilation, dilation=dilation,
                                      bias=False)
        self.add_module(self.norm1_name, norm1)
        self.conv2 = build_conv_layer(conv_cfg, planes, planes, 3, padding=1, bias=False)
        self.add_module(self.norm2_name, norm2)
        self.relu = torch.nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride
        self.dilation = dilation
        self.with_cp = with_cp

    @property
    def norm1(self):
        return getattr(self, self.norm1_name)

    @property
    def norm2(self):
        return getattr(self, self.norm2_name)


class Bottleneck(torch.nn.Module):
    """only named by an import of the reference's sparse_block.py; never built here"""
