"""Decode and losses of the NlosPose training/eval callers and of the transformer heads.

Drop-in for the symbols of utils/criterion.py: `softmax_integral_tensor`
(:129-153), `L2JointLocationLoss` (:66-87), `weighted_mse_loss` (:156-162),
`DiceLoss`/`BCEDiceLoss` (:348-385), and the heads' `JointsMSELoss` (:166-270), `JointTarget` (:273-345) and
`NMTNORMCritierion` (:10-63); `get_criterion(cfg)` selects by `cfg.LOSS.TYPE`.  Joint coordinates are returned in heat-map voxel
units, order (x, y, z) = (W-, H-, D-axis expectation), concatenated to (B, 3J); the
[-0.5, 0.5] normalisation is commented out in the reference and is not applied.
"""
from __future__ import annotations

import torch
from torch import nn

from . import hip_ops as ops


def softmax_integral_tensor(preds, num_joints, output_3d, hm_width, hm_height, hm_depth):
    assert output_3d, "Not Implemented!"
    return ops.softmax_integral(preds, num_joints, hm_width, hm_height, hm_depth)


def weighted_mse_loss(input, target, weights, size_average):
    """sum((input - target)^2 * weights) [/ len(input)]  (utils/criterion.py:156-162) in one HIP kernel."""
    return ops.weighted_mse(input, target, weights, size_average)


class L2JointLocationLoss(nn.Module):
    def __init__(self, output_3d, size_average=True, reduce=True):
        super().__init__()
        self.size_average, self.reduce, self.output_3d = size_average, reduce, output_3d

    def forward(self, preds, *args):
        gt_joints, gt_joints_vis = args[0], args[1]
        assert not gt_joints.requires_grad and not gt_joints_vis.requires_grad
        num_joints = int(gt_joints_vis.shape[1] / 3)
        pred = softmax_integral_tensor(preds, num_joints, self.output_3d, preds.shape[-1], preds.shape[-2],
                                       preds.shape[-3])
        return weighted_mse_loss(pred, gt_joints, gt_joints_vis, self.size_average)


class JointsMSELoss(nn.Module):
    """Gaussian heat-map MSE of the 2-D heat-map heads (utils/criterion.py:166-270) in one HIP pass per direction.

    forward(output (B, J, H, W), target (B, J, >= 2), target_weight, writer=None, global_iter_num=None): `target` holds
    (mu_x, mu_y) in heat-map pixels and may live on the host or on the device; H = HEATMAP_SIZE[1], W = HEATMAP_SIZE[0].
    The Gaussian targets are never materialised.  One deviation: the reference overwrites the caller's `target_weight` (a
    host tensor in its loop) with the range flags, which would cost a device-to-host copy per step; here the flags are kept
    in `self.last_target_weight`, a (B, J, 1) device tensor, and the caller's tensor is left alone.  Its incoming values never
    matter in the reference either (they are overwritten before use), so they are not read."""

    def __init__(self, cfg, use_target_weight):
        super().__init__()
        self.use_target_weight = bool(use_target_weight)
        self.num_joints = cfg.DATASET.NUM_JOINTS
        self.target_type = cfg.DATASET.TARGET_TYPE
        self.heatmap_size = cfg.DATASET.HEATMAP_SIZE
        self.sigma = cfg.DATASET.SIGMA
        self.use_different_joints_weight = cfg.DATASET.USE_DIFFERENT_JOINTS_WEIGHT
        self.joints_weight = 1
        self.last_target_weight = None

    def forward(self, output, target, target_weight=None, writer=None, global_iter_num=None):
        assert self.target_type == "gaussian", "Only support gaussian map now!"
        assert output.dim() == 4, "JointsMSELoss: output is (B, J, H, W)"
        hm = self.heatmap_size
        assert tuple(output.shape[-2:]) == (hm[1], hm[0]), \
            f"JointsMSELoss: output maps are {tuple(output.shape[-2:])}, DATASET.HEATMAP_SIZE says (H, W) = ({hm[1]}, {hm[0]})"
        assert not torch.as_tensor(target).requires_grad
        loss, flags = ops.joints_mse(output, target, self.sigma, self.use_target_weight)
        self.last_target_weight = flags.unsqueeze(-1)
        return loss


class JointTarget:
    """Gaussian target maps of one sample (utils/criterion.py:273-345), rendered by hp_joint_heatmaps."""

    def __init__(self, cfg):
        self.num_joints = cfg.DATASET.NUM_JOINTS
        self.target_type = cfg.DATASET.TARGET_TYPE
        self.heatmap_size = cfg.DATASET.HEATMAP_SIZE
        self.sigma = cfg.DATASET.SIGMA * cfg.DATASET.HEATMAP_SIZE[0] // cfg.DATASET.IMAGE_SIZE[0]
        self.use_different_joints_weight = cfg.DATASET.USE_DIFFERENT_JOINTS_WEIGHT
        self.joints_weight = 1

    def generate_target(self, joints, joints_vis):
        """joints, joints_vis (num_joints, >= 2) on the device -> target (J, H, W), target_weight (J, 1): joints_vis[:, 0]
        where any part of the Gaussian truncated at 3 sigma' is in range, else 0; maps with a weight <= 0.5 stay zero."""
        assert self.target_type == "gaussian", "Only support gaussian map now!"
        joints = torch.as_tensor(joints, dtype=torch.float32)
        if not joints.is_cuda:                      # the reference takes host tensors: inputs are moved, nothing is computed there
            joints = joints.to("cuda")
        vis = torch.as_tensor(joints_vis)[:, 0]
        target, flags = ops.joint_heatmaps(joints, self.heatmap_size[1], self.heatmap_size[0], self.sigma, self.sigma * 3, vis)
        if self.use_different_joints_weight:
            flags = flags * self.joints_weight
        return target, flags.unsqueeze(-1)


class NMTNORMCritierion(nn.Module):
    """Loss of the 1-D coordinate classifiers ("SimDR"; utils/criterion.py:10-63): KL divergence between a label-smoothed
    one-hot target and the log-softmax of each axis, weighted per joint, in one HIP pass per direction.

    forward(output_x, output_y, output_z (B, J, bins each; the three may differ), target (B, J, 3), target_weight (B, J),
    (B, J, 1) or None).  Views out[:, :, a, :] of one packed (B, J, 3, bins) tensor are read in place.
    label_smoothing == 0: the reference raises (its NLL branch takes mean(dim=1) of a 1-D tensor); here the formula's limit
    with 0 log 0 = 0 is computed, -log_softmax[label] / bins, which only the float64 model of the tests pins.
    A label outside [0, bins): the reference's scatter_ raises; here no bin receives the confidence (the kernel compares
    the label with the bin index and never indexes by it), the loss stays finite and nothing is checked on the host."""

    def __init__(self, label_smoothing):
        super().__init__()
        if not 0.0 <= float(label_smoothing) < 1.0:
            raise ValueError(f"label_smoothing {label_smoothing} outside [0, 1)")
        self.label_smoothing = float(label_smoothing)
        self.confidence = 1.0 - self.label_smoothing

    def forward(self, output_x, output_y, output_z, target, target_weight=None):
        return ops.simdr_loss(output_x, output_y, output_z, target, target_weight, self.label_smoothing)


def get_criterion(cfg):
    """The criterion `cfg.LOSS.TYPE` names: "L2JointLocationLoss" (NlosPose, the default), "JointsMSELoss" (2-D heat-map
    heads) or "NMTNORMCritierion" (SimDR heads)."""
    kind = cfg.LOSS.TYPE
    if kind == "L2JointLocationLoss":
        return L2JointLocationLoss(output_3d=True)
    if kind == "JointsMSELoss":
        return JointsMSELoss(cfg, cfg.LOSS.USE_TARGET_WEIGHT)
    if kind == "NMTNORMCritierion":
        return NMTNORMCritierion(cfg.LOSS.LABEL_SMOOTHING)
    raise ValueError(f"unknown LOSS.TYPE {kind!r}: L2JointLocationLoss, JointsMSELoss or NMTNORMCritierion")


class DiceLoss(nn.Module):
    def __init__(self, eps: float = 1e-9):
        super().__init__()
        self.eps = eps

    def forward(self, logits, targets):
        p = torch.sigmoid(logits)
        return 1.0 - (2.0 * (p * targets).sum() + self.eps) / (p.sum() + targets.sum())


class BCEDiceLoss(nn.Module):
    """BCEWithLogits(mean) + Dice over the whole batch (one fused reduction).

    `global_batch=True` (data parallelism): the Dice sums are taken over every rank's samples, as the reference's
    single process does over its whole batch (utils/criterion.py:358-368); with gradient averaging over ranks the
    result is exactly the loss and gradient of the concatenated batch (hip_ops._BceDiceGlobal)."""

    def __init__(self, global_batch: bool = False, group=None):
        super().__init__()
        self.global_batch, self.group = global_batch, group

    def forward(self, logits, targets):
        assert logits.shape == targets.shape
        return ops.bce_dice(logits, targets, global_batch=self.global_batch, group=self.group)
