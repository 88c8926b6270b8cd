"""modules/loss/functional.py:6-51 of the reference: `focal_loss` (RetinaNet) and `focal_loss_for_hm` on the fused kernel.

The reference takes `pred` = clamp(sigmoid(logits), 1e-4, 1-1e-4) (operators/rrnet_operator.py:55);
the fused kernel wants the logits, so that sigmoid, clamp, the focal terms and the three global
sums are a single HBM pass.  `focal_loss_for_hm(pred, gt)` keeps the reference signature by
inverting the (monotone) sigmoid; the operators call `focal_loss_hm_from_logits` directly."""
import torch

from rrnet_amd.functional import focal_loss_hm_from_logits


def focal_loss_for_hm(pred, gt):
    p = pred.clamp(1e-4, 1 - 1e-4)
    logits = torch.log(p) - torch.log1p(-p)
    return focal_loss_hm_from_logits(logits, gt)


def focal_loss(cls_preds, cls_targets, gamma=2.0, alpha=0.75):
    """modules/loss/functional.py:6-22: the summed (not averaged) focal loss of logits `cls_preds` against the 0/1 table
    `cls_targets` of the same shape.  This is the dense-table form in tensor operations, for callers that hold such a
    table (and for the host); the training criterion never builds the table: RF.retina_criterion derives the target bit
    from the anchor assignment inside its kernels."""
    p = torch.sigmoid(cls_preds).clamp(1e-7, 1. - 1e-7)
    hot = cls_targets == 1.
    weight = torch.where(hot, torch.full_like(p, alpha), torch.full_like(p, 1. - alpha))
    weight = weight * torch.pow(torch.where(hot, 1. - p, p), gamma)
    cross = -(cls_targets * torch.log(p) + (1.0 - cls_targets) * torch.log(1.0 - p))
    return (weight * cross).sum()
