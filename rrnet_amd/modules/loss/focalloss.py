"""modules/loss/focalloss.py:5-20 (FocalLoss, FocalLossHM)."""
import torch.nn as nn

from .functional import focal_loss, focal_loss_for_hm
from rrnet_amd.functional import focal_loss_hm_from_logits


class FocalLoss(nn.Module):
    def __init__(self, gamma=2, ignore=-1):
        super().__init__()
        self.gamma = gamma
        self.ignore = ignore

    def forward(self, input, target):
        return focal_loss(input, target, self.gamma)


class FocalLossHM(nn.Module):
    def forward(self, out, target):
        return focal_loss_for_hm(out, target)

    @staticmethod
    def from_logits(logits, target):
        return focal_loss_hm_from_logits(logits, target)
