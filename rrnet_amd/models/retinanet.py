"""RetinaNet = ResNet (or, builder-defined, ShuffleNetV2) backbone + FPN + the shared classification / box heads (reference: models/retinanet.py:8-38).
forward returns (loc_pre [N, anchors, 4], cls_pre [N, anchors, num_classes]) over the three pyramid levels, finest first.
Activations are NHWC in memory, so the reference's permute(0,2,3,1).contiguous().view(...) (:27,29) is a view."""
import torch
import torch.nn as nn

from rrnet_amd import functional as RF
from rrnet_amd import ops
from rrnet_amd.detectors.retinanet_detector import RetinaNetDetector
from rrnet_amd.modules.fpn import FPN
from rrnet_amd.utils.model_tools import get_backbone


def _rows(t, width):
    """NHWC map [N, A*width, H, W] -> [N, H*W*A, width] without a copy."""
    t = ops.to_nhwc(t)
    return t.permute(0, 2, 3, 1).reshape(t.size(0), -1, width)


class RetinaNet(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.num_anchors = cfg.Model.num_anchors
        self.num_classes = cfg.num_classes
        self.backbone = get_backbone(cfg.Model.backbone, pretrained=cfg.Train.pretrained)
        # (a backbone that names the widths of its maps — ShuffleNetV2's `out_channels` — gets lateral convolutions to fit)
        widths = getattr(self.backbone, "out_channels", None)
        self.fpn = FPN() if widths is None else FPN(in_channels=tuple(widths)[-3:])
        self.cls = RetinaNetDetector(planes=self.num_anchors * self.num_classes)
        self.loc = RetinaNetDetector(planes=self.num_anchors * 4)

    def forward(self, input):
        input = ops.to_nhwc(input)
        l2, l3, l4 = self.backbone(input)[-3:]            # strides 8, 16, 32: the last three maps (ResNet returns stride 4 too)
        loc_pres, cls_pres = [], []
        for fm in self.fpn(l2, l3, l4):
            fm_loc, fm_cls = RF.fanout(fm, 2)
            loc_pres.append(_rows(self.loc(fm_loc), 4))
            cls_pres.append(_rows(self.cls(fm_cls), self.num_classes))
        return torch.cat(loc_pres, 1), torch.cat(cls_pres, 1)


def build_net(cfg):
    return RetinaNet(cfg)
