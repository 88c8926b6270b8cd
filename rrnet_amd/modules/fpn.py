"""modules/fpn.py:5-51 of the reference: three 1x1 lateral convolutions, two top-down merges (bilinear resize to the
lateral map's size + add: one kernel, RF.bilinear_add) and two 3x3 output convolutions.  Same attribute names, so the
`state_dict` keys are the reference's.  `in_channels` (builder-defined; the reference hard-codes ResNet's widths, the default) names
the widths of (c3, c4, c5) for a backbone of other widths: lat_layer3, lat_layer2 and lat_layer1 take them in that order."""
import torch.nn as nn

from rrnet_amd import functional as RF


class FPN(nn.Module):
    def __init__(self, in_channels=(512, 1024, 2048)):
        super().__init__()
        c3, c4, c5 = (int(c) for c in in_channels)
        self.lat_layer1 = nn.Conv2d(c5, 256, kernel_size=1, stride=1, padding=0)
        self.lat_layer2 = nn.Conv2d(c4, 256, kernel_size=1, stride=1, padding=0)
        self.lat_layer3 = nn.Conv2d(c3, 256, kernel_size=1, stride=1, padding=0)
        self.top_layer1 = nn.Conv2d(256, 256, kernel_size=3, stride=1, padding=1)
        self.top_layer2 = nn.Conv2d(256, 256, kernel_size=3, stride=1, padding=1)

    @staticmethod
    def upsample_add(x, y):
        """F.interpolate(x, size(y), mode='bilinear', align_corners=False) + y (:39-40): any sizes, odd maps included."""
        return RF.bilinear_add(x, y)

    def forward(self, c3, c4, c5):
        p5 = RF.conv_bias(c5, self.lat_layer1)
        p5_up, p5_out = RF.fanout(p5, 2)                  # p5 feeds the merge and leaves as the coarsest level
        p4 = RF.conv_bias(self.upsample_add(p5_up, RF.conv_bias(c4, self.lat_layer2)), self.top_layer1)
        p4_up, p4_out = RF.fanout(p4, 2)
        p3 = RF.conv_bias(self.upsample_add(p4_up, RF.conv_bias(c3, self.lat_layer3)), self.top_layer2)
        return p3, p4_out, p5_out
