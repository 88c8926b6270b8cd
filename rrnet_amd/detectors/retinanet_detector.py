"""detectors/retinanet_detector.py:4-15 of the reference: four 3x3 convolutions with ReLU and a 3x3 output convolution,
shared by the pyramid levels.  `detect_layer` keeps the reference's nn.Sequential (keys `detect_layer.{0,2,4,6,8}.*`);
the forward runs each convolution with its bias and ReLU in the kernel's epilogue."""
import torch.nn as nn

from rrnet_amd import functional as RF


class RetinaNetDetector(nn.Module):
    def __init__(self, planes):
        super().__init__()
        layers = []
        for _ in range(4):
            layers += [nn.Conv2d(256, 256, kernel_size=3, stride=1, padding=1), nn.ReLU(True)]
        layers.append(nn.Conv2d(256, planes, kernel_size=3, stride=1, padding=1))
        self.detect_layer = nn.Sequential(*layers)

    def forward(self, x):
        convs = [m for m in self.detect_layer if isinstance(m, nn.Conv2d)]
        for conv in convs[:-1]:
            x = RF.conv_bias(x, conv, relu=True)
        return RF.conv_bias(x, convs[-1])
