"""backbones/resnet.py of the reference: Bottleneck (:17-53), used by the stage-2 head of RRNet
(detectors/fasterrcnn_detector.py:10) and by the ResNet backbones of the RetinaNet model (:56-143): same attribute
names, so the `state_dict` keys are the reference's (and torchvision's)."""
import math
import os
import warnings

import torch
import torch.nn as nn

from rrnet_amd import functional as RF


class Bottleneck(nn.Module):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * 4, kernel_size=1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * 4)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x):
        xa, xb = RF.fanout(x, 2)
        out = RF.conv_bn_act(xa, self.conv1, self.bn1, relu=True)
        out = RF.conv_bn_act(out, self.conv2, self.bn2, relu=True)
        residual = self.downsample(xb) if self.downsample is not None else xb
        return RF.conv_bn_act(out, self.conv3, self.bn3, relu=True, residual=residual)


class ResNet(nn.Module):
    """backbones/resnet.py:56-107.  Stem: 7x7 stride-2 convolution + BatchNorm + ReLU (one fused layer), the 3x3 stride-2
    max-pool kernel, then four stages of Bottlenecks; forward returns (l1, l2, l3, l4) at strides 4, 8, 16, 32."""

    def __init__(self, block, layers):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(block, 64, layers[0])
        self.layer2 = self._make_layer(block, 128, layers[1], stride=2)
        self.layer3 = self._make_layer(block, 256, layers[2], stride=2)
        self.layer4 = self._make_layer(block, 512, layers[3], stride=2)
        for m in self.modules():                           # :71-77
            if isinstance(m, nn.Conv2d):
                fan_out = m.kernel_size[0] * m.kernel_size[1] * m.out_channels
                m.weight.data.normal_(0, math.sqrt(2. / fan_out))
            elif isinstance(m, nn.BatchNorm2d):
                m.weight.data.fill_(1)
                m.bias.data.zero_()

    def _make_layer(self, block, planes, blocks, stride=1):
        out_planes = planes * block.expansion
        downsample = None
        if stride != 1 or self.inplanes != out_planes:
            downsample = _Projection(nn.Conv2d(self.inplanes, out_planes, kernel_size=1, stride=stride, bias=False),
                                     nn.BatchNorm2d(out_planes))
        stage = [block(self.inplanes, planes, stride, downsample)]
        self.inplanes = out_planes
        stage += [block(out_planes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*stage)

    def forward(self, x):
        x = RF.conv_bn_act(x, self.conv1, self.bn1, relu=True)
        x = RF.max_pool3x3s2(x)
        l1 = self.layer1(x)
        l1a, l1b = RF.fanout(l1, 2)
        l2 = self.layer2(l1a)
        l2a, l2b = RF.fanout(l2, 2)
        l3 = self.layer3(l2a)
        l3a, l3b = RF.fanout(l3, 2)
        l4 = self.layer4(l3a)
        return l1b, l2b, l3b, l4


class _Projection(nn.Sequential):
    """The residual projection nn.Sequential(conv1x1, BatchNorm) (keys `downsample.0.*`, `downsample.1.*`) as one fused
    conv + BatchNorm layer."""

    def forward(self, x):
        return RF.conv_bn_act(x, self[0], self[1], relu=False)


def _build(layers, pretrained, weights_path):
    model = ResNet(Bottleneck, layers)
    if pretrained:
        # the reference downloads the torchvision weights (:117-118, through backbones/load.py); nothing is fetched here:
        # a file on disk is loaded (matching keys and shapes only), a missing one leaves the initialisation, loudly
        if weights_path and os.path.exists(weights_path):
            own = model.state_dict()
            given = torch.load(weights_path, map_location='cpu')
            model.load_state_dict({k: v for k, v in given.items() if k in own and v.shape == own[k].shape}, strict=False)
        else:
            warnings.warn("resnet: pretrained weights %r not found: the backbone keeps its random initialisation (the "
                          "reference downloads them; nothing is fetched here)" % (weights_path,), RuntimeWarning, stacklevel=3)
    return model


def resnet10(pretrained=False, weights_path='./resnet50.pth'):
    """backbones/resnet.py:110-119 (one Bottleneck per stage; the reference seeds it from the resnet50 weights)."""
    return _build([1, 1, 1, 1], pretrained, weights_path)


def resnet50(pretrained=False, weights_path='./resnet50.pth'):
    return _build([3, 4, 6, 3], pretrained, weights_path)


def resnet101(pretrained=False, weights_path='./resnet101.pth'):
    return _build([3, 4, 23, 3], pretrained, weights_path)
