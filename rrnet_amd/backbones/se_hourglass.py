"""Squeeze-and-excitation hourglass on the MI355X kernels.

Same module tree / attribute names / construction order as the reference's backbones/se_hourglass.py (SELayer :12-27,
ResidualBlock :30-60, ConvBNRelu :64-79, Hourglass :82-142, HourglassNet :145-217), so `state_dict()` keys, default
initialisation under a seed and checkpoints are interchangeable.  What differs from backbones/hourglass.py:

  * the ResidualBlock carries an SELayer between bn2 and the residual add: relu(bn2(conv2(.)) * s + skip) with
    s = sigmoid(W2 relu(W1 mean(.))) per sample and channel.  conv2 -> bn2 stays the ordinary convolution node (relu=False);
    squeeze, excite, scale, add and ReLU are ONE node behind it (functional.se_scale_res_relu, csrc/se.hip);
  * the stem is a stride-1 block followed by MaxPool2d(2) (functional.max_pool2x2);
  * the ConvBNRelu behind every stack keeps its ReLU, so the features come out rectified (RRNet / CenterNet rectify whatever
    the backbone returns: a second ReLU changes nothing).

nn.Linear / nn.AdaptiveAvgPool2d / nn.Sigmoid / nn.MaxPool2d are parameter holders and place holders only.  The sizes are
keyword arguments, as in backbones/hourglass.py.  fp32 and cfg.Model.conv_math = "f16x3" (the convolutions only) are
supported; cfg.Model.bf16 is refused by the models (utils/model_tools.refuse_bf16): no bf16-only activation exists here.
"""
import torch.nn as nn

from rrnet_amd import functional as RF
from rrnet_amd.backbones import hourglass as _hg
from rrnet_amd.backbones.hourglass import HG104, HG_TINY, _blocks, _load_pretrained

__all__ = ['HourglassNet', 'Hourglass', 'ResidualBlock', 'ConvBNRelu', 'SELayer', 'se_hourglass_net', 'se_hourglass_tiny']


class SELayer(nn.Module):
    """Parameter holder of the block's squeeze-and-excitation weights (fc.0: [c/r, c], fc.2: [c, c/r], no biases)."""

    def __init__(self, channel, reduction=16):
        super().__init__()
        self.reduction = reduction
        self.avg_pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Sequential(
            nn.Linear(channel, channel // reduction, bias=False),
            nn.ReLU(inplace=True),
            nn.Linear(channel // reduction, channel, bias=False),
            nn.Sigmoid())

    def forward(self, x):
        raise NotImplementedError("SELayer alone is not on the accelerated path: ResidualBlock.tail runs it fused with the "
                                  "residual add and the ReLU (functional.se_scale_res_relu)")


class ResidualBlock(_hg.ResidualBlock):
    expansion = 2

    def __init__(self, inplanes, planes, stride=1):
        nn.Module.__init__(self)
        self.conv1 = nn.Conv2d(inplanes, planes, kernel_size=3, stride=stride, padding=1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, kernel_size=3, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.se = SELayer(planes, 16)
        self.relu = nn.ReLU(inplace=True)
        projected = stride != 1 or inplanes != planes
        self.skip_connection = nn.Sequential(
            nn.Conv2d(inplanes, planes, (1, 1), stride=stride, bias=False),
            nn.BatchNorm2d(planes)) if projected else nn.Sequential()
        self.stride = stride

    def tail(self, out, skip):
        """relu(se(bn2(conv2(out))) + skip): the convolution node without ReLU, then squeeze / excite / scale / add / ReLU as one node."""
        u = RF.conv_bn_act(out, self.conv2, self.bn2, relu=False)
        return RF.se_scale_res_relu(u, self.se.fc[0].weight, self.se.fc[2].weight, skip, self.se.reduction)


class ConvBNRelu(_hg.ConvBNRelu):
    """backbones/se_hourglass.py:64-79: always with its ReLU."""

    def __init__(self, kernel_size, inplane, plane, stride=1, with_bn=True):
        super().__init__(kernel_size, inplane, plane, stride=stride, with_bn=with_bn, with_relu=True)


class Hourglass(_hg.Hourglass):
    block = ResidualBlock

    make_residual_layer = staticmethod(lambda inplane, plane, layer_num, stride=1: _blocks(inplane, plane, layer_num, stride, block=ResidualBlock))
    make_hg_layer = staticmethod(lambda inplane, plane, layer_num: _blocks(inplane, plane, layer_num, 2, block=ResidualBlock))
    make_reverse_residual_layer = staticmethod(
        lambda inplane, plane, layer_num, stride=1: _blocks(inplane, plane, layer_num, widen_last=True, block=ResidualBlock))


class HourglassNet(nn.Module):
    def __init__(self, num_stacks=2, n=HG104['n'], inplanes=HG104['inplanes'], layer_nums=HG104['layer_nums'],
                 stem=HG104['stem'], num_feats=HG104['num_feats']):
        super().__init__()
        inplanes, layer_nums = list(inplanes), list(layer_nums)
        self.inplanes = stem
        self.num_feats = num_feats
        self.num_stacks = num_stacks
        self.pre_layer = nn.Sequential(
            nn.Conv2d(3, stem, kernel_size=7, stride=2, padding=3, bias=False),
            nn.BatchNorm2d(stem),
            nn.ReLU(inplace=True),
            ResidualBlock(stem, 2 * stem, 1),
            nn.MaxPool2d(2))
        assert 2 * stem == inplanes[0], "the stem's ResidualBlock must produce inplanes[0] channels"
        self.hgs = nn.ModuleList([Hourglass(n, inplanes, layer_nums) for _ in range(num_stacks)])
        self.convs = nn.ModuleList([ConvBNRelu(3, inplanes[0], num_feats) for _ in range(num_stacks)])
        self.residual = nn.ModuleList([ResidualBlock(inplanes[0], inplanes[0]) for _ in range(num_stacks - 1)])
        self.inter_ = nn.ModuleList([nn.Sequential(nn.Conv2d(inplanes[0], inplanes[0], (1, 1), bias=False),
                                                   nn.BatchNorm2d(inplanes[0])) for _ in range(num_stacks - 1)])
        self.conv_ = nn.ModuleList([nn.Sequential(nn.Conv2d(num_feats, inplanes[0], (1, 1), bias=False),
                                                  nn.BatchNorm2d(inplanes[0])) for _ in range(num_stacks - 1)])
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        """-> list of num_stacks rectified feature maps [B, num_feats, H/4, W/4] (NHWC memory)."""
        pre = RF.conv_bn_act(x, self.pre_layer[0], self.pre_layer[1], relu=True)
        pre = RF.max_pool2x2(self.pre_layer[3](pre))
        outs = []
        for i in range(self.num_stacks):
            last = i == self.num_stacks - 1
            pa, pb = (pre, None) if last else RF.fanout_shared(pre, 2)[:2]
            feat = self.convs[i](self.hgs[i](pa))
            if last:
                outs.append(feat)
            else:
                fa, fb = RF.fanout(feat, 2)                 # the feature leaves the backbone and feeds the next stack
                outs.append(fa)
                a = RF.conv_bn_act(pb, self.inter_[i][0], self.inter_[i][1], relu=False)
                pre = RF.conv_bn_act(fb, self.conv_[i][0], self.conv_[i][1], relu=True, residual=a)
                pre = self.residual[i](pre)
        return outs


def se_hourglass_net(num_stacks=2, pretrained_path='./hourglass.pth'):
    """backbones/se_hourglass.py:220-228 (`hourglass_net` there; 'se_hourglass' is this package's name for it in
    utils/model_tools).  The reference loads './hourglass.pth' strictly, which cannot succeed with a plain hourglass file (the
    SE weights are missing); here it is strict=False like the dense network's, and a missing file warns."""
    return _load_pretrained(HourglassNet(num_stacks=num_stacks), pretrained_path, "se_hourglass_net")


def se_hourglass_tiny(num_stacks=2):
    """The SE network at the numbers of "hourglass-tiny" (hidden widths 2 and 3)."""
    return HourglassNet(num_stacks=num_stacks, **HG_TINY)
