"""backbones/shufflenet.py of the reference (ShuffleNetV2): InvertedResidual (:48-110, both `benchmodel`s) and ShuffleNetV2
(:113-172) with the reference's constructor signatures, attribute names (`banch1`, `banch2`, `features`, `conv_last`) and
construction order, so that the `state_dict` keys, the default initialisation under a seed and the published checkpoints
are the reference's.  The nn.Sequential members are parameter holders: the forward runs the fused layers of
rrnet_amd.functional — the dense 1x1 / 3x3 convolutions with their BatchNorm (conv_bn_act), the depthwise 3x3 with its
BatchNorm (dwconv_bn, csrc/depthwise.hip) and the channel shuffle as one interleaving pass (shuffle_cat).

forward returns (os8, os16, os32), the three strides modules/fpn.py merges; `out_channels` names their widths.  The map
sizes equal ResNet's for every input size (stem 3x3 / 2 / 1, pool 3x3 / 2 / 1), so RetinaNet's anchors fit unchanged."""
import os
import warnings

import torch
import torch.nn as nn

from rrnet_amd import functional as RF

__all__ = ['shufflenet_v2']

# file names of the published checkpoints (:9-12 of the reference, without its author's home directory)
models = {
    '0.5': './shufflenetv2_x0.5_60.646_81.696.pth',
    '1.0': './shufflenetv2_x1_69.402_88.374.pth',
}


def conv_bn(inp, oup, stride):
    return nn.Sequential(
        nn.Conv2d(inp, oup, 3, stride, 1, bias=False),
        nn.BatchNorm2d(oup),
        nn.ReLU(inplace=True)
    )


def conv_1x1_bn(inp, oup):
    return nn.Sequential(
        nn.Conv2d(inp, oup, 1, 1, 0, bias=False),
        nn.BatchNorm2d(oup),
        nn.ReLU(inplace=True)
    )


def _pw_dw_pw(seq, x):
    """pw -> BN -> ReLU -> dw -> BN -> pw-linear -> BN -> ReLU (`banch2`, :59-71,83-95)."""
    x = RF.conv_bn_act(x, seq[0], seq[1], relu=True)
    x = RF.dwconv_bn(x, seq[3], seq[4])
    return RF.conv_bn_act(x, seq[5], seq[6], relu=True)


def _dw_pw(seq, x):
    """dw -> BN -> pw-linear -> BN -> ReLU (`banch1`, :73-81)."""
    x = RF.dwconv_bn(x, seq[0], seq[1])
    return RF.conv_bn_act(x, seq[2], seq[3], relu=True)


class InvertedResidual(nn.Module):
    def __init__(self, inp, oup, stride, benchmodel):
        super(InvertedResidual, self).__init__()
        self.benchmodel = benchmodel
        self.stride = stride
        assert stride in [1, 2]

        oup_inc = oup // 2

        if self.benchmodel == 1:
            self.banch2 = nn.Sequential(
                # pw
                nn.Conv2d(oup_inc, oup_inc, 1, 1, 0, bias=False),
                nn.BatchNorm2d(oup_inc),
                nn.ReLU(inplace=True),
                # dw
                nn.Conv2d(oup_inc, oup_inc, 3, stride, 1, groups=oup_inc, bias=False),
                nn.BatchNorm2d(oup_inc),
                # pw-linear
                nn.Conv2d(oup_inc, oup_inc, 1, 1, 0, bias=False),
                nn.BatchNorm2d(oup_inc),
                nn.ReLU(inplace=True),
            )
        else:
            self.banch1 = nn.Sequential(
                # dw
                nn.Conv2d(inp, inp, 3, stride, 1, groups=inp, bias=False),
                nn.BatchNorm2d(inp),
                # pw-linear
                nn.Conv2d(inp, oup_inc, 1, 1, 0, bias=False),
                nn.BatchNorm2d(oup_inc),
                nn.ReLU(inplace=True),
            )

            self.banch2 = nn.Sequential(
                # pw
                nn.Conv2d(inp, oup_inc, 1, 1, 0, bias=False),
                nn.BatchNorm2d(oup_inc),
                nn.ReLU(inplace=True),
                # dw
                nn.Conv2d(oup_inc, oup_inc, 3, stride, 1, groups=oup_inc, bias=False),
                nn.BatchNorm2d(oup_inc),
                # pw-linear
                nn.Conv2d(oup_inc, oup_inc, 1, 1, 0, bias=False),
                nn.BatchNorm2d(oup_inc),
                nn.ReLU(inplace=True),
            )

    def forward(self, x):
        if 1 == self.benchmodel:
            # the lower half is handed through in place (a view: the interleave moves it once), the upper half is copied out
            # once for the branch
            x1, x2 = RF.split_halves(x)
            return RF.shuffle_cat(x1, _pw_dw_pw(self.banch2, x2))
        xa, xb = RF.fanout(x, 2)
        return RF.shuffle_cat(_dw_pw(self.banch1, xa), _pw_dw_pw(self.banch2, xb))


class ShuffleNetV2(nn.Module):
    def __init__(self, n_class=1000, input_size=224, width_mult=1.):
        """
        :param n_class:
        :param input_size:
        :param width_mult: [0.5,1.0,1.5,2.0]
        """
        super(ShuffleNetV2, self).__init__()

        assert input_size % 32 == 0

        self.stage_repeats = [4, 8, 4]
        # index 0 is invalid and should never be called.
        # only used for indexing convenience.
        if width_mult == 0.5:
            self.stage_out_channels = [-1, 24, 48, 96, 192, 1024]
        elif width_mult == 1.0:
            self.stage_out_channels = [-1, 24, 116, 232, 464, 1024]
        elif width_mult == 1.5:
            self.stage_out_channels = [-1, 24, 176, 352, 704, 1024]
        elif width_mult == 2.0:
            self.stage_out_channels = [-1, 24, 224, 488, 976, 2048]
        else:
            raise ValueError(
                """{} groups is not supported for
                       1x1 Grouped Convolutions""".format(width_mult))

        # building first layer
        input_channel = self.stage_out_channels[1]
        self.conv1 = conv_bn(3, input_channel, 2)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)

        self.features = []

        # building inverted residual blocks
        for idxstage in range(len(self.stage_repeats)):
            numrepeat = self.stage_repeats[idxstage]
            output_channel = self.stage_out_channels[idxstage + 2]
            for i in range(numrepeat):
                if i == 0:
                    self.features.append(InvertedResidual(input_channel, output_channel, 2, 2))
                else:
                    self.features.append(InvertedResidual(input_channel, output_channel, 1, 1))
                input_channel = output_channel

        # make it nn.Sequential
        self.features = nn.Sequential(*self.features)

        # building last several layers
        self.conv_last = conv_1x1_bn(input_channel, self.stage_out_channels[-1])
        # widths of (os8, os16, os32): what an FPN behind this backbone builds its lateral convolutions from
        self.out_channels = (self.stage_out_channels[2], self.stage_out_channels[3], self.stage_out_channels[-1])

    def forward(self, x):
        x = RF.conv_bn_act(x, self.conv1[0], self.conv1[1], relu=True)
        x = RF.max_pool3x3s2(x)
        os8 = self.features[:4](x)
        os8a, os8b = RF.fanout(os8, 2)
        os16 = self.features[4:12](os8a)
        os16a, os16b = RF.fanout(os16, 2)
        os32 = self.features[12:](os16a)
        os32 = RF.conv_bn_act(os32, self.conv_last[0], self.conv_last[1], relu=True)

        return os8b, os16b, os32


def shufflenet_v2(pretrained=False, width_mult=1.0, weights_path=None):
    """:175-179 of the reference.  Nothing is fetched: a checkpoint on disk is loaded (matching keys and shapes only, as
    backbones/resnet.py does), a missing one leaves the initialisation, loudly."""
    m = ShuffleNetV2(width_mult=width_mult)
    if pretrained:
        if weights_path is None:
            weights_path = models.get(str(width_mult))
        if weights_path and os.path.exists(weights_path):
            own = m.state_dict()
            given = torch.load(weights_path, map_location='cpu')
            given = given.get('state_dict', given) if isinstance(given, dict) else given
            m.load_state_dict({k: v for k, v in given.items() if k in own and v.shape == own[k].shape}, strict=False)
        else:
            warnings.warn("shufflenet_v2: pretrained weights %r not found: the backbone keeps its random initialisation (the "
                          "reference loads a file from its author's disk; nothing is fetched here)" % (weights_path,),
                          RuntimeWarning, stacklevel=3)
    return m
