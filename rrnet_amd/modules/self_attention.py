"""modules/self_attention.py:7-94 of the reference: a residual context block whose last convolution `W` starts at zero.
Key and query are two conv -> bn -> relu layers each, value one convolution; every pixel attends to the kh x kw dilated
window around it.  Same constructor signature, attribute names and construction order, so `state_dict` keys, the default
initialisation under a seed and checkpoints are the reference's.

The reference unfolds key and value ([b, c, kh*kw, h, w]) and runs products, softmax and weighted sum as torch ops; here
the three are RF.window_attention (csrc/attn.hip).  The device path is built for scale == 1, stride 1 and
padding == dilation * (kernel // 2) per axis: the context then has the input's size and the reference's closing
F.interpolate(.., align_corners=True) is the identity.  Everything else raises NotImplementedError (the 2x2 pool exists, a
bilinear align_corners=True backward does not)."""
from itertools import repeat
from types import SimpleNamespace

import torch
import torch.nn as nn

from rrnet_amd import functional as RF


class SelfAttentionModule(nn.Module):

    def __init__(self, in_channels, key_channels, value_channels,
                 out_channels=None, kernel_size=1, dilation=1, padding=0, stride=1, scale=1):
        super(SelfAttentionModule, self).__init__()
        self.scale = scale
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.key_channels = key_channels
        self.value_channels = value_channels
        self.kernel_size = self._pair(kernel_size)
        self.dilation = self._pair(dilation)
        self.padding = self._pair(padding)
        self.stride = self._pair(stride)
        if out_channels is None:
            self.out_channels = in_channels
        self.pool = nn.MaxPool2d(kernel_size=(scale, scale))
        self.f_key = self._two_layers()
        self.f_query = self._two_layers()
        self.f_value = nn.Conv2d(in_channels=self.in_channels, out_channels=self.value_channels,
                                 kernel_size=1, stride=1, padding=0)
        self.W = nn.Conv2d(in_channels=self.value_channels, out_channels=self.out_channels,
                           kernel_size=1, stride=1, padding=0)
        nn.init.constant_(self.W.weight, 0)
        nn.init.constant_(self.W.bias, 0)

    def _two_layers(self):
        return nn.Sequential(
            nn.Conv2d(in_channels=self.in_channels, out_channels=self.key_channels, kernel_size=1, stride=1, padding=0),
            nn.BatchNorm2d(self.key_channels),
            nn.ReLU(),
            nn.Conv2d(in_channels=self.key_channels, out_channels=self.key_channels, kernel_size=1, stride=1, padding=0),
            nn.BatchNorm2d(self.key_channels),
            nn.ReLU())

    @staticmethod
    def _pair(x):
        if isinstance(x, (list, tuple)):
            return x
        return tuple(repeat(x, 2))

    def check_supported(self):
        """Raises NotImplementedError naming what the device path lacks for this module's geometry."""
        if self.scale != 1:
            raise NotImplementedError("SelfAttentionModule: scale = %r needs the backward of a bilinear align_corners=True "
                                      "resize, which is not built (scale == 1 only)" % (self.scale,))
        if tuple(self.stride) != (1, 1):
            raise NotImplementedError("SelfAttentionModule: stride = %r is not built: the window kernels are stride 1 and the "
                                      "resize back to the input's size (bilinear, align_corners=True) has no backward"
                                      % (tuple(self.stride),))
        centre = tuple(self.dilation[i] * (self.kernel_size[i] // 2) for i in range(2))
        if tuple(self.padding) != centre:
            raise NotImplementedError("SelfAttentionModule: padding = %r != dilation * (kernel_size // 2) = %r changes the map's "
                                      "size, and the bilinear align_corners=True resize back has no backward"
                                      % (tuple(self.padding), centre))
        if any(k % 2 == 0 for k in self.kernel_size):
            raise NotImplementedError("SelfAttentionModule: an even kernel_size %r changes the map's size, and the bilinear "
                                      "align_corners=True resize back has no backward" % (tuple(self.kernel_size),))
        if self.key_channels % 4 or self.value_channels % 4:
            raise NotImplementedError("SelfAttentionModule: key_channels = %d and value_channels = %d must be multiples of 4 "
                                      "(16 bytes per lane along the channels)" % (self.key_channels, self.value_channels))

    @staticmethod
    def _conv_bn_relu(x, conv, bn):
        """conv (with its bias) -> bn -> relu on RF.conv_bn_act, which runs the convolution bias-free.  In training the batch
        mean absorbs the bias: output and every other gradient are unchanged, the bias' own gradient is identically zero (none is
        produced) and only the running mean has to be moved by momentum * bias.  In inference the bias is folded into the
        running mean the layer's coefficients are made from."""
        if conv.bias is None:
            return RF.conv_bn_act(x, conv, bn, relu=True)
        if bn.training:
            out = RF.conv_bn_act(x, conv, bn, relu=True)
            with torch.no_grad():
                bn.running_mean.add_(conv.bias.detach(), alpha=bn.momentum if bn.momentum is not None else 0.1)
            return out
        folded = SimpleNamespace(training=False, weight=bn.weight, bias=bn.bias, running_var=bn.running_var, eps=bn.eps,
                                 momentum=bn.momentum, num_batches_tracked=bn.num_batches_tracked,
                                 running_mean=bn.running_mean - conv.bias.detach())
        return RF.conv_bn_act(x, conv, folded, relu=True)

    def _two(self, layers, x):
        return self._conv_bn_relu(self._conv_bn_relu(x, layers[0], layers[1]), layers[3], layers[4])

    def forward(self, x):
        self.check_supported()
        x_value, x_key, x_query = RF.fanout(x, 3)
        value = RF.conv_bias(x_value, self.f_value)
        key = self._two(self.f_key, x_key)
        query = self._two(self.f_query, x_query)
        context = RF.window_attention(query, key, value, tuple(self.kernel_size), tuple(self.dilation), tuple(self.padding))
        return RF.conv_bias(context, self.W)
