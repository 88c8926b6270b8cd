"""Densely connected stacked hourglass on the MI355X kernels.

The reference's backbones/dense_hourglass.py is its hourglass.py plus dense skip sums in HourglassNet.forward (:187-193):
every stack's feature map is convs[i](hgs[i](pre)) + the pre-layer's output + every earlier stack's feature map.  Module
tree, attribute names, construction order and `state_dict()` keys are those of backbones/hourglass.py, so the classes are
the same objects and only the forward differs: the skip rides on the stack's conv -> bn node as its `residual=` (one
earlier tensor) or is one rr_sum_n launch in front of it (several).  The sums need the pre-layer to produce num_feats
channels (2 * stem == inplanes[0] == num_feats), as the reference's hard-coded 128 / 256 / 256 do.

fp32 and cfg.Model.conv_math = "f16x3" are supported; cfg.Model.bf16 is refused by the models
(utils/model_tools.refuse_bf16): `pre` and the features would have to be summed from bf16-only images into tensors that
leave the backbone, so no ops.phantom_scope is opened here.
"""
from rrnet_amd import functional as RF
from rrnet_amd.backbones import hourglass as _hg
from rrnet_amd.backbones.hourglass import HG_TINY, ConvBNRelu, Hourglass, ResidualBlock, _load_pretrained

__all__ = ['HourglassNet', 'Hourglass', 'ResidualBlock', 'ConvBNRelu', 'dense_hourglass_net', 'dense_hourglass_tiny']

# "hourglass-tiny" with the two numbers the dense sums force: the pre-layer's output is added to num_feats = 256 channels
DENSE_TINY = dict(HG_TINY, stem=128, inplanes=(256, 32, 48))


class HourglassNet(_hg.HourglassNet):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        width = self.pre_layer[3].conv2.out_channels
        if width != self.num_feats:
            raise ValueError("dense hourglass: the pre-layer's %d channels are added to the %d-channel features (2 * stem == "
                             "inplanes[0] == num_feats)" % (width, self.num_feats))

    def forward(self, x):
        """-> list of num_stacks pre-ReLU feature maps [B, num_feats, H/4, W/4] (NHWC memory)."""
        stacks = self.num_stacks
        pre = RF.conv_bn_act(x, self.pre_layer[0], self.pre_layer[1], relu=True)
        pre = self.pre_layer[3](pre)
        # the pre-layer's output: the first stack's input (and inter_[0]'s) and one term of every stack's sum
        pre, *pre_terms = RF.fanout(pre, 1 + stacks)
        earlier = []                      # per earlier stack: its feature's views for the later stacks' sums
        outs = []
        for i in range(stacks):
            last = i == stacks - 1
            pa, pb = (pre, None) if last else RF.fanout_shared(pre, 2)[:2]
            hg = self.hgs[i](pa)
            terms = [pre_terms[i]] + [views.pop() for views in earlier]
            skip = terms[0] if len(terms) == 1 else RF.sum_n(terms)
            feat = RF.conv_bn_act(hg, self.convs[i].conv, self.convs[i].bn, relu=False, residual=skip)
            if last:
                outs.append(feat)
                break
            # the feature leaves the backbone, feeds the next stack and is a term of every later stack's sum
            fa, fb, *later = RF.fanout(feat, 2 + (stacks - 1 - i))
            earlier.append(later)
            outs.append(fa)
            a = RF.conv_bn_act(pb, self.inter_[i][0], self.inter_[i][1], relu=False)
            pre = RF.conv_bn_act(RF.relu(fb), self.conv_[i][0], self.conv_[i][1], relu=True, residual=a)
            pre = self.residual[i](pre)
        return outs


def dense_hourglass_net(num_stacks=2, pretrained_path='./hourglass.pth'):
    """backbones/dense_hourglass.py:205-213: './hourglass.pth' loaded with strict=False when it exists; a missing file warns
    and leaves the default initialisation (the policy of backbones/hourglass.hourglass_net)."""
    return _load_pretrained(HourglassNet(num_stacks=num_stacks), pretrained_path, "dense_hourglass_net")


def dense_hourglass_tiny(num_stacks=2):
    return HourglassNet(num_stacks=num_stacks, **DENSE_TINY)
