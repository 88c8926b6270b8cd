"""utils/model_tools.py:9-33 of the reference, restricted to the backbones this package carries: the hourglass family of
RRNet / CenterNet — 'hourglass' (configs/rrnet_config.py:80), 'dense_hourglass' (:26-27) and 'se_hourglass' (the reference
ships backbones/se_hourglass.py without a name in its table; the name is this package's), each with a builder-defined
'_tiny' sibling ('hourglass_tiny' is the backbone of BASELINE.json config 1) — and the three ResNets of RetinaNet
(configs/retinanet_config.py:72 -> 'resnet50').  ShuffleNetV2 (backbones/shufflenet.py, which the reference ships without a
name in its table: the names 'shufflenet_v2_x0_5' / '_x1_5' / '_x2_0' and the composition with RetinaNet are this package's)
is a fourth, light backbone for RetinaNet.  The other names ('hrnet', 'hrnetv2', 'trident') load weight files nobody has or
are commented out in the reference itself."""
from rrnet_amd.backbones.dense_hourglass import dense_hourglass_net, dense_hourglass_tiny
from rrnet_amd.backbones.hourglass import hourglass_net, hourglass_tiny
from rrnet_amd.backbones.resnet import resnet10, resnet50, resnet101
from rrnet_amd.backbones.se_hourglass import se_hourglass_net, se_hourglass_tiny
from rrnet_amd.backbones.shufflenet import shufflenet_v2

_RESNETS = {'resnet10': resnet10, 'resnet50': resnet50, 'resnet101': resnet101}
_HOURGLASSES = {'hourglass': hourglass_net, 'hourglass_tiny': hourglass_tiny,
                'dense_hourglass': dense_hourglass_net, 'dense_hourglass_tiny': dense_hourglass_tiny,
                'se_hourglass': se_hourglass_net, 'se_hourglass_tiny': se_hourglass_tiny}
_SHUFFLENETS = {'shufflenet_v2_x0_5': 0.5, 'shufflenet_v2_x1_5': 1.5, 'shufflenet_v2_x2_0': 2.0}      # name -> width_mult
FP32_ONLY_BACKBONES = ('dense_hourglass', 'dense_hourglass_tiny', 'se_hourglass', 'se_hourglass_tiny')


def get_backbone(backbone, pretrained=False, num_stacks=2):
    if backbone in _HOURGLASSES:
        return _HOURGLASSES[backbone](num_stacks=num_stacks)
    if backbone in _RESNETS:
        return _RESNETS[backbone](pretrained=pretrained)
    if backbone in _SHUFFLENETS:
        return shufflenet_v2(pretrained=pretrained, width_mult=_SHUFFLENETS[backbone])
    if backbone == 'shufflenet_v2_x1_0':
        raise NotImplementedError(
            "backbone 'shufflenet_v2_x1_0' is not built: at width 1.0 the units' halves have 58 channels, and the BatchNorm "
            "backward kernels (rr_bn_bwd_reduce) require c % 4 == 0 (use 'shufflenet_v2_x0_5', '_x1_5' or '_x2_0')")
    raise NotImplementedError(
        "backbone %r is outside the accelerated path (only 'hourglass' / 'hourglass_tiny', 'dense_hourglass' / "
        "'dense_hourglass_tiny', 'se_hourglass' / 'se_hourglass_tiny' and 'resnet10' / 'resnet50' / 'resnet101', "
        "'shufflenet_v2_x0_5' / 'shufflenet_v2_x1_5' / 'shufflenet_v2_x2_0')" % (backbone,))


def refuse_bf16(model_cfg):
    """cfg.Model.bf16 (or conv_math = "bf16") with the dense or the SE hourglass: inside ops.phantom_scope `pre` and the block
    outputs may exist as bf16 images only, and summing them into a feature that leaves the scope, or reducing them in the
    squeeze, needs rules nobody has tested.  fp32 and conv_math = "f16x3" (the convolutions only) are supported."""
    from rrnet_amd import ops
    if getattr(model_cfg, "backbone", None) in FP32_ONLY_BACKBONES and ops.math_mode(model_cfg) == ops.MATH_BF16:
        raise NotImplementedError(
            "cfg.Model.bf16 / conv_math = 'bf16' is not built for backbone %r: its skip sums and its squeeze would read "
            "bf16-only activations (use fp32 or cfg.Model.conv_math = 'f16x3')" % (model_cfg.backbone,))


def build_attention(model_cfg, num_stacks, in_channels=256):
    """cfg.Model.attention (builder-defined; absent or None: no attention, None is returned): a dict of SelfAttentionModule
    keyword arguments -> one module per stack, applied to the feature the stage-1 heads read (models/centernet.run_stage1_heads).
    `in_channels` defaults to the backbones' 256 features.  Refused together with cfg.Model.bf16 / conv_math = "bf16": the window
    kernels read fp32 tensors and the block's sum with a bf16-only feature has no tested rule; fp32 and conv_math = "f16x3" (the
    convolutions only) are supported."""
    import torch.nn as nn

    from rrnet_amd import ops
    from rrnet_amd.modules.self_attention import SelfAttentionModule
    kwargs = getattr(model_cfg, "attention", None)
    if kwargs is None:
        return None
    if ops.math_mode(model_cfg) == ops.MATH_BF16:
        raise NotImplementedError(
            "cfg.Model.attention is not built for cfg.Model.bf16 / conv_math = 'bf16': the window-attention kernels are fp32 "
            "(use fp32 or cfg.Model.conv_math = 'f16x3')")
    kwargs = dict(kwargs)
    kwargs.setdefault("in_channels", in_channels)
    modules = [SelfAttentionModule(**kwargs) for _ in range(num_stacks)]
    for m in modules:
        m.check_supported()
        if m.out_channels != kwargs["in_channels"]:
            raise ValueError("cfg.Model.attention: out_channels = %d, the residual sum needs the feature's %d"
                             % (m.out_channels, kwargs["in_channels"]))
    return nn.ModuleList(modules)


def attention_kwargs(kernel_size, dilation, channels=64):
    """The --attention K DIL of tools/train.py and tools/detect.py -> cfg.Model.attention."""
    return dict(key_channels=channels, value_channels=channels, kernel_size=int(kernel_size), dilation=int(dilation),
                padding=int(dilation) * (int(kernel_size) // 2))
