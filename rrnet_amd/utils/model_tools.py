"""utils/model_tools.py:9-33 of the reference, restricted to the backbones of the models this package carries: the
hourglass of RRNet / CenterNet (configs/rrnet_config.py:80 -> 'hourglass'; 'hourglass_tiny' is the builder-defined backbone
of BASELINE.json config 1) and the three ResNets of RetinaNet (configs/retinanet_config.py:72 -> 'resnet50').  The other
names belong to out-of-scope models."""
from rrnet_amd.backbones.hourglass import hourglass_net, hourglass_tiny
from rrnet_amd.backbones.resnet import resnet10, resnet50, resnet101

_RESNETS = {'resnet10': resnet10, 'resnet50': resnet50, 'resnet101': resnet101}


def get_backbone(backbone, pretrained=False, num_stacks=2):
    if backbone == 'hourglass':
        return hourglass_net(num_stacks=num_stacks)
    if backbone == 'hourglass_tiny':
        return hourglass_tiny(num_stacks=num_stacks)
    if backbone in _RESNETS:
        return _RESNETS[backbone](pretrained=pretrained)
    raise NotImplementedError(
        "backbone %r is outside the accelerated path (only 'hourglass' / 'hourglass_tiny' and 'resnet10' / 'resnet50' / "
        "'resnet101')" % (backbone,))
