"""Regenerates tests/golden/hgvariants.npz and tests/golden/hgvariants_keys.json by running the
REFERENCE's own dense and SE hourglass classes (backbones/dense_hourglass.py, backbones/se_hourglass.py) on the CPU in
float64.  Needs the reference tree (tools/ref_shims.py); both files hold data only.

  python tools/gen_golden_hgvariants.py

  blocks    the SE ResidualBlock for identity, projection and stride 2 on an odd map, SELayer alone, nn.MaxPool2d(2) on odd
            and even sizes with planted ties: whole tensors (train outputs, input and parameter gradients under a fixed
            upstream gradient, BatchNorm buffers, eval outputs)
  networks  the dense network with 2 and 3 stacks and the SE network with 2, at the tiny numbers, driven by the reference's
            own HourglassNet.forward (the object is built without its hard-coded __init__ and given tiny submodules of the
            reference's classes).  A whole record would be tens of MB, so the file keeps every 64th channel of the outputs, every
            4th pixel of the input gradient, the SE weights' gradients whole and (sum, sum of squares) of every
            parameter gradient (tests/hgvariant_cases.net_record); the float64 restatement that reproduces these is what
            the GPU tests compare whole tensors with.
  keys      state_dict keys with shapes of the full-size networks, constructed on the meta device

Weights come from helpers.det_fill on both sides, as in tools/gen_goldens.py; the tiny networks run with BatchNorm momentum 1
(the eval pass then sees the batch's statistics) and with the BatchNorm biases that settle_relus moved, recorded as
`<tag>/nudge_*`.
"""
import importlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ref_shims  # noqa: E402

ref_shims.install()
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import hgvariant_cases as hc  # noqa: E402
from helpers import det_fill, shapes_of  # noqa: E402

ref_se = importlib.import_module("backbones.se_hourglass")          # (reference)
ref_dense = importlib.import_module("backbones.dense_hourglass")    # (reference)
GOLD = os.path.join(ROOT, "tests", "golden")
torch.set_num_threads(8)


def load_det(module, seed):
    module.load_state_dict(det_fill(shapes_of(module.state_dict()), seed), strict=True)
    return module.double()


def tiny_reference_net(variant, num_stacks, n, inplanes, layer_nums, stem, num_feats):
    """The reference's HourglassNet object without its __init__ (which hard-codes the sizes), filled in its order with tiny
    submodules of the reference's own classes; forward is the reference's."""
    ref = ref_se if variant == "se" else ref_dense
    inplanes, layer_nums = list(inplanes), list(layer_nums)
    net = ref.HourglassNet.__new__(ref.HourglassNet)
    nn.Module.__init__(net)
    net.inplanes, net.num_feats, net.num_stacks = stem, num_feats, num_stacks
    pre = [nn.Conv2d(3, stem, kernel_size=7, stride=2, padding=3, bias=False), nn.BatchNorm2d(stem), nn.ReLU(inplace=True),
           ref.ResidualBlock(stem, 2 * stem, 1 if variant == "se" else 2)]
    net.pre_layer = nn.Sequential(*(pre + ([nn.MaxPool2d(2)] if variant == "se" else [])))
    c0 = inplanes[0]
    cbr = (lambda: ref.ConvBNRelu(3, c0, num_feats)) if variant == "se" else (lambda: ref.ConvBNRelu(3, c0, num_feats, with_relu=False))
    net.hgs = nn.ModuleList([ref.Hourglass(n, inplanes, layer_nums) for _ in range(num_stacks)])
    net.convs = nn.ModuleList([cbr() for _ in range(num_stacks)])
    net.residual = nn.ModuleList([ref.ResidualBlock(c0, c0) for _ in range(num_stacks - 1)])
    net.inter_ = nn.ModuleList([nn.Sequential(nn.Conv2d(c0, c0, (1, 1), bias=False), nn.BatchNorm2d(c0)) for _ in range(num_stacks - 1)])
    net.conv_ = nn.ModuleList([nn.Sequential(nn.Conv2d(num_feats, c0, (1, 1), bias=False), nn.BatchNorm2d(c0))
                               for _ in range(num_stacks - 1)])
    net.relu = nn.ReLU(inplace=True)
    return net


def main():
    d = {}
    for tag, ((cin, cout, stride), shape) in hc.BLOCK_CASES.items():
        d.update(hc.block_record(tag, load_det(ref_se.ResidualBlock(cin, cout, stride), 40), hc.det_input(shape, 41)))
    d.update(hc.block_record("selayer", load_det(ref_se.SELayer(32, 16), 42), hc.det_input((2, 32, 4, 5), 43)))
    for h, w in ((5, 7), (8, 8)):
        d.update(hc.block_record("pool_%dx%d" % (h, w), nn.MaxPool2d(2), hc.pool_case(h, w, 4, nan=False).double()))
    for tag, (variant, stacks, batch) in hc.NET_CASES.items():
        sizes = hc.DENSE_TINY if variant == "dense" else hc.HG_TINY
        x = hc.det_input((batch, 3) + hc.NET_HW, 61)
        # det_fill's weights with the BatchNorm biases settled (no ReLU input within RELU_MARGIN of 0: hgvariant_cases.settle_relus,
        # worked out on the restatement, whose ReLUs can be watched), then the same state in the reference's network
        settled = hc.full_momentum(load_det(hc.tiny_net(variant, stacks), 60))
        moved = hc.settle_relus(settled, x)
        net = hc.full_momentum(tiny_reference_net(variant, stacks, **sizes).double())
        net.load_state_dict(settled.state_dict(), strict=True)
        d.update(hc.net_record(tag, net, x))
        d[tag + "/nudge_keys"] = np.array([k for k, _, _ in moved])
        d[tag + "/nudge_ch"] = np.array([c for _, c, _ in moved], dtype=np.int64)
        d[tag + "/nudge_val"] = np.array([v for _, _, v in moved], dtype=np.float64)
        print("%s: %d biases moved" % (tag, len(moved)))
    path = os.path.join(GOLD, "hgvariants.npz")
    np.savez_compressed(path, **d)
    print("wrote %s %d bytes, %d records" % (path, os.path.getsize(path), len(d)))

    with torch.device("meta"):
        keys = {"dense_hourglass": hc.key_shapes(ref_dense.HourglassNet(2)), "se_hourglass": hc.key_shapes(ref_se.HourglassNet(2))}
    path = os.path.join(GOLD, "hgvariants_keys.json")
    with open(path, "w") as f:
        json.dump(keys, f, separators=(",", ":"))
    print("wrote %s %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
