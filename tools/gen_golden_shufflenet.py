"""Regenerates tests/golden/shufflenet.npz and tests/golden/shufflenet_keys.json by running the REFERENCE's own
backbones/shufflenet.py (imported from the reference tree: none of it is copied) on the CPU in float64 and again in float32.
Both files hold data only.

  python tools/gen_golden_shufflenet.py --reference REF

shufflenet.npz: nn.Sequential(InvertedResidual(24, 48, 2, 2), InvertedResidual(48, 48, 1, 1)) (tests/shufflenet_cases.UNITS)
on a 2 x 24 x 9 x 11 input:
  state/<key>     the state dict the run starts from: the default initialisation under the stored seed, BatchNorm affine
                  parameters randomised (gamma 1, beta 0 would hide them)
  init/<key>      the convolution weights exactly as the seeded constructor drew them (= state/<key>; kept under a name of
                  their own for the initialisation test)
  x, gy           input and the fixed upstream gradient (float32-exact values)
  y, dx, grad/<parameter>, buf/<BatchNorm buffer>, y_eval
                  train-mode output, gradients, the BatchNorm buffers after that step, the eval-mode output that follows
  f32/...         the same run in float32: its distance from the float64 run is the yardstick of the unit tests
  margin, seed    the smallest distance of a pre-ReLU BatchNorm output from zero (float64 and float32 runs); the seed is
                  re-drawn until it exceeds shufflenet_cases.RELU_MARGIN — a flipped ReLU mask is not what the tests measure
shufflenet_keys.json: {width: [[key, shape], ...]} of the reference's ShuffleNetV2 at widths 0.5, 1.0, 1.5 and 2.0."""
import argparse
import importlib
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402
import shufflenet_cases as sc  # noqa: E402


def reference_module(ref_root):
    """The reference's backbones/shufflenet.py under a package name of its own (it imports its sibling `.load`)."""
    pkg = types.ModuleType("reference_backbones")
    pkg.__path__ = [os.path.join(ref_root, "backbones")]
    sys.modules["reference_backbones"] = pkg
    return importlib.import_module("reference_backbones.shufflenet")


def build(ref, seed):
    torch.manual_seed(seed)
    m = nn.Sequential(*[ref.InvertedResidual(*u) for u in sc.UNITS])
    init = {k: v.detach().clone() for k, v in m.state_dict().items() if v.dim() == 4}
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, nn.BatchNorm2d):
                mod.weight.copy_(torch.rand(mod.weight.shape, generator=g) + 0.5)
                mod.bias.copy_(torch.rand(mod.bias.shape, generator=g) * 0.6 - 0.3)
        x = torch.randn(sc.UNIT_INPUT, generator=g)
        y = m.eval()(x)
        gy = torch.randn(y.shape, generator=g)
    return m, init, x, gy


def run(m, x, gy, dtype):
    """One train-mode forward and backward, then an eval-mode forward -> (record, smallest |pre-ReLU BatchNorm output|)."""
    m = m.to(dtype).train()
    x = x.to(dtype).clone().requires_grad_(True)
    margin = [float("inf")]

    def watch(_mod, _inp, out):
        margin[0] = min(margin[0], float(out.detach().abs().min()))

    hooks = []
    for seq in [s for u in m for s in u.children()]:
        mods = list(seq)
        hooks += [a.register_forward_hook(watch) for a, b in zip(mods, mods[1:]) if isinstance(b, nn.ReLU)]
    y = m(x)
    y.backward(gy.to(dtype))
    for h in hooks:
        h.remove()
    rec = {"y": y.detach(), "dx": x.grad}
    for name, p in m.named_parameters():
        rec["grad/" + name] = p.grad
    for name, b in m.named_buffers():
        rec["buf/" + name] = b.detach().clone()
    with torch.no_grad():
        rec["y_eval"] = m.eval()(x.detach())
    return {k: v.numpy().copy() for k, v in rec.items()}, margin[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of the reference tree")
    args = ap.parse_args()
    ref = reference_module(args.reference)
    torch.set_num_threads(4)
    seed = 2300
    while True:
        m, init, x, gy = build(ref, seed)
        state = {k: v.detach().clone() for k, v in m.state_dict().items()}
        rec64, m64 = run(m, x, gy, torch.float64)
        m32 = nn.Sequential(*[ref.InvertedResidual(*u) for u in sc.UNITS])
        m32.load_state_dict(state)
        rec32, mg32 = run(m32, x, gy, torch.float32)
        margin = min(m64, mg32)
        if margin > sc.RELU_MARGIN:
            break
        seed += 1
    d = {}
    for k, v in state.items():
        d["state/" + k] = v.numpy().astype(np.int64 if v.dtype == torch.long else np.float64)
    for k, v in init.items():
        d["init/" + k] = v.numpy()
    d["x"], d["gy"] = x.numpy(), gy.numpy()
    d.update(rec64)
    d.update({"f32/" + k: v for k, v in rec32.items()})
    d["margin"], d["seed"] = np.float64(margin), np.int64(seed)
    print("seed %d, margin %.3g" % (seed, margin))
    np.savez_compressed(sc.GOLDEN, **d)
    print("wrote %s %d bytes, %d records" % (sc.GOLDEN, os.path.getsize(sc.GOLDEN), len(d)))
    keys = {}
    for width in sc.WIDTHS:
        net = ref.ShuffleNetV2(width_mult=width)
        keys[str(width)] = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    with open(sc.KEYS, "w") as fh:
        json.dump(keys, fh, separators=(",", ":"))
        fh.write("\n")
    print("wrote %s %d bytes" % (sc.KEYS, os.path.getsize(sc.KEYS)))


if __name__ == "__main__":
    main()
