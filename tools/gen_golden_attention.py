"""Regenerates tests/golden/self_attention.npz by running the REFERENCE's own SelfAttentionModule (modules/self_attention.py
of the reference tree, imported from there: none of it is copied) on the CPU in float64 and again in float32.  The file
holds data only.

  python tools/gen_golden_attention.py --reference REF

Per case of tests/attn_cases.MODULE_CASES (`<tag>/...`):
  state/<key>     the state dict the run starts from: the default initialisation under the stored seed, BatchNorm affine
                  parameters and `W` (weight and bias) randomised — a zero `W` makes the output and every other gradient vanish
  x, gy           input and the fixed upstream gradient (float32-exact values)
  y, dx, grad/<parameter>, buf/<BatchNorm buffer>, y_eval
                  train-mode output, gradients, the BatchNorm buffers after that step, the eval-mode output that follows
  f32/...         the same run in float32: its distance from the float64 run is the yardstick of the module tests
  q, k, v, ctx, dq, dk, dv, dctx
                  the tensors around the unfold / softmax / weighted-sum chain (NCHW): what the oracle of tests/attn_cases.py
                  is held against
  margin, seed    the smallest distance of a pre-ReLU BatchNorm output from zero (float64 and float32 runs); the seed is
                  re-drawn until it exceeds attn_cases.RELU_MARGIN — a flipped ReLU mask is not what the tests measure
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402
import attn_cases as ac  # noqa: E402


def reference_class(ref_root):
    path = os.path.join(ref_root, "modules", "self_attention.py")
    spec = importlib.util.spec_from_file_location("reference_self_attention", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.SelfAttentionModule


def build(cls, case, seed):
    torch.manual_seed(seed)
    m = cls(case["cin"], case["ck"], case["cv"], kernel_size=case["kernel"], dilation=case["dilation"], padding=case["padding"])
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for name, p in m.named_parameters():
            leaf = name.rsplit(".", 1)[-1]
            if p.dim() == 1 and name.split(".")[0] in ("f_key", "f_query") and name.split(".")[1] in ("1", "4"):
                p.copy_(torch.rand(p.shape, generator=g) + 0.5 if leaf == "weight" else torch.rand(p.shape, generator=g) * 0.6 - 0.3)
            elif name.startswith("W."):
                p.copy_(torch.randn(p.shape, generator=g) * (0.3 if leaf == "weight" else 0.1))
        x = torch.randn((case["n"], case["cin"]) + tuple(case["hw"]), generator=g)
        gy = torch.randn((case["n"], case["cin"]) + tuple(case["hw"]), generator=g)
    return m, x, gy


def run(m, x, gy, dtype):
    """One train-mode forward and backward, then an eval-mode forward -> (record, smallest |pre-ReLU BatchNorm output|)."""
    m = m.to(dtype).train()
    x = x.to(dtype).clone().requires_grad_(True)
    kept, margin = {}, [float("inf")]

    def keep(name):
        def hook(_mod, _inp, out):
            out.retain_grad()
            kept[name] = out
        return hook

    def watch(_mod, _inp, out):
        margin[0] = min(margin[0], float(out.detach().abs().min()))

    hooks = [m.f_query.register_forward_hook(keep("q")), m.f_key.register_forward_hook(keep("k")),
             m.f_value.register_forward_hook(keep("v"))]
    hooks += [seq[i].register_forward_hook(watch) for seq in (m.f_key, m.f_query) for i in (1, 4)]

    def keep_ctx(_mod, inp):
        inp[0].retain_grad()
        kept["ctx"] = inp[0]
    hooks.append(m.W.register_forward_pre_hook(keep_ctx))
    y = m(x)
    y.backward(gy.to(dtype))
    for h in hooks:
        h.remove()
    rec = {"y": y.detach(), "dx": x.grad}
    for name, t in kept.items():
        rec[name] = t.detach()
        rec["d" + name] = t.grad
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
    cls = reference_class(args.reference)
    torch.set_num_threads(4)
    d = {}
    for tag, case in ac.MODULE_CASES.items():
        seed = 100 * (1 + sorted(ac.MODULE_CASES).index(tag))
        while True:
            m, x, gy = build(cls, case, seed)
            state = {k: v.detach().clone() for k, v in m.state_dict().items()}
            rec64, m64 = run(m, x, gy, torch.float64)
            m32 = cls(case["cin"], case["ck"], case["cv"], kernel_size=case["kernel"], dilation=case["dilation"],
                      padding=case["padding"])
            m32.load_state_dict(state)
            rec32, mg32 = run(m32, x, gy, torch.float32)
            margin = min(m64, mg32)
            if margin > ac.RELU_MARGIN:
                break
            seed += 1
        for k, v in state.items():
            d["%s/state/%s" % (tag, k)] = v.numpy().astype(np.int64 if v.dtype == torch.long else np.float64)
        d[tag + "/x"], d[tag + "/gy"] = x.numpy(), gy.numpy()
        for k, v in rec64.items():
            d["%s/%s" % (tag, k)] = v
        for k, v in rec32.items():
            if k not in ("q", "k", "v", "ctx", "dq", "dk", "dv", "dctx"):
                d["%s/f32/%s" % (tag, k)] = v
        d[tag + "/margin"], d[tag + "/seed"] = np.float64(margin), np.int64(seed)
        print("%s: seed %d, margin %.3g" % (tag, seed, margin))
    path = ac.GOLDEN
    np.savez_compressed(path, **d)
    print("wrote %s %d bytes, %d records" % (path, os.path.getsize(path), len(d)))


if __name__ == "__main__":
    main()
