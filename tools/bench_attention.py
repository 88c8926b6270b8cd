"""Times the dilated-window attention (csrc/attn.hip) on the GPU and writes profiles/attention.json.

  python tools/bench_attention.py [--out profiles/attention.json] [--iters 10] [--no-step]

At B = 8, 256 -> 64 / 64 channels, kernel 5, dilation 6, padding 12, on 256x256 and 128x128 maps:
  kernels   rr_attn_fwd, rr_attn_bwd_q, rr_attn_bwd_kv, each beside a device copy (Tensor.copy_) that moves the bytes the
            kernel must move once (operands read once + results written once, ops.py's count): the ratio says how far the
            gathers from L2 sit from the copy rate
  torch     the same result as the unfold / multiply / sum / softmax chain in plain torch ops on the device, forward and
            forward + backward, next to the fused node (RF.window_attention); the outputs are compared
  step      RRNet's fp32 train step on `hourglass` (B = 8, 1024x1024: a 256x256 feature map) with and without
            cfg.Model.attention = --attention 5 6
Every time is the median of --iters runs between device events after 3 warm-up runs.  A run without a GPU fails."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

B, CK, CV, KERNEL, DIL, PAD = 8, 64, 64, 5, 6, 12
MAPS = (256, 128)


def timed(fn, iters, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ms.append(s.elapsed_time(e))
    ms.sort()
    return ms[len(ms) // 2]


def copy_ms(nbytes, iters):
    """A device copy whose read + written bytes are nbytes."""
    src = torch.empty(int(nbytes) // 8, dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src), iters)


def torch_chain(q, k, v):
    """Plain torch ops (NCHW): unfold key and value, multiply by the query, sum over channels, softmax over the taps, weigh."""
    n, ck, h, w = q.shape
    taps = KERNEL * KERNEL
    uk = F.unfold(k, KERNEL, dilation=DIL, padding=PAD).view(n, ck, taps, h, w)
    uv = F.unfold(v, KERNEL, dilation=DIL, padding=PAD).view(n, v.shape[1], taps, h, w)
    sim = torch.softmax((uk * q.unsqueeze(2)).sum(1, keepdim=True), 2)
    return (sim * uv).sum(2)


def bench_map(size, iters):
    from rrnet_amd import functional as RF, ops
    geom = ((KERNEL, KERNEL), (DIL, DIL), (PAD, PAD))
    g = torch.Generator(device="cuda").manual_seed(size)
    rnd = lambda c, scale: ops.to_nhwc(torch.randn(B, c, size, size, device="cuda", generator=g) * scale)
    q, k, v, dctx = rnd(CK, 0.35), rnd(CK, 0.35), rnd(CV, 1.0), rnd(CV, 1.0)        # logits of order 1
    ctx, p = ops.window_attention_fwd(q, k, v, *geom)
    ops.TIMER = ops.KernelTimer()
    try:
        ops.window_attention_fwd(q, k, v, *geom)
        ops.window_attention_bwd(dctx, q, k, v, p, *geom)
        torch.cuda.synchronize()
        nbytes = dict(ops.TIMER.bytes)
    finally:
        ops.TIMER = None
    fam = ops._ATTN
    dims = (B, size, size, CK, CV, KERNEL, KERNEL, DIL, DIL, PAD, PAD)
    ds, dq, dk, dv = torch.empty_like(p), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    launches = {
        "attn_fwd": lambda: fam.call("rr_attn_fwd", q, k, v, ctx, p, *dims),
        "attn_bwd_q": lambda: fam.call("rr_attn_bwd_q", dctx, v, k, p, ds, dq, *dims),
        "attn_bwd_kv": lambda: fam.call("rr_attn_bwd_kv", ds, p, q, dctx, dk, dv, *dims),
    }
    out = {"kernels": {}}
    for name, fn in launches.items():
        ms, cms = timed(fn, iters), copy_ms(nbytes[name], iters)
        out["kernels"][name] = {"ms": round(ms, 4), "bytes_moved_once": int(nbytes[name]), "GBps": round(nbytes[name] / ms / 1e6, 1),
                                "copy_ms": round(cms, 4), "copy_GBps": round(nbytes[name] / cms / 1e6, 1),
                                "time_over_copy": round(ms / cms, 3)}
    # the fused node against the chain of torch ops: forward, and forward + backward
    leaves = [t.detach().clone().requires_grad_() for t in (q, k, v)]
    tleaves = [t.detach().contiguous().clone().requires_grad_() for t in (q, k, v)]
    dplain = dctx.contiguous()

    def fused_fb():
        RF.window_attention(*leaves, *geom).backward(dctx)
        for t in leaves:
            t.grad = None

    def torch_fb():
        torch_chain(*tleaves).backward(dplain)
        for t in tleaves:
            t.grad = None

    with torch.no_grad():
        plain = [t.detach() for t in tleaves]
        ref = torch_chain(*plain)
        out["max_abs_difference_of_the_outputs"] = float((ref - ctx).abs().max())
        del ref
        f_fused = timed(lambda: ops.window_attention_fwd(q, k, v, *geom), iters)
        f_torch = timed(lambda: torch_chain(*plain), iters)
    fb_fused, fb_torch = timed(fused_fb, iters), timed(torch_fb, iters)
    unfolded = 4.0 * B * size * size * KERNEL * KERNEL * (CK + CV)
    out["forward"] = {"fused_ms": round(f_fused, 4), "torch_ms": round(f_torch, 4), "torch_over_fused": round(f_torch / f_fused, 2)}
    out["forward_backward"] = {"fused_ms": round(fb_fused, 4), "torch_ms": round(fb_torch, 4),
                               "torch_over_fused": round(fb_torch / fb_fused, 2)}
    out["backward"] = {"fused_ms": round(fb_fused - f_fused, 4), "torch_ms": round(fb_torch - f_torch, 4),
                       "torch_over_fused": round((fb_torch - f_torch) / (fb_fused - f_fused), 2),
                       "how": "forward + backward minus forward"}
    out["unfolded_key_and_value_bytes"] = int(unfolded)
    out["stash_bytes"] = int(p.numel() * 4)
    return out


def bench_step(attention, steps, warmup=2):
    """ms per fp32 RRNet train step on `hourglass`, B = 8 at 1024x1024, the synthetic loader's resident batches."""
    import copy
    import importlib
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    from rrnet_amd.utils.model_tools import attention_kwargs
    cfg = copy.deepcopy(importlib.import_module("rrnet_amd.configs.rrnet_config").Config)
    cfg.Train.batch_size, cfg.Train.crop_size, cfg.Model.backbone = B, (1024, 1024), "hourglass"
    cfg.Distributed.gpu_id, cfg.Distributed.rank, cfg.Distributed.world_size = 0, 0, 1
    if attention:
        cfg.Model.attention = attention_kwargs(KERNEL, DIL)
    torch.manual_seed(cfg.seed)
    op = RRNetOperator(cfg)
    op.model.train()
    batch = op.training_loader.get_batch()
    fresh = lambda: (batch[0], batch[1].clone()) + tuple(batch[2:])
    step = [1]

    def one():
        op.train_step(step[0], fresh())
        step[0] += 1
    ms = timed(one, steps, warmup)
    del op
    torch.cuda.empty_cache()
    return round(ms, 2)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention.json"))
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--no-step", action="store_true", help="skip the two RRNet train-step measurements")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_attention needs the GPU: nothing here is measured on a CPU")
    res = {"shape": {"batch": B, "in_channels": 256, "key_channels": CK, "value_channels": CV, "kernel": KERNEL, "dilation": DIL,
                     "padding": PAD}, "device": torch.cuda.get_device_name(0), "maps": {}}
    for size in MAPS:
        res["maps"]["%dx%d" % (size, size)] = bench_map(size, a.iters)
        torch.cuda.empty_cache()
    if not a.no_step:
        plain, attn = bench_step(False, a.steps), bench_step(True, a.steps)
        res["rrnet_train_step_hourglass_fp32_b8_1024"] = {"plain_ms": plain, "attention_5_6_ms": attn,
                                                          "added_ms": round(attn - plain, 2), "how": "median of %d steps" % a.steps}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
