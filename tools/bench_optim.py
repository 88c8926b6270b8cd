"""What the guarded optimiser step costs: device time of the fused Adam, of the guarded chain with and without
averaged weights, and of the same semantics written in plain torch ops, each next to a plain device copy of its bytes.

  python tools/bench_optim.py [--models hourglass retinanet] [--repeats 10] [--out profiles/optim_guard.json]

Sizes: the flat parameter buffers of hourglass-104 RRNet and of RetinaNet-resnet50 (built with random weights, wrapped in
FlatParams, so that the torch variant clips over the real parameter views).  Per size, HIP-event time of
  adam             rr_adam_step alone                                              7 streams: 28 n bytes
  norm             rr_grad_norm alone                                              1 stream:   4 n bytes
  decide           rr_guard_decide alone                                           (a few KB)
  adam_guarded     rr_adam_step_guarded without EMA                                28 n bytes
  adam_guarded_ema rr_adam_step_guarded with EMA                                   36 n bytes
  chain            norm + decide + adam_guarded, one event pair                    32 n bytes
  chain_ema        norm + decide + adam_guarded_ema                                40 n bytes
  torch_chain_ema  clip_grad_norm_ over the parameter views + rr_adam_step + ema.lerp_   (rated on the 40 n bytes of its semantics)
  copy_<bytes>     dst.copy_(src) moving the same number of bytes (read + write)
The variants alternate inside every repeat, after a warm-up of each.  Rates are bytes the algorithm needs over the measured
time; `expected` restates the byte-count expectation (norm = one more read of the gradient at the copy rate, EMA = one read
and one write more) so that the report can say whether it held.  No threshold is applied."""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": [round(x, 4) for x in v]}


def _build(which):
    import torch
    if which == "hourglass":
        from rrnet_amd.configs.rrnet_config import Config
        from rrnet_amd.models.rrnet import RRNet
        cfg = copy.deepcopy(Config)
        return "hourglass-104 RRNet", RRNet(cfg).cuda().to(memory_format=torch.channels_last)
    from rrnet_amd.configs.retinanet_config import Config
    from rrnet_amd.models.retinanet import RetinaNet
    cfg = copy.deepcopy(Config)
    return "RetinaNet-resnet50", RetinaNet(cfg).cuda().to(memory_format=torch.channels_last)


def measure(which, repeats):
    import torch
    from rrnet_amd import ops
    from rrnet_amd.flat import FlatParams
    name, model = _build(which)
    fp = FlatParams(model)
    n, dev = fp.numel, fp.flat.device
    sync = torch.cuda.synchronize
    g = torch.Generator(device=dev).manual_seed(7)
    fp.grad.normal_(0, 1e-3, generator=g)
    m, v, ema = torch.zeros_like(fp.flat), torch.zeros_like(fp.flat), fp.flat.clone()
    partial, bad = ops.grad_norm(fp.grad)
    ctl = ops.guard_ctl_fresh().to(dev)
    views = [p for p in fp.params]
    lr, b1, b2, eps, decay = 2.5e-4, 0.9, 0.999, 1e-8, 0.999
    step = [0]

    def decide(ema_on):
        ops.guard_decide(partial, bad, ctl, 1.0, 35.0, True, lr, b1, b2, decay if ema_on else 0.0, ema_on)

    def adam():
        step[0] += 1
        ops.adam_step(fp.flat, fp.grad, m, v, lr, b1, b2, eps, step[0], 1.0)

    def torch_chain_ema():
        torch.nn.utils.clip_grad_norm_(views, 35.0)
        adam()
        ema.lerp_(fp.flat, 1.0 - decay)

    def chain(ema_on):
        ops.grad_norm(fp.grad, partial, bad)
        decide(ema_on)
        ops.adam_step_guarded(fp.flat, fp.grad, m, v, ema if ema_on else None, eps, ctl)

    variants = {
        "adam": (adam, 28 * n),
        "norm": (lambda: ops.grad_norm(fp.grad, partial, bad), 4 * n),
        "decide": (lambda: decide(False), None),
        "adam_guarded": (lambda: ops.adam_step_guarded(fp.flat, fp.grad, m, v, None, eps, ctl), 28 * n),
        "adam_guarded_ema": (lambda: ops.adam_step_guarded(fp.flat, fp.grad, m, v, ema, eps, ctl), 36 * n),
        "chain": (lambda: chain(False), 32 * n),
        "chain_ema": (lambda: chain(True), 40 * n),
        "torch_chain_ema": (torch_chain_ema, 40 * n),
    }
    copies = {}
    for nbytes in sorted({b for _, b in variants.values() if b}):
        src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        src.zero_()
        dst = torch.empty_like(src)
        copies[nbytes] = (src, dst)
        variants["copy_%d" % nbytes] = ((lambda s=src, d=dst: d.copy_(s)), nbytes)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1)
    for _ in range(2):
        for fn, _b in variants.values():
            timed(fn)
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, (fn, _b) in variants.items():
            times[k].append(timed(fn))
    stats = dict(zip(ops.GUARD_CTL_SLOTS, ctl.tolist()))
    assert stats["skipped"] == 0 and bool(torch.isfinite(fp.flat).all()) and bool(torch.isfinite(ema).all())
    res = {"model": name, "numel": n, "parameter_tensors": len(fp.params), "grad_norm_blocks": ops.grad_norm_blocks(n),
           "gnorm": stats["norm"], "clipped_steps": stats["clipped"], "applied_steps": stats["applied"], "ms": {}, "GBps": {}}
    for k, (_fn, nbytes) in variants.items():
        res["ms"][k] = _stats(times[k])
        if nbytes:
            res["GBps"][k] = nbytes / 1e9 / (res["ms"][k]["median"] * 1e-3)
    med = {k: res["ms"][k]["median"] for k in variants}
    copy_rate = res["GBps"]["copy_%d" % (28 * n)]                       # GB/s of the copy that moves Adam's byte count
    exp_chain = med["adam"] + 4 * n / 1e9 / copy_rate * 1e3 + med["decide"]
    exp_ema = med["adam"] * 36.0 / 28.0
    res["expected"] = {
        "copy_rate_GBps": copy_rate,
        "chain_ms": exp_chain, "chain_measured_over_expected": med["chain"] / exp_chain,
        "norm_ms_at_copy_rate": 4 * n / 1e9 / copy_rate * 1e3, "norm_measured_over_copy_rate_time": med["norm"] / (4 * n / 1e9 / copy_rate * 1e3),
        "adam_guarded_ema_ms": exp_ema, "adam_guarded_ema_measured_over_expected": med["adam_guarded_ema"] / exp_ema,
        "adam_guarded_over_adam": med["adam_guarded"] / med["adam"],
        "chain_ema_over_torch_chain_ema": med["chain_ema"] / med["torch_chain_ema"],
    }
    del copies, model
    torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--models", nargs="+", default=["hourglass", "retinanet"], choices=["hourglass", "retinanet"])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_optim.py needs the GPU")
    torch.cuda.set_device(0)
    torch.manual_seed(219)
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats, "sizes": [measure(w, a.repeats) for w in a.models]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
