"""What the SE hourglass' new kernels cost, and what a train step on each member of the hourglass family costs.

  python tools/bench_hgvariants.py [--repeats 10] [--steps 5] [--warmup 2] [--no-steps] [--out profiles/hg_variants.json]

Kernels (csrc/se.hip), at the full-size network's block shapes with B = 8 — 256 channels at 256x256, 384 at 64x64, 512 at
8x8 and the stem's block, 256 at 512x512: HIP-event time of every entry point, of the forward chain (squeeze, excite, scale)
and the backward chain (reduce, excite, apply) under one event pair each, of the same chains in plain torch ops on the
device, and of the 2x2 pool and ATen's — each beside `dst.copy_(src)` moving the bytes the kernel has to move (T = the
map's bytes: squeeze T, scale 3 T, reduce 3 T, apply 4 T, pool forward 1.3125 T, backward 1.3125 T).  The variants alternate
inside every repeat, after a warm-up of each.

Train steps: RRNet's fp32 step at B = 8, 1024x1024 on hourglass, dense_hourglass and se_hourglass by the method of bench.py's
step (every step from the seeded initial state, wall time around train_step + synchronize; bench.py itself takes the
hourglass only).  Numbers are reported, not judged."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [("c256_256x256", 256, 256, 256), ("c384_64x64", 384, 64, 64), ("c512_8x8", 512, 8, 8), ("stem_c256_512x512", 256, 512, 512)]
BATCH = 8


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def measure(tag, c, h, w, repeats):
    import torch
    import torch.nn.functional as F
    from rrnet_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(7)
    mk = lambda: torch.randn((BATCH, h, w, c), device=dev, generator=g).permute(0, 3, 1, 2)
    u, skip, dout = mk(), mk(), mk()
    cr, hw = c // 16, h * w
    w1 = torch.randn((cr, c), device=dev, generator=g) / c ** 0.5
    w2 = torch.randn((c, cr), device=dev, generator=g) / cr ** 0.5
    dw1, dw2 = torch.zeros_like(w1), torch.zeros_like(w2)
    T = u.numel() * 4
    st = {}

    def fwd():
        st["part"] = ops.se_squeeze(u)
        st["m"], st["h"], st["s"] = ops.se_excite_fwd(st["part"], w1, w2, hw)
        st["out"] = ops.se_scale_res_relu_fwd(u, st["s"], skip)

    def bwd():
        st["bpart"] = ops.se_bwd_reduce(dout, st["out"], u)
        st["dm"] = ops.se_excite_bwd(st["bpart"], st["s"], st["h"], st["m"], w1, w2, dw1, dw2)
        st["du"], st["dskip"] = ops.se_bwd_apply(dout, st["out"], st["s"], st["dm"])

    def torch_fwd():
        m = u.mean((2, 3))
        hh = torch.relu(m @ w1.t())
        s = torch.sigmoid(hh @ w2.t())
        st["t_out"], st["t_m"], st["t_h"], st["t_s"] = torch.relu(u * s[:, :, None, None] + skip), m, hh, s

    def torch_bwd():
        gg = dout * (st["t_out"] > 0)
        ds = (gg * u).sum((2, 3))
        dz2 = ds * st["t_s"] * (1 - st["t_s"])
        dz1 = (dz2 @ w2) * (st["t_h"] > 0)
        dm = dz1 @ w1
        dw2.add_(dz2.t() @ st["t_h"])
        dw1.add_(dz1.t() @ st["t_m"])
        st["t_du"] = gg * st["t_s"][:, :, None, None] + (dm / hw)[:, :, None, None]

    fwd(), bwd(), torch_fwd()
    _, idx = ops.maxpool2x2_fwd(u)
    dy = torch.randn((BATCH, h // 2, w // 2, c), device=dev, generator=g).permute(0, 3, 1, 2)
    variants = {
        "squeeze": (lambda: ops.se_squeeze(u), T),
        "excite_fwd": (lambda: ops.se_excite_fwd(st["part"], w1, w2, hw), None),
        "scale_res_relu": (lambda: ops.se_scale_res_relu_fwd(u, st["s"], skip), 3 * T),
        "bwd_reduce": (lambda: ops.se_bwd_reduce(dout, st["out"], u), 3 * T),
        "excite_bwd": (lambda: ops.se_excite_bwd(st["bpart"], st["s"], st["h"], st["m"], w1, w2, dw1, dw2), None),
        "bwd_apply": (lambda: ops.se_bwd_apply(dout, st["out"], st["s"], st["dm"]), 4 * T),
        "fwd_chain": (fwd, 4 * T),
        "bwd_chain": (bwd, 7 * T),
        "torch_fwd_chain": (torch_fwd, 4 * T),
        "torch_bwd_chain": (torch_bwd, 7 * T),
        "maxpool2x2_fwd": (lambda: ops.maxpool2x2_fwd(u), T + T // 4 + T // 16),
        "maxpool2x2_bwd": (lambda: ops.maxpool2x2_bwd(dy, idx, tuple(u.shape)), T + T // 4 + T // 16),
        "aten_maxpool2x2_fwd": (lambda: F.max_pool2d(u, 2), T + T // 4),
    }
    for nbytes in sorted({b for _, b in variants.values() if b}):
        src = torch.zeros(nbytes // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        variants["copy_%d" % nbytes] = ((lambda s_=src, d_=dst: d_.copy_(s_)), nbytes)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(2):
        for fn, _b in variants.values():
            timed(fn)
    times = {k: [] for k in variants}
    for _ in range(repeats):
        for k, (fn, _b) in variants.items():
            times[k].append(timed(fn))
    assert bool(torch.isfinite(st["du"]).all()) and bool(torch.isfinite(st["t_du"]).all())
    res = {"shape": tag, "batch": BATCH, "channels": c, "h": h, "w": w, "hidden": cr, "map_bytes": T,
           "chunk_rows_chunks": list(ops.se_chunk_rows(hw)), "ms": {}, "GBps": {}, "fraction_of_copy_rate": {}}
    for k, (_fn, nbytes) in variants.items():
        res["ms"][k] = _stats(times[k])
        if nbytes:
            res["GBps"][k] = nbytes / 1e9 / (res["ms"][k]["median"] * 1e-3)
    for k, (_fn, nbytes) in variants.items():
        if nbytes and not k.startswith("copy_"):
            res["fraction_of_copy_rate"][k] = res["GBps"][k] / res["GBps"]["copy_%d" % nbytes]
    res["fwd_chain_over_torch"] = res["ms"]["fwd_chain"]["median"] / res["ms"]["torch_fwd_chain"]["median"]
    res["bwd_chain_over_torch"] = res["ms"]["bwd_chain"]["median"] / res["ms"]["torch_bwd_chain"]["median"]
    del variants, st, u, skip, dout
    torch.cuda.empty_cache()
    return res


def train_step(backbone, steps, warmup):
    """The fp32 train step of RRNet on `backbone` at B = 8, 1024x1024, timed the way bench.py times its step (bench.py itself
    takes the hourglass only): synthetic batches resident on the device, every step from the seeded initial state (restored
    outside the clock), wall time around train_step + synchronize."""
    import copy
    import time
    import torch
    from rrnet_amd.configs.rrnet_config import Config
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    cfg = copy.deepcopy(Config)
    cfg.Train.batch_size, cfg.Train.crop_size, cfg.Model.backbone = BATCH, (1024, 1024), backbone
    cfg.Distributed.gpu_id, cfg.Distributed.rank, cfg.Distributed.world_size = 0, 0, 1
    torch.manual_seed(cfg.seed)
    op = RRNetOperator(cfg)
    op.model.train()
    batches = [op.training_loader.get_batch() for _ in range(len(op.training_loader))]
    opt = op.optimizer
    flat0 = opt.fp.flat.clone()
    bufs = [b for b in op.model.buffers()]
    bufs0 = [b.clone() for b in bufs]
    sched0, lrs0 = op.lr_sch.state_dict(), [g["lr"] for g in opt.param_groups]

    def restore():
        with torch.no_grad():
            opt.fp.flat.copy_(flat0)
            for b, b0 in zip(bufs, bufs0):
                b.copy_(b0)
            opt.exp_avg.zero_()
            opt.exp_avg_sq.zero_()
        opt.step_count = 0
        op.lr_sch.load_state_dict(sched0)
        for g, lr in zip(opt.param_groups, lrs0):
            g["lr"] = lr
        opt.fp.refresh_wt()

    step_no, elapsed, last = 0, [], None
    for i in range(warmup + steps):
        restore()
        b = batches[step_no % len(batches)]
        batch = (b[0], b[1].clone()) + tuple(b[2:])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, last = op.train_step(step_no, batch)
        torch.cuda.synchronize()
        if i >= warmup:
            elapsed.append((time.perf_counter() - t0) * 1e3)
        step_no += 1
    finite = bool(all(torch.isfinite(v.detach()).all() for v in last)) and bool(torch.isfinite(opt.fp.grad).all())
    res = {"backbone": backbone, "ms_per_step": _stats(elapsed), "images_per_s": BATCH * 1e3 / statistics.mean(elapsed),
           "steps": steps, "warmup": warmup, "finite": finite, "parameters": int(opt.fp.numel),
           "max_memory_GB": torch.cuda.max_memory_allocated() / 2 ** 30}
    del op, opt, batches, bufs, bufs0, flat0
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-steps", action="store_true", help="kernels only")
    ap.add_argument("--no-kernels", action="store_true", help="train steps only")
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_hgvariants.py needs the GPU")
    torch.cuda.set_device(0)
    res = {"device": torch.cuda.get_device_name(0), "repeats": a.repeats}
    if not a.no_kernels:
        res["kernels"] = [measure(*s, a.repeats) for s in SHAPES]
    if not a.no_steps:
        import warnings
        warnings.simplefilter("ignore", RuntimeWarning)          # (the missing ./hourglass.pth: random weights are what is timed)
        res["train_step_B8_1024"] = [train_step(b, a.steps, a.warmup) for b in ("hourglass", "dense_hourglass", "se_hourglass")]
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
