"""Times ShuffleNetV2's kernels (csrc/depthwise.hip) on the GPU and writes profiles/shufflenet.json.

  python tools/bench_shufflenet.py [--out profiles/shufflenet.json] [--iters 20] [--steps 10] [--no-kernels] [--no-step]
                                   [--no-detect]

At retinanet_config's batch and crop (B = 2, 512x512), for the layer shapes of shufflenet_v2_x0_5 and _x1_5:
  kernels   rr_dwconv3x3_fwd (with the slab), _bwd_data, _bwd_weight at every distinct (map, channels, stride) of the backbone;
            rr_shuffle_interleave, _deinterleave, rr_channel_copy, rr_channel_join at every distinct (map, half).  Each beside a
            device copy (Tensor.copy_) that moves the bytes the kernel must move once (operands read once + results written
            once, ops.py's count) and beside the same operation in plain torch on the device (F.conv2d with groups = c,
            torch.nn.grad.conv2d_input / conv2d_weight, cat + reshape + transpose + contiguous, slicing + contiguous, cat)
  step      RetinaNet's fp32 train step on resnet50 and on each built width
  detect    frames/s of tools/bench_detect.py --retinanet (a child process per backbone) on resnet50 and on each built width
Every time is the median of --iters runs between device events after 3 warm-up runs.  A part that is skipped keeps what an
existing --out file holds for it.  A run without a GPU fails."""
import argparse
import copy
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

WIDTHS = {"shufflenet_v2_x0_5": 0.5, "shufflenet_v2_x1_5": 1.5}
BUILT = ("shufflenet_v2_x0_5", "shufflenet_v2_x1_5", "shufflenet_v2_x2_0")


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
    src = torch.empty(max(int(nbytes) // 8, 1), dtype=torch.float32, device="cuda").normal_()
    dst = torch.empty_like(src)
    return timed(lambda: dst.copy_(src), iters)


def layer_shapes(width, batch, crop):
    """-> (depthwise layers {(n, h, w, c, s)}, shuffles {(n, h, w, half)}) of ShuffleNetV2(width) on a batch x 3 x crop input,
    read off the module itself."""
    from rrnet_amd.backbones.shufflenet import ShuffleNetV2
    from rrnet_amd.ops import dw_out_hw
    net = ShuffleNetV2(width_mult=width)
    h, w = dw_out_hw(*dw_out_hw(crop[0], crop[1], 2), 2)            # the stem and the pool: 3x3 / 2 / 1 each
    dws, shuffles = set(), set()
    for u in net.features:
        for seq in u.children():
            for m in seq:
                if isinstance(m, torch.nn.Conv2d) and m.groups > 1:
                    dws.add((batch, h, w, m.in_channels, m.stride[0]))
        h, w = dw_out_hw(h, w, u.stride)
        shuffles.add((batch, h, w, u.banch2[-3].out_channels))
    return sorted(dws), sorted(shuffles)


def record(out, name, shape, fn, torch_fn, nbytes, iters):
    ms, cms, tms = timed(fn, iters), copy_ms(nbytes, iters), timed(torch_fn, iters)
    out.setdefault(name, []).append({"shape": list(shape), "ms": round(ms, 4), "bytes_moved_once": int(nbytes),
                                     "GBps": round(nbytes / ms / 1e6, 1), "copy_ms": round(cms, 4),
                                     "time_over_copy": round(ms / cms, 3), "torch_ms": round(tms, 4),
                                     "torch_over_kernel": round(tms / ms, 2)})


def bench_kernels(width, batch, crop, iters):
    from rrnet_amd import ops
    dws, shuffles = layer_shapes(width, batch, crop)
    out = {}
    g = torch.Generator(device="cuda").manual_seed(int(width * 10))
    rnd = lambda n, c, h, w: torch.randn((n, h, w, c), device="cuda", generator=g).permute(0, 3, 1, 2)
    for n, h, w, c, s in dws:
        p, q = ops.dw_out_hw(h, w, s)
        x, dy, wt = rnd(n, c, h, w), rnd(n, c, p, q), torch.randn((c, 1, 3, 3), device="cuda", generator=g)
        dw = torch.empty_like(wt)
        moved = 4.0 * c * (n * h * w + n * p * q)
        shape = (n, h, w, c, s)
        record(out, "dwconv3x3_fwd", shape, lambda: ops.dwconv3x3_fwd(x, wt, None, s, want_stats=True),
               lambda: F.conv2d(x, wt, None, s, 1, 1, c), moved, iters)
        record(out, "dwconv3x3_bwd_data", shape, lambda: ops.dwconv3x3_bwd_data(dy, wt, tuple(x.shape), s),
               lambda: torch.nn.grad.conv2d_input(x.shape, wt, dy, s, 1, 1, c), moved, iters)
        record(out, "dwconv3x3_bwd_weight", shape, lambda: ops.dwconv3x3_bwd_weight(x, dy, dw, s),
               lambda: torch.nn.grad.conv2d_weight(x, wt.shape, dy, s, 1, 1, c), moved, iters)
    for n, h, w, half in shuffles:
        x, b = rnd(n, 2 * half, h, w), rnd(n, half, h, w)
        lo, hi = x[:, :half], x[:, half:]
        shape = (n, h, w, half)
        whole = 16.0 * n * h * w * half                      # both halves read once and written once
        record(out, "shuffle_interleave", shape, lambda: ops.shuffle_interleave(lo, b),
               lambda: torch.cat([lo, b], 1).reshape(n, 2, half, h, w).transpose(1, 2).contiguous(), whole, iters)
        record(out, "shuffle_deinterleave", shape, lambda: ops.shuffle_deinterleave(x),
               lambda: (x[:, 0::2].contiguous(), x[:, 1::2].contiguous()), whole, iters)
        record(out, "channel_copy", shape, lambda: ops.channel_copy(hi), lambda: hi.contiguous(memory_format=torch.channels_last),
               whole / 2, iters)
        record(out, "channel_join", shape, lambda: ops.channel_join(b, b), lambda: torch.cat([b, b], 1), whole, iters)
    return out


def bench_step(backbone, batch, crop, steps, warmup=3):
    """ms per fp32 RetinaNet train step, the synthetic loader's resident batch."""
    import importlib
    from rrnet_amd.operators.retinanet_operator import RetinaNetOperator
    cfg = copy.deepcopy(importlib.import_module("rrnet_amd.configs.retinanet_config").Config)
    cfg.Train.batch_size, cfg.Train.crop_size, cfg.Model.backbone, cfg.Train.pretrained = batch, tuple(crop), backbone, False
    cfg.data_root = None
    cfg.Distributed.gpu_id, cfg.Distributed.rank, cfg.Distributed.world_size = 0, 0, 1
    torch.manual_seed(219)
    op = RetinaNetOperator(cfg)
    op.model.train()
    batch_ = op.training_loader.get_batch()
    fresh = lambda: (batch_[0], batch_[1].clone()) + tuple(batch_[2:])
    step = [1]

    def one():
        op.train_step(step[0], fresh())
        step[0] += 1
    ms = timed(one, steps, warmup)
    params = sum(p.numel() for p in op.model.parameters())
    del op
    torch.cuda.empty_cache()
    return {"ms": round(ms, 2), "parameters": int(params)}


def bench_detect(backbone, extra):
    """frames/s of tools/bench_detect.py --retinanet --backbone `backbone`, run in a child process."""
    with tempfile.TemporaryDirectory(prefix="bench_shufflenet_") as tmp:
        path = os.path.join(tmp, "detect.json")
        cmd = [sys.executable, os.path.join(ROOT, "tools", "bench_detect.py"), "--retinanet", "--backbone", backbone, "--out", path] + extra
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit("bench_detect.py failed for %s:\n%s" % (backbone, r.stderr[-3000:]))
        with open(path) as f:
            res = json.load(f)
    entry = res["modes"]["f32"]
    return {"frames_per_sec": res["value"], "of": res["value_of"],
            "by_path": {k: v["frames_per_sec"] for k, v in entry.items() if isinstance(v, dict) and "frames_per_sec" in v},
            "score_thr": entry.get("score_thr")}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shufflenet.json"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-kernel measurements")
    ap.add_argument("--no-step", action="store_true", help="skip the RetinaNet train-step measurements")
    ap.add_argument("--no-detect", action="store_true", help="skip the frames/s of tools/bench_detect.py --retinanet")
    ap.add_argument("--detect-args", default="--frames 16 --windows 3 --batches 1,4",
                    help="what tools/bench_detect.py --retinanet is given beside the backbone")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench_shufflenet needs the GPU: nothing here is measured on a CPU")
    from rrnet_amd.configs.retinanet_config import Config
    batch, crop = int(Config.Train.batch_size), tuple(Config.Train.crop_size)
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update(device=torch.cuda.get_device_name(0), batch=batch, crop=list(crop))
    say = lambda *what: print(*what, file=sys.stderr, flush=True)
    if not a.no_kernels:
        res["kernels"] = {"how": "median of %d runs between device events after 3 warm-up runs" % a.iters}
        for name, width in WIDTHS.items():
            res["kernels"][name] = bench_kernels(width, batch, crop, a.iters)
            torch.cuda.empty_cache()
            say("kernels of", name, "done")
    if not a.no_step:
        steps = res["retinanet_train_step_fp32"] = {}
        for b in ("resnet50",) + BUILT:
            steps[b] = bench_step(b, batch, crop, a.steps)
            say("train step", b, steps[b])
        steps["how"] = "median of %d steps after 3 warm-up steps, B = %d at %dx%d" % ((a.steps, batch) + crop)
    if not a.no_detect:
        fps = res["detect_frames_per_sec"] = {}
        for b in ("resnet50",) + BUILT:
            fps[b] = bench_detect(b, a.detect_args.split())
            say("detect", b, fps[b])
        fps["how"] = "tools/bench_detect.py --retinanet %s" % a.detect_args
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
