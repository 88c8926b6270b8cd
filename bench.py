"""bench.py — RRNet train-step throughput on MI355X (BASELINE.json metric: images/sec, train step).

  python bench.py [--gpus N] [--steps K] [--warmup W] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

Workload (BASELINE.json configs[1]): RRNet hourglass-104 (2 stacks), B=8 per GPU, 1024x1024
synthetic VisDrone-shaped frames, fp32; one "step" = forward + focal/L1/stage-2 losses + backward
+ (RCCL gradient all-reduce when N>1) + fused Adam — nothing skipped.  Weak scaling: B=8 per GPU.
Inputs are resident in HBM before the timed region.  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps, writes the last step's outputs when
--dump-outputs is given, and prints the headline line.  Every step, warm-up included, starts from
the seeded initial parameters and optimizer state (restored outside the clock), so the same
arguments give the same computation in every run.  --full adds everything else to that line:
`roofline` and `kernels` (dominant kernel = the implicit-GEMM forward convolution, MFMA-bound;
per-launch durations measured live with HIP events on the launch stream, inside the timed steps),
the secondary workloads (`config5`, `config4`, `config2_f16x3`), the host-fed variant
(`input_residency_host`) and `cpu_baseline` (the oracle's torch-CPU restatement of the same step,
timed on this box's host cores on a bounded sample); the --no-* options switch parts of it off.
"""
import argparse
import json
import os
import sys
import time

os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

FP32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: Peak FP32 (matrix), dense
ALGO_TFLOP_PER_IMAGE = 7.02        # fprop+dgrad+wgrad conv FLOPs of one 1024^2 image


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8, help="images per GPU (BASELINE config: 8)")
    ap.add_argument("--size", type=int, default=1024, help="frame height = width (BASELINE config: 1024)")
    ap.add_argument("--backbone", default="hourglass", choices=["hourglass", "hourglass_tiny"])
    ap.add_argument("--dump-outputs", metavar="DIR", help="after the timed steps, write what the last timed step computed (model "
                    "logits and losses; large arrays as a fixed, seeded sample) as DIR/<name>.npy, float32, <= 64 MB in all")
    ap.add_argument("--full", action="store_true", help="also measure and check everything beyond the headline: kernel timing and "
                    "roofline, secondary workloads, host-fed variant, CPU baseline (each can be switched off by its --no-* option)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true", help="skip the config-5 / config-4 secondary workloads")
    ap.add_argument("--extra-frames", type=int, default=10000, help="frames of the config-5 pass (BASELINE: 10k frames)")
    ap.add_argument("--extra-pool", type=int, default=512, help="distinct resident frames of the config-5 pass (4 batches of 128)")
    ap.add_argument("--no-kernel-timing", action="store_true")
    ap.add_argument("--time-every", type=int, default=4, help="HIP-event pair around every n-th launch of the dominant kernel")
    ap.add_argument("--math", default="f32", choices=["f32", "f16x3"], help="cfg.Model.conv_math of the timed train step (f16x3: "
                    "split-operand kernels on the large layers; the default line stays on the fp32 matrix instruction)")
    ap.add_argument("--detail", action="store_true", help="print a per-layer-shape conv time table to stderr (--full)")
    ap.add_argument("--no-host-fed", action="store_true", help="skip the host-fed variant of the headline (pinned host pool -> "
                    "copy stream -> device slots; reported as the extra key `input_residency_host`)")
    return ap.parse_args()


def _cpu_stepper(seed, size, k, frames=1):
    """-> a closure running one oracle train step (forward, criterion, backward, Adam update) on `frames` size x size frames and
    returning its seconds; model, optimizer state and buffers persist between calls (warm steps)."""
    from types import SimpleNamespace
    from oracle import model as om, ops as oo
    from oracle.targets import host_batch
    from rrnet_amd.datasets.synthetic import synth_frames
    from rrnet_amd.models.rrnet import RRNet
    cfg = SimpleNamespace(num_classes=10, Model=SimpleNamespace(num_stacks=2, backbone="hourglass",
                          nms_type_for_stage1="nms", nms_per_class_for_stage1=True))
    torch.manual_seed(seed)
    net = RRNet(cfg)
    sd = {kk: v.detach().clone() for kk, v in net.state_dict().items()}
    params = []
    for kk, _ in net.named_parameters():
        sd[kk].requires_grad_()
        params.append(sd[kk])
    del net
    opt = torch.optim.Adam(params, lr=2.5e-4)
    imgs, annos, hms, whs, inds, offs, masks, _ = host_batch(*synth_frames(frames, size, size, boxes_per_image=100, seed=seed))
    P = om.Params(sd, training=True)

    def one():
        t0 = time.perf_counter()
        opt.zero_grad()
        outs = om.rrnet_forward(P, imgs, k=k)
        losses = oo.criterion(outs, (hms, whs, inds, offs, masks, annos.clone()))
        (losses[0] + 0.1 * losses[1] + losses[2] + losses[3] * 0).backward()
        opt.step()
        return time.perf_counter() - t0
    return one


def cpu_baseline(seed, k=100, budget_s=300.0):
    """The oracle ("port": torch-CPU restatement of the reference graph, oracle/model.py + ops.py) running the
    hourglass-104 RRNet train step INCLUDING the Adam update on this box's host cores, on the bench's own frame size.
    The thread count is CHOSEN, not assumed: one warm 512x512 step at 8 / 16 / 32 / 64 / all threads (round 6: on the 256-CPU GPU
    box torch's default of 128 threads ran the step 6.7x SLOWER than 8 threads — a batch-1 graph of ~170 small convolutions does
    not spread over 128 cores, it drowns in fork / join; the 128-thread figure of earlier rounds under-stated the host).
    `value` = 1 / mean of two WARM real 1024x1024 steps (one frame each) at the fastest thread count (a first, cold step of the
    same stepper is run and reported beside them, never averaged in); `cores` = that thread count.  Side figures, never `value`:
    the sweep itself (`threads_sweep_512`), the all-threads 1024x1024 step of earlier rounds when the budget allows
    (`all_threads_1024`), and the stepper at B=4 x 512x512 — the same pixels per step as one 1024x1024 frame — at the chosen
    thread count (`batch4_512`: does a batch help?).  Reference loop: operators/rrnet_operator.py:116-138."""
    t_start = time.perf_counter()
    default_threads = torch.get_num_threads()
    one512 = _cpu_stepper(seed, 512, k)
    one512()                                          # cold: allocator, thread pool
    sweep = {}
    for th in sorted({8, 16, 32, 64, default_threads}):
        if th > (os.cpu_count() or th):
            continue
        torch.set_num_threads(th)
        one512()                                      # the pool's first step at this size is not representative either
        sweep[th] = round(one512(), 3)
    best = min(sweep, key=sweep.get)
    torch.set_num_threads(best)
    t512 = sweep[best]
    del one512
    out = {"unit": "images/sec", "cores": best, "kind": "port", "torch_default_threads": default_threads, "host_cpus": os.cpu_count(),
           "threads_sweep_512": {"seconds_per_warm_512x512_step_by_threads": sweep, "chosen": best},
           "images_per_sec_from_512_x4": round(1.0 / (t512 * 4.0), 5)}
    try:
        one1024 = _cpu_stepper(seed, 1024, k)
        all1024 = [one1024() for _ in range(3)]
        t1024 = 0.5 * (all1024[1] + all1024[2])
        out["value"] = round(1.0 / t1024, 5)
        out["t_1024_s"] = [round(t, 2) for t in all1024]
        out["sample"] = ("oracle torch-CPU RRNet hourglass-104 train step (fwd+losses+bwd+Adam), 1 frame 1024x1024 (the bench's frame "
                         "size), k=%d, %d threads (the fastest of the sweep %s s per 512x512 step): steps %s s (first = cold); value = 1 / mean of "
                         "the two warm ones = 1 / %.2f s" % (k, best, sweep, " / ".join("%.2f" % t for t in all1024), t1024))
        if default_threads != best and time.perf_counter() - t_start + 2.2 * 4.0 * sweep[default_threads] < budget_s:
            torch.set_num_threads(default_threads)
            one1024()
            out["all_threads_1024"] = {"threads": default_threads, "t_s": round(one1024(), 2)}
            torch.set_num_threads(best)
        del one1024
        four = _cpu_stepper(seed, 512, k, frames=4)
        t4 = [four() for _ in range(2)]              # cold, warm
        del four
        out["batch4_512"] = {"t_s": [round(t, 2) for t in t4], "images_per_sec": round(4.0 / t4[-1], 5), "threads": best,
                             "vs_batch1_512": round((4.0 / t4[-1]) * t512, 3)}
    except Exception as e:
        out.setdefault("value", out["images_per_sec_from_512_x4"])
        out.setdefault("sample", "1024x1024 steps failed (%r): value = 1 / (4 x the warm 512x512 step at %d threads) — an EXTRAPOLATION" % (e, best))
    finally:
        torch.set_num_threads(default_threads)
    return out


def extras(a):
    """Secondary workloads the driver's run reproduces next to the headline line (BASELINE configs[4] and [3]):
    `config5` = inference-only post-process on a stream of 1920x1080 frames, `config4` = the DCNv2 head layer."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    out = {}
    try:
        import bench_infer
        # cpu_frames=3: the oracle post-process (all host cores) and the single-core ext/nms Soft-NMS on 3 of the same frames
        # (BASELINE configs[4]: "boxes/sec vs CPU ext/nms"), ~3 s
        r = bench_infer.run(frames=a.extra_frames, batch=128, pool_frames=max(128, a.extra_pool // 128 * 128), cpu_frames=3)
        out["config5"] = {kk: r[kk] for kk in ("metric", "value", "unit", "frames_per_sec", "frames", "ms_per_batch",
                                               "output_boxes_per_frame", "cpu_baseline")}
        out["config5"]["workload"] = r["config"]["workload"]
        torch.cuda.empty_cache()
        try:
            import bench_softnms
            out["config5"]["softnms"] = bench_softnms.run()
        except Exception as e:
            out["config5"]["softnms"] = {"error": repr(e)}
    except Exception as e:                                       # never sink the headline number
        out["config5"] = {"value": None, "error": repr(e)}
    torch.cuda.empty_cache()
    try:
        import bench_dcn
        layer = bench_dcn.run()
        out["config4"] = {"layer": layer, "roofline": layer.get("roofline")}      # LDS roofline of the bf16 forward
        if a.backbone == "hourglass" and a.size == 1024:
            out["config4"].update(config4_train_step(a))
    except Exception as e:
        out["config4"] = {"value": None, "error": repr(e)}
    torch.cuda.empty_cache()
    if a.backbone == "hourglass" and a.size == 1024 and a.math == "f32":
        try:
            out["config2_f16x3"] = config2_split(a)
        except Exception as e:
            out["config2_f16x3"] = {"value": None, "error": repr(e)}
        torch.cuda.empty_cache()
    return out


def config2_split(a, steps=5):
    """The HEADLINE workload (configs[1], same model, batch, loop) with cfg.Model.conv_math = "f16x3": the large 3x3
    convolutions on the split-operand kernels (csrc/conv_bf16.hip rr_conv_*_f16x3: each fp32 operand as two fp16 parts,
    three matrix products, fp32 accumulation), the rest on the fp32-MFMA kernels.  Reported NEXT to the headline, not as
    it: the headline stays on v_mfma_f32_32x32x2_f32.  Evidence that the arithmetic is fp32-class rides along: the error
    of one layer against an fp64 convolution under both kernels (tests/test_conv_split_gpu.py, tests/test_split_model_gpu.py
    hold the bounds)."""
    import bench_config4
    import bench_conv_split
    r = bench_config4.run(a.batch, a.size, steps, False, a.backbone, False, "f16x3")
    r["vs_headline_arithmetic"] = "same tensors, same autograd graph, same launches except the convolutions with >= 2048 output " \
                                  "pixels, >= 64 channels and a reduction length >= 1024 (ops._bf16_ok)"
    r["error_vs_fp64_one_layer"] = bench_conv_split.accuracy(verbose=False)
    rates = bench_conv_split.layer_rates()
    r["dominant_layer"] = {"shape": "N8 C256 256x256 K256 3x3", **rates}
    # matrix-pipe ceiling of this arithmetic: three v_mfma_f32_32x32x16_f16 per product tile at the 16-bit dense peak
    r["mfma_peak_tflops"] = round(2500.0 / 3.0, 1)
    r["step_mfma_frac"] = round(r["value"] * ALGO_TFLOP_PER_IMAGE / (2500.0 / 3.0), 4)
    r["fprop_frac_of_peak"] = round(rates["f16x3"]["fprop"]["tflops"] / (2500.0 / 3.0), 4)
    return r


def config4_train_step(a, steps=5):
    """BASELINE configs[3] at model level (tools/bench_config4.py): the headline train step with the three heads' 3x3
    convolutions replaced by DCN layers (bf16 matrix operands, non-degenerate offsets), same batch, same loop; `plain` = the
    same bf16 model without the DCN heads; `conv16_dominant_layer` = the 16-bit-activation convolutions (csrc/conv16.hip) at the
    dominant layer, against the 2.5 PFLOP/s dense bf16 peak."""
    import bench_config4
    out = bench_config4.run(a.batch, a.size, steps, True, a.backbone)
    try:
        pl = bench_config4.run(a.batch, a.size, steps, False, a.backbone, True)
        out["plain"] = {kk: pl[kk] for kk in ("value", "unit", "ms_per_step", "steps", "workload", "allocator", "step_mfma_frac", "finite_after_timed_steps",
                                              "host_enqueue_ms_per_step")
                        if kk in pl}
    except Exception as e:
        out["plain"] = {"value": None, "error": repr(e)}
    try:
        import bench_conv16
        r = bench_conv16.run_shape(8, 256, 256, 256, 256, 3, 1, reps=10, check=True)
        out["conv16_dominant_layer"] = {"shape": "N8 C256 256x256 K256 3x3", "gflop": 618.5, "mfma_peak_tflops": 2500.0,
                                        **{kk: r[kk] for kk in r if kk.endswith("_tflops") or kk.endswith("_ms") or kk.endswith("_err")},
                                        "fprop_frac_of_peak": round(r["fprop_nostats_tflops"] / 2500.0, 4),
                                        # not a live measurement: the bare MFMA loop of this tile on random operands (no DMA, reads or
                                        # barriers) measured 1 285 TFLOP/s — the chip does not hold 2.4 GHz under sustained matrix load
                                        "mfma_loop_alone_tflops": 1285.0, "mfma_loop_alone_source": "profiles/r06_conv16_w4_ablation.txt",
                                        "fprop_frac_of_mfma_loop_alone": round(r["fprop_nostats_tflops"] / 1285.0, 4)}
    except Exception as e:
        out["conv16_dominant_layer"] = {"error": repr(e)}
    return out


def host_fed_steps(op, cfg, a, step_no):
    """`a.steps` timed train steps of the SAME operator fed from pinned host memory (one ~100 MB H2D copy per step on a
    copy stream, one batch ahead) -> {"value", "ms_per_step", ...}.  Reported next to the device-resident headline."""
    from rrnet_amd.datasets.synthetic import HostFedDronesDET
    ld = HostFedDronesDET(cfg, a.batch, a.size, a.size, rank=0, pool=2)
    for _ in range(3):
        op.train_step(step_no, ld.get_batch()); step_no += 1
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for _ in range(a.steps):
        last = op.train_step(step_no, ld.get_batch())[1]; step_no += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    finite = bool(all(torch.isfinite(v.detach()).all() for v in last))
    nbytes = sum(t.numel() * t.element_size() for t in ld.host[0][:3])
    return {"value": round(a.batch * a.steps / dt, 4), "unit": "images/sec", "ms_per_step": round(dt / a.steps * 1e3, 3),
            "steps": a.steps, "h2d_bytes_per_step": nbytes, "finite": finite,
            "how": "pinned host pool -> copy stream (one batch ahead) -> two device slots, event-ordered hand-over; targets "
                   "built on the device from the copied annotations inside the timed region"}


DUMP_BYTES = 60 << 20              # --dump-outputs: all arrays together stay under 64 MB
DUMP_MAX_ELEMS = 1 << 20           # a larger output is written as a fixed, seeded sample of this many elements
def dump_outputs(path, outs, losses):
    """--dump-outputs: what the last timed step handed its caller, as <path>/<name>.npy in float32 — RRNet's per-stack
    heat-map / size / offset logits and the five losses.  An array of more elements than the per-array cap is written as
    <name>_sample.npy: the elements (flattened in logical order) at sorted distinct positions drawn by a generator seeded
    with the array's index, so that the same arguments give the same positions.
    The step's RoIs, their scores and classes and the stage-2 regression over them are not written: stage 1 keeps the top
    1500 of 655 360 class-pixel scores per image, tied at the cut within the logits' rounding, so which RoIs are kept (and
    in which order among equal scores) changes with the rounding of the float atomics from run to run.  What is computed
    from them, the stage-2 loss, is written and agrees to rounding."""
    import numpy as np
    hms, whs, offs = outs[:3]
    arrays = [("hm_%d" % i, t) for i, t in enumerate(hms)] + [("wh_%d" % i, t) for i, t in enumerate(whs)] + \
             [("offset_%d" % i, t) for i, t in enumerate(offs)] + \
             list(zip(("loss", "hm_loss", "wh_loss", "offset_loss", "s2_reg_loss"), losses))
    cap = min(DUMP_MAX_ELEMS, DUMP_BYTES // 4 // len(arrays))
    os.makedirs(path, exist_ok=True)
    for i, (name, t) in enumerate(arrays):
        t = t.detach().float()
        if t.numel() > cap:
            pos = np.sort(np.random.default_rng(i).choice(t.numel(), cap, replace=False))
            t = t.reshape(-1)[torch.from_numpy(pos).to(t.device)]
            name += "_sample"
        np.save(os.path.join(path, name + ".npy"), t.cpu().numpy())


def self_launch(n):
    """`python bench.py --gpus N ...` without launcher variables -> run N ranks under torch.distributed.run as a child
    process with the same arguments; returns its exit code.  Nothing here imports or initialises the GPU runtime."""
    import socket
    import subprocess
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print("bench.py: no launcher variables in the environment — starting %d ranks: %s" % (n, " ".join(cmd)), file=sys.stderr, flush=True)
    return subprocess.run(cmd, cwd=os.getcwd(), env=dict(os.environ)).returncode


def main():
    a = parse()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if a.gpus > 1 and "RANK" not in os.environ:
        # Started without a launcher (`python bench.py --gpus N`): this process becomes the launcher.  Decided HERE, before
        # anything has touched the GPU (a process that has initialised HIP must never re-launch itself on this pool), and as a
        # CHILD process — no exec: `python -m torch.distributed.run` with one rank per GPU, env rendezvous on 127.0.0.1
        # (the reference spawns its own workers the same way: operators/distributed_wrapper.py:47-61).  Rank 0's JSON line goes
        # straight to our stdout; we exit with the launcher's code.
        sys.exit(self_launch(a.gpus))
    if not torch.cuda.is_available():
        print("bench.py: no GPU visible — the HIP path has no CPU fallback", file=sys.stderr)
        sys.exit(3)
    # RR_SINGLE_DEVICE=1 + RR_DIST_BACKEND=gloo: builder-side check of the N>1 code path on a 1-GPU box (every
    # rank on cuda:0, collectives through gloo).  The driver's multi-GPU runs use neither: one GPU per rank, RCCL.
    if os.environ.get("RR_SINGLE_DEVICE") == "1":
        local = 0
    torch.cuda.set_device(local)
    # RR_DP_FORCE=1 at N=1: a one-rank RCCL process group, every collective of the N>1 path issued for real (identity
    # collectives; rrnet_amd/dptrace.py) — the builder-side check that the real backend runs the data-parallel code
    dp_force = os.environ.get("RR_DP_FORCE", "0") == "1"
    if world > 1 or dp_force:
        if world == 1:
            import socket
            sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", str(port))
        dist.init_process_group(backend=os.environ.get("RR_DIST_BACKEND", "nccl"), init_method="env://",
                                world_size=world, rank=rank)

    from rrnet_amd import ops
    from rrnet_amd.configs.rrnet_config import Config as cfg
    from rrnet_amd.operators.rrnet_operator import RRNetOperator

    cfg.Train.batch_size = a.batch
    cfg.Train.crop_size = (a.size, a.size)
    cfg.Model.backbone = a.backbone
    cfg.Model.conv_math = a.math if a.math != "f32" else None
    cfg.Distributed.gpu_id = local
    cfg.Distributed.rank = rank
    cfg.Distributed.world_size = world
    torch.manual_seed(cfg.seed)                       # default torch init under seed 219 (same on every rank)
    op = RRNetOperator(cfg)
    op.model.train()
    batches = [op.training_loader.get_batch() for _ in range(len(op.training_loader))]   # resident in HBM
    torch.cuda.synchronize()

    def sync_all():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    def fresh(b):
        # the criterion converts annos xywh -> xyxy IN PLACE (as the reference does): hand it a copy
        return (b[0], b[1].clone()) + tuple(b[2:])

    # Every step starts from the seeded initial state: parameters, BatchNorm buffers, Adam moments and step count, learning
    # rate.  A step's float atomics (split-K convolutions, weight gradients) leave rounding-sized differences between runs,
    # which the ill-conditioned deep gradients and Adam's near-sign first updates magnify; steps chained from one another
    # would compute from different parameters in every run.  Restored outside the clock, so each step costs what a
    # training step costs.
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
        opt.fp.refresh_wt()           # the flipped-filter cache follows the restored parameters (as after an Adam step)

    step_no = 0
    for _ in range(a.warmup):
        restore()
        op.train_step(step_no, fresh(batches[step_no % len(batches)]))
        step_no += 1
    timer = None
    if a.full and not a.no_kernel_timing:
        # HIP events around every launch of the dominant kernel (the roofline leg); --detail times all conv kernels
        timer = ops.KernelTimer(None if a.detail else {"conv_fprop<BN=128,vec4>" + ("+f16x3" if a.math == "f16x3" else "")},
                                every=1 if a.detail else a.time_every)
        ops.TIMER = timer
    sync_all()
    from rrnet_amd import dptrace
    dptrace.reset()
    ops.SYNC_WAIT_S = 0.0
    host_s = 0.0
    elapsed = 0.0
    outs = last = None
    for _ in range(a.steps):
        restore()
        batch = fresh(batches[step_no % len(batches)])
        torch.cuda.synchronize()
        h0 = time.perf_counter()
        outs, last = op.train_step(step_no, batch)
        host_s += time.perf_counter() - h0
        torch.cuda.synchronize()
        elapsed += time.perf_counter() - h0
        if not a.dump_outputs:
            outs = None
        step_no += 1
    sync_all()
    # a timing on non-finite numbers is not a timing (NaN arithmetic draws less power: every kernel runs faster)
    finite = bool(all(torch.isfinite(v.detach()).all() for v in last)) and bool(torch.isfinite(op.optimizer.fp.grad).all()) \
        and bool(torch.isfinite(op.optimizer.fp.flat).all())
    if not finite:
        raise RuntimeError("bench.py: non-finite losses / gradients / parameters after the timed steps")
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, outs, last)
    outs = None
    # the loss tensors hold the last step's autograd graph, whose nodes keep what they attached to their ctx by hand (shared
    # fan-in buffers, bf16 images, parameter references): 20 GiB that counted into the extras' allocator peaks (round 5)
    last = None
    # host side of a step: time inside train_step() minus the time blocked in its one device->host read (RoI count)
    host_enqueue_ms = (host_s - ops.SYNC_WAIT_S) / a.steps * 1e3
    ops.TIMER = None
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())

    if rank == 0:
        images = a.batch * world * a.steps
        ms = elapsed / a.steps * 1e3
        out = {
            "metric": "images/sec (train step)", "value": round(images / elapsed, 4), "unit": "images/sec",
            "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(ms, 3),
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32" if a.math == "f32" else "f32 storage / accumulation; large convolutions multiply fp16 hi+lo operand pairs (f16x3)",
            "data": "synthetic",
            # the batches are resident in HBM before the timed region (tier contract); the reference's loader would pay a
            # ~100 MB host-to-device image copy per step inside it
            "input_residency": "device", "finite_after_timed_steps": finite,
            "config": {"workload": "RRNet %s (2 stacks) train step, %dx%d synthetic VisDrone frames, %s" %
                                   ("hourglass-104" if a.backbone == "hourglass" else "hourglass-tiny", a.size, a.size,
                                    "fp32" if a.math == "f32" else "fp32 tensors, conv_math f16x3"),
                       "per_gpu_batch": a.batch, "global_batch": a.batch * world, "k": 1500,
                       "parallelism": "dp%d" % world},
        }
        if timer is not None:
            summ = timer.summary()
            split = a.math == "f16x3"
            dom = "conv_fprop<BN=128,vec4>" + ("+f16x3" if split else "")
            peak = 2500.0 / 3.0 if split else FP32_MFMA_PEAK_TFLOPS      # f16x3: three 16-bit matrix instructions per product tile
            if dom in summ:
                d = summ[dom]
                achieved = d["flops"] / (d["ms"] * 1e-3) / 1e12
                # HBM traffic per launch of this kernel: last committed rocprofv3 PMC pass over this same command
                # (tools/prof_bench.sh -> tools/pmc_traffic.py -> profiles/rNN_traffic_pmc.json); PMC counters
                # cannot be read from inside the process, so the field names its source
                traffic, traffic_source = None, None
                for tag in ("r06", "r05", "r04", "r03", "r02", "r01"):
                    tpath = os.path.join(ROOT, "profiles", "%s_traffic_pmc.json" % tag)
                    if os.path.exists(tpath) and a.backbone == "hourglass" and a.size == 1024 and a.batch == 8:
                        with open(tpath) as f:
                            tj = json.load(f)
                        traffic = (tj.get("conv_igemm_kernel<128, 0, false, 32, 2, false, false>") or
                                   tj.get("conv_igemm_kernel<128, 0, false, 32, 2, false>") or
                                   tj.get("conv_igemm_kernel<128, 0, false, 32, 2>", {})).get("traffic_bytes_per_launch")
                        # not a live measurement: the file and the commit the PMC passes were taken at
                        traffic_source = "profiles/%s_traffic_pmc.json (rocprofv3 FETCH_SIZE + WRITE_SIZE passes of this command at commit %s)" % (
                            tag, tj.get("_commit", "bb2459f" if tag == "r01" else "unrecorded"))
                        break
                if split:
                    traffic, traffic_source = None, None        # (the committed PMC passes are of the fp32 kernel)
                out["roofline"] = {"bound": "mfma", "achieved": round(achieved, 2), "peak": round(peak, 1),
                                   "unit": "TFLOP/s", "frac": round(achieved / peak, 4),
                                   "traffic": traffic, "traffic_source": traffic_source,
                                   "algorithmic_bytes_per_launch": round(timer.bytes.get(dom, 0.0) / d["launches"]),
                                   "kernel": ("conv_igemm_bf16_kernel<128, *, *, false, 2, false, true> (split-operand implicit-GEMM forward kernel, three "
                                              "v_mfma_f32_32x32x16_f16 per product tile: peak = 2500 / 3; fprop and stride-1 dgrad)") if split else
                                             "conv_igemm_kernel<128, 0, false, 32, 2, false, false> (implicit-GEMM forward kernel, v_mfma_f32_32x32x2_f32; "
                                             "launched for fprop and for stride-1 dgrad on flipped weights; the dgrad launches that also "
                                             "reduce the producer's BatchNorm-backward sums are the <..., true> instantiation)",
                                   "launches": d["launches"], "launches_timed": "every %d-th launch of the timed region (systematic sample)" % a.time_every,
                                   "avg_launch_ms": round(d["ms"] / d["launches"], 4),
                                   "algorithmic_gflop_per_launch": round(d["flops"] / d["launches"] / 1e9, 3)}
            out["kernels"] = {k: {"launches": v["launches"], "ms": round(v["ms"], 2),
                                  "tflops": round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 2) if v["ms"] > 0 else None}
                              for k, v in sorted(summ.items())}
            if a.detail:
                rows = sorted(timer.by_shape().items(), key=lambda kv: -kv[1]["ms"])
                for (name, shp), v in rows[:40]:
                    print("%-28s %-38s n=%4d %8.2f ms %6.1f TF" % (name, shp, v["launches"], v["ms"],
                          v["flops"] / (v["ms"] * 1e-3) / 1e12), file=sys.stderr)
            if a.detail:
                conv_ms = sum(v["ms"] for v in summ.values())
                out["conv_time_fraction"] = round(conv_ms / (elapsed * 1e3), 4)
        out["host_enqueue_ms_per_step"] = round(host_enqueue_ms, 2)
        # collectives issued per step and rank, by communicator (rrnet_amd/dptrace.py): SyncBN statistic exchanges on
        # the default one, gradient buckets on their own; 0 at N=1
        cc = dptrace.counts()
        out["collectives_per_step"] = {"total": round(sum(cc.values()) / a.steps, 1),
                                       **{k: round(v / a.steps, 1) for k, v in sorted(cc.items())}}
        if dptrace.HOST_S:
            out["dp_host_ms_per_step"] = {k: round(v / a.steps * 1e3, 2) for k, v in sorted(dptrace.HOST_S.items())}
        if dp_force and world == 1:
            out["dp_force"] = "one-rank %s process group: SyncBN exchanges + bucketed gradient all-reduce issued for real" % \
                              dist.get_backend()
        if a.backbone == "hourglass" and a.size == 1024:
            out["step_mfma_frac"] = round(out["value"] / world * ALGO_TFLOP_PER_IMAGE / (2500.0 / 3.0 if a.math == "f16x3" else FP32_MFMA_PEAK_TFLOPS), 4)
        if world == 1 and a.full and not a.no_extras:
            del op, batches
            import gc
            gc.collect()
            torch.cuda.empty_cache()
            op = batches = None
            out.update(extras(a))
        if world == 1 and a.full and not a.no_host_fed and a.math == "f32":
            # the reference's hand-over: host batches, one PCIe crossing per step (rrnet_amd/datasets/synthetic.py:
            # HostFedDronesDET: pinned pool, copy stream one batch ahead, event-ordered).  Run LAST among the GPU workloads, on an
            # operator of its own when the headline's was released for the extras: measured in this process, the f16x3 step that
            # followed the host-fed steps ran 2x slower (543 ms against 274-300 without them; the bf16 steps were unaffected) —
            # not understood, so nothing on the GPU is timed behind it.
            try:
                if op is None:
                    cfg.Model.conv_math = None
                    cfg.Model.bf16 = False
                    cfg.Model.dcn_heads = False
                    cfg.Train.batch_size, cfg.Train.crop_size, cfg.Model.backbone = a.batch, (a.size, a.size), a.backbone
                    torch.manual_seed(cfg.seed)
                    op = RRNetOperator(cfg)
                    op.model.train()
                out["input_residency_host"] = host_fed_steps(op, cfg, a, step_no)
            except Exception as e:
                out["input_residency_host"] = {"value": None, "error": repr(e)}
            del op
        if world == 1 and a.full and not a.no_cpu_baseline:
            try:
                out["cpu_baseline"] = cpu_baseline(cfg.seed)
            except Exception as e:                                   # the baseline must never sink the GPU number
                out["cpu_baseline"] = {"value": None, "unit": "images/sec", "cores": torch.get_num_threads(),
                                       "kind": "port", "sample": "failed: %r" % (e,)}
        print(json.dumps(out), flush=True)
    if dist.is_initialized():
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
