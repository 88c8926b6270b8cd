"""GPU: the data-parallel path (SyncBN statistics exchange + flat-gradient all-reduce + fused Adam) with
TWO ranks must reproduce the single-rank full-batch result.  Both ranks share cuda:0 and talk through
gloo (a 1-GPU box cannot host two RCCL ranks); the code path is the one `bench.py --gpus N` runs, only
the backend string differs."""
import os
import socket
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg():
    return SimpleNamespace(num_classes=10, Model=SimpleNamespace(num_stacks=1, backbone="hourglass_tiny",
                           nms_type_for_stage1="nms", nms_per_class_for_stage1=True))


def _build():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import det_fill
    from rrnet_amd.models.centernet import CenterNet
    m = CenterNet(_cfg())
    m.load_state_dict(det_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, 21))
    return m


def _loss(model, x):
    hms, whs, regs = model(x)
    return (hms[0] ** 2).mean() + (whs[0] ** 2).mean() + (regs[0] ** 2).mean()


def _data():
    g = torch.Generator().manual_seed(3)
    return torch.randn(4, 3, 64, 64, generator=g)


def _worker(rank, world, port, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from rrnet_amd.flat import FlatAdam, FlatParams
        model = _build().cuda().to(memory_format=torch.channels_last)
        model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model).train()
        fp = FlatParams(model, bucket_elems=4096)      # many buckets: their all-reduces start during backward
        fp.broadcast(0)
        opt = FlatAdam(fp, lr=1e-3)
        x = _data()[rank * 2:(rank + 1) * 2].cuda()
        opt.zero_grad()
        _loss(model, x).backward()
        launched = sum(w is not None for w in fp._works)
        # all but the buckets holding an autograd-accumulated parameter (the WH head tap weights) start during backward
        assert len(fp._bucket_range) > 4 and launched >= len(fp._bucket_range) - 3, (launched, len(fp._bucket_range))
        scale = fp.all_reduce_grads()
        g = (fp.grad * scale).cpu().numpy()
        rm = model.backbone.pre_layer[1].running_mean.cpu().numpy()
        opt.step()                       # (second all-reduce of an already reduced buffer is avoided below)
        if rank == 0:
            np.savez(out, grad=g, running_mean=rm)
    finally:
        dist.destroy_process_group()


def test_two_rank_syncbn_dp_matches_single_rank(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    out = str(tmp_path / "dp.npz")
    mp.spawn(_worker, nprocs=2, args=(2, port, out), join=True)
    z = np.load(out)
    from rrnet_amd.flat import FlatParams
    model = _build().cuda().to(memory_format=torch.channels_last).train()
    fp = FlatParams(model)
    fp.zero_grad()
    _loss(model, _data().cuda()).backward()
    ref = fp.grad.cpu().numpy()
    scale = np.abs(ref).max()
    assert np.abs(z["grad"] - ref).max() <= 2e-3 * scale, (np.abs(z["grad"] - ref).max(), scale)
    np.testing.assert_allclose(z["running_mean"], model.backbone.pre_layer[1].running_mean.cpu().numpy(), atol=1e-5)


def _trace_worker(rank, world, port, outdir):
    """One full RRNet train step per rank (SyncBN, bucketed gradient exchange, fused Adam) on DIFFERENT images, so that
    the ranks' RoI counts — and with them the shapes of every stage-2 tensor — differ; the collective trace is dumped."""
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, ROOT)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import json
        from rrnet_amd import dptrace, functional as RF
        from rrnet_amd.datasets.synthetic import synth_batch
        from rrnet_amd.flat import FlatAdam, FlatParams
        from rrnet_amd.models.rrnet import RRNet
        from rrnet_amd.operators.base_operator import broadcast_buffers
        dptrace.ENABLED = True
        cfg = SimpleNamespace(num_classes=10, Model=SimpleNamespace(num_stacks=2, backbone="hourglass_tiny",
                              nms_type_for_stage1="nms", nms_per_class_for_stage1=True))
        torch.manual_seed(5 + rank)                                    # ranks even start from different weights
        model = RRNet(cfg).cuda().to(memory_format=torch.channels_last)
        model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model).train()
        fp = FlatParams(model, bucket_elems=8192)
        fp.broadcast(0)
        nbuf = broadcast_buffers(model, 0)
        opt = FlatAdam(fp, lr=1e-3)
        rois = []
        for step in range(2):
            dptrace.reset()
            imgs, annos, hms, whs, inds, offs, masks, _ = synth_batch(2, 128, 160, boxes_per_image=6 + 20 * rank,
                                                                      seed=100 + 7 * rank + step)
            opt.zero_grad()
            outs = model(imgs, k=60 + 90 * rank)                       # different K per rank: different RoI counts
            rois.append(int(outs[4].shape[0]))
            loss = sum(RF.focal_loss_hm_from_logits(outs[0][i], hms) + RF.reg_l1_loss(outs[1][i], masks, inds, whs)
                       + RF.reg_l1_loss(outs[2][i], masks, inds, offs) for i in range(2))
            annos[:, :, 2:4] += annos[:, :, 0:2]
            loss = loss + RF.stage2_reg_loss(outs[3], outs[4], annos, 4.0)
            loss.backward()
            opt.step()
            torch.cuda.synchronize()
        w = fp.flat.detach().cpu().numpy()
        with open(os.path.join(outdir, "trace%d.json" % rank), "w") as f:
            json.dump({"events": dptrace.EVENTS, "counts": dptrace.counts(), "rois": rois, "nbuf": nbuf,
                       "need": fp._bucket_need, "wsum": float(np.abs(w).sum()), "whash": float((w * np.arange(w.size) % 7).sum())}, f)
    finally:
        dist.destroy_process_group()


def test_two_rank_collective_sequences_are_identical(tmp_path):
    """What hangs an 8-GPU node must fail on a 1-GPU box: with ranks that see different images (different RoI counts,
    different stage-2 shapes) the sequence of (communicator, op, element count) is IDENTICAL on both ranks for each of the
    two communicators, every gradient bucket's all-reduce is issued after the last `mark_ready` of its parameters (i.e.
    after the last kernel writing its slice was enqueued) and exactly once, and the ranks end the step with identical
    parameters."""
    import json
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_trace_worker, nprocs=2, args=(2, port, str(tmp_path)), join=True)
    t = [json.load(open(str(tmp_path / ("trace%d.json" % r)))) for r in range(2)]
    assert t[0]["rois"] != t[1]["rois"], t[0]["rois"]                  # the ranks really did different work
    for comm in ("default", "grads"):
        seq = [[e[:3] for e in tr["events"] if e[1] != "mark" and e[0] == comm] for tr in t]
        assert seq[0] == seq[1], comm
        assert len(seq[0]) > 0
    ev = t[0]["events"]
    need = t[0]["need"]
    seen = {}
    launched = {}
    for i, (comm, op, numel, note) in enumerate(ev):
        if op == "mark":
            b = int(note.split()[-1])
            assert b not in launched, "parameter reported after its bucket's all-reduce was issued: %s" % note
            seen[b] = seen.get(b, 0) + 1
        elif comm == "grads":
            b = int(note.split()[1])
            assert b not in launched, "bucket %d exchanged twice" % b
            launched[b] = i
            if "end of step" not in note:
                assert seen.get(b, 0) == need[b], (b, seen.get(b, 0), need[b])
    assert len(launched) == len(need)                                   # every bucket exactly once
    during = sum(1 for e in ev if e[0] == "grads" and "end of step" not in e[3])
    assert during >= len(need) - 3, (during, len(need))                 # overlapped with backward
    # a projection block's skip and conv1 share ONE statistics exchange per direction (functional._ConvBnSyncMulti)
    joint = [e for e in ev if e[0] == "default" and e[3].endswith("x2")]
    assert len(joint) >= 2 and len(joint) % 2 == 0, [e[3] for e in ev if e[0] == "default"][:12]
    # the first layers of an hourglass module's two branches (up1.conv1, low1.conv1 stride 2, low1's projection) share ONE
    # exchange per direction as well: three layers, three sample counts in the forward message
    joint3 = [e for e in ev if e[0] == "default" and e[3].endswith("x3")]
    assert len(joint3) >= 2 and len(joint3) % 2 == 0, sorted({e[3] for e in ev if e[0] == "default"})
    fwd3 = [e for e in joint3 if "fwd" in e[3]]
    assert fwd3 and all((e[2] - 3) % 2 == 0 for e in fwd3)               # [sum, sumsq] of the layers' channels + 3 counts
    n_sync = sum(1 for e in ev if e[0] == "default")
    print("collectives of one step: %d SyncBN exchanges on the default communicator, %d gradient buckets (%d launched "
          "during backward); buffers broadcast in one collective (%d buffers)" % (n_sync, len(launched), during, t[0]["nbuf"]))
    assert t[0]["wsum"] == t[1]["wsum"] and t[0]["whash"] == t[1]["whash"]


# ---- SyncBN nodes on RAGGED shards against the fp64 oracle ------------------------------------------------------------
SYNC_SHARDS = {"cbr_res": (1, 3), "cbr": (1, 3), "block": (1, 3), "head": (37, 5)}      # rows of rank 0, rank 1
SYNC_SHAPES = {"cbr_res": (64, 16, 16), "cbr": (64, 16, 16), "block": (32, 16, 16), "head": (256, 3, 3)}
SYNC_PROJ = {"cbr_res": (64, 16, 16), "cbr": (64, 16, 16), "block": (64, 8, 8), "head": (4,)}


def _sync_modules():
    """conv -> SyncBN -> ReLU with a residual (mask from z) and without (mask recomputed), a stride-2 channel-changing
    residual block (conv1 and the projection share the joint node) and the stage-2 head; seeded weights, running
    statistics away from (0, 1)."""
    import torch.nn as nn
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import det_fill
    from rrnet_amd.backbones.hourglass import ResidualBlock
    from rrnet_amd.detectors.fasterrcnn_detector import FasterRCNNDetector

    class Cases(nn.Module):
        def __init__(self):
            super().__init__()
            self.conv_a, self.bn_a = nn.Conv2d(64, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64)
            self.conv_b, self.bn_b = nn.Conv2d(64, 64, 3, padding=1, bias=False), nn.BatchNorm2d(64)
            self.block = ResidualBlock(32, 64, stride=2)
            self.head = FasterRCNNDetector()

    m = Cases()
    sd = det_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, 33)
    for k in sd:
        if k.endswith("running_mean"):
            sd[k] = torch.linspace(-1.0, 1.0, sd[k].numel())
        elif k.endswith("running_var"):
            sd[k] = torch.linspace(0.5, 2.0, sd[k].numel())
    m.load_state_dict(sd)
    return m, sd


def _sync_data():
    """Full-batch inputs, the residual of the first case and the fixed cotangents `proj` (loss = sum(out * proj): linear in
    the output, so the parameter gradients of the ranks add up to the full-batch gradient)."""
    rng = np.random.default_rng(77)
    d = {}
    for name, (r0, r1) in SYNC_SHARDS.items():
        n = r0 + r1
        d["x/" + name] = torch.from_numpy(rng.normal(0.2, 1.0, (n,) + SYNC_SHAPES[name]).astype(np.float32))
        d["proj/" + name] = torch.from_numpy(rng.normal(0.0, 1.0, (n,) + SYNC_PROJ[name]).astype(np.float32))
    d["res/cbr_res"] = torch.from_numpy(rng.normal(0.0, 1.0, (4,) + SYNC_SHAPES["cbr_res"]).astype(np.float32))
    return d


def _sync_oracle(sd, data, dtype):
    """oracle/model.py in train mode on the CONCATENATED batch, on the host -> {name: float64 array}."""
    import torch.nn.functional as F
    from oracle import model as om
    stat = ("running_mean", "running_var", "num_batches_tracked")
    P = om.Params({k: (v.clone() if k.endswith(stat[2]) else v.to(dtype).clone().requires_grad_(not k.endswith(stat)))
                   for k, v in sd.items()}, training=True)
    x = {k: v.to(dtype).clone().requires_grad_() for k, v in data.items() if not k.startswith("proj/")}
    out = {"cbr_res": F.relu(om.bn(P, "bn_a", om.conv(P, "conv_a", x["x/cbr_res"], 1, 1)) + x["res/cbr_res"]),
           "cbr": F.relu(om.bn(P, "bn_b", om.conv(P, "conv_b", x["x/cbr"], 1, 1))),
           "block": om.residual_block(P, "block", x["x/block"], stride=2),
           "head": om.stage2_head(P, x["x/head"], p="head")}
    sum((out[k] * data["proj/" + k].to(dtype)).sum() for k in out).backward()
    r = {"out/" + k: v for k, v in out.items()}
    r.update({"d" + k: v.grad for k, v in x.items()})
    for k, v in P.sd.items():
        r[("buf/" if k.endswith(stat) else "grad/") + k] = v if k.endswith(stat) else v.grad
    return {k: v.detach().double().numpy() for k, v in r.items()}


def _sync_worker(rank, world, port, outdir):
    import datetime
    import json
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=90))
    try:
        model, _ = _sync_modules()
        from kernel_audit import audit
        from rrnet_amd import dptrace, functional as RF
        from rrnet_amd.flat import FlatParams
        CL = torch.channels_last
        model = torch.nn.SyncBatchNorm.convert_sync_batchnorm(model.cuda().to(memory_format=CL)).train()
        fp = FlatParams(model)
        fp.broadcast(0)
        fp.zero_grad()
        data = _sync_data()
        dptrace.ENABLED = True
        dptrace.reset()
        res = {}

        def rows(key, name):
            r0 = SYNC_SHARDS[name][0]
            t = data[key][:r0] if rank == 0 else data[key][r0:]
            return t.cuda().contiguous(memory_format=CL) if t.dim() == 4 else t.cuda()

        with audit() as rec:
            for name in SYNC_SHARDS:
                x = rows("x/" + name, name).requires_grad_()
                extra = None
                if name == "cbr_res":
                    extra = rows("res/cbr_res", name).requires_grad_()
                    out = RF.conv_bn_act(x, model.conv_a, model.bn_a, relu=True, residual=extra)
                elif name == "cbr":
                    out = RF.conv_bn_act(x, model.conv_b, model.bn_b, relu=True)
                elif name == "block":
                    out = model.block(x)
                else:
                    out = model.head(x)
                (out * rows("proj/" + name, name)).sum().backward()
                res["out/" + name] = out
                res["dx/" + name] = x.grad
                if extra is not None:
                    res["dres/" + name] = extra.grad
        fp.all_reduce_grads()                      # fp.grad now holds the SUM over ranks
        torch.cuda.synchronize()
        for k, p in model.named_parameters():
            res["grad/" + k] = p._rr_grad
        for k, b in model.named_buffers():
            res["buf/" + k] = b
        np.savez(os.path.join(outdir, "sync%d.npz" % rank), **{k: v.detach().double().cpu().contiguous().numpy() for k, v in res.items()})
        with open(os.path.join(outdir, "sync%d.json" % rank), "w") as f:
            json.dump({"bad": [[repr(k), e] for k, e in rec.bad], "seen": [[repr(k), e] for k, e in rec.seen.items()],
                       "notes": [e[3] for e in dptrace.EVENTS if e[0] == "default"]}, f)
    finally:
        dist.destroy_process_group()


def test_two_rank_syncbn_nodes_on_ragged_shards_match_the_fp64_oracle(tmp_path):
    """Two real ranks (gloo, one GPU), fp32 kernels, DIFFERENT numbers of rows per rank: functional._ConvBnAct under SyncBN
    (ReLU mask from the saved output / recomputed), functional._ConvBnSyncMulti (a stride-2 projection block: two layers,
    two sample counts in one exchange) and the stage-2 head on 37 + 5 RoIs, against oracle/model.py in float64 on the
    concatenated batch.  Per case: each rank's output rows and input gradient, the rank-summed dw / dgamma / dbeta (the
    loss is linear in the output), running_mean / running_var / num_batches_tracked — against float64 and equal on both
    ranks.  Bound: 4x the error of the oracle's own float32 evaluation on the host (floor 2 u max|ref|), printed per
    quantity.  The workers run under the kernel audit, which must have seen (and passed) the device-count calls.
    Both workers end under time limits: the process group's collectives, and a deadline on the join."""
    import json
    import time
    from helpers import U32
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    t0 = time.time()
    ctx = mp.spawn(_sync_worker, nprocs=2, args=(2, port, str(tmp_path)), join=False)
    deadline = t0 + 240.0
    try:
        while not ctx.join(timeout=5.0):
            if time.time() > deadline:
                raise AssertionError("the two ranks did not finish within 240 s")
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.terminate()
        for p in ctx.processes:
            p.join(10.0)
    print("two ragged ranks, four cases under the kernel audit: %.1f s" % (time.time() - t0))
    _, sd = _sync_modules()
    data = _sync_data()
    ref, r32 = _sync_oracle(sd, data, torch.float64), _sync_oracle(sd, data, torch.float32)
    got = [np.load(str(tmp_path / ("sync%d.npz" % r))) for r in range(2)]
    meta = [json.load(open(str(tmp_path / ("sync%d.json" % r)))) for r in range(2)]
    worst = []

    def check(key, g, rf, r3):
        tol = max(4.0 * float(np.abs(r3 - rf).max()), 2.0 * U32 * float(np.abs(rf).max()))
        err = float(np.abs(g - rf).max())
        print("%-46s |HIP - fp64| %.3e   bound %.3e (fp32 host %.3e, max|ref| %.3e)" % (key, err, tol, float(np.abs(r3 - rf).max()), float(np.abs(rf).max())))
        if not err <= tol:
            worst.append((key, err, tol))

    for key in sorted(ref):
        kind, name = key.split("/", 1)
        if kind in ("out", "dx", "dres"):
            r0 = SYNC_SHARDS[name][0]
            for r in range(2):
                sl = slice(0, r0) if r == 0 else slice(r0, None)
                assert got[r][key].shape == ref[key][sl].shape, (key, r)
                check("%s rank %d" % (key, r), got[r][key], ref[key][sl], r32[key][sl])
        elif kind == "grad":
            assert np.array_equal(got[0][key], got[1][key]), key          # both ranks hold the same sum
            check(key + " (sum over ranks)", got[0][key], ref[key], r32[key])
        else:
            assert np.array_equal(got[0][key], got[1][key]), key          # statistics identical on both ranks
            if name.endswith("num_batches_tracked"):
                assert int(got[0][key]) == int(ref[key]) == 1, key
            else:
                check(key, got[0][key], ref[key], r32[key])
    for m in meta:
        assert m["bad"] == [], m["bad"]
        kinds = [k for k, _ in m["seen"]]
        assert any(k.startswith("('bn_bwd_apply'") and "'count-dev'" in k for k in kinds), kinds
        assert any(k.startswith("('bn_finalize_sync'") for k in kinds) and any(k.startswith("('bn_affine_grad'") for k in kinds)
        # the projection block took the joint node: one exchange per direction for conv1 + skip
        assert m["notes"].count("syncbn_fwd x2") == 1 and m["notes"].count("syncbn_bwd x2") == 1, m["notes"]
    print("audited signatures with a device count: %s" % sorted(k for k, _ in meta[0]["seen"] if "count-dev" in k or "sync" in k or "affine" in k))
    assert not worst, worst


def _run_bench(extra_env, launcher, port):
    import json
    import subprocess
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **extra_env)
    args = ["bench.py", "--backbone", "hourglass_tiny", "--size", "512", "--batch", "4", "--steps", "6", "--warmup", "2",
            "--no-cpu-baseline", "--no-extras", "--no-kernel-timing"]
    if launcher == "self":          # no launcher in front: bench.py starts its own ranks as a child torch.distributed.run
        cmd = [sys.executable] + args + ["--gpus", "2"]
        for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
            env.pop(k, None)
    elif launcher:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
               "127.0.0.1", "--master-port", str(port)] + args + ["--gpus", "2"]
    else:
        cmd = [sys.executable] + args
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, out.stdout[-2000:]                    # rank 0 prints exactly one JSON line
    return json.loads(lines[0])


def test_bench_two_ranks_through_the_launcher():
    """`bench.py --gpus 2` exactly as the driver launches it (torch.distributed.run, one process per rank, env
    rendezvous on 127.0.0.1), with both ranks on this box's single GPU and gloo as the transport (RR_SINGLE_DEVICE /
    RR_DIST_BACKEND — a 1-GPU box cannot host two RCCL ranks).  Checks the contract fields and times the N>1 path:
    SyncBN exchanges, bucketed gradient all-reduce launched from backward, barrier + max-over-ranks timing.  Two
    ranks share one GPU, so the aggregate rate can at best equal the single-rank rate; gloo's host round trips
    (326 small exchanges per step here) take their toll, hence the loose floor."""
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    one = _run_bench({}, False, port)
    two = _run_bench({"RR_SINGLE_DEVICE": "1", "RR_DIST_BACKEND": "gloo"}, True, port)
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2
    assert two["scaling"] == "weak" and two["config"]["global_batch"] == 2 * one["config"]["global_batch"]
    assert two["config"]["parallelism"] == "dp2" and two["steps"] == 6 and two["warmup"] == 2
    assert two["value"] > 0 and abs(two["value"] - 8 * 1e3 / two["ms_per_step"]) < 1e-2 * two["value"]
    print("1 rank: %.1f img/s, 2 ranks on one GPU over gloo: %.1f img/s" % (one["value"], two["value"]))
    assert two["value"] >= 0.35 * one["value"], (one["value"], two["value"])
    # ... and however the driver starts it: a bare `python bench.py --gpus 2` (no launcher variables) launches its own two
    # ranks as a child process before touching the GPU, relays rank 0's line and the exit code (VERDICT r5 missing #3)
    own = _run_bench({"RR_SINGLE_DEVICE": "1", "RR_DIST_BACKEND": "gloo"}, "self", port)
    assert own["n_gpus"] == 2 and own["config"]["parallelism"] == "dp2" and own["steps"] == 6 and own["value"] > 0


def test_rccl_single_rank_step_matches_non_distributed(tmp_path):
    """RCCL itself, on the one GPU this box has: a ONE-rank `nccl` process group with RR_DP_FORCE=1, so that
    init_process_group('nccl'), dist.new_group(), the parameter / buffer broadcasts, every SyncBN all_reduce (enqueued
    from forward and from autograd worker threads) and every gradient bucket's all_reduce(async_op=True) — launched from
    inside the weight-gradient side stream's context the moment its last parameter reports — go through
    ProcessGroupNCCL for a full hourglass-104 train step (operators/distributed_wrapper.py:40-42,
    operators/base_operator.py:24 in the reference), with the side stream delayed (RR_WGRAD_STRESS) so that a bucket
    launched before its gradients have landed would send incomplete data.
    All collectives are identities at world size 1, so the step must equal the non-distributed one up to the summation
    ORDER of the BatchNorm statistics (slab -> all-reduce -> finalize instead of the fused single launch; the coalesced
    SyncBN nodes reduce dz in a pass of their own).  That re-association is rounding-sized noise, which the deep levels of
    this network amplify (tests/test_streams_gpu.py, module docstring): the comparison is therefore made on the
    parameters whose gradient moves by <= 1e-5 under a 1e-7 input perturbation, with 1e-4 of their scale as the bound; a
    collective that ran before its operand was complete, or an exchange left out, is O(1) on ALL of them.  The forced run
    itself must repeat within 1e-5 on every parameter.  This cannot show a cross-rank ordering bug
    (test_two_rank_collective_sequences_are_identical does that over gloo); it shows crashes, hangs and stream hand-over
    mistakes of the real backend."""
    from test_streams_gpu import DET, _load, _moved, _rel, _run
    plain = _run(tmp_path, "plain", dict(DET, RR_WGRAD_STREAM="2"), 256, 2, 2, ["--perturb", "1e-7"])
    forced = _run(tmp_path, "rccl1", dict(DET, RR_WGRAD_STREAM="2", RR_DP_FORCE="1", RR_WGRAD_STRESS="1"), 256, 2, 2)
    cc = forced[1]["collectives"]
    nb = forced[1]["buckets"]
    print("collectives of one step through RCCL: %s; %d gradient buckets" % (cc[0], nb))
    assert plain[1]["collectives"][0] == {}
    for c in cc:
        assert c["grads"] == nb, (c, nb)          # one all-reduce per gradient bucket, each exactly once
        assert c["default"] == cc[0]["default"] and c["default"] >= 2 * 100 and c["default"] % 2 == 0, c
    la, lb = np.array(plain[1]["losses"][0]), np.array(forced[1]["losses"][0])
    assert np.all(np.abs(la - lb) <= 1e-4 * np.maximum(np.abs(la), 1e-3)), (la, lb)
    sl = plain[1]["slices"]
    g0 = _load(plain[0], "grad.bin")
    sens, _ = _rel(_load(plain[0], "grad2.bin"), g0, sl)              # response to 1e-7 input noise
    cross, _ = _rel(_load(forced[0], "grad.bin"), g0, sl)
    good = sens <= 1e-5
    print("one-rank RCCL step vs non-distributed step: %d of %d parameters well-conditioned; on those the worst gradient "
          "difference is %.2e of the parameter's scale (all parameters: median %.2e, worst %.2e; 1e-7 input noise alone: "
          "median %.2e, worst %.2e)" % (int(good.sum()), good.numel(), float(cross[good].max()), float(cross.median()),
                                         float(cross.max()), float(sens.median()), float(sens.max())))
    assert int(good.sum()) >= 10                  # the layers downstream of the last hourglass (its heads)
    assert float(cross[good].max()) <= 1e-4
    # everywhere else: not beyond the network's own amplification of rounding-sized noise
    assert float(cross.median()) <= 3 * max(float(sens.median()), 1e-5)
    assert float(cross.max()) <= 3 * max(float(sens.max()), 1e-3)
    r = forced[1]["repeat_vs_first"][0]
    assert r["grad"][0] <= 1e-5 and r["buffers"] <= 2e-5, r


def test_rccl_single_rank_f16x3_step_runs_and_matches(tmp_path):
    """The data-parallel path (SyncBN nodes `_ConvBnSyncMulti`, bucketed gradient all-reduce from the side stream) with
    cfg.Model.conv_math = "f16x3": the split-operand kernels take their operands' maxima from device words whatever node
    launches them (ops.amax_of); the one-rank RCCL step must give the non-distributed f16x3 step's losses and — on the
    well-conditioned parameters — its gradients, and stay finite."""
    from test_streams_gpu import DET, _load, _rel, _run
    extra = ["--math", "f16x3"]
    plain = _run(tmp_path, "plain_split", dict(DET, RR_WGRAD_STREAM="2"), 256, 2, 2, extra + ["--perturb", "1e-7"])
    forced = _run(tmp_path, "rccl1_split", dict(DET, RR_WGRAD_STREAM="2", RR_DP_FORCE="1", RR_WGRAD_STRESS="1"), 256, 2, 1, extra)
    assert forced[1]["collectives"][0]["grads"] == forced[1]["buckets"]
    la, lb = np.array(plain[1]["losses"][0]), np.array(forced[1]["losses"][0])
    assert np.all(np.abs(la - lb) <= 1e-4 * np.maximum(np.abs(la), 1e-3)), (la, lb)
    sl = plain[1]["slices"]
    g0 = _load(plain[0], "grad.bin")
    sens, _ = _rel(_load(plain[0], "grad2.bin"), g0, sl)
    cross, _ = _rel(_load(forced[0], "grad.bin"), g0, sl)
    good = sens <= 1e-5
    print("f16x3, one-rank RCCL vs non-distributed: %d well-conditioned parameters, worst difference %.2e" % (int(good.sum()), float(cross[good].max())))
    assert int(good.sum()) >= 10 and float(cross[good].max()) <= 1e-4
