"""What a checkpoint costs the training loop: the reference-format save_ckp against the full-state save.

  python tools/bench_state.py [--backbone hourglass] [--repeats 10] [--dir TMP] [--out profiles/state.json]

hourglass-104 RRNet with random weights and zero moments (no training step is needed), one MI355X.  Reports
  save_ckp_ms            wall time of BaseOperator.save_ckp on the training thread, a device synchronise on either side
  save_state_call_ms     wall time of save_state, call to return (the first call, which allocates staging, separately)
  snapshot_device_ms     device time of the three rr_state_snapshot launches (HIP events)
  copy_device_ms         device time of three plain dst.copy_(src) over the same buffers, same process, alternating
  digest_only_device_ms  the three launches with dst = NULL (what load_state's verification costs)
  state_file_ms          save_state call until state-N.pth is in place
  load_state_ms          load_state, synchronised
Every list is one value per repeat; median, min and max are given beside it."""
import argparse
import copy
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": [round(x, 4) for x in v]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--backbone", default="hourglass")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--file-repeats", type=int, default=3)
    ap.add_argument("--dir", help="where the files go (default: a temporary directory, removed afterwards)")
    ap.add_argument("--out")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_state.py needs the GPU")
    from rrnet_amd import checkpoint, ops
    from rrnet_amd.configs.rrnet_config import Config
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    cfg = copy.deepcopy(Config)
    cfg.Model.backbone = a.backbone
    cfg.Distributed.gpu_id, cfg.Distributed.rank, cfg.Distributed.world_size = 0, 0, 1
    torch.cuda.set_device(0)
    torch.manual_seed(219)
    op = RRNetOperator(cfg)
    fp, opt = op.optimizer.fp, op.optimizer
    n = fp.numel
    work = a.dir or tempfile.mkdtemp(prefix="rr_state_bench_")
    os.makedirs(work, exist_ok=True)
    sync = torch.cuda.synchronize
    res = {"backbone": a.backbone, "numel": n, "tensors_in_state_dict": len(op.model.module.state_dict()),
           "bytes_per_buffer": 4 * n, "device": torch.cuda.get_device_name(0), "chunk": checkpoint.CHUNK}

    # device time: snapshot (copy + digest), plain copy, digest only -- alternating, after a warm-up of each
    srcs = (fp.flat, opt.exp_avg, opt.exp_avg_sq)
    dsts = [torch.empty_like(fp.flat) for _ in srcs]
    nch = (n + checkpoint.CHUNK - 1) // checkpoint.CHUNK
    dig = torch.empty((3, nch, 3), dtype=torch.int64, device=fp.flat.device)

    def snap():
        for i, s in enumerate(srcs):
            ops.state_snapshot(s, dsts[i], checkpoint.CHUNK, out=dig[i])

    def plain():
        for i, s in enumerate(srcs):
            dsts[i].copy_(s)

    def digest_only():
        for i, s in enumerate(srcs):
            ops.state_snapshot(s, None, checkpoint.CHUNK, out=dig[i])

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        sync()
        return e0.elapsed_time(e1)
    for fn in (snap, plain, digest_only) * 2:
        timed(fn)
    t = {"snap": [], "plain": [], "digest": []}
    for _ in range(a.repeats):
        t["snap"].append(timed(snap))
        t["plain"].append(timed(plain))
        t["digest"].append(timed(digest_only))
    res["snapshot_device_ms"], res["copy_device_ms"] = _stats(t["snap"]), _stats(t["plain"])
    res["digest_only_device_ms"] = _stats(t["digest"])
    gb = 3 * 8 * n / 1e9                              # read + write of three buffers
    res["snapshot_GBps"] = gb / (res["snapshot_device_ms"]["median"] * 1e-3)
    res["copy_GBps"] = gb / (res["copy_device_ms"]["median"] * 1e-3)
    res["snapshot_over_copy"] = res["snapshot_device_ms"]["median"] / res["copy_device_ms"]["median"]
    for i, s in enumerate(srcs):
        assert torch.equal(dsts[i], s)
    del dsts

    # the blocking cost today
    ck = []
    for r in range(a.file_repeats):
        sync()
        t0 = time.perf_counter()
        op.save_ckp(op.model.module, r, work)
        sync()
        ck.append((time.perf_counter() - t0) * 1e3)
        os.remove(os.path.join(work, "ckp-%d.pth" % r))
    res["save_ckp_ms"] = _stats(ck)

    # the full-state save: call to return, call to file
    calls, files = [], []
    for r in range(a.file_repeats + 1):
        sync()
        t0 = time.perf_counter()
        op.save_state(r, work)
        t1 = time.perf_counter()
        op._state_writer._collect()
        t2 = time.perf_counter()
        assert os.path.exists(os.path.join(work, "state-%d.pth" % r))
        calls.append((t1 - t0) * 1e3)
        files.append((t2 - t0) * 1e3)
    res["save_state_first_call_ms"] = calls[0]            # allocates 3 x numel floats on the device and pinned on the host
    res["save_state_call_ms"] = _stats(calls[1:])
    res["state_file_ms"] = _stats(files[1:])
    op.close_state()
    path = checkpoint.latest_state(work)
    res["state_file_bytes"] = os.path.getsize(path)
    ld = []
    for _ in range(a.file_repeats):
        sync()
        t0 = time.perf_counter()
        start = op.load_state(path)
        sync()
        ld.append((time.perf_counter() - t0) * 1e3)
    assert start == a.file_repeats + 1
    res["load_state_ms"] = _stats(ld)
    if not a.dir:
        shutil.rmtree(work, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
