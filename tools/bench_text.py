"""Times the device-side text codec (rrnet_amd/textio.py, csrc/textio.hip) against the host route it replaces, in the same
process on the same files -> profiles/textio.json.  Reported, not asserted (the equalities are the tests' business).

  reading   the generated folders of tools/bench_eval.py (548 result + 548 annotation files, 500 / 120 rows) and of
            tools/bench_wbf.py (3 x 548 result files): metrics._read per file against textio.read_files, split into file
            read / upload / kernels / download, the launches alone between HIP events, and the share of files that took the
            host route;
  writing   128 808 rows in 548 frames and one 9000-row frame: the host expression against textio.write_frames, split
            into kernels / download / file write, and rr_text_format_len / rr_text_format alone between HIP events;
  end to end  evaluate_results(device=...) and fuse_result_dirs with text="host" and text="device".

  python tools/bench_text.py [--files 548] [--out profiles/textio.json]"""
import argparse
import contextlib
import io
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

REPS = 5


def best_of(fn, reps=REPS):
    import torch
    best, out = None, None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None or dt < best else best
    return best, out


def events_ms(fn, reps=REPS):
    import torch
    best = None
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None or ms < best else best
    return best


def bench_read(paths, dev, host_read):
    import torch
    from rrnet_amd import ops, textio
    res = {"files": len(paths), "bytes": int(sum(os.path.getsize(p) for p in paths))}
    res["host_read_s"], ref = best_of(lambda: [host_read(p) for p in paths], reps=3)
    textio.read_files(paths[:4], dev, host_read=host_read)                       # first-launch costs stay out
    best = None
    for _ in range(REPS):
        timing = {}
        t0 = time.perf_counter()
        arrays, n_host = textio.read_files(paths, dev, host_read=host_read, timing=timing)
        timing["total"] = time.perf_counter() - t0
        best = timing if best is None or timing["total"] < best["total"] else best
    res["device_read_s"] = {k: round(v, 5) for k, v in best.items()}
    res["files_on_host_route"] = n_host
    res["rows"] = int(sum(a.shape[0] for a in arrays))
    res["equal_to_host"] = bool(all(np.array_equal(a.view(np.int64), np.asarray(r)[:, :8].astype(np.float64).view(np.int64))
                                    for a, r in zip(arrays, ref)))
    blob = b"".join(open(p, "rb").read() for p in paths)
    off = np.cumsum([0] + [os.path.getsize(p) for p in paths]).astype(np.int64)
    text, foff = torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev), torch.from_numpy(off).to(dev)
    line_pos, _ = ops.text_lines(text, foff)
    res["kernels_event_ms"] = {"lines (count, host sum of the blocks, scatter, file offsets)": round(events_ms(lambda: ops.text_lines(text, foff)), 4),
                               "parse": round(events_ms(lambda: ops.text_parse(text, line_pos, 8)), 4)}
    res["host_over_device"] = round(res["host_read_s"] / best["total"], 2)
    return res


def frames_of(nrows, nframes, seed):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, 1900, (nrows, 2)); wh = rng.uniform(1, 300, (nrows, 2))
    rows = np.concatenate([xy, wh, rng.uniform(0.01, 1, (nrows, 1)), rng.integers(1, 11, (nrows, 1))], 1).astype(np.float32)
    cuts = np.sort(rng.integers(0, nrows + 1, nframes - 1))
    return rows, np.concatenate([[0], cuts, [nrows]]).astype(np.int64)


def format_kernel_ms(nrows, nframes, dev):
    import torch
    from rrnet_amd import ops
    rows, _ = frames_of(nrows, nframes, 7)
    d = torch.from_numpy(rows).to(dev)
    length, flag, byte_off = ops.text_format_len(d, 0, 1)
    buf = torch.empty(int(byte_off[-1]), dtype=torch.uint8, device=dev)
    return {"rows": nrows, "bytes": buf.numel(), "format_len_ms": round(events_ms(lambda: ops.text_format_len(d, 0, 1)), 4),
            "format_ms": round(events_ms(lambda: ops.text_format(d, 0, 1, byte_off, buf)), 4)}


def bench_write(nrows, nframes, dev, root, tag):
    import torch
    from rrnet_amd import textio
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    rows, off = frames_of(nrows, nframes, 7)
    names = ["%07d" % i for i in range(nframes)]
    host_dir, dev_dir = os.path.join(root, tag + "_host"), os.path.join(root, tag + "_dev")
    os.makedirs(host_dir), os.makedirs(dev_dir)

    def host():
        for i, n in enumerate(names):
            RRNetOperator.write_results(os.path.join(host_dir, n + ".txt"), rows[off[i]:off[i + 1]])
    res = {"rows": nrows, "frames": nframes}
    res["host_write_s"], _ = best_of(host, reps=3)
    res["host_format_only_s"], _ = best_of(lambda: [textio.format_rows_host(rows[off[i]:off[i + 1]], 0, 1) for i in range(nframes)], reps=3)
    d = torch.from_numpy(rows).to(dev)
    paths = [os.path.join(dev_dir, n + ".txt") for n in names]
    textio.write_frames(paths, d, off, 0, True)
    best = None
    for _ in range(REPS):
        timing = {}
        t0 = time.perf_counter()
        textio.write_frames(paths, d, off, 0, True, timing=timing)
        timing["total"] = time.perf_counter() - t0
        best = timing if best is None or timing["total"] < best["total"] else best
    res["device_write_s"] = {k: round(v, 5) for k, v in best.items()}
    res["equal_to_host"] = all(open(os.path.join(host_dir, n + ".txt"), "rb").read() == open(os.path.join(dev_dir, n + ".txt"), "rb").read()
                               for n in names)
    res["host_over_device"] = round(res["host_write_s"] / best["total"], 2)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--files", type=int, default=548)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "textio.json"))
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_text.py measures on the GPU; none is visible")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    import bench_eval
    import bench_wbf
    from rrnet_amd import ensemble
    from rrnet_amd.utils.metrics import metrics as M
    res = {"tool": "bench_text", "device": torch.cuda.get_device_name(0), "files": a.files}
    with tempfile.TemporaryDirectory() as root:
        pd_dir, gt_dir = bench_eval.write_files(os.path.join(root, "eval"), a.files, 500, 120)
        runs = bench_wbf.gen_result_dirs(os.path.join(root, "wbf"), a.files, np.random.default_rng(548))
        eval_paths = [os.path.join(d, n) for d in (pd_dir, gt_dir) for n in sorted(os.listdir(d))]
        wbf_paths = [os.path.join(d, n) for d in runs for n in sorted(os.listdir(d))]
        print("reading ...", file=sys.stderr, flush=True)
        res["read_eval_folders"] = bench_read(eval_paths, dev, M._read)
        res["read_wbf_folders"] = bench_read(wbf_paths, dev, ensemble._read_or_empty)
        print("writing ...", file=sys.stderr, flush=True)
        res["write_128808_rows"] = bench_write(128808, a.files, dev, root, "w548")
        res["write_one_9000_row_frame"] = bench_write(9000, 1, dev, root, "w1")
        res["format_kernel_event_ms"] = [format_kernel_ms(128808, 548, dev), format_kernel_ms(9000, 1, dev)]
        print("end to end ...", file=sys.stderr, flush=True)
        e2e = {}
        for text in ("host", "device"):
            with M.text_route(text):
                t, got = best_of(lambda: M.evaluate_results(pd_dir, gt_dir, device=dev), reps=4)
            e2e["evaluate_results_%s_text_s" % text] = round(t, 4)
            e2e["ap_%s" % text] = [float(v) for v in got[0]]
        e2e["ap_equal"] = e2e.pop("ap_host") == e2e["ap_device"]
        kw = dict(weights=[2.0, 1.0, 1.0], iou_thr=0.55, skip_score=0.05, conf_type="avg", max_det=500)
        for text in ("host", "device"):
            with contextlib.redirect_stdout(io.StringIO()):
                ensemble.fuse_result_dirs(runs, os.path.join(root, "warm_" + text), text=text, **kw)
            best = None
            for rep in range(3):
                timing = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    ensemble.fuse_result_dirs(runs, os.path.join(root, "fused_%s%d" % (text, rep)), timing=timing, text=text, **kw)
                timing["total"] = time.perf_counter() - t0
                best = timing if best is None or timing["total"] < best["total"] else best
            e2e["fuse_result_dirs_%s_text_s" % text] = {k: round(v, 4) for k, v in best.items()}
        names = sorted(os.listdir(os.path.join(root, "fused_host0")))
        e2e["fused_files_equal"] = all(open(os.path.join(root, "fused_host0", n), "rb").read()
                                       == open(os.path.join(root, "fused_device0", n), "rb").read() for n in names)
        t0 = time.perf_counter()
        for d in runs:
            os.listdir(d)
        e2e["listdir_3_folders_s"] = round(time.perf_counter() - t0, 5)
        res["end_to_end"] = e2e
    for k in ("read_eval_folders", "read_wbf_folders", "write_128808_rows", "write_one_9000_row_frame"):
        for kk, v in list(res[k].items()):
            if isinstance(v, float):
                res[k][kk] = round(v, 5)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
