"""Time of one VisDrone evaluation and of the (ctnet_min, softnms_min) sweep, host evaluator against device evaluator.

Generates a seeded temporary directory of result / annotation text files in save_result's layout (548 files, 500
detections and 120 annotations each, ignored regions in every third file: the size of VisDrone's validation split at
max_det_num) and times
  * evaluate_results on the host (get_tp / calculate_ap_rc, the functions as they were before the device path),
  * evaluate_results(device=...), and its three parts: parse (read, snap, cut), upload, kernels (sort, rr_eval_match,
    list building, rr_eval_ap),
  * ONE auto_evaluate_results pair on the host (files re-read, Soft-NMS on the GPU, matching on the host),
  * sweep_evaluate_results(device=...) over scripts/RRNet/auto_eval.py's 4 x 10 threshold pairs.
It asserts that host and device AP / AR agree (rtol 1e-5, atol 1e-6) on evaluate_results and on the pair both run.
Scores are written with six decimals and are pairwise distinct over the whole set: on equal scores the host order is
whatever torch's unstable sort gives, the device order is defined as stable, and the two only have to agree without
ties.  Every timed section ends in a device synchronise.  One JSON line on stdout; --out writes the object to a file.

  python tools/bench_eval.py [--files 548] [--dets 500] [--annos 120] [--out profiles/eval_device.json]"""
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

CTNET_MIN = [0.05, 0.08, 0.10, 0.20]
SOFTNMS_MIN = [0.01, 0.02, 0.03, 0.04, 0.05, 0.06, 0.07, 0.08, 0.09, 0.1]


def write_files(root, n_files, n_det, n_gt, seed=219, size=(1360, 765)):
    pd_dir, gt_dir = os.path.join(root, "pred"), os.path.join(root, "gt")
    os.makedirs(pd_dir), os.makedirs(gt_dir)
    rng = np.random.default_rng(seed)
    assert n_files * n_det < 1000000
    scores = (rng.permutation(999999)[:n_files * n_det] + 1).reshape(n_files, n_det) / 1e6
    for i in range(n_files):
        gt = np.zeros((n_gt, 8), np.int64)
        gt[:, 0] = rng.integers(0, size[0] - 160, n_gt)
        gt[:, 1] = rng.integers(0, size[1] - 160, n_gt)
        gt[:, 2:4] = np.exp(rng.uniform(np.log(8), np.log(160), (n_gt, 2))).astype(np.int64)
        gt[:, 4] = 1
        gt[:, 5] = rng.integers(1, 11, n_gt)
        if i % 3 == 0:                                          # three ignored regions
            gt[:3, 2:4] = (200, 120)
            gt[:3, 4:6] = 0
        src = rng.integers(0, n_gt, n_det)
        det = gt[src, :4].astype(np.float64) + rng.normal(0, 3, (n_det, 4))
        det[:, 2:4] = np.maximum(det[:, 2:4], 1.0)
        cls = np.where(gt[src, 5] > 0, gt[src, 5], 1)
        stray = rng.random(n_det) < 0.3                         # boxes that copy nothing
        det[stray, 0] = rng.uniform(0, size[0] - 160, int(stray.sum()))
        det[stray, 1] = rng.uniform(0, size[1] - 160, int(stray.sum()))
        cls[stray] = rng.integers(1, 11, int(stray.sum()))
        order = np.argsort(-scores[i])
        with open(os.path.join(pd_dir, "%07d.txt" % i), "w") as f:
            f.write("".join('%f,%f,%f,%f,%.6f,%d,-1,-1\n' % (det[k, 0], det[k, 1], det[k, 2], det[k, 3], scores[i, k], cls[k])
                            for k in order))
        with open(os.path.join(gt_dir, "%07d.txt" % i), "w") as f:
            f.write("".join(",".join(str(v) for v in r) + "\n" for r in gt))
    return pd_dir, gt_dir


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--files", type=int, default=548)
    ap.add_argument("--dets", type=int, default=500)
    ap.add_argument("--annos", type=int, default=120)
    ap.add_argument("--out", default=None)
    ap.add_argument("--host-text", action="store_true", help="the device line parses the files on the host (pandas), as before")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures on the GPU; none is visible")
    from rrnet_amd.utils.metrics import metrics as M
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)

    def timed(fn, *args, **kw):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            out = fn(*args, **kw)
        torch.cuda.synchronize()
        return out, time.perf_counter() - t0

    def agree(got, ref, what):
        worst = float((got[0] - ref[0]).abs().max())
        np.testing.assert_allclose(got[0].numpy(), ref[0].numpy(), rtol=1e-5, atol=1e-6, err_msg=what)
        np.testing.assert_allclose(float(got[1]), float(ref[1]), rtol=1e-5, atol=1e-6, err_msg=what)
        return worst

    res = {"tool": "bench_eval", "files": a.files, "detections_per_file": a.dets, "annotations_per_file": a.annos,
           "thresholds": int(M.THRESHOLDS.numel()), "device": torch.cuda.get_device_name(0)}
    with tempfile.TemporaryDirectory() as root:
        pd_dir, gt_dir = write_files(root, a.files, a.dets, a.annos)
        timed(M.evaluate_arrays, [np.zeros((1, 6), np.float32)], [np.zeros((1, 8), np.float32)], device=dev)   # warm-up
        print("host evaluate_results ...", file=sys.stderr, flush=True)
        host, res["host_evaluate_results_s"] = timed(M.evaluate_results, pd_dir, gt_dir)
        print("device evaluate_results ...", file=sys.stderr, flush=True)
        text = "host" if a.host_text else "device"
        res["text"] = text
        with M.text_route(text):
            timed(M.evaluate_results, pd_dir, gt_dir, device=dev)                        # warm-up of the text route
            got, total = timed(M.evaluate_results, pd_dir, gt_dir, device=dev)

        max_det = 500                                           # the drivers' default max_det_num

        def parse():
            preds, targets = [], []
            read = M._reader(pd_dir, gt_dir, text, dev)           # pandas per file, or one pass of rrnet_amd.textio
            for name in M._names(pd_dir):
                pred = M._snap(read(os.path.join(pd_dir, name + ".txt")).astype(np.float64))
                preds.append(torch.from_numpy(pred).float()[:max_det, :6])
                targets.append(torch.from_numpy(read(os.path.join(gt_dir, name + ".txt"))).float()[:max_det, :6])
            return preds, targets
        (preds, targets), t_parse = timed(parse)
        (dets, det_len, gts, gt_len), t_up = timed(lambda: M._pad(preds, dev) + M._pad(targets, dev))
        _, t_kern = timed(lambda: M._device_eval(M._sort_frames(dets, det_len), det_len, gts, gt_len, M.THRESHOLDS, 11))
        res["device_evaluate_results"] = {"total_s": total, "parse_s": t_parse, "upload_s": t_up, "kernels_s": t_kern,
                                          "ap_max_abs_diff_to_host": agree(got, host, "evaluate_results")}
        res["ap"] = [float(v) for v in host[0]]
        print("host auto_evaluate_results pair ...", file=sys.stderr, flush=True)
        pair, res["host_auto_pair_s"] = timed(M.auto_evaluate_results, pd_dir, gt_dir, CTNET_MIN[0], SOFTNMS_MIN[0])
        print("device sweep ...", file=sys.stderr, flush=True)
        with M.text_route(text):
            sweep, t_sweep = timed(M.sweep_evaluate_results, pd_dir, gt_dir, CTNET_MIN, SOFTNMS_MIN, device=dev)
        first = (torch.from_numpy(sweep[0, 0, :-1]), torch.tensor(sweep[0, 0, -1]))
        res["device_sweep"] = {"pairs": len(CTNET_MIN) * len(SOFTNMS_MIN), "total_s": t_sweep,
                               "per_pair_s": t_sweep / (len(CTNET_MIN) * len(SOFTNMS_MIN)),
                               "ap_max_abs_diff_to_host_pair": agree(first, pair, "sweep pair")}
        res["host_sweep_extrapolated_s"] = res["host_auto_pair_s"] * len(CTNET_MIN) * len(SOFTNMS_MIN)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
