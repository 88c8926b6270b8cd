"""Fuse the VisDrone result folders of several runs into one: weighted boxes fusion on the device (rrnet_amd/ensemble.py).

  python tools/ensemble.py --runs DIR [DIR ...] --out DIR [--weights W ...] [--iou 0.55] [--skip-score S]
                           [--conf avg|max] [--max-det 500] [--method wbf|soft-nms] [--targets DIR]

Every run is a folder of <frame>.txt files as tools/detect.py and RRNetOperator.write_results write them
(x,y,w,h,score,cls,-1,-1).  The file names are the union over the runs; a file that a run lacks counts as no detections of
that run, and the number of such files is printed.  --method wbf (default) averages the boxes of a group, weighted by
confidence; --method soft-nms sends the concatenation of the runs through the evaluator's per-class gaussian Soft-NMS
(utils.metrics.ext_nms_batch, --skip-score as its score threshold): the baseline to compare against.  With --targets the AP
of every input run and of the fused output is printed (the device evaluator)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", nargs="+", required=True, metavar="DIR", help="result folders, one per run")
    ap.add_argument("--out", required=True, metavar="DIR", help="folder the fused files go to")
    ap.add_argument("--weights", nargs="+", type=float, default=None, metavar="W", help="one weight per run (default 1)")
    ap.add_argument("--iou", type=float, default=0.55, help="a row joins a cluster above this IoU with its fused box")
    ap.add_argument("--skip-score", type=float, default=0.0, help="rows with weighted score <= this are dropped")
    ap.add_argument("--conf", choices=("avg", "max"), default="avg")
    ap.add_argument("--max-det", type=int, default=500, help="rows kept per frame")
    ap.add_argument("--method", choices=("wbf", "soft-nms"), default="wbf")
    ap.add_argument("--targets", default=None, metavar="DIR", help="annotation folder: print the AP of the runs and the output")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--host-text", action="store_true",
                    help="read and write the files on the host (pandas, formatted writes) instead of on the device")
    args = ap.parse_args(argv)
    if args.weights is not None:
        if len(args.weights) != len(args.runs):
            ap.error("--weights: %d values for %d runs" % (len(args.weights), len(args.runs)))
        if not all(np.isfinite(w) and w > 0 for w in args.weights):
            ap.error("--weights must be positive and finite")
    if not (np.isfinite(args.skip_score) and args.skip_score >= 0):
        ap.error("--skip-score must be >= 0")
    if not np.isfinite(args.iou):
        ap.error("--iou must be finite")
    if args.max_det < 1:
        ap.error("--max-det must be at least 1")
    for d in args.runs:
        if not os.path.isdir(d):
            ap.error("--runs: %s is not a folder" % d)
        if os.path.abspath(d) == os.path.abspath(args.out):
            ap.error("--out must not be one of the runs")
    if args.targets is not None and not os.path.isdir(args.targets):
        ap.error("--targets: %s is not a folder" % args.targets)
    return args


def soft_nms_dirs(dirs, out_dir, threshold, max_det, text="host"):
    """The baseline: per frame the concatenation of the runs through ext_nms_batch, score-descending, max_det rows."""
    from rrnet_amd import ensemble
    from rrnet_amd.utils.metrics.metrics import ext_nms_batch
    names, sets, missing = ensemble.read_result_dirs(dirs, text=text)
    print("%d files of %d runs, %d missing (counted as no detections)" % (len(names), len(dirs), missing))
    cat = [np.concatenate([np.asarray(s[f])[:, :6] for s in sets], 0).astype(np.float32) for f in range(len(names))]
    kept = ext_nms_batch(cat, threshold) if names else []
    frames = [k[np.argsort(-k[:, 4], kind="stable")][:max_det] for k in kept]
    ensemble.write_result_dir(out_dir, names, frames, text=text)
    return missing


def main(argv=None):
    args = parse_args(argv)
    import torch
    from rrnet_amd import ensemble
    torch.cuda.set_device(args.device)
    text = "host" if args.host_text else "device"
    if args.method == "wbf":
        ensemble.fuse_result_dirs(args.runs, args.out, weights=args.weights, iou_thr=args.iou, skip_score=args.skip_score,
                                  conf_type=args.conf, max_det=args.max_det, text=text)
    else:
        soft_nms_dirs(args.runs, args.out, args.skip_score, args.max_det, text=text)
    print("wrote %s" % args.out)
    if args.targets is not None:
        from rrnet_amd.utils.metrics.metrics import evaluate_results, text_route
        dev = torch.device("cuda", args.device)
        for d in list(args.runs) + [args.out]:
            print("== %s" % d)
            with text_route(text):
                evaluate_results(d, args.targets, max_det_num=args.max_det, device=dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
