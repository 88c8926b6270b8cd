"""Detect on a folder of images: RRNet or CenterNet multi-scale inference, one VisDrone result file per image.

  python tools/detect.py --checkpoint ckp-89999.pth --images DIR --out DIR [--config rrnet_config] [--batch 4]
                         [--scales 1,1.1,1.2,1.3,1.4,1.5] [--raw | --nms] [--bf16] [--flip | --no-flip]
                         [--random-weights]

Frames are decoded in threads, grouped by size, uploaded as uint8 and run `--batch` at a time through
rrnet_amd.inference.detect_frames; every image gets `<out>/<name>.txt` with the lines `x,y,w,h,score,cls,-1,-1` that
RRNetOperator.save_result writes (utils/metrics reads them).  --raw keeps every box of every scale (the config's
auto_test=True, for a later threshold sweep); --nms filters by score and runs the per-class Soft-NMS (auto_test=False);
without either the config decides.  --random-weights runs without a checkpoint (a smoke run: the boxes mean nothing).

--config centernet_config runs CenterNet through rrnet_amd.inference.detect_frames_centernet and writes the integer lines
of CenterNetOperator.save_result.  Every scale is run flipped and plain in one model pass, as the reference's evaluation
does (--no-flip: plain only).  CenterNet is fp32 only: --bf16 is refused with it."""
import argparse
import copy
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ("rrnet_config", "rrnet_fillduck_config", "centernet_config")


def load_config(name):
    if name not in CONFIGS:
        raise SystemExit("unknown config %r (one of %s)" % (name, ", ".join(CONFIGS)))
    return copy.deepcopy(importlib.import_module("rrnet_amd.configs." + name).Config)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--config", default="rrnet_config")
    ap.add_argument("--checkpoint")
    ap.add_argument("--images", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--scales", help="comma-separated factors; default: the config's Val.scales")
    mode = ap.add_mutually_exclusive_group()
    mode.add_argument("--raw", action="store_true")
    mode.add_argument("--nms", action="store_true")
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--flip", dest="flip", action="store_true", default=True,
                    help="CenterNet: every scale flipped and plain, as the reference evaluates (default)")
    ap.add_argument("--no-flip", dest="flip", action="store_false", help="CenterNet: the plain image only")
    ap.add_argument("--random-weights", action="store_true")
    ap.add_argument("--workers", type=int, default=8)
    args = ap.parse_args(argv)
    cfg = load_config(args.config)
    if (args.checkpoint is None) == (not args.random_weights):
        raise SystemExit("give --checkpoint FILE or --random-weights (one of them)")
    centernet = args.config.startswith("centernet")
    if args.bf16 and centernet:
        raise SystemExit("--bf16: CenterNet runs in fp32 only (the model has no bf16 scope)")
    if args.bf16:
        cfg.Model.bf16 = True
    scales = [float(s) for s in args.scales.split(",")] if args.scales else list(cfg.Val.scales)
    nms = True if args.nms else False if args.raw else not cfg.Val.auto_test

    import torch
    from rrnet_amd import ops
    from rrnet_amd.datasets.frames import FrameFolder, SizeBucketedFrames
    from rrnet_amd import inference
    if centernet:
        from rrnet_amd.operators.centernet_operator import CenterNetOperator as Operator
        per_scale, what = (2 if args.flip else 1) * 250, "%d x 250" % (2 if args.flip else 1)
    else:
        from rrnet_amd.operators.rrnet_operator import RRNetOperator as Operator
        per_scale, what = 1500, "1500"
    if len(scales) * per_scale > ops.DETECT_MAX_ROWS:
        raise SystemExit("%d scales x %s boxes exceed %d rows per frame" % (len(scales), what, ops.DETECT_MAX_ROWS))
    if not torch.cuda.is_available():
        raise SystemExit("tools/detect.py needs the GPU (there is no CPU path)")
    folder = FrameFolder(args.images)
    if len(folder) == 0:
        raise SystemExit("no images in %s" % args.images)
    os.makedirs(args.out, exist_ok=True)
    torch.manual_seed(219)
    checkpoint = None if args.random_weights else args.checkpoint
    if centernet:
        detector = inference.CenterNetFrameDetector(cfg, checkpoint)
        extra = dict(flip=args.flip)
    else:
        detector = inference.Detector(cfg, checkpoint)
        extra = {}
    t0, frames_done, boxes_done = time.perf_counter(), 0, 0
    for frames_u8, names in SizeBucketedFrames(folder, args.batch, num_workers=args.workers):
        boxes, frame_off = detector.detect(frames_u8, scales=scales, nms=nms, **extra)
        rows, off = boxes.cpu().numpy(), frame_off.cpu().tolist()             # one copy per batch
        for i, name in enumerate(names):
            Operator.write_results(os.path.join(args.out, name + ".txt"), rows[off[i]:off[i + 1]])
        frames_done += len(names)
        boxes_done += rows.shape[0]
    dt = time.perf_counter() - t0
    print("%d frames, %d boxes -> %s in %.2f s (%.2f frames/s, %s, %d scales, batch %d%s)"
          % (frames_done, boxes_done, args.out, dt, frames_done / dt, "nms" if nms else "raw", len(scales), args.batch,
             ", random weights" if args.random_weights else ""))


if __name__ == "__main__":
    main()
