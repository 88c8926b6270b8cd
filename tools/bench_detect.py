"""Frames per second of multi-scale detection from raw frames to result files: the per-frame path (DeviceValLoader ->
RRNetOperator.evaluate_images -> save_result) against detect_frames at several batch sizes, same process, same frames.

Workload: RRNet with the hourglass-104 backbone and RANDOM weights, generated 1360x765 frames (VisDrone's common size),
cfg.Val.scales, the config's auto_test (True: every box of every scale is kept and written).  Random weights keep all 1500
boxes per scale whatever the filter: the worst case for the cross-scale tail and the writer; a trained model with --nms
keeps far fewer.

Every configuration runs 1 + --windows windows of --window-frames frames over a pool of --frames frames; the first window
warms up (all scales' shapes), frames/s is the median of the others.  A window is timed with the host clock from the first
decode to the last result file and ends in a device synchronise.  Device time per stage (prepare / model / post-process)
comes from HIP events recorded between the stages of detect_frames; writer time is host time inside write_results /
save_result.  One JSON line on stdout; --out writes the object to a file.

--centernet measures the other detector the same way: hourglass-104 CenterNet (centernet_config: six scales, each run
flipped and plain, auto_test=True), the per-frame path DeviceValLoader -> CenterNetOperator.evaluate_images -> save_result
against detect_frames_centernet; fp32 only (CenterNet has no bf16 scope).  Random weights keep all 250 boxes of each of the
twelve passes: 3000 rows per frame.

--retinanet measures RetinaNet (retinanet_config: resnet50, one scale, hard NMS at 0.3; fp32 only): the per-frame path
DeviceValLoader -> RetinaNetOperator.evaluate_images -> save_result against detect_frames_retinanet.  With random weights
every anchor scores near 0.5 and passes the reference's 0.1, more candidates than the score sort holds: the tool picks, from
one model pass on the first frames, the score threshold that leaves at most --rows candidates in any of them, uses it on
both paths (the per-frame path reads the operator module's SCORE_THRESH) and records it with the counts.

  python tools/bench_detect.py [--frames 32] [--window-frames 8] [--windows 3] [--batches 1,2,4] [--modes f32,bf16]
                               [--nms] [--centernet | --retinanet [--rows 1000]] [--out profiles/detect.json]"""
import argparse
import copy
import json
import os
import statistics
import sys
import tempfile
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME_H, FRAME_W = 765, 1360


class GeneratedFrames:
    """DronesDET's load surface over seeded uint8 frames held as PIL images (decode cost: the uint8 copy only)."""

    def __init__(self, n, seed=219, sizes=None):
        """sizes (optional): (H, W) choices; every frame draws one (seeded), a folder of mixed sizes."""
        from PIL import Image
        rng = np.random.default_rng(seed)
        self.images = []
        self.sizes = [(FRAME_H, FRAME_W)] * n if sizes is None else \
            [sizes[i] for i in np.random.default_rng(seed + 1).integers(0, len(sizes), n)]
        for h, w in self.sizes:
            coarse = rng.integers(0, 256, (h // 16 + 1, w // 16 + 1, 3), dtype=np.uint8)
            img = np.kron(coarse, np.ones((16, 16, 1), np.uint8))[:h, :w]                  # blocks, not white noise
            img = (img.astype(np.int16) + rng.integers(-8, 9, img.shape, dtype=np.int16)).clip(0, 255).astype(np.uint8)
            self.images.append(Image.fromarray(img))
        self.mdf = ["frame%04d" % i for i in range(n)]
        self.annos = np.asarray([[10, 10, 50, 50, 1, 1, 0, 0]], np.int64)

    def __len__(self):
        return len(self.images)

    def load(self, i):
        return self.images[i].copy(), self.annos.copy(), self.mdf[i]


class Window:
    """A view of `count` frames of the pool starting at `start` (wrapping)."""

    def __init__(self, pool, start, count):
        self.pool, self.idx = pool, [(start + i) % len(pool) for i in range(count)]
        self.mdf = [pool.mdf[i] for i in self.idx]

    def __len__(self):
        return len(self.idx)

    def load(self, i):
        return self.pool.load(self.idx[i])


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--window-frames", type=int, default=8)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--batches", default="1,2,4")
    ap.add_argument("--modes", default="f32,bf16")
    ap.add_argument("--nms", action="store_true", help="auto_test=False: score filter and Soft-NMS (default: the config's raw mode)")
    ap.add_argument("--centernet", action="store_true", help="CenterNet (centernet_config) instead of RRNet; fp32 only")
    ap.add_argument("--retinanet", action="store_true", help="RetinaNet (retinanet_config) instead of RRNet; fp32 only")
    ap.add_argument("--rows", type=int, default=1000, help="--retinanet: candidates per frame the picked threshold leaves")
    ap.add_argument("--backbone", default=None, help="override cfg.Model.backbone (rehearsals; --retinanet: resnet10 / resnet50 / resnet101, "
                    "shufflenet_v2_x0_5 / _x1_5 / _x2_0)")
    ap.add_argument("--tile", type=int, help="--retinanet: measure tiled inference on NxN tiles over a pool of mixed frame sizes")
    ap.add_argument("--tile-overlap", type=int, default=128)
    ap.add_argument("--tile-zoom", type=float, default=1.0)
    ap.add_argument("--tile-margin", type=float, default=0.0)
    ap.add_argument("--tile-batches", default="4,8,16", help="--tile: tiles per model pass")
    ap.add_argument("--tile-frames", type=int, default=4, help="--tile: frames per detect_tiled call")
    ap.add_argument("--out")
    args = ap.parse_args(argv)
    assert args.windows >= 3, "frames/s is the median of at least 3 windows"
    if args.tile is not None:
        assert args.retinanet, "--tile measures RetinaNet: give --retinanet"
        return main_tiled(args)

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_detect.py measures on the GPU; there is nothing to measure without one")
    from rrnet_amd.datasets.augment import DeviceValLoader, chain_params
    from rrnet_amd.datasets.frames import SizeBucketedFrames
    assert not (args.centernet and args.retinanet), "--centernet or --retinanet, not both"
    if args.retinanet:
        from rrnet_amd.configs.retinanet_config import Config
        from rrnet_amd.inference import RetinaNetFrameDetector as Detector
        from rrnet_amd.operators import retinanet_operator as retina_mod
        Operator = retina_mod.RetinaNetOperator
        args.modes = "f32"
    elif args.centernet:
        from rrnet_amd.configs.centernet_config import Config
        from rrnet_amd.inference import CenterNetFrameDetector as Detector
        from rrnet_amd.operators.centernet_operator import CenterNetOperator as Operator
        args.modes = "f32"
    else:
        from rrnet_amd.configs.rrnet_config import Config
        from rrnet_amd.inference import Detector
        from rrnet_amd.operators.rrnet_operator import RRNetOperator as Operator

    pool = GeneratedFrames(args.frames)
    out_dir = tempfile.mkdtemp(prefix="bench_detect_")
    dev_dir = tempfile.mkdtemp(prefix="bench_detect_devtext_")           # the same files, written through rrnet_amd.textio
    from rrnet_amd import textio
    result = {"metric": "frames/sec, raw frame -> result file (%s detection)"
                        % ("single-scale RetinaNet" if args.retinanet else "multi-scale CenterNet flip" if args.centernet
                           else "multi-scale RRNet"), "unit": "frames/sec",
              "higher_is_better": True, "data": "generated %dx%d frames, pool of %d" % (FRAME_W, FRAME_H, args.frames),
              "weights": "random: the score threshold is picked so that at most %d candidates of a frame survive" % args.rows
                         if args.retinanet else
                         "random: all %s boxes of every %s survive, the worst case for the tail and the writer"
                         % (("250", "pass (two per scale)") if args.centernet else ("1500", "scale")),
              "windows": args.windows, "window_frames": args.window_frames, "modes": {}}

    for mode in args.modes.split(","):
        cfg = copy.deepcopy(Config)
        if args.backbone:
            cfg.Model.backbone = args.backbone
        if mode == "bf16":
            cfg.Model.bf16 = True
        if args.retinanet:
            cfg.Train.pretrained = False
        elif args.nms:
            cfg.Val.auto_test = False
        nms = True if args.retinanet else not cfg.Val.auto_test
        torch.manual_seed(219)
        det = Detector(cfg)
        params = chain_params(cfg.Val.transforms)
        ns = types.SimpleNamespace(cfg=cfg, model=det.model)
        if args.retinanet:
            from rrnet_amd.modules.anchor import Anchors
            ns.anchor_maker, ns._anchor_sets, ns._nms_rows = Anchors(sizes=(16, 64, 128)), {}, Operator._nms_rows
            ns.make_anchor = types.MethodType(Operator.make_anchor, ns)
            first = next(iter(SizeBucketedFrames(Window(pool, 0, max(int(v) for v in args.batches.split(","))), 64,
                                                 num_workers=8)))[0]
            score_thr, at_thr = det.threshold_for_rows(first, args.rows)
            retina_mod.SCORE_THRESH = score_thr                          # what evaluate_images decodes with
            del first
        elif args.centernet:
            ns.transform_bbox = types.MethodType(Operator.transform_bbox, ns)
            ns._ext_nms = Operator._ext_nms
        else:
            ns.generate_bbox = types.MethodType(Operator.generate_bbox, ns)
            ns._ext_nms, ns._ext_nms_device = Operator._ext_nms, Operator._ext_nms_device
        entry = {"scales": [1] if args.retinanet else list(cfg.Val.scales), "nms": nms, "backbone": cfg.Model.backbone}
        if args.retinanet:
            entry.update(score_thr=score_thr, candidates_at_threshold=at_thr, rows_asked=args.rows)

        def per_frame_window(w):
            """The parent's path: one frame at a time, D2H per frame, save_result's per-row loop."""
            writer, boxes = 0.0, 0
            t0 = time.perf_counter()
            with torch.no_grad():
                for imgs, _, names in DeviceValLoader(Window(pool, w * args.window_frames, args.window_frames), params,
                                                      num_workers=8):
                    pred = Operator.evaluate_images(ns, imgs)
                    pred = pred[0] if args.retinanet else pred           # RetinaNet returns one tensor per image
                    t1 = time.perf_counter()
                    Operator.save_result(os.path.join(out_dir, names[0] + ".txt"), pred)
                    writer += time.perf_counter() - t1
                    boxes += pred.shape[0]
            torch.cuda.synchronize()
            return time.perf_counter() - t0, writer, boxes, None

        def batched_window(w, batch):
            writer, writer_dev, boxes = 0.0, 0.0, 0
            layout = "retinanet" if args.retinanet else "centernet" if args.centernet else "rrnet"
            marks = []

            def timer(stage):
                ev = torch.cuda.Event(enable_timing=True)
                ev.record()
                marks.append((stage, ev))

            t0 = time.perf_counter()
            for frames_u8, names in SizeBucketedFrames(Window(pool, w * args.window_frames, args.window_frames), batch,
                                                       num_workers=8):
                timer("start")
                if args.retinanet:
                    pred, frame_off = det.detect(frames_u8, score_thr=score_thr, timer=timer)
                else:
                    pred, frame_off = det.detect(frames_u8, nms=nms, timer=timer)
                rows, off = pred.cpu().numpy(), frame_off.cpu().tolist()
                t1 = time.perf_counter()
                if args.retinanet:
                    Operator.write_results(out_dir, names, rows, off)
                else:
                    for i, name in enumerate(names):
                        Operator.write_results(os.path.join(out_dir, name + ".txt"), rows[off[i]:off[i + 1]])
                writer += time.perf_counter() - t1
                t1 = time.perf_counter()                  # the same files once more through the device codec (textio)
                textio.write_frames([os.path.join(dev_dir, name + ".txt") for name in names], pred, off, layout, True)
                writer_dev += time.perf_counter() - t1
                boxes += rows.shape[0]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0 - writer_dev    # the frames/s are those of the host writer, as before
            stages = {"prepare": 0.0, "model": 0.0, "post": 0.0}
            for (_, a), (stage, b) in zip(marks, marks[1:]):
                if stage != "start":
                    stages[stage] += a.elapsed_time(b)
            return dt, writer, boxes, stages, writer_dev

        def run(name, fn):
            torch.cuda.reset_peak_memory_stats()
            rows = []
            for w in range(args.windows + 1):
                r = fn(w)
                dt, writer, boxes, stages = r[:4]
                print("  %s %s window %d: %.2f s" % (mode, name, w, dt), file=sys.stderr, flush=True)
                if w > 0:                                                   # window 0 warms up
                    rows.append((args.window_frames / dt, writer, boxes, stages, r[4] if len(r) > 4 else None))
            fps = [r[0] for r in rows]
            rec = {"frames_per_sec": round(statistics.median(fps), 3), "frames_per_sec_windows": [round(v, 3) for v in fps],
                   "writer_ms_per_frame": round(1e3 * statistics.median(r[1] for r in rows) / args.window_frames, 3),
                   "boxes_per_frame": rows[0][2] / args.window_frames,
                   "allocator_peak_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)}
            if rows[0][4] is not None:
                rec["writer_device_ms_per_frame"] = round(1e3 * statistics.median(r[4] for r in rows) / args.window_frames, 3)
            if rows[0][3] is not None:
                rec["device_ms_per_frame"] = {k: round(statistics.median(r[3][k] for r in rows) / args.window_frames, 3)
                                              for k in rows[0][3]}
            return rec

        entry["per_frame"] = run("per-frame", per_frame_window)
        for b in [int(v) for v in args.batches.split(",")]:
            try:
                entry["batch_%d" % b] = run("batch %d" % b, lambda w, b=b: batched_window(w, b))
            except torch.cuda.OutOfMemoryError as e:
                entry["batch_%d" % b] = {"error": "out of memory: %s" % str(e).split("\n")[0]}
                torch.cuda.empty_cache()
        result["modes"][mode] = entry
        del det, ns
        torch.cuda.empty_cache()

    best = max((v["frames_per_sec"], k) for k, v in result["modes"][args.modes.split(",")[0]].items()
               if isinstance(v, dict) and "frames_per_sec" in v)
    result["value"], result["value_of"] = best[0], "%s %s" % (args.modes.split(",")[0], best[1])
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


MIXED_SIZES = [(765, 1360), (1080, 1920), (1500, 2000)]         # VisDrone's common frame sizes


def main_tiled(args):
    """--retinanet --tile N: tiled inference (OrderedFrames -> detect_tiled_retinanet) at several tiles-per-pass against the
    only other way through a folder of mixed sizes (SizeBucketedFrames -> detect_frames_retinanet at batch 4, whose batches
    run short), on one generated pool; then the two new kernels alone, timed with HIP events per call: rr_prepare_tiles
    against rr_prepare_frames on the host-cropped stack of the same tiles (both write the same bytes), and rr_merge_tiles at
    --rows candidates per tile.  Random weights: each path picks the score threshold that keeps its candidate counts within
    what its score sort holds, and records it.  What tiling does to AP needs a trained checkpoint: not measured here."""
    import math
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_detect.py measures on the GPU; there is nothing to measure without one")
    from rrnet_amd import _C, inference, ops
    from rrnet_amd.configs.retinanet_config import Config
    from rrnet_amd.datasets.frames import OrderedFrames, SizeBucketedFrames
    from rrnet_amd.operators.retinanet_operator import RetinaNetOperator

    tile, overlap, zoom, margin = (args.tile, args.tile), args.tile_overlap, args.tile_zoom, args.tile_margin
    pool = GeneratedFrames(args.frames, sizes=MIXED_SIZES)
    out_dir = tempfile.mkdtemp(prefix="bench_detect_tiled_")
    cfg = copy.deepcopy(Config)
    if args.backbone:
        cfg.Model.backbone = args.backbone
    cfg.Train.pretrained = False
    torch.manual_seed(219)
    det = inference.RetinaNetFrameDetector(cfg)
    tiles_of = {s: len(inference.plan_tiles(s[0], s[1], tile, overlap)) for s in MIXED_SIZES}
    first = next(iter(OrderedFrames(Window(pool, 0, args.tile_frames), args.tile_frames, num_workers=8)))[0]
    rows_per_tile = min(args.rows, inference.TILE_MAX_ROWS // (2 * max(tiles_of.values())))
    thr_tiled, most_tile = det.threshold_for_tile_rows(first, tile, overlap, zoom, rows_per_tile)
    largest = max(range(len(pool)), key=lambda i: pool.sizes[i][0] * pool.sizes[i][1])
    big = torch.from_numpy(np.asarray(pool.load(largest)[0], dtype=np.uint8).copy()).cuda()[None]
    thr_frames, at_thr = det.threshold_for_rows(big, args.rows)
    del big
    result = {"metric": "frames/sec, raw frame -> result file (RetinaNet on %dx%d tiles, overlap %d, zoom %g, margin %g)"
                        % (tile + (overlap, zoom, margin)), "unit": "frames/sec", "higher_is_better": True,
              "data": "generated frames of %s drawn at random, pool of %d: %s"
                      % (", ".join("%dx%d" % (w, h) for h, w in MIXED_SIZES), args.frames,
                         {"%dx%d" % (w, h): pool.sizes.count((h, w)) for h, w in MIXED_SIZES}),
              "backbone": cfg.Model.backbone, "windows": args.windows, "window_frames": args.window_frames,
              "tiles_per_frame": {"%dx%d" % (w, h): n for (h, w), n in tiles_of.items()},
              "weights": "random; tiled: score > %.9g keeps at most %d candidates of a tile of the first frames (asked %d); "
                         "whole frames: score > %.9g keeps %s of the largest frame (asked %d)"
                         % (thr_tiled, most_tile, rows_per_tile, thr_frames, at_thr, args.rows),
              "ap": "not measured: needs a trained checkpoint and the dataset", "tiled": {}}

    def window(w, frames_iter, detect):
        writer, boxes, marks, lengths = 0.0, 0, [], []

        def timer(stage):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            marks.append((stage, ev))

        t0 = time.perf_counter()
        for frames, names in frames_iter(Window(pool, w * args.window_frames, args.window_frames)):
            timer("start")
            pred, frame_off = detect(frames, timer)
            rows, off = pred.cpu().numpy(), frame_off.cpu().tolist()
            t1 = time.perf_counter()
            RetinaNetOperator.write_results(out_dir, names, rows, off)
            writer += time.perf_counter() - t1
            boxes += rows.shape[0]
            lengths.append(len(names))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        stages = {"prepare": 0.0, "model": 0.0, "post": 0.0}
        for (_, a), (stage, b) in zip(marks, marks[1:]):
            if stage != "start":
                stages[stage] += a.elapsed_time(b)
        return dt, writer, boxes, stages, lengths

    def run(name, frames_iter, detect):
        torch.cuda.reset_peak_memory_stats()
        rows = []
        for w in range(args.windows + 1):
            r = window(w, frames_iter, detect)
            print("  %s window %d: %.2f s" % (name, w, r[0]), file=sys.stderr, flush=True)
            if w > 0:                                                       # window 0 warms up
                rows.append(r)
        fps = [args.window_frames / r[0] for r in rows]
        lengths = [n for r in rows for n in r[4]]
        return {"frames_per_sec": round(statistics.median(fps), 3), "frames_per_sec_windows": [round(v, 3) for v in fps],
                "writer_ms_per_frame": round(1e3 * statistics.median(r[1] for r in rows) / args.window_frames, 3),
                "boxes_per_frame": round(sum(r[2] for r in rows) / (len(rows) * args.window_frames), 1),
                "device_ms_per_frame": {k: round(statistics.median(r[3][k] for r in rows) / args.window_frames, 3)
                                        for k in rows[0][3]},
                "mean_frames_per_call": round(sum(lengths) / len(lengths), 3),
                "allocator_peak_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 3)}

    for tb in [int(v) for v in args.tile_batches.split(",")]:
        result["tiled"]["tile_batch_%d" % tb] = run(
            "tiled, %d tiles per pass" % tb, lambda win: OrderedFrames(win, args.tile_frames, num_workers=8),
            lambda frames, timer, tb=tb: det.detect_tiled(frames, tile, overlap, zoom=zoom, margin=margin, tile_batch=tb,
                                                          score_thr=thr_tiled, timer=timer))
    result["whole_frames_batch_4"] = run(
        "whole frames, batch 4", lambda win: SizeBucketedFrames(win, 4, num_workers=8),
        lambda frames, timer: det.detect(frames, score_thr=thr_frames, timer=timer))

    # ---- the kernels alone: one HIP-event pair per call, the two prepares alternating ----
    def timed(call, before=None):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if before is not None:
            before()
        a.record()
        call()
        b.record()
        return a, b

    reps = 50
    mean, std = inference._vec3(det.mean, det.device), inference._vec3(det.std, det.device)
    sizes, table = inference._tiles_of(first, tile, overlap)
    table_np, _ = ops.check_tiles(table, sizes, tile)
    oh, ow = int(math.floor(tile[0] * zoom)), int(math.floor(tile[1] * zoom))
    t = len(table)
    packed = torch.cat([f.contiguous().view(-1) for f in first])
    base = torch.from_numpy(np.concatenate([[0], np.cumsum([h * w * 3 for h, w in sizes])[:-1]]).astype(np.int64)).cuda()
    hw = torch.tensor(sizes, dtype=torch.int32).cuda()
    tiles_dev = torch.from_numpy(table_np).cuda()
    stack = torch.stack([first[f][y0:y0 + tile[0], x0:x0 + tile[1]] for f, y0, x0 in table]).contiguous()
    out_a, out_b = ops.empty_nhwc(t, 3, oh, ow, det.device), ops.empty_nhwc(t, 3, oh, ow, det.device)
    prep_tiles = lambda: _C.check(_C.fn("rr_prepare_tiles")(
        _C.ptr(packed), _C.ptr(base), _C.ptr(hw), len(sizes), _C.ptr(tiles_dev), t, tile[0], tile[1], oh, ow, _C.ptr(mean),
        _C.ptr(std), _C.ptr(out_a), _C.stream()), "rr_prepare_tiles")
    prep_stack = lambda: _C.check(_C.fn("rr_prepare_frames")(
        _C.ptr(stack), _C.ptr(mean), _C.ptr(std), _C.ptr(out_b), t, tile[0], tile[1], oh, ow, _C.stream()), "rr_prepare_frames")
    for _ in range(3):
        prep_tiles(), prep_stack()
    pairs = [(timed(prep_tiles), timed(prep_stack)) for _ in range(reps)]
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b)                                        # the same bytes
    ms_tiles = statistics.median(a.elapsed_time(b) for (a, b), _ in pairs)
    ms_stack = statistics.median(a.elapsed_time(b) for _, (a, b) in pairs)
    out_bytes = t * oh * ow * 12
    kernels = {"calls_each": reps, "tiles": t, "frames": len(sizes), "output_mib": round(out_bytes / 2 ** 20, 2),
               "rr_prepare_tiles_ms": round(ms_tiles, 4), "rr_prepare_frames_on_the_cropped_stack_ms": round(ms_stack, 4),
               "ratio": round(ms_tiles / ms_stack, 3),
               "rr_prepare_tiles_output_gb_per_s": round(out_bytes / ms_tiles / 1e6, 1)}

    m_sizes = [MIXED_SIZES[0]] * 8                                          # 8 tiles of 512 per frame at overlap 128
    m_table = []
    for f, (h, w) in enumerate(m_sizes):
        m_table += [(f, y0, x0) for y0, x0 in inference.plan_tiles(h, w, tile, overlap)]
    k_in = int(args.rows)
    g = torch.Generator(device="cuda").manual_seed(5)
    m_rows = torch.rand((len(m_table), k_in, 6), device="cuda", generator=g)
    m_rows[:, :, 0:2] *= float(min(oh, ow) - 40)
    m_rows[:, :, 2:4] = m_rows[:, :, 2:4] * 30 + 4
    m_count_in = torch.full((len(m_table),), k_in, dtype=torch.int32, device="cuda")
    per_frame_rows = k_in * len(m_table) // len(m_sizes)
    merged, count = ops.merge_buffers(len(m_sizes), min(per_frame_rows, ops.DETECT_MAX_ROWS), det.device)
    m_table_np, m_off = ops.check_tiles(m_table, m_sizes, tile)
    m_tiles_dev, m_off_dev = torch.from_numpy(m_table_np).cuda(), torch.from_numpy(m_off).cuda()
    m_hw = torch.tensor(m_sizes, dtype=torch.int32).cuda()
    m_margin = margin if margin > 0 else 4.0
    merge = lambda: _C.check(_C.fn("rr_merge_tiles")(
        _C.ptr(m_rows), _C.ptr(m_count_in), _C.ptr(m_tiles_dev), _C.ptr(m_off_dev), _C.ptr(m_hw), len(m_sizes), k_in, tile[0],
        tile[1], oh, ow, float(np.float32(zoom)), float(m_margin), _C.ptr(merged), _C.ptr(count), merged.shape[1],
        _C.stream()), "rr_merge_tiles")
    for _ in range(3):
        count.zero_()
        merge()
    m_pairs = [timed(merge, before=count.zero_) for _ in range(reps)]
    torch.cuda.synchronize()
    kernels["rr_merge_tiles"] = {"frames": len(m_sizes), "tiles": len(m_table), "candidates_per_tile": k_in, "margin": m_margin,
                                 "kept_per_frame": count.tolist(),
                                 "ms": round(statistics.median(a.elapsed_time(b) for a, b in m_pairs), 4)}
    result["kernels"] = kernels

    best = max((v["frames_per_sec"], k) for k, v in result["tiled"].items())
    result["value"], result["value_of"] = best[0], "tiled %s" % best[1]
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
