"""Feeding rate of the real-data loaders and the time of rr_augment_frames.

Generates a seeded temporary dataset of 1360x765 JPEGs with PIL (VisDrone's common frame size; boxes and ignore
regions from a seeded generator) and reports, per crop size (512x512 and 1024x1024) at B=8 and 16 threads:
  * images/s of the host-path loader (every pixel step on CPU threads, float frames over PCIe),
  * images/s of the device loader (decode + decisions on the threads, rr_augment_frames on the GPU),
  * rr_augment_frames time by HIP events on one resident batch (median of --reps launches after a warm-up).
Loader rates are medians over --runs timed windows of --batches batches each, after a warm-up window; each window ends
in a device synchronise.  One JSON line on stdout; --out writes the same object to a file.

--fill-duck measures the full chain instead: every image gets a generated road map (a road band across the lower
half), the chain holds FillDuck, and the kernel entry is rr_augment_frames_pasted with the time of each of its three
stages (canvas, paste, finish) and of the whole call.

--color-jitter measures the chain with ColorJitter(0.5, 0.5, 0.5) in front on the same generated data set: both loaders,
rr_jitter_gray_mean, rr_augment_frames_jitter beside the unjittered kernel (on the windows the plain loader ships and on
the whole frames the jittered one ships) and the bytes each ships per batch; written to profiles/loader_jitter.json
unless --out names another file.

  python tools/bench_loader.py [--images 48] [--batches 12] [--runs 3] [--threads 16] [--out profiles/loader.json]
  python tools/bench_loader.py --fill-duck --crops 1024 --out profiles/loader_fillduck.json
  python tools/bench_loader.py --color-jitter"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def write_dataset(root, n, size=(1360, 765), seed=219):
    from PIL import Image
    w, h = size
    os.makedirs(os.path.join(root, "train", "images"))
    os.makedirs(os.path.join(root, "train", "annotations"))
    for i in range(n):
        rng = np.random.default_rng([seed, i])
        # smooth structure plus noise: a JPEG of pure noise decodes slower than a photograph, a flat one faster
        coarse = Image.fromarray(rng.integers(0, 256, (h // 16 + 1, w // 16 + 1, 3), dtype=np.uint8)).resize((w, h), Image.BICUBIC)
        img = np.clip(np.asarray(coarse, np.int16) + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, "train", "images", "%06d.jpg" % i), quality=90)
        rows = []
        for _ in range(60):
            bw, bh = int(np.exp(rng.uniform(np.log(8), np.log(160)))), int(np.exp(rng.uniform(np.log(8), np.log(160))))
            rows.append((int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh)), bw, bh, 1, int(rng.integers(1, 11)), 0, 0))
        for _ in range(3):
            rows.append((int(rng.integers(0, w - 200)), int(rng.integers(0, h - 120)), 200, 120, 0, 0, 0, 0))
        with open(os.path.join(root, "train", "annotations", "%06d.txt" % i), "w") as f:
            f.write("".join(",".join(str(v) for v in r) + "\n" for r in rows))


def write_roadmaps(root, n, size=(1360, 765)):
    """A road band across the lower half of every frame."""
    from PIL import Image
    w, h = size
    os.makedirs(os.path.join(root, "train", "roadmap"))
    road = np.zeros((h, w, 3), np.uint8)
    road[h // 2:] = 255
    for i in range(n):
        Image.fromarray(road).save(os.path.join(root, "train", "roadmap", "%06d.jpg" % i), quality=90)


def chain(crop, fill_duck=False, color_jitter=False):
    from rrnet_amd.datasets.transforms import (ColorJitter, Compose, FillDuck, HorizontalFlip, MaskIgnore, MultiScale,
                                               Normalize, RandomCrop, ToHeatmap, ToTensor)
    ts = [MultiScale(scale=(1, 1.15, 1.25, 1.35, 1.5)), ToTensor(), MaskIgnore(MEAN), HorizontalFlip(),
          RandomCrop((crop, crop)), Normalize(MEAN, STD), ToHeatmap(scale_factor=4)]
    if fill_duck:
        ts.insert(3, FillDuck())
    if color_jitter:
        ts.insert(0, ColorJitter(0.5, 0.5, 0.5))
    return Compose(ts)


def loader_rate(loader, batch, batches, runs):
    import torch
    for _ in range(max(batches // 2, 2)):
        loader.get_batch()
    torch.cuda.synchronize()
    rates = []
    for _ in range(runs):
        t0 = time.perf_counter()
        for _ in range(batches):
            loader.get_batch()
        torch.cuda.synchronize()
        rates.append(batch * batches / (time.perf_counter() - t0))
    return rates


def kernel_time(ds, params, batch, crop, reps):
    """One batch of real windows resident on the device; rr_augment_frames alone between HIP events."""
    import torch
    from rrnet_amd import ops
    from rrnet_amd.datasets import augment as A
    taps = A.TapCache()
    sampler = A.AugmentSampler(params, seed=219)
    items = []
    for i in range(batch):
        image, annos, _ = ds.load(i % len(ds))
        d = sampler.sample(annos, image.size[1], image.size[0], 0, i)
        win = A.source_window(d, image.size[1], image.size[0], crop, crop, taps)
        y0, x0, wh, ww = win[:4]
        items.append((d, image.size[1], image.size[0], win, np.asarray(image.crop((x0, y0, x0 + ww, y0 + wh)), dtype=np.uint8)))
    src, prm, rects, rect_off = A.pack_batch(items)
    dev = torch.device("cuda", 0)
    args = (torch.from_numpy(src.copy()).to(dev), torch.from_numpy(prm).to(dev),
            torch.from_numpy(rects).to(dev) if len(rects) else None, torch.from_numpy(rect_off).to(dev), taps.device(dev),
            torch.tensor(MEAN, device=dev), torch.tensor(STD, device=dev), crop, crop)
    for _ in range(10):
        ops.augment_frames(*args)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.augment_frames(*args)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    out_bytes = batch * crop * crop * 3 * 4
    med = statistics.median(ms)
    return {"ms_median": med, "ms_min": min(ms), "ms_max": max(ms), "bytes_written": out_bytes,
            "bytes_read_windows": int(src.size), "write_GBps": out_bytes / med / 1e6}


def _timed(fn, reps):
    import torch
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def jitter_kernel_time(ds, params, batch, crop, reps):
    """One batch of whole frames and their factors resident on the device: rr_jitter_gray_mean, rr_augment_frames_jitter
    and, on the same whole-frame records, the unjittered kernel (what the arithmetic per tap costs apart from what
    reading whole frames costs; kernel_time has the unjittered kernel on windows)."""
    import torch
    from rrnet_amd import ops
    from rrnet_amd.datasets import augment as A
    taps = A.TapCache()
    sampler = A.AugmentSampler(params, seed=219)
    items = []
    for i in range(batch):
        image, annos, _ = ds.load(i % len(ds))
        h, w = image.size[1], image.size[0]
        d = sampler.sample(annos, h, w, 0, i)
        win = (0, 0, h, w) + A.source_window(d, h, w, crop, crop, taps)[4:]
        items.append((d, h, w, win, np.asarray(image, dtype=np.uint8)))
    src, prm, rects, rect_off = A.pack_batch(items)
    factors, max_pixels = A.pack_jitter(items)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    args = (t(src.copy()), t(prm), t(rects) if len(rects) else None, t(rect_off), taps.device(dev))
    mean, std, fac = torch.tensor(MEAN, device=dev), torch.tensor(STD, device=dev), t(factors)
    work = ops.jitter_workspace(batch, dev)
    gray, _ = ops.jitter_gray_mean(args[0], args[1], fac, max_pixels, work=work)
    runs = {"rr_jitter_gray_mean": lambda: ops.jitter_gray_mean(args[0], args[1], fac, max_pixels, work=work),
            "rr_augment_frames_jitter": lambda: ops.augment_frames_jitter(*args, fac, gray, mean, std, crop, crop),
            "rr_augment_frames_whole_frames": lambda: ops.augment_frames(*args, mean, std, crop, crop)}
    out = {"factors": factors.tolist(), "gray_mean": gray.cpu().tolist(), "bytes_read_frames": int(src.size),
           "bytes_written": batch * crop * crop * 3 * 4}
    for name, fn in runs.items():
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        out[name] = _timed(fn, reps)
    return out


def pasted_kernel_time(ds, params, batch, crop, reps):
    """One batch of whole frames and their paste plans resident on the device; rr_augment_frames_pasted stage by stage
    (the canvas stage restores what the paste stage changes, so each timed paste starts from the same canvas)."""
    import torch
    from rrnet_amd import ops
    from rrnet_amd.datasets import augment as A
    taps = A.TapCache()
    sampler = A.AugmentSampler(params, seed=219)
    items, ds_ = [], []
    for i in range(batch):
        image, annos, _, road = ds.load(i % len(ds))
        d = sampler.sample(annos, image.size[1], image.size[0], 0, i, road)
        win = A.source_window(d, image.size[1], image.size[0], crop, crop, taps)
        if A.n_pastes(d):
            win = (0, 0, image.size[1], image.size[0]) + win[4:]
        y0, x0, wh, ww = win[:4]
        items.append((d, image.size[1], image.size[0], win, np.asarray(image.crop((x0, y0, x0 + ww, y0 + wh)), dtype=np.uint8)))
        ds_.append(d)
    src, prm, rects, rect_off = A.pack_batch(items)
    pastes, paste_off, canvas_pix, scratch_pix = A.pack_pastes(ds_)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    work = ops.paste_workspace(batch, canvas_pix, scratch_pix, dev)
    args = (t(src.copy()), t(prm), t(rects) if len(rects) else None, t(rect_off), taps.device(dev),
            t(pastes) if len(pastes) else None, t(paste_off), torch.tensor(MEAN, device=dev),
            torch.tensor(STD, device=dev), crop, crop)
    run = lambda stages: ops.augment_frames_pasted(*args, stages=stages, work=work)
    for _ in range(5):
        run(7)
    torch.cuda.synchronize()
    out = {"pastes": int(len(pastes)), "pastes_per_frame": np.diff(paste_off).tolist(),
           "depth": [d.plan.depth if d.plan is not None else 0 for d in ds_],
           "canvas_pixels_per_frame": int(canvas_pix), "largest_object_pixels": int(scratch_pix),
           "bytes_read_frames": int(src.size), "all": _timed(lambda: run(7), reps), "canvas": _timed(lambda: run(1), reps)}
    ms = []
    for _ in range(reps):
        run(1)
        ms.append(_timed(lambda: run(2), 1)["ms_median"])
    out["paste"] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}
    out["finish"] = _timed(lambda: run(4), reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--batches", type=int, default=12)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--crops", type=int, nargs="+", default=[512, 1024])
    ap.add_argument("--out", default=None)
    ap.add_argument("--fill-duck", action="store_true", help="the full chain with FillDuck on generated road maps")
    ap.add_argument("--color-jitter", action="store_true", help="the chain with ColorJitter(0.5, 0.5, 0.5) in front")
    a = ap.parse_args()
    if a.color_jitter and a.fill_duck:
        raise SystemExit("--color-jitter and --fill-duck are measured one at a time")
    if a.color_jitter and a.out is None:
        a.out = os.path.join(ROOT, "profiles", "loader_jitter.json")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_loader.py measures on the GPU; none is visible")
    from rrnet_amd.datasets import augment as A
    from rrnet_amd.datasets.drones_det import DronesDET
    res = {"tool": "bench_loader", "frame": [1360, 765], "images": a.images, "batch": a.batch, "threads": a.threads,
           "batches_per_window": a.batches, "windows": a.runs, "fill_duck": a.fill_duck, "crops": {}}
    if a.color_jitter:
        res["color_jitter"] = [0.5, 0.5, 0.5]
    with tempfile.TemporaryDirectory() as root:
        t0 = time.perf_counter()
        write_dataset(root, a.images)
        if a.fill_duck:
            write_roadmaps(root, a.images)
        res["dataset_write_s"] = time.perf_counter() - t0
        for crop in a.crops:
            tr = chain(crop, a.fill_duck, a.color_jitter)
            ds = DronesDET(root, tr, "train", with_road_map=a.fill_duck)
            p = A.chain_params(tr)
            entry = {}
            for name, cls in (("host_loader", A.HostAugmentLoader), ("device_loader", A.DeviceAugmentLoader)):
                loader = cls(ds, p, a.batch, seed=219, num_workers=a.threads)
                try:
                    rates = loader_rate(loader, a.batch, a.batches, a.runs)
                finally:
                    loader.close()
                entry[name] = {"images_per_s_median": statistics.median(rates), "images_per_s": rates,
                               "redraws": loader.redraws}
            if a.fill_duck:
                entry["rr_augment_frames_pasted"] = pasted_kernel_time(ds, p, a.batch, crop, a.reps)
            elif a.color_jitter:
                entry["rr_augment_frames"] = kernel_time(ds, dict(p, jitter=None), a.batch, crop, a.reps)
                entry["jitter"] = jitter_kernel_time(ds, p, a.batch, crop, a.reps)
                entry["h2d_bytes_per_batch"] = {"windows": entry["rr_augment_frames"]["bytes_read_windows"],
                                                "whole_frames": entry["jitter"]["bytes_read_frames"]}
            else:
                entry["rr_augment_frames"] = kernel_time(ds, p, a.batch, crop, a.reps)
            res["crops"]["%dx%d" % (crop, crop)] = entry
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
