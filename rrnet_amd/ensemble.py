"""Fuse the detections of several runs (models, scales, flips, tiles) with weighted boxes fusion (Solovyev, Wang, Gabruseva
2021) on the device: rr_wbf_segments over (frame, class) segments.  The reference has no fusion; this is the project's own
feature.  `fuse_rows` works on arrays, `fuse_result_dirs` on folders of VisDrone result files."""
import os
import time

import numpy as np
import torch

CONF_TYPES = ("avg", "max")
RESULT_FORMAT = "%f,%f,%f,%f,%.4f,%d,-1,-1"          # RRNetOperator.write_results


def _check_weights(weights, nruns):
    if weights is None:
        weights = [1.0] * nruns
    weights = [float(w) for w in weights]
    if len(weights) != nruns:
        raise ValueError("fuse_rows: %d weights for %d runs" % (len(weights), nruns))
    if not all(np.isfinite(w) and w > 0.0 for w in weights):
        raise ValueError("fuse_rows: weights must be positive and finite, got %s" % (weights,))
    return weights


def _stage(sets, weights, max_classes, frame_names):
    """Validates and lays the runs out for ONE upload: host [F,K,7] = x,y,w,h,score,cls,run weight (padding: cls -1), and
    the longest (frame, class) run of rows that could reach the kernel."""
    nruns = len(sets)
    nf = len(sets[0])
    for m, s in enumerate(sets):
        if len(s) != nf:
            raise ValueError("fuse_rows: run %d has %d frames, run 0 has %d" % (m, len(s), nf))
    frames, longest, longest_frame = [], 0, None
    for f in range(nf):
        name = frame_names[f] if frame_names is not None else f
        parts = []
        for m in range(nruns):
            a = np.asarray(sets[m][f])
            if a.size == 0:
                continue
            if a.ndim != 2 or a.shape[1] < 6:
                raise ValueError("fuse_rows: frame %s of run %d is %s, expected [n, >=6]" % (name, m, a.shape))
            a = a[:, :6].astype(np.float32)
            if not np.isfinite(a).all():
                raise ValueError("fuse_rows: frame %s of run %d holds non-finite values" % (name, m))
            cls = a[:, 5].astype(np.int64)
            if cls.min() < 0 or cls.max() >= max_classes:
                raise ValueError("fuse_rows: frame %s of run %d holds a class id outside [0, %d)" % (name, m, max_classes))
            parts.append(np.concatenate([a, np.full((a.shape[0], 1), np.float32(weights[m]), np.float32)], 1))
        a = np.concatenate(parts, 0) if parts else np.zeros((0, 7), np.float32)
        if a.shape[0]:
            n = int(np.bincount(a[:, 5].astype(np.int64)).max())
            if n > longest:
                longest, longest_frame = n, name
        frames.append(a)
    kmax = max([a.shape[0] for a in frames] + [0])
    host = np.zeros((nf, max(kmax, 1), 7), np.float32)
    host[:, :, 5] = -1.0
    for f, a in enumerate(frames):
        host[f, :a.shape[0]] = a
    return host, kmax, longest, longest_frame


def fuse_rows(sets, weights=None, iou_thr=0.55, skip_score=0.0, conf_type="avg", max_det=500, max_classes=32, device=None,
              want_members=False, frame_names=None, timing=None):
    """sets[m][f]: [n,>=6] x,y,w,h,score,cls of run m, frame f -> list of float32 [k,6] fused rows per frame (and, with
    want_members, a list of int32 [k] member counts).  Per frame: concatenate the runs, score * float32(weight), drop
    score <= skip_score, xywh -> xyxy, stable sort by score, group by class, fuse every class (rr_wbf_segments, weight_sum =
    sum of the weights), xyxy -> xywh, stable sort by confidence, keep max_det.  One upload, one launch sequence and one
    download for all frames; everything is checked before the first launch (ValueError names the frame)."""
    from rrnet_amd import ops
    if conf_type not in CONF_TYPES:
        raise ValueError("fuse_rows: conf_type %r, expected one of %s" % (conf_type, CONF_TYPES))
    if not (np.isfinite(skip_score) and skip_score >= 0.0):
        raise ValueError("fuse_rows: skip_score %r must be >= 0" % (skip_score,))
    if not np.isfinite(iou_thr):
        raise ValueError("fuse_rows: iou_thr %r" % (iou_thr,))
    if len(sets) == 0:
        raise ValueError("fuse_rows: no runs")
    weights = _check_weights(weights, len(sets))
    host, kmax, longest, longest_frame = _stage(sets, weights, max_classes, frame_names)
    nf = host.shape[0]
    empty = [np.zeros((0, 6), np.float32) for _ in range(nf)]
    if kmax == 0:
        return (empty, [np.zeros(0, np.int32) for _ in range(nf)]) if want_members else empty
    limit = ops.wbf_plan(1, 1)[5]                      # the longest segment rr_wbf_segments takes (csrc/wbf_plan.h)
    if longest > limit:
        raise ValueError("fuse_rows: frame %s holds %d rows of one class, the kernel takes segments of up to %d"
                         % (longest_frame, longest, limit))
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    t0 = time.perf_counter()
    with torch.cuda.device(dev):
        a = torch.from_numpy(host).to(dev)                                       # the one upload
        if timing is not None:
            torch.cuda.synchronize()
            timing["upload"] = timing.get("upload", 0.0) + time.perf_counter() - t0
            t0 = time.perf_counter()
        b = a[:, :, :6].contiguous()
        b[:, :, 4] = a[:, :, 4] * a[:, :, 6]
        b[:, :, 5] = torch.where(b[:, :, 4] > float(np.float32(skip_score)), b[:, :, 5], torch.full_like(b[:, :, 5], -1.0))
        b[:, :, 2:4] += b[:, :, 0:2]
        live = b[:, :, 5] >= 0
        key = torch.where(live, b[:, :, 4], torch.full_like(b[:, :, 4], float("-inf")))
        order = torch.sort(key, dim=1, descending=True, stable=True)[1]
        b = torch.gather(b, 1, order.unsqueeze(2).expand(-1, -1, 6)).contiguous()
        grouped, seg_off, seg_len = ops.group_by_class(b, max_classes)
        rows = grouped.view(-1, 6)
        out, members, n_out = ops.wbf_segments(rows, seg_off, longest, iou_thr, conf_type, float(sum(weights)), seg_len=seg_len)
        _, _, _, kept, out_off = ops.pack_segments(out, seg_off, n_out, max_classes, want_rois=False, want_rows=True,
                                                   want_offsets=True)
        kept[:, 2:4] -= kept[:, 0:2]
        fo = out_off[::max_classes].contiguous()                                  # [F+1] row offsets of the frames
        r = kept.shape[0]
        frame = torch.searchsorted(fo[1:].contiguous(), torch.arange(r, device=dev, dtype=torch.int32), right=True)
        o1 = torch.sort(kept[:, 4], descending=True, stable=True)[1]
        o2 = torch.sort(frame[o1], stable=True)[1]
        order = o1[o2]
        kept = kept[order]
        if want_members:
            # members ride in the layout of `out`: pack them the same way
            mrows = torch.zeros_like(out)
            mrows[:, 4] = members.float()
            mem = ops.pack_segments(mrows, seg_off, n_out, max_classes, want_rois=False, want_rows=True)[3][:, 4][order]
        if timing is not None:
            torch.cuda.synchronize()
            timing["kernels"] = timing.get("kernels", 0.0) + time.perf_counter() - t0
            t0 = time.perf_counter()
        kept_h = kept.cpu().numpy()
        fo_h = fo.cpu().numpy()
        mem_h = mem.cpu().numpy().astype(np.int32) if want_members else None
        if timing is not None:
            timing["download"] = timing.get("download", 0.0) + time.perf_counter() - t0
    res = [kept_h[fo_h[f]:fo_h[f + 1]][:max_det] for f in range(nf)]
    if want_members:
        return res, [mem_h[fo_h[f]:fo_h[f + 1]][:max_det] for f in range(nf)]
    return res


def _read_or_empty(path):
    from rrnet_amd.utils.metrics.metrics import _read
    if not os.path.exists(path):
        return None
    if os.path.getsize(path) == 0:
        return np.zeros((0, 8), np.float64)
    return _read(path)


def result_names(dirs):
    """Sorted union of the result files' names (without .txt) over the runs."""
    names = set()
    for d in dirs:
        names.update(os.path.splitext(x)[0] for x in os.listdir(d) if x.endswith(".txt"))
    return sorted(names)


def _text_route(text, device):
    if text not in ("host", "device"):
        raise ValueError("text=%r, expected 'host' or 'device'" % (text,))
    if text == "device":
        return torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return None


def read_result_dirs(dirs, text="host", device=None):
    """-> (names, sets, missing): sets[m][f] the rows of run m for names[f]; a file a run lacks counts as no detections of
    that run, and `missing` counts such files.  text="device" parses all files of all runs in one pass of
    rrnet_amd.textio.read_files (files the codec flags, and missing or empty ones, still go through _read_or_empty)."""
    names = result_names(dirs)
    sets, missing = [], 0
    dev = _text_route(text, device)
    if dev is not None:
        from rrnet_amd import textio
        paths = [os.path.join(d, name + ".txt") for d in dirs for name in names]
        arrays, _ = textio.read_files(paths, dev, host_read=_read_or_empty)
        for m in range(len(dirs)):
            run = arrays[m * len(names):(m + 1) * len(names)]
            missing += sum(a is None for a in run)
            sets.append([np.zeros((0, 8), np.float64) if a is None else a for a in run])
        return names, sets, missing
    for d in dirs:
        run = []
        for name in names:
            a = _read_or_empty(os.path.join(d, name + ".txt"))
            if a is None:
                missing += 1
                a = np.zeros((0, 8), np.float64)
            run.append(a)
        sets.append(run)
    return names, sets, missing


def format_rows(rows):
    """The text of one result file."""
    return "".join((RESULT_FORMAT % (r[0], r[1], r[2], r[3], r[4], int(r[5]))) + "\n" for r in rows)


def write_result_dir(out_dir, names, frames, text="host", device=None):
    """One result file per frame.  text="device": the float32 rows are uploaded once, formatted by rr_text_format and written
    in binary mode; the files are the same bytes."""
    os.makedirs(out_dir, exist_ok=True)
    dev = _text_route(text, device)
    if dev is not None:
        from rrnet_amd import textio
        frames = [np.asarray(rows) for rows in frames[:len(names)]]
        if any(rows.dtype != np.float32 for rows in frames):
            raise ValueError("write_result_dir: text='device' formats float32 rows")
        frames = [rows.reshape(-1, 6) for rows in frames]
        host = np.concatenate(frames, 0) if frames else np.zeros((0, 6), np.float32)
        frame_off = np.cumsum([0] + [rows.shape[0] for rows in frames])
        textio.write_frames([os.path.join(out_dir, name + ".txt") for name in names[:len(frames)]],
                            torch.from_numpy(np.ascontiguousarray(host)).to(dev), frame_off, "rrnet", False)
        return
    for name, rows in zip(names, frames):
        with open(os.path.join(out_dir, name + ".txt"), "w") as f:
            f.write(format_rows(rows))


def fuse_result_dirs(dirs, out_dir, timing=None, text="host", **kw):
    """Fuses the result folders `dirs` (one per run) into `out_dir`.  Returns the number of files that some run lacked.
    text="device" reads and writes the files through the device-side text codec (rrnet_amd/textio.py)."""
    t0 = time.perf_counter()
    names, sets, missing = read_result_dirs(dirs, text=text, device=kw.get("device"))
    if timing is not None:
        timing["read"] = timing.get("read", 0.0) + time.perf_counter() - t0
    print("%d files of %d runs, %d missing (counted as no detections)" % (len(names), len(dirs), missing))
    frames = fuse_rows(sets, frame_names=names, timing=timing, **kw) if names else []
    t0 = time.perf_counter()
    write_result_dir(out_dir, names, frames, text=text, device=kw.get("device"))
    if timing is not None:
        timing["write"] = timing.get("write", 0.0) + time.perf_counter() - t0
    return missing
