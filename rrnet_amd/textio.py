"""VisDrone result and annotation files through the device-side text codec (csrc/textio.hip): `read_files`
parses many files in one upload and two launches, `format_frames` turns device rows into the bytes the operators'
write_results write.  Both are exact; whatever the codec cannot decide (a flagged line or row) goes to the host functions,
which keep their behaviour, including what they raise."""
import os
import time

import numpy as np
import torch

LAYOUTS = {"rrnet": 0, "centernet": 1, "retinanet": 2}
CHUNK_BYTES = 1 << 30                    # text of one upload / one formatted buffer


def _tick(timing, key, t0, sync=False):
    if timing is not None:
        if sync:
            torch.cuda.synchronize()
        timing[key] = timing.get(key, 0.0) + time.perf_counter() - t0
    return time.perf_counter()


def _host_read(path):
    from rrnet_amd.utils.metrics.metrics import _read
    return _read(path)


def _chunks(sizes, limit):
    """Index ranges [a, b) whose sizes sum to at most `limit` (a single larger item stands alone)."""
    out, a, total = [], 0, 0
    for i, s in enumerate(sizes):
        if i > a and total + s > limit:
            out.append((a, i))
            a, total = i, 0
        total += s
    out.append((a, len(sizes)))
    return out


def read_files(paths, device, ncol=8, host_read=_host_read, timing=None, chunk_bytes=CHUNK_BYTES):
    """-> (list of float64 arrays [n_i, ncol], number of files that took the host route).  One host read per file into a
    pinned buffer, one upload, rr_text_line_counts / rr_text_lines / rr_text_parse, one download of rows and flags.  A file
    with a flagged line, with the surplus field on some lines only, without any line, or that is missing or empty is handed
    to `host_read(path)` and its answer returned as it is.  For every other file the array equals, bit for bit,
    host_read(path)[:, :ncol].astype(float64).  timing (a dict) collects file / upload / kernels / download / host seconds."""
    from rrnet_amd import ops
    device = torch.device(device)
    paths = list(paths)
    out, on_host = [None] * len(paths), []
    t0 = time.perf_counter()
    sizes = []
    for i, p in enumerate(paths):
        try:
            sizes.append(os.path.getsize(p))
        except OSError:
            sizes.append(0)
        if sizes[-1] == 0:
            on_host.append(i)
    live = [i for i in range(len(paths)) if sizes[i] > 0]
    t0 = _tick(timing, "file", t0)
    for a, b in (_chunks([sizes[i] + 1 for i in live], chunk_bytes) if live else []):
        with torch.cuda.device(device):
            part = live[a:b]
            pinned = torch.empty(sum(sizes[i] + 1 for i in part), dtype=torch.uint8, pin_memory=True)
            host = pinned.numpy()
            file_off = np.zeros(len(part) + 1, np.int64)
            at = 0
            for j, i in enumerate(part):
                with open(paths[i], "rb", buffering=0) as f:
                    n = f.readinto(memoryview(host)[at:at + sizes[i]])
                at += n
                if n and host[at - 1] != 10:                       # every non-empty file ends in '\n'
                    host[at] = 10
                    at += 1
                file_off[j + 1] = at
            t0 = _tick(timing, "file", t0)
            text = pinned[:at].to(device)
            foff = torch.from_numpy(file_off).to(device)
            t0 = _tick(timing, "upload", t0, sync=True)
            line_pos, file_line_off = ops.text_lines(text, foff)
            rows, flags = ops.text_parse(text, line_pos, ncol)
            # per file: lines, flagged lines, lines with the surplus field
            bad = _exclusive((flags & ops.TEXT_LINE_FLAGGED) != 0)
            surplus = _exclusive(flags == ops.TEXT_LINE_SURPLUS)
            lo, hi = file_line_off[:-1], file_line_off[1:]
            per_file = torch.stack((bad[hi] - bad[lo], surplus[hi] - surplus[lo]), 1)
            t0 = _tick(timing, "kernels", t0, sync=True)
            rows_h = rows.cpu().numpy()
            flo = file_line_off.cpu().numpy()
            per_file = per_file.cpu().numpy()
            t0 = _tick(timing, "download", t0)
            for j, i in enumerate(part):
                n = int(flo[j + 1] - flo[j])
                bad, surplus = int(per_file[j, 0]), int(per_file[j, 1])
                if n == 0 or bad or (surplus and surplus != n):
                    on_host.append(i)
                else:
                    out[i] = rows_h[flo[j]:flo[j + 1]]
    t0 = time.perf_counter()
    for i in on_host:
        out[i] = host_read(paths[i])
    _tick(timing, "host", t0)
    return out, len(on_host)


def format_rows_host(rows, layout, clamp):
    """The writers' own expressions (RRNetOperator / CenterNetOperator / RetinaNetOperator.write_results) on host rows ->
    bytes; raises what they raise."""
    layout = LAYOUTS.get(layout, layout)
    rows = np.asarray(rows).astype(np.float32, copy=False).reshape(-1, 6)
    if clamp:
        rows = np.where(rows < 0, np.float32(0.), rows)
    if layout == 0:
        text = ''.join('%f,%f,%f,%f,%.4f,%d,-1,-1\n' % (r[0], r[1], r[2], r[3], r[4], int(r[5])) for r in rows.tolist())
    elif layout == 1:
        rows = np.concatenate((np.rint(rows[:, :4]), rows[:, 4:]), axis=1)
        text = ''.join('%d,%d,%d,%d,%.4f,%d,-1,-1\n' % (int(r[0]), int(r[1]), int(r[2]) - int(r[0]), int(r[3]) - int(r[1]),
                                                        r[4], int(r[5])) for r in rows.tolist())
    elif layout == 2:
        text = ''.join('%d,%d,%d,%d,%.4f,%d,-1,-1\n' % (int(r[0]), int(r[1]), int(r[2]), int(r[3]), r[4], int(r[5]))
                       for r in rows.tolist())
    else:
        raise ValueError("format_rows_host: layout %r" % (layout,))
    return text.encode()


def format_frames(rows6, frame_off, layout, clamp, timing=None, chunk_bytes=CHUNK_BYTES):
    """rows6: device float32 [R,6]; frame_off [F+1] row offsets (tensor, array or list) -> list of F bytes-like objects, the
    text of each frame's rows in `layout` ("rrnet" / 0: RRNetOperator.write_results and ensemble.format_rows, "centernet" /
    1, "retinanet" / 2), with the writers' clamp where `clamp`.  rr_text_format_len, an exclusive sum, rr_text_format, one
    download.  A frame with a flagged row is formatted by the host expression instead (which raises where Python raises)."""
    from rrnet_amd import ops
    layout = LAYOUTS.get(layout, layout)
    off = np.asarray(frame_off.cpu() if torch.is_tensor(frame_off) else frame_off, np.int64)
    rows6 = rows6.detach().to(torch.float32)                # the writers' astype(float32)
    if rows6.dim() != 2 or rows6.shape[1] != 6:
        raise ValueError("format_frames: rows must be [R,6], got %s" % (tuple(rows6.shape),))
    if off.ndim != 1 or off.size < 1 or off[0] < 0 or off[-1] > rows6.shape[0] or (np.diff(off) < 0).any():
        raise ValueError("format_frames: frame_off must ascend inside [0, %d]" % rows6.shape[0])
    nf = off.size - 1
    out = [b""] * nf
    limit = max(chunk_bytes // ops.TEXT_MAX_ROW, 1)
    t0 = time.perf_counter()
    with torch.cuda.device(rows6.device):
        for a, b in (_chunks(np.diff(off).tolist(), limit) if nf else []):
            lo, hi = int(off[a]), int(off[b])
            if hi == lo:
                continue
            part = rows6[lo:hi].contiguous()
            length, flag, byte_off = ops.text_format_len(part, layout, clamp)
            rel = torch.from_numpy(off[a:b + 1] - lo).to(part.device)
            marks = torch.stack((byte_off[rel], _exclusive(flag)[rel]), 1).cpu().numpy()     # the one sync: bytes and flags
            buf = torch.empty(int(marks[-1, 0]), dtype=torch.uint8, device=part.device)
            ops.text_format(part, layout, clamp, byte_off, buf)
            t0 = _tick(timing, "kernels", t0, sync=True)
            pinned = torch.empty(buf.numel(), dtype=torch.uint8, pin_memory=True)
            pinned.copy_(buf)
            view = memoryview(pinned.numpy())
            t0 = _tick(timing, "download", t0)
            for j in range(b - a):
                if marks[j + 1, 1] != marks[j, 1]:
                    out[a + j] = format_rows_host(rows6[int(off[a + j]):int(off[a + j + 1])].cpu().numpy(), layout, clamp)
                else:
                    out[a + j] = view[int(marks[j, 0]):int(marks[j + 1, 0])]
            t0 = _tick(timing, "host", t0)
    return out


def _exclusive(counts):
    out = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
    torch.cumsum(counts, 0, dtype=torch.int64, out=out[1:])
    return out


def write_frames(paths, rows6, frame_off, layout, clamp, timing=None):
    """The files the writers produce for the frames of `rows6`, one per path, opened in binary mode."""
    bufs = format_frames(rows6, frame_off, layout, clamp, timing=timing)
    if len(bufs) != len(paths):
        raise ValueError("write_frames: %d paths for %d frames" % (len(paths), len(bufs)))
    t0 = time.perf_counter()
    for path, data in zip(paths, bufs):
        with open(path, "wb") as f:
            f.write(data)
    _tick(timing, "write", t0)
