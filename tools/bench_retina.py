"""Times RetinaNet's criterion and decode kernels against the same chains written in plain torch ops on the device.

  python tools/bench_retina.py [--batch 2] [--size 512 512] [--boxes 100] [--classes 10] [--iters 50] [--nms-frames 4]
                               [--out profiles/retina.json]

criterion: RF.retina_criterion forward + backward (rr_retina_assign, rr_retina_loss_fwd, rr_retina_loss_bwd) against the
per-image loop of tensor operations the reference's operator runs (IoU table, max, masks, focal loss, smooth-L1, autograd).
decode: rr_retina_decode for the batch against the per-image chain of tensor operations (sigmoid, max, mask, gather, exp,
stack).  decode_frames: rr_retina_decode_frames (an image's anchors over many workgroups) beside rr_retina_decode (one
workgroup per image) at the shape above and at B = 1 / 4 on the 192 888 anchors of a 1360x765 frame.  nms_frames:
rr_nms_frames for B frames beside B calls of rr_nms_sorted (without the read of num_out that its callers add) at 1000 and
8000 score-ordered rows per frame.  Times are medians of HIP-event intervals after a warm-up; the result is a report,
nothing is asserted."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_criterion(loc_preds, cls_preds, annos, anchors):
    bs = cls_preds.size(0)
    boxes = annos[:, :, :4].clone()
    boxes[:, :, 2:4] += boxes[:, :, 0:2]
    aw, ah = anchors[:, 2] - anchors[:, 0], anchors[:, 3] - anchors[:, 1]
    acx, acy = anchors[:, 0] + 0.5 * aw, anchors[:, 1] + 0.5 * ah
    a_area = aw * ah
    cls_losses, reg_losses = [], []
    for n in range(bs):
        g = boxes[n]
        iw = (torch.min(g[:, None, 2], anchors[None, :, 2]) - torch.max(g[:, None, 0], anchors[None, :, 0])).clamp(min=0)
        ih = (torch.min(g[:, None, 3], anchors[None, :, 3]) - torch.max(g[:, None, 1], anchors[None, :, 1])).clamp(min=0)
        inter = iw * ih
        union = (((g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]))[:, None] + a_area[None, :] - inter).clamp(min=1e-8)
        best, which = (inter / union).max(dim=0)
        pos = best >= 0.5
        used = pos | (best < 0.4)
        npos = pos.sum()
        target = torch.zeros_like(cls_preds[n])
        picked = g[which[pos]]
        target[pos, annos[n][which[pos], 5].long() - 1] = 1
        p = torch.sigmoid(cls_preds[n][used]).clamp(1e-7, 1. - 1e-7)
        t = target[used]
        hot = t == 1.
        w = torch.where(hot, 0.75 * (1. - p) ** 2, 0.25 * p ** 2)
        cls_losses.append((w * -(t * torch.log(p) + (1. - t) * torch.log(1. - p))).sum() / npos.float().clamp(min=1.))
        gw, gh = picked[:, 2] - picked[:, 0], picked[:, 3] - picked[:, 1]
        gcx, gcy = picked[:, 0] + 0.5 * gw, picked[:, 1] + 0.5 * gh
        gw, gh = gw.clamp(min=1), gh.clamp(min=1)
        tgt = torch.stack(((gcx - acx[pos]) / aw[pos], (gcy - acy[pos]) / ah[pos], torch.log(gw / aw[pos]),
                           torch.log(gh / ah[pos])), dim=1) / torch.tensor([0.1, 0.1, 0.2, 0.2], device=g.device)
        d = (tgt - loc_preds[n][pos]).abs()
        reg = torch.where(d <= 1.0 / 9.0, 4.5 * d * d, d - 0.5 / 9.0)
        reg_losses.append(reg.sum() / (npos.float() * 4).clamp(min=1.))
    return sum(cls_losses) / bs, sum(reg_losses) / bs


def torch_decode(cls_preds, loc_preds, anchors):
    out = []
    for n in range(cls_preds.size(0)):
        prob, which = torch.sigmoid(cls_preds[n]).max(dim=1)
        keep = prob > 0.1
        box, d = anchors[keep], loc_preds[n][keep]
        w, h = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
        pw, ph = torch.exp(d[:, 2] * 0.2) * w, torch.exp(d[:, 3] * 0.2) * h
        px = box[:, 0] + 0.5 * w + d[:, 0] * 0.1 * w - 0.5 * pw
        py = box[:, 1] + 0.5 * h + d[:, 1] * 0.1 * h - 0.5 * ph
        out.append(torch.stack((px, py, pw, ph, prob[keep], (which[keep] + 1).float()), dim=1))
    return out


def clustered_rows(n, seed):
    """n score-descending x,y,w,h,score,class rows: clusters of about four overlapping boxes on a quarter-pixel grid."""
    g = np.random.default_rng(seed)
    centres = g.uniform(0, 40.0 * np.sqrt(n), (max(n // 4, 1), 2))
    rows = np.zeros((n, 6), dtype=np.float32)
    rows[:, 0:2] = np.round((centres[g.integers(0, len(centres), n)] + g.uniform(-6, 6, (n, 2))) * 4) / 4
    rows[:, 2:4] = np.round(g.uniform(12, 36, (n, 2)) * 4) / 4
    rows[:, 4], rows[:, 5] = g.uniform(0.1, 1.0, n), g.integers(1, 11, n)
    return rows[np.argsort(-rows[:, 4], kind="stable")]


def bench_decode_frames(report, key, cls, loc, anchors, iters):
    from rrnet_amd import ops
    rows, count = ops.retina_decode(cls, loc, anchors)
    rows_f, count_f = ops.retina_decode_frames(cls, loc, anchors)
    n = count.tolist()
    same = torch.equal(count, count_f) and all(torch.equal(rows[i, :k], rows_f[i, :k]) for i, k in enumerate(n))
    one, _ = timed(lambda: ops.retina_decode(cls, loc, anchors), iters)
    many, _ = timed(lambda: ops.retina_decode_frames(cls, loc, anchors), iters)
    report[key] = {"batch": cls.size(0), "anchors": cls.size(1), "kept": n, "same_rows": bool(same), "decode_ms": one,
                   "decode_frames_ms": many, "speedup": one / many}


def bench_nms_frames(report, key, b, n, iters):
    from rrnet_amd import _C, ops
    dev = torch.device("cuda", 0)
    frames = [torch.from_numpy(clustered_rows(n, 100 + i)).to(dev) for i in range(b)]
    packed = torch.cat(frames)
    off = torch.arange(b + 1, dtype=torch.int32, device=dev) * n
    xyxy = [f.clone() for f in frames]
    for t in xyxy:
        t[:, 2:4] += t[:, 0:2]
    ws = torch.empty(_C.fn("rr_nms_workspace_bytes")(n), dtype=torch.uint8, device=dev)
    keep1 = torch.empty((b, n), dtype=torch.int32, device=dev)
    num1 = torch.zeros(b, dtype=torch.int32, device=dev)
    f_sorted = _C.fn("rr_nms_sorted")

    def sequential():
        for i in range(b):
            _C.check(f_sorted(_C.ptr(xyxy[i]), n, 6, 0.3, 0, _C.ptr(ws), _C.ptr(keep1[i]), _C.ptr(num1[i:]), _C.stream()),
                     "rr_nms_sorted")

    sequential()
    keep, kept = ops.nms_frames(packed, off, n, 0.3)
    same = torch.equal(kept, num1) and all(torch.equal(keep[i * n:i * n + k], keep1[i, :k]) for i, k in enumerate(kept.tolist()))
    seq, _ = timed(sequential, iters)
    bat, _ = timed(lambda: ops.nms_frames(packed, off, n, 0.3), iters)
    pack, _ = timed(lambda: ops.pack_frames(packed, off, keep, kept, n), iters)
    report[key] = {"frames": b, "rows_per_frame": n, "kept": kept.tolist(), "same_indices": bool(same),
                   "nms_sorted_calls_ms": seq, "nms_frames_ms": bat, "pack_frames_ms": pack, "speedup": seq / bat}


def timed(fn, iters, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), float(np.min(times))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--size", type=int, nargs=2, default=(512, 512))
    ap.add_argument("--boxes", type=int, default=100)
    ap.add_argument("--classes", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--nms-frames", type=int, default=4, help="frames of the rr_nms_frames comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retina.json"))
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_retina.py needs the GPU")
    from rrnet_amd import functional as RF
    from rrnet_amd import ops
    from rrnet_amd.modules.anchor import Anchors
    dev = torch.device("cuda", 0)
    h, w = args.size
    anchors = Anchors(sizes=(16, 64, 128))((h, w)).to(dev)
    a, b, c = anchors.size(0), args.batch, args.classes
    g = torch.Generator().manual_seed(219)
    xy = torch.rand((b, args.boxes, 2), generator=g) * torch.tensor([w - 80.0, h - 80.0])
    wh = 8.0 + torch.rand((b, args.boxes, 2), generator=g) * 70.0
    annos = torch.zeros((b, args.boxes + 20, 8))                 # 20 padding rows, as a collate leaves them
    annos[:, :args.boxes, 0:2], annos[:, :args.boxes, 2:4] = xy, wh
    annos[:, :args.boxes, 5] = torch.randint(1, c + 1, (b, args.boxes), generator=g).float()
    annos = annos.to(dev)
    loc = (torch.randn((b, a, 4), generator=g) * 0.5).to(dev).requires_grad_()
    cls = (torch.randn((b, a, c), generator=g) * 2.0 - 3.0).to(dev).requires_grad_()

    def hip_criterion():
        loc.grad = cls.grad = None
        cl, ll = RF.retina_criterion(loc, cls, annos, anchors, c)
        (cl + ll).backward()
        return cl, ll

    def plain_criterion():
        loc.grad = cls.grad = None
        cl, ll = torch_criterion(loc, cls, annos, anchors)
        (cl + ll).backward()
        return cl, ll

    hc, pc = hip_criterion(), plain_criterion()
    g_hip = (loc.grad.clone(), cls.grad.clone())
    hip_criterion()
    report = {
        "device": torch.cuda.get_device_name(0), "batch": b, "size": [h, w], "anchors": a, "classes": c, "boxes": args.boxes,
        "positives": ops.retina_assign(annos, anchors, c)["npos"].tolist(), "iters": args.iters,
        "criterion_losses_hip": [float(hc[0]), float(hc[1])], "criterion_losses_torch": [float(pc[0]), float(pc[1])],
    }
    plain_criterion()
    report["criterion_grad_max_abs_diff"] = [float((loc.grad - g_hip[0]).abs().max()), float((cls.grad - g_hip[1]).abs().max())]
    for name, fn in (("criterion_hip_ms", hip_criterion), ("criterion_torch_ms", plain_criterion)):
        report[name], report[name.replace("_ms", "_min_ms")] = timed(fn, args.iters)
    with torch.no_grad():
        cd, ld = cls.detach(), loc.detach()
        rows, count = ops.retina_decode(cd, ld, anchors)
        plain = torch_decode(cd, ld, anchors)
        report["decode_kept"] = count.tolist()
        report["decode_kept_torch"] = [int(p.size(0)) for p in plain]
        for name, fn in (("decode_hip_ms", lambda: ops.retina_decode(cd, ld, anchors)),
                         ("decode_torch_ms", lambda: torch_decode(cd, ld, anchors))):
            report[name], report[name.replace("_ms", "_min_ms")] = timed(fn, args.iters)
        bench_decode_frames(report, "decode_frames", cd, ld, anchors, args.iters)
        big = Anchors(sizes=(16, 64, 128))((765, 1360)).to(dev)                # a 1360x765 VisDrone frame: 192 888 anchors
        for bb in (1, 4):
            lg = (torch.randn((bb, big.size(0), c), generator=g) * 2.0 - 3.0).to(dev)
            lo = (torch.randn((bb, big.size(0), 4), generator=g) * 0.5).to(dev)
            bench_decode_frames(report, "decode_frames_1360x765_b%d" % bb, lg, lo, big, args.iters)
            del lg, lo
        for n in (1000, 8000):
            bench_nms_frames(report, "nms_frames_%d_rows" % n, args.nms_frames, n, args.iters if n <= 1000 else 10)
    report["criterion_speedup"] = report["criterion_torch_ms"] / report["criterion_hip_ms"]
    report["decode_speedup"] = report["decode_torch_ms"] / report["decode_hip_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(report, sort_keys=True))


if __name__ == "__main__":
    main()
