"""VisDrone-DET AP / AR evaluation — the reference's utils/metrics/metrics.py (bbox_iou :10-49, get_tp :52-131,
calculate_ap_rc :134-176, evaluate_once :179-207, evaluate_results :210-253, auto_evaluate_results :256-306,
_ext_nms :309-323) with the same function names, arguments and printed report.

Host logic (file parsing, greedy matching, precision/recall integration) stays on the host as in the reference; it
is pinned against goldens produced by the reference's own get_tp / calculate_ap_rc / evaluate_once
(tests/golden/metrics.npz).  The part that dominates a threshold sweep — per-file, per-class Soft-NMS, called
files x classes times per (ctnet, softnms) threshold pair — runs as ONE batched launch of the bit-exact HIP
Soft-NMS over every (file, class) segment (`ext_nms_batch`).

With `device=` (evaluate_results, auto_evaluate_results, evaluate_arrays, sweep_evaluate_results; default None = the
host path above, unchanged) the matching and the AP integration run on the GPU as well: rr_eval_match / rr_eval_ap of
csrc/evalmatch.hip, see "the device evaluator" at the end of this file.

Differences from the reference, all in code that cannot run as written under numpy >= 1.24 / torch 2:
`np.int` / `np.float` (:234,:287) are spelled int64 / float64; the reference's `_ext_nms` (:309-323) has no return
statement and `auto_evaluate_results` mixes tensors and arrays (:286-289) — restated with the evident intent
(xywh float32 array back); evaluate_results / auto_evaluate_results also RETURN (ap, rc) besides printing.
Quirk kept: detections of a class are dropped (not counted as false positives) in images that hold no ground
truth of that class (:112-113)."""
import contextlib
import glob
import os
import time

import numpy as np
import torch

THRESHOLDS = torch.arange(0.5, 1.0, 0.05)


def bbox_iou(a, b, x1y1x2y2=True, overlap=False):
    """IoU [m,n] between box sets a [m,4], b [n,4]; with overlap=True also intersection / area(a)."""
    assert isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)
    a, b = a.clone().float(), b.clone().float()
    if not x1y1x2y2:
        a[:, 2:4] += a[:, 0:2]
        b[:, 2:4] += b[:, 0:2]
    a_area = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    b_area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    iw = (torch.min(a[:, 2:3], b[:, 2]) - torch.max(a[:, 0:1], b[:, 0])).clamp(min=0)
    ih = (torch.min(a[:, 3:4], b[:, 3]) - torch.max(a[:, 1:2], b[:, 1])).clamp(min=0)
    inter = iw * ih
    union = (a_area.unsqueeze(1) + b_area - inter).clamp(min=1e-8)
    iou = inter / union
    if overlap:
        return iou, inter / a_area.unsqueeze(1)
    return iou


def _greedy_match(tp_iou):
    """tp_iou [D,G,T]: IoU of detection d (score order) with same-class ground truth g where it clears threshold
    t, else 0.  Every (g, t) is given to the first detection whose best remaining match it is -> flags [D,T]."""
    d_n, g_n, t_n = tp_iou.shape
    work = tp_iou.clone()
    flags = torch.zeros(d_n, t_n)
    cols = torch.arange(t_n)
    for d in range(d_n):
        best, arg = work[d].max(dim=0)
        hit = best != 0
        if hit.any():
            work[:, arg[hit], cols[hit]] = 0
            flags[d, hit] = 1
    return flags


def get_tp(pred, target, cls_tp_flags, cls_tp_confs, cls_target_count, cls_in_img_count,
           thresholds=THRESHOLDS, cls_num=11):
    """One image: pred [m,6] = x,y,w,h,score,cls; target [n,>=6] VisDrone rows (cls 0 = ignored region).
    Appends per-class true-positive flags [d,T] / confidences and bumps the ground-truth counters."""
    order = torch.sort(pred[:, 4], descending=True)[1]
    pred = pred[order, :]
    # ground truth mostly inside an ignored region is removed (the regions themselves stay for the next step)
    ignore = target[:, 5] == 0
    if ignore.sum() != 0:
        _, gt_ov = bbox_iou(target[:, :4], target[:, :4], x1y1x2y2=False, overlap=True)
        keep = (gt_ov[:, ignore].max(dim=1)[0] < 0.5) | ignore
        target = target[keep, :]
    ignore = target[:, 5] == 0
    iou, ov = bbox_iou(pred[:, :4], target[:, :4], x1y1x2y2=False, overlap=True)
    if ignore.sum() != 0:
        keep = ov[:, ignore].max(dim=1)[0] < 0.5
        pred = pred[keep, :]
        iou = iou[keep, :]
    pred_cls = pred[:, 5].long()
    target_cls = target[:, 5].long()
    thr = thresholds.to(iou.dtype)
    for cls in range(1, cls_num):
        g_sel = target_cls == cls
        n_gt = int(g_sel.sum())
        cls_target_count[cls - 1] += n_gt
        cls_in_img_count[cls - 1] += 1 if n_gt != 0 else 0
        d_sel = pred_cls == cls
        if n_gt == 0 or int(d_sel.sum()) == 0:
            continue
        sub = iou[d_sel][:, g_sel]                                       # [D,G]
        clears = (sub.unsqueeze(2) - thr) >= 0
        flags = _greedy_match(sub.unsqueeze(2) * clears.float())
        cls_tp_flags[cls - 1] = torch.cat((cls_tp_flags[cls - 1], flags))
        cls_tp_confs[cls - 1] = torch.cat((cls_tp_confs[cls - 1], pred[d_sel, 4]))
    return cls_tp_flags, cls_tp_confs, cls_target_count, cls_in_img_count


def calculate_ap_rc(cls_tp_flags, cls_tp_confs, cls_target_count, cls_in_img_count):
    """-> AP per IoU threshold [T] (classes weighted by the number of images they occur in), mean max recall."""
    cls_num = cls_target_count.size(0)
    t_n = cls_tp_flags[0].size(1)
    total_ap = torch.zeros(t_n)
    total_rc = torch.zeros(t_n)
    for cls in range(cls_num):
        if cls_target_count[cls] == 0:
            continue
        order = torch.sort(cls_tp_confs[cls], descending=True)[1]
        tp_cum = cls_tp_flags[cls][order, :].cumsum(dim=0)
        rank = torch.arange(1., tp_cum.size(0) + 1, step=1.).unsqueeze(1)
        prec = tp_cum / rank
        rec = tp_cum / cls_target_count[cls].clamp(min=1)
        mrec = torch.cat((torch.zeros(1, t_n), rec, torch.ones(1, t_n)))
        mpre = torch.cat((torch.zeros(1, t_n), prec, torch.zeros(1, t_n)))
        mpre = torch.flip(torch.cummax(torch.flip(mpre, [0]), dim=0)[0], [0])     # precision envelope
        step = ((mrec[1:] - mrec[:-1]) > 0).float()
        total_ap += torch.sum((mrec[1:] * step - mrec[:-1] * step) * mpre[1:] * step, dim=0) * cls_in_img_count[cls]
        total_rc += mrec[:-1].max(dim=0)[0] * cls_in_img_count[cls]
    ap = total_ap / cls_in_img_count.sum()
    rc = (total_rc / cls_in_img_count.sum()).mean()
    return ap, rc


def _fresh(cls_num, t_n):
    return ([torch.zeros(0, t_n) for _ in range(1, cls_num)], [torch.zeros(0) for _ in range(1, cls_num)],
            torch.zeros(cls_num - 1), torch.zeros(cls_num - 1))


def evaluate_once(pred, target, thresholds=THRESHOLDS, cls_num=11, max_det_num=500):
    assert isinstance(pred, torch.Tensor) and isinstance(target, torch.Tensor)
    flags, confs, tc, ic = _fresh(cls_num, thresholds.size(0))
    flags, confs, tc, ic = get_tp(pred[:max_det_num], target, flags, confs, tc, ic, thresholds, cls_num)
    ap, rc = calculate_ap_rc(flags, confs, tc, ic)
    print(ap)
    return ap, rc


def _read(path):
    import pandas as pd
    return np.array(pd.read_csv(path, header=None, float_precision='high'))


_TEXT = ["host"]                 # how the device evaluators read their files; text_route() changes it for a block


@contextlib.contextmanager
def text_route(text):
    """with text_route("device"): evaluate_results(..., device=dev) parses the files on the device as well (rrnet_amd.textio);
    "host" is the default, pandas per file.  The evaluators' signatures stay the reference's plus `device`."""
    if text not in ("host", "device"):
        raise ValueError("text=%r, expected 'host' or 'device'" % (text,))
    _TEXT.append(text)
    try:
        yield
    finally:
        _TEXT.pop()


def _reader(pred_dir, target_dir, text, device):
    """path -> rows for the result and annotation files of one evaluation.  text="host": _read itself.  text="device": every
    file goes through rrnet_amd.textio.read_files once (one upload, the parse kernels, one download; files the codec flags
    are read by _read), and the function looks the arrays up."""
    if text == "host":
        return _read
    if text != "device":
        raise ValueError("text=%r, expected 'host' or 'device'" % (text,))
    from rrnet_amd import textio
    paths = [os.path.join(d, "{}.txt".format(name)) for name in _names(pred_dir) for d in (pred_dir, target_dir)]
    arrays, _ = textio.read_files(paths, device, host_read=_read)
    return dict(zip(paths, arrays)).__getitem__


def _names(pred_dir):
    return [os.path.splitext(os.path.basename(x))[0] for x in glob.glob(os.path.join(pred_dir, '*.txt'))]


def _snap(pred):
    """xywh -> integer corner coordinates -> xywh (:232-235)."""
    pred[:, 2:4] += pred[:, 0:2]
    pred[:, :4] = pred[:, :4].astype(np.int64).astype(np.float64)
    pred[:, 2:4] -= pred[:, 0:2]
    return pred


def _report(ap, rc, st):
    print("Average Precision  (AP) @[ IoU=0.50:0.95] = {:.4}.".format(ap.mean().item()))
    print("Average Precision  (AP) @[ IoU=0.50     ] = {:.4}.".format(ap[0].item()))
    print("Average Precision  (AP) @[ IoU=0.75     ] = {:.4}.".format(ap[5].item()))
    print("Average Recall     (AR) @[ IoU=0.50:0.95] = {:.4}.".format(rc.item()))
    print("Cost Time: {}s".format(time.time() - st))


def evaluate_results(pred_dir, target_dir, thresholds=THRESHOLDS, cls_num=11, max_det_num=500, device=None):
    if device is not None:
        return _evaluate_results_device(pred_dir, target_dir, thresholds, cls_num, max_det_num, device, text=_TEXT[-1])
    st = time.time()
    flags, confs, tc, ic = _fresh(cls_num, thresholds.size(0))
    for name in _names(pred_dir):
        pred = _snap(_read(os.path.join(pred_dir, "{}.txt".format(name))).astype(np.float64))
        pred = torch.from_numpy(pred).float()[:max_det_num]
        target = torch.from_numpy(_read(os.path.join(target_dir, "{}.txt".format(name)))).float()[:max_det_num]
        flags, confs, tc, ic = get_tp(pred, target, flags, confs, tc, ic, thresholds, cls_num)
    ap, rc = calculate_ap_rc(flags, confs, tc, ic)
    _report(ap, rc, st)
    return ap, rc


def ext_nms_batch(preds, threshold, max_classes=32):
    """Per-class gaussian Soft-NMS (Nt 0.7) of MANY detection sets in one launch.  preds: list of float32 [n_i,6]
    xywh,score,cls arrays / tensors -> list of float32 numpy [n_i',6] xywh arrays, each in the order
    `np.concatenate` over ascending classes gives (:313-323)."""
    from rrnet_amd import ops
    from rrnet_amd.ext.nms.nms_wrapper import soft_nms_segments
    nf = len(preds)
    kmax = max((int(p.shape[0]) for p in preds), default=0)
    if kmax == 0:
        return [np.zeros((0, 6), np.float32) for _ in preds]
    host = np.full((nf, kmax, 6), -1.0, np.float32)          # class -1 rows are padding: grouping drops them
    for i, p in enumerate(preds):
        p = p.detach().cpu().numpy() if torch.is_tensor(p) else np.asarray(p)
        host[i, :p.shape[0]] = p[:, :6]
        cls = p[:, 5].astype(np.int64)
        assert cls.size == 0 or (cls.min() >= 0 and cls.max() < max_classes), "class id outside [0, %d)" % max_classes
    dev = torch.device("cuda", torch.cuda.current_device())
    b = torch.from_numpy(host).to(dev)
    b[:, :, 2:4] += b[:, :, 0:2]
    grouped, seg_off, seg_len = ops.group_by_class(b, max_classes)   # explicit lengths: the padding leaves gaps
    rows = grouped.view(-1, 6)
    n_out = soft_nms_segments(rows, seg_off, kmax, sigma=0.5, Nt=0.7, threshold=threshold, method=2, seg_len=seg_len)
    _, _, _, kept, out_off = ops.pack_segments(rows, seg_off, n_out, max_classes, want_rois=False, want_rows=True,
                                               want_offsets=True)
    kept[:, 2:4] -= kept[:, 0:2]
    kept = kept.cpu().numpy()
    fo = out_off.cpu().numpy()[::max_classes]
    return [kept[fo[i]:fo[i + 1]] for i in range(nf)]


def _ext_nms(pred_bbox, threshold):
    """One detection set (:309-323)."""
    if pred_bbox.shape[0] == 0:
        return pred_bbox
    return ext_nms_batch([pred_bbox], threshold)[0]


def auto_evaluate_results(pred_dir, target_dir, ctnet_min_threshold, softnms_min_threshold, thresholds=THRESHOLDS,
                          cls_num=11, max_det_num=500, device=None):
    if device is not None:
        return _auto_evaluate_results_device(pred_dir, target_dir, ctnet_min_threshold, softnms_min_threshold,
                                             thresholds, cls_num, max_det_num, device, text=_TEXT[-1])
    st = time.time()
    names = _names(pred_dir)
    preds, targets = [], []
    for name in names:
        pred = _read(os.path.join(pred_dir, "{}.txt".format(name)))
        pred = torch.from_numpy(pred[pred[:, 4] > ctnet_min_threshold]).float()
        preds.append(pred[torch.sort(pred[:, 4], descending=True)[1]])
        targets.append(_read(os.path.join(target_dir, "{}.txt".format(name))))
    kept = ext_nms_batch(preds, softnms_min_threshold)        # every file and class in one launch
    flags, confs, tc, ic = _fresh(cls_num, thresholds.size(0))
    for pred, target in zip(kept, targets):
        pred = torch.from_numpy(_snap(pred.astype(np.float64))).float()
        pred = pred[torch.sort(pred[:, 4], descending=True)[1]][:max_det_num]
        target = torch.from_numpy(target).float()[:max_det_num]
        flags, confs, tc, ic = get_tp(pred, target, flags, confs, tc, ic, thresholds, cls_num)
    ap, rc = calculate_ap_rc(flags, confs, tc, ic)
    _report(ap, rc, st)
    return ap, rc


# ---- the device evaluator ------------------------------------------------------------------------------------------
# rr_eval_match / rr_eval_ap (csrc/evalmatch.hip) give get_tp's true-positive flags and calculate_ap_rc's AP / AR.  Two
# rules the host leaves to torch's unstable sort are DEFINED here: equal scores keep row order within a frame, equal
# confidences keep (frame, row) order within a class (torch.sort(stable=True) on the device).  On pairwise distinct
# scores both paths agree; on ties the host's answer depends on torch internals and this one does not.

def _rows6(x):
    x = x.detach().cpu() if torch.is_tensor(x) else torch.from_numpy(np.asarray(x))
    return x.float()[:, :6]


def _pad(rows, device):
    """list of float32 [n_i,6] host tensors -> device [F, max(n_i, 1), 6] zero padded, int32 [F] lengths: one upload."""
    lens = [int(r.shape[0]) for r in rows]
    host = torch.zeros((len(rows), max(lens + [1]), 6), dtype=torch.float32)
    for i, r in enumerate(rows):
        host[i, :lens[i]] = r
    return host.to(device), torch.tensor(lens, dtype=torch.int32).to(device)


def _sort_frames(dets, det_len):
    """Rows of every frame by score descending, equal scores in row order; padding stays behind."""
    live = torch.arange(dets.shape[1], device=dets.device).unsqueeze(0) < det_len.unsqueeze(1)
    key = torch.where(live, dets[:, :, 4], torch.full_like(dets[:, :, 4], float("-inf")))
    order = torch.sort(key, dim=1, descending=True, stable=True)[1]
    return torch.gather(dets, 1, order.unsqueeze(2).expand(-1, -1, 6)).contiguous()


def _device_eval(dets, det_len, gts, gt_len, thresholds, cls_num, want_detail=False):
    """dets [F,D,6] in evaluation order, gts [F,G,6], their int32 lengths, all on the device -> (ap [T], rc) device
    tensors and, on request, the per-class lists in get_tp's layout (host tensors)."""
    from rrnet_amd import ops
    dev = dets.device
    t_n, c_n = thresholds.numel(), cls_num - 1
    thr = thresholds.detach().to(torch.float32).contiguous().to(dev)       # the host's values, not recomputed
    bits, counted, tc = ops.eval_match(dets, det_len, gts, gt_len, thr, cls_num)
    target_count = tc.sum(dim=0).to(torch.int32)
    in_img_count = (tc > 0).sum(dim=0).to(torch.int32)
    idx = counted.view(-1).nonzero().squeeze(1)                             # (frame, row) order
    rows = dets.view(-1, 6)
    cls = rows[idx, 5].long() - 1
    conf = rows[idx, 4]
    word = bits.view(-1)[idx]
    by_conf = torch.sort(conf, descending=True, stable=True)[1]
    order = by_conf[torch.sort(cls[by_conf], stable=True)[1]]               # class by class, confidence descending
    per_cls = torch.bincount(cls, minlength=c_n)
    seg_off = torch.zeros(c_n + 1, dtype=torch.int32, device=dev)
    seg_off[1:] = per_cls.cumsum(0)
    ap, rc = ops.eval_ap(word[order].contiguous(), seg_off, target_count, in_img_count, t_n)
    if not want_detail:
        return ap, rc, None
    host_order = torch.sort(cls, stable=True)[1]                            # get_tp's layout: (frame, row) inside a class
    flags = ((word[host_order].unsqueeze(1) >> torch.arange(t_n, device=dev)) & 1).float().cpu()
    confs = conf[host_order].cpu()
    split = per_cls.cpu().tolist()
    detail = {"flags": list(torch.split(flags, split)), "confs": list(torch.split(confs, split)),
              "target_count": target_count.float().cpu(), "in_img_count": in_img_count.float().cpu()}
    return ap, rc, detail


def _evaluate_device(preds, targets, thresholds, cls_num, device, want_detail=False):
    """Host lists of cut [n,6] rows -> one upload, a stable per-frame sort, the two kernels."""
    dets, det_len = _pad(preds, device)
    gts, gt_len = _pad(targets, device)
    ap, rc, detail = _device_eval(_sort_frames(dets, det_len), det_len, gts, gt_len, thresholds, cls_num, want_detail)
    return ap.cpu(), rc.cpu(), detail


def evaluate_arrays(preds, targets, thresholds=THRESHOLDS, cls_num=11, max_det_num=500, device=None):
    """In-memory form of evaluate_results: preds / targets are lists of [n,>=6] arrays or tensors (detections x,y,w,h,
    score,cls; VisDrone annotation rows), one pair per image, each cut to max_det_num rows as evaluate_results cuts
    them.  device=None runs get_tp / calculate_ap_rc on the host; a torch.device runs rr_eval_match / rr_eval_ap.
    -> (ap [T], rc, detail); detail = {"flags": [cls_num-1] x [d,T], "confs": [cls_num-1] x [d], "target_count",
    "in_img_count"} in get_tp's layout."""
    preds = [_rows6(p)[:max_det_num] for p in preds]
    targets = [_rows6(t)[:max_det_num] for t in targets]
    if device is not None:
        return _evaluate_device(preds, targets, thresholds, cls_num, torch.device(device), want_detail=True)
    flags, confs, tc, ic = _fresh(cls_num, thresholds.size(0))
    for pred, target in zip(preds, targets):
        flags, confs, tc, ic = get_tp(pred, target, flags, confs, tc, ic, thresholds, cls_num)
    ap, rc = calculate_ap_rc(flags, confs, tc, ic)
    return ap, rc, {"flags": flags, "confs": confs, "target_count": tc, "in_img_count": ic}


def _evaluate_results_device(pred_dir, target_dir, thresholds, cls_num, max_det_num, device, text="host"):
    st = time.time()
    preds, targets = [], []
    read = _reader(pred_dir, target_dir, text, device)
    for name in _names(pred_dir):
        pred = _snap(read(os.path.join(pred_dir, "{}.txt".format(name))).astype(np.float64))
        preds.append(torch.from_numpy(pred).float()[:max_det_num, :6])
        targets.append(torch.from_numpy(read(os.path.join(target_dir, "{}.txt".format(name)))).float()[:max_det_num, :6])
    ap, rc, _ = _evaluate_device(preds, targets, thresholds, cls_num, torch.device(device))
    _report(ap, rc, st)
    return ap, rc


def _auto_evaluate_results_device(pred_dir, target_dir, ctnet_min_threshold, softnms_min_threshold, thresholds, cls_num,
                                  max_det_num, device, text="host"):
    st = time.time()
    preds, targets = [], []
    read = _reader(pred_dir, target_dir, text, device)
    for name in _names(pred_dir):
        pred = read(os.path.join(pred_dir, "{}.txt".format(name)))
        pred = torch.from_numpy(pred[pred[:, 4] > ctnet_min_threshold]).float()
        preds.append(pred[torch.sort(pred[:, 4], descending=True, stable=True)[1]])
        targets.append(torch.from_numpy(read(os.path.join(target_dir, "{}.txt".format(name)))).float()[:max_det_num, :6])
    kept = ext_nms_batch(preds, softnms_min_threshold)
    preds = []
    for pred in kept:
        pred = torch.from_numpy(_snap(pred.astype(np.float64))).float()
        preds.append(pred[torch.sort(pred[:, 4], descending=True, stable=True)[1]][:max_det_num, :6])
    ap, rc, _ = _evaluate_device(preds, targets, thresholds, cls_num, torch.device(device))
    _report(ap, rc, st)
    return ap, rc


def _sweep_read(pred_dir, target_dir, ctnet_min_thresholds, max_det_num, text="host", device=None):
    """Every file once -> score-sorted float32 detections, per (ctnet threshold, file) how many of them pass the score
    filter (a prefix: the filter compares the parsed float64 score as auto_evaluate_results does), cut annotations."""
    preds, targets, lens = [], [], []
    read = _reader(pred_dir, target_dir, text, device)
    for name in _names(pred_dir):
        raw = read(os.path.join(pred_dir, "{}.txt".format(name)))
        order = torch.sort(torch.from_numpy(raw[:, 4]).float(), descending=True, stable=True)[1].numpy()
        raw = raw[order]
        row = []
        for ct in ctnet_min_thresholds:
            keep = raw[:, 4] > ct
            n = int(keep.sum())
            if not keep[:n].all():
                raise ValueError("%s: scores on both sides of ctnet_min_threshold %r are equal in float32" % (name, ct))
            row.append(n)
        lens.append(row)
        preds.append(torch.from_numpy(raw).float()[:, :6])
        targets.append(torch.from_numpy(read(os.path.join(target_dir, "{}.txt".format(name)))).float()[:max_det_num, :6])
    return preds, targets, np.asarray(lens, np.int32).reshape(len(preds), len(ctnet_min_thresholds)).T


def sweep_nms_rows(dets, live_len, softnms_min_threshold, max_det_num=500, max_classes=32):
    """One (ctnet, softnms) pair of the sweep up to the rows that enter the matching, all on the device.  dets [F,K,6]
    score-sorted xywh rows, live_len int32 [F]: the prefix of every frame that passed the score filter.  Per-class
    gaussian Soft-NMS exactly as ext_nms_batch runs it, the integer snap of `_snap` (the add and the truncation in
    float64), a stable per-frame sort by score and the cut to max_det_num -> rows [F,D,6], det_len int32 [F]."""
    from rrnet_amd import ops
    from rrnet_amd.ext.nms.nms_wrapper import soft_nms_segments
    dev = dets.device
    nf, kmax, _ = dets.shape
    b = dets.clone()
    live = torch.arange(kmax, device=dev).unsqueeze(0) < live_len.unsqueeze(1)
    b[:, :, 5] = torch.where(live, b[:, :, 5], torch.full_like(b[:, :, 5], -1.0))   # class -1: grouping drops the row
    b[:, :, 2:4] += b[:, :, 0:2]
    grouped, seg_off, seg_len = ops.group_by_class(b, max_classes)
    rows = grouped.view(-1, 6)
    n_out = soft_nms_segments(rows, seg_off, kmax, sigma=0.5, Nt=0.7, threshold=softnms_min_threshold, method=2,
                              seg_len=seg_len)
    _, _, _, kept, out_off = ops.pack_segments(rows, seg_off, n_out, max_classes, want_rois=False, want_rows=True,
                                               want_offsets=True)
    kept[:, 2:4] -= kept[:, 0:2]
    wide = kept[:, :4].double()                                      # _snap: x+w in float64, truncate, subtract
    lo = wide[:, 0:2].trunc()
    hi = (wide[:, 2:4] + wide[:, 0:2]).trunc()
    kept[:, 0:2] = lo.float()
    kept[:, 2:4] = (hi - lo).float()
    fo = out_off[::max_classes].long()
    r = kept.shape[0]
    frame = torch.searchsorted(fo[1:].contiguous(), torch.arange(r, device=dev), right=True)
    by_score = torch.sort(kept[:, 4], descending=True, stable=True)[1]
    order = by_score[torch.sort(frame[by_score], stable=True)[1]]   # frame by frame, score descending, ties in row order
    frame = frame[order]
    rank = torch.arange(r, device=dev) - fo[frame]
    det_len = (fo[1:] - fo[:-1]).clamp(max=max_det_num).to(torch.int32)
    out = torch.zeros((nf, max(int(det_len.max()) if nf else 0, 1), 6), dtype=torch.float32, device=dev)
    fits = rank < max_det_num
    out[frame[fits], rank[fits]] = kept[order][fits]
    return out, det_len


def sweep_evaluate_results(pred_dir, target_dir, ctnet_min_thresholds, softnms_min_thresholds, thresholds=THRESHOLDS,
                           cls_num=11, max_det_num=500, device=None):
    """auto_evaluate_results for every (ctnet_min, softnms_min) pair, in scripts/RRNet/auto_eval.py's loop order, with
    the report printed per pair -> float32 array [n_ct, n_snms, T+1]: AP per IoU threshold, then AR.
    device=None loops over auto_evaluate_results (which reads every file again per pair).  With a torch.device every
    file is read once, the score-sorted detections and the annotations are uploaded once, and each pair runs score
    filter -> per-class Soft-NMS -> snap -> sort and cut -> rr_eval_match -> rr_eval_ap without leaving the device."""
    out = np.zeros((len(ctnet_min_thresholds), len(softnms_min_thresholds), thresholds.size(0) + 1), np.float32)
    if device is None:
        for i, ct in enumerate(ctnet_min_thresholds):
            for j, snms in enumerate(softnms_min_thresholds):
                ap, rc = auto_evaluate_results(pred_dir, target_dir, ct, snms, thresholds, cls_num, max_det_num)
                out[i, j, :-1], out[i, j, -1] = ap.numpy(), float(rc)
        return out
    device = torch.device(device)
    preds, targets, lens = _sweep_read(pred_dir, target_dir, ctnet_min_thresholds, max_det_num, text=_TEXT[-1], device=device)
    dets, _ = _pad(preds, device)
    gts, gt_len = _pad(targets, device)
    lens = torch.from_numpy(np.ascontiguousarray(lens)).to(device)
    for i in range(len(ctnet_min_thresholds)):
        for j, snms in enumerate(softnms_min_thresholds):
            st = time.time()
            rows, det_len = sweep_nms_rows(dets, lens[i], snms, max_det_num)
            ap, rc, _ = _device_eval(rows, det_len, gts, gt_len, thresholds, cls_num)
            ap, rc = ap.cpu(), rc.cpu()
            _report(ap, rc, st)
            out[i, j, :-1], out[i, j, -1] = ap.numpy(), float(rc)
    return out
