"""Weighted boxes fusion as include/rrnet_hip.h states it (rr_wbf_segments), restated in numpy, and the table of cases that
tests/test_wbf_host.py proves things about and tests/test_wbf_gpu.py runs the kernel on.  The restatement is the only
yardstick: float32 scalars / elementwise float32 arrays for the IoU, Python floats for the sums.  No golden file."""
import numpy as np

f32 = np.float32

# rr_wbf_plan's layout (include/rrnet_hip.h)
PLAN_INTS = 32
P_LAUNCHES, P_NEEDS_WS, P_ONE_WAVE, P_SHORT, P_LDS_MAX, P_MAX_SEG, P_WS_GRID = 0, 1, 2, 3, 4, 5, 6
P_L0, P_LSTRIDE = 8, 7
L_T, L_LDS, L_CAP, L_LO, L_HI, L_WS, L_GRID = range(7)


def iou_against(F, r, dtype=f32):
    """IoU of the fused boxes F [nc,4] against row r [4]: every operation on its own in `dtype`."""
    F = F.astype(dtype)
    r = r.astype(dtype)
    iw = np.minimum(F[:, 2], r[2]) - np.maximum(F[:, 0], r[0])
    ih = np.minimum(F[:, 3], r[3]) - np.maximum(F[:, 1], r[1])
    ok = (iw > 0) & (ih > 0)
    inter = iw * ih
    u = ((F[:, 2] - F[:, 0]) * (F[:, 3] - F[:, 1]) + (r[2] - r[0]) * (r[3] - r[1])) - inter
    ok &= u > 0
    out = np.zeros(F.shape[0], dtype)
    out[ok] = inter[ok] / u[ok]
    return out


def wbf_segment(rows, iou_thr, conf_type, weight_sum, dtype=f32):
    """One segment.  rows [n,6] float32 -> (out [nc,6] float32, members int32 [nc], trace), trace[j] = (cluster the row
    went to, joined?, the deciding IoU or None with no cluster yet, the runner-up IoU or None)."""
    rows = np.ascontiguousarray(rows, f32)
    n = rows.shape[0]
    thr = dtype(f32(iou_thr))
    F = np.zeros((max(n, 1), 4), f32)
    acc, S, cnt, mx, cls = [], [], [], [], []
    trace = []
    for j in range(n):
        r = rows[j]
        score = float(r[4])
        nc = len(S)
        best, second, k = None, None, -1
        if nc:
            iou = iou_against(F[:nc], r[:4], dtype)
            k = int(np.argmax(iou))                       # the first of equal maxima
            best = iou[k]
            if nc > 1:
                second = np.delete(iou, k).max()
        if nc and best > thr:
            for q in range(4):
                acc[k][q] += score * float(r[q])
            S[k] += score
            cnt[k] += 1
            mx[k] = max(mx[k], r[4])
            for q in range(4):
                F[k, q] = f32(acc[k][q] / S[k])
            trace.append((k, True, best, second))
        else:
            F[nc] = r[:4]
            acc.append([score * float(r[q]) for q in range(4)])
            S.append(score)
            cnt.append(1)
            mx.append(r[4])
            cls.append(r[5])
            trace.append((nc, False, best, second))
    nc = len(S)
    out = np.zeros((nc, 6), f32)
    W = float(weight_sum)
    for c in range(nc):
        base = float(mx[c]) if conf_type == 1 else S[c] / cnt[c]
        out[c, :4] = F[c]
        out[c, 4] = f32(base * min(float(cnt[c]), W) / W)
        out[c, 5] = cls[c]
    return out, np.array(cnt, np.int32).reshape(nc), trace


def wbf_segments(rows, seg_off, seg_len, iou_thr, conf_type, weight_sum):
    """All segments -> [(out, members)] per segment."""
    res = []
    for s in range(len(seg_off) - 1):
        n = int(seg_len[s]) if seg_len is not None else int(seg_off[s + 1] - seg_off[s])
        o, m, _ = wbf_segment(rows[seg_off[s]:seg_off[s] + n], iou_thr, conf_type, weight_sum)
        res.append((o, m))
    return res


def gen_rows(n, seed, dense=False, cls=3.0):
    """n score-descending rows: quarter-pixel boxes jittered around shared centres (three rows per centre on average; `dense`:
    two centres, small jitter, so that one cluster collects more than a hundred rows)."""
    rng = np.random.default_rng(seed)
    if n == 0:
        return np.zeros((0, 6), f32)
    ncent = 2 if dense else max(1, n // 3)
    side = 400.0 if dense else 90.0 * np.sqrt(ncent) + 60.0
    wh = rng.integers(80, 240, (ncent, 2)) * 0.25                 # 20 .. 60 px
    cxy = rng.uniform(0.0, side, (ncent, 2))
    if dense:
        cxy = np.array([[50.0, 50.0], [300.0, 300.0]])
    which = rng.integers(0, ncent, n)
    amp = 0.04 if dense else 0.17
    j = rng.uniform(-amp, amp, (n, 4)) * np.concatenate([wh[which], wh[which]], 1)
    x1y1 = cxy[which] - 0.5 * wh[which]
    box = np.concatenate([x1y1, x1y1 + wh[which]], 1) + j
    box = np.round(box * 4.0) / 4.0
    score = np.sort(rng.uniform(0.05, 1.0, n))[::-1]
    rows = np.concatenate([box, score[:, None], np.full((n, 1), cls)], 1).astype(f32)
    assert (rows[:, 2] > rows[:, 0]).all() and (rows[:, 3] > rows[:, 1]).all()
    return rows


def _planted(rows5):
    a = np.array(rows5, np.float64)
    return np.concatenate([a, np.full((a.shape[0], 1), 1.0)], 1).astype(f32)


PLANTED1 = _planted([[0, 0, 2, 1, .9], [0, 0, 1, 1, .8]])
PLANTED2 = _planted([[0, 0, 2, 2, .9], [2, 0, 4, 2, .8], [1, 0, 3, 2, .7]])
PLANTED3 = _planted([[0, 0, 10, 10, .9], [3, 0, 13, 10, .8], [6, 0, 16, 10, .7]])
ZERO_AREA = _planted([[0, 0, 10, 10, .9], [5, 5, 5, 9, .8], [5, 5, 5, 9, .7], [1, 0, 10, 10, .6]])
CONF = _planted([[0, 0, 10, 10, .9], [0, 0, 10, 10.25, .5], [0, 0.25, 10, 10, .4], [0, 0, 10.25, 10, .3],
                 [40, 40, 50, 50, .8], [40, 40, 50, 50.25, .6], [80, 80, 90, 90, .7]])      # clusters of 4, 2, 1 rows

# (name, [segment rows], gap rows behind every segment (seg_len is then handed on), iou_thr, conf_type, weight_sum,
#  exact: planted ties / threshold hits, exempt from the float64 margins, random: joins and new clusters both required)
ROWS = [
    ("planted1", [PLANTED1], 0, 0.5, 0, 2.0, True, False),
    ("planted2", [PLANTED2], 0, 0.3, 0, 3.0, True, False),
    ("planted3", [PLANTED3], 0, 0.3, 0, 3.0, True, False),
    ("zero_area", [ZERO_AREA], 0, 0.5, 0, 2.0, True, False),
    ("conf_max", [CONF], 0, 0.55, 1, 3.0, True, False),
    ("conf_avg_below_and_above", [CONF], 0, 0.55, 0, 3.0, True, False),
    ("thr_one", [gen_rows(70, 11)], 0, 1.0, 0, 1.0, True, False),
    ("thr_above_one", [gen_rows(9, 12)], 0, 1.5, 1, 1.0, True, False),
    ("wave", [gen_rows(n, 20 + n) for n in (0, 1, 2, 63, 0, 64)], 0, 0.55, 0, 3.0, False, True),
    ("short", [gen_rows(n, 30 + n) for n in (65, 0, 64, 150)], 0, 0.55, 0, 3.0, False, True),
    ("short_ragged", [gen_rows(n, 40 + n) for n in (65, 0, 33, 256)], 5, 0.55, 1, 2.0, False, True),
    ("split", [gen_rows(n, 52 + n) for n in (257, 0, 40, 200, 1025)], 0, 0.55, 0, 3.0, False, True),
    ("split_ragged", [gen_rows(n, 60 + n) for n in (300, 2, 0, 257)], 3, 0.4, 0, 4.0, False, True),
    ("long", [gen_rows(4096, 71), gen_rows(0, 0), gen_rows(300, 72, dense=True), gen_rows(30, 73), gen_rows(150, 75),
              gen_rows(1025, 74)], 0, 0.55, 0, 3.0, False, True),
]


def layout(segs, gap):
    """-> rows [R,6] (gap rows are filled with a value the kernel must never read as a row: NaN), seg_off, seg_len or None."""
    parts, off, lens = [], [0], []
    for s in segs:
        parts.append(s)
        if gap:
            parts.append(np.full((gap, 6), np.nan, f32))
        off.append(off[-1] + s.shape[0] + gap)
        lens.append(s.shape[0])
    rows = np.concatenate(parts, 0) if parts else np.zeros((0, 6), f32)
    return (np.ascontiguousarray(rows, f32), np.array(off, np.int32), np.array(lens, np.int32) if gap else None)


def bound_of(segs):
    return max(s.shape[0] for s in segs)


def body_of(v, n):
    """The kernel body that runs a segment of n rows in a call planned as v (rr_wbf_plan's ints)."""
    for i in range(v[P_LAUNCHES]):
        l = v[P_L0 + i * P_LSTRIDE:P_L0 + (i + 1) * P_LSTRIDE]
        if l[L_LO] < n <= l[L_HI]:
            where = "launch%d/%d" % (i + 1, v[P_LAUNCHES])
            if l[L_WS]:
                return where + ":t%d/ws" % l[L_T]
            if l[L_T] > 64 and n <= v[P_ONE_WAVE]:
                return where + ":t%d/wave0" % l[L_T]
            return where + ":t%d" % l[L_T]
    raise AssertionError("no launch takes a segment of %d rows" % n)


# every body a call can reach (wbf_plan.h): the table must sit on each
BODIES = {"launch1/1:t64", "launch1/1:t256", "launch1/1:t256/wave0",
          "launch1/2:t256", "launch1/2:t256/wave0", "launch2/2:t512",
          "launch1/3:t256", "launch1/3:t256/wave0", "launch2/3:t512", "launch3/3:t512/ws"}


# ---- the fuse_rows pipeline (rrnet_amd/ensemble.py), restated per frame
def fuse_frame(dets, weights, iou_thr, skip_score, conf_type, max_det):
    """dets: one [n,>=6] xywh,score,cls array per run -> float32 [m,6]."""
    parts = []
    for d, w in zip(dets, weights):
        d = np.asarray(d)[:, :6].astype(f32)
        d[:, 4] = d[:, 4] * f32(w)
        parts.append(d)
    a = np.concatenate(parts, 0)
    a = a[a[:, 4] > f32(skip_score)]
    a[:, 2] = a[:, 0] + a[:, 2]
    a[:, 3] = a[:, 1] + a[:, 3]
    a = a[np.argsort(-a[:, 4], kind="stable")]
    outs = []
    for c in np.unique(a[:, 5].astype(np.int64)):
        seg = a[a[:, 5].astype(np.int64) == c]
        outs.append(wbf_segment(seg, iou_thr, conf_type, float(sum(weights)))[0])
    o = np.concatenate(outs, 0) if outs else np.zeros((0, 6), f32)
    o[:, 2] = o[:, 2] - o[:, 0]
    o[:, 3] = o[:, 3] - o[:, 1]
    o = o[np.argsort(-o[:, 4], kind="stable")]
    return o[:max_det]


def gen_runs(nframes, seed, nruns=3, nobj=40):
    """Three runs over the frames: jittered copies of common boxes, some dropped, some spurious; xywh,score,cls, file order
    (not sorted)."""
    rng = np.random.default_rng(seed)
    sets = [[] for _ in range(nruns)]
    for f in range(nframes):
        k = nobj + 7 * f
        xy = np.round(rng.uniform(0, 900, (k, 2)) * 4) / 4
        wh = rng.integers(48, 320, (k, 2)) * 0.25
        cls = rng.integers(1, 6, k).astype(np.float64)
        for m in range(nruns):
            keep = rng.uniform(size=k) > 0.2
            j = np.round(rng.uniform(-0.08, 0.08, (k, 4)) * np.concatenate([wh, wh], 1) * 4) / 4
            box = np.concatenate([xy, wh], 1) + j
            sc = rng.uniform(0.02, 0.99, k)
            d = np.concatenate([box, sc[:, None], cls[:, None]], 1)[keep]
            ns = int(rng.integers(3, 9))
            sp = np.concatenate([np.round(rng.uniform(0, 900, (ns, 2)) * 4) / 4, rng.integers(48, 320, (ns, 2)) * 0.25,
                                 rng.uniform(0.02, 0.4, (ns, 1)), rng.integers(1, 6, (ns, 1)).astype(np.float64)], 1)
            d = np.concatenate([d, sp], 0)
            d = d[rng.permutation(d.shape[0])]
            d[:, 4] = np.round(d[:, 4] * 1e4) / 1e4          # what a result file's %.4f keeps
            sets[m].append(np.concatenate([d, -np.ones((d.shape[0], 2))], 1))
    return sets
