"""Soft-NMS route cases: the table of (nseg, declared bound, segment lengths) rows that reaches every answer of the launch plan
(rrnet_amd/csrc/softnms_plan.h), the seeded input recipe, and an instrumented numpy restatement of the reference loop that says
which renumbering / compaction branch every outer step of a segment takes.  Everything here is built on the host;
tests/test_softnms_routes_host.py proves what the table reaches, tests/test_softnms_routes_gpu.py runs it.

The recipe.  A segment is made of
  * clusters: a cluster of size m is one box of 60..120 px plus a jitter of +/-2 px per coordinate; one member scores in `top`
    (default [0.9, 1]), the rest in [0.11, 0.2].  Clusters sit on a band of their own, 400 px apart: selecting the top member
    kills exactly its m - 1 mates (IoU >= (56/64)^2 = 0.77: gaussian weight <= 0.31, linear <= 0.24, hard 0; times 0.2 is below
    the threshold 0.1 of every case) and touches nothing else;
  * background: boxes of 8..60 px, one per 64-px cell of a grid, so they never overlap anything; scores in `bg`;
  * a crowd: boxes of 8..120 px thrown over a small square on a third band, the uniform-box recipe of tests/test_softnms_gpu.py,
    for decays without deaths and steps with a few deaths;
  * ties: all scores optionally rounded to multiples of 1/q (16 or 32);
  * layout: the rows are shuffled; `tail` then puts the mates of the best-scoring cluster into the last rows, so that step 0
    kills exactly the tail (the dead include the last position, nothing moves); `tail="front"` puts that cluster into the first
    rows and the second-best box, untied, into the last: step 0 pre-selects a box that the compaction then moves.
`lane_tie` segments are laid out by hand instead, see lane_tie_segment."""
import math
import zlib

import numpy as np

F = np.float32
SIGMA, NT, THR = 0.5, 0.3, 0.1          # every case: (float)0.5 gaussian width, Nt for the linear / hard methods, death threshold

# indices into the answer of rr_soft_nms_plan (include/rrnet_hip.h)
PLAN_INTS = 18
(P_LAUNCHES, P_KERNEL, P_T, P_NB, P_LDS, P_CAP, P_RAISE, P_T0, P_LDS0, P_NEEDS_WS, P_USES_WS,
 P_REG_LIST, P_REG_SHORT, P_ONE_WAVE, P_MID_SEG, P_LDS_MAX, P_MASK_BOXES) = range(17)

# every label the plan can produce
LABELS = ("reg<256,1>", "reg<512,3>", "reg<1024,3>", "reg<512,12>", "reg<512,18>",
          "lds<256>", "lds<256>+<256>", "lds<256>+<1024>", "lds<1024>/ws")


def plan_label(v):
    """The label of an answer of rr_soft_nms_plan."""
    if v[P_KERNEL] == 0:
        return "reg<%d,%d>" % (v[P_T], v[P_NB])
    s = "lds<%d>" % v[P_T] if v[P_LAUNCHES] == 1 else "lds<%d>+<%d>" % (v[P_T0], v[P_T])
    return s + ("/ws" if v[P_USES_WS] else "")


# ---------------------------------------------------------------------------------------------------------------------
# the recipe
def seg(n, clusters=(), q=0, crowd=0, tail=False, top=(0.9, 1.0), bg=(0.25, 0.85), lane_tie=None):
    return dict(n=n, clusters=tuple(clusters), q=q, crowd=crowd, tail=tail, top=top, bg=bg, lane_tie=lane_tie)


def kill_all(n, m):
    """n - m background boxes that all outscore the one cluster of m: the last death step kills everything left."""
    return seg(n, clusters=(m,), top=(0.5, 0.6), bg=(0.7, 1.0))


def _seed(spec, salt):
    return zlib.crc32(repr((sorted(spec.items()), salt)).encode())


def _cluster(rng, m, k, top):
    w, h = rng.uniform(60, 120, 2)
    x, y = 400.0 * k + 10.0, -1000.0
    base = np.array([x, y, x + w, y + h])
    b = base[None, :] + rng.uniform(-2, 2, (m, 4))
    s = rng.uniform(0.11, 0.2, m)
    s[0] = rng.uniform(*top)
    return np.concatenate([b, s[:, None]], 1)


def _background(rng, m, bg):
    cell = rng.permutation(128 * 128)[:m]
    wh = rng.uniform(8, 60, (m, 2))
    xy = np.stack([cell % 128, cell // 128], 1) * 64.0 + rng.uniform(0, 1, (m, 2)) * (62.0 - wh)
    return np.concatenate([xy, xy + wh, rng.uniform(*bg, (m, 1))], 1)


def _crowd(rng, m):
    span = 40.0 * math.sqrt(max(m, 1)) + 60.0
    xy = rng.uniform(0, span, (m, 2)) + np.array([0.0, -6000.0])
    wh = rng.uniform(8, 120, (m, 2))
    return np.concatenate([xy, xy + wh, rng.uniform(0.01, 1, (m, 1))], 1)


def lane_tie_segment(n, T, deaths, rng):
    """Two boxes A (row 2) and B (row 2 + T) — the same lane of a register kernel with T threads — share the second-best
    score, and nobody else has it.  Row 0 is a cluster's top, its `deaths` mates sit in row 1 and in the last rows, with
    n - deaths <= 2 + T: step 0 kills them, B is the right-most survivor above the new N and moves into the hole at position 1,
    in FRONT of A.  The reference then selects B (the lowest position among equal maxima), not A."""
    assert n == T + 2 + deaths
    rows = _background(rng, n, (0.25, 0.75))
    cl = _cluster(rng, deaths + 1, 0, (0.95, 1.0))
    rows[0] = cl[0]
    rows[1] = cl[1]
    rows[n - (deaths - 1):] = cl[2:]
    rows[2, 4] = rows[2 + T, 4] = 0.8
    return rows


def make_segment(spec, salt=0, stride=5):
    """float32 [n, stride] rows of one segment; columns 5.. hold a per-row pattern that must come back untouched."""
    rng = np.random.default_rng(_seed(spec, salt))
    n = spec["n"]
    if spec["lane_tie"]:
        rows = lane_tie_segment(n, *spec["lane_tie"], rng)
    else:
        parts = [_cluster(rng, m, k, spec["top"]) for k, m in enumerate(spec["clusters"])]
        nbg = n - sum(spec["clusters"]) - spec["crowd"]
        assert nbg >= 0, spec
        parts += [_crowd(rng, spec["crowd"]), _background(rng, nbg, spec["bg"])]
        rows = np.concatenate(parts, 0)
        if spec["q"]:
            rows[:, 4] = np.maximum(np.round(rows[:, 4] * spec["q"]), 1) / spec["q"]
        order = rng.permutation(n)
        if spec["tail"]:
            tops = [sum(spec["clusters"][:k]) for k in range(len(spec["clusters"]))]
            best = max(range(len(tops)), key=lambda k: rows[tops[k], 4])
            mates = np.arange(tops[best] + 1, tops[best] + spec["clusters"][best])
            rows[tops[best], 4] = 1.0625                     # above every other score, a multiple of 1/16: step 0 selects it
            rest = order[~np.isin(order, mates)]
            if spec["tail"] == "front":
                rest = rest[rest != tops[best]]
                rows[rest[-1], 4] = 1.03125                  # the pre-selected next box, untied, in the last row
                order = np.concatenate([[tops[best]], mates, rest])
            else:
                order = np.concatenate([rest, mates])
        rows = rows[order]
    out = np.empty((n, stride), F)
    out[:, :5] = rows.astype(F)
    for c in range(5, stride):
        out[:, c] = (np.arange(n) * 7 + c * 1000 + salt % 97).astype(F)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the instrumented restatement of oracle/soft_nms.c
def soft_nms_traced(boxes, sigma, Nt, thr, method):
    """The reference loop on a copy of `boxes` (float32 [n, >= 5]), step by step in numpy: float32 values, double `+ 1.0`,
    (float)exp((double)q) — the arithmetic of oracle/soft_nms.c.  Returns (rows, N', steps); steps holds one dict per outer
    step i < N:
      N       boxes in play when the step began          D      deaths of the step
      nmove   dead positions below the new N (rows the compaction moves)      top    the highest dead position (-1: none)
      left    survivors in (i, N): 0 means the step killed everything left (no pre-selected next box)
      tied    the pre-selected next box — the best survivor after the decay, lowest position among equal scores — shares its score
      moved   that box sat at or above the new N: the compaction moves it
    Raises ZeroDivisionError where the reference does."""
    b = np.array(boxes, dtype=F, order="C", copy=True)
    c = [np.ascontiguousarray(b[:, k]) for k in range(5)]
    x1, y1, x2, y2, s = c
    sigma, Nt, thr = F(sigma), F(Nt), F(thr)
    one = np.float64(1.0)
    N = b.shape[0]
    steps = []
    i = 0
    while i < N:
        mp = i + int(np.argmax(s[i:N]))                      # first maximum wins
        if mp != i:
            for a in c:
                a[i], a[mp] = a[mp], a[i]
        tx1, ty1, tx2, ty2 = x1[i], y1[i], x2[i], y2[i]
        lo = i + 1
        iw = ((np.minimum(tx2, x2[lo:N]) - np.maximum(tx1, x1[lo:N])).astype(np.float64) + one).astype(F)
        ih = ((np.minimum(ty2, y2[lo:N]) - np.maximum(ty1, y1[lo:N])).astype(np.float64) + one).astype(F)
        hit = lo + np.nonzero((iw > 0) & (ih > 0))[0]
        dead = np.zeros(0, np.int64)
        if hit.size:
            iw, ih = iw[hit - lo], ih[hit - lo]
            area = (((x2[hit] - x1[hit]).astype(np.float64) + one) * ((y2[hit] - y1[hit]).astype(np.float64) + one)).astype(F)
            tarea = (np.float64(tx2 - tx1) + one) * (np.float64(ty2 - ty1) + one)
            inter = iw * ih
            ua = ((tarea + area.astype(np.float64)) - inter.astype(np.float64)).astype(F)
            if np.any(ua == 0):
                raise ZeroDivisionError("float division")
            ov = inter / ua
            if method == 1:
                w = np.where(ov > Nt, (one - ov.astype(np.float64)).astype(F), F(1))
            elif method == 2:
                if sigma == 0:
                    raise ZeroDivisionError("float division")
                qq = (-(ov * ov)) / sigma
                w = np.array([math.exp(v) for v in qq.astype(np.float64)], np.float64).astype(F)
            else:
                w = np.where(ov > Nt, F(0), F(1))
            ns = (w * s[hit]).astype(F)
            s[hit] = ns
            dead = hit[ns < thr]
        D = int(dead.size)
        alive = np.ones(N - lo, bool)
        alive[dead - lo] = False
        st = dict(i=i, N=N, D=D, nmove=0, top=int(dead[-1]) if D else -1, left=int(alive.sum()), tied=False, moved=False)
        if st["left"]:
            sv = np.where(alive, s[lo:N], -np.inf)
            best = int(np.argmax(sv))
            st["tied"] = int(np.count_nonzero(sv == sv[best])) > 1
            st["moved"] = lo + best >= N - D
        if D:
            newN = N - D
            holes = dead[dead < newN]
            movers = (lo + np.nonzero(alive)[0])
            movers = movers[movers >= newN][::-1]
            assert holes.size == movers.size
            for a in c:
                a[holes] = a[movers]
            st["nmove"] = int(holes.size)
            N = newN
        steps.append(st)
        i += 1
    for k in range(5):
        b[:, k] = c[k]
    return b, N, steps


# ---------------------------------------------------------------------------------------------------------------------
# the table
def _mix(n, q=0, tail=False, big=0):
    """A segment of n boxes with as many of the 66 / 65-clusters (65 / 64 deaths: one more / exactly what the register kernel's
    list holds) as fit into 70 % of it behind an optional big cluster, a crowd of 12 %, the rest background."""
    cl = [big] if big else []
    for m in (66, 66, 65, 66, 65, 65, 66, 66, 65, 66, 40, 12, 5, 3):
        if sum(cl) + m <= 0.7 * n:
            cl.append(m)
    return seg(n, cl, q=q, crowd=int(0.12 * n), tail=tail)


# step 0 moves its untied pre-selection, once behind a list step (49 deaths) and once behind a mask step (99)
FRONT = [seg(700, (50,), crowd=30, tail="front"), seg(900, (100,), crowd=30, tail="front")]


def _lane_ties(T):
    """The in-lane tie behind a mask step (86 deaths) and behind a list step (56 deaths) of a register kernel with T threads."""
    return [seg(T + 2 + 86, lane_tie=(T, 86)), seg(T + 2 + 56, lane_tie=(T, 56))]


# the segments of the <256, 1> row; every register row with T > 256 carries them too: there they run the short-segment path
SHORT = [seg(0), seg(1), seg(2), _mix(63), kill_all(64, 30), _mix(65), _mix(255), _mix(256, tail=True),
         seg(100, (100,)), _mix(256, q=16), _mix(250, q=32), seg(256, (66, 65, 66, 40), crowd=10), kill_all(200, 65)]

FILLER = "filler"     # a row's segment list ends with this: segments of 0..3 boxes up to nseg

# (name, label, nseg, declared bound, method, segments).  Every row runs twice: through rr_soft_nms_segments (segments back to
# back) and through rr_soft_nms_ragged (explicit lengths, gaps between the segments).
ROWS = [
    ("reg256x1", "reg<256,1>", len(SHORT), 256, 2, SHORT),
    ("reg512x3", "reg<512,3>", 0, 1536, 1,
     [seg(256, (66, 66, 65)), _mix(257), _mix(512, q=16), seg(513, (513,)), kill_all(1025, 40), _mix(1536, big=300),
      _mix(700), _mix(900, q=32, tail=True)] + _lane_ties(512) + FRONT + SHORT),
    ("reg1024x3", "reg<1024,3>", 0, 3072, 0,
     [_mix(256, q=32), _mix(257), _mix(1537, q=16), kill_all(2049, 50), _mix(3072, big=900), seg(1600, (1600,)),
      _mix(1700, tail=True)] + _lane_ties(1024) + FRONT + SHORT),
    ("reg512x12", "reg<512,12>", 0, 6144, 2,
     [_mix(200), _mix(3073, q=16), _mix(6144, big=700, tail=True), seg(400, (400,)), kill_all(600, 60), _mix(800)]
     + _lane_ties(512) + FRONT + SHORT),
    ("reg512x18", "reg<512,18>", 0, 9216, 2,
     [_mix(6145, q=32), _mix(9216, big=500, tail=True), seg(300, (300,)), kill_all(500, 33), _mix(1000), _mix(640, q=16)]
     + _lane_ties(512) + FRONT),
    ("reg512x18_many", "reg<512,18>", 520, 9216, 1,
     [_mix(6145, q=32), _mix(9216, big=500, tail=True), seg(300, (300,)), kill_all(500, 33), _mix(1000), _mix(640, q=16)]
     + _lane_ties(512) + FRONT + [FILLER]),
    ("ws_one", "lds<1024>/ws", 1, 9217, 2, [_mix(9217, big=1100, tail=True)]),
    ("ws_many", "lds<1024>/ws", 515, 9217, 0,
     [_mix(9217, big=1100, tail=True), _mix(5000, q=16, big=1030), _mix(150, tail=True), FILLER]),
    ("lds_single", "lds<256>", 530, 512, 1,
     [seg(0), seg(1), _mix(64), _mix(65, tail=True), _mix(192, tail=True), _mix(193, tail=True), _mix(256, q=16),
      seg(512, (300, 66, 65), crowd=40, tail=True), seg(130, (100,), crowd=20), FILLER]),
    ("lds_split256", "lds<256>+<256>", 540, 2560, 2,
     [_mix(192, q=16), _mix(193), _mix(512, tail=True), _mix(513, tail=True), _mix(1500, big=280, q=32), _mix(2560, big=600),
      seg(150, (80, 30), crowd=20, tail=True), FILLER]),
    ("lds_split1024", "lds<256>+<1024>", 525, 6000, 0,
     [_mix(512, q=32), _mix(513), _mix(2561, big=1100, tail=True), _mix(6000, big=1200, q=16), seg(100, (70,), tail=True),
      FILLER]),
]


def cases():
    """[(id, row, ragged)]"""
    return [("%s-%s" % (r[0], "ragged" if rg else "segments"), r, rg) for r in ROWS for rg in (False, True)]


_SEGMENTS = {}


def row_segments(row, stride=5):
    """The segments of a row (cached: rows and their two layouts share them), filler expanded: [(spec, rows)]."""
    name, _, nseg, _, _, specs = row
    key = (name, stride)
    if key not in _SEGMENTS:
        out = []
        for k, sp in enumerate(specs):
            if sp == FILLER:
                rng = np.random.default_rng(zlib.crc32(name.encode()))
                while len(out) < nseg:
                    n = int(rng.integers(0, 4))
                    out.append((seg(n, crowd=n), make_segment(seg(n, crowd=n), len(out), stride)))
            else:
                out.append((sp, make_segment(sp, k, stride)))
        assert nseg in (0, len(out)), (name, nseg, len(out))
        _SEGMENTS[key] = out
    return _SEGMENTS[key]


def row_nseg(row):
    return row[2] or len(row[5])


def row_stride(row):
    """5, 6 or 7 floats per row, in turn down the table."""
    return 5 + [r[0] for r in ROWS].index(row[0]) % 3


NAN_ROW = np.uint32(0x7fc0dead)          # what the gap rows of a ragged layout and the guard bands are filled with


def layout(segs, ragged, seed=0):
    """The device image of a list of segments (float32 [n, stride] each): (flat float32 [guard + rows + guard, stride], guard
    rows, seg_off [nseg + 1], seg_len [nseg] or None) — seg_off counts from the first row behind the front guard.  Ragged: gaps
    of 1..5 rows behind the segments (every third has none).  Gaps and guards hold NAN_ROW."""
    stride = segs[0].shape[1]
    rng = np.random.default_rng(seed)
    gaps = [(0 if (k % 3 == 0 or not ragged) else int(rng.integers(1, 6))) for k in range(len(segs))]
    lens = np.array([r.shape[0] for r in segs], np.int32)
    starts = np.concatenate([[0], np.cumsum(lens + np.array(gaps, np.int32))]).astype(np.int32)
    guard = 16
    flat = np.full((guard + int(starts[-1]) + guard, stride), NAN_ROW, np.uint32).view(F)
    for r, o in zip(segs, starts[:-1]):
        flat[guard + o:guard + o + r.shape[0]] = r
    return flat, guard, starts, lens if ragged else None


def fillers(count, stride, seed):
    """`count` segments of 0..3 crowded boxes."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = int(rng.integers(0, 4))
        out.append(make_segment(seg(n, crowd=n), seed + k, stride))
    return out


def bench_shape_segments(nseg=520, bound=1500, stride=6, seed=55):
    """The benchmark's config-5 batch in small: (frame, class) segments of around 150 uniformly thrown boxes, four of 1400..bound,
    six columns (the class rides along)."""
    rng = np.random.default_rng(seed)
    lens = np.clip(rng.normal(150, 40, nseg), 0, 400).astype(int)
    lens[rng.permutation(nseg)[:4]] = [1400, 1437, 1499, bound]
    out = []
    for n in lens:
        span = 300.0 if n < 1000 else 700.0
        xy = rng.uniform(0, span, (n, 2))
        wh = rng.uniform(8, 120, (n, 2))
        cols = [xy, xy + wh, rng.uniform(0.01, 1, (n, 1)), rng.integers(0, 10, (n, 1)).astype(np.float64)]
        out.append(np.concatenate(cols, 1).astype(F))
    return out
