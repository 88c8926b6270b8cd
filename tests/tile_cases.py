"""Tiled inference: the numpy float32 restatement of rr_merge_tiles, written from the contract in include/rrnet_hip.h and
DESIGN 16.2 (not from the kernel), plan_tiles' expected lists, and the case tables the host and GPU tests share."""
import numpy as np

F32 = np.float32

# plan_tiles(h, w, tile, overlap) -> origins, row-major with y outer
PLAN_5x7_T4_O1 = [(0, 0), (0, 3), (1, 0), (1, 3)]
PLAN_765x1360_T512_O128 = [(0, 0), (0, 384), (0, 768), (0, 848), (253, 0), (253, 384), (253, 768), (253, 848)]
PLAN_SHAPES = [(5, 7, 4, 1), (765, 1360, 512, 128), (37, 53, 16, 0), (37, 53, 16, 15), (16, 16, 16, 3), (100, 17, 17, 5),
               (1080, 1920, 512, 128), (1500, 2000, 512, 200), (33, 64, (32, 16), 4)]


def merge_tiles(rows, count_in, tiles, sizes, tile, in_size, div, margin):
    """rows [T,k_in,6] float32 (x, y, w, h, score, cls in the model's input coordinates), count_in [T], tiles = T rows
    (frame, y0, x0) sorted by frame, sizes = (H, W) per frame, tile = (th, tw), in_size = (oh, ow).
    -> (kept rows in frame coordinates per frame, list of [n_f,6] float32; the leave mask per tile, list of bool arrays).
    Per frame its tiles in table order, of each the first min(max(count_in[t], 0), k_in) rows in row order.  float32, every
    operation rounded on its own."""
    th, tw = tile
    oh, ow = in_size
    div, margin = F32(div), F32(margin)
    rows = np.asarray(rows, dtype=F32)
    kept, masks = [[] for _ in sizes], []
    for t, (f, y0, x0) in enumerate(tiles):
        fh, fw = sizes[f]
        n = min(max(int(count_in[t]), 0), rows.shape[1])
        r = rows[t, :n]
        x, y, w, h = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
        leave = np.zeros(n, dtype=bool)
        if margin > 0:
            with np.errstate(invalid="ignore"):                    # a NaN compares false: the row stays
                if x0 > 0:
                    leave |= x < margin
                if y0 > 0:
                    leave |= y < margin
                if x0 + tw < fw:
                    leave |= (x + w) > (F32(ow) - margin)
                if y0 + th < fh:
                    leave |= (y + h) > (F32(oh) - margin)
        moved = r.copy()
        moved[:, 0] = x / div + F32(x0)
        moved[:, 1] = y / div + F32(y0)
        moved[:, 2] = w / div
        moved[:, 3] = h / div
        kept[f].append(moved[~leave])
        masks.append(leave)
    return [np.concatenate(k).reshape(-1, 6) if k else np.zeros((0, 6), F32) for k in kept], masks


def into_buffer(kept, k, fill):
    """The kept rows of merge_tiles as rr_merge_tiles leaves them: merged [F,k,6] holding `fill` where nothing is written,
    count [F] = the true number of kept rows, also above k."""
    merged = np.full((len(kept), k, 6), fill, dtype=F32)
    for f, rows in enumerate(kept):
        merged[f, :min(len(rows), k)] = rows[:k]
    return merged, np.array([len(rows) for rows in kept], dtype=np.int32)


# ---- the merge cases: three frames with 1, 4 and 6 tiles of 32x32; every tile of the middle frame is empty ----
MERGE_TILE = (32, 32)
MERGE_SIZES = [(32, 32), (48, 48), (48, 64)]
MERGE_TILES = ([(0, 0, 0)] + [(1, y, x) for y in (0, 16) for x in (0, 16)] + [(2, y, x) for y in (0, 16) for x in (0, 16, 32)])
MERGE_K_IN = 257
# per-tile counts; 262 = k_in + 5 is clamped to 257.  Layout "a": frame 2 holds 1 + 64 + 257 = 322 rows at margin 0
MERGE_COUNTS = {"a": [63] + [0] * 4 + [1, 64, 0, 0, MERGE_K_IN + 5, 0],
                "b": [65] + [0] * 4 + [MERGE_K_IN, 0, 1, 63, 64, 0]}
MERGE_DIVS = [1.0, 1.5, 2.0, 0.7]
MERGE_MARGINS = [0.0, 2.25]
PLANTED = ("left_at", "left_in", "top_at", "top_in", "right_at", "right_in", "bottom_at", "bottom_in", "nan")


def merge_in_size(div):
    return int(np.floor(MERGE_TILE[0] * div)), int(np.floor(MERGE_TILE[1] * div))


def merge_rows(div, margin, seed=0):
    """rows [T,k_in,6] on a quarter-pixel grid for the input size of `div`.  The leading rows of every tile are planted, in
    PLANTED's order: on each of the four sides a box exactly at the margin (`_at`: stays wherever it is) and one a quarter
    pixel inside it (`_in`: leaves iff that side is interior), then a row whose x is NaN (stays).  The planted boxes sit in the
    middle of the other axis, clear of its margins.  The rest is random, a good part of it within the margin of a side."""
    oh, ow = merge_in_size(div)
    g = np.random.default_rng(seed + int(div * 100))
    t = len(MERGE_TILES)
    rows = np.zeros((t, MERGE_K_IN, 6), dtype=F32)
    wh = np.round(g.uniform(1, 6, (t, MERGE_K_IN, 2)) * 4) / 4
    rows[:, :, 2:4] = wh
    rows[:, :, 0] = np.round(g.uniform(0, ow - 6, (t, MERGE_K_IN)) * 4) / 4
    rows[:, :, 1] = np.round(g.uniform(0, oh - 6, (t, MERGE_K_IN)) * 4) / 4
    rows[:, :, 4] = np.round(g.uniform(0.1, 1.0, (t, MERGE_K_IN)), 3)
    rows[:, :, 5] = g.integers(1, 11, (t, MERGE_K_IN))
    m = max(float(margin), 2.25)                                   # planted against 2.25 also when the test is off
    cx, cy = np.floor(ow / 2) - 1, np.floor(oh / 2) - 1            # a 2x2 box there is clear of every margin (ow >= 22)
    planted = {"left_at": (m, cy, 2, 2), "left_in": (m - 0.25, cy, 2, 2), "top_at": (cx, m, 2, 2), "top_in": (cx, m - 0.25, 2, 2),
               "right_at": (ow - m - 2, cy, 2, 2), "right_in": (ow - m - 1.75, cy, 2, 2),
               "bottom_at": (cx, oh - m - 2, 2, 2), "bottom_in": (cx, oh - m - 1.75, 2, 2), "nan": (np.nan, cy, 2, 2)}
    for i, name in enumerate(PLANTED):
        rows[:, i, :4] = planted[name]
    return rows
