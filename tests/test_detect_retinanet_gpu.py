"""GPU: RetinaNet detection on raw frames — rr_retina_decode_frames against rr_retina_decode (bits) and against float64,
rr_nms_frames / rr_pack_frames against the float32 restatement of the reference's hard NMS and against rr_nms_sorted frame
by frame, the whole tail, rr_prepare_frames without a resize, and detect_frames_retinanet / tools/detect.py end to end."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import retina_cases as rc
import test_retina_gpu as base            # the decode inputs, cases and acceptance rule of the per-image kernel's tests
from rrnet_amd import ops

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = ops.RETINA_DECODE_CHUNK
SENTINEL = -7.25e30                        # what a buffer holds where the kernel must not write
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _u32(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


# --------------------------------------------------------------------------------------------------------------------
# decode
# --------------------------------------------------------------------------------------------------------------------
def _both_decodes(logits, loc, anchors, thr, k=None):
    """-> (rows, count) of rr_retina_decode and (rows [B,k,6], count, guard row) of rr_retina_decode_frames writing into a
    buffer of sentinels with one row to spare behind the last frame."""
    b, a, _ = logits.shape
    k = a if k is None else k
    dev = _dev(logits, loc, anchors)
    ref_rows, ref_count = ops.retina_decode(*dev, thr)
    flat = torch.full((b * k + 1, 6), SENTINEL, dtype=torch.float32, device="cuda")
    rows, count = ops.retina_decode_frames(*dev, thr, k=k, rows=flat[:b * k].view(b, k, 6))
    torch.cuda.synchronize()
    return ref_rows.cpu().numpy(), ref_count.cpu().numpy(), rows.cpu().numpy(), count.cpu().numpy(), flat[b * k].cpu().numpy()


def _assert_same_rows(ref_rows, ref_count, rows, count, guard, k):
    sentinel = np.float32(SENTINEL).view(np.uint32)
    assert np.array_equal(count, ref_count)                                    # the true totals, also above k
    for i, n in enumerate(ref_count.tolist()):
        m = min(n, k)
        assert np.array_equal(_u32(rows[i, :m]), _u32(ref_rows[i, :m])), i
        assert (_u32(rows[i, m:]) == sentinel).all(), i                        # between the count and k: untouched
    assert (_u32(guard) == sentinel).all()                                     # behind k of the last frame: untouched


@pytest.mark.parametrize("thr", [0.05, 0.5])
@pytest.mark.parametrize("c", [1, 4, 10, 80])
@pytest.mark.parametrize("a", [1, L - 1, L, L + 1, 3 * L + 7])
def test_decode_frames_equals_decode_bit_for_bit(a, c, thr):
    """Rows and counts as uint32 at the chunk's edges: one anchor, one short of a chunk, a chunk, one into the second, and a
    fourth chunk of seven anchors.  "mixed" inputs: first-maximum ties on every third anchor, nothing within 1e-5 of the
    threshold."""
    logits, loc, anchors = base._decode_inputs(a, c, 5000 + a + 31 * c, "mixed", b=2, thr=thr)
    ref_rows, ref_count, rows, count, guard = _both_decodes(logits, loc, anchors, thr)
    print("\ndecode_frames A=%d C=%d threshold %g: kept %s" % (a, c, thr, count.tolist()))
    _assert_same_rows(ref_rows, ref_count, rows, count, guard, a)


def _special_batch():
    """B = 3, A = 3L+7, C = 10: image 0 keeps some rows and carries NaN / +inf rows on both sides of the first chunk edge and
    in the last, short chunk; image 1 keeps nothing; image 2 keeps every anchor."""
    a = 3 * L + 7
    logits, loc, anchors = base._decode_inputs(a, 10, 77, "batch3", b=3)
    special = {"nan_first": L - 1, "nan_later": L, "nan_all": L + 1, "inf": 2 * L, "nan_all_2": 0, "inf_2": a - 1}
    for kind, r in special.items():
        logits[0, r, :] = -4.0
        if kind.startswith("nan_all"):
            logits[0, r, :] = np.nan
        elif kind == "nan_first":
            logits[0, r, 0], logits[0, r, 4] = np.nan, 6.0
        elif kind == "nan_later":
            logits[0, r, 3], logits[0, r, 5] = np.nan, 6.0
        else:
            logits[0, r, 2] = np.inf
    return logits, loc, anchors, special


def _host_keep(logits, thr):
    """Which anchors stay, decided in float64: a row with a NaN leaves, the others stay when their best probability is above
    the threshold.  Only for inputs with nothing near the threshold."""
    with np.errstate(over="ignore"):
        p = 1.0 / (1.0 + np.exp(-logits.astype(np.float64)))
    nan = np.isnan(p).any(axis=-1)
    top = np.where(nan, 0.0, np.nanmax(np.where(np.isnan(p), -1.0, p), axis=-1))
    assert float(np.abs(top[~nan] - thr).min()) > 1e-5
    return ~nan & (top > thr)


def test_decode_frames_batch_of_three_with_nan_and_inf_rows():
    logits, loc, anchors, special = _special_batch()
    keep = _host_keep(logits, 0.1)
    assert 0 < keep[0].sum() < keep.shape[1] and keep[1].sum() == 0 and keep[2].all()
    for kind, r in special.items():
        assert bool(keep[0, r]) == kind.startswith("inf"), kind
    ref_rows, ref_count, rows, count, guard = _both_decodes(logits, loc, anchors, 0.1)
    assert ref_count.tolist() == keep.sum(axis=1).tolist()
    _assert_same_rows(ref_rows, ref_count, rows, count, guard, keep.shape[1])
    at = int(keep[0, :2 * L].sum())                                            # the +inf row at 2L: probability 1, class 3
    assert rows[0, at, 4] == 1.0 and rows[0, at, 5] == 3.0


def test_decode_frames_with_an_empty_chunk_between_kept_ones():
    """Image 0: chunk 1 keeps nothing between chunks 0 and 2 that do; image 1: chunks 0 and 2 keep nothing, 1 and 3 do."""
    a = 3 * L + 7
    logits, loc, anchors = base._decode_inputs(a, 4, 78, "mixed", b=2)
    low = (-5.0 - np.abs(logits)).astype(np.float32)
    logits[0, L:2 * L] = low[0, L:2 * L]
    logits[1, :L], logits[1, 2 * L:3 * L] = low[1, :L], low[1, 2 * L:3 * L]
    keep = _host_keep(logits, 0.1)
    per_chunk = [[int(keep[i, j * L:(j + 1) * L].sum()) for j in range(4)] for i in range(2)]
    assert per_chunk[0][1] == 0 and per_chunk[0][0] > 0 and per_chunk[0][2] > 0
    assert per_chunk[1][0] == 0 and per_chunk[1][2] == 0 and per_chunk[1][1] > 0 and per_chunk[1][3] > 0
    ref_rows, ref_count, rows, count, guard = _both_decodes(logits, loc, anchors, 0.1)
    _assert_same_rows(ref_rows, ref_count, rows, count, guard, a)


@pytest.mark.parametrize("k", [1, L - 1, L + 3])
def test_decode_frames_with_fewer_rows_than_candidates(k):
    """k below the kept total of images 0 and 2 and above image 1's (none): count is the true total, the first k rows are the
    per-image kernel's, and neither the next frame's block nor the row behind the last frame is written."""
    logits, loc, anchors, _ = _special_batch()
    ref_rows, ref_count, rows, count, guard = _both_decodes(logits, loc, anchors, 0.1, k=k)
    assert ref_count[0] > k and ref_count[1] == 0 and ref_count[2] == 3 * L + 7 > k
    _assert_same_rows(ref_rows, ref_count, rows, count, guard, k)


@pytest.mark.parametrize("a,mode,c,thr", base.DECODE_CASES)
def test_decode_frames_vs_fp64(a, mode, c, thr):
    """The cases of test_retina_decode_vs_fp64 on rr_retina_decode_frames, by its rule: counts, kept anchors and classes equal
    to rc.decode in float64, probabilities and boxes within 4 x the float32 restatement's own error."""
    b = 3 if mode == "batch3" else 2
    args = {} if thr is None else {"thr": thr}
    logits, loc, anchors = base._decode_inputs(a, c, 1000 + a + (0 if c == 10 else 31 * c), mode, b=b, **args)
    rows, count = ops.retina_decode_frames(*_dev(logits, loc, anchors), 0.1 if thr is None else thr)
    rows, count = rows.cpu().numpy(), count.cpu().numpy()
    print("\ndecode_frames A=%d %s C=%d: kept %s" % (a, mode, c, count.tolist()))
    for i in range(b):
        r64, keep64 = rc.decode(logits[i], loc[i], anchors, torch.float64, **args)
        r32, _ = rc.decode(logits[i], loc[i], anchors, torch.float32, **args)
        k = keep64.numel()
        assert int(count[i]) == k
        got = rows[i, :k]
        assert np.array_equal(got[:, 5], r64[:, 5].numpy())
        if k:
            base._judge("prob", got[:, 4], r64[:, 4].numpy(), r32[:, 4].numpy())
            base._judge("boxes", got[:, :4], r64[:, :4].numpy(), r32[:, :4].numpy())
        assert not rows[i, k:].any()


# --------------------------------------------------------------------------------------------------------------------
# NMS
# --------------------------------------------------------------------------------------------------------------------
def _clustered_rows(n, seed):
    """n score-descending x,y,w,h,score,class rows on a quarter-pixel grid: about n/4 clusters of boxes that overlap each other,
    scores with two decimals (ties), row order = a stable descending sort."""
    g = np.random.default_rng(seed)
    centres = g.uniform(0, 40.0 * max(np.sqrt(n), 1.0), (max(n // 4, 1), 2))
    xy = centres[g.integers(0, len(centres), n)] + g.uniform(-6, 6, (n, 2))
    wh = g.uniform(12, 36, (n, 2))
    rows = np.zeros((n, 6), dtype=np.float32)
    rows[:, 0:2], rows[:, 2:4] = np.round(xy * 4) / 4, np.round(wh * 4) / 4
    rows[:, 4] = np.round(g.uniform(0.1, 1.0, n), 2)
    rows[:, 5] = g.integers(1, 11, n)
    return rows[np.argsort(-rows[:, 4], kind="stable")]


def _xyxy(rows):
    out = rows.copy()
    out[:, 2:4] += out[:, 0:2]                                                 # float32, as _nms_rows and the kernel add
    return out


def _nms_sorted_single(rows, thresh, inclusive):
    """rr_nms_sorted on one frame, called as RetinaNetOperator._nms_rows calls it -> kept indices."""
    from rrnet_amd import _C
    n = rows.shape[0]
    if n == 0:
        return []
    xyxy = torch.from_numpy(rows).cuda()
    xyxy[:, 2:4] += xyxy[:, 0:2]
    ws = torch.empty(_C.fn("rr_nms_workspace_bytes")(n), dtype=torch.uint8, device="cuda")
    keep = torch.empty(n, dtype=torch.int32, device="cuda")
    num = torch.zeros(1, dtype=torch.int32, device="cuda")
    _C.check(_C.fn("rr_nms_sorted")(_C.ptr(xyxy), n, 6, float(np.float32(thresh)), int(inclusive), _C.ptr(ws), _C.ptr(keep),
                                    _C.ptr(num), _C.stream()), "rr_nms_sorted")
    return keep[:int(num.item())].cpu().tolist()


def _nms_frames(frames, thresh, inclusive=False):
    """frames: list of [n_f,6] arrays -> (kept indices per frame, packed rows, out_off) through rr_nms_frames and
    rr_pack_frames.  The packed buffer is padded with NaN rows to B * max_rows, the space the entry point may address."""
    lens = [f.shape[0] for f in frames]
    b, most = len(frames), max(lens)
    packed = np.full((max(b * most, 1), 6), np.nan, dtype=np.float32)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    for f, o in zip(frames, off):
        packed[o:o + f.shape[0]] = f
    rows6, frame_off = _dev(packed, off)
    keep, kept = ops.nms_frames(rows6, frame_off, most, thresh, inclusive)
    out6, out_off = ops.pack_frames(rows6, frame_off, keep, kept, most)
    torch.cuda.synchronize()
    keep, kept, out_off = keep.cpu().numpy(), kept.cpu().tolist(), out_off.cpu().numpy()
    return [keep[o:o + k].tolist() for o, k in zip(off, kept)], out6.cpu().numpy()[:out_off[-1]], out_off


LENGTHS = [(0,), (1,), (63,), (64,), (65,), (129,), (1000,), (65, 0, 129), (1000, 63, 129), (1, 1000, 64)]


@pytest.mark.parametrize("lens", LENGTHS, ids=lambda v: "-".join(map(str, v)))
def test_nms_frames_equals_restatement_and_single_frame_kernel(lens):
    """Kept indices and counts against rc.hard_nms_sorted (float32, "+1" IoU, IoU > 0.3 suppresses) and against rr_nms_sorted on
    every frame alone, also with IoU >= 0.3; the packed rows are those rows, frames back to back.  Frame lengths on both
    sides of the 64-row mask block; batches whose frames differ in length, so that a block past one frame's end lies inside
    another's, with an empty frame in the middle."""
    frames = [_clustered_rows(n, 900 + 7 * n + i) for i, n in enumerate(lens)]
    want = [rc.hard_nms_sorted(_xyxy(f), 0.3) for f in frames]
    for f, w in zip(frames, want):                                             # asked of the restatement before the GPU
        n = f.shape[0]
        assert (0 < len(w) < n) if n >= 63 else len(w) == n
        assert n < 63 or len(np.unique(f[:, 4])) < n                           # score ties
    got, out6, out_off = _nms_frames(frames, 0.3)
    print("\nnms_frames %s rows: kept %s" % (list(lens), [len(g) for g in got]))
    assert got == want
    assert got == [_nms_sorted_single(f, 0.3, 0) for f in frames]
    assert out_off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want])]).tolist()
    assert np.array_equal(_u32(out6), _u32(np.concatenate([f[w] for f, w in zip(frames, want)]).reshape(-1, 6)))
    got_inclusive, _, _ = _nms_frames(frames, 0.3, inclusive=True)
    assert got_inclusive == [_nms_sorted_single(f, 0.3, 1) for f in frames]


def test_nms_frames_chain_across_mask_blocks():
    """a at row 0, b at row 70 overlapping a, c at row 140 overlapping b only, singletons far away in between: b leaves through
    a, so c stays although b's mask word names it.  Second frame: a different length."""
    n = 200
    rows = np.zeros((n, 6), dtype=np.float32)
    rows[:, 0], rows[:, 1] = 1000.0 + 50.0 * np.arange(n), 1000.0
    rows[:, 2:4], rows[:, 5] = 10.0, 1.0
    rows[:, 4] = 1.0 - np.arange(n, dtype=np.float32) / 1000.0
    for r, x in ((0, 100.0), (70, 120.0), (140, 140.0)):
        rows[r, :4] = (x, 100.0, 40.0, 40.0)
    want = rc.hard_nms_sorted(_xyxy(rows), 0.3)
    assert want == [i for i in range(n) if i != 70]
    other = _clustered_rows(77, 5)
    got, _, _ = _nms_frames([rows, other], 0.3)
    assert got[0] == want and 0 in got[0] and 140 in got[0] and 70 not in got[0]
    assert got[1] == rc.hard_nms_sorted(_xyxy(other), 0.3)


def test_nms_frames_iou_exactly_at_the_threshold():
    """(0,0,9,9) and (0,0,9,4) as xyxy: areas 100 and 50 under the "+1" convention, intersection 50, IoU exactly 0.5."""
    pair = np.array([[0, 0, 9, 9, 0.9, 1], [0, 0, 9, 4, 0.8, 1]], dtype=np.float32)
    assert rc.hard_nms_sorted(_xyxy(pair), 0.5) == [0, 1]
    assert _nms_frames([pair, pair[:1]], 0.5, inclusive=False)[0] == [[0, 1], [0]]
    assert _nms_frames([pair, pair[:1]], 0.5, inclusive=True)[0] == [[0], [0]]
    assert _nms_sorted_single(pair, 0.5, 0) == [0, 1] and _nms_sorted_single(pair, 0.5, 1) == [0]


# --------------------------------------------------------------------------------------------------------------------
# decode -> sort -> NMS -> pack
# --------------------------------------------------------------------------------------------------------------------
def _tail_inputs(b=2, a=4000, cands=3000, c=10, seed=17):
    """Logits, box deltas and anchors whose float32 decode does not depend on whose expf computes it, so that the CPU
    restatement and the kernel can be compared as bits: a candidate's one live logit x lies in (7, 12) and is kept only when
    1 + e gives the same float32 for every e within two ulps of exp(-x) (the division that follows is IEEE on both sides);
    every other logit is -40 (probability 4e-18, whatever its last bit); the size deltas are 0 (exp(0) = 1 exactly)."""
    g = np.random.default_rng(seed)
    logits = np.full((b, a, c), -40.0, dtype=np.float32)
    for i in range(b):
        for r in g.choice(a, cands, replace=False):
            while True:
                x = np.float32(g.uniform(7.0, 12.0))
                e = np.float32(np.exp(-np.float64(x)))
                lo = np.nextafter(np.nextafter(e, np.float32(0)), np.float32(0))
                hi = np.nextafter(np.nextafter(e, np.float32(1)), np.float32(1))
                if np.float32(1) + lo == np.float32(1) + hi:
                    break
            logits[i, r, g.integers(0, c)] = x
    loc = np.zeros((b, a, 4), dtype=np.float32)
    loc[:, :, :2] = (g.standard_normal((b, a, 2)) * 0.8).astype(np.float32)
    centres = g.uniform(0, 900, (a // 5, 2))
    xy = np.round((centres[g.integers(0, len(centres), a)] + g.uniform(-8, 8, (a, 2))) * 4) / 4
    wh = np.round(g.uniform(16, 64, (a, 2)) * 4) / 4
    anchors = np.concatenate([xy, xy + wh], axis=1).astype(np.float32)
    return logits, loc, anchors


def test_whole_tail_equals_restated_decode_sort_and_nms():
    """rr_retina_decode_frames -> rr_sort_frames_by_score -> rr_nms_frames -> rr_pack_frames on 2 x 3000 candidates against
    rc.decode in float32 -> stable argsort by descending score -> rc.hard_nms_sorted: rows as uint32, order and offsets
    included."""
    logits, loc, anchors = _tail_inputs()
    want = []
    for i in range(2):
        r32, keep = rc.decode(logits[i], loc[i], anchors, torch.float32)
        r32 = r32.numpy()
        assert keep.numel() == 3000
        ordered = r32[np.argsort(-r32[:, 4], kind="stable")]
        kept = rc.hard_nms_sorted(_xyxy(ordered), 0.3)
        assert 0 < len(kept) < 3000
        want.append(ordered[kept])
    dl, dc, da = _dev(logits, loc, anchors)
    rows, count = ops.retina_decode_frames(dl, dc, da, 0.1, k=4000)
    assert count.tolist() == [3000, 3000]
    cand_off = ops.seg_prefix(count)
    ordered = ops.sort_frames_by_score(rows, count, out_off=cand_off)
    keep, kept = ops.nms_frames(ordered, cand_off, 3000, 0.3)
    out6, out_off = ops.pack_frames(ordered, cand_off, keep, kept, 3000)
    out_off = out_off.cpu().tolist()
    print("\ntail: 2 x 3000 candidates, kept %s" % [len(w) for w in want])
    assert out_off == [0, len(want[0]), len(want[0]) + len(want[1])]
    assert np.array_equal(_u32(out6[:out_off[-1]]), _u32(np.concatenate(want)))


# --------------------------------------------------------------------------------------------------------------------
# prepare without a resize
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(5, 7), (37, 53)])
def test_prepare_frames_at_the_frames_own_size_is_totensor_normalize(hw):
    g = np.random.default_rng(hw[0])
    frames = g.integers(0, 256, (2,) + hw + (3,), dtype=np.uint8)
    frames[0, 0, 0] = (0, 255, 124)
    mean, std = np.array(MEAN, dtype=np.float32), np.array(STD, dtype=np.float32)
    want = (frames.astype(np.float32) / np.float32(255) - mean) / std          # float32 throughout
    got = ops.prepare_frames(torch.from_numpy(frames).cuda(), *_dev(mean, std), 1)
    assert tuple(got.shape) == (2, 3) + hw
    assert np.array_equal(_u32(got.permute(0, 2, 3, 1)), _u32(want))


# --------------------------------------------------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def operator():
    from rrnet_amd.operators.retinanet_operator import RetinaNetOperator
    torch.manual_seed(219)
    op = RetinaNetOperator(rc.retina_cfg("resnet10", crop=(128, 128)))
    op.model.eval()
    return op


def _frames():
    g = np.random.default_rng(128)
    coarse = g.integers(0, 256, (2, 16, 16, 3), dtype=np.uint8)
    return torch.from_numpy(np.kron(coarse, np.ones((1, 8, 8, 1), np.uint8))).cuda()      # [2,128,128,3] in 8x8 blocks


def _inner(op):
    return getattr(op.model, "module", op.model)


def test_detect_frames_retinanet_equals_restatement_of_the_captured_outputs(operator):
    """B = 2, resnet10, 128x128.  The model's outputs are captured by a forward hook; on them the restatement of
    test_evaluate_images_equals_restated_decode_and_nms: the per-image kernel's candidates equal rc.decode in float64 (same
    anchors, values by the measured rule), and the returned rows are exactly what a float32 stable score sort and hard NMS at
    0.3 keep from those candidates, frames back to back."""
    from rrnet_amd import inference
    model, anchors = _inner(operator), rc.anchors_of((128, 128))
    seen = []
    handle = model.register_forward_hook(lambda m, inp, out: seen.append(out))
    try:
        boxes, frame_off = inference.detect_frames_retinanet(model, _frames(), MEAN, STD, anchors.cuda())
    finally:
        handle.remove()
    assert len(seen) == 1                                                      # one model pass
    loc, cls = seen[0]
    rows, count = ops.retina_decode(cls, loc, anchors.cuda())
    off = frame_off.cpu().tolist()
    assert frame_off.dtype == torch.int32 and frame_off.is_cuda and len(off) == 3 and off[0] == 0 and off[2] == boxes.shape[0]
    for i in range(2):
        r64, keep64 = rc.decode(cls[i].cpu(), loc[i].cpu(), anchors, torch.float64)
        r32, _ = rc.decode(cls[i].cpu(), loc[i].cpu(), anchors, torch.float32)
        assert float((torch.sigmoid(cls[i].cpu().double()).max(dim=1).values - 0.1).abs().min()) > 1e-5
        k = int(count[i])
        assert k == keep64.numel() and k > 0
        got = rows[i, :k].cpu().numpy()
        assert np.array_equal(got[:, 5], r64[:, 5].numpy())
        tol = max(4 * float((r32 - r64).abs().max()), 2 * rc.U32 * float(r64.abs().max()))
        assert float(np.abs(got - r64.numpy()).max()) <= tol
        ordered = got[np.argsort(-got[:, 4], kind="stable")]
        want = ordered[rc.hard_nms_sorted(_xyxy(ordered), 0.3)]
        out = boxes[off[i]:off[i + 1]].cpu().numpy()
        print("\nframe %d: %d candidates, %d kept" % (i, k, len(want)))
        assert 0 < len(want) < k
        assert out.shape == want.shape and np.array_equal(_u32(out), _u32(want))


def test_detect_frames_retinanet_equals_evaluate_images_row_for_row(operator):
    """The same call against the per-frame path on prepare_frames of the same batch: both make the same model call on the
    same bits."""
    from rrnet_amd import inference
    frames = _frames()
    anchors = rc.anchors_of((128, 128)).cuda()
    boxes, frame_off = inference.detect_frames_retinanet(_inner(operator), frames, MEAN, STD, anchors)
    x = ops.prepare_frames(frames, *_dev(np.array(MEAN, np.float32), np.array(STD, np.float32)), 1)
    with torch.no_grad():
        per_frame = operator.evaluate_images(x)
    off = frame_off.cpu().tolist()
    assert len(per_frame) == 2
    for i, want in enumerate(per_frame):
        got = boxes[off[i]:off[i + 1]]
        assert got.shape == want.shape and want.shape[0] > 0
        assert np.array_equal(_u32(got), _u32(want)), i


def test_detect_frames_retinanet_refuses_too_many_candidates(operator, monkeypatch):
    from rrnet_amd import inference
    monkeypatch.setattr(inference, "RETINA_MAX_CANDIDATES", 8)
    with pytest.raises(ValueError, match=r"frame 0 has \d+ candidates"):
        inference.detect_frames_retinanet(_inner(operator), _frames(), MEAN, STD, rc.anchors_of((128, 128)).cuda())


def test_detect_frames_retinanet_without_candidates(operator):
    """No anchor of the untrained model reaches 0.999: empty ranges, nothing launched behind the decode."""
    from rrnet_amd import inference
    boxes, frame_off = inference.detect_frames_retinanet(_inner(operator), _frames(), MEAN, STD,
                                                         rc.anchors_of((128, 128)).cuda(), score_thr=0.999)
    assert tuple(boxes.shape) == (0, 6) and frame_off.tolist() == [0, 0, 0] and frame_off.dtype == torch.int32


def test_detect_tool_runs_retinanet(tmp_path, golden_dir):
    """tools/detect.py --config retinanet_config --random-weights in a child process on the demo image, twice: two result
    files whose every line has save_result's format.  The tool picks the score threshold itself (random weights)."""
    src = os.path.join(golden_dir, "visdrone_demo", "images")
    name = sorted(os.listdir(src))[0]
    os.makedirs(tmp_path / "images")
    for copy in ("a", "b"):
        shutil.copy(os.path.join(src, name), tmp_path / "images" / (copy + os.path.splitext(name)[1]))
    cmd = [sys.executable, os.path.join(ROOT, "tools", "detect.py"), "--config", "retinanet_config", "--backbone", "resnet10",
           "--random-weights", "--images", str(tmp_path / "images"), "--out", str(tmp_path / "out"), "--batch", "2"]
    out = subprocess.run(cmd, cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "2 frames" in out.stdout and "score threshold" in out.stdout
    assert sorted(os.listdir(tmp_path / "out")) == ["a.txt", "b.txt"]
    line = re.compile(r"^\d+,\d+,\d+,\d+,[01]\.\d{4},([1-9]|10),-1,-1$")
    for f in ("a.txt", "b.txt"):
        lines = open(tmp_path / "out" / f).read().splitlines()
        assert lines and all(line.match(t) for t in lines), lines[:3]
    assert open(tmp_path / "out" / "a.txt").read() == open(tmp_path / "out" / "b.txt").read()      # the same image twice
