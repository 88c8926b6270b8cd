"""GPU: tiled RetinaNet inference — rr_prepare_tiles against rr_prepare_frames on the host-cropped tiles, rr_merge_tiles
against the numpy restatement (tile_cases), detect_tiled_retinanet against detect_frames_retinanet where a tile is the frame,
mixed frame sizes end to end, and finish_tiles' refusals.  Every comparison is equality."""
import numpy as np
import pytest
import torch

import retina_cases as rc
import tile_cases as tc
from rrnet_amd import inference, ops

pytestmark = pytest.mark.gpu
SENTINEL = -7.25e30                        # what a buffer holds where the kernel must not write
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _u32(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _dev(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


# --------------------------------------------------------------------------------------------------------------------
# rr_prepare_tiles
# --------------------------------------------------------------------------------------------------------------------
FRAME_SIZES = [(5, 7), (37, 53), (16, 16)]            # 5*7*3 = 105 bytes: the second frame starts at an odd address
# (tile, overlap, the frames that get tiles)
PREPARE_CASES = {"4x4": ((4, 4), 1, (0, 1, 2)), "5x7": ((5, 7), 2, (0, 1, 2)), "16x16": ((16, 16), 5, (1, 2)),
                 "1x7": ((1, 7), 0, (0, 1, 2))}


@pytest.fixture(scope="module")
def frames_np():
    g = np.random.default_rng(57)
    frames = [g.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in FRAME_SIZES]
    frames[0][0, 0] = (0, 255, 124)
    return frames


@pytest.mark.parametrize("zoom", [1, 1.5, 2, 0.7])
@pytest.mark.parametrize("case", sorted(PREPARE_CASES))
def test_prepare_tiles_equals_prepare_frames_on_the_cropped_tiles(frames_np, case, zoom):
    """Tile t as uint32 against ops.prepare_frames on frame[y0:y0+th, x0:x0+tw]; the buffer is pre-filled with a sentinel and
    the spare tile behind the last one comes back untouched.  At zoom 1 also against (u8/255 - mean)/std in numpy float32."""
    (th, tw), overlap, with_tiles = PREPARE_CASES[case]
    table = [(f, y0, x0) for f in with_tiles for y0, x0 in inference.plan_tiles(*FRAME_SIZES[f], (th, tw), overlap)]
    if case == "5x7":
        assert table[0] == (0, 0, 0) and [t[0] for t in table].count(0) == 1   # one tile on the first frame, flush with its border
    mean, std = _dev(np.array(MEAN, np.float32), np.array(STD, np.float32))
    frames = _dev(*frames_np)
    oh, ow = int(np.floor(th * zoom)), int(np.floor(tw * zoom))
    if oh == 0:                                                                # 1x7 at 0.7: no output rows
        with pytest.raises(ValueError, match="is empty"):
            ops.prepare_tiles(frames, table, (th, tw), zoom, mean, std)
        return
    t = len(table)
    buf = torch.full((t + 1, oh, ow, 3), SENTINEL, dtype=torch.float32, device="cuda")
    got = ops.prepare_tiles(frames, table, (th, tw), zoom, mean, std, out=buf[:t].permute(0, 3, 1, 2))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (t, 3, oh, ow)
    crops = np.stack([frames_np[f][y0:y0 + th, x0:x0 + tw] for f, y0, x0 in table])
    want = ops.prepare_frames(torch.from_numpy(crops).cuda(), mean, std, zoom)
    assert tuple(want.shape) == (t, 3, oh, ow)
    print("\nprepare_tiles %s zoom %g: %d tiles -> %dx%d" % (case, zoom, t, oh, ow))
    assert np.array_equal(_u32(buf[:t]), _u32(want.permute(0, 2, 3, 1)))
    assert (_u32(buf[t]) == np.float32(SENTINEL).view(np.uint32)).all()
    if zoom == 1:
        m, s = np.array(MEAN, np.float32), np.array(STD, np.float32)
        assert np.array_equal(_u32(buf[:t]), _u32((crops.astype(np.float32) / np.float32(255) - m) / s))


def test_prepare_tiles_takes_a_batch_tensor_and_checks_the_table(frames_np):
    g = np.random.default_rng(5)
    batch = g.integers(0, 256, (3, 9, 11, 3), dtype=np.uint8)
    table = [(f, y0, x0) for f in range(3) for y0, x0 in inference.plan_tiles(9, 11, (4, 6), 1)]
    mean, std = _dev(np.array(MEAN, np.float32), np.array(STD, np.float32))
    got = ops.prepare_tiles(torch.from_numpy(batch).cuda(), table, (4, 6), 1.5, mean, std)
    crops = np.stack([batch[f, y0:y0 + 4, x0:x0 + 6] for f, y0, x0 in table])
    want = ops.prepare_frames(torch.from_numpy(crops).cuda(), mean, std, 1.5)
    assert np.array_equal(_u32(got.permute(0, 2, 3, 1)), _u32(want.permute(0, 2, 3, 1)))
    with pytest.raises(ValueError, match="leaves frame 2"):                    # refused on the host, before the upload
        ops.prepare_tiles(torch.from_numpy(batch).cuda(), [(2, 6, 0)], (4, 6), 1, mean, std)
    with pytest.raises(ValueError, match="names frame 3"):
        ops.prepare_tiles(_dev(*frames_np), [(3, 0, 0)], (4, 4), 1, mean, std)


# --------------------------------------------------------------------------------------------------------------------
# rr_merge_tiles
# --------------------------------------------------------------------------------------------------------------------
def _merge_on_device(rows, counts, div, margin, k):
    """-> (merged [F,k,6], count [F], the guard row behind the last frame) of rr_merge_tiles writing into sentinels."""
    nf = len(tc.MERGE_SIZES)
    flat = torch.full((nf * k + 1, 6), SENTINEL, dtype=torch.float32, device="cuda")
    count = torch.zeros(nf, dtype=torch.int32, device="cuda")
    drows, dcount = _dev(rows, np.asarray(counts, np.int32))
    ops.merge_tiles(drows, dcount, tc.MERGE_TILES, tc.MERGE_SIZES, tc.MERGE_TILE, tc.merge_in_size(div), div, margin,
                    flat[:nf * k].view(nf, k, 6), count)
    torch.cuda.synchronize()
    return flat[:nf * k].view(nf, k, 6).cpu().numpy(), count.cpu().numpy(), flat[nf * k].cpu().numpy()


@pytest.mark.parametrize("margin", tc.MERGE_MARGINS)
@pytest.mark.parametrize("div", tc.MERGE_DIVS)
@pytest.mark.parametrize("layout", sorted(tc.MERGE_COUNTS))
def test_merge_tiles_equals_the_restatement_bit_for_bit(layout, div, margin):
    """Rows and counts as uint32.  Three frames with 1, 4 and 6 tiles, every tile of the middle frame empty, per-tile counts
    from {0, 1, 63, 64, 65, 257} and one of k_in + 5 (clamped); what the planted rows and the margin do is asserted of the
    restatement in test_tiled_host.py."""
    counts = tc.MERGE_COUNTS[layout]
    rows = tc.merge_rows(div, margin)
    kept, _ = tc.merge_tiles(rows, counts, tc.MERGE_TILES, tc.MERGE_SIZES, tc.MERGE_TILE, tc.merge_in_size(div), div, margin)
    k = 400
    want, want_count = tc.into_buffer(kept, k, SENTINEL)
    total = sum(min(max(c, 0), tc.MERGE_K_IN) for c in counts)
    assert want_count.sum() == total if margin == 0 else 0 < want_count.sum() < total
    assert want_count.max() <= k and want_count[1] == 0
    got, got_count, guard = _merge_on_device(rows, counts, div, margin, k)
    print("\nmerge_tiles %s div %g margin %g: %s of %d rows kept" % (layout, div, margin, got_count.tolist(), total))
    assert np.array_equal(got_count, want_count)
    assert np.array_equal(_u32(got), _u32(want))                               # also the sentinels between count[f] and k
    assert (_u32(guard) == np.float32(SENTINEL).view(np.uint32)).all()


def test_merge_tiles_counts_beyond_k_and_writes_nothing_there():
    """K = 100 against 322 kept rows: count is 322, the first 100 rows are the restatement's, rows from 100 on keep their
    sentinel, and so does the row behind the last frame's block."""
    counts = tc.MERGE_COUNTS["a"]
    rows = tc.merge_rows(1.5, 0.0)
    kept, _ = tc.merge_tiles(rows, counts, tc.MERGE_TILES, tc.MERGE_SIZES, tc.MERGE_TILE, tc.merge_in_size(1.5), 1.5, 0.0)
    assert [len(r) for r in kept] == [63, 0, 322]
    want, want_count = tc.into_buffer(kept, 100, SENTINEL)
    got, got_count, guard = _merge_on_device(rows, counts, 1.5, 0.0, 100)
    assert got_count.tolist() == [63, 0, 322] == want_count.tolist()
    assert np.array_equal(_u32(got), _u32(want))
    assert np.array_equal(_u32(got[2]), _u32(kept[2][:100]))
    assert (_u32(got[0, 63:]) == np.float32(SENTINEL).view(np.uint32)).all()
    assert (_u32(guard) == np.float32(SENTINEL).view(np.uint32)).all()


# --------------------------------------------------------------------------------------------------------------------
# end to end
# --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def detector():
    torch.manual_seed(219)
    return inference.RetinaNetFrameDetector(rc.retina_cfg("resnet10", crop=(128, 128)))


def _blocks(h, w, seed):
    g = np.random.default_rng(seed)
    coarse = g.integers(0, 256, (h // 8 + 1, w // 8 + 1, 3), dtype=np.uint8)
    return np.kron(coarse, np.ones((8, 8, 1), np.uint8))[:h, :w]              # 8x8 blocks, not white noise


def test_detect_tiled_with_the_frame_as_its_tile_equals_detect_frames(detector):
    """Two 128x128 frames, tile 128, zoom 1, margin 0: one tile per frame at the origin, so x / 1 + 0 must give
    detect_frames_retinanet's rows and offsets.  Rows are compared with float ==, because x + 0.0 turns -0.0 into +0.0.  Like
    test_detect_frames_retinanet_equals_evaluate_images_row_for_row this rests on the forward pass being reproducible run to run
    at this shape: both calls make the same model call on the same bits."""
    frames = torch.from_numpy(np.stack([_blocks(128, 128, 128), _blocks(128, 128, 129)])).cuda()
    thr, at_thr = detector.threshold_for_rows(frames, 1000)
    want, want_off = detector.detect(frames, score_thr=thr)
    got, got_off = detector.detect_tiled(frames, 128, 0, zoom=1.0, margin=0.0, score_thr=thr)
    print("\nidentity: threshold %.9g keeps %s candidates, %s rows after the NMS" % (thr, at_thr, want_off.tolist()))
    assert got_off.dtype == torch.int32 and got_off.is_cuda
    off = want_off.tolist()
    assert got_off.tolist() == off and off[1] > 0 and off[2] > off[1]
    assert got.shape == want.shape and bool((got == want).all())
    as_list, list_off = detector.detect_tiled([frames[0], frames[1]], (128, 128), 0, score_thr=thr)    # a list of frames
    assert list_off.tolist() == want_off.tolist() and bool((as_list == want).all())


@pytest.mark.parametrize("zoom", [1.0, 1.5])
def test_detect_tiled_on_mixed_frame_sizes_equals_the_restated_tail(detector, zoom):
    """Frames of 128x128 and 160x192 in one call, tile 96, overlap 32, four tiles per pass: ten tiles in passes of 4, 4 and 2,
    the second of which straddles the frames.  The model's outputs are captured by a forward hook; the expected rows are
    ops.retina_decode_frames on them -> the numpy restatement of the merge -> the existing sort / NMS / pack, compared as
    uint32 (no CPU expf on either side).  Margin 0 and 3."""
    frames = [torch.from_numpy(_blocks(128, 128, 1)).cuda(), torch.from_numpy(_blocks(160, 192, 2)).cuda()]
    sizes = [(128, 128), (160, 192)]
    table = [(f, y0, x0) for f, (h, w) in enumerate(sizes) for y0, x0 in inference.plan_tiles(h, w, 96, 32)]
    assert [t[0] for t in table] == [0] * 4 + [1] * 6
    side = int(np.floor(96 * zoom))
    anchors = detector.anchors((side, side))
    thr, most = detector.threshold_for_tile_rows(frames, 96, 32, zoom, 300, tile_batch=4)
    entering = {}
    for margin in (0.0, 3.0):
        seen = []
        handle = detector.model.register_forward_hook(lambda m, inp, out: seen.append(out))
        try:
            got, got_off = detector.detect_tiled(frames, 96, 32, zoom=zoom, margin=margin, tile_batch=4, score_thr=thr)
        finally:
            handle.remove()
        assert [out[1].shape[0] for out in seen] == [4, 4, 2]
        k = min(anchors.shape[0], 16384)
        decoded = [ops.retina_decode_frames(cls, loc, anchors, thr, k=k) for loc, cls in seen]
        rows = torch.cat([r for r, _ in decoded]).cpu().numpy()
        count_in = torch.cat([c for _, c in decoded]).cpu().numpy()
        assert count_in.max() <= k
        kept, _ = tc.merge_tiles(rows, count_in, table, sizes, (96, 96), (side, side), np.float32(zoom), margin)
        entering[margin] = sum(len(r) for r in kept)
        merged, count = _dev(*tc.into_buffer(kept, max(len(r) for r in kept), -1.0))
        cand_off = ops.seg_prefix(count)
        ordered = ops.sort_frames_by_score(merged, count, out_off=cand_off)
        most_rows = int(count.max())
        keep, n_kept = ops.nms_frames(ordered, cand_off, most_rows, 0.3)
        want, want_off = ops.pack_frames(ordered, cand_off, keep, n_kept, most_rows)
        want_off = want_off.cpu().tolist()
        print("\nmixed sizes zoom %g margin %g: %s candidates per tile -> %s rows enter the sort -> %s kept"
              % (zoom, margin, count_in.tolist(), count.tolist(), np.diff(want_off).tolist()))
        assert got_off.tolist() == want_off and want_off[1] > 0 and want_off[2] > want_off[1]      # both frames keep rows
        assert np.array_equal(_u32(got), _u32(want[:want_off[-1]]))
    assert 0 < entering[3.0] < entering[0.0]


# --------------------------------------------------------------------------------------------------------------------
# refusals
# --------------------------------------------------------------------------------------------------------------------
def _grid_rows(t, k, seed):
    """[t,k,6] boxes of 2x2 on a grid with pitch 4 inside a 512-pixel-wide tile: no two overlap, none within half a pixel of a
    tile side; random scores."""
    idx = np.arange(k)
    rows = np.zeros((t, k, 6), dtype=np.float32)
    rows[:, :, 0], rows[:, :, 1] = (idx % 128) * 4.0 + 1.0, (idx // 128) * 4.0 + 1.0
    rows[:, :, 2:4], rows[:, :, 5] = 2.0, 1.0
    rows[:, :, 4] = np.random.default_rng(seed).uniform(0.1, 1.0, (t, k)).astype(np.float32)
    return rows


def test_finish_tiles_refuses_a_tile_above_k_and_a_frame_above_the_sort():
    sizes, tile, table = [(512, 512), (512, 1024)], (512, 512), [(0, 0, 0), (1, 0, 0), (1, 0, 512)]
    k = 8193
    rows, = _dev(_grid_rows(3, k, 4))
    with pytest.raises(ValueError, match=r"tile 2 \(frame 1, origin y 0 x 512\) has 8194 candidates"):
        inference.finish_tiles(rows, torch.tensor([5, 8193, 8194], dtype=torch.int32).cuda(), table, sizes, tile, tile)
    for margin in (0.0, 0.5):                                                  # known from the tile counts / after the merge
        with pytest.raises(ValueError, match=r"frame 1 has 16385 merged rows"):
            inference.finish_tiles(rows, torch.tensor([5, 8193, 8192], dtype=torch.int32).cuda(), table, sizes, tile, tile,
                                   margin=margin)
    boxes, off = inference.finish_tiles(rows, torch.tensor([5, 8192, 8192], dtype=torch.int32).cuda(), table, sizes, tile, tile)
    assert off.tolist() == [0, 5, 5 + 16384] and tuple(boxes.shape) == (5 + 16384, 6)    # 16384 rows pass; nothing overlaps
    assert bool((boxes[5:, 0] >= 0).all()) and float(boxes[5:, 0].max()) == 509.0 + 512.0
