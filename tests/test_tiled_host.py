"""Host-side tests of tiled RetinaNet inference: plan_tiles, the numpy restatement of rr_merge_tiles and its cases, the
host check of a tile table, OrderedFrames, the command's refusals and evaluate_batched's routing.  No GPU."""
import functools
import importlib.util
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import tile_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# --------------------------------------------------------------------------------------------------------------------
# plan_tiles
# --------------------------------------------------------------------------------------------------------------------
def _hw(tile):
    return tuple(tile) if isinstance(tile, tuple) else (tile, tile)


@pytest.mark.parametrize("h,w,tile,overlap", tc.PLAN_SHAPES)
def test_plan_tiles_covers_the_frame_with_full_tiles(h, w, tile, overlap):
    from rrnet_amd.inference import plan_tiles
    th, tw = _hw(tile)
    plan = plan_tiles(h, w, tile, overlap)
    covered = np.zeros((h, w), dtype=bool)
    for y0, x0 in plan:
        assert 0 <= y0 and y0 + th <= h and 0 <= x0 and x0 + tw <= w           # inside the frame, full size
        covered[y0:y0 + th, x0:x0 + tw] = True
    assert covered.all()
    ys, xs = sorted({y for y, _ in plan}), sorted({x for _, x in plan})
    assert plan == [(y, x) for y in ys for x in xs]                            # row-major, y outer
    for origins, length, t in ((ys, h, th), (xs, w, tw)):
        assert len(origins) == math.ceil((length - t) / (t - overlap)) + 1
        assert origins[0] == 0 and origins[-1] == length - t
        assert all(a + t - b >= overlap for a, b in zip(origins, origins[1:]))  # neighbours share at least `overlap`


def test_plan_tiles_literal_lists_and_refusals():
    from rrnet_amd.inference import plan_tiles
    assert plan_tiles(5, 7, 4, 1) == tc.PLAN_5x7_T4_O1 == plan_tiles(5, 7, (4, 4), 1)
    assert plan_tiles(765, 1360, 512, 128) == tc.PLAN_765x1360_T512_O128
    assert plan_tiles(16, 16, 16, 3) == [(0, 0)]                               # L == t: one tile
    assert plan_tiles(16, 40, 16, 0) == [(0, 0), (0, 16), (0, 24)]
    with pytest.raises(ValueError, match=r"15x40 frame .* 16x16 tile"):        # names the frame size and the tile
        plan_tiles(15, 40, 16, 0)
    with pytest.raises(ValueError, match=r"40x15 frame .* 16x16 tile"):
        plan_tiles(40, 15, 16, 0)
    for overlap in (16, 17, -1):
        with pytest.raises(ValueError, match="overlap"):
            plan_tiles(40, 40, 16, overlap)
    with pytest.raises(ValueError, match="overlap"):
        plan_tiles(40, 40, (32, 8), 8)                                         # against the smaller side


def test_check_tiles_refuses_what_the_kernels_must_not_see():
    from rrnet_amd import ops
    sizes = [(5, 7), (16, 16)]
    table, off = ops.check_tiles([(0, 0, 0), (0, 1, 3), (1, 12, 12)], sizes, (4, 4))
    assert table.dtype == np.int32 and table.tolist() == [[0, 0, 0], [0, 1, 3], [1, 12, 12]] and off.tolist() == [0, 2, 3]
    assert ops.check_tiles([], sizes, (4, 4))[1].tolist() == [0, 0, 0]
    assert ops.check_tiles([(1, 0, 0)], sizes, (4, 4))[1].tolist() == [0, 0, 1]   # a frame without tiles
    for bad, sentence in (([(2, 0, 0)], "names frame 2"), ([(-1, 0, 0)], "names frame -1"), ([(0, 2, 0)], "leaves frame 0"),
                          ([(0, 0, 4)], "leaves frame 0"), ([(0, -1, 0)], "leaves frame 0"), ([(1, 0, 13)], "leaves frame 1"),
                          ([(1, 0, 0), (0, 0, 0)], "sorted by frame")):
        with pytest.raises(ValueError, match=sentence):
            ops.check_tiles(bad, sizes, (4, 4))


# --------------------------------------------------------------------------------------------------------------------
# the restatement
# --------------------------------------------------------------------------------------------------------------------
def test_restatement_identity_on_one_tile_at_the_origin():
    """One tile at (0, 0), div 1, margin 0: x / 1 + 0 is x.  Compared with ==, not as bits: -0.0 + 0.0 is +0.0."""
    g = np.random.default_rng(3)
    rows = g.standard_normal((1, 40, 6)).astype(np.float32) * 50
    rows[0, 0, 0] = -0.0
    kept, masks = tc.merge_tiles(rows, [40], [(0, 0, 0)], [(32, 32)], (32, 32), (32, 32), 1.0, 0.0)
    assert len(kept) == 1 and kept[0].shape == (40, 6) and not masks[0].any()
    assert (kept[0] == rows[0]).all()
    merged, count = tc.into_buffer(kept, 16, -3.0)
    assert count.tolist() == [40] and (merged[0] == rows[0, :16]).all()


@pytest.mark.parametrize("layout", sorted(tc.MERGE_COUNTS))
@pytest.mark.parametrize("div", tc.MERGE_DIVS)
def test_margin_cases_keep_some_rows_and_drop_some(layout, div):
    """Asked of the restatement before any GPU comparison: with the margin, 0 < kept < total; the planted rows stay or leave
    as the rule says, on every tile that holds them; without it, nothing leaves and frame 2 of layout "a" holds 322 rows."""
    counts = tc.MERGE_COUNTS[layout]
    taken = [min(max(c, 0), tc.MERGE_K_IN) for c in counts]
    rows = tc.merge_rows(div, 2.25)
    kept0, masks0 = tc.merge_tiles(rows, counts, tc.MERGE_TILES, tc.MERGE_SIZES, tc.MERGE_TILE, tc.merge_in_size(div), div, 0.0)
    assert [len(k) for k in kept0] == [taken[0], 0, sum(taken[5:])] and not any(m.any() for m in masks0)
    if layout == "a":
        assert len(kept0[2]) == 322
    kept, masks = tc.merge_tiles(rows, counts, tc.MERGE_TILES, tc.MERGE_SIZES, tc.MERGE_TILE, tc.merge_in_size(div), div, 2.25)
    total, stay = sum(taken), sum(len(k) for k in kept)
    assert 0 < stay < total
    assert len(kept[0]) == taken[0] and len(kept[1]) == 0 and 0 < len(kept[2]) < sum(taken[5:])   # frame 0: all sides on the border
    sides_seen = set()
    for (f, y0, x0), n, mask in zip(tc.MERGE_TILES, taken, masks):
        fh, fw = tc.MERGE_SIZES[f]
        interior = {"left": x0 > 0, "top": y0 > 0, "right": x0 + 32 < fw, "bottom": y0 + 32 < fh}
        for i, name in enumerate(tc.PLANTED[:n]):
            side, _, where = name.partition("_")
            want = where == "in" and interior[side]
            assert bool(mask[i]) == want, (f, y0, x0, name)
            if want:
                sides_seen.add(side)
    assert sides_seen == {"left", "top", "right", "bottom"}                    # each side drops its planted row somewhere
    nan_rows = [k for k in kept if len(k) and np.isnan(k[:, 0]).any()]
    assert nan_rows                                                            # the NaN rows stayed


# --------------------------------------------------------------------------------------------------------------------
# OrderedFrames
# --------------------------------------------------------------------------------------------------------------------
class _Frames:
    """Dataset stand-in with DronesDET's load surface: frame i is filled with the value i."""

    def __init__(self, sizes):
        self.sizes = sizes
        self.mdf = ["img%02d" % i for i in range(len(sizes))]

    def __len__(self):
        return len(self.sizes)

    def load(self, i):
        from PIL import Image
        h, w = self.sizes[i]
        return Image.fromarray(np.full((h, w, 3), i, np.uint8)), None, self.mdf[i]


def test_ordered_frames_keeps_file_order_whatever_the_sizes(tmp_path):
    from PIL import Image
    from rrnet_amd.datasets.frames import FrameFolder, OrderedFrames, SizeBucketedFrames
    sizes = [(4, 6), (5, 3), (4, 6), (7, 7), (5, 3), (4, 6), (7, 7)]
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(np.full((h, w, 3), 10 + i, np.uint8)).save(tmp_path / ("f%02d.png" % i))
    folder = FrameFolder(str(tmp_path))
    steps = list(OrderedFrames(folder, 3, num_workers=2, device="cpu"))
    assert [len(frames) for frames, _ in steps] == [3, 3, 1] == [len(names) for _, names in steps]
    assert [n for _, names in steps for n in names] == ["f%02d" % i for i in range(7)]
    flat = [fr for frames, _ in steps for fr in frames]
    for i, fr in enumerate(flat):
        assert fr.dtype == torch.uint8 and tuple(fr.shape) == sizes[i] + (3,) and int(fr[0, 0, 0]) == 10 + i
    assert [len(f) for f, _ in OrderedFrames(folder, 8, num_workers=1, device="cpu")] == [7]
    assert [n for _, names in OrderedFrames(folder, 2, rank=1, world_size=2, device="cpu") for n in names] == ["f01", "f03", "f05"]
    # the bucketed iterator, on the same folder, cuts batches short: what tiling removes
    assert [f.shape[0] for f, _ in SizeBucketedFrames(folder, 3, num_workers=2, device="cpu")] == [3, 2, 2]


# --------------------------------------------------------------------------------------------------------------------
# the command
# --------------------------------------------------------------------------------------------------------------------
def _detect_tool():
    spec = importlib.util.spec_from_file_location("detect_tool_tiled", os.path.join(ROOT, "tools", "detect.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_detect_command_tile_refusals(tmp_path):
    tool = _detect_tool()
    tail = ["--images", str(tmp_path), "--out", str(tmp_path / "out"), "--random-weights"]
    for other in ("rrnet_config", "rrnet_fillduck_config", "centernet_config"):
        with pytest.raises(SystemExit, match="retinanet_config only"):
            tool.main(["--config", other] + tail + ["--tile", "512"])
        with pytest.raises(SystemExit, match="retinanet_config only"):
            tool.main(["--config", other] + tail + ["--tile-zoom", "1.5"])
    base = ["--config", "retinanet_config"] + tail
    for bad in ("abc", "512,", "1,2,3", "0", "-4", "512x512", "5.5"):
        with pytest.raises(SystemExit, match="--tile takes N or H,W"):
            tool.main(base + ["--tile=" + bad])
    for overlap in ("512", "600", "-1"):
        with pytest.raises(SystemExit, match="--tile-overlap"):
            tool.main(base + ["--tile", "512", "--tile-overlap=" + overlap])
    with pytest.raises(SystemExit, match="--tile-overlap"):
        tool.main(base + ["--tile", "512,64", "--tile-overlap", "64"])         # against the smaller side
    with pytest.raises(SystemExit, match="need --tile"):
        tool.main(base + ["--tile-overlap", "64"])
    with pytest.raises(SystemExit, match="--tile-zoom"):
        tool.main(base + ["--tile", "512", "--tile-zoom", "0"])
    with pytest.raises(SystemExit, match="--tile-margin"):
        tool.main(base + ["--tile", "512", "--tile-margin=-1"])
    with pytest.raises(SystemExit, match="--tile-batch"):
        tool.main(base + ["--tile", "512", "--tile-batch", "0"])
    ns = SimpleNamespace(tile="512", tile_overlap=None, tile_zoom=None, tile_margin=None, tile_batch=None)
    assert tool.parse_tile(ns) == dict(tile=(512, 512), overlap=128, zoom=1.0, margin=0.0, batch=8)
    ns = SimpleNamespace(tile="96,128", tile_overlap=32, tile_zoom=1.5, tile_margin=4.0, tile_batch=4)
    assert tool.parse_tile(ns) == dict(tile=(96, 128), overlap=32, zoom=1.5, margin=4.0, batch=4)


def test_detect_command_runs_the_tiled_path(tmp_path, monkeypatch, capsys):
    import rrnet_amd.datasets.frames as frames_mod
    import rrnet_amd.inference as inference
    tool = _detect_tool()
    made = []

    class FakeDetector:
        def __init__(self, cfg, checkpoint=None, device=None):
            made.append(self)
            self.calls = []

        def threshold_for_tile_rows(self, frames, tile, overlap, zoom, rows_per_tile, tile_batch=8):
            self.calls.append(("pick", [tuple(f.shape) for f in frames], tile, overlap, zoom, rows_per_tile, tile_batch))
            return 0.625, rows_per_tile

        def detect(self, *a, **k):
            raise AssertionError("the whole-frame path ran with --tile")

        def detect_tiled(self, frames, tile, overlap, zoom=1.0, margin=0.0, tile_batch=8, score_thr=0.1, nms_thresh=0.3,
                         timer=None):
            self.calls.append(("tiled", len(frames), tile, overlap, zoom, margin, tile_batch, score_thr))
            n = len(frames)
            return torch.tensor([[1.5, 2.5, 10.5, 20.5, 0.25, 3.0]] * n), torch.arange(n + 1, dtype=torch.int32)

    monkeypatch.setattr(inference, "RetinaNetFrameDetector", FakeDetector)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(frames_mod, "FrameFolder", lambda path: _Frames([(40, 60), (50, 33), (40, 60)]))
    monkeypatch.setattr(frames_mod, "OrderedFrames", functools.partial(frames_mod.OrderedFrames, device="cpu"))
    tool.main(["--config", "retinanet_config", "--images", str(tmp_path), "--out", str(tmp_path / "out"), "--random-weights",
               "--batch", "2", "--tile", "32", "--tile-overlap", "8", "--tile-zoom", "1.5", "--tile-margin", "4",
               "--tile-batch", "4"])
    # the threshold comes from the first batch's tiles: 2 x 3 and 2 x 2 tiles, at most 6 per frame
    rows = min(tool.RANDOM_WEIGHT_ROWS, 16384 // (2 * 6))
    assert made[-1].calls == [("pick", [(40, 60, 3), (50, 33, 3)], (32, 32), 8, 1.5, rows, 4),
                              ("tiled", 2, (32, 32), 8, 1.5, 4.0, 4, 0.625), ("tiled", 1, (32, 32), 8, 1.5, 4.0, 4, 0.625)]
    for name in ("img00", "img01", "img02"):
        assert open(tmp_path / "out" / (name + ".txt")).read() == "1,2,10,20,0.2500,3,-1,-1\n"
    out = capsys.readouterr().out
    assert "3 frames, 3 boxes" in out and "32x32 tiles" in out and "score threshold 0.625" in out


# --------------------------------------------------------------------------------------------------------------------
# evaluate_batched
# --------------------------------------------------------------------------------------------------------------------
def _operator_stub(tmp_path, val, calls):
    from rrnet_amd.datasets.transforms import Compose, Normalize, ToTensor
    from rrnet_amd.operators.retinanet_operator import RetinaNetOperator
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    val = dict(val, model_path="ckp.pth", result_dir=str(tmp_path / "results"), num_workers=2,
               transforms=Compose([ToTensor(), Normalize(mean, std)]))
    cfg = SimpleNamespace(num_classes=10, Val=SimpleNamespace(**val), Distributed=SimpleNamespace(rank=0, world_size=1))
    inner = SimpleNamespace(load_state_dict=lambda sd: calls.append(("load", sd)))
    model = SimpleNamespace(module=inner, eval=lambda: calls.append(("eval",)))

    class _Loader:
        dataset = _Frames([(40, 60), (50, 33), (40, 60), (40, 60), (50, 33)])

        def __iter__(self):
            for i in range(0, 5, 2):
                yield SimpleNamespace(cuda=lambda: None), None, self.dataset.mdf[i:i + 2]

        def __len__(self):
            return 3

    op = SimpleNamespace(cfg=cfg, model=model, validation_loader=_Loader(), main_proc_flag=False)
    op.evaluate_images = lambda imgs: (calls.append(("per_frame",)), [torch.tensor([[1., 2., 3., 4., .5, 6.]])] * 2)[1]
    op.save_result = RetinaNetOperator.save_result
    op.write_results = RetinaNetOperator.write_results
    op.make_anchor = lambda size: (calls.append(("anchors", tuple(int(s) for s in size))), (torch.zeros((9, 4)),))[1]
    op.evaluate_batched = lambda n, d=None: (calls.append(("batched", n)), RetinaNetOperator.evaluate_batched(op, n, d))[1]
    return op


def test_evaluate_batched_routes_on_the_two_config_keys(tmp_path, monkeypatch):
    import rrnet_amd.datasets.frames as frames_mod
    import rrnet_amd.inference as inference
    from rrnet_amd.configs.retinanet_config import Config
    from rrnet_amd.operators.retinanet_operator import RetinaNetOperator
    for key in ("tile", "tile_overlap", "tile_zoom", "tile_margin", "device_batch"):
        assert not hasattr(Config.Val, key)                                    # the config modules do not carry the keys
    monkeypatch.setattr(torch, "load", lambda *a, **k: {"w": 1})
    monkeypatch.setattr(frames_mod, "SizeBucketedFrames", functools.partial(frames_mod.SizeBucketedFrames, device="cpu"))
    monkeypatch.setattr(frames_mod, "OrderedFrames", functools.partial(frames_mod.OrderedFrames, device="cpu"))
    seen = []

    def fake_tiled(model, frames, mean, std, anchors, *, tile, overlap, zoom=1.0, margin=0.0, tile_batch=8, score_thr=0.1,
                   nms_thresh=0.3, timer=None):
        ids = [int(f[0, 0, 0]) for f in frames]
        seen.append(("tiled", ids, tile, overlap, zoom, margin, score_thr, nms_thresh, tuple(anchors.shape)))
        return torch.tensor([[v + 0.75, 1.0, 3.0, 4.0, 0.5, 2.0] for v in ids]), torch.arange(len(ids) + 1, dtype=torch.int32)

    def fake_frames(model, frames_u8, mean, std, anchors, *, score_thr=0.1, nms_thresh=0.3, timer=None):
        ids = [int(frames_u8[j, 0, 0, 0]) for j in range(frames_u8.shape[0])]
        seen.append(("frames", ids))
        return torch.tensor([[v + 0.75, 1.0, 3.0, 4.0, 0.5, 2.0] for v in ids]), torch.arange(len(ids) + 1, dtype=torch.int32)

    monkeypatch.setattr(inference, "detect_tiled_retinanet", fake_tiled)
    monkeypatch.setattr(inference, "detect_frames_retinanet", fake_frames)

    def run(val):
        del seen[:]
        calls = []
        RetinaNetOperator.evaluation_process(_operator_stub(tmp_path, val, calls))
        return calls, list(seen)

    calls, got = run(dict(tile=32))                                            # tile without device_batch: the per-frame loop
    assert not got and [c[0] for c in calls].count("per_frame") == 3
    calls, got = run(dict(tile=32, device_batch=0))
    assert not got and [c[0] for c in calls].count("per_frame") == 3
    calls, got = run(dict(device_batch=2))                                     # device_batch without tile: whole frames, bucketed
    assert [g[:2] for g in got] == [("frames", [0, 2]), ("frames", [1, 4]), ("frames", [3])]
    calls, got = run(dict(device_batch=2, tile=None))
    assert [g[0] for g in got] == ["frames"] * 3
    calls, got = run(dict(device_batch=2, tile=32))                            # both: tiled, file order, default companions
    assert got == [("tiled", ids, (32, 32), 8, 1.0, 0.0, 0.1, 0.3, (9, 4)) for ids in ([0, 1], [2, 3], [4])]
    assert [c[1] for c in calls if c[0] == "anchors"] == [(32, 32)]            # the anchors of the model's input size, once
    calls, got = run(dict(device_batch=3, tile=(32, 24), tile_overlap=4, tile_zoom=1.5, tile_margin=2.0))
    assert got == [("tiled", ids, (32, 24), 4, 1.5, 2.0, 0.1, 0.3, (9, 4)) for ids in ([0, 1, 2], [3, 4])]
    assert [c[1] for c in calls if c[0] == "anchors"] == [(48, 36)]
    out = tmp_path / "results"
    for v in range(5):
        assert open(out / ("img%02d.txt" % v)).read() == "%d,1,3,4,0.5000,2,-1,-1\n" % v
