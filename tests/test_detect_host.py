"""Host-side tests of detection on raw frames: the result writer, the size-bucket planner, the opt-in batched validation
driver and detect_frames' argument checks.  No GPU."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch


def test_write_results_equals_save_result_byte_for_byte(tmp_path):
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    rng = np.random.default_rng(5)
    special = torch.tensor([[-3.5, 2.25, 10.0, 20.0, 0.12345, 1.0],          # negative coordinate: clamped
                            [1e-7, 1e4, 1e-7, 1e4, 0.00005, 10.0],           # tiny and large, score at a %.4f boundary
                            [1234.56789, 0.5, 1e4 + 0.5, 3.14159274, 0.99995, 4.0],
                            [0.0, -0.0, 7.0, 7.0, 0.00015, 2.0],
                            [5.0, 5.0, -1e-7, 2.0, 0.12344999, 3.0],
                            [16777216.0, 1.0, 1.0, 1.0, 1.0, 9.0]], dtype=torch.float32)
    rows = torch.from_numpy(np.concatenate([rng.uniform(-5, 2000, (200, 4)), rng.uniform(0, 1, (200, 1)),
                                            rng.integers(1, 11, (200, 1))], 1).astype(np.float32))
    for i, block in enumerate((special, rows, torch.zeros((0, 6)), special[:1])):
        a, b = str(tmp_path / ("a%d.txt" % i)), str(tmp_path / ("b%d.txt" % i))
        RRNetOperator.save_result(a, block)
        RRNetOperator.write_results(b, block)
        assert open(a, 'rb').read() == open(b, 'rb').read()
        RRNetOperator.write_results(b, block.numpy())                        # arrays as the batched driver hands them
        assert open(a, 'rb').read() == open(b, 'rb').read()


def test_plan_buckets_emits_every_index_once_in_a_defined_order():
    from rrnet_amd.datasets.frames import plan_buckets
    A, B, C = (765, 1360), (1080, 1920), (540, 960)
    sizes = [A, B, A, A, C, B, A, A, B, A, B, B]
    plan = plan_buckets(sizes, 3)
    assert plan == [[0, 2, 3], [1, 5, 8], [6, 7, 9], [10, 11], [4]]           # full buckets as they fill; rest: A (none), B, C
    assert plan == plan_buckets(list(sizes), 3)
    rng = np.random.default_rng(1)
    pool = [A, B, C, (1, 9)]
    for batch in (1, 2, 4, 7):
        sizes = [pool[i] for i in rng.integers(0, 4, 61)]
        plan = plan_buckets(sizes, batch)
        assert sorted(i for b in plan for i in b) == list(range(61))
        first_seen = list(dict.fromkeys(sizes))
        rest = [b for b in plan if len(b) < batch]
        for b in plan:
            assert 1 <= len(b) <= batch and len({sizes[i] for i in b}) == 1 and b == sorted(b)
        # remainders come last, one per size at most, in first-seen order of the sizes
        assert plan[len(plan) - len(rest):] == rest
        assert [first_seen.index(sizes[b[0]]) for b in rest] == sorted(first_seen.index(sizes[b[0]]) for b in rest)
        assert len({sizes[b[0]] for b in rest}) == len(rest)
    assert plan_buckets([], 4) == []


class _Frames:
    """Dataset stand-in with DronesDET's load surface: frames of two sizes."""

    def __init__(self, sizes):
        self.sizes = sizes
        self.mdf = ["img%02d" % i for i in range(len(sizes))]

    def __len__(self):
        return len(self.sizes)

    def load(self, i):
        from PIL import Image
        h, w = self.sizes[i]
        arr = np.full((h, w, 3), i, np.uint8)
        return Image.fromarray(arr), None, self.mdf[i]


def test_size_bucketed_frames_follows_the_plan_and_splits_by_rank():
    from rrnet_amd.datasets.frames import SizeBucketedFrames, plan_buckets
    sizes = [(4, 6), (5, 3), (4, 6), (4, 6), (5, 3), (4, 6), (2, 2)]
    ds = _Frames(sizes)
    got = list(SizeBucketedFrames(ds, 2, num_workers=3, device="cpu"))
    plan = plan_buckets(sizes, 2)
    assert [names for _, names in got] == [[ds.mdf[i] for i in b] for b in plan]
    for (frames, names), b in zip(got, plan):
        assert frames.dtype == torch.uint8 and tuple(frames.shape) == (len(b),) + sizes[b[0]] + (3,)
        assert [int(frames[j, 0, 0, 0]) for j in range(len(b))] == b
    seen = []
    for rank in range(3):
        for _, names in SizeBucketedFrames(ds, 2, rank=rank, world_size=3, num_workers=40, device="cpu"):
            seen += names
    assert sorted(seen) == ds.mdf


def _operator_stub(tmp_path, val, calls):
    from rrnet_amd.datasets.transforms import Compose, Normalize, ToTensor
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    mean, std = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
    val = dict(val, model_path="ckp.pth", result_dir=str(tmp_path / "results"), num_workers=2,
               transforms=Compose([ToTensor(), Normalize(mean, std)]))
    cfg = SimpleNamespace(num_classes=10, Val=SimpleNamespace(**val), Train=SimpleNamespace(scale_factor=4),
                          Distributed=SimpleNamespace(rank=0, world_size=1))
    inner = SimpleNamespace(load_state_dict=lambda sd: calls.append(("load", sd)))
    model = SimpleNamespace(module=inner, eval=lambda: calls.append(("eval",)))

    class _Img:
        def cuda(self):
            return self

    class _Loader:
        dataset = _Frames([(4, 6), (5, 3), (4, 6), (4, 6), (5, 3)])

        def __iter__(self):
            for n in self.dataset.mdf:
                yield _Img(), None, [n]

    op = SimpleNamespace(cfg=cfg, model=model, validation_loader=_Loader())
    op.evaluate_images = lambda imgs: (calls.append(("per_frame",)), torch.tensor([[1., 2., 3., 4., .5, 6.]]))[1]
    op.save_result = lambda path, rows: (calls.append(("save", os.path.basename(path))), RRNetOperator.save_result(path, rows))[1]
    op.write_results = RRNetOperator.write_results
    op.evaluate_batched = lambda n, k=1500: (calls.append(("batched", n)), RRNetOperator.evaluate_batched(op, n, k))[1]
    return op


def test_evaluation_process_default_is_the_per_frame_path(tmp_path, monkeypatch):
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    monkeypatch.setattr(torch, "load", lambda *a, **k: {"w": 1})
    for val in (dict(scales=[1, 1.5], auto_test=False), dict(scales=[1, 1.5], auto_test=False, device_batch=0),
                dict(scales=[1] * 11, auto_test=False, device_batch=2)):      # 11 x 1500 rows: falls back, with a warning
        calls = []
        op = _operator_stub(tmp_path, val, calls)
        RRNetOperator.evaluation_process(op)
        assert [c[0] for c in calls].count("per_frame") == 5 and not any(c[0] == "batched" for c in calls)
        assert sorted(c[1] for c in calls if c[0] == "save") == ["img%02d.txt" % i for i in range(5)]
        assert ("load", {"w": 1}) in calls and ("eval",) in calls


def test_evaluation_process_device_batch_writes_the_detectors_rows(tmp_path, monkeypatch, capsys):
    import rrnet_amd.datasets.frames as frames_mod
    import rrnet_amd.inference as inference
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    monkeypatch.setattr(torch, "load", lambda *a, **k: {"w": 1})
    monkeypatch.setattr(frames_mod, "SizeBucketedFrames", functools.partial(frames_mod.SizeBucketedFrames, device="cpu"))
    seen = []

    def fake_detect(model, frames_u8, scales, mean, std, *, nms, k=1500, scale_factor=4, num_classes=10, **kw):
        """Frame with pixel value v gets v + 1 rows whose x is v: tells the frames and their row ranges apart."""
        ids = [int(frames_u8[j, 0, 0, 0]) for j in range(frames_u8.shape[0])]
        seen.append((ids, list(scales), nms, tuple(mean), tuple(std)))
        rows = [[float(v), -1.0, 2.0 + r, 3.0, 0.5 / (r + 1), 1 + v] for v in ids for r in range(v + 1)]
        off = np.cumsum([0] + [v + 1 for v in ids]).astype(np.int32)
        return torch.tensor(rows, dtype=torch.float32).view(-1, 6), torch.from_numpy(off)

    monkeypatch.setattr(inference, "detect_frames", fake_detect)
    calls = []
    op = _operator_stub(tmp_path, dict(scales=[1, 1.25], auto_test=True, device_batch=2), calls)
    RRNetOperator.evaluation_process(op)
    assert ("batched", 2) in calls and not any(c[0] == "per_frame" for c in calls)
    assert [ids for ids, *_ in seen] == [[0, 2], [1, 4], [3]]
    assert all(s[1] == [1, 1.25] and s[2] is False and s[3] == (0.485, 0.456, 0.406) for s in seen)
    out = tmp_path / "results"
    assert sorted(os.listdir(out)) == ["img%02d.txt" % i for i in range(5)]
    for v in range(5):
        lines = open(out / ("img%02d.txt" % v)).read().splitlines()
        assert lines == ['%f,%f,%f,%f,%.4f,%d,-1,-1' % (v, 0.0, 2.0 + r, 3.0, float(np.float32(0.5 / (r + 1))), 1 + v)
                         for r in range(v + 1)]


def test_detect_frames_argument_checks():
    from rrnet_amd import _C, inference
    u8 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    mean = std = (0.5, 0.5, 0.5)
    with pytest.raises(_C.RRNetHipError, match="cpu"):
        inference.detect_frames(None, u8, [1], mean, std, nms=True)
    with pytest.raises(TypeError, match="uint8"):
        inference.detect_frames(None, u8.float(), [1], mean, std, nms=True)
    with pytest.raises(ValueError, match="limit 16384"):
        inference.detect_frames(None, u8, [1] * 11, mean, std, nms=True)      # 11 x 1500 = 16500 rows
    with pytest.raises(ValueError, match="limit 16384"):
        inference.detect_frames(None, u8, [1, 1.5], mean, std, nms=False, k=8193)
    with pytest.raises(ValueError):
        inference.detect_frames(None, torch.zeros((8, 8, 3), dtype=torch.uint8), [1], mean, std, nms=True)
