"""Host-side tests of CenterNet detection on raw frames: the result writer, the opt-in batched validation driver, the
command's argument handling and detect_frames_centernet's argument checks.  No GPU."""
import functools
import importlib.util
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_write_results_equals_save_result_byte_for_byte(tmp_path):
    from rrnet_amd.operators.centernet_operator import CenterNetOperator
    rng = np.random.default_rng(6)
    special = torch.tensor([[0.5, 1.5, 2.5, 3.5, 0.12345, 1.0],               # halves round to even: 0, 2, 2, 4
                            [-3.5, -0.0, 10.5, 20.49999, 0.00005, 10.0],     # negatives clamp; -0.0 passes as 0
                            [-0.4, 0.4, -2.5, 7.5, 0.99995, 4.0],
                            [16777216.0, 16777218.0, 33554432.0, 16777216.0, 0.00015, 2.0],      # >= 2^24: exact integers
                            [2147483648.0, 1.0, 4294967296.0, 3.0, 1.0, 9.0],
                            [100.6, 50.2, 40.4, 20.1, 0.12344999, 3.0],      # x2 < x, y2 < y: negative third / fourth field
                            [7.0, 7.0, 7.0, 7.0, 0.5, 5.0]], dtype=torch.float32)
    rows = torch.from_numpy(np.concatenate([rng.uniform(-5, 2000, (200, 4)), rng.uniform(0, 1, (200, 1)),
                                            rng.integers(1, 11, (200, 1))], 1).astype(np.float32))
    halves = torch.from_numpy(np.concatenate([rng.integers(-4, 4000, (200, 4)) + 0.5, rng.uniform(0, 1, (200, 1)),
                                              rng.integers(1, 11, (200, 1))], 1).astype(np.float32))
    for i, block in enumerate((special, rows, halves, torch.zeros((0, 6)), special[:1])):
        a, b = str(tmp_path / ("a%d.txt" % i)), str(tmp_path / ("b%d.txt" % i))
        CenterNetOperator.save_result(a, block.clone())
        CenterNetOperator.write_results(b, block)
        assert open(a, 'rb').read() == open(b, 'rb').read()
        CenterNetOperator.write_results(b, block.numpy())                     # arrays as the batched driver hands them
        assert open(a, 'rb').read() == open(b, 'rb').read()
    text = open(str(tmp_path / "a0.txt")).read().splitlines()
    assert text[0] == "0,2,2,2,0.1235,1,-1,-1" and text[5] == "101,50,-61,-30,0.1234,3,-1,-1"


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
        return Image.fromarray(np.full((h, w, 3), i, np.uint8)), None, self.mdf[i]


def _operator_stub(tmp_path, val, calls):
    from rrnet_amd.datasets.transforms import Compose, Normalize, ToTensor
    from rrnet_amd.operators.centernet_operator import CenterNetOperator
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
    op.save_result = lambda path, rows: (calls.append(("save", os.path.basename(path))),
                                         CenterNetOperator.save_result(path, rows))[1]
    op.write_results = CenterNetOperator.write_results
    op.evaluate_batched = lambda n, k=250: (calls.append(("batched", n)), CenterNetOperator.evaluate_batched(op, n, k))[1]
    return op


def test_evaluation_process_default_is_the_per_frame_path(tmp_path, monkeypatch, capsys):
    from rrnet_amd.operators.centernet_operator import CenterNetOperator
    monkeypatch.setattr(torch, "load", lambda *a, **k: {"w": 1})
    for val, warns in ((dict(scales=[1, 1.5], auto_test=True), False),
                       (dict(scales=[1, 1.5], auto_test=True, device_batch=0), False),
                       (dict(scales=[1] * 33, auto_test=True, device_batch=2), True)):   # 33 x 2 x 250 rows: falls back
        calls = []
        op = _operator_stub(tmp_path, val, calls)
        CenterNetOperator.evaluation_process(op)
        assert [c[0] for c in calls].count("per_frame") == 5 and not any(c[0] == "batched" for c in calls)
        assert sorted(c[1] for c in calls if c[0] == "save") == ["img%02d.txt" % i for i in range(5)]
        assert ("load", {"w": 1}) in calls and ("eval",) in calls
        out = capsys.readouterr().out
        if warns:
            assert "warning: Val.device_batch ignored" in out and "16384" in out
        else:
            assert "warning" not in out


def test_evaluation_process_device_batch_writes_the_detectors_rows(tmp_path, monkeypatch):
    import rrnet_amd.datasets.frames as frames_mod
    import rrnet_amd.inference as inference
    from rrnet_amd.operators.centernet_operator import CenterNetOperator
    monkeypatch.setattr(torch, "load", lambda *a, **k: {"w": 1})
    monkeypatch.setattr(frames_mod, "SizeBucketedFrames", functools.partial(frames_mod.SizeBucketedFrames, device="cpu"))
    seen = []

    def fake_detect(model, frames_u8, scales, mean, std, *, nms, k=250, scale_factor=4, num_classes=10, **kw):
        """Frame with pixel value v gets v + 1 rows whose x is v + 0.5: tells the frames and their row ranges apart."""
        ids = [int(frames_u8[j, 0, 0, 0]) for j in range(frames_u8.shape[0])]
        seen.append((ids, list(scales), nms, tuple(mean), k))
        rows = [[v + 0.5, -1.0, v + 10.5 + r, 3.0, 0.5 / (r + 1), 1 + v] for v in ids for r in range(v + 1)]
        off = np.cumsum([0] + [v + 1 for v in ids]).astype(np.int32)
        return torch.tensor(rows, dtype=torch.float32).view(-1, 6), torch.from_numpy(off)

    monkeypatch.setattr(inference, "detect_frames_centernet", fake_detect)
    calls = []
    op = _operator_stub(tmp_path, dict(scales=[1, 1.25], auto_test=True, device_batch=2), calls)
    CenterNetOperator.evaluation_process(op)
    assert ("batched", 2) in calls and not any(c[0] == "per_frame" for c in calls)
    assert [ids for ids, *_ in seen] == [[0, 2], [1, 4], [3]]
    assert all(s[1] == [1, 1.25] and s[2] is False and s[3] == (0.485, 0.456, 0.406) and s[4] == 250 for s in seen)
    out = tmp_path / "results"
    assert sorted(os.listdir(out)) == ["img%02d.txt" % i for i in range(5)]
    for v in range(5):
        x0 = int(np.rint(np.float32(v + 0.5)))
        lines = open(out / ("img%02d.txt" % v)).read().splitlines()
        assert lines == ['%d,%d,%d,%d,%.4f,%d,-1,-1' % (x0, 0, int(np.rint(np.float32(v + 10.5 + r))) - x0, 3,
                                                        float(np.float32(0.5 / (r + 1))), 1 + v) for r in range(v + 1)]


def _detect_tool():
    spec = importlib.util.spec_from_file_location("detect_tool", os.path.join(ROOT, "tools", "detect.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_detect_command_accepts_centernet_and_passes_flip(tmp_path, monkeypatch, capsys):
    import rrnet_amd.datasets.frames as frames_mod
    import rrnet_amd.inference as inference
    tool = _detect_tool()
    cfg = tool.load_config("centernet_config")                                # accepted
    assert cfg.Model.backbone == "hourglass" and cfg.Val.auto_test is True
    with pytest.raises(SystemExit, match="unknown config"):
        tool.load_config("no_such_config")
    base = ["--config", "centernet_config", "--images", str(tmp_path), "--out", str(tmp_path / "out"), "--random-weights"]
    with pytest.raises(SystemExit, match="bf16"):
        tool.main(base + ["--bf16"])
    made = []

    class FakeDetector:
        def __init__(self, cfg, checkpoint=None, device=None):
            made.append(self)
            self.calls = []

        def detect(self, frames_u8, scales=None, nms=None, flip=True, k=250, timer=None):
            self.calls.append((tuple(scales), nms, flip))
            n = frames_u8.shape[0]
            rows = torch.tensor([[1.5, 2.5, 10.5, 20.5, 0.25, 3.0]] * n)
            return rows, torch.arange(n + 1, dtype=torch.int32)

    def rrnet_detector(*a, **k):
        raise AssertionError("the RRNet detector was built for a CenterNet config")

    monkeypatch.setattr(inference, "CenterNetFrameDetector", FakeDetector)
    monkeypatch.setattr(inference, "Detector", rrnet_detector)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(frames_mod, "FrameFolder", lambda path: _Frames([(4, 6), (4, 6), (5, 3)]))
    monkeypatch.setattr(frames_mod, "SizeBucketedFrames", functools.partial(frames_mod.SizeBucketedFrames, device="cpu"))
    for extra, flip in (([], True), (["--flip"], True), (["--no-flip"], False)):
        tool.main(base + ["--scales", "1,1.5", "--batch", "2"] + extra)
        assert made[-1].calls == [((1.0, 1.5), False, flip), ((1.0, 1.5), False, flip)]      # auto_test=True: raw
        for name in ("img00", "img01", "img02"):
            assert open(tmp_path / "out" / (name + ".txt")).read() == "2,2,8,18,0.2500,3,-1,-1\n"
    assert "3 frames, 3 boxes" in capsys.readouterr().out
    with pytest.raises(SystemExit, match="rows per frame"):
        tool.main(base + ["--scales", ",".join(["1"] * 33)])
    tool.main(base + ["--scales", ",".join(["1"] * 33), "--no-flip"])          # 33 x 250 fits


def test_detect_frames_centernet_argument_checks():
    from rrnet_amd import _C, inference
    u8 = torch.zeros((1, 8, 8, 3), dtype=torch.uint8)
    mean = std = (0.5, 0.5, 0.5)
    with pytest.raises(_C.RRNetHipError, match="cpu"):
        inference.detect_frames_centernet(None, u8, [1], mean, std, nms=True)
    with pytest.raises(TypeError, match="uint8"):
        inference.detect_frames_centernet(None, u8.float(), [1], mean, std, nms=True)
    with pytest.raises(TypeError, match="uint8"):
        inference.detect_frames_centernet(None, u8.numpy(), [1], mean, std, nms=True)
    with pytest.raises(ValueError, match="limit 16384"):
        inference.detect_frames_centernet(None, u8, [1] * 33, mean, std, nms=True)        # 33 x 2 x 250 = 16500 rows
    with pytest.raises(_C.RRNetHipError, match="cpu"):
        inference.detect_frames_centernet(None, u8, [1] * 32, mean, std, nms=True)        # 16000 rows fit: the next check
    with pytest.raises(ValueError, match="limit 16384"):
        inference.detect_frames_centernet(None, u8, [1], mean, std, nms=False, k=8193)    # 1 x 2 x 8193
    with pytest.raises(_C.RRNetHipError, match="cpu"):
        inference.detect_frames_centernet(None, u8, [1], mean, std, nms=False, flip=False, k=8193)
    with pytest.raises(ValueError, match="limit 16384"):
        inference.detect_frames_centernet(None, u8, [], mean, std, nms=True)
    with pytest.raises(ValueError):
        inference.detect_frames_centernet(None, torch.zeros((8, 8, 3), dtype=torch.uint8), [1], mean, std, nms=True)
