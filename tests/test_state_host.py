"""Host side of the full-state checkpoints (rrnet_amd/checkpoint.py), no GPU: the numpy statement of the digest that the
GPU tests hold rr_state_snapshot against, the choice of a state file, the layout fingerprint and its message, loader
positions (seek / position) of the host augmentation loader over the committed demo frame, and tools/train.py's
arguments."""
import os

import numpy as np
import pytest
import torch

import augment_cases as C
from rrnet_amd import checkpoint as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_digest_reference_against_hand_computed_records():
    """Nine words, chunk 4: two full records and a one-word record, the sums worked out by hand; then a chunk long
    enough for d1 to wrap around 2^64."""
    M = 0xffffffff
    u = np.array([1, 2, 3, 4,   M, M, 0x7f800000, 0xffc00001,   0x80000000], dtype=np.uint32)
    d = K.digest_reference(u, 4)
    assert d.dtype == np.uint64 and d.shape == (3, 3)
    # chunk 0: 1+2+3+4 = 10; 1*1 + 2*2 + 3*3 + 4*4 = 30; no exponent of all ones
    assert [int(v) for v in d[0]] == [10, 30, 0]
    # chunk 1: +Inf (0x7f800000) and a NaN with a payload (0xffc00001) count; the all-ones words have the exponent set too
    d0 = (M + M + 0x7f800000 + 0xffc00001) % 2 ** 64
    d1 = (1 * M + 2 * M + 3 * 0x7f800000 + 4 * 0xffc00001) % 2 ** 64
    assert [int(v) for v in d[1]] == [d0, d1, 4]
    assert d0 == 0x37f3fffff and d1 == 0x87d800001             # 3 * 0xffffffff + 3 * 0x7f800000 + 4 * 0xffc00001
    # chunk 2: -0.0 alone, at j = 0
    assert [int(v) for v in d[2]] == [0x80000000, 0x80000000, 0]
    # a float32 view is read as its bits
    assert np.array_equal(K.digest_reference(u.view(np.float32), 4), d)
    # a chunk of 2^17 all-ones words: d1 = (2^32 - 1) * 2^17 * (2^17 + 1) / 2 > 2^64 wraps
    n, ch = 140000, 131072
    ones = np.full(n, M, dtype=np.uint32)
    w = K.digest_reference(ones, ch)
    assert M * (ch * (ch + 1) // 2) > 2 ** 64
    assert int(w[0, 0]) == ch * M and int(w[0, 1]) == (M * (ch * (ch + 1) // 2)) % 2 ** 64 and int(w[0, 2]) == ch
    assert int(w[1, 0]) == (n - ch) * M and int(w[1, 2]) == n - ch
    assert K.digest_reference(np.zeros(0, np.uint32), 4).shape == (0, 3)


def test_latest_state_orders_by_step_and_ignores_tmp(tmp_path):
    assert K.latest_state(str(tmp_path)) is None and K.list_states(str(tmp_path)) == []
    for name in ("state-9.pth", "state-10.pth", "state-4999.pth", "state-20000.pth.tmp", "ckp-99999.pth", "state-x.pth",
                 "state-7.pth.bak"):
        (tmp_path / name).write_bytes(b"")
    assert K.latest_state(str(tmp_path)) == str(tmp_path / "state-4999.pth")           # numeric order, not 9 > 4999
    assert [s for s, _ in K.list_states(str(tmp_path))] == [4999, 10, 9]
    assert K.latest_state(str(tmp_path / "missing")) is None


def _fingerprint(stacks, width=8):
    """A small module tree through the real FlatParams (CPU tensors are accepted)."""
    from rrnet_amd.flat import FlatParams
    layers = []
    for s in range(stacks):
        layers += [torch.nn.Conv2d(3 if s == 0 else width, width, 3), torch.nn.BatchNorm2d(width)]
    m = torch.nn.Sequential(*layers, torch.nn.Conv2d(width, 5, 1))
    return K.layout_fingerprint(m, FlatParams(m)), m


def test_fingerprint_comparison_names_the_first_difference():
    a, m = _fingerprint(1)
    assert a["model"] == "Sequential" and a["entries"][0] == ("0.weight", (8, 3, 3, 3), 0)
    assert a["entries"][1] == ("0.bias", (8,), 216) and a["numel"] == sum((p.numel() + 3) // 4 * 4 for p in m.parameters())
    K.compare_fingerprint(a, _fingerprint(1)[0])                    # equal layouts pass
    K.compare_fingerprint(a, {"model": a["model"], "numel": a["numel"], "entries": [list(e) for e in a["entries"]]})
    b, _ = _fingerprint(2)
    with pytest.raises(K.StateError) as e:
        K.compare_fingerprint(a, b)
    # 0.weight, 0.bias, 1.weight, 1.bias agree; #4 is the head `2.weight` [5,8,1,1] in one, the second conv in the other
    msg = str(e.value)
    assert "#4" in msg and "2.weight" in msg and "(5, 8, 1, 1)" in msg and "(8, 8, 3, 3)" in msg
    c, _ = _fingerprint(1, width=12)
    with pytest.raises(K.StateError) as e:
        K.compare_fingerprint(a, c)
    assert "#0" in str(e.value) and "0.weight" in str(e.value)
    short = dict(a, entries=a["entries"][:-1])
    with pytest.raises(K.StateError) as e:
        K.compare_fingerprint(a, short)
    assert "2.bias" in str(e.value) and "saved" in str(e.value)
    with pytest.raises(K.StateError) as e:
        K.compare_fingerprint(dict(a, model="RRNet"), a)
    assert "RRNet" in str(e.value)


def _chain(crop):
    from rrnet_amd.datasets.transforms import (Compose, HorizontalFlip, MaskIgnore, MultiScale, Normalize, RandomCrop,
                                               ToHeatmap, ToTensor)
    return Compose([MultiScale(scale=(1, 1.15, 1.25, 1.35, 1.5)), ToTensor(), MaskIgnore(C.MEAN), HorizontalFlip(),
                    RandomCrop(crop), Normalize(C.MEAN, C.STD), ToHeatmap(scale_factor=4)])


def _host_collate(annos_list, height, width, scale_factor=4, num_classes=10, device="cpu"):
    """collate_ctnet_device without its kernel: the padded annotations; the targets (a function of them, built by
    rr_ctnet_targets on the device) are left out.  What seek() must reproduce -- decisions, pixels, annotations -- is
    all made on the host."""
    m = max(int(a.size(0)) for a in annos_list)
    annos = torch.zeros(len(annos_list), m, 8)
    for i, a in enumerate(annos_list):
        annos[i, :a.size(0)] = a[:, :8]
    return annos, None, None, None, None, None


def test_host_augment_loader_seek_and_position(tmp_path, monkeypatch):
    """After seek(3) the next two batches are batches 3 and 4 of a fresh loader, bit for bit; position() counts the
    batches handed out.  One frame, batch 2: every sample of these batches lies in another epoch."""
    from rrnet_amd.datasets import augment as A
    from rrnet_amd.datasets import synthetic
    from rrnet_amd.datasets.drones_det import DronesDET
    monkeypatch.setattr(synthetic, "collate_ctnet_device", _host_collate)
    root = C.write_dataset(str(tmp_path), splits=("train",), extra=0)
    chain = _chain((96, 128))
    ds = DronesDET(root, chain, "train")
    assert len(ds) == 1
    p = A.chain_params(chain)
    fresh = A.HostAugmentLoader(ds, p, 2, seed=5, num_workers=2, device="cpu")
    moved = A.HostAugmentLoader(ds, p, 2, seed=5, num_workers=2, device="cpu")
    try:
        assert fresh.position() == 0
        ref = [fresh.get_batch() for _ in range(5)]
        assert fresh.position() == 5
        assert not torch.equal(ref[3][0], ref[4][0]) and not torch.equal(ref[0][0], ref[3][0])
        first = moved.get_batch()                         # futures for batches 1 and 2 are queued now
        assert torch.equal(first[0].view(torch.int32), ref[0][0].view(torch.int32)) and moved.position() == 1
        moved.seek(3)
        assert moved.position() == 3 and moved.futures == {}
        for want in ref[3:5]:
            got = moved.get_batch()
            assert got[0].shape == (2, 3, 96, 128)
            assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
            assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32)) and got[7] == want[7]
        assert moved.position() == 5
        moved.seek(0)                                     # and backwards
        assert torch.equal(moved.get_batch()[0].view(torch.int32), ref[0][0].view(torch.int32))
    finally:
        fresh.close()
        moved.close()


def test_train_tool_arguments_set_the_config_keys():
    """tools/train.py: parsing and configuring only; no operator is built."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("rr_tools_train", os.path.join(ROOT, "tools", "train.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    from rrnet_amd.configs.rrnet_config import Config
    from rrnet_amd.datasets.transforms import RandomCrop
    cfg = T.configure(T.parse(["--config", "rrnet_config", "--data-root", "/d", "--iters", "12", "--batch", "3", "--crop", "128",
                               "192", "--backbone", "hourglass_tiny", "--bf16", "--full-state", "--resume", "auto",
                               "--checkpoint-interval", "4", "--keep-states", "3"]))
    assert (cfg.data_root, cfg.Train.iter_num, cfg.Train.batch_size, cfg.Train.crop_size) == ("/d", 12, 3, (128, 192))
    assert cfg.Model.backbone == "hourglass_tiny" and cfg.Model.bf16 is True
    assert cfg.Train.full_state is True and cfg.Train.resume == "auto" and cfg.Train.checkpoint_interval == 4
    assert cfg.Train.keep_states == 3 and (cfg.Distributed.gpu_id, cfg.Distributed.world_size) == (0, 1)
    assert [(t.h, t.w) for t in cfg.Train.transforms.transforms if isinstance(t, RandomCrop)] == [(128, 192)]
    # the module's Config is not touched, and the keys stay absent unless asked for
    assert Config.Train.iter_num == 100000 and not hasattr(Config.Train, "full_state")
    assert [(t.h, t.w) for t in Config.Train.transforms.transforms if isinstance(t, RandomCrop)] == [(512, 512)]
    plain = T.configure(T.parse(["--config", "centernet_config"]))
    assert getattr(plain.Train, "full_state", None) is None and getattr(plain.Train, "resume", None) is None
    assert T.configure(T.parse(["--resume", "/x/state-9.pth"])).Train.resume == "/x/state-9.pth"
    with pytest.raises(SystemExit):
        T.configure(T.parse(["--config", "centernet_config", "--bf16"]))
    with pytest.raises(SystemExit):
        T.configure(T.parse(["--config", "nope"]))
