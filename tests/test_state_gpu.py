"""GPU: full-state checkpoints (rrnet_amd/checkpoint.py, csrc/snapshot.hip).

  * rr_state_snapshot against the numpy statement of its digest (checkpoint.digest_reference, itself held to hand-computed
    records in tests/test_state_host.py): copy as bits, guard words, every size around the vector width, the workgroup
    width, the unrolled loop and the chunk; refusals;
  * a snapshot is of the moment it was taken, whatever the training stream does next;
  * save -> load round trip into a differently initialised operator with stale filter caches;
  * refusals: NaN in a moment buffer, a damaged file, another model;
  * the step after a resume against the same step of the uninterrupted run (child process, deterministic kernels), with
    the bounds tests/test_streams_gpu.py uses for two correct runs of one step;
  * training_process with cfg.Train.full_state / cfg.Train.resume."""
import copy
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import det_fill

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "state_resume_worker.py")
CL = torch.channels_last

SIZES = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2055, 70001)
PLANTED = (0x7fc00001, 0x7f800001, 0xffa00123, 0x7f800000, 0xff800000, 0x80000000, 0x00000001)   # qNaN, sNaN, -sNaN, +-Inf, -0.0, denormal
GUARD = 0x5a5aa5a5


def _words(n, seed):
    u = np.random.default_rng([219, n, seed]).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    if n >= 256:
        at = [0, 1, n // 3, n // 2, n - 3, n - 2, n - 1]
        u[at] = np.array(PLANTED, dtype=np.uint32)
    return u


def _dev(u):
    return torch.from_numpy(u.view(np.int32).copy()).cuda().view(torch.float32)


def _u32(t):
    return t.contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _u64(d):
    return d.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("chunk", [256, 1024, 65536])
def test_snapshot_kernel_against_numpy(chunk):
    from rrnet_amd import ops
    from rrnet_amd.checkpoint import digest_reference
    for n in SIZES:
        u = _words(n, chunk)
        ref = digest_reference(u, chunk)
        assert ref.shape == ((n + chunk - 1) // chunk, 3)
        assert int(ref[:, 2].sum()) == int(np.count_nonzero((u & 0x7f800000) == 0x7f800000))
        src = _dev(u)
        buf = _dev(np.full(n + 64, GUARD, dtype=np.uint32))
        d = ops.state_snapshot(src, buf[:n], chunk)
        assert d.dtype == torch.int64 and tuple(d.shape) == ref.shape
        got = _u32(buf)
        assert np.array_equal(got[:n], u), (n, chunk)                       # bits, NaN payloads and -0.0 included
        assert np.all(got[n:] == GUARD), (n, chunk)                         # nothing behind n
        assert np.array_equal(_u64(d), ref), (n, chunk, _u64(d), ref)
        assert np.array_equal(_u64(ops.state_snapshot(src, None, chunk)), ref), (n, chunk, "digest only")
        pre = torch.empty_like(d)
        assert ops.state_snapshot(src, None, chunk, out=pre) is not None and np.array_equal(_u64(pre), ref)
        if n >= 256:
            # two unequal words of one chunk exchanged: d1 of that chunk moves, nothing else does
            c = ref.shape[0] - 1
            if n - c * chunk < 3:                                           # a last chunk too short to swap in
                c -= 1
            lo = c * chunk
            i, j = lo, lo + min(chunk, n - lo) // 2
            if u[i] == u[j]:
                j += 1
            assert lo <= i < j < min(lo + chunk, n) and u[i] != u[j]
            v = u.copy()
            v[i], v[j] = u[j], u[i]
            dv = _u64(ops.state_snapshot(_dev(v), None, chunk))
            assert np.array_equal(dv, digest_reference(v, chunk))
            diff = dv != ref
            assert diff[c, 1] and int(diff.sum()) == 1, (n, chunk, diff)


def test_snapshot_kernel_edges_and_refusals():
    from rrnet_amd import _C, ops
    src = _dev(_words(1024, 0))
    empty = ops.state_snapshot(src[:0], None, 256)
    assert tuple(empty.shape) == (0, 3) and empty.dtype == torch.int64
    assert tuple(ops.state_snapshot(src, src.new_empty(8), 256, n=0).shape) == (0, 3)
    buf = _dev(np.full(1024 + 64, GUARD, dtype=np.uint32))
    big = _dev(_words(1032, 1))
    for kw, what in ((dict(src=src, chunk=6), "chunk"), (dict(src=src, chunk=0), "chunk"), (dict(src=src, chunk=256, n=-4), "negative"),
                     (dict(src=big[1:1025], chunk=256), "aligned")):
        with pytest.raises(_C.RRNetHipError) as e:
            ops.state_snapshot(kw.pop("src"), buf[:1024], **kw)
        assert what in str(e.value), str(e.value)
    with pytest.raises(_C.RRNetHipError):
        ops.state_snapshot(src, buf[1:1025], 256)                            # misaligned destination
    torch.cuda.synchronize()
    assert np.all(_u32(buf) == GUARD)
    with pytest.raises(_C.RRNetHipError):
        ops.state_snapshot(src.cpu(), None, 256)


# ---------------------------------------------------------------------------------------------------------------------
def _ct_cfg(stacks):
    from types import SimpleNamespace
    return SimpleNamespace(num_classes=10, Model=SimpleNamespace(num_stacks=stacks, backbone="hourglass_tiny",
                           nms_type_for_stage1="nms", nms_per_class_for_stage1=True))


def _ct_model(stacks=1, seed=11):
    """The tiny CenterNet of tests/test_train_gpu.py (_model)."""
    from rrnet_amd.models.centernet import CenterNet
    m = CenterNet(_ct_cfg(stacks))
    m.load_state_dict(det_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed))
    return m.cuda().to(memory_format=CL).train()


def _ct_loss(model, x):
    hms, whs, regs = model(x)
    return (hms[0] ** 2).mean() + whs[0].abs().mean() + (regs[0] ** 2).mean()


def test_snapshot_is_of_the_moment_it_was_taken(tmp_path):
    """save_state returns after enqueueing; two optimizer steps follow on the same stream at once and rewrite all three
    buffers while the copy to the host may still be running.  The file holds the buffers as they were at the call."""
    from rrnet_amd.checkpoint import StateWriter
    from rrnet_amd.flat import FlatAdam
    m = _ct_model()
    opt = FlatAdam(m, lr=1e-2)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(0)).cuda()
    opt.zero_grad()
    _ct_loss(m, x).backward()
    opt.step()                                            # non-zero moments
    live = (opt.fp.flat, opt.exp_avg, opt.exp_avg_sq)
    before = [t.clone() for t in live]
    w = StateWriter(m, opt, str(tmp_path))
    w.save_state(0)
    opt.step()
    opt.step()
    w.close()
    assert w.warnings == [] and sorted(os.listdir(str(tmp_path))) == ["state-0.pth"]
    sd = torch.load(str(tmp_path / "state-0.pth"), map_location="cpu", weights_only=False)
    assert sd["format"] == 1 and sd["step"] == 0 and sd["step_count"] == 1 and sd["lr"] == 1e-2
    for name, b, l in zip(("flat", "exp_avg", "exp_avg_sq"), before, live):
        assert sd[name].dtype == torch.float32 and sd[name].numel() == opt.fp.numel
        assert np.array_equal(_u32(sd[name]), _u32(b)), name
        assert not np.array_equal(_u32(sd[name]), _u32(l)), name
    assert int(sd["digests"][:, :, 2].sum()) == 0 and sd["digests"].shape[0] == 3


def test_state_of_another_model_is_refused(tmp_path):
    """A state saved from num_stacks=1 does not load into num_stacks=2: the error names the first differing parameter and
    nothing is scattered into the live buffers."""
    from rrnet_amd.checkpoint import StateError, StateWriter, layout_fingerprint, load_state
    from rrnet_amd.flat import FlatAdam
    m1 = _ct_model(1)
    o1 = FlatAdam(m1, lr=1e-3)
    w = StateWriter(m1, o1, str(tmp_path))
    w.save_state(7)
    w.close()
    m2 = _ct_model(2)
    o2 = FlatAdam(m2, lr=1e-3)
    f1, f2 = layout_fingerprint(m1, o1.fp), layout_fingerprint(m2, o2.fp)
    first = next((i for i, (a, b) in enumerate(zip(f1["entries"], f2["entries"])) if a != b), len(f1["entries"]))
    assert first < len(f1["entries"])
    keep = o2.fp.flat.clone()
    with pytest.raises(StateError) as e:
        load_state(str(tmp_path / "state-7.pth"), m2, o2)
    msg = str(e.value)
    assert "#%d" % first in msg and f1["entries"][first][0] in msg and f2["entries"][first][0] in msg, msg
    assert torch.equal(keep, o2.fp.flat)
    m3 = _ct_model(1, seed=12)                            # the same architecture takes it
    o3 = FlatAdam(m3, lr=5e-3)
    assert load_state(str(tmp_path / "state-7.pth"), m3, o3) == 8
    assert torch.equal(o3.fp.flat, o1.fp.flat) and o3.param_groups[0]["lr"] == 1e-3


# ---------------------------------------------------------------------------------------------------------------------
def _rr_cfg():
    from rrnet_amd.configs.rrnet_config import Config
    cfg = copy.deepcopy(Config)
    cfg.Train.batch_size = 2
    cfg.Train.crop_size = (256, 256)
    cfg.Model.backbone = "hourglass_tiny"
    cfg.Distributed.gpu_id, cfg.Distributed.rank, cfg.Distributed.world_size = 0, 0, 1
    return cfg


def _operator(seed):
    """A tiny RRNet operator with a synthetic loader of its own (make_dataloader caches loaders per configuration)."""
    from rrnet_amd.datasets import synthetic
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    saved = dict(synthetic._LOADERS)
    synthetic._LOADERS.clear()
    try:
        torch.manual_seed(seed)
        op = RRNetOperator(_rr_cfg())
    finally:
        synthetic._LOADERS.clear()
        synthetic._LOADERS.update(saved)
    op.model.train()
    return op


@pytest.fixture(scope="module")
def saved(tmp_path_factory):
    """Operator A after steps 0..2 and its state file; left unchanged by the tests that share it."""
    log_dir = str(tmp_path_factory.mktemp("state"))
    op = _operator(219)
    for step in range(3):
        op.train_step(step, op.training_loader.get_batch())
    op.save_state(2, log_dir)
    op.close_state()
    assert os.listdir(log_dir) == ["state-2.pth"]
    return op, log_dir


@pytest.fixture(scope="module")
def fresh():
    """Operator B: another initialisation, one step of its own (filter caches exist)."""
    op = _operator(7)
    op.train_step(0, op.training_loader.get_batch())
    return op


def _stale(op):
    """One more step of its own: whatever a test loaded into B is overwritten and its caches follow those weights."""
    op.train_step(0, op.training_loader.get_batch())


def test_round_trip_into_a_fresh_operator(saved, fresh):
    a, log_dir = saved
    b = fresh
    assert not torch.equal(a.optimizer.fp.flat, b.optimizer.fp.flat)
    assert b.optimizer.fp.wt_flat is not None             # B's backward filled the flipped-filter cache from B's weights
    start = b.load_state(os.path.join(log_dir, "state-2.pth"))
    assert start == 3
    for x, y in ((a.optimizer.fp.flat, b.optimizer.fp.flat), (a.optimizer.exp_avg, b.optimizer.exp_avg),
                 (a.optimizer.exp_avg_sq, b.optimizer.exp_avg_sq)):
        assert np.array_equal(_u32(x), _u32(y))
    ba, bb = dict(a.model.module.named_buffers()), dict(b.model.module.named_buffers())
    assert list(ba) == list(bb) and any(v.dtype == torch.int64 for v in bb.values())
    for k in ba:
        assert ba[k].dtype == bb[k].dtype and torch.equal(ba[k], bb[k]), k
    assert b.optimizer.step_count == a.optimizer.step_count == 3
    assert b.optimizer.param_groups[0]["lr"] == a.optimizer.param_groups[0]["lr"]
    assert b.lr_sch.state_dict() == a.lr_sch.state_dict()
    assert b.training_loader.position() == a.training_loader.position() == 3
    # the flipped-filter cache was filled from B's own weights: it must follow the loaded ones
    fa, fb = a.optimizer.fp, b.optimizer.fp
    k = next(i for i, p in enumerate(fb.params) if p.dim() == 4 and tuple(p.shape[2:]) == (3, 3))
    wt = fb.wt_view(fb.params[k])
    assert wt is not None
    want = fa.params[k].detach().flip(2, 3).permute(1, 2, 3, 0).contiguous().reshape(-1)      # wt[c][R-1-r][S-1-s][k]
    assert torch.equal(wt, want)
    _stale(b)


def test_nan_in_a_moment_buffer_is_never_written(saved, capsys):
    a, src_dir = saved
    log_dir = os.path.join(src_dir, "nan_case")
    os.makedirs(log_dir)
    shutil.copy(os.path.join(src_dir, "state-2.pth"), log_dir)
    old = open(os.path.join(log_dir, "state-2.pth"), "rb").read()
    from rrnet_amd.checkpoint import StateWriter
    w = StateWriter(a.model.module, a.optimizer, log_dir, a.lr_sch, a.training_loader)
    at = a.optimizer.fp.numel // 2
    keep = a.optimizer.exp_avg[at].clone()
    try:
        a.optimizer.exp_avg[at] = float("nan")
        w.save_state(3)
        w.close()
    finally:
        a.optimizer.exp_avg[at] = keep
    assert sorted(os.listdir(log_dir)) == ["state-2.pth"]
    assert open(os.path.join(log_dir, "state-2.pth"), "rb").read() == old
    assert len(w.warnings) == 1 and "exp_avg holds 1 NaN/Inf" in w.warnings[0] and "step 3" in w.warnings[0]
    assert "flat holds" not in w.warnings[0] and "exp_avg_sq" not in w.warnings[0]
    out = capsys.readouterr().out
    assert "warning:" in out and "exp_avg holds 1 NaN/Inf" in out


def test_damaged_file_is_refused_and_auto_falls_back(saved, fresh, capsys):
    from rrnet_amd.checkpoint import StateError, resume
    a, src_dir = saved
    b = fresh
    log_dir = os.path.join(src_dir, "flip_case")
    os.makedirs(log_dir)
    good = os.path.join(log_dir, "state-2.pth")
    bad = os.path.join(log_dir, "state-9.pth")
    shutil.copy(os.path.join(src_dir, "state-2.pth"), good)
    raw = bytearray(open(good, "rb").read())
    flat = a.optimizer.fp.flat.cpu().numpy().tobytes()
    mid = len(flat) // 2 // 4 * 4
    at = bytes(raw).find(flat[mid:mid + 256])             # the archive stores tensors uncompressed
    assert at > 0
    raw[at + 5] ^= 0x10
    open(bad, "wb").write(bytes(raw))
    (open(os.path.join(log_dir, "state-11.pth.tmp"), "wb")).close()          # a torn write: never looked at
    before = b.optimizer.fp.flat.clone()
    with pytest.raises(StateError):
        b.load_state(bad)
    assert torch.equal(before, b.optimizer.fp.flat)       # refused before anything live was touched
    capsys.readouterr()
    start = resume("auto", log_dir, b.model.module, b.optimizer, b.lr_sch, b.training_loader)
    out = capsys.readouterr().out
    assert start == 3 and "state-9.pth" in out and "warning" in out and "continuing at step 3" in out
    assert np.array_equal(_u32(b.optimizer.fp.flat), _u32(a.optimizer.fp.flat))
    empty = os.path.join(log_dir, "none")
    os.makedirs(empty)
    shutil.copy(bad, os.path.join(empty, "state-4.pth"))
    assert resume("auto", empty, b.model.module, b.optimizer, b.lr_sch, b.training_loader) == 0
    assert "starting at step 0" in capsys.readouterr().out
    _stale(b)


def test_loaders_seek_to_a_batch(tmp_path):
    """position() / seek(n) of the device-side loaders: after seek(n) the next batch is batch n of a fresh loader, bit
    for bit, with prefetches in flight."""
    from types import SimpleNamespace
    import augment_cases as C
    from rrnet_amd.datasets import augment as A
    from rrnet_amd.datasets.drones_det import DronesDET
    from rrnet_amd.datasets.synthetic import HostFedDronesDET, SyntheticDronesDET
    from test_state_host import _chain

    def same(x, y):
        return all(torch.equal(p, q) if torch.is_tensor(p) else p == q for p, q in zip(x, y))

    def held(b):                                          # HostFedDronesDET hands out its device slots themselves
        return tuple(t.clone() if torch.is_tensor(t) else t for t in b)
    cfg = SimpleNamespace(seed=219, num_classes=10, Train=SimpleNamespace(scale_factor=4))
    for make in (lambda: SyntheticDronesDET(cfg, 2, 128, 160, boxes_per_image=9, pool=3),
                 lambda: HostFedDronesDET(cfg, 2, 128, 160, boxes_per_image=9, pool=3)):
        ref_ld, ld = make(), make()
        ref = [held(ref_ld.get_batch()) for _ in range(6)]
        assert ref_ld.position() == 6 and not torch.equal(ref[0][0], ref[1][0])
        ld.get_batch()
        ld.seek(4)
        assert ld.position() == 4
        assert same(ld.get_batch(), ref[4]) and same(ld.get_batch(), ref[5]) and ld.position() == 6
        ld.seek(1)
        assert same(ld.get_batch(), ref[1])
    root = C.write_dataset(str(tmp_path), splits=("train",), extra=2)
    chain = _chain((96, 128))
    ds = DronesDET(root, chain, "train")
    p = A.chain_params(chain)
    ref_ld = A.DeviceAugmentLoader(ds, p, 2, seed=5, num_workers=2)
    ld = A.DeviceAugmentLoader(ds, p, 2, seed=5, num_workers=2)
    try:
        ref = [held(ref_ld.get_batch()) for _ in range(5)]
        ld.get_batch()
        ld.seek(3)
        assert ld.position() == 3
        for want in ref[3:5]:
            got = ld.get_batch()
            assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)) and same(got[1:], want[1:])
        assert ld.position() == 5
    finally:
        ref_ld.close()
        ld.close()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
def test_resumed_step_equals_the_uninterrupted_step(tmp_path, bf16):
    """Operator A: steps 0-2, save, step 3.  Operator B (fresh, stale caches): load, step 3.  B's batch equals A's as
    bits; losses, parameters and BatchNorm statistics after the step agree within the bounds tests/test_streams_gpu.py
    holds two correct runs of ONE step to (losses 2e-5 relative, share of parameter elements whose Adam update differs
    <= 1e-3, running statistics 2e-5).  One step only: trajectories of this model diverge."""
    from stream_step_worker import frac_moved
    out = str(tmp_path)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", RR_CONV_SPLITK="0")
    for k in ("RR_WGRAD_STREAM", "RR_WGRAD_STRESS", "RR_DCN_BWD_STREAMS", "RR_DP_FORCE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, WORKER, "--out", out] + (["--bf16"] if bf16 else []), cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    meta = json.load(open(os.path.join(out, "meta.json")))
    assert meta["splitk"] == "0" and meta["start"] == 3 and meta["step_count"] == [4, 4]
    assert meta["same_batch"] and meta["int_buffers_equal"]
    la, lb = np.array(meta["losses_a"]), np.array(meta["losses_b"])

    def load(name):
        return torch.from_numpy(np.fromfile(os.path.join(out, name), dtype=np.float32))
    pa, pb = load("a_param.bin"), load("b_param.bin")
    ba, bb = load("a_buffers.bin"), load("b_buffers.bin")
    moved = frac_moved(pb, pa)
    bw = float(((bb - ba).abs() / ba.abs().clamp_min(1e-3)).max())
    print("resumed step (%s): losses %s vs %s; share of parameter elements whose Adam update differs %.2e; BN running "
          "statistics %.2e" % ("bf16" if bf16 else "fp32", la, lb, moved, bw))
    assert np.isfinite(la).all() and np.isfinite(lb).all() and torch.isfinite(pb).all()
    assert np.all(np.abs(la - lb) <= 2e-5 * np.maximum(np.abs(la), 1e-3)), (la, lb)
    assert moved <= 1e-3, moved
    assert bw <= 2e-5, bw


def test_training_process_with_full_state_and_resume(tmp_path, monkeypatch, capsys):
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    monkeypatch.chdir(tmp_path)
    cfg = _rr_cfg()
    cfg.Train.iter_num, cfg.Train.print_interval, cfg.Train.checkpoint_interval = 4, 1, 2
    cfg.Train.full_state, cfg.Train.keep_states = True, 2
    torch.manual_seed(219)
    RRNetOperator(cfg).training_process()
    log_dir = tmp_path / "log" / cfg.log_prefix
    names = sorted(os.listdir(str(log_dir)))
    assert names == ["ckp-1.pth", "ckp-3.pth", "state-1.pth", "state-3.pth"], names
    out = capsys.readouterr().out
    assert all("step %d " % s in out for s in range(4)) and "resumed" not in out
    cfg2 = _rr_cfg()
    cfg2.Train.iter_num, cfg2.Train.print_interval, cfg2.Train.checkpoint_interval = 6, 1, 2
    cfg2.Train.full_state, cfg2.Train.keep_states, cfg2.Train.resume = True, 2, "auto"
    torch.manual_seed(5)
    op = RRNetOperator(cfg2)
    op.training_process()
    out = capsys.readouterr().out
    assert "continuing at step 4" in out and "state-3.pth" in out
    reported = [int(l.split()[1]) for l in out.splitlines() if l.startswith("step ")]
    assert reported == [4, 5], out
    assert op.optimizer.step_count == 6 and op._state_writer is None
    names = sorted(os.listdir(str(log_dir)))
    assert names == ["ckp-1.pth", "ckp-3.pth", "ckp-5.pth", "state-3.pth", "state-5.pth"], names
