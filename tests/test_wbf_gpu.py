"""rr_wbf_segments, rrnet_amd.ensemble and tools/ensemble.py on the device against the numpy restatement of the contract
(tests/wbf_cases.py; tests/test_wbf_host.py proves what the table holds and that it sits on every route of the plan).
Everything is compared as bits."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wbf_cases as WC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


def run_case(case, dev):
    from rrnet_amd import ops
    name, segs, gap, thr, conf, wsum, exact, random = case
    rows, seg_off, seg_len = WC.layout(segs, gap)
    d_rows = torch.from_numpy(rows).to(dev)
    d_off = torch.from_numpy(seg_off).to(dev)
    d_len = torch.from_numpy(seg_len).to(dev) if seg_len is not None else None
    out = torch.full_like(d_rows, SENTINEL)
    res = ops.wbf_segments(d_rows, d_off, WC.bound_of(segs), thr, conf, wsum, seg_len=d_len, out=out)
    assert res[0] is out
    return rows, seg_off, [t.cpu().numpy() for t in res]


@pytest.mark.parametrize("case", WC.ROWS, ids=[r[0] for r in WC.ROWS])
def test_kernel_equals_the_restatement(case, dev):
    name, segs, gap, thr, conf, wsum, exact, random = case
    rows, seg_off, (out, members, n_out) = run_case(case, dev)
    again = run_case(case, dev)[2]
    for a, b in zip((out, members, n_out), again):                         # the same bits on every run
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    touched = np.zeros(rows.shape[0], bool)
    for s, seg in enumerate(segs):
        ref, ref_members, _ = WC.wbf_segment(seg, thr, conf, wsum)
        nc, o = ref.shape[0], int(seg_off[s])
        assert int(n_out[s]) == nc, (name, s, int(n_out[s]), nc)
        assert np.array_equal(members[o:o + nc], ref_members), (name, s)
        got = out[o:o + nc]
        bad = np.nonzero((got.view(np.uint32) != ref.view(np.uint32)).any(1))[0]
        assert bad.size == 0, (name, s, bad[:5], got[bad[:3]], ref[bad[:3]])
        touched[o:o + nc] = True
    assert (out[~touched] == np.float32(SENTINEL)).all() and (members[~touched] == 0).all()


def test_empty_batch_and_refusals(dev):
    from rrnet_amd import _C, ops
    rows = torch.zeros((0, 6), device=dev)
    out, members, n_out = ops.wbf_segments(rows, torch.zeros(1, dtype=torch.int32, device=dev), 0, 0.5, "avg", 1.0)
    assert out.shape == (0, 6) and n_out.numel() == 0
    rows = torch.ones((4, 6), device=dev)
    off = torch.tensor([0, 4], dtype=torch.int32, device=dev)
    with pytest.raises(_C.RRNetHipError, match=r"segment of 8193 rows \(limit 8192\)"):
        ops.wbf_segments(rows, off, 8193, 0.5, 0, 1.0)
    with pytest.raises(_C.RRNetHipError, match="weight_sum"):
        ops.wbf_segments(rows, off, 4, 0.5, 0, 0.0)
    with pytest.raises(_C.RRNetHipError, match="conf_type"):
        ops.wbf_segments(rows, off, 4, 0.5, 2, 1.0)
    with pytest.raises(ValueError, match="another"):
        ops.wbf_segments(rows, off, 4, 0.5, 0, 1.0, out=rows)


FUSE = dict(weights=[2.0, 1.0, 1.0], iou_thr=0.55, skip_score=0.05, conf_type="avg", max_det=50)


@pytest.fixture(scope="module")
def runs():
    sets = WC.gen_runs(6, seed=5)
    ref = [WC.fuse_frame([s[f] for s in sets], FUSE["weights"], FUSE["iou_thr"], FUSE["skip_score"], 0, 10 ** 9)
           for f in range(6)]
    return sets, ref


def test_fuse_rows_equals_the_restated_pipeline(runs, dev):
    from rrnet_amd import ensemble
    sets, ref = runs
    assert all(r.shape[0] > FUSE["max_det"] for r in ref)                  # more clusters than max_det keeps
    got, mem = ensemble.fuse_rows(sets, device=dev, want_members=True, **FUSE)
    assert len(got) == 6
    for f in range(6):
        assert got[f].dtype == np.float32 and got[f].shape == (FUSE["max_det"], 6)
        assert np.array_equal(got[f].view(np.uint32), ref[f][:FUSE["max_det"]].view(np.uint32)), f
        assert mem[f].shape == (FUSE["max_det"],) and mem[f].min() >= 1 and mem[f].max() > 1
    # the same whether the frames go in one call or one at a time
    for f in range(6):
        one = ensemble.fuse_rows([[s[f]] for s in sets], device=dev, **FUSE)
        assert len(one) == 1 and np.array_equal(one[0].view(np.uint32), got[f].view(np.uint32))
    # conf "max", and a frame without detections among the others
    sets2 = [[s[0], np.zeros((0, 8)), s[1]] for s in sets]
    got2 = ensemble.fuse_rows(sets2, device=dev, **dict(FUSE, conf_type="max"))
    assert got2[1].shape == (0, 6)
    for f, g in ((0, 0), (1, 2)):
        r = WC.fuse_frame([s[f] for s in sets], FUSE["weights"], 0.55, 0.05, 1, 50)
        assert np.array_equal(got2[g].view(np.uint32), r.view(np.uint32))


def _write(d, name, rows):
    from rrnet_amd import ensemble
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, name + ".txt"), "w") as f:
        f.write(ensemble.format_rows(rows))


def test_tool_in_a_fresh_process(runs, dev, tmp_path):
    from rrnet_amd import ensemble
    from rrnet_amd.utils.metrics.metrics import ext_nms_batch
    sets, _ = runs
    dirs = [str(tmp_path / ("run%d" % m)) for m in range(3)]
    names = ["img%02d" % f for f in range(3)]
    for m in range(3):
        for f in range(3):
            if (m, f) != (1, 2):                                           # run 1 lacks the last file
                _write(dirs[m], names[f], sets[m][f])
    env = dict(os.environ, PYTHONPATH=ROOT)
    tool = os.path.join(ROOT, "tools", "ensemble.py")
    out = str(tmp_path / "fused")
    r = subprocess.run([sys.executable, tool, "--runs"] + dirs + ["--out", out, "--weights", "2", "1", "1", "--skip-score", "0.05",
                        "--max-det", "50"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "1 missing" in r.stdout
    names2, read, missing = ensemble.read_result_dirs(dirs)               # what the files hold (six decimals), not what was generated
    assert names2 == names and missing == 1
    want = ensemble.fuse_rows(read, device=dev, **FUSE)
    for f, name in enumerate(names):
        assert open(os.path.join(out, name + ".txt")).read() == ensemble.format_rows(want[f]), name
        ref = WC.fuse_frame([s[f] for s in read], FUSE["weights"], 0.55, 0.05, 0, 50)
        assert np.array_equal(want[f].view(np.uint32), ref.view(np.uint32))
    out2 = str(tmp_path / "softnms")
    r = subprocess.run([sys.executable, tool, "--runs"] + dirs + ["--out", out2, "--method", "soft-nms", "--skip-score", "0.05",
                        "--max-det", "100000"], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    cat = [np.concatenate([np.asarray(s[f])[:, :6] for s in read], 0).astype(np.float32) for f in range(3)]
    kept = ext_nms_batch(cat, 0.05)
    for f, name in enumerate(names):
        k = kept[f][np.argsort(-kept[f][:, 4], kind="stable")]
        assert k.shape[0] > 0 and open(os.path.join(out2, name + ".txt")).read() == ensemble.format_rows(k), name
