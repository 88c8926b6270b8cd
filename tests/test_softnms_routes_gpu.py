"""GPU parity of Soft-NMS on every launch route of rrnet_amd/csrc/softnms_plan.h: each row of tests/softnms_cases.py through
rr_soft_nms_segments and through rr_soft_nms_ragged, bit for bit against the oracle — N' and rows [0, N') of every segment as
uint32 words in columns 0..4; columns 5.. unchanged everywhere; nothing outside the segments touched; the error flag 0.
tests/test_softnms_routes_host.py proves which kernel bodies and branches these inputs reach."""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import softnms_cases as SC

pytestmark = pytest.mark.gpu


def _plan_label(nseg, bound):
    from rrnet_amd import _C
    buf = (ctypes.c_int * SC.PLAN_INTS)()
    _C.check(_C.fn("rr_soft_nms_plan")(nseg, bound, buf, SC.PLAN_INTS), "rr_soft_nms_plan")
    return SC.plan_label(list(buf))


def _expected(segs, sigma, Nt, thr, method):
    """The oracle on the segments back to back: (n_out, rows)."""
    from oracle import nms as onms
    off = np.concatenate([[0], np.cumsum([b.shape[0] for b in segs])]).astype(np.int32)
    rows = np.ascontiguousarray(np.concatenate(segs, 0))
    n_out = onms.soft_nms_segments(rows, off, sigma, Nt, thr, method)
    return n_out, [rows[off[k]:off[k] + n_out[k]] for k in range(len(segs))]


def _run_and_compare(segs, expected, ragged, bound, sigma, Nt, thr, method, seed, what):
    from rrnet_amd.ext.nms.nms_wrapper import soft_nms_segments
    flat, guard, seg_off, seg_len = SC.layout(segs, ragged, seed)
    total = int(seg_off[-1])
    dev = torch.from_numpy(flat.copy()).cuda()
    n_out, err = soft_nms_segments(dev[guard:guard + total], torch.from_numpy(seg_off).cuda(), bound, sigma, Nt, thr, method,
                                   seg_len=None if seg_len is None else torch.from_numpy(seg_len).cuda(), check=False)
    got = dev.cpu().numpy().view(np.uint32)
    n_out = n_out.cpu().numpy()
    assert int(err.item()) == 0, what
    want_n, want_rows = expected
    assert np.array_equal(n_out, want_n), (what, np.nonzero(n_out != want_n)[0][:8])
    before = flat.view(np.uint32)
    assert np.array_equal(got[:, 5:], before[:, 5:]), what          # columns 5.. never move
    inside = np.zeros(flat.shape[0], bool)
    for k, b in enumerate(segs):
        lo = guard + int(seg_off[k])
        inside[lo:lo + b.shape[0]] = True
        w = want_rows[k]
        same = got[lo:lo + w.shape[0], :5] == w[:, :5].view(np.uint32)
        assert same.all(), (what, "segment %d of %d boxes: first differing row %d of %d kept" %
                            (k, b.shape[0], int(np.nonzero(~same.all(1))[0][0]), w.shape[0]))
    assert np.array_equal(got[~inside], before[~inside]), what      # guard bands and the gaps of a ragged layout


_EXPECTED = {}


@pytest.mark.parametrize("cid,row,ragged", SC.cases(), ids=[c[0] for c in SC.cases()])
def test_route_equals_the_oracle(cid, row, ragged):
    name, label, _, bound, method, _ = row
    segs = [b for _, b in SC.row_segments(row, SC.row_stride(row))]
    assert _plan_label(len(segs), bound) == label
    if name not in _EXPECTED:                                       # computed once, shared by the row's two layouts
        _EXPECTED[name] = _expected(segs, SC.SIGMA, SC.NT, SC.THR, method)
    _run_and_compare(segs, _EXPECTED[name], ragged, bound, SC.SIGMA, SC.NT, SC.THR, method, zlib.crc32(name.encode()), cid)


def test_every_golden_through_the_lds_loop(golden_dir):
    """Each golden of softnms.npz (the reference's own outputs) in front of 513 small segments with a declared bound above 256:
    the throughput regime, so the LDS loop runs it — the register kernel runs the same goldens alone in test_softnms_gpu.py."""
    z = np.load(os.path.join(golden_dir, "softnms.npz"))
    ran = 0
    for k, name in enumerate(z["names"]):
        name = str(name)
        sigma, Nt, thr, method = z[name + "/params"]
        inp = z[name + "/in"]
        bound = max(257, inp.shape[0])
        segs = [inp] + SC.fillers(513, inp.shape[1], 1000 + k)
        assert _plan_label(len(segs), bound).startswith("lds")
        want_n, want_rows = _expected(segs, sigma, Nt, thr, int(method))
        assert want_n[0] == int(z[name + "/n_out"])
        assert np.array_equal(want_rows[0][:, :5].view(np.uint32), z[name + "/out"][:, :5].view(np.uint32)), name
        _run_and_compare(segs, (want_n, want_rows), k % 2 == 1, bound, sigma, Nt, thr, int(method), k, name)
        ran += 1
    assert ran >= 29


def test_benchmark_shape_in_small():
    """Config 5 of the benchmark in small: 520 ragged (frame, class) segments of around 150 boxes, a few of 1400..1500, declared
    bound 1500, gaussian — the two-launch split of the LDS loop, as the 1280 x 1500 batch of the benchmark."""
    segs = SC.bench_shape_segments()
    assert len(segs) == 520 and max(b.shape[0] for b in segs) == 1500
    assert _plan_label(520, 1500) == "lds<256>+<256>"
    _run_and_compare(segs, _expected(segs, 0.5, 0.7, 0.1, 2), True, 1500, 0.5, 0.7, 0.1, 2, 5, "bench shape")
