"""Host proofs for tests/test_softnms_routes_gpu.py (no GPU): the launch plan of Soft-NMS (rrnet_amd/csrc/softnms_plan.h, through
rr_soft_nms_plan) answers every row of tests/softnms_cases.py with the label written there and the boundary pairs correctly;
the instrumented numpy restatement of the reference loop equals the oracle bit for bit; and, read off that restatement with the
kernels' constants taken from the plan, the table's segments reach every renumbering branch of every register instantiation and
every compaction branch of every team width of the LDS loop."""
import ctypes
import os

import numpy as np
import pytest

import softnms_cases as SC
from softnms_cases import (P_CAP, P_KERNEL, P_LAUNCHES, P_LDS, P_LDS0, P_LDS_MAX, P_MASK_BOXES, P_MID_SEG, P_NB, P_NEEDS_WS,
                           P_ONE_WAVE, P_RAISE, P_REG_LIST, P_REG_SHORT, P_T, P_T0, P_USES_WS)


def plan(nseg, bound):
    """rr_soft_nms_plan -> list of ints, or None where the library refuses (a refusal must come with a reason)."""
    from rrnet_amd import _C
    buf = (ctypes.c_int * SC.PLAN_INTS)(*([-7] * SC.PLAN_INTS))
    rc = _C.fn("rr_soft_nms_plan")(nseg, bound, buf, SC.PLAN_INTS)
    if rc != 0:
        assert _C.lib().rr_last_error().decode().startswith("rr_soft_nms"), _C.lib().rr_last_error()
        return None
    assert buf[17] == 0
    return list(buf)


def body_of(v, n):
    """The kernel body that runs a segment of n boxes in a launch planned as v."""
    if v[P_KERNEL] == 0:
        if v[P_T] > 256 and n <= v[P_REG_SHORT]:
            return "reg<256,1>/short"
        return "reg<%d,%d>" % (v[P_T], v[P_NB])
    ws = "/ws" if v[P_USES_WS] else ""
    if n <= v[P_ONE_WAVE]:
        return "lds64" + ws
    if v[P_LAUNCHES] == 2 and n <= v[P_MID_SEG]:
        return "lds%d" % v[P_T0]
    return "lds%d" % v[P_T] + ws


@pytest.fixture(scope="module")
def traces():
    """{row name: [(spec, rows in, rows out, N', steps)]} of every segment of the table, with the row's method."""
    out = {}
    for row in SC.ROWS:
        out[row[0]] = [(sp, b) + SC.soft_nms_traced(b, SC.SIGMA, SC.NT, SC.THR, row[4]) for sp, b in SC.row_segments(row)]
    return out


def test_restatement_equals_the_oracle_on_every_golden(golden_dir):
    from oracle import nms as onms
    z = np.load(os.path.join(golden_dir, "softnms.npz"))
    assert len(z["names"]) >= 29
    for name in z["names"]:
        name = str(name)
        sigma, Nt, thr, method = z[name + "/params"]
        inp = z[name + "/in"]
        rows, n_out, _ = SC.soft_nms_traced(inp, sigma, Nt, thr, int(method))
        w = inp.copy()
        keep = onms.cpu_soft_nms(w, sigma, Nt, thr, int(method))
        assert n_out == len(keep) == int(z[name + "/n_out"]), name
        assert np.array_equal(rows[:n_out].view(np.uint32), w[:n_out].view(np.uint32)), name
        assert np.array_equal(rows[:n_out, :5].view(np.uint32), z[name + "/out"][:, :5].view(np.uint32)), name


def test_restatement_equals_the_oracle_on_every_segment_of_the_table(traces):
    from oracle import nms as onms
    for row in SC.ROWS:
        for sp, b, rows, n_out, steps in traces[row[0]]:
            w = b.copy()
            keep = onms.cpu_soft_nms(w, SC.SIGMA, SC.NT, SC.THR, row[4])
            assert n_out == len(keep), (row[0], sp)
            assert np.array_equal(rows[:n_out].view(np.uint32), w[:n_out].view(np.uint32)), (row[0], sp)
            assert len(steps) == n_out                       # one outer step per kept box


def test_cluster_recipe_kills_exactly_the_mates(traces):
    """Selecting a cluster's top kills its m - 1 mates and nothing else (crowd-free segments: their death steps are the clusters')."""
    seen = 0
    for row in SC.ROWS:
        for sp, b, rows, n_out, steps in traces[row[0]]:
            if sp["crowd"] == 0 and sp["clusters"] and not sp["lane_tie"]:
                assert sorted(st["D"] for st in steps if st["D"]) == sorted(m - 1 for m in sp["clusters"] if m > 1), (row[0], sp)
                seen += 1
    assert seen >= 10


def test_plan_answers_every_row_with_its_label_and_the_table_reaches_every_label():
    reached = set()
    for row in SC.ROWS:
        name, label, _, bound, method, _ = row
        segs = SC.row_segments(row)
        assert len(segs) == SC.row_nseg(row)
        assert max(b.shape[0] for _, b in segs) <= bound, name
        v = plan(len(segs), bound)
        assert v is not None and SC.plan_label(v) == label, (name, v)
        assert label in SC.LABELS
        reached.add(label)
        assert method in (0, 1, 2)
    # (one launch of the LDS loop with 1024 threads on LDS would need a bound above 2560 that is at most MID_SEG = 512: no such label)
    assert reached == set(SC.LABELS)
    for nseg in (1, 2, 512, 513, 5000):
        for bound in list(range(0, 700)) + list(range(1400, 9400, 7)) + [9216, 9217, 20000, 65535]:
            v = plan(nseg, bound)
            assert SC.plan_label(v) in reached, (nseg, bound, v)
    kernels, strides = {}, {}
    for row in SC.ROWS:
        kernels.setdefault(row[1][:3], set()).add(row[4])
        strides.setdefault(row[1][:3], set()).add(SC.row_stride(row))
    assert kernels == {"reg": {0, 1, 2}, "lds": {0, 1, 2}}   # every method on both kernels
    assert strides == {"reg": {5, 6, 7}, "lds": {5, 6, 7}}   # and every stride


def test_plan_boundaries_and_fields():
    label = lambda nseg, bound: SC.plan_label(plan(nseg, bound))
    pairs = {256: ("reg<256,1>", "reg<512,3>"), 1536: ("reg<512,3>", "reg<1024,3>"), 3072: ("reg<1024,3>", "reg<512,12>"),
             6144: ("reg<512,12>", "reg<512,18>"), 9216: ("reg<512,18>", "lds<1024>/ws")}
    for b, (at, above) in pairs.items():
        assert (label(1, b), label(1, b + 1)) == (at, above), b
    for b, (few, many) in {257: ("reg<512,3>", "lds<256>"), 513: ("reg<512,3>", "lds<256>+<256>"),
                           2561: ("reg<1024,3>", "lds<256>+<1024>"), 6001: ("reg<512,12>", "reg<512,12>")}.items():
        assert (label(512, b), label(513, b)) == (few, many), b
    assert label(513, 256) == "reg<256,1>" and label(513, 512) == "lds<256>" and label(513, 2560) == "lds<256>+<256>"
    assert label(513, 6000) == "lds<256>+<1024>" and label(513, 9216) == "reg<512,18>" and label(513, 9217) == "lds<1024>/ws"
    # the constants the kernels share with the plan
    v = plan(1, 100)
    assert (v[P_REG_LIST], v[P_REG_SHORT], v[P_ONE_WAVE], v[P_MID_SEG], v[P_LDS_MAX], v[P_MASK_BOXES]) == (64, 256, 192, 512, 6000, 9216)
    assert v[P_LAUNCHES] == 1 and v[P_LDS] == v[P_CAP] == v[P_T0] == v[P_LDS0] == v[P_NEEDS_WS] == v[P_USES_WS] == 0
    assert plan(0, 100)[P_LAUNCHES] == 0 and plan(0, 7000)[P_NEEDS_WS] == 0          # an empty batch launches nothing
    # LDS bytes: 25 per row of the capacity (the bound rounded up to 4) + 16; above 48 KB the limit is raised first
    for bound, lds, raised in ((257, 260 * 25 + 16, 0), (512, 512 * 25 + 16, 0), (1500, 1500 * 25 + 16, 0), (1965, 1968 * 25 + 16, 1),
                               (2560, 64016, 1), (6000, 150016, 1)):
        v = plan(513, bound)
        assert (v[P_LDS], v[P_CAP], v[P_RAISE]) == (lds, (bound + 3) & ~3, raised), bound
        assert (v[P_LAUNCHES], v[P_T0], v[P_LDS0]) == ((2, 256, 512 * 25 + 16) if bound > 512 else (1, 0, 0)), bound
        assert v[P_LDS] + 512 <= 160 * 1024
    assert (1964 * 25 + 16 <= 48 * 1024 < 1968 * 25 + 16) and plan(513, 1964)[P_RAISE] == 0
    v = plan(513, 9217)
    assert (v[P_LDS], v[P_CAP], v[P_NEEDS_WS], v[P_USES_WS], v[P_T], v[P_LAUNCHES]) == (0, 9220, 1, 1, 1024, 1)
    v = plan(1, 6001)
    assert (v[P_NEEDS_WS], v[P_USES_WS]) == (1, 0)               # the register kernel needs none, the entry point still asks
    assert plan(1, 6000)[P_NEEDS_WS] == 0


def test_refusals_of_the_plan_and_of_the_entry_points():
    from rrnet_amd import _C
    assert plan(1, 65536) is None and "limit 65535" in _C.lib().rr_last_error().decode()
    assert plan(1, 65535) is not None
    assert plan(-1, 10) is None and plan(1, -1) is None
    buf = (ctypes.c_int * 4)()
    assert _C.fn("rr_soft_nms_plan")(1, 10, buf, 4) != 0         # too short an answer buffer
    null = ctypes.c_void_p(0)
    # the entry points refuse before anything touches a device: null pointers are never read

    def entry(nseg, bound, stride, ws, ragged=False, seg_len=null):
        # (sigma == 0 with the gaussian method is refused behind the checks under test: no call here can reach a launch)
        tail = (nseg, bound, stride, 0.0, 0.3, 0.1, 2, null, null, ws, null)
        if ragged:
            return _C.fn("rr_soft_nms_ragged")(null, null, seg_len, *tail)
        return _C.fn("rr_soft_nms_segments")(null, null, *tail)
    some = ctypes.c_void_p(64)
    for ragged in (False, True):
        assert entry(1, 10, 4, null, ragged, some) != 0 and "stride 4 < 5" in _C.lib().rr_last_error().decode()
        assert entry(1, 65536, 5, some, ragged, some) != 0 and "limit 65535" in _C.lib().rr_last_error().decode()
        assert entry(1, 6001, 5, null, ragged, some) != 0 and "workspace required" in _C.lib().rr_last_error().decode()
        assert entry(-1, 10, 5, null, ragged, some) != 0
        assert entry(0, 6001, 5, null, ragged, some) == 0          # an empty batch is taken as it is
    assert entry(1, 10, 5, null, True, null) != 0 and "seg_len is null" in _C.lib().rr_last_error().decode()
    assert _C.fn("rr_soft_nms_workspace_bytes")(1000, 6000) == 0 and _C.fn("rr_soft_nms_workspace_bytes")(1000, 6001) == 28064


def _bodies(traces):
    """{kernel body: [(spec, steps)]} over the table."""
    out = {}
    for row in SC.ROWS:
        v = plan(len(traces[row[0]]), row[3])
        for sp, b, rows, n_out, steps in traces[row[0]]:
            if b.shape[0]:
                out.setdefault(body_of(v, b.shape[0]), []).append((sp, steps))
    return out


REG_BODIES = ("reg<256,1>", "reg<256,1>/short", "reg<512,3>", "reg<1024,3>", "reg<512,12>", "reg<512,18>")


@pytest.mark.parametrize("body", REG_BODIES)
def test_table_reaches_every_renumbering_branch_of_the_register_kernel(traces, body):
    L = plan(1, 100)[P_REG_LIST]
    segs = _bodies(traces)[body]
    got = set()
    for sp, steps in segs:
        deaths = [st for st in steps if st["D"]]
        for st in deaths:
            path = "list" if st["D"] <= L else "mask"
            if st["D"] == L:
                got.add("D == list")
            if st["D"] == L + 1:
                got.add("D == list + 1")
            if st["left"] == 0:
                got.add("kills all, " + path)
            elif st["tied"]:
                got.add("tied, " + path)
            elif st["moved"]:
                got.add("moved untied, " + path)
        for a, b in zip(deaths, deaths[1:]):
            got.add(("L" if a["D"] <= L else "M") + ("L" if b["D"] <= L else "M"))
    want = {"D == list", "D == list + 1", "LM", "ML", "MM", "LL", "tied, list", "tied, mask", "moved untied, list",
            "moved untied, mask", "kills all, list", "kills all, mask"}
    assert want <= got, (body, sorted(want - got))


def test_in_lane_ties_are_what_they_claim(traces):
    """The lane_tie segments: step 0 pre-selects A at position 2, untied by any OTHER lane's candidate — both boxes of the
    maximal surviving score belong to lane 2 — and the compaction moves B from position 2 + T to position 1, in front of A."""
    seen = set()
    for row in SC.ROWS:
        v = plan(len(traces[row[0]]), row[3])
        for sp, b, rows, n_out, steps in traces[row[0]]:
            if sp["lane_tie"]:
                T, deaths = sp["lane_tie"]
                assert v[P_KERNEL] == 0 and v[P_T] == T and v[P_NB] > 1 and b.shape[0] > v[P_REG_SHORT]
                st = steps[0]
                assert st["D"] == deaths and st["tied"] and not st["moved"] and st["nmove"] == 1
                sv = b[:, 4].copy()
                assert np.count_nonzero(sv == sv[2]) == 2 and sv[2 + T] == sv[2] and (2 + T) % T == 2
                assert np.array_equal(rows[1], b[2 + T]) and np.array_equal(rows[2], b[2])
                seen.add((SC.plan_label(v), "list" if deaths <= v[P_REG_LIST] else "mask"))
    assert seen == {(k, p) for k in ("reg<512,3>", "reg<1024,3>", "reg<512,12>", "reg<512,18>") for p in ("list", "mask")}


def test_last_mask_position_dies_in_the_9216_box_segment(traces):
    v = plan(1, 9216)
    hit = 0
    for name in ("reg512x18", "reg512x18_many"):
        for sp, b, rows, n_out, steps in traces[name]:
            if b.shape[0] == v[P_MASK_BOXES]:
                hit += any(st["D"] > v[P_REG_LIST] and st["top"] == v[P_MASK_BOXES] - 1 for st in steps)
    assert hit == 2


@pytest.mark.parametrize("body,width", [("lds64", 64), ("lds256", 256), ("lds1024", 1024), ("lds1024/ws", 1024), ("lds64/ws", 64)])
def test_table_reaches_every_compaction_branch_of_the_lds_loop(traces, body, width):
    segs = _bodies(traces)[body]
    got = set()
    for sp, steps in segs:
        for st in steps:
            if st["D"]:
                got.add("moves" if st["nmove"] else "nothing moves")
                if st["D"] > width:
                    got.add("more deaths than threads")
                if st["nmove"] > width:
                    got.add("more moves than threads")
    want = {"moves", "nothing moves", "more deaths than threads"}
    assert want <= got, (body, sorted(want - got))
