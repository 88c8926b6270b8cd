"""Host proofs for tests/test_wbf_gpu.py (no GPU): the numpy restatement of rr_wbf_segments' contract (tests/wbf_cases.py)
gives the planted outcomes; on every random case float64 can make every decision; the table sits on every route of
csrc/wbf_plan.h (asked through rr_wbf_plan); the refusals say what they refuse; tools/ensemble.py checks its arguments and
fuse_result_dirs takes the union of the file names."""
import ctypes
import os
import sys

import numpy as np
import pytest

import wbf_cases as WC
from wbf_cases import f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan(nseg, bound):
    from rrnet_amd import _C
    buf = (ctypes.c_int * WC.PLAN_INTS)(*([-7] * WC.PLAN_INTS))
    rc = _C.fn("rr_wbf_plan")(nseg, bound, buf, WC.PLAN_INTS)
    if rc != 0:
        return None, _C.lib().rr_last_error().decode()
    return list(buf), None


@pytest.fixture(scope="module")
def results():
    """{case name: [(rows, out, members, trace)] per segment} in float32, computed once."""
    out = {}
    for name, segs, gap, thr, conf, wsum, exact, random in WC.ROWS:
        out[name] = [(s,) + WC.wbf_segment(s, thr, conf, wsum) for s in segs]
    return out


def test_planted_case_1_iou_exactly_at_the_threshold_does_not_join(results):
    (_, out, mem, tr), = results["planted1"]
    assert tr[1][2] == f32(0.5) and not tr[1][1]
    assert mem.tolist() == [1, 1]
    assert out[:, 4].tolist() == [f32(0.45), f32(0.4)]
    assert np.array_equal(out[:, :4], WC.PLANTED1[:, :4])


def test_planted_case_2_a_tie_goes_to_the_lowest_cluster(results):
    (_, out, mem, tr), = results["planted2"]
    assert tr[2][2] == tr[2][3] == f32(0.33333334) and tr[2][0] == 0 and tr[2][1]
    assert mem.tolist() == [2, 1]
    assert out[0, 0] == f32(0.4375) and out[0, 2] == f32(2.4375) and out[0, 1] == 0 and out[0, 3] == 2
    assert out[0, 4] == f32(0.5333333) and out[1, 4] == f32(0.26666668)


def test_planted_case_3_the_row_is_compared_with_the_fused_box(results):
    (rows, out, mem, tr), = results["planted3"]
    assert WC.iou_against(rows[:1, :4], rows[2, :4])[0] == f32(0.25)          # against the first ROW it would not join
    assert tr[2][1] and tr[2][2] > f32(0.3)
    assert mem.tolist() == [3]
    assert out[0].tolist() == [2.75, 0.0, 12.75, 10.0, f32(0.8), 1.0]


def test_zero_area_rows_open_their_own_clusters(results):
    (_, out, mem, tr), = results["zero_area"]
    assert [t[1] for t in tr] == [False, False, False, True]
    assert tr[2][2] == 0 and mem.tolist() == [2, 1, 1]                         # two identical zero-area rows: IoU 0, two clusters
    assert np.array_equal(out[1:3, :4], WC.ZERO_AREA[1:3, :4])


def test_conf_types_and_member_counts_on_both_sides_of_the_weight_sum(results):
    (rows, out_max, mem, _), = results["conf_max"]
    (_, out_avg, mem2, _), = results["conf_avg_below_and_above"]
    assert mem.tolist() == mem2.tolist() == [4, 2, 1]                          # weight_sum 3: above, below, below
    assert np.array_equal(out_max[:, :4], out_avg[:, :4])
    s = [float(x) for x in rows[:, 4]]
    assert out_max[:, 4].tolist() == [f32(s[0] * 3.0 / 3.0), f32(s[4] * 2.0 / 3.0), f32(s[6] * 1.0 / 3.0)]
    avg0 = (((s[0] + s[1]) + s[2]) + s[3]) / 4
    assert out_avg[:, 4].tolist() == [f32(avg0 * 3.0 / 3.0), f32((s[4] + s[5]) / 2 * 2.0 / 3.0), f32(s[6] * 1.0 / 3.0)]


@pytest.mark.parametrize("name", ["thr_one", "thr_above_one"])
def test_threshold_of_one_or_more_returns_the_input_bits(results, name):
    (rows, out, mem, tr), = results[name]
    assert not any(t[1] for t in tr) and (mem == 1).all()
    assert np.array_equal(out.view(np.uint32), rows.view(np.uint32))


def test_random_cases_hold_what_the_table_needs(results):
    sizes = set()
    largest = 0
    for name, segs, gap, thr, conf, wsum, exact, random in WC.ROWS:
        if not random:
            continue
        joins = opens = 0
        for rows, out, mem, tr in results[name]:
            sizes.add(rows.shape[0])
            assert (np.diff(rows[:, 4]) <= 0).all() and (rows[:, 4] > 0).all() and np.isfinite(rows).all()
            assert np.array_equal(rows[:, :4] * 4, np.round(rows[:, :4] * 4))     # quarter pixels
            joins += sum(t[1] for t in tr)
            opens += sum(not t[1] for t in tr)
            largest = max([largest] + mem.tolist())
            assert int(mem.sum()) == rows.shape[0] and out.shape[0] == len(mem) == sum(not t[1] for t in tr)
        assert joins > 0 and opens > 0, name
    assert {0, 1, 2, 63, 64, 65, 257, 1025, 4096} <= sizes
    assert largest > 100
    assert any(gap for _, _, gap, *_ in WC.ROWS) and any(0 in [s.shape[0] for s in segs[1:-1]] for _, segs, *_ in WC.ROWS)


def test_float64_can_make_every_decision(results):
    """The IoU in float64 takes every row to the same cluster, and no decision hangs on the last bits of a float32 IoU."""
    for name, segs, gap, thr, conf, wsum, exact, random in WC.ROWS:
        if exact:
            continue
        for rows, out, mem, tr in results[name]:
            out64, mem64, tr64 = WC.wbf_segment(rows, thr, conf, wsum, dtype=np.float64)
            assert [(t[0], t[1]) for t in tr] == [(t[0], t[1]) for t in tr64], name
            assert np.array_equal(out, out64) and np.array_equal(mem, mem64)
            for (k, joined, best, second) in tr64:
                if best is None:
                    continue
                assert abs(best - float(f32(thr))) > 1e-6, (name, best)
                if joined and second is not None:
                    assert best - second > 1e-6, (name, best, second)


def test_the_table_sits_on_every_route_of_the_plan():
    reached = set()
    for name, segs, gap, thr, conf, wsum, exact, random in WC.ROWS:
        v, err = plan(len(segs), WC.bound_of(segs))
        assert err is None, err
        assert v[WC.P_LAUNCHES] in (1, 2, 3) and v[-1] == 0
        for s in segs:
            reached.add(WC.body_of(v, s.shape[0]))
    assert reached == WC.BODIES, (reached ^ WC.BODIES)


def test_plan_boundaries_and_lds():
    v, _ = plan(5, 64)
    one_wave, short, lds_max, max_seg, grid = v[WC.P_ONE_WAVE:WC.P_WS_GRID + 1]
    assert (one_wave, short) == (64, 256) and max_seg >= 4096 and lds_max < max_seg
    for bound, launches, needs_ws in ((1, 1, 0), (one_wave, 1, 0), (one_wave + 1, 1, 0), (short, 1, 0), (short + 1, 2, 0),
                                      (lds_max, 2, 0), (lds_max + 1, 3, 1), (4096, 3, 1), (max_seg, 3, 1)):
        v, err = plan(7, bound)
        assert err is None and (v[WC.P_LAUNCHES], v[WC.P_NEEDS_WS]) == (launches, needs_ws), bound
        ls = [v[WC.P_L0 + i * WC.P_LSTRIDE:WC.P_L0 + (i + 1) * WC.P_LSTRIDE] for i in range(launches)]
        # the launches partition the segment lengths, each holds its longest segment, and the LDS fits a CU's 160 KB
        assert ls[0][WC.L_LO] == -1 and ls[-1][WC.L_HI] == 0x7fffffff
        for a, b in zip(ls, ls[1:]):
            assert a[WC.L_HI] == b[WC.L_LO]
        for l in ls:
            assert l[WC.L_CAP] >= min(l[WC.L_HI], bound) and l[WC.L_CAP] % 4 == 0
            assert l[WC.L_LDS] == l[WC.L_CAP] * (16 if l[WC.L_WS] else 68) and l[WC.L_LDS] + 1024 <= 160 * 1024
            assert l[WC.L_T] in (64, 256, 512) and (l[WC.L_T] == 64) == (bound <= one_wave)
            assert (l[WC.L_GRID] > 0) == bool(l[WC.L_WS])
    from rrnet_amd import _C
    ws = _C.fn("rr_wbf_workspace_bytes")
    assert ws(7, lds_max) == 0 and ws(7, 4096) == 7 * 4096 * 52 and ws(100000, 4096) == grid * 4096 * 52
    v, err = plan(0, 4096)
    assert err is None and v[WC.P_LAUNCHES] == 0


def test_refusals_name_the_limit():
    v, _ = plan(1, 1)
    v, err = plan(3, v[WC.P_MAX_SEG] + 1)
    assert v is None and err == "rr_wbf_segments: segment of 8193 rows (limit 8192)"
    v, err = plan(-1, 5)
    assert v is None and err == "rr_wbf_segments: negative size"
    from rrnet_amd import _C
    nul = ctypes.c_void_p(0)
    f = _C.fn("rr_wbf_segments")
    assert f(nul, nul, nul, 0, 100, 0.5, 0, 1.0, nul, nul, nul, nul, 0, nul) == 0       # an empty batch launches nothing
    assert f(nul, nul, nul, 2, 9000, 0.5, 0, 1.0, nul, nul, nul, nul, 0, nul) != 0
    assert _C.lib().rr_last_error().decode() == "rr_wbf_segments: segment of 9000 rows (limit 8192)"
    assert f(nul, nul, nul, 2, 100, 0.5, 0, 1.0, nul, nul, nul, nul, 0, nul) != 0
    assert _C.lib().rr_last_error().decode() == "rr_wbf_segments: null pointer"


def _sets(n=2):
    a = np.array([[0, 0, 10, 10, 0.9, 1, -1, -1], [50, 50, 10, 10, 0.8, 2, -1, -1]], np.float64)
    return [[a.copy(), a.copy()] for _ in range(n)]


def test_fuse_rows_refuses_before_any_launch(monkeypatch):
    from rrnet_amd import ensemble, ops

    def no_launch(*a, **k):
        raise AssertionError("a launch was attempted")
    monkeypatch.setattr(ops, "group_by_class", no_launch)
    monkeypatch.setattr(ops, "wbf_segments", no_launch)
    s = _sets()
    s[1][1][0, 5] = 32
    with pytest.raises(ValueError, match=r"frame 1 of run 1 holds a class id outside \[0, 32\)"):
        ensemble.fuse_rows(s)
    s = _sets()
    s[0][1][1, 2] = np.inf
    with pytest.raises(ValueError, match="frame 1 of run 0 holds non-finite values"):
        ensemble.fuse_rows(s)
    s = _sets()
    s[0][0][0, 4] = np.nan
    with pytest.raises(ValueError, match="frame b of run 0 holds non-finite"):
        ensemble.fuse_rows(s, frame_names=["b", "c"])
    big = np.tile(np.array([[0, 0, 10, 10, 0.5, 3, -1, -1]], np.float64), (5000, 1))
    with pytest.raises(ValueError, match="frame 1 holds 10000 rows of one class, the kernel takes segments of up to 8192"):
        ensemble.fuse_rows([[np.zeros((0, 8)), big], [np.zeros((0, 8)), big]])
    for w in ([1.0], [1.0, 0.0], [1.0, -2.0], [1.0, float("nan")], [1.0, float("inf")]):
        with pytest.raises(ValueError, match="weights"):
            ensemble.fuse_rows(_sets(), weights=w)
    with pytest.raises(ValueError, match="skip_score"):
        ensemble.fuse_rows(_sets(), skip_score=-0.1)
    with pytest.raises(ValueError, match="conf_type"):
        ensemble.fuse_rows(_sets(), conf_type="box_and_model_avg")
    with pytest.raises(ValueError, match="run 1 has 1 frames"):
        ensemble.fuse_rows([_sets()[0], _sets()[0][:1]])


def test_tool_arguments(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import ensemble as tool
    finally:
        sys.path.pop(0)
    a, b, out = str(tmp_path / "a"), str(tmp_path / "b"), str(tmp_path / "out")
    os.makedirs(a)
    os.makedirs(b)
    args = tool.parse_args(["--runs", a, b, "--out", out])
    assert (args.iou, args.skip_score, args.conf, args.max_det, args.method, args.weights, args.targets) == \
        (0.55, 0.0, "avg", 500, "wbf", None, None)
    args = tool.parse_args(["--runs", a, b, "--out", out, "--weights", "2", "1", "--iou", "0.6", "--skip-score", "0.05",
                            "--conf", "max", "--max-det", "100", "--method", "soft-nms", "--targets", a])
    assert (args.weights, args.iou, args.skip_score, args.conf, args.max_det, args.method, args.targets) == \
        ([2.0, 1.0], 0.6, 0.05, "max", 100, "soft-nms", a)
    for bad in (["--runs", a, b, "--out", out, "--weights", "1"],
                ["--runs", a, b, "--out", out, "--weights", "1", "0"],
                ["--runs", a, b, "--out", out, "--skip-score", "-1"],
                ["--runs", a, b, "--out", out, "--conf", "box_and_model_avg"],
                ["--runs", a, b, "--out", out, "--method", "nms"],
                ["--runs", a, b, "--out", out, "--max-det", "0"],
                ["--runs", a, str(tmp_path / "nowhere"), "--out", out],
                ["--runs", a, b, "--out", a],
                ["--runs", a, b, "--out", out, "--targets", str(tmp_path / "nowhere")],
                ["--runs", a, b],
                ["--out", out]):
        with pytest.raises(SystemExit) as e:
            tool.parse_args(bad)
        assert e.value.code == 2, bad
    capsys.readouterr()


def test_file_names_are_the_union_over_the_runs(tmp_path):
    from rrnet_amd import ensemble
    dirs = [str(tmp_path / n) for n in "abc"]
    for d in dirs:
        os.makedirs(d)
    row = "1.000000,2.000000,3.000000,4.000000,0.5000,1,-1,-1\n"
    for d, names in zip(dirs, (("f1", "f2"), ("f2", "f3"), ("f1", "f2", "f3"))):
        for n in names:
            with open(os.path.join(d, n + ".txt"), "w") as f:
                f.write(row if (d, n) != (dirs[2], "f3") else "")                # an empty file: no detections, not missing
    open(os.path.join(dirs[0], "notes.md"), "w").close()
    names, sets, missing = ensemble.read_result_dirs(dirs)
    assert names == ["f1", "f2", "f3"] and missing == 2
    assert [[s[f].shape[0] for f in range(3)] for s in sets] == [[1, 1, 0], [0, 1, 1], [1, 1, 0]]
    assert sets[0][0][0].tolist() == [1, 2, 3, 4, 0.5, 1, -1, -1]
    assert ensemble.format_rows(np.array([[1, 2, 3, 4, 0.5, 1]], np.float32)) == row
