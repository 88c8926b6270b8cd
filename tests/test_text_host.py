"""The text codec without a device: the pure-Python restatement (tests/text_cases.py) against Python's own %, int() and
float(); the library's host loops (rr_text_format_host, rr_text_lines_host, rr_text_parse_host: the same csrc/textcodec.h
the kernels run) against Python's formatting and metrics._read; and the text= keywords of the evaluator and the fusion
with a stub in textio's place."""
import os
import sys

import numpy as np
import pytest

import text_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    from rrnet_amd.csrc import build
    build.build(verbose=False)
    from rrnet_amd import ops
    return ops


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


# ---- the restatement against Python ------------------------------------------------------------------------------------

def test_restatement_formats_as_python_does():
    vals = np.concatenate([tc.special_floats(), tc.strided_floats(stride=1048573)])
    for v in vals.tolist():
        v32 = np.float32(v)
        big = np.isfinite(v32) and abs(v) >= 2.0 ** 63
        for dec, fmt in ((6, "%f"), (4, "%.4f")):
            got = tc.fmt_fixed(v32, dec)
            assert got == (tc.FLAG if big else fmt % v), (v, dec)
        if np.isfinite(v32) and not big:
            assert tc.to_int(v32) == int(v), v
        else:
            assert tc.to_int(v32) is tc.FLAG, v


def test_restatement_parses_as_float_does():
    rng = np.random.default_rng(3)
    vals = np.concatenate([rng.uniform(-3000, 3000, 3000), rng.uniform(0, 1, 1000), 10.0 ** rng.uniform(-6, 9, 1000)])
    for v in vals.astype(np.float32).tolist():
        for fmt in ("%f", "%.4f"):
            s = fmt % v
            got = tc.parse_field(s.encode())
            if float(s) == 0.0 and s.startswith("-"):
                assert got is tc.FLAG
            else:
                assert got == float(s) and np.signbit(got) == np.signbit(float(s)), s
    for s, want in ((b"+1.5", 1.5), (b".5", 0.5), (b"5.", 5.0), (b"0.1234567890123456", 0.1234567890123456),
                    (b"9007199254740991", 9007199254740991.0), (b"00012.500", 12.5)):
        assert tc.parse_field(s) == want, s
    for s in (b"", b"-", b".", b"1e3", b"nan", b"inf", b"-0", b"-0.000", b" 1", b"1 ", b"0.00000000001234567890123", b"0.0000000001234567890123", b"0.12345678901234567",
              b"9007199254740992", b"1.2.3", b"--1", b"0x10"):
        assert tc.parse_field(s) is tc.FLAG, s


def test_restatement_rows_equal_the_writers_expressions():
    rows = np.concatenate([tc.rows_from_values(tc.special_floats())[::5], tc.detection_rows(500, seed=1)])
    for layout in (0, 1, 2):
        for clamp in (0, 1):
            for r in rows:
                got, want = tc.fmt_row(r, layout, clamp), tc.python_row(r, layout, clamp)
                assert (got is tc.FLAG) == tc.must_flag(r, layout, clamp), (r, layout, clamp)
                assert got == want or (got is tc.FLAG and want is not tc.FLAG), (r, layout, clamp)   # flagged: the host decides


# ---- the library's host loops ------------------------------------------------------------------------------------------

def _expect(rows, layout, clamp):
    """The writers' expression over all rows at once -> (bytes of the rows Python can format, flags)."""
    r = np.asarray(rows, np.float32)
    if clamp:
        r = np.where(r < 0, np.float32(0.), r)
    if layout == 1:
        r = np.concatenate((np.rint(r[:, :4]), r[:, 4:]), axis=1)
    out, flags = [], np.zeros(len(r), np.int32)
    for i, x in enumerate(r.tolist()):
        try:
            if layout == 0:
                out.append("%f,%f,%f,%f,%.4f,%d,-1,-1\n" % (x[0], x[1], x[2], x[3], x[4], int(x[5])))
            elif layout == 1:
                out.append("%d,%d,%d,%d,%.4f,%d,-1,-1\n" % (int(x[0]), int(x[1]), int(x[2]) - int(x[0]), int(x[3]) - int(x[1]),
                                                            x[4], int(x[5])))
            else:
                out.append("%d,%d,%d,%d,%.4f,%d,-1,-1\n" % (int(x[0]), int(x[1]), int(x[2]), int(x[3]), x[4], int(x[5])))
        except (ValueError, OverflowError):
            flags[i] = 1
    return "".join(out).encode(), flags


def _big(v):
    return np.isfinite(v) & (np.abs(v.astype(np.float64)) >= 2.0 ** 63)


def test_format_host_strided_sweep_of_all_bit_patterns(ops):
    """%f and %.4f of every 8191st float32 bit pattern (524 k values, every exponent, both signs), then %d of the same."""
    v = tc.strided_floats(stride=8191)
    rows = np.zeros((v.size, 6), np.float32)
    rows[:, 0], rows[:, 4], rows[:, 5] = v, v, 1.0
    out, off, flag = ops.text_format_host(rows, 0, 0)
    assert np.array_equal(flag.astype(bool), _big(v))
    keep = ~_big(v)
    want = "".join("%f,0.000000,0.000000,0.000000,%.4f,1,-1,-1\n" % (x, x) for x in v[keep].tolist()).encode()
    assert out.tobytes() == want
    fin = np.isfinite(v) & ~_big(v)
    rows[:, 0], rows[:, 4], rows[:, 5] = 0.0, 0.5, v
    out, off, flag = ops.text_format_host(rows, 2, 0)
    assert np.array_equal(flag.astype(bool), ~fin)
    want = "".join("0,0,0,0,0.5000,%d,-1,-1\n" % int(x) for x in v[fin].tolist()).encode()
    assert out.tobytes() == want


@pytest.mark.parametrize("layout", [0, 1, 2])
@pytest.mark.parametrize("clamp", [0, 1])
def test_format_host_equals_the_writers(ops, layout, clamp):
    rows = np.concatenate([tc.rows_from_values(tc.special_floats(), seed=layout), tc.detection_rows(2000, seed=2)])
    out, off, flag = ops.text_format_host(rows, layout, clamp)
    want_flag = np.asarray([tc.must_flag(x, layout, clamp) for x in rows], np.int32)
    py, py_flag = _expect(rows, layout, clamp)
    assert not (py_flag & ~want_flag).any()                       # whatever Python refuses, the codec flags
    want, _ = _expect(rows[want_flag == 0], layout, clamp)
    assert np.array_equal(flag, want_flag)
    assert out.tobytes() == want
    assert int(np.diff(off).max()) <= ops.TEXT_MAX_ROW
    assert want_flag.any() and not want_flag.all()


def test_format_host_flagged_rows_write_nothing(ops):
    ok = np.asarray([10.5, 20.25, 30.0, 40.0, 0.5, 3.0], np.float32)
    for row, layouts in tc.flagged_rows():
        for layout in (0, 1, 2):
            rows = np.stack([ok, row, ok])
            out, off, flag = ops.text_format_host(rows, layout, 0, pad=64, fill=0xAB)
            want = layout in layouts
            assert flag.tolist() == [0, int(want), 0], (row, layout)
            mid = b"" if want else tc.python_row(row, layout, 0)
            one = tc.python_row(ok, layout, 0)
            assert out[:off[-1]].tobytes() == one + mid + one
            assert off[2] - off[1] == len(mid)
            assert (out[off[-1]:] == 0xAB).all() and out.size == off[-1] + 64


def test_format_host_longest_row_is_the_bound(ops):
    big = np.float32(-(2.0 ** 63 - 2.0 ** 39))                    # the largest float32 below 2^63, negative
    out, off, flag = ops.text_format_host(np.full((1, 6), big, np.float32), 0, 0)
    assert flag[0] == 0 and off[1] == ops.TEXT_MAX_ROW == 165
    assert out.tobytes() == tc.python_row(np.full(6, big, np.float32), 0, 0)


def _read(path):
    from rrnet_amd.utils.metrics.metrics import _read
    return _read(path)


def test_parse_host_equals_read_on_clean_files(ops, tmp_path):
    files = tc.clean_files()
    paths = tc.write_files(str(tmp_path), files)
    names = sorted(files)
    text, file_off = tc.pack_files([b"xx"] + [files[n] for n in names])     # an odd prefix: unaligned file starts
    text[:2] = 10
    rows, flags, line_pos, flo = ops.text_parse_host(text, file_off, 8)
    assert flo[0] == 0 and flo[1] == 0 and flo[-1] == rows.shape[0]
    for i, n in enumerate(names):
        got, fl = rows[flo[i + 1]:flo[i + 2]], flags[flo[i + 1]:flo[i + 2]]
        want_rows, want_flags = tc.parse_text(files[n])
        assert np.array_equal(fl, want_flags), n
        assert tc.file_on_device(fl), n
        assert np.array_equal(_bits(got), _bits(want_rows)), n
        ref = _read(paths[n])
        assert ref.shape[0] == got.shape[0], n
        assert np.array_equal(_bits(got), _bits(ref[:, :8].astype(np.float64))), n
    assert (text[line_pos - 1] == 10).all()


def test_parse_host_empty_and_blank_files(ops):
    text, file_off = tc.pack_files([b"", b"\n\r\n\n", b"", b"1,2,3,4,0.5,1,-1,-1"])
    rows, flags, line_pos, flo = ops.text_parse_host(text, file_off, 8)
    assert flo.tolist() == [0, 0, 0, 0, 1] and flags.tolist() == [0]
    assert rows.tolist() == [[1, 2, 3, 4, 0.5, 1, -1, -1]]
    rows, flags, line_pos, flo = ops.text_parse_host(np.zeros(0, np.uint8), np.zeros(1, np.int64), 8)
    assert rows.shape == (0, 8) and flo.tolist() == [0]


def test_parse_host_flags_what_it_must(ops):
    files = tc.flagged_files()
    for name, data in files.items():
        text, file_off = tc.pack_files([data])
        rows, flags, _, flo = ops.text_parse_host(text, file_off, 8)
        want_rows, want_flags = tc.parse_text(data)
        assert np.array_equal(flags, want_flags), name
        assert (flags & 1).sum() >= 1 and flags[0] == 0 and flags[-1] == 0, name
        assert not tc.file_on_device(flags), name
        keep = flags != 1
        assert np.array_equal(_bits(rows[keep]), _bits(want_rows[keep])), name
    text, file_off = tc.pack_files([tc.mixed_surplus_file()])
    flags = ops.text_parse_host(text, file_off, 8)[1]
    assert flags.tolist() == [0, 2] and not tc.file_on_device(flags)


def test_parse_host_other_column_counts(ops):
    text, file_off = tc.pack_files([b"1.5,2.5,3.5,4.5,0.25,7\n"])
    rows, flags, _, _ = ops.text_parse_host(text, file_off, 6)
    assert flags.tolist() == [0] and rows.tolist() == [[1.5, 2.5, 3.5, 4.5, 0.25, 7.0]]
    assert ops.text_parse_host(text, file_off, 5)[1].tolist() == [1]          # a surplus field that is not empty
    assert ops.text_parse_host(text, file_off, 8)[1].tolist() == [1]          # a short line


def test_round_trip_on_the_host(ops):
    rows = tc.detection_rows(2000, seed=9)
    rows[:, :4] = np.round(rows[:, :4] * 64) / 64          # six decimals hold these exactly
    rows[:, 4] = np.round(rows[:, 4] * 10000) / 10000
    rows = np.abs(rows).astype(np.float32)
    out, off, flag = ops.text_format_host(rows, 0, 0)
    got, flags, _, _ = ops.text_parse_host(out, np.asarray([0, out.size], np.int64), 8)
    assert not flag.any() and not flags.any()
    assert np.array_equal(got.astype(np.float32)[:, :4], rows[:, :4]) and np.array_equal(got[:, 5], rows[:, 5])
    assert np.array_equal(got[:, 4].astype(np.float32), rows[:, 4])


def test_generated_folders_stay_on_the_device(ops, tmp_path):
    """No line of tools/bench_eval.py's generated folders is flagged: on the restatement first, then on the host loops."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_eval
    pd_dir, gt_dir = bench_eval.write_files(str(tmp_path), 6, 40, 12)
    for d in (pd_dir, gt_dir):
        for name in sorted(os.listdir(d)):
            data = open(os.path.join(d, name), "rb").read()
            want_rows, want_flags = tc.parse_text(data)
            assert tc.file_on_device(want_flags), name
            text, file_off = tc.pack_files([data])
            rows, flags, _, _ = ops.text_parse_host(text, file_off, 8)
            assert np.array_equal(flags, want_flags) and np.array_equal(_bits(rows), _bits(want_rows))
            assert np.array_equal(_bits(rows), _bits(_read(os.path.join(d, name)).astype(np.float64)))


# ---- the text= keywords, with a stub in textio's place -------------------------------------------------------------------

class _Stub:
    """Stands where textio.read_files stands: records the call and answers through the host function it is given."""

    def __init__(self):
        self.calls = []

    def __call__(self, paths, device, ncol=8, host_read=None, **kw):
        paths = list(paths)
        self.calls.append((paths, device, host_read))
        return [host_read(p) for p in paths], len(paths)


def _folders(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_eval
    return bench_eval.write_files(str(tmp_path), 3, 10, 5)


def test_metrics_reader_routes(tmp_path, monkeypatch):
    from rrnet_amd import textio
    from rrnet_amd.utils.metrics import metrics as M
    pd_dir, gt_dir = _folders(tmp_path)
    stub = _Stub()
    monkeypatch.setattr(textio, "read_files", stub)
    assert M._reader(pd_dir, gt_dir, "host", None) is M._read and stub.calls == []
    read = M._reader(pd_dir, gt_dir, "device", "cuda:0")
    (paths, device, host_read), = stub.calls
    assert device == "cuda:0" and host_read is M._read                       # fallbacks reach _read
    assert sorted(paths) == sorted(os.path.join(d, n) for d in (pd_dir, gt_dir) for n in os.listdir(d))
    for p in paths:
        assert np.array_equal(read(p), M._read(p))
    with pytest.raises(ValueError):
        M._reader(pd_dir, gt_dir, "gpu", None)
    # the defaults stay on the host: _sweep_read never asks textio
    stub.calls.clear()
    preds, targets, lens = M._sweep_read(pd_dir, gt_dir, [0.05], 500)
    assert stub.calls == [] and len(preds) == 3
    preds_d, targets_d, lens_d = M._sweep_read(pd_dir, gt_dir, [0.05], 500, text="device", device="cuda:0")
    assert len(stub.calls) == 1 and np.array_equal(lens, lens_d)
    assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(preds + targets, preds_d + targets_d))


def test_ensemble_reader_routes(tmp_path, monkeypatch):
    from rrnet_amd import ensemble, textio
    a_dir, _ = _folders(tmp_path / "a")
    b_dir, _ = _folders(tmp_path / "b")
    os.remove(os.path.join(b_dir, "0000001.txt"))
    open(os.path.join(b_dir, "0000002.txt"), "w").close()
    stub = _Stub()
    monkeypatch.setattr(textio, "read_files", stub)
    names, sets, missing = ensemble.read_result_dirs([a_dir, b_dir])
    assert stub.calls == [] and missing == 1
    names_d, sets_d, missing_d = ensemble.read_result_dirs([a_dir, b_dir], text="device", device="cuda:0")
    (paths, device, host_read), = stub.calls
    assert host_read is ensemble._read_or_empty and len(paths) == 6 and str(device) == "cuda:0"
    assert names_d == names and missing_d == 1
    for run, run_d in zip(sets, sets_d):
        assert len(run) == len(run_d) == 3
        for x, y in zip(run, run_d):
            assert x.shape == y.shape and np.array_equal(x, y)
    with pytest.raises(ValueError):
        ensemble.read_result_dirs([a_dir], text="gpu")
    with pytest.raises(ValueError):
        ensemble.write_result_dir(str(tmp_path / "o"), ["x"], [np.zeros((1, 6), np.float64)], text="device", device="cuda:0")
    ensemble.write_result_dir(str(tmp_path / "o"), ["x"], [np.asarray([[1.5, 2, 3, 4, 0.25, 7]], np.float64)])
    assert open(str(tmp_path / "o" / "x.txt")).read() == "1.500000,2.000000,3.000000,4.000000,0.2500,7,-1,-1\n"


def test_read_files_answers_missing_and_empty_files_without_a_device(tmp_path):
    """Nothing reaches the device when no file has bytes: the host function answers, and what it raises passes through."""
    from rrnet_amd import textio
    empty = str(tmp_path / "e.txt")
    open(empty, "w").close()
    seen = []
    out, n = textio.read_files([empty, str(tmp_path / "nope.txt")], "cuda:0", host_read=lambda p: seen.append(p))
    assert n == 2 and out == [None, None] and len(seen) == 2
    with pytest.raises(Exception):
        textio.read_files([empty], "cuda:0")                      # pandas' EmptyDataError, as metrics._read raises it
    assert textio.format_rows_host(np.asarray([[1.5, 2, 3.5, 4, 0.25, 7]]), 1, 1) == b"2,2,2,2,0.2500,7,-1,-1\n"


def test_text_route_reaches_the_device_evaluators(tmp_path, monkeypatch):
    """The public evaluators keep their signatures; metrics.text_route hands the route to the private functions."""
    from rrnet_amd.utils.metrics import metrics as M
    seen = []
    monkeypatch.setattr(M, "_evaluate_results_device", lambda *a, text="host": seen.append(("eval", text)))
    monkeypatch.setattr(M, "_auto_evaluate_results_device", lambda *a, text="host": seen.append(("auto", text)))
    M.evaluate_results("p", "t", device="cuda:0")
    with M.text_route("device"):
        M.evaluate_results("p", "t", device="cuda:0")
        M.auto_evaluate_results("p", "t", 0.05, 0.01, device="cuda:0")
        with M.text_route("host"):
            M.evaluate_results("p", "t", device="cuda:0")
    M.auto_evaluate_results("p", "t", 0.05, 0.01, device="cuda:0")
    assert seen == [("eval", "host"), ("eval", "device"), ("auto", "device"), ("eval", "host"), ("auto", "host")]
    with pytest.raises(ValueError):
        with M.text_route("gpu"):
            pass
    assert M._TEXT == ["host"]
