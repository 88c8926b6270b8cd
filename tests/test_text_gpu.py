"""The text codec on the device (csrc/textio.hip) against metrics._read, the writers' files and the host loops: equalities
throughout.  tests/text_cases.py builds the cases, tests/test_text_host.py proves them on the host."""
import os
import sys

import numpy as np
import pytest
import torch

import text_cases as tc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [0, 1, 63, 64, 65, 257, 1025]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def ops():
    from rrnet_amd import ops
    return ops


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _read(path):
    from rrnet_amd.utils.metrics.metrics import _read
    return _read(path)


def _parse_on_device(ops, dev, blobs):
    text, file_off = tc.pack_files(blobs)
    t, fo = torch.from_numpy(text).to(dev), torch.from_numpy(file_off).to(dev)
    line_pos, flo = ops.text_lines(t, fo)
    rows, flags = ops.text_parse(t, line_pos, 8)
    return text, file_off, rows.cpu().numpy(), flags.cpu().numpy(), line_pos.cpu().numpy(), flo.cpu().numpy()


def test_parse_equals_read_and_the_host_loops(ops, dev, tmp_path):
    """Clean and flagged files packed into one buffer behind a two-byte file (unaligned starts): line positions, per-file
    line ranges, flags and rows equal the host loops'; every clean file equals metrics._read bit for bit."""
    clean, bad = tc.clean_files(), tc.flagged_files()
    files = dict(clean, **bad)
    files["mixed_surplus"] = tc.mixed_surplus_file()
    names = sorted(files)
    paths = tc.write_files(str(tmp_path), files)
    blobs = [b"\n\n"] + [files[n] for n in names] + [b""]
    text, file_off, rows, flags, line_pos, flo = _parse_on_device(ops, dev, blobs)
    assert any(int(o) % 4 for o in file_off[1:-1])
    h_rows, h_flags, h_pos, h_flo = ops.text_parse_host(text, file_off, 8)
    assert np.array_equal(line_pos, h_pos) and np.array_equal(flo, h_flo) and np.array_equal(flags, h_flags)
    assert np.array_equal(_bits(rows), _bits(h_rows))
    assert flo[1] == 0 and flo[-1] == flo[-2] == rows.shape[0]
    for i, n in enumerate(names):
        got, fl = rows[flo[i + 1]:flo[i + 2]], flags[flo[i + 1]:flo[i + 2]]
        assert tc.file_on_device(fl) == (n in clean), n
        if n in clean:
            ref = _read(paths[n])
            assert ref.shape[0] == got.shape[0], n
            assert np.array_equal(_bits(got), _bits(ref[:, :8].astype(np.float64))), n


def test_lines_across_many_blocks(ops, dev):
    """More than one workgroup's bytes, lines of every length from 0 to 40 fields' worth, blank lines and CRLF mixed in."""
    rng = np.random.default_rng(5)
    lines = []
    for i in range(3000):
        k = int(rng.integers(0, 4))
        lines.append([b"", b"\r", b"1,2,3,4,0.5,1,-1,-1", b"10.250000,20.500000,3.000000,4.000000,0.1234,7,-1,-1\r"][k])
    blob = b"\n".join(lines) + b"\n"
    assert len(blob) > 8 * 4096
    cut = len(blob) // 3
    cut = blob.index(b"\n", cut) + 1
    text, file_off, rows, flags, line_pos, flo = _parse_on_device(ops, dev, [blob[:cut], blob[cut:]])
    h_rows, h_flags, h_pos, h_flo = ops.text_parse_host(text, file_off, 8)
    assert np.array_equal(line_pos, h_pos) and np.array_equal(flo, h_flo)
    assert np.array_equal(flags, h_flags) and np.array_equal(_bits(rows), _bits(h_rows))
    assert not flags.any() and rows.shape[0] == sum(1 for l in lines if l not in (b"", b"\r"))


def test_read_files_falls_back_per_file(dev, tmp_path):
    from rrnet_amd import textio
    good = tc.clean_files()
    files = {"a": good["rows65"], "b": tc.flagged_files()["exponent"], "c": good["crlf"], "d": tc.mixed_surplus_file(),
             "e": good["trailing_comma"]}
    paths = tc.write_files(str(tmp_path), files)
    order = ["a", "b", "c", "e"]
    seen = []

    def host_read(path):
        seen.append(os.path.basename(path))
        return _read(path)
    arrays, n_host = textio.read_files([paths[n] for n in order], dev, host_read=host_read)
    assert n_host == 1 and seen == ["b.txt"]
    for n, a in zip(order, arrays):
        ref = _read(paths[n])
        assert a.shape[0] == ref.shape[0] and np.array_equal(_bits(a[:, :8]), _bits(ref[:, :8].astype(np.float64))), n
    empty = str(tmp_path / "empty.txt")
    open(empty, "wb").close()
    seen.clear()
    arrays, n_host = textio.read_files([paths["a"], empty, str(tmp_path / "missing.txt"), paths["c"]], dev,
                                       host_read=lambda p: seen.append(os.path.basename(p)))
    assert n_host == 2 and seen == ["empty.txt", "missing.txt"] and arrays[1] is None and arrays[2] is None
    assert np.array_equal(_bits(arrays[3]), _bits(_read(paths["c"]).astype(np.float64)))
    with pytest.raises(Exception):                               # pandas' own error for the file it cannot read
        textio.read_files([paths["d"]], dev)
    # chunked uploads give the same arrays
    small, _ = textio.read_files([paths[n] for n in ("a", "c", "e")], dev, chunk_bytes=64)
    for n, a in zip(("a", "c", "e"), small):
        assert np.array_equal(_bits(a), _bits(_read(paths[n])[:, :8].astype(np.float64))), n


def _frame_offsets(r):
    """Frames of uneven sizes with an empty one in the middle."""
    return [0, r // 3, r // 3, (2 * r) // 3, r]


def _write_host(folder, names, rows, off, layout):
    from rrnet_amd import ensemble
    from rrnet_amd.operators.centernet_operator import CenterNetOperator
    from rrnet_amd.operators.retinanet_operator import RetinaNetOperator
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    os.makedirs(folder, exist_ok=True)
    if layout == 2:
        RetinaNetOperator.write_results(folder, names, rows, off)
        return
    for i, name in enumerate(names):
        part = rows[off[i]:off[i + 1]]
        if layout == 1:
            CenterNetOperator.write_results(os.path.join(folder, name + ".txt"), part)
        elif layout == 0:
            RRNetOperator.write_results(os.path.join(folder, name + ".txt"), part)
        else:                                                     # ensemble.format_rows: layout 0 without the clamp
            with open(os.path.join(folder, name + ".txt"), "w") as f:
                f.write(ensemble.format_rows(part))


def _rows(r, seed):
    rows = tc.detection_rows(r, seed=seed)
    special = tc.special_floats()
    ok = special[np.isfinite(special) & (np.abs(special) < 2.0 ** 40)]
    rng = np.random.default_rng(seed)
    for c in range(5):                                            # ties, tiny and large values in a fifth of the slots
        pick = rng.random(r) < 0.2
        rows[pick, c] = ok[rng.integers(0, ok.size, int(pick.sum()))]
    return rows


@pytest.mark.parametrize("r", SIZES)
def test_format_equals_the_writers_files(ops, dev, tmp_path, r):
    """All three write_results and ensemble.format_rows, file for file; the device and host entry points agree; the buffer
    beyond the last byte keeps its sentinel."""
    from rrnet_amd import textio
    rows = _rows(r, seed=r + 1)
    off = _frame_offsets(r)
    names = ["f%d" % i for i in range(4)]
    d_rows = torch.from_numpy(rows).to(dev)
    for layout, clamp, which in ((0, 1, 0), (1, 1, 1), (2, 1, 2), (0, 0, 3)):
        host_dir, dev_dir = str(tmp_path / ("h%d" % which)), str(tmp_path / ("d%d" % which))
        _write_host(host_dir, names, rows, off, which)
        os.makedirs(dev_dir)
        textio.write_frames([os.path.join(dev_dir, n + ".txt") for n in names], d_rows, off, layout, clamp)
        for n in names:
            assert open(os.path.join(dev_dir, n + ".txt"), "rb").read() == open(os.path.join(host_dir, n + ".txt"), "rb").read()
        length, flag, byte_off = ops.text_format_len(d_rows, layout, clamp)
        total = int(byte_off[-1])
        buf = torch.full((total + 300,), 0xA5, dtype=torch.uint8, device=dev)
        ops.text_format(d_rows, layout, clamp, byte_off, buf[3:])                # an odd start address
        got = buf.cpu().numpy()
        h_out, h_off, h_flag = ops.text_format_host(rows, layout, clamp)
        assert np.array_equal(byte_off.cpu().numpy(), h_off) and np.array_equal(flag.cpu().numpy(), h_flag)
        assert np.array_equal(got[3:3 + total], h_out)
        assert (got[:3] == 0xA5).all() and (got[3 + total:] == 0xA5).all()
        assert not h_flag.any()


def test_format_flagged_rows_and_host_fallback(ops, dev):
    """Flagged rows take no bytes and set the flag; format_frames hands exactly their frames to the host expression."""
    from rrnet_amd import textio
    ok = tc.detection_rows(300, seed=4)
    rows = ok.copy()
    rows[150, 0] = np.float32(2.0 ** 63)
    rows[10, 5] = np.float32(3.9)
    d_rows = torch.from_numpy(rows).to(dev)
    for layout in (0, 1, 2):
        length, flag, byte_off = ops.text_format_len(d_rows, layout, 1)
        h_out, h_off, h_flag = ops.text_format_host(rows, layout, 1)
        assert flag.cpu().numpy().tolist() == h_flag.tolist() and h_flag.sum() == 1 and h_flag[150] == 1
        buf = torch.full((int(byte_off[-1]) + 64,), 0xA5, dtype=torch.uint8, device=dev)
        ops.text_format(d_rows, layout, 1, byte_off, buf)
        got = buf.cpu().numpy()
        assert np.array_equal(got[:h_out.size], h_out) and (got[h_out.size:] == 0xA5).all()
        frames = textio.format_frames(d_rows, [0, 100, 200, 300], layout, 1)
        for i in range(3):
            assert bytes(frames[i]) == textio.format_rows_host(rows[100 * i:100 * (i + 1)], layout, 1)
    bad = ok.copy()
    bad[5, 5] = np.nan
    with pytest.raises(ValueError):                               # int(nan): what write_results raises
        textio.format_frames(torch.from_numpy(bad).to(dev), [0, 300], 0, 1)


def test_round_trip(ops, dev):
    """2000 rows whose values six (four) decimals hold exactly: format -> parse -> float32 gives them back."""
    rows = tc.detection_rows(2000, seed=9)
    rows[:, :4] = np.round(rows[:, :4] * 64) / 64
    rows[:, 4] = np.round(rows[:, 4] * 10000) / 10000
    rows = np.abs(rows).astype(np.float32)
    d_rows = torch.from_numpy(rows).to(dev)
    length, flag, byte_off = ops.text_format_len(d_rows, 0, 0)
    buf = torch.empty(int(byte_off[-1]), dtype=torch.uint8, device=dev)
    ops.text_format(d_rows, 0, 0, byte_off, buf)
    line_pos, flo = ops.text_lines(buf, torch.tensor([0, buf.numel()], dtype=torch.int64, device=dev))
    back, flags = ops.text_parse(buf, line_pos, 8)
    assert int(flag.sum()) == 0 and int(flags.sum()) == 0 and flo.tolist() == [0, 2000]
    assert np.array_equal(line_pos.cpu().numpy(), byte_off[:-1].cpu().numpy())
    back = back.cpu().numpy()
    assert np.array_equal(back[:, :6].astype(np.float32), rows) and (back[:, 6:] == -1).all()


def test_fusion_and_evaluation_through_the_device_text_route(dev, tmp_path, capsys):
    """fuse_result_dirs(text="device") and the evaluators under metrics.text_route("device") on 3 x 6 generated files against
    the host route: files byte for byte, AP with ==.  (The evaluators' public signatures are pinned by
    test_eval_device_host.py, so their route is a context manager; the private functions carry the text= keyword.)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bench_eval
    from rrnet_amd import ensemble, textio
    from rrnet_amd.utils.metrics import metrics as M
    runs, gt_dir = [], None
    for m in range(3):
        pd_dir, gt = bench_eval.write_files(str(tmp_path / ("run%d" % m)), 6, 40, 12, seed=219 + m)
        runs.append(pd_dir)
        gt_dir = gt_dir or gt
    os.remove(os.path.join(runs[2], "0000003.txt"))               # a file one run lacks
    host_read = []
    real = textio.read_files

    def spy(paths, device, **kw):
        out, n = real(paths, device, **kw)
        host_read.append((len(list(paths)), n))
        return out, n
    textio.read_files = spy
    try:
        missing_h = ensemble.fuse_result_dirs(runs, str(tmp_path / "fused_host"), device=dev)
        missing_d = ensemble.fuse_result_dirs(runs, str(tmp_path / "fused_dev"), device=dev, text="device")
        assert missing_h == missing_d == 1 and host_read == [(18, 1)]            # the missing file alone went to the host
        names = sorted(os.listdir(str(tmp_path / "fused_host")))
        assert len(names) == 6 and names == sorted(os.listdir(str(tmp_path / "fused_dev")))
        for n in names:
            a, b = (open(os.path.join(str(tmp_path / d), n), "rb").read() for d in ("fused_host", "fused_dev"))
            assert a == b and len(a) > 0, n
        host_read.clear()
        ap_h, rc_h = M.evaluate_results(str(tmp_path / "fused_dev"), gt_dir, device=dev)
        with M.text_route("device"):
            ap_d, rc_d = M.evaluate_results(str(tmp_path / "fused_dev"), gt_dir, device=dev)
        assert host_read == [(12, 0)]                              # no file of the generated folders is flagged
        assert torch.equal(ap_h, ap_d) and float(rc_h) == float(rc_d) and float(ap_h.max()) > 0
        ap_a, rc_a = M.auto_evaluate_results(runs[0], gt_dir, 0.05, 0.01, device=dev)
        with M.text_route("device"):
            ap_b, rc_b = M.auto_evaluate_results(runs[0], gt_dir, 0.05, 0.01, device=dev)
        assert torch.equal(ap_a, ap_b) and float(rc_a) == float(rc_b)
        sw_a = M.sweep_evaluate_results(runs[0], gt_dir, [0.05, 0.1], [0.01, 0.05], device=dev)
        with M.text_route("device"):
            sw_b = M.sweep_evaluate_results(runs[0], gt_dir, [0.05, 0.1], [0.01, 0.05], device=dev)
        assert M._TEXT == ["host"]
        assert np.array_equal(sw_a, sw_b)
    finally:
        textio.read_files = real
