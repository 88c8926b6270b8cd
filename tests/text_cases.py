"""The text codec's contract (include/rrnet_hip.h, "VisDrone text files") restated in pure Python integers, the Python
expressions it must equal, and the case builders test_text_host.py and test_text_gpu.py share.  Nothing here imports the
library."""
import os
import struct

import numpy as np

FLAG = None                      # what the restatement answers where the codec flags


# ---- format: integers only -------------------------------------------------------------------------------------------

def split_float(v):
    """float32 -> (sign, m, e) with |v| = m * 2^e, or (sign, None, mantissa bits) for infinity / NaN."""
    u = struct.unpack("<I", struct.pack("<f", v))[0]
    sign, ex, mant = u >> 31, (u >> 23) & 0xff, u & 0x7fffff
    if ex == 255:
        return sign, None, mant
    return (sign, mant | 0x800000, ex - 150) if ex else (sign, mant, -149)


def fmt_fixed(v, decimals):
    sign, m, e = split_float(v)
    if m is None:
        return "nan" if e else ("-inf" if sign else "inf")
    p10 = 10 ** decimals
    if e >= 0:
        if e > 39:
            return FLAG
        q = (m << e) * p10
    else:
        sh = -e
        if sh >= 64:
            q = 0
        else:
            n = m * p10
            q, rem, half = n >> sh, n & ((1 << sh) - 1), 1 << (sh - 1)
            if rem > half or (rem == half and q & 1):
                q += 1
    return "%s%d.%0*d" % ("-" if sign else "", q // p10, decimals, q % p10)


def to_int(v):
    sign, m, e = split_float(v)
    if m is None or e > 39:
        return FLAG
    a = m << e if e >= 0 else (0 if -e >= 24 else m >> -e)
    return -a if sign else a


def fmt_row(r6, layout, clamp):
    """One row of six float32 -> its bytes, or FLAG."""
    v = [np.float32(x) for x in r6]
    if clamp:
        v = [np.float32(0.0) if x < 0 else x for x in v]
    if layout == 0:
        head = [fmt_fixed(x, 6) for x in v[:4]]
    else:
        c = [to_int(np.rint(x) if layout == 1 else x) for x in v[:4]]
        if any(x is FLAG for x in c) or (layout == 1 and any(abs(x) >= 1 << 62 for x in c)):
            return FLAG
        if layout == 1:
            c = [c[0], c[1], c[2] - c[0], c[3] - c[1]]
        head = ["%d" % x for x in c]
    score, cls = fmt_fixed(v[4], 4), to_int(v[5])
    if any(x is FLAG for x in head) or score is FLAG or cls is FLAG:
        return FLAG
    return (",".join(head) + "," + score + "," + "%d" % cls + ",-1,-1\n").encode()


def must_flag(r6, layout, clamp):
    """The rows the contract hands to the host, straight from its words: a finite |v| >= 2^63 anywhere, NaN or infinity under
    %d, and in layout 1 a rounded corner at or beyond 2^62."""
    v = np.asarray(r6, np.float32).astype(np.float64)
    if clamp:
        v = np.where(v < 0, 0.0, v)
    as_int = [5] if layout == 0 else [0, 1, 2, 3, 5]
    if (np.isfinite(v) & (np.abs(v) >= 2.0 ** 63)).any() or not np.isfinite(v[as_int]).all():
        return True
    return layout == 1 and bool((np.abs(np.rint(v[:4])) >= 2.0 ** 62).any())


def python_row(r6, layout, clamp):
    """The writers' own expressions (the three write_results and ensemble.format_rows); FLAG where Python raises."""
    rows = np.asarray(r6, np.float32).reshape(1, 6)
    if clamp:
        rows = np.where(rows < 0, np.float32(0.), rows)
    if layout == 1:
        rows = np.concatenate((np.rint(rows[:, :4]), rows[:, 4:]), axis=1)
    r = rows.tolist()[0]
    try:
        if layout == 0:
            return ("%f,%f,%f,%f,%.4f,%d,-1,-1\n" % (r[0], r[1], r[2], r[3], r[4], int(r[5]))).encode()
        if layout == 1:
            return ("%d,%d,%d,%d,%.4f,%d,-1,-1\n" % (int(r[0]), int(r[1]), int(r[2]) - int(r[0]), int(r[3]) - int(r[1]),
                                                     r[4], int(r[5]))).encode()
        return ("%d,%d,%d,%d,%.4f,%d,-1,-1\n" % (int(r[0]), int(r[1]), int(r[2]), int(r[3]), r[4], int(r[5]))).encode()
    except (ValueError, OverflowError):
        return FLAG


# ---- parse: integers and one division ----------------------------------------------------------------------------------

def parse_field(s):
    """bytes of one field -> float, or FLAG."""
    i, neg = 0, False
    if s[:1] in (b"+", b"-"):
        neg, i = s[:1] == b"-", 1
    whole = i
    while i < len(s) and 48 <= s[i] <= 57:
        i += 1
    digits, k = s[whole:i], 0
    if s[i:i + 1] == b".":
        j = i + 1
        while j < len(s) and 48 <= s[j] <= 57:
            j += 1
        k = j - i - 1
        digits, i = digits + s[i + 1:j], j
    if i != len(s) or not digits or k > 22 or len(digits) > 17:     # pandas reads 17 digit characters of a field
        return FLAG
    d = int(digits)
    if d >= 1 << 53 or (neg and d == 0):
        return FLAG
    v = float(d) / float(10 ** k)
    return -v if neg else v


def parse_text(data, ncol=8):
    """bytes of one file (ending in a newline unless empty) -> (rows float64 [L,ncol], flags int [L]) by the contract:
    0, 2 (one empty surplus field) or 1 (flagged)."""
    rows, flags = [], []
    for line in data.split(b"\n")[:-1] if data.endswith(b"\n") else data.split(b"\n"):
        if line in (b"", b"\r"):
            continue
        if line.endswith(b"\r"):
            line = line[:-1]
        fields = line.split(b",") if b"\r" not in line else []
        vals = [parse_field(f) for f in fields[:ncol]]
        surplus = fields[ncol:]
        if len(vals) < ncol or any(v is FLAG for v in vals) or (surplus and surplus != [b""]):
            rows.append([0.0] * ncol)          # what a flagged line leaves in its row is not compared
            flags.append(1)
        else:
            rows.append(vals)
            flags.append(2 if surplus else 0)
    return np.asarray(rows, np.float64).reshape(-1, ncol), np.asarray(flags, np.int32)


def file_on_device(flags):
    """Whether a file with these line flags stays on the device route: some line, none flagged, the surplus field on all lines
    or on none (pandas fixes the column count by the first line)."""
    flags = np.asarray(flags)
    return flags.size > 0 and not (flags & 1).any() and ((flags == 2).all() or (flags == 0).all())


# ---- cases -----------------------------------------------------------------------------------------------------------

def special_floats():
    """The values the issue lists: ties, [0,1), tiny to huge, zeros, infinities, NaNs, subnormals, 2^24, +-2^62, 2^63."""
    rng = np.random.default_rng(11)
    k = np.arange(-4096, 4096, dtype=np.float32)
    parts = [
        rng.uniform(-3000, 3000, 4000).astype(np.float32), k / np.float32(64), k / np.float32(128), k / np.float32(32) + np.float32(0.5),
        rng.uniform(0, 1, 2000).astype(np.float32),
        (10.0 ** rng.uniform(-45, 18, 3000)).astype(np.float32), -(10.0 ** rng.uniform(-45, 18, 1000)).astype(np.float32),
        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 2.0 ** 24, 2.0 ** 24 + 2, 2.0 ** 62, -2.0 ** 62, 2.0 ** 63, -2.0 ** 63,
                  2.0 ** 64, 3.4028235e38, 1e-45, -1e-45, 1.1754942e-38, 1.17549435e-38, 0.5, 1.5, 2.5, -0.5, -1.5, 0.00005,
                  0.0000005, 0.99995, 0.9999995, 9.9999995, 999999.5, 0.49999997, 8388607.5, 4194303.75], np.float32),
        np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x00000001, 0x807fffff, 0x007fffff, 0x5effffff, 0xdeffffff],
                 np.uint32).view(np.float32),
    ]
    return np.concatenate(parts)


def strided_floats(stride=4093, start=7):
    """Every stride-th float32 bit pattern (a prime stride walks through all exponents and both signs)."""
    return np.arange(start, 1 << 32, stride, dtype=np.uint64).astype(np.uint32).view(np.float32)


def rows_from_values(vals, seed=0):
    """[R,6] rows whose every column walks through `vals` in a different order."""
    vals = np.asarray(vals, np.float32)
    rng = np.random.default_rng(seed)
    return np.stack([vals] + [vals[rng.permutation(vals.size)] for _ in range(5)], 1)


def detection_rows(n, seed=0):
    """Rows as the detectors produce them: coordinates in a frame, scores in (0, 1), classes 1..10."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-5, 1900, (n, 2)); wh = rng.uniform(0, 300, (n, 2))
    return np.concatenate([xy, wh, rng.uniform(0, 1, (n, 1)), rng.integers(1, 11, (n, 1))], 1).astype(np.float32)


def flagged_rows():
    """(row, layouts in which it must be flagged) with clamp off."""
    base = [10.5, 20.25, 30.0, 40.0, 0.5, 3.0]

    def put(col, v):
        r = list(base)
        r[col] = v
        return np.asarray(r, np.float32)
    return [(put(5, np.nan), (0, 1, 2)), (put(5, np.inf), (0, 1, 2)), (put(5, 2.0 ** 63), (0, 1, 2)),
            (put(4, 2.0 ** 63), (0, 1, 2)), (put(0, -2.0 ** 63), (0, 1, 2)), (put(1, np.inf), (1, 2)), (put(2, np.nan), (1, 2)),
            (put(3, 2.0 ** 62), (1,))]


def _line(r):
    return "%f,%f,%f,%f,%.4f,%d,-1,-1" % (r[0], r[1], r[2], r[3], r[4], int(r[5]))


def clean_files():
    """name -> bytes of files every line of which the codec parses."""
    files = {}
    for n in (1, 63, 64, 65, 257):
        files["rows%d" % n] = ("\n".join(_line(r) for r in detection_rows(n, seed=n).tolist()) + "\n").encode()
    rows = detection_rows(5, seed=5).tolist()
    files["crlf"] = ("\r\n".join(_line(r) for r in rows) + "\r\n").encode()
    files["blank_lines"] = ("\n\n" + _line(rows[0]) + "\n\n\r\n" + _line(rows[1]) + "\n\n").encode()
    files["no_final_newline"] = (_line(rows[0]) + "\n" + _line(rows[1])).encode()
    files["trailing_comma"] = b"684,8,273,116,0,0,0,0,\n406,119,265,70,0,0,0,0,\n"
    files["integers"] = b"684,8,273,116,0,0,0,0\n406,119,265,70,1,4,0,1\n255,22,119,128,1,9,0,2\n"
    files["signs_and_points"] = b"+1.5,.5,5.,-2.25,0.5000,3,-1,-1\n1,2,3,4,+.25,1,-1,-1\n"
    files["digits17"] = b"0.1234567890123456,0123456.7890123456,00000000000000012,1,0.5,1,-1,-1\n"
    files["below_2_53"] = b"9007199254740991,900719925474.0991,1,1,0.5,1,-1,-1\n"
    files["leading_zeros"] = b"000012.500,0007,1,1,0.5,1,-1,-1\n"
    return files


def flagged_files():
    """name -> bytes of files with a line that must be flagged (each holds clean lines around it)."""
    ok = b"1.000000,2.000000,3.000000,4.000000,0.5000,1,-1,-1\n"
    bad = {"exponent": b"1e3,2,3,4,0.5,1,-1,-1\n", "nan": b"nan,2,3,4,0.5,1,-1,-1\n", "minus_zero": b"-0,2,3,4,0.5,1,-1,-1\n",
           "minus_zero_point": b"1,2,3,4,-0.0000,1,-1,-1\n", "blank": b"1, 2,3,4,0.5,1,-1,-1\n",
           "short": b"1,2,3,4,0.5,1\n", "two_surplus": b"1,2,3,4,0.5,1,-1,-1,7,8\n", "surplus_value": b"1,2,3,4,0.5,1,-1,-1,7\n",
           "digits23": b"0.00000000001234567890123,1,1,1,0.5,1,-1,-1\n",
           "digits22": b"0.0000000001234567890123,1,1,1,0.5,1,-1,-1\n", "digits18": b"0.12345678901234567,1,1,1,0.5,1,-1,-1\n",
           "zeros18": b"000000000000000012.5,1,1,1,0.5,1,-1,-1\n", "at_2_53": b"9007199254740992,1,1,1,0.5,1,-1,-1\n",
           "empty_field": b"1,,3,4,0.5,1,-1,-1\n", "inf": b"1,2,inf,4,0.5,1,-1,-1\n", "lone_cr": b"1,2,3,4,0.5,1,-1,-1\r1,2\n",
           "only_sign": b"1,-,3,4,0.5,1,-1,-1\n", "only_point": b"1,.,3,4,0.5,1,-1,-1\n"}
    return {name: ok + line + ok for name, line in bad.items()}


def mixed_surplus_file():
    """Every line parses, but only the second carries the trailing comma: pandas raises on it, so the file belongs to the host."""
    return b"1,2,3,4,0,0,0,0\n1,2,3,4,0,0,0,0,\n"


def pack_files(blobs):
    """list of bytes -> (uint8 buffer with every non-empty file ending in a newline, int64 file_off [F+1])."""
    parts, off = [], [0]
    for b in blobs:
        if b and not b.endswith(b"\n"):
            b = b + b"\n"
        parts.append(b)
        off.append(off[-1] + len(b))
    return np.frombuffer(b"".join(parts), np.uint8).copy(), np.asarray(off, np.int64)


def write_files(folder, files):
    os.makedirs(folder, exist_ok=True)
    paths = {}
    for name, data in files.items():
        paths[name] = os.path.join(folder, name + ".txt")
        with open(paths[name], "wb") as f:
            f.write(data)
    return paths
