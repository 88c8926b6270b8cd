"""Host-side tests of rrnet_amd._C.call, the one helper every binding reaches the C ABI through: what it refuses before an
entry point is fetched (a host tensor for a device pointer, a dtype the header's pointee does not admit, a tensor where the
header declares a number, a wrong argument count), what it passes on (NULL for None, the current stream where the prototype
ends in one, read per call), how a failing status is reported, and that the header parser knows every pointee.  No GPU: the
entry points are stubs that convert their arguments the way ctypes would, or host-only entries of the real library."""
import ctypes

import pytest
import torch

from rrnet_amd import _C

SIGS = _C.header_signatures()


class _OnDevice(torch.Tensor):
    """A host tensor that says it lives on the device: what a device tensor is to _C.call, without a GPU.  Only ever handed
    to a stub."""
    is_cuda = True


def on_device(t):
    return t.as_subclass(_OnDevice)


class Stub:
    """Stands in for _C.fn: hands out entries that carry the header's argtypes, convert every argument with them (as the
    foreign call would) and record what arrived.  reachable=False: any lookup fails the test."""

    def __init__(self, monkeypatch, reachable=True, rc=0):
        self.reachable, self.rc, self.lookups, self.calls, self.streams = reachable, rc, [], [], 0
        monkeypatch.setattr(_C, "fn", self.fn)
        monkeypatch.setattr(_C, "stream", self.stream)

    def stream(self):
        self.streams += 1
        return ctypes.c_void_p(0x1000 * self.streams)        # a new stream at every read

    def fn(self, name, *a, **kw):
        assert self.reachable, "%s was looked up" % name
        self.lookups.append(name)

        def entry(*args):
            assert len(args) == len(entry.argtypes), (name, len(args))
            for t, v in zip(entry.argtypes, args):
                t.from_param(v)                              # raises on what ctypes would not take
            self.calls.append((name, args))
            return self.rc
        entry.restype, entry.argtypes = SIGS[name]
        return entry


def _addr(v):
    return v.value if isinstance(v, ctypes.c_void_p) else v


def test_device_tensors_go_in_as_their_addresses_and_the_entry_is_fetched_once(monkeypatch):
    stub = Stub(monkeypatch)
    x, out = on_device(torch.zeros(8)), on_device(torch.zeros(8))
    assert _C.call("rr_relu_fwd", x, out, 8) is None
    assert stub.lookups == ["rr_relu_fwd"]
    (name, args), = stub.calls
    assert [_addr(a) for a in args] == [x.data_ptr(), out.data_ptr(), 8, 0x1000]
    assert all(isinstance(a, ctypes.c_void_p) for a in (args[0], args[1], args[3]))


def test_host_tensor_for_a_device_pointer_is_refused_before_the_entry_is_reached(monkeypatch):
    Stub(monkeypatch, reachable=False)
    with pytest.raises(_C.RRNetHipError, match="MI355X only: got a cpu tensor"):
        _C.call("rr_relu_fwd", on_device(torch.zeros(8)), torch.zeros(8), 8)
    with pytest.raises(_C.RRNetHipError) as e:
        _C.call("rr_relu_fwd", torch.zeros(8), torch.zeros(8), 8)
    with pytest.raises(_C.RRNetHipError) as want:
        _C.require_cuda(torch.zeros(8))
    assert str(e.value) == str(want.value)                   # require_cuda's own message


def test_host_entries_take_host_tensors(monkeypatch):
    stub = Stub(monkeypatch)
    text, pos = torch.zeros(16, dtype=torch.uint8), torch.zeros(2, dtype=torch.int64)
    rows, flags = torch.zeros((2, 8), dtype=torch.float64), torch.zeros(2, dtype=torch.int32)
    _C.call("rr_text_parse_host", text, 16, pos, 2, 8, rows, flags)
    (_, args), = stub.calls
    assert [_addr(a) for a in args] == [text.data_ptr(), 16, pos.data_ptr(), 2, 8, rows.data_ptr(), flags.data_ptr()]
    assert stub.streams == 0                                 # no hipStream_t in that prototype: none appended


@pytest.mark.parametrize("entry,args,bad", [
    ("rr_relu_fwd", lambda: (torch.zeros(8, dtype=torch.float64), torch.zeros(8), 8), "torch.float64 tensor.*declares float"),
    ("rr_text_parse_host", lambda: (torch.zeros(16, dtype=torch.uint8), 16, torch.zeros(2, dtype=torch.int64), 2, 8,
                                    torch.zeros((2, 8), dtype=torch.int32), torch.zeros(2, dtype=torch.int32)),
     "torch.int32 tensor.*declares double"),
    ("rr_to_bf16", lambda: (torch.zeros(8), torch.zeros(8, dtype=torch.int32), 8), "torch.int32 tensor.*declares unsigned short"),
    ("rr_absmax_bits", lambda: (torch.zeros(8), 8, torch.zeros(1, dtype=torch.float64)), "torch.float64 tensor.*declares unsigned"),
    ("rr_sum_n", lambda: (torch.zeros(8), 1, None, torch.zeros(8), 8), r"declares float \* \*"),
])
def test_dtype_the_pointee_does_not_admit_is_refused(monkeypatch, entry, args, bad):
    Stub(monkeypatch, reachable=False)
    with pytest.raises(_C.RRNetHipError, match=bad) as e:
        _C.call(entry, *[on_device(a) if torch.is_tensor(a) else a for a in args()])
    assert str(e.value).startswith(entry + ": argument ")


def test_void_pointer_takes_any_dtype_and_none_is_null(monkeypatch):
    stub = Stub(monkeypatch)
    rows, off = on_device(torch.zeros((4, 6))), on_device(torch.zeros(2, dtype=torch.int32))
    keep, kept = on_device(torch.zeros(4, dtype=torch.int32)), on_device(torch.zeros(1, dtype=torch.int32))
    for ws in (on_device(torch.zeros(64, dtype=torch.uint8)), on_device(torch.zeros(8, dtype=torch.float64)), None):
        _C.call("rr_nms_frames", rows, off, 1, 4, 0.5, 0, ws, keep, kept)
        args = stub.calls[-1][1]
        assert _addr(args[6]) == (ws.data_ptr() if ws is not None else None)
    _C.call("rr_bn_bwd_reduce", rows, None, rows, rows, rows, None, None, on_device(torch.zeros(4, dtype=torch.float64)), 4, 6, 1)
    args = stub.calls[-1][1]
    assert [i for i, a in enumerate(args) if _addr(a) is None] == [1, 5, 6]
    # the 16-bit pointee: bf16 images and the fp16 parts of a split filter
    for dt in (torch.bfloat16, torch.float16):
        _C.call("rr_to_bf16", on_device(torch.zeros(8)), on_device(torch.zeros(8, dtype=dt)), 8)


def test_ctypes_pointers_and_numpy_addresses_pass_through(monkeypatch):
    stub = Stub(monkeypatch)
    arr = (ctypes.c_void_p * 2)(1, 2)
    cast, out = ctypes.cast(arr, ctypes.c_void_p), on_device(torch.zeros(8))
    _C.call("rr_sum_n", cast, 2, None, out, 8)
    assert stub.calls[-1][1][0] is cast
    buf = (ctypes.c_int * 32)()
    _C.call("rr_wbf_plan", 4, 64, buf, 32)
    assert stub.calls[-1][1][2] is buf
    addr = _C.c_void_p(0x40)
    _C.call("rr_text_parse_host", addr, 0, addr, 0, 8, addr, addr)
    assert all(a is addr for a in stub.calls[-1][1][::2][:2])


def test_tensor_where_the_header_declares_a_number_is_refused(monkeypatch):
    Stub(monkeypatch, reachable=False)
    x = on_device(torch.zeros(8))
    with pytest.raises(_C.RRNetHipError, match="rr_relu_fwd: argument 2 is a tensor"):
        _C.call("rr_relu_fwd", x, x, on_device(torch.tensor(8)))
    with pytest.raises(_C.RRNetHipError, match="rr_bn_eval_coeffs: argument 4 is a tensor"):
        _C.call("rr_bn_eval_coeffs", x, x, x, x, on_device(torch.tensor(1e-5)), x, x, 8)


def test_argument_count_is_checked_against_the_header(monkeypatch):
    Stub(monkeypatch, reachable=False)
    x = on_device(torch.zeros(8))
    for args in ((x, x), (x, x, 8, 9), (x, x, 8, _C.c_void_p(0))):        # one too few, one too many, the stream spelled out
        with pytest.raises(_C.RRNetHipError, match=r"^rr_relu_fwd takes 3 arguments and the stream .* got %d$" % len(args)):
            _C.call("rr_relu_fwd", *args)
    with pytest.raises(_C.RRNetHipError, match=r"^rr_conv_stat_slab_bytes takes 4 arguments \(.*got 5$"):
        _C.call("rr_conv_stat_slab_bytes", 1, 2, 3, 4, 5)
    with pytest.raises(_C.RRNetHipError, match="rr_no_such_entry is not declared"):
        _C.call("rr_no_such_entry", 1)


def test_stream_is_appended_only_where_the_prototype_ends_in_one_and_is_read_at_every_call(monkeypatch):
    stub = Stub(monkeypatch)
    x = on_device(torch.zeros(8))
    _C.call("rr_relu_fwd", x, x, 8)
    _C.call("rr_relu_fwd", x, x, 8)
    assert [_addr(args[-1]) for _, args in stub.calls] == [0x1000, 0x2000] and stub.streams == 2
    _C.call("rr_conv_stat_slab_bytes", 2, 8, 8, 64)
    assert stub.streams == 2 and stub.calls[-1][1] == (2, 8, 8, 64)
    with_stream = [n for n, s in SIGS.items() if s.pointees[-1:] == ("hipStream_t",)]
    assert len(with_stream) == 139 and all("hipStream_t" not in s.pointees[:-1] for s in SIGS.values())


def test_status_raises_under_the_entry_name_and_counts_come_back(monkeypatch):
    stub = Stub(monkeypatch, rc=7)
    x = on_device(torch.zeros(8))
    with pytest.raises(_C.RRNetHipError, match=r"^rr_relu_fwd failed \(7\): "):
        _C.call("rr_relu_fwd", x, x, 8)
    # size_t, and int-returning entries whose value is a count: handed back, never read as a status
    for name, args in (("rr_conv_stat_slab_bytes", (2, 8, 8, 64)), ("rr_grad_norm_blocks", (1024,)), ("rr_conv16_supported", (128, 128, 3, 3, 1)),
                       ("rr_dcn_fused_bwd_supported_dil", (64, 64, 3, 3, 1, 1, 1)), ("rr_abi_version", ())):
        assert _C.call(name, *args) == 7
    assert stub.lookups[0] == "rr_relu_fwd" and len(stub.lookups) == 6


def test_real_library_refusal_carries_the_entry_name_and_its_last_error():
    """Host-only entries of the built library: nothing is launched."""
    buf = (ctypes.c_int * 32)()
    with pytest.raises(_C.RRNetHipError) as e:
        _C.call("rr_wbf_plan", 1, 8193, buf, 32)
    text = _C.lib().rr_last_error().decode()
    assert "8193" in text and str(e.value).startswith("rr_wbf_plan failed (") and str(e.value).endswith("): " + text)
    _C.call("rr_wbf_plan", 1, 64, buf, 32)                   # and a plan it takes
    assert _C.call("rr_conv_stat_slab_bytes", 2, 8, 8, 64) > 0 and _C.call("rr_abi_version") == 1
    from rrnet_amd import ops
    with pytest.raises(_C.RRNetHipError, match=r"^rr_wbf_plan failed \("):
        ops.wbf_plan(1, 8193)


KNOWN_POINTEES = {"float", "double", "int", "unsigned", "unsigned short", "unsigned char", "signed char", "long", "long long",
                  "unsigned long long", "void", "float *"}


def test_header_has_171_entries_and_every_pointee_has_its_dtypes():
    assert len(SIGS) == 171
    assert set(_C.POINTEE_DTYPES) == KNOWN_POINTEES
    sizes = {"float": 4, "double": 8, "int": 4, "unsigned": 4, "unsigned short": 2, "unsigned char": 1, "signed char": 1, "long": 8,
             "long long": 8, "unsigned long long": 8}
    for pointee, size in sizes.items():
        assert _C.POINTEE_DTYPES[pointee] and all(torch.empty(0, dtype=d).element_size() == size for d in _C.POINTEE_DTYPES[pointee])
    assert _C.POINTEE_DTYPES["void"] is None and _C.POINTEE_DTYPES["float *"] == ()


@pytest.mark.parametrize("name", sorted(SIGS))
def test_every_pointer_parameter_has_a_known_pointee(name):
    restype, argtypes = SIGS[name]
    pointees = SIGS[name].pointees
    assert len(pointees) == len(argtypes)
    for argtype, pointee in zip(argtypes, pointees):
        if pointee == "hipStream_t" or pointee is None:
            assert pointee is None or argtype is _C.c_void_p
            assert pointee is not None or argtype is not _C.c_void_p
        else:
            assert argtype is _C.c_void_p and pointee in KNOWN_POINTEES, (name, pointee)
