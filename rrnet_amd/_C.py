"""ctypes binding of librrnet_hip.so (include/rrnet_hip.h, and a kernel family's companion header beside it: Family).

The product path has no CPU fallback: if the HIP library is missing or an entry point is
absent, importing/using an op raises — loudly — instead of computing something else."""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "librrnet_hip.so")
_lib = None

c_int, c_float, c_void_p, c_size_t = ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t
c_long, c_double = ctypes.c_long, ctypes.c_double


class RRNetHipError(RuntimeError):
    pass


def lib():
    global _lib
    if _lib is None:
        global LIB_PATH
        LIB_PATH = os.environ.get("RRNET_HIP_LIB", LIB_PATH)     # kernel experiments: an alternative build of the library
        if not os.path.exists(LIB_PATH):
            raise RRNetHipError(
                "librrnet_hip.so not found at %s — build it with `python rrnet_amd/csrc/build.py` "
                "(there is no CPU fallback for the HIP path)" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        L.rr_last_error.restype = ctypes.c_char_p
        L.rr_abi_version.restype = c_int
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        raise RRNetHipError("%s failed (%d): %s" % (what, rc, lib().rr_last_error().decode()))


def ptr(t):
    """Device (or host) pointer of a tensor, None -> NULL."""
    if t is None:
        return c_void_p(0)
    return c_void_p(t.data_ptr())


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


_CTYPE = {"int": c_int, "float": c_float, "double": c_double, "size_t": c_size_t, "long": c_long,
          "hipStream_t": c_void_p, "void": None}
_SIGS = None


class Signature(tuple):
    """(restype, [argtypes]) of one entry point, plus `.pointees`: per parameter what a pointer points to ("float",
    "unsigned short", "void", "float *", ...), "hipStream_t" for the stream, None for a number."""
    pointees = ()


def _parse_header(fname):
    """Parses include/<fname> (shipped next to the library as rrnet_amd/<fname> when installed) -> {name: Signature}."""
    import re
    cands = [os.path.join(_HERE, fname), os.path.join(os.path.dirname(_HERE), "include", fname)]
    path = next(p for p in cands if os.path.exists(p))
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    sigs = {}
    for m in re.finditer(r"(?m)^\s*(const\s+char\s*\*|int\s|size_t\s|void\s|double\s)\s*(rr_\w+|_nms)\s*\(([^;{]*?)\)\s*;", text):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        restype = ctypes.c_char_p if "char" in ret else _CTYPE[ret.strip()]
        argtypes, pointees = [], []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "*" in a:
                    argtypes.append(c_void_p)
                    base = " ".join(re.sub(r"\b(const|__restrict__)\b", "", a[:a.index("*")]).split())
                    pointees.append(base + " *" * (a.count("*") - 1))
                else:
                    toks = a.replace("const", "").split()
                    argtypes.append(_CTYPE[toks[0]])
                    pointees.append("hipStream_t" if toks[0] == "hipStream_t" else None)
        sigs[name] = Signature((restype, argtypes))
        sigs[name].pointees = tuple(pointees)
    return sigs


def header_signatures():
    """Parses include/rrnet_hip.h (shipped next to the library as rrnet_amd/rrnet_hip.h when
    installed, otherwise <repo>/include) -> {name: Signature = (restype, [argtypes])}.  The header is the
    single source of truth for the ABI; pointers map to void* in argtypes, and the signature's `.pointees`
    keeps what each one points to."""
    global _SIGS
    if _SIGS is None:
        _SIGS = _parse_header(MAIN_HEADER)
    return _SIGS


MAIN_HEADER = "rrnet_hip.h"
# Companion headers: a kernel family with a header of its own beside rrnet_hip.h (same grammar, same library, same rules).
# header_signatures() stays the main header's table; a family's entries are reached through its Family object.
COMPANION_HEADERS = ("rrnet_hip_se.h", "rrnet_hip_attn.h", "rrnet_hip_dw.h", "rrnet_hip_rows.h", "rrnet_hip_wino.h")
_FAMILY_SIGS = {}


def family_signatures(header):
    """{name: Signature} of a companion header (parsed once)."""
    if header not in COMPANION_HEADERS:
        raise RRNetHipError("%s is not a header of this library (%s)" % (header, ", ".join((MAIN_HEADER,) + COMPANION_HEADERS)))
    if header not in _FAMILY_SIGS:
        _FAMILY_SIGS[header] = _parse_header(header)
    return _FAMILY_SIGS[header]


def declared(name):
    """-> (Signature, header that declares `name`), or (None, None)."""
    sig = header_signatures().get(name)
    if sig is not None:
        return sig, MAIN_HEADER
    for header in COMPANION_HEADERS:
        sig = family_signatures(header).get(name)
        if sig is not None:
            return sig, header
    return None, None


def fn(name, argtypes=None, restype=None):
    """Entry point `name` with the prototype declared in include/rrnet_hip.h (or a companion header)."""
    f = getattr(lib(), name, None)
    if f is None:
        raise RRNetHipError("librrnet_hip.so does not export %s (stale build?)" % name)
    if f.argtypes is None:
        sig, _ = declared(name)
        if sig is None:
            raise RRNetHipError("%s is not declared in include/%s" % (name, " or include/".join((MAIN_HEADER,) + COMPANION_HEADERS)))
        f.restype, f.argtypes = sig[0], sig[1]
    return f


_NO_CPU = "rrnet_amd ops run on the MI355X only: got a %s tensor (no CPU fallback)"


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RRNetHipError(_NO_CPU % t.device)


# What a tensor handed to a pointer parameter may hold, by the header's pointee: the dtypes the wrappers really pass, each of
# the pointee's element size.  None: anything (a workspace); (): no tensor at all (rr_sum_n's array of pointers).
POINTEE_DTYPES = {
    "float": (torch.float32,), "double": (torch.float64,), "void": None, "float *": (),
    "int": (torch.int32,), "unsigned": (torch.int32,),                    # (unsigned: the maxima's bit patterns)
    "unsigned short": (torch.bfloat16, torch.float16),                    # bf16 images, the fp16 parts of a split filter
    "unsigned char": (torch.uint8,), "signed char": (torch.int8,),
    "long": (torch.int64,), "long long": (torch.int64,), "unsigned long long": (torch.int64,),
}
_NUMBER = object()
_Tensor = torch.Tensor
_COUNTS = ("_blocks", "_supported", "_supported_dil")       # int-returning entries whose value is a count, not a status
_PLANS = {}


def _plan(name):
    """name -> (per caller argument the admitted dtypes | None | _NUMBER, stream appended?, host tensors allowed?,
    the return value is a status?), from the header, built once per entry."""
    sig, _ = declared(name)
    if sig is None:
        raise RRNetHipError("%s is not declared in include/%s" % (name, " or include/".join((MAIN_HEADER,) + COMPANION_HEADERS)))
    kinds = sig.pointees
    with_stream = bool(kinds) and kinds[-1] == "hipStream_t"
    slots = tuple(_NUMBER if k is None else POINTEE_DTYPES[k] for k in (kinds[:-1] if with_stream else kinds))
    plan = _PLANS[name] = (slots, with_stream, name.endswith("_host"),
                           sig[0] is c_int and not name.endswith(_COUNTS) and name != "rr_abi_version")
    return plan


def call(name, *args):
    """Calls entry point `name` of include/rrnet_hip.h: tensors go in as themselves and are checked against the header
    (a device tensor of a dtype the pointee admits, only in a pointer slot; None is NULL), the current stream is appended
    where the prototype ends in one, a failing status raises under the entry's own name.  Everything else (numbers,
    ctypes pointers) passes through.  The tensors are this frame's arguments: they outlive the enqueue."""
    slots, with_stream, host, status = _PLANS.get(name) or _plan(name)
    if len(args) != len(slots):
        raise RRNetHipError("%s takes %d arguments%s (include/rrnet_hip.h), got %d"
                            % (name, len(slots), " and the stream" if with_stream else "", len(args)))
    conv = list(args)
    for i, a in enumerate(args):
        kind = type(a)               # (numbers and None first: most arguments are, and the test is three pointer compares)
        if kind is not int and kind is not float and a is not None and isinstance(a, _Tensor):
            admits = slots[i]
            if admits is _NUMBER:
                raise RRNetHipError("%s: argument %d is a tensor, include/rrnet_hip.h declares a number" % (name, i))
            if not (a.is_cuda or host):
                raise RRNetHipError(_NO_CPU % a.device)
            if admits is not None and a.dtype not in admits:
                raise RRNetHipError("%s: argument %d is a %s tensor, include/rrnet_hip.h declares %s *"
                                    % (name, i, a.dtype, declared(name)[0].pointees[i]))
            conv[i] = c_void_p(a.data_ptr())
    if with_stream:
        conv.append(stream())                       # read now, never cached: the weight gradients run on side streams
    rc = fn(name)(*conv)
    if not status:
        return rc
    if rc != 0:
        raise RRNetHipError("%s failed (%d): %s" % (name, rc, lib().rr_last_error().decode()))


class Family:
    """The entry points of one companion header: `Family("rrnet_hip_se.h").call(name, ...)` is call() for a name that header
    declares, and an error for any other."""

    def __init__(self, header):
        self.header = header

    def signatures(self):
        return family_signatures(self.header)

    def call(self, name, *args):
        if name not in self.signatures():
            raise RRNetHipError("%s is not declared in include/%s" % (name, self.header))
        return call(name, *args)
