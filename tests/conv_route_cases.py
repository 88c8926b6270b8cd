"""The backward convolution dispatch pinned at the ABI (not a test: tests/test_conv_routes_gpu.py and tests/test_host_logic.py
import it).  cases() lists small conv_dgrad / conv_wgrad calls that cross every threshold of the dispatch in rrnet_amd/ops.py;
record(ops) runs them on the device and returns, per case, the ordered list of what reached the library:

    ["T", timer name, flops, detail, nbytes]     a launch handed to ops.TIMER (bench.py's roofline leg keys on the names)
    ["C", entry point, arg, arg, ...]            a call of an entry point of include/rrnet_hip.h; a pointer argument is
                                                 recorded as "NULL" or "PTR", every other argument by value

tests/golden/conv_bwd_routes.json is this record taken from the dispatch as it stood BEFORE ops.dgrad_route existed; the same
calls must keep producing the same launches.  Left out of the record are the two shape predicates rr_conv16_supported and
rr_conv16_wgrad_supported: they launch nothing, and how often the host asks them is not part of what a call computes.
Values are not compared here (the numerical suites do that): inputs are seeded randn."""
import contextlib

import torch

MODES = {"f32": 0, "bf16": 1, "f16x3": 2}
FLAGS = {"_CONV16": True, "_DGRAD_VIA_FPROP": True, "_DGRAD_BNSUM": True, "_HEAD_DGRAD": True, "_BF16_S2_DGRAD": True}
NOT_RECORDED = ("rr_conv16_supported", "rr_conv16_wgrad_supported")


def _dgrad(name, x, k, f, stride, pad, link=None, flags=None, b16=(), modes=MODES):
    """link: None | "bn" (recomputed mask) | "bn_z" (use_z, with z) | "relu_bias" | "mask_only";  b16: which of dy / y / z
    exist as a bf16 image only."""
    out = []
    for mode in modes:
        for acc in (False, True):
            out.append(dict(id="%s/%s%s" % (name, mode, "/acc" if acc else ""), op="dgrad", x=x, k=k, f=(f, f), stride=stride,
                            pad=(pad, pad), link=link, flags=dict(flags or {}), b16=sorted(b16), mode=mode, accumulate=acc))
    return out


def _wgrad(name, x, k, f, stride, pad, b16=(), modes=MODES, dy_hw=None):
    return [dict(id="%s/%s" % (name, mode), op="wgrad", x=x, k=k, f=(f, f), stride=stride, pad=(pad, pad), b16=sorted(b16),
                 mode=mode, flags={}, dy_hw=dy_hw) for mode in modes]


def cases():
    a, b, f, kx = (2, 128, 64, 64), (2, 128, 32, 32), (2, 128, 128, 128), (2, 256, 64, 64)
    bf = ("bf16",)
    out = []
    # A: every stride-1 route above the pixel thresholds
    out += _dgrad("A", a, 128, 3, 1, 1)
    out += _dgrad("A-bn", a, 128, 3, 1, 1, "bn")
    out += _dgrad("A-bn_z", a, 128, 3, 1, 1, "bn_z")
    out += _dgrad("A-conv16_off", a, 128, 3, 1, 1, flags={"_CONV16": False})
    out += _dgrad("A-bn-conv16_off", a, 128, 3, 1, 1, "bn", flags={"_CONV16": False})       # (the BN sums under bf16 operands)
    out += _dgrad("A-bn_z-conv16_off", a, 128, 3, 1, 1, "bn_z", flags={"_CONV16": False})
    out += _dgrad("A-bn-bnsum_off", a, 128, 3, 1, 1, "bn", flags={"_DGRAD_BNSUM": False})
    out += _dgrad("A-via_fprop_off", a, 128, 3, 1, 1, flags={"_DGRAD_VIA_FPROP": False})
    out += _dgrad("B", b, 128, 3, 1, 1)                       # below the conv16 and via-fprop pixel thresholds, at the f16x3 one
    out += _dgrad("C", (1, 128, 16, 16), 128, 3, 1, 1)        # below the f16x3 threshold
    out += _dgrad("D", (2, 6, 32, 32), 10, 3, 1, 1)           # scalar channels
    out += _dgrad("E", a, 128, 1, 1, 1)                       # pad not below the filter
    out += _dgrad("F", f, 128, 3, 2, 1)
    out += _dgrad("F-conv16_off", f, 128, 3, 2, 1, flags={"_CONV16": False})
    out += _dgrad("F-s2_off", f, 128, 3, 2, 1, flags={"_BF16_S2_DGRAD": False})
    out += _dgrad("G", b, 128, 3, 2, 1)
    out += _dgrad("H", (2, 64, 128, 128), 128, 3, 2, 1)       # C not a multiple of 128
    out += _dgrad("I", a, 128, 3, 2, 2)                       # parity pads fail
    out += _dgrad("J", f, 256, 1, 2, 0)
    # K: producers of the form conv + bias + ReLU, and bare ReLUs
    for link in ("relu_bias", "mask_only"):
        out += _dgrad("K-%s-k10" % link, kx, 10, 1, 1, 0, link)
        out += _dgrad("K-%s-k10-head_off" % link, kx, 10, 1, 1, 0, link, flags={"_HEAD_DGRAD": False})
        out += _dgrad("K-%s-k34" % link, kx, 34, 1, 1, 0, link)
        out += _dgrad("K-%s-k128" % link, kx, 128, 3, 1, 1, link)
    out += _dgrad("K-relu_bias-small_map", (2, 256, 32, 32), 128, 3, 1, 1, "relu_bias")       # link ignored
    out += _dgrad("K-relu_bias-ragged", (1, 256, 72, 72), 128, 3, 1, 1, "relu_bias")          # n*h*w % 128 != 0: link ignored
    # L: bf16-only operands
    out += _dgrad("L-A-dy16", a, 128, 3, 1, 1, b16=("dy",), modes=bf)
    out += _dgrad("L-B-dy16", b, 128, 3, 1, 1, b16=("dy",), modes=bf)
    out += _dgrad("L-F-dy16", f, 128, 3, 2, 1, b16=("dy",), modes=bf)
    out += _dgrad("L-K-mask_only-dy16", kx, 128, 3, 1, 1, "mask_only", b16=("dy",), modes=bf)
    out += _dgrad("L-A-bn-y16", a, 128, 3, 1, 1, "bn", b16=("y",), modes=bf)
    out += _dgrad("L-A-bn_z-z16", a, 128, 3, 1, 1, "bn_z", b16=("z",), modes=bf)
    out += _dgrad("L-K-relu_bias-z16", kx, 128, 3, 1, 1, "relu_bias", b16=("z",), modes=bf)
    # M: weight gradients
    out += _wgrad("M-A", a, 128, 3, 1, 1)
    out += _wgrad("M-B", b, 128, 3, 1, 1)
    out += _wgrad("M-F", f, 128, 3, 2, 1)
    out += _wgrad("M-k28", a, 28, 3, 1, 1)
    out += _wgrad("M-k10", a, 10, 1, 1, 0)
    out += _wgrad("M-explicit_out", (2, 12, 16, 16), 32, 4, 1, 2, dy_hw=(16, 16))
    out += _wgrad("M-A-16", a, 128, 3, 1, 1, b16=("x", "dy"), modes=bf)
    return out


def dy_shape(case):
    n, _, h, w = case["x"]
    (r, s), st, (ph, pw) = case["f"], case["stride"], case["pad"]
    p, q = case.get("dy_hw") or ((h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1)
    return (n, case["k"], p, q)


@contextlib.contextmanager
def configured(ops, case):
    """The module flags and the thread's arithmetic as the case wants them; put back on the way out."""
    saved = {name: getattr(ops, name) for name in FLAGS}
    try:
        for name, default in FLAGS.items():
            setattr(ops, name, case["flags"].get(name, default))
        with ops.bf16_scope(MODES[case["mode"]], force=True):
            yield
    finally:
        for name, value in saved.items():
            setattr(ops, name, value)


def _plain(v):
    """A ctypes / Python argument -> something JSON holds: pointers as NULL / PTR, numbers by value."""
    import ctypes
    if v is None:
        return "NULL"
    if isinstance(v, ctypes.c_void_p):
        return "PTR" if v.value else "NULL"
    if isinstance(v, (tuple, list)):
        return [_plain(e) for e in v]
    if isinstance(v, (bool, int, float, str)):
        return v
    return _plain(v.value)                                  # c_int, c_float, ...


def _run(ops, case, dev):
    g = torch.Generator(device=dev).manual_seed(219)

    def fp32(shape):
        return ops.to_nhwc(torch.randn(shape, device=dev, generator=g))

    def operand(shape, what):
        t = fp32(shape)
        return ops.phantom_f32(shape, dev, t.to(torch.bfloat16)) if what in case["b16"] else t

    n, c, h, w = case["x"]
    k, (r, s) = case["k"], case["f"]
    dy = operand(dy_shape(case), "dy")
    if case["op"] == "wgrad":
        x, dw = operand(case["x"], "x"), ops.zeros_nhwc(k, c, r, s, dev)
        return lambda: ops.conv_wgrad(x, dy, dw, case["stride"], case["pad"], explicit_out=bool(case["dy_hw"]))
    wt = ops.to_nhwc(torch.randn((k, c, r, s), device=dev, generator=g) * 0.05)
    link, z = None, None
    if case["link"] in ("bn", "bn_z"):
        link = ops.BnLink()
        link.y, link.mean, link.invstd = operand(case["x"], "y"), torch.randn(c, device=dev, generator=g), torch.rand(c, device=dev, generator=g) + 0.5
        link.use_z = case["link"] == "bn_z"
        if not link.use_z:
            link.msc, link.msh = torch.randn(c, device=dev, generator=g), torch.randn(c, device=dev, generator=g)
        z = operand(case["x"], "z")            # (a node hands its saved input on whatever the link says)
    elif case["link"] is not None:
        link = ops.BnLink()
        link.relu_bias = link.use_z = True
        link.mask_only = case["link"] == "mask_only"
        z = operand(case["x"], "z")
    out = fp32(case["x"]) if case["accumulate"] else None
    return lambda: ops.conv_dgrad(dy, wt, case["x"], case["stride"], case["pad"], out=out, accumulate=case["accumulate"], bnsum=link, bnsum_z=z)


def record(ops):
    """-> {case id: [entries]} (see the module's docstring); the module flags, the timer and ops._C.fn are put back."""
    dev = torch.device("cuda", torch.cuda.current_device())
    log = []

    class Timer:
        def launch(self, name, flops, fn, detail=None, nbytes=0.0):
            log.append(["T", name, flops, _plain(detail), nbytes])
            return fn()

    real_fn = ops._C.fn

    def fn(name, *a, **kw):
        f = real_fn(name, *a, **kw)
        if name in NOT_RECORDED:
            return f

        def call(*args):
            log.append(["C", name] + [_plain(v) for v in args])
            return f(*args)
        return call

    saved_timer = ops.TIMER
    out = {}
    try:
        ops.TIMER, ops._C.fn = Timer(), fn
        for case in cases():
            with configured(ops, case):
                call = _run(ops, case, dev)        # (the operands are made outside the record)
                del log[:]
                call()
            out[case["id"]] = list(log)
        torch.cuda.synchronize()
    finally:
        ops.TIMER, ops._C.fn = saved_timer, real_fn
    return out


if __name__ == "__main__":          # python tests/conv_route_cases.py OUT.json: writes the record of the rrnet_amd that is importable
    import json
    import sys
    from rrnet_amd import ops as _ops
    rec = record(_ops)
    with open(sys.argv[1], "w") as fh:
        fh.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, separators=(",", ":"))) for k, v in rec.items()) + "\n}\n")
    print("%d cases recorded" % len(rec))
