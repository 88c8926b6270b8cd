"""Thin, autograd-free wrappers over the C ABI (include/rrnet_hip.h).  Tensors are torch CUDA
tensors used purely as device-memory handles: logical shape NCHW with channels_last strides,
i.e. NHWC in memory; conv weights logical [K,C,R,S] with channels_last strides = OHWI."""
import os
import sys
import threading
import types
import weakref

import torch

from rrnet_amd import _C

CL = torch.channels_last


class KernelTimer:
    """Optional live timing of individual conv launches with HIP events recorded on the launch
    stream (bench.py's roofline leg).  Off (None) in normal operation: no events, no overhead."""

    def __init__(self, only=None, every=1):
        self.records = []      # (kernel name, flops, start event, end event)
        self.bytes = {}        # kernel name -> algorithmic bytes (operands read once + result written once)
        self.only = only       # optional set of kernel names: the others run without events (each pair costs ~10 us)
        # time every `every`-th launch of a kernel name: an event pair is two tiny blit kernels on the stream (rocprofv3
        # shows them as __amd_rocclr_copyBuffer, 346 per step = 1.45 ms when every launch of the dominant kernel is
        # timed); a 1-in-4 systematic sample over the timed region (173 launches per step: the phase shifts every step)
        # keeps the average and costs a quarter
        self.every = max(int(every), 1)
        self.seen = {}

    def launch(self, name, flops, fn, detail=None, nbytes=0.0):
        if self.only is not None and name not in self.only:
            return fn()
        k = self.seen.get(name, 0)
        self.seen[name] = k + 1
        if k % self.every:
            return fn()
        self.bytes[name] = self.bytes.get(name, 0.0) + nbytes
        s = torch.cuda.Event(enable_timing=True)
        e = torch.cuda.Event(enable_timing=True)
        s.record()
        rc = fn()
        e.record()
        self.records.append((name, flops, s, e, detail))
        return rc

    def by_shape(self):
        torch.cuda.synchronize()
        out = {}
        for name, flops, s, e, detail in self.records:
            d = out.setdefault((name, detail), dict(launches=0, ms=0.0, flops=0.0))
            d["launches"] += 1
            d["ms"] += s.elapsed_time(e)
            d["flops"] += flops
        return out

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for name, flops, s, e, _ in self.records:
            d = out.setdefault(name, dict(launches=0, ms=0.0, flops=0.0))
            d["launches"] += 1
            d["ms"] += s.elapsed_time(e)
            d["flops"] += flops
        return out


AUX_STREAMS = {}       # (device type, index) -> auxiliary HIP streams that may hold kernels writing gradient buffers


def join_aux_streams(device):
    """The current stream waits for everything enqueued on the auxiliary streams (weight gradients on their side
    stream): called before a collective is launched on, or a consumer reads, the flat gradient buffer."""
    if device.type != "cuda":
        return
    cur = torch.cuda.current_stream(device)
    for st in AUX_STREAMS.get((device.type, device.index), ()):
        if st != cur:
            cur.wait_stream(st)


TIMER = None
SYNC_WAIT_S = 0.0      # host time spent blocked in the RoI-count read (bench.py separates it from the enqueue time)


def _launch(key, flops, entry, args, detail=None, nbytes=0.0, call=_C.call):
    """Entry point `entry` on `args` (_C.call, or a companion header's Family.call), under the timer key `key` when a timer is
    on: it is reached inside the timer's fn()."""
    if TIMER is None:
        return call(entry, *args)
    return TIMER.launch(key, flops, lambda: call(entry, *args), detail, nbytes)


_SMALL_TILES = 16
_MID_TILES = 48


def _igemm_name(kind, n_gemm, scalar, m_rows=1 << 30, stride=1):
    """Timer key = the HIP kernel instance that runs (tile width as picked in csrc/conv.hip: 128 columns, 64 for
    33..64-column layers, 32 for narrow ones and for layers with at most rr_conv_small_tiles() 128x128 tiles)."""
    bn = 128 if n_gemm > 64 or (scalar and n_gemm > 32) else (64 if n_gemm > 32 else 32)
    if bn == 128 and not scalar and (kind == "fprop" or stride == 1):
        tiles = -(-m_rows // 128) * -(-n_gemm // 128)
        if tiles <= _SMALL_TILES:
            bn = 32
        elif tiles <= _MID_TILES:
            bn = 64
    return "conv_%s<BN=%d,%s>" % (kind, bn, "scalar" if scalar else "vec4")


def is_nhwc(t):
    return t.dim() == 4 and t.permute(0, 2, 3, 1).is_contiguous()


def is_phantom(t):
    """A bf16-only activation / gradient (phantom_f32): an fp32 tensor OBJECT without memory whose values live in its bf16 image.
    Recognised by IDENTITY: every such handle is a zero-stride view of the one per-device NaN stub (_PHANTOM_STUB), so the test is
    "does t view that storage" — views and tensors unpacked from an autograd node keep it, nothing else can have it (round 5 went
    by a signature: strides 0, offset 1, an 8-byte storage).  A view that lost the image link (the Python attribute) fails loudly
    in image_of(); a torch-native read of the handle returns NaN."""
    if t is None or t.dim() != 4 or t.stride() != (0, 0, 0, 0):
        return False
    stub = _PHANTOM_STUB.get(t.device)
    return stub is not None and t.untyped_storage().data_ptr() == stub.untyped_storage().data_ptr()


def image_of(t):
    img = b16_side.carry(t)
    if img is None:
        raise RuntimeError("a bf16-only tensor of shape %s reached a consumer without its bf16 image (a view / saved tensor whose "
                           "producer did not hand the image on: ops.side_carry / side_restore)" % (tuple(t.shape),))
    return img


def f32_of(t):
    """The fp32 tensor a consumer without a bf16 form needs: t itself, or — for a bf16-only tensor — its image widened into a FRESH
    tensor of the caller's (allocated on the current stream, never remembered on t: a copy cached on the tensor object in the forward
    outlived it until the backward, where the weight-gradient side stream read it while the main stream's allocator had already
    reused the block — found by the stress arm of tests/test_streams_gpu.py)."""
    if not is_phantom(t):
        return t
    img = image_of(t)
    out = torch.empty_like(img, dtype=torch.float32)
    assert out.stride() == img.stride()
    _C.call("rr_from_bf16", img, out, img.numel())
    return out


def to_nhwc(t, keep_phantom=False):
    """Returns a tensor with the same logical NCHW shape whose memory is NHWC.  A bf16-only tensor is handed through only to
    callers that say they can read its image (keep_phantom); everybody else receives the widened fp32 copy."""
    if is_phantom(t):
        return t if keep_phantom else f32_of(t)
    if is_nhwc(t):
        return t
    return t.contiguous(memory_format=CL)


def empty_nhwc(n, c, h, w, device, dtype=torch.float32):
    return torch.empty((n, h, w, c), device=device, dtype=dtype).permute(0, 3, 1, 2)


def zeros_nhwc(n, c, h, w, device, dtype=torch.float32):
    return torch.zeros((n, h, w, c), device=device, dtype=dtype).permute(0, 3, 1, 2)


def out_hw(h, w, r, s, stride, ph, pw):
    return (h + 2 * ph - r) // stride + 1, (w + 2 * pw - s) // stride + 1


# bf16 matrix operands for the convolutions (BASELINE config 4; csrc/conv_bf16.hip).  A process-wide switch set by the
# model (cfg.Model.bf16 -> rrnet_amd.models.rrnet) for the duration of its forward / backward: same tensors (fp32 in
# HBM), same autograd graph, only the kernels the launches go to differ.  The headline configuration never sets it.
#
# The switch has three positions (cfg.Model.conv_math, math_mode()):
#   0 / False  "f32"    v_mfma_f32_32x32x2_f32 (csrc/conv.hip) — the reference's arithmetic
#   1 / True   "bf16"   operands rounded to bf16 (config 4)
#   2          "f16x3"  operands split into two fp16 parts, three products: fp32-level accuracy at the 16-bit matrix rate
MATH_F32, MATH_BF16, MATH_F16X3 = 0, 1, 2
_MATH_NAMES = {"f32": MATH_F32, "fp32": MATH_F32, "bf16": MATH_BF16, "f16x3": MATH_F16X3}


def _env_mode():
    name = os.environ.get("RR_CONV_MATH", "f32")
    if name not in _MATH_NAMES:
        raise ValueError("RR_CONV_MATH must be one of %s, got %r" % (sorted(_MATH_NAMES), name))
    return _MATH_NAMES[name]


_BF16_ENV = _env_mode()


# The switch is per THREAD (two models of different conv_math driven from two threads, or a backward on an autograd worker
# while another thread runs a forward, must not see each other's setting); a thread that never set it reads the
# environment's default.  `ops.BF16` stays readable / assignable as a module attribute (the module class below).
class _Mode(threading.local):
    def __init__(self):
        self.value = _BF16_ENV


_MODE = _Mode()


def _mode():
    return _MODE.value


def math_mode(model_cfg):
    """cfg.Model -> the switch position: conv_math ("f32" | "bf16" | "f16x3") if present, else the older bf16 flag."""
    name = getattr(model_cfg, "conv_math", None)
    if name:
        if name not in _MATH_NAMES:
            raise ValueError("cfg.Model.conv_math must be one of %s, got %r" % (sorted(_MATH_NAMES), name))
        return _MATH_NAMES[name]
    return MATH_BF16 if getattr(model_cfg, "bf16", False) else MATH_F32


class bf16_scope:
    """`with ops.bf16_scope(mode):` — the convolutions launched inside (by this thread) take the fp32 (0 / None: the
    environment's default, RR_CONV_MATH), bf16-operand (1 / True) or split-operand (2) kernels; `force=True` takes `mode`
    literally, so that 0 means the fp32 kernels whatever the environment says.  RRNet.forward opens it for a model built
    with cfg.Model.bf16 / conv_math; every convolution node remembers the setting of its forward and re-opens it around
    its backward (rrnet_amd/functional.py)."""

    def __init__(self, on, force=False):
        self.on = int(on or 0) if force else (int(on or 0) or _BF16_ENV)

    def __enter__(self):
        self.prev, _MODE.value = _MODE.value, self.on

    def __exit__(self, *exc):
        _MODE.value = self.prev


def _bf16_ok(c, k, r, s, *tensors, pixels=None):
    """Shapes csrc/conv_bf16.hip takes: vector path (C and K multiples of 4, <= 64 taps), tensors below 2 GiB.
    -> 0 (fp32 kernels) or the switch position (MATH_BF16 / MATH_F16X3)."""
    ok = _mode() and c % 4 == 0 and k % 4 == 0 and r * s <= 64 and all(t.numel() * 4 < (1 << 31) for t in tensors)
    if ok and _mode() == MATH_F16X3:
        # the split kernels pay two small reductions (the operands' maxima) per launch and three matrix instructions per tile:
        # they beat the fp32-MFMA kernels on the large 3x3 layers only; the rest stays on csrc/conv.hip — same accuracy class
        if pixels is None or pixels < _SPLIT_MIN_PIXELS or c * r * s < _SPLIT_MIN_K or k < _SPLIT_MIN_CH or c < _SPLIT_MIN_CH:
            return 0
    return int(_mode()) if ok else 0


_SPLIT_MIN_PIXELS = 2048    # N*P*Q below which a layer stays on the fp32 kernels
_SPLIT_PRESPLIT_PIXELS = 65536   # from here on the filter is split once per launch


def split_filter(w, amax_word, pixels, flat=None):
    """The two fp16 images of a filter for the f16x3 kernels (rr_weight_split_f16: hi, then lo; scaled by the power of two
    the kernels derive from `amax_word`), or None below the layer size where a ready-made split pays.  w: the OHWI filter
    (forward) — or, with `flat`, the flat flipped / transposed copy of it (data gradients), whose K and C trade places."""
    k, c = (w.shape[0], w.shape[1])
    if pixels < _SPLIT_PRESPLIT_PIXELS or c % 8 != 0 or k % 8 != 0 or min(k, c) <= 64:
        return None
    src = w if flat is None else flat
    out = torch.empty(2 * src.numel(), dtype=torch.float16, device=src.device)
    _C.call("rr_weight_split_f16", src, src.numel(), amax_word, out)
    return out


_SPLIT_MIN_CH = 64                                                         # narrower layers (either side) likewise
_SPLIT_MIN_K = 1024               # C*R*S (reduction length) likewise


_AMAX_CHECK = os.environ.get("RR_AMAX_CHECK", "0") == "1"     # recompute every remembered maximum when it is used; raise on mismatch
_CONV16 = os.environ.get("RR_CONV16", "1") != "0"               # 0: the round-4 kernels (fp32 tensors, converted inside every launch)
_CONV16_MIN_PIXELS = 8192     # output pixels below which the 256-pixel tiles lose to the round-4 kernels (8 x 32 x 32 x 384: 351 vs 229 TFLOP/s; 16 x 16: 24 workgroups)


# ---- sidecars: derived values that ride on tensor OBJECTS ------------------------------------------------------------------
# Two kinds.  The maximum: the device word holding the bit pattern of max|t| that the f16x3 kernels scale their operands by
# (amax_of).  The image: the bf16 copy of an fp32 tensor that csrc/conv16.hip reads both operands of a convolution as — under
# cfg.Model.bf16 the producers of a convolution's operands (bn_apply, bn_bwd_apply) write it next to the fp32 tensor in the
# same pass, an operand without one (a fan-in sum, the up-sample add, a head's masked gradient) is converted on first use
# (bf16_of); for a bf16-only activation (phantom_f32) it is the only data there is.
# One rule for both, and this section is the only code that knows how it is stored (a Python attribute holding
# `(version | None, stream id | None, payload)`): the payload is valid for this version of the tensor (None: whatever the
# version — a phantom handle, below), on the stream that made it (None: on every stream — published, restored, or not on the
# GPU), and a kernel that writes the tensor through its raw pointer drops it.
class _Sidecar:
    def __init__(self, attr):
        self.attr = attr

    def _hit(self, t):
        """The stored triple if it is valid for t's version, else None."""
        hit = getattr(t, self.attr, None) if t is not None else None
        return hit if (hit is not None and (hit[0] is None or hit[0] == t._version)) else None

    def attach(self, t, payload, versioned=True):
        """payload was made on the current stream.  versioned=False: a phantom handle — every such handle is a view of one stub
        and shares its version counter, while its image is its value, written once and never updated in place: a version
        test there protects nothing and could only lose data."""
        setattr(t, self.attr, (t._version if versioned else None, torch.cuda.current_stream(t.device).cuda_stream if t.is_cuda else None, payload))

    def now(self, t):
        """For use by a kernel launched now: valid for this version and on the current stream (or None)."""
        hit = self._hit(t)
        if hit is None or (hit[1] is not None and hit[1] != torch.cuda.current_stream(t.device).cuda_stream):
            return None
        return hit[2]

    def carry(self, t):
        """Valid for this version, on whatever stream (or None) — for an autograd node to keep next to a tensor it saves: saved
        tensors come back as new Python objects, restore() hands the payload to the unpacked one."""
        hit = self._hit(t)
        return hit[2] if hit is not None else None

    def restore(self, t, payload, versioned=True):
        """Backward: a payload made in the forward (complete long before: valid on every stream) onto the fresh object."""
        if payload is not None and t is not None:
            setattr(t, self.attr, (t._version if versioned else None, None, payload))

    def publish(self, t):
        """The caller has just ordered another stream behind the current one (wait_stream): a payload made on the current stream
        may be read there."""
        hit = getattr(t, self.attr, None) if t is not None else None
        if hit is not None and hit[1] is not None and hit[1] == torch.cuda.current_stream(t.device).cuda_stream:
            setattr(t, self.attr, (hit[0], None, hit[2]))

    def share(self, t, views):
        """views ARE t (view_as): what rides on t, as valid as it is there, travels with them."""
        hit = self._hit(t)
        if hit is not None:
            for o in views:
                setattr(o, self.attr, (None if hit[0] is None else o._version, hit[1], hit[2]))

    def drop(self, t):
        if t is not None and getattr(t, self.attr, None) is not None:
            setattr(t, self.attr, None)


amax_side, b16_side = _Sidecar("_rr_amax"), _Sidecar("_rr_b16")
amax_carry, b16_carry = amax_side.carry, b16_side.carry
# (rows, count) of active_rows(): the pixels where a gradient tensor may be non-zero, made next to it by the launch that wrote it
rows_side = _Sidecar("_rr_rows")


def amax_drop(t):
    """`t` is about to be (or has just been) written through its raw pointer by a kernel — an accumulate-form data gradient,
    bn_bwd_apply's g_into, any `out=` argument: such writes never move `t._version`, so a maximum remembered on the tensor
    object would look valid and be stale (too low: the fp16 parts overflow; too high: bits are dropped silently)."""
    amax_side.drop(t)
    b16_side.drop(t)                           # (the bf16 image is as stale as the maximum)


def side_carry(x, *image_only):
    """What an autograd node keeps next to the tensors it saves: both kinds of x, the images of the rest (None entries allowed)."""
    return (amax_side._hit(x),) + tuple(b16_side._hit(t) for t in (x,) + image_only)


def side_restore(carried, x, *image_only):
    """side_carry's result onto the unpacked tensors, in the same order (a phantom's image stays free of the version)."""
    if carried is not None:
        for side, t, hit in zip((amax_side, b16_side) + (b16_side,) * len(image_only), (x, x) + image_only, carried):
            if hit is not None:
                side.restore(t, hit[2], versioned=hit[0] is not None)


def side_publish(t):
    amax_side.publish(t)
    b16_side.publish(t)
    rows_side.publish(t)


def image_wanted(c, pixels, device, multiple=128):
    """Does the producer of a c-channel tensor of this many pixels write its bf16 image in the same pass (its consumer is a conv16
    kernel)?  Read at call time: the thread's arithmetic and the module switches."""
    return bool(_CONV16 and _mode() == MATH_BF16 and device.type == "cuda" and c % multiple == 0 and pixels >= _CONV16_MIN_PIXELS)


def amax_wanted(c, pixels, device):
    """Does the producer publish max|t| out of the same pass (split-operand convolutions: the consumer's operand scale, see amax_of)?"""
    return bool(_mode() == MATH_F16X3 and device.type == "cuda" and pixels >= _SPLIT_MIN_PIXELS)


class _PhantomScope(threading.local):
    def __init__(self):
        self.on = False


_PHANTOM = _PhantomScope()
_PHANTOM_ENABLED = os.environ.get("RR_BF16_ONLY_ACT", "1") != "0"      # 0: every activation keeps its fp32 tensor next to the image


class phantom_scope:
    """Inside (HourglassNet.forward under cfg.Model.bf16): conv -> bn [-> +res] -> relu layers and the up-path add may return
    bf16-ONLY activations (phantom_f32) where the shape qualifies — everything that consumes them there reads the image.  Tensors
    that leave the backbone are produced outside the scope and are ordinary fp32 tensors."""

    def __init__(self, on=True):
        self.on = bool(on)

    def __enter__(self):
        self.prev, _PHANTOM.on = _PHANTOM.on, self.on

    def __exit__(self, *exc):
        _PHANTOM.on = self.prev


def phantom_out_ok(c, pixels, device):
    # (no grad-mode test: inside an autograd Function's forward grad mode is always off)
    return bool(_PHANTOM.on and _PHANTOM_ENABLED and image_wanted(c, pixels, device, 256))


def phantom_y_ok(k, x, w, stride, pad):
    """conv -> bn layers inside the backbone (phantom_scope): may the convolution's pre-BN output exist as a bf16 image only?"""
    if not x.is_cuda:
        return False
    n, c, h, wd = x.shape
    r, s = w.shape[2], w.shape[3]
    p, q = out_hw(h, wd, r, s, stride, pad[0], pad[1])
    return phantom_out_ok(k, n * p * q, x.device) and conv16_ok(c, k, r, s, stride, n * p * q, x)


def bf16_of(t):
    """bf16 image of the fp32 NHWC tensor t (same logical shape, same memory order), converted on the current stream and
    remembered on the tensor object when none rides on it."""
    if is_phantom(t):
        return image_of(t)
    img = b16_side.now(t)
    if img is not None:
        return img
    assert t.numel() % 4 == 0
    img = torch.empty_like(t, dtype=torch.bfloat16)
    assert img.stride() == t.stride()
    _C.call("rr_to_bf16", t, img, t.numel())
    try:
        b16_side.attach(t, img)
    except AttributeError:
        pass
    return img


_PHANTOM_STUB = {}       # device -> the two-NaN storage every handle on that device is a view of


def phantom_f32(shape, device, image):
    """An fp32 tensor OBJECT of the given logical shape that owns no memory (one element, stride 0) and carries `image` as its
    bf16 image: the handle of a gradient that exists only in bf16 — every consumer is a conv16 kernel.  A kernel wrapper that
    would read its fp32 data trips over `is_nhwc` (stride 0); a torch-native consumer (a hook, `+`, `.sum()`, a print) reads
    NaN — the stub's one element — so an accidental read poisons the loss loudly instead of training on one garbage value."""
    device = torch.device(device)
    stub = _PHANTOM_STUB.get(device)
    if stub is None:
        stub = _PHANTOM_STUB[device] = torch.full((2,), float("nan"), dtype=torch.float32, device=device)
    # (a 0-dim view of element 1 of 2: expanding the 1-element slice stub[1:] kept stride 1 on a last dimension of size 1, so a
    # handle of width 1 failed is_phantom's all-zero-strides test and its consumer read the stub as if it were the data)
    t = stub[1].expand(shape)
    b16_side.attach(t, image, versioned=False)
    return t


def wgrad_16bit_shape(c, k, r, s):
    """Layer shapes whose weight gradient leaves the fp32 kernel when a 16-bit arithmetic is on (conv_wgrad and the kernel audit ask).  Narrow filter
    banks stay on its 32-filter tiles — except 3x3 banks of 16..32 filters, the DCN offset / mask convolution's 28: 1.20 ms fp32 against 0.54 ms bf16."""
    return c > 32 and (k > 32 or (k >= 16 and r * s >= 9))


def wgrad16_takes(x_shape, dy_shape, w_shape, stride):
    """True when conv_wgrad(x, dy, dw, stride, ...) goes to rr_conv16_wgrad (the explicit_out form never does)."""
    k, c, r, s = w_shape
    npix, xn = dy_shape[0] * dy_shape[2] * dy_shape[3], x_shape[0] * x_shape[1] * x_shape[2] * x_shape[3]
    return bool(_CONV16 and _mode() == MATH_BF16 and npix >= _CONV16_MIN_PIXELS and _C.call("rr_conv16_wgrad_supported", c, k, r, s, stride)
                and max(xn, npix * k) * 2 < (1 << 31))


def conv16_ok(c, k, r, s, stride, pixels, *tensors):
    """-> True when a forward-kernel launch of this shape goes to csrc/conv16.hip (bf16 mode only)."""
    return bool(_CONV16 and _mode() == MATH_BF16 and pixels >= _CONV16_MIN_PIXELS and all(t is None or t.is_cuda for t in tensors)
                and _C.call("rr_conv16_supported", c, k, r, s, stride) and all(t is None or t.numel() * 2 < (1 << 31) for t in tensors))


def _amax_word(device):
    """A zeroed device word for a maximum's bit pattern: 8 zeroed bytes as int32 [2]; the kernels read and write the first."""
    return _ZEROS.take(1, device).view(torch.int32)


def _absmax_word(t):
    word = _amax_word(t.device)
    n = t.numel()
    assert n % 4 == 0
    _C.call("rr_absmax_bits", t, n, word)
    return word


def amax_of(t):
    """Device word holding the bit pattern of max|t| (rr_absmax_bits) for the split-operand kernels, computed on the
    current stream and remembered on the tensor object (same version, same stream): a gradient serves its data
    gradient and its weight gradient with one reduction.  RR_AMAX_CHECK=1 (tests): every remembered word is checked
    against a fresh reduction at the moment it is used."""
    word = amax_side.now(t)
    if word is not None:
        if _AMAX_CHECK:
            fresh = int(_absmax_word(t)[0].item())
            kept = int(word.view(torch.int32)[0].item())
            if fresh != kept:
                raise RuntimeError("ops.amax_of: stale remembered maximum on a tensor of shape %s: remembered bits 0x%08x, "
                                   "actual 0x%08x (a kernel wrote it through its raw pointer without ops.amax_drop)"
                                   % (tuple(t.shape), kept & 0xffffffff, fresh & 0xffffffff))
            AMAX_CHECKED[0] += 1
        return word
    word = _absmax_word(t)
    try:
        amax_side.attach(t, word)
    except AttributeError:
        pass
    return word


AMAX_CHECKED = [0]       # remembered maxima verified under RR_AMAX_CHECK=1 (the audit asserts that the check really ran)


def _math_call(mode, a, b, filter16=None, filter_split=None, takes_filter=False):
    """-> (entry-point suffix, timer tag, trailing arguments) of a convolution entry point under arithmetic `mode`: fp32 ("", "", ()),
    bf16 ("_bf16", "+bf16", ()), f16x3 ("_f16x3", "+f16x3", the maxima of the operands a and b).  takes_filter (rr_conv_fprop*,
    rr_conv_dgrad_s1{,_bnsum}*; not _relubias, _s2, wgrad): behind them the filter's cached bf16 copy / fp16 split, or None (NULL)."""
    sfx = ("", "_bf16", "_f16x3")[mode]
    tail = (amax_of(a), amax_of(b)) if mode == MATH_F16X3 else ()
    if takes_filter and mode != MATH_F32:
        tail += (filter_split if mode == MATH_F16X3 else filter16,)
    return sfx, sfx.replace("_", "+"), tail


def conv_fprop(x, w, bias=None, stride=1, pad=(0, 0), relu=False, want_stats=False, algo_kg=None, w16=None, w_split=None,
               y_bf16_only=False):
    """x [N,C,H,W] (NHWC memory), w [K,C,R,S] (OHWI memory) -> y [N,K,P,Q] (NHWC memory)
    and, if want_stats, the per-block BatchNorm partial-sum slab (see rr_conv_fprop).
    algo_kg: the useful reduction length when the operands carry zero padding (timer FLOPs stay algorithmic)."""
    _C.require_cuda(x, w, bias)
    n, c, h, wd = x.shape
    k, c2, r, s = w.shape
    assert c == c2
    p, q = out_hw(h, wd, r, s, stride, pad[0], pad[1])
    use16 = conv16_ok(c, k, r, s, stride, n * p * q, x) and n * p * q * k * 4 < (1 << 31)
    y16 = None
    if use16 and y_bf16_only:
        # the output as a bf16 image only (the caller's BatchNorm reads it; the statistics below come from the fp32 accumulators)
        y16 = torch.empty((n, p, q, k), dtype=torch.bfloat16, device=x.device).permute(0, 3, 1, 2)
        y = phantom_f32((n, k, p, q), x.device, y16)
    else:
        y = empty_nhwc(n, k, p, q, x.device)
    slab = None
    if is_phantom(x) and not use16:
        x = f32_of(x)                       # a bf16-only input in front of a layer the conv16 kernels do not take
    assert (is_nhwc(x) or is_phantom(x)) and is_nhwc(w), "conv_fprop wants NHWC activations / OHWI weights"
    if use16:
        # both operands as bf16 tensors (csrc/conv16.hip): x's image from its producer (or converted once), the filter's from
        # the flat cache
        x16 = bf16_of(x)
        if w16 is None:
            w16 = bf16_of(w)
        if want_stats:
            slab = torch.empty(_C.call("rr_conv16_stat_slab_bytes", n, p, q, k) // 8, dtype=torch.float64, device=x.device)
        flops = 2.0 * n * p * q * k * (c * r * s if algo_kg is None else algo_kg)
        _launch("conv16_fprop", flops, "rr_conv16_fprop",
                (x16, w16, bias, None if y16 is not None else y, y16, slab, n, h, wd, c, k, r, s, stride, pad[0], pad[1], int(relu)),
                (n, h, wd, c, k, r, s, stride), 2.0 * (x.numel() + w.numel()) + (2.0 if y16 is not None else 4.0) * y.numel())
        return (y, slab) if want_stats else y
    if want_stats:
        nbytes = _C.call("rr_conv_stat_slab_bytes", n, p, q, k)
        slab = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    bf = _bf16_ok(c, 4 if _mode() != MATH_F16X3 else k, r, s, x, w, y, pixels=n * p * q)
    flops = 2.0 * n * p * q * k * (c * r * s if algo_kg is None else algo_kg)
    if bf == MATH_F32 and wino_takes(n, h, wd, c, k, r, s, stride, pad, bias is not None, relu, want_stats):
        # the Winograd route (csrc/conv_wino.hip); its timer key carries the multiplications it executes, 16 of the direct 36
        u, ws = _wino_filter(w, False), _wino_ws(x.device, n, h, wd, c, k)
        _launch("conv_fprop<wino>", flops * 16.0 / 36.0, "rr_conv_wino_fprop",
                (x, u, bias, y, slab, ws, ws.numel() * 4, n, h, wd, c, k, int(relu), 0), (n, h, wd, c, k, r, s, stride),
                4.0 * (x.numel() + y.numel() + w.numel()) + 2.0 * ws.numel() * 4.0, call=_WINO.call)
        return (y, slab) if want_stats else y
    # w16: the filter already rounded to bf16 (optional); split operands: the two tensors' maxima
    if bf == MATH_F16X3 and w_split is None:
        # a LOCAL that lives until the launch below has been enqueued: built inside the argument tuple the temporary was
        # released before the launch, the caching allocator handed its block to the next zero-filled scratch, and the
        # data gradients read a filter of zeros / garbage — non-finite gradients, and a step that ran 10 % FASTER
        w_split = split_filter(w, amax_of(w), n * p * q)
    sfx, tag, tail = _math_call(bf, x, w, w16, w_split, takes_filter=True)
    _launch(_igemm_name("fprop", k, c % 4 != 0, n * p * q) + tag, flops, "rr_conv_fprop" + sfx,
            (x, w, bias, y, slab, n, h, wd, c, k, r, s, stride, pad[0], pad[1], int(relu)) + tail,
            (n, h, wd, c, k, r, s, stride), 4.0 * (x.numel() + y.numel() + w.numel()))
    return (y, slab) if want_stats else y


def conv_packable(x, w, stride):
    """A convolution on very few channels (the 7x7 stride-2 stem on an RGB image): its taps are packed into one row
    per output pixel and it runs as a 1x1 convolution on the vector kernels (conv_fprop_packed / conv_wgrad_packed)."""
    k, c, r, s = w.shape
    return c % 4 != 0 and 32 < r * s * c <= 512 and k >= 32 and not x.requires_grad


def conv_fprop_packed(x, w, stride, pad, want_stats=False):
    """-> (y, slab | None, xp): xp [N,KP,P,Q] = the packed taps (rr_conv_pack_taps), kept for the weight gradient."""
    n, c, h, wd = x.shape
    k, _, r, s = w.shape
    kg = r * s * c
    kp = (kg + 31) // 32 * 32
    p, q = out_hw(h, wd, r, s, stride, pad[0], pad[1])
    xp = empty_nhwc(n, kp, p, q, x.device)
    _C.call("rr_conv_pack_taps", x, xp, n, h, wd, c, r, s, stride, pad[0], pad[1], kp)
    wp = torch.zeros((k, kp), dtype=torch.float32, device=x.device)
    wp[:, :kg] = w.permute(0, 2, 3, 1).reshape(k, kg)                       # OHWI memory = [k][(r,s,c)]
    out = conv_fprop(xp, wp.view(k, kp, 1, 1), None, 1, (0, 0), False,
                     want_stats, algo_kg=kg)
    return (out[0], out[1], xp) if want_stats else (out, None, xp)


def conv_wgrad_packed(xp, dy, dw):
    """dw [K,C,R,S] (OHWI memory) += the weight gradient of the convolution whose packed taps are xp."""
    k, c, r, s = dw.shape
    kg, kp = r * s * c, xp.shape[1]
    dwp = zeros_nhwc(k, kp, 1, 1, xp.device)
    conv_wgrad(xp, dy, dwp, 1, (0, 0), algo_c=kg)
    dw.permute(0, 2, 3, 1).add_(dwp.reshape(k, kp)[:, :kg].view(k, r, s, c))
    return dw


def stem_wgrad_s2d(x, dy, dw):
    """wgrad of the 7x7 stride-2 pad-3 stem on a 3-channel image, computed on the space-to-depth image:
    y[p] = sum_r x[2p-3+r] w[r]  ==  sum_{a<4,i<2} x2[p-2+a, i] w'[2a+i],  x2[u,i] = x[2u+i], w'[r+1] = w[r]
    i.e. a 4x4 stride-1 convolution over 12 channels with leading pad 2 (trailing 1).  Per tap the MFMA
    tile then carries 12 useful channels instead of 3 (49 taps x 32 padded -> 16 taps x 32 padded)."""
    n, c, h, w = x.shape
    k = dw.shape[0]
    assert c == 3 and h % 2 == 0 and w % 2 == 0 and tuple(dw.shape[1:]) == (3, 7, 7)
    xm = x.permute(0, 2, 3, 1)                                   # NHWC view of the memory
    x2 = xm.reshape(n, h // 2, 2, w // 2, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 12)
    x2 = x2.contiguous().permute(0, 3, 1, 2)                     # logical [n,12,h/2,w/2], NHWC memory
    dw2 = zeros_nhwc(k, 12, 4, 4, x.device)                      # OHWI [k][a][b][(i,j,c)]
    conv_wgrad(x2, dy, dw2, 1, (2, 2), explicit_out=True)
    g = dw2.permute(0, 2, 3, 1).reshape(k, 4, 4, 2, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(k, 8, 8, 3)
    dw.permute(0, 2, 3, 1).add_(g[:, 1:, 1:, :])                 # drop the phantom taps r' = 0 / s' = 0
    return dw


_DGRAD_VIA_FPROP = True             # False: rr_conv_dgrad (tests/test_conv_gpu.py::test_conv_fprop_dgrad_wgrad checks both)
_DGRAD_VIA_FPROP_MIN_PIXELS = 4096  # below: the dgrad kernel's split-K wins


class BnLink:
    """What the data gradient of a convolution needs to ALSO produce the BatchNorm-backward sums of the conv -> bn
    [-> +residual] -> relu layer that produced its input (rr_conv_dgrad_s1_bnsum): the producer's pre-BN output y, its
    statistics, and the source of its ReLU mask (z for layers with a residual, scale / shift otherwise).  The consumer's
    backward leaves `sums` (and the gradient tensor they were taken of) here; the producer's backward picks them up
    instead of running rr_bn_bwd_reduce when the gradient it receives is that very tensor."""
    __slots__ = ("y", "use_z", "mean", "invstd", "msc", "msh", "sums", "dz", "consumers", "relu_bias", "mask_only", "want_rows", "rows")

    def __init__(self):
        self.y = self.mean = self.invstd = self.msc = self.msh = self.sums = self.dz = None
        # want_rows: the producer sits behind a loss that touches few pixels (expect_sparse_grad): the consumer's data gradient
        # also lists the pixels of its own dy that are not all zero and leaves (rows, count) in `rows`, next to dz
        self.want_rows = False
        self.rows = None
        # relu_bias: the producer is conv + bias + ReLU (a head's 3x3 layer): the consumer's data gradient stores the
        # ReLU-masked gradient and sums[:c] is the producer's bias gradient (rr_conv_dgrad_s1_relubias)
        self.relu_bias = False
        self.mask_only = False      # relu_bias, and the producer is a bare ReLU (functional._ReLU): only the mask is wanted, no column sums
        # the mask comes from the producer's OUTPUT z (layers with a residual).  The link must not hold z itself — z
        # carries the link as an attribute, and such a cycle keeps a step's activations alive until the cyclic GC runs
        # (the caching allocator then thrashes); the consumer passes its own saved input, which IS z.
        self.use_z = False
        self.consumers = 0


_DGRAD_BNSUM = True     # False: rr_bn_bwd_reduce (test_conv_gpu.py::test_train_step_gradients_equal_with_and_without_fused_bn_sums)
# measured at 8 x 256 x 256 x 256 (tools/bench_head_dgrad.py): K = 10: 0.23 ms against 0.40, K = 2: 0.22 against 0.39; K = 34 (the WH head: 144 filter
# registers per lane, two waves per SIMD): 0.58 against 0.48 — that layer stays on the implicit-GEMM kernel
_HEAD_DGRAD_MAX_K = 12
_HEAD_DGRAD = True      # False: the heads' narrow 1x1 data gradients on the implicit-GEMM kernel
                        # (test_conv_gpu.py::test_head_1x1_dgrad_kernel_accumulate_and_legacy_path checks both)
_BF16_S2_DGRAD = True   # False: stride-2 data gradients stay on the fp32 kernel
_DGRAD_DY16 = ("conv16_s1", "conv16_s2")      # the routes (dgrad_route) that read dy as a bf16 image; every other one reads fp32 memory


def _s2_parity_pads_ok(r, s, pad):
    """The parity-class launches of rr_conv_dgrad_s2_bf16 / _f16x3 need a non-negative leading pad in every class that has
    taps (csrc/conv_bf16.hip, dgrad_s2_impl: lead = taps - 1 - (parity + pad - first tap) // 2); e.g. 3x3 stride 2 pad 2 has
    none — such a layer takes rr_conv_dgrad like every other unsupported shape instead of raising."""
    for size, pd in ((r, pad[0]), (s, pad[1])):
        for par in (0, 1):
            t0 = (par + pd) & 1
            taps = (size - t0 + 1) // 2 if t0 < size else 0
            if taps and (taps - 1) - (par + pd - t0) // 2 < 0:
                return False
    return True


def dgrad_route(dy_shape, w_shape, x_shape, stride, pad, link=None, link_b16=False, have_z=False, device=True):
    """The ONE place where the data-gradient kernel is chosen: conv_dgrad launches what this names; dgrad16_takes and the kernel
    audit ask it.  Shapes and facts in, nothing allocated, no tensor touched; the thread's arithmetic and the module flags are read
    at call time.  link: the producer link the launch may serve — None, "bn", "relu_bias" (conv + bias + ReLU) or "mask_only" (a
    bare ReLU); link_b16: the link's y, or the z handed in, is a bf16 image only; have_z: the mask source the link needs is there.
    -> (route, arithmetic MATH_*); each route's launcher (_dgrad_*, below) names its entry point."""
    n, c, h, wd = x_shape
    k, _, r, s = w_shape
    npx, dx_elems, dy_elems = n * h * wd, n * h * wd * c, dy_shape[0] * dy_shape[1] * dy_shape[2] * dy_shape[3]
    if link == "bn" and link_b16:
        link = None         # no fp32 y / z for the epilogue to read: the producer runs its own reduce pass (rr_bn_bwd_reduce_b16)
    relu_bias = link in ("relu_bias", "mask_only")
    inside, fits32 = pad[0] < r and pad[1] < s, dx_elems * 4 < (1 << 31)
    # csrc/conv16.hip (bf16 mode): both operands as bf16 tensors below 2 GiB, maps of at least _CONV16_MIN_PIXELS output pixels
    conv16 = _CONV16 and _mode() == MATH_BF16 and device and max(dy_elems, dx_elems) * 2 < (1 << 31)
    s1_16 = bool(stride == 1 and inside and conv16 and npx >= _CONV16_MIN_PIXELS and _C.call("rr_conv16_supported", k, c, r, s, 1))

    def math(kk, pixels):           # the arithmetic of a csrc/conv_bf16.hip launch on a dy of kk channels
        return _bf16_ok(kk, c, r, s, pixels=pixels) if max(dy_elems // k * kk, dx_elems) * 4 < (1 << 31) else 0
    if (relu_bias and _DGRAD_BNSUM and stride == 1 and c % 4 == 0 and have_z and fits32 and r * s <= 64 and inside
            and dy_shape[2] * dy_shape[3] >= _DGRAD_VIA_FPROP_MIN_PIXELS and npx % 128 == 0):      # whole 128-row tiles only (fprop_impl in csrc/conv.hip)
        if link == "mask_only" and s1_16:
            return "relumask", MATH_BF16
        if r == 1 and s == 1 and k <= _HEAD_DGRAD_MAX_K and 1024 % c == 0 and _HEAD_DGRAD and device:
            return "head", MATH_F32           # an fp32 element-wise pass in every arithmetic
        return "relubias", math((k + 3) // 4 * 4, npx)       # (a 10- / 2-channel dy is zero-padded to 12 / 4)
    if s1_16 and not relu_bias:
        return "conv16_s1", MATH_BF16
    if stride == 1 and k % 4 == 0 and c % 4 == 0 and r * s <= 64 and inside and _DGRAD_VIA_FPROP:
        # 16-bit operands: the forward kernel at every size — its split-K covers the small maps, and the dgrad kernel is fp32-only
        bf = math(k, npx)
        if bf or dy_shape[2] * dy_shape[3] >= _DGRAD_VIA_FPROP_MIN_PIXELS:
            return ("fprop_bnsum" if link == "bn" and _DGRAD_BNSUM and c <= 1024 and fits32 and have_z else "fprop"), bf
    if stride == 2 and _BF16_S2_DGRAD and _s2_parity_pads_ok(r, s, pad):
        if conv16 and k % 64 == 0 and c % 128 == 0 and r * s <= 16 and npx // 4 >= _CONV16_MIN_PIXELS:
            return "conv16_s2", MATH_BF16
        bf = math(k, npx // 4)
        if bf:
            return "parity_s2", bf
    return "dgrad", MATH_F32


def dgrad16_takes(dy_shape, w_shape, x_shape, stride, pad, relu_bias_link=False):
    """True when conv_dgrad(dy, w, x_shape, ...) reads dy's bf16 image only (functional: the fp32 dy need not be written)."""
    return dgrad_route(dy_shape, w_shape, x_shape, stride, pad, "relu_bias" if relu_bias_link else None)[0] in _DGRAD_DY16


def link_facts(bnsum, bnsum_z, x_shape):
    """A BnLink and the z that came with it -> (link, link_b16, have_z) as dgrad_route takes them."""
    if bnsum is None or not (bnsum.relu_bias or (bnsum.y is not None and tuple(bnsum.y.shape) == tuple(x_shape))):
        return None, False, False
    z_ok = bnsum_z is not None and (is_phantom(bnsum_z) or is_nhwc(bnsum_z)) and tuple(bnsum_z.shape) == tuple(x_shape)
    if bnsum.relu_bias:
        return "mask_only" if bnsum.mask_only else "relu_bias", is_phantom(bnsum_z), z_ok
    return "bn", is_phantom(bnsum.y) or is_phantom(bnsum_z), not bnsum.use_z or z_ok


def _flipped_filter(w, wt, wt16, want16):
    """-> (wt, wt16): the flipped / transposed filter (one tiny transpose per layer and step) and, with want16, its bf16 copy —
    unless the caller brought them (FlatParams.wt_view / w16_views)."""
    if wt is None and not (want16 and wt16 is not None):
        wt = torch.empty(w.numel(), dtype=torch.float32, device=w.device)
        _C.call("rr_weight_flip_transpose", w, wt, *w.shape)
    if want16 and wt16 is None:
        wt16 = torch.empty(wt.numel(), dtype=torch.bfloat16, device=w.device)
        _C.call("rr_to_bf16", wt, wt16, wt.numel())
    return wt, wt16


# The launchers, one per route or family.  geo = (n, h, wd, c, k, r, s, pad_h, pad_w, accumulate): the argument run the entry
# points share; geo[:7] + (stride,) is the timer's detail.  link: the BnLink the launch serves (None: none).
def _dgrad_conv16_s1(dy, w, out, geo, flops, wt, wt16, link=None, z=None):
    """conv16_s1 / relumask (csrc/conv16.hip): the forward kernel on dY's bf16 image and the flipped filter's bf16 copy; for a bare
    ReLU producer (link) with its mask in the epilogue.  (The producer's BatchNorm-backward sums are NOT carried by this kernel: the
    producer runs its reduce pass.  An epilogue that did — round 5 — lost: with one workgroup per CU its image reads are in the open,
    config-4 step 111.8-113.3 ms against 108.9-110.8 ms; removed in round 6, the numbers live in DESIGN §13.1.)"""
    dy16 = bf16_of(dy)
    wt16 = _flipped_filter(w, wt, wt16, True)[1]
    if link is None:
        _launch("conv16_dgrad_s1", flops, "rr_conv16_dgrad_s1", (dy16, wt16, out, None) + geo, geo[:7] + (1,),
                2.0 * (dy.numel() + w.numel()) + 4.0 * out.numel() * (2 if geo[9] else 1))
        return
    _launch("conv16_dgrad_s1+relumask", flops, "rr_conv16_dgrad_s1_relumask", (dy16, wt16, out) + geo + (z,), geo[:7] + (1,))
    link.sums, link.dz = _ZEROS.take(2, dy.device), out          # (sums: the "done" marker _ReLU.backward looks for)


def _dgrad_relubias(dy, w, out, geo, flops, bf, link, z, wt, head):
    """relubias / head: producer = conv + bias + ReLU: masked gradient + bias column sums in this launch's epilogue.  head: a head's narrow
    1x1 layer (K = 10 / 2 / 34 of 36) is not a GEMM worth a matrix kernel — one HBM-bound pass of the same contract; under conv16 the bf16
    image of dx comes out of it too.  Else a 10- or 2-channel dy is zero-padded to a multiple of 4 for the vector kernel (25 MB at 8x256x256)."""
    n, h, wd, c, k, r, s = geo[:7]
    link.sums, link.dz = _ZEROS.take(2 * c, dy.device), out
    if link.want_rows and _CONV_ROWS and r == 1 and s == 1 and _mode() == MATH_F32:
        link.rows = active_rows(dy)          # a 1x1 layer: dz is zero wherever dy is (the masked gradient and the sums are written as ever)
    if head:
        want16 = image_wanted(c, n * h * wd, dy.device, 256)
        out16 = torch.empty_like(out, dtype=torch.bfloat16) if want16 else None
        _C.call("rr_head_dgrad_relubias", dy, w, out, out16, z, link.sums, n * h * wd, c, k, geo[9])
        if want16:
            b16_side.attach(out, out16)
        return
    kp = (k + 3) // 4 * 4
    if kp != k:
        dyp, wp, wt = empty_nhwc(dy.shape[0], kp, dy.shape[2], dy.shape[3], dy.device), zeros_nhwc(kp, c, r, s, dy.device), None
        _C.call("rr_pad_channels", dy, dyp, dy.shape[0] * dy.shape[2] * dy.shape[3], k, kp)
        wp[:k] = w
        dy, w = dyp, wp
    wt = _flipped_filter(w, wt, None, False)[0]
    slab = torch.empty(_C.call("rr_conv_stat_slab_bytes", n, h, wd, c) // 8, dtype=torch.float64, device=dy.device)
    sfx, tag, tail = _math_call(bf, dy, w)
    _launch(_igemm_name("fprop", c, False, n * h * wd) + "+relubias" + tag, flops, "rr_conv_dgrad_s1_relubias" + sfx,
            (dy, wt, out, n, h, wd, c, kp) + geo[5:] + (z, slab, link.sums) + tail, geo[:7] + (1,))


def _dgrad_fprop(dy, w, out, geo, flops, bf, wt, wt16, wt_split, link=None, z=None):
    """fprop / fprop_bnsum: the forward kernel on dy with the flipped / transposed filter — the same HIP kernel instance as a forward
    convolution, timed under its name; with a link the producer's BatchNorm-backward sums come out of its epilogue."""
    n, h, wd, c = geo[:4]
    wt = _flipped_filter(w, wt, None, False)[0]
    if bf == MATH_F16X3 and wt_split is None:
        wt_split = split_filter(w, amax_of(w), n * h * wd, flat=wt)
    sfx, tag, tail = _math_call(bf, dy, w, wt16, wt_split, takes_filter=True)
    sfx = ("_bnsum" if link is not None else "") + sfx
    name = _igemm_name("fprop", c, False, n * h * wd) + ("+bnsum" if link is not None else "") + tag
    if link is not None:
        slab = torch.empty(_C.call("rr_conv_stat_slab_bytes", n, h, wd, c) // 8, dtype=torch.float64, device=dy.device)
        link.sums, link.dz = _ZEROS.take(2 * c, dy.device), out
        tail = (link.y, z if link.use_z else None, link.mean, link.invstd, link.msc, link.msh, slab, link.sums) + tail
    _launch(name, flops, "rr_conv_dgrad_s1" + sfx, (dy, wt, out) + geo + tail, geo[:7] + (1,),
            4.0 * (dy.numel() + out.numel() * ((2 if geo[9] else 1) + (link is not None)) + w.numel()))


def _dgrad_s2(dy, w, out, geo, flops, bf, conv16):
    """conv16_s2 / parity_s2: a forward-kernel launch per output parity class on its sub-filter, packed inside the call, on dY's bf16 image / on dy."""
    src = bf16_of(dy) if conv16 else dy
    wsub = torch.empty(w.numel(), dtype=torch.bfloat16 if conv16 else torch.float32, device=dy.device)
    sfx, tag, tail = _math_call(bf, dy, w)             # (bf is never MATH_F32 here, and MATH_BF16 under conv16: dgrad_route)
    _launch("conv16_dgrad_s2" if conv16 else "conv_dgrad_s2" + tag, flops, "rr_conv16_dgrad_s2" if conv16 else "rr_conv_dgrad_s2" + sfx,
            (src, w, out) + geo + (wsub,) + tail, geo[:7] + (2,))


def _dgrad_fp32(dy, w, out, geo, flops, stride):
    n, h, wd, c, k = geo[:5]
    _launch(_igemm_name("dgrad", c, (k % 4 != 0) or (c % 4 != 0), n * h * wd, stride), flops, "rr_conv_dgrad",
            (dy, w, out) + geo[:7] + (stride,) + geo[7:], geo[:7] + (stride,))


# The Winograd F(2x2,3x3) route of the large stride-1 fp32 3x3 convolutions (csrc/conv_wino.hip): conv_fprop and the
# "fprop" / "fprop_bnsum" data gradients take it where rr_conv_wino_plan does.  RR_CONV_WINO=0: never taken (the A/B switch).
_WINO = _C.Family("rrnet_hip_wino.h")
_CONV_WINO = os.environ.get("RR_CONV_WINO", "1") != "0"
_WINO_BELOW_FLOOR = False       # test switch: the route also where the plan's pixel floor is its only objection (tests/test_conv_wino_gpu.py)
_WINO_TAKES = {}                # plan arguments -> the plan's answer (take, the floor is the only reason not to)
_WINO_PLAN_FN = {}              # plan entry -> its typed function
_WINO_WS = {}                   # (device, stream) -> the grow-only workspace V + M of the launches enqueued there
FLAT_BUFFERS = weakref.WeakSet()     # the FlatParams that keep transformed filters (rrnet_amd/flat.py registers itself)


def wino_takes(n, h, wd, c, k, r, s, stride, pad, bias=False, relu=False, stats=False, accumulate=False, link=False):
    """Does the Winograd route take this forward-kernel launch (fp32 arithmetic; a data gradient in its forward geometry)?
    rr_plan::wino_plan's decision, asked once per distinct launch."""
    if not _CONV_WINO:
        return False
    key = (n, h, wd, c, k, r, s, stride, pad[0], pad[1], int(bias) | int(relu) << 1 | int(stats) << 2 | int(accumulate) << 3 | int(link) << 8)
    hit = _WINO_TAKES.get(key)
    if hit is None:
        plan = (_C.c_int * 11)()
        _C.check(_wino_plan_fn("rr_conv_wino_plan")(MATH_F32, *key[:10], 0, 0, key[10], plan), "rr_conv_wino_plan")
        hit = _WINO_TAKES[key] = (bool(plan[0]), bool(plan[1]))
    return hit[0] or (hit[1] and _WINO_BELOW_FLOOR)


def _wino_plan_fn(entry):
    # typed from the header like every entry, but asked past _C.fn: a shape predicate launches nothing, and how often the host
    # asks it is not part of what a call computes (the launch records of tests/conv_route_cases.py)
    f = _WINO_PLAN_FN.get(entry)
    if f is None:
        f, (sig, _) = getattr(_C.lib(), entry), _C.declared(entry)
        f.restype, f.argtypes = sig[0], sig[1]
        _WINO_PLAN_FN[entry] = f
    return f


def _wino_ws(device, n, h, wd, c, k, entry="rr_conv_wino_ws_bytes"):
    """The workspace of one launch: never allocated per call, grown to the largest layer seen on this stream.  The compute stream's
    block serves the forward and data-gradient launches; the weight gradients of the route (entry: rr_conv_wino_wgrad_ws_bytes) run
    on functional._wgrad_async's side stream and get a block of their own there."""
    need = _WINO.call(entry, n, h, wd, c, k) // 4
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    ws = _WINO_WS.get(key)
    if ws is None or ws.numel() < need:
        _WINO_WS[key] = None         # (the old block goes back before the larger one is asked for)
        ws = _WINO_WS[key] = torch.empty(need, dtype=torch.float32, device=device)
    return ws


def _wino_filter(w, flipped, wt=None):
    """U [16][K'][C'] of the filter w (flipped: of its flipped / transposed form, the data gradient's filter): the cached transform
    of a FlatParams buffer's parameter (one launch per optimizer step for all of them), else transformed here."""
    for flat in FLAT_BUFFERS:
        u = flat.wino_view(w, flipped)
        if u is not None:
            return u
    k, c = w.shape[0], w.shape[1]
    src = _flipped_filter(w, wt, None, False)[0] if flipped else w
    u = torch.empty(16 * k * c, dtype=torch.float32, device=w.device)
    _WINO.call("rr_wino_filter", src, u, *((c, k) if flipped else (k, c)))
    return u


# The weight gradients of the same layers as F(3x3,2x2) (rr_conv_wino_wgrad): conv_wgrad takes the route where
# rr_conv_wino_wgrad_plan does.  RR_CONV_WINO_WGRAD=0: never taken (an A/B switch of its own: RR_CONV_WINO keeps its meaning).
_CONV_WINO_WGRAD = os.environ.get("RR_CONV_WINO_WGRAD", "1") != "0"
_WINO_WGRAD_BELOW_FLOOR = False       # test switch (tests/test_conv_wino_wgrad_gpu.py), as _WINO_BELOW_FLOOR
_WINO_WGRAD_TAKES = {}


def wino_wgrad_takes(n, h, wd, c, k, r, s, stride, pad, explicit_out=False, gated=False):
    """Does the Winograd route take this fp32 weight-gradient launch?  rr_plan::wino_wgrad_plan's decision, asked once per shape."""
    if not _CONV_WINO_WGRAD or explicit_out:        # (an explicit output size: the plan refuses it)
        return False
    key = (n, h, wd, c, k, r, s, stride, pad[0], pad[1], 0, 0, int(gated))
    hit = _WINO_WGRAD_TAKES.get(key)
    if hit is None:
        plan = (_C.c_int * 10)()
        _C.check(_wino_plan_fn("rr_conv_wino_wgrad_plan")(MATH_F32, *key, plan), "rr_conv_wino_wgrad_plan")
        hit = _WINO_WGRAD_TAKES[key] = (bool(plan[0]), bool(plan[1]))
    return hit[0] or (hit[1] and _WINO_WGRAD_BELOW_FLOOR)


def _dgrad_wino(dy, w, out, geo, flops, wt, link=None, z=None):
    """fprop / fprop_bnsum on the Winograd route: the data gradient as the convolution of dy with the flipped filter; with a link the
    producer's BatchNorm-backward sums come out of the output transform's epilogue (rr_conv_dgrad_s1_bnsum's contract)."""
    n, h, wd, c, k = geo[:5]
    u, ws = _wino_filter(w, True, wt), _wino_ws(dy.device, n, h, wd, k, c)
    nbytes = 4.0 * (dy.numel() + out.numel() * ((2 if geo[9] else 1) + (link is not None)) + w.numel()) + 2.0 * ws.numel() * 4.0
    if link is None:
        _launch("conv_dgrad<wino>", flops * 16.0 / 36.0, "rr_conv_wino_fprop",
                (dy, u, None, out, None, ws, ws.numel() * 4, n, h, wd, k, c, 0, geo[9]), geo[:7] + (1,), nbytes, call=_WINO.call)
        return
    slab = torch.empty(_C.call("rr_conv_stat_slab_bytes", n, h, wd, c) // 8, dtype=torch.float64, device=dy.device)
    link.sums, link.dz = _ZEROS.take(2 * c, dy.device), out
    _launch("conv_dgrad<wino>+bnsum", flops * 16.0 / 36.0, "rr_conv_wino_dgrad_bnsum",
            (dy, u, out, ws, ws.numel() * 4, n, h, wd, c, k, geo[9], link.y, z if link.use_z else None, link.mean, link.invstd, link.msc,
             link.msh, slab, link.sums), geo[:7] + (1,), nbytes, call=_WINO.call)


# The rows route (csrc/conv_rows.hip).  RR_CONV_ROWS=0: never taken (the A/B switch).
_ROWS = _C.Family("rrnet_hip_rows.h")       # the family's own header beside include/rrnet_hip.h
_CONV_ROWS = os.environ.get("RR_CONV_ROWS", "1") != "0"
# the list length up to which the rows kernels do the work, as a share of the map's pixels: a design constant below the crossover
# measured with tools/bench_conv.py --rows (profiles/conv_rows_shapes.txt); the choice itself is made on the device
_ROWS_MAX_SHARE = 8
_TARGETS_MAX_SHARE = 4      # the same for the data gradient's list of dx pixels (a 3x3 reaches up to nine per listed dy pixel)


def active_rows(dy):
    """dy [N,K,H,W] (NHWC) -> (rows int32[N*H*W], count int32[1], work): the ascending indices of its pixels that hold a non-zero value;
    work: the scratch with the bit per pixel that active_targets reads."""
    m, k = dy.shape[0] * dy.shape[2] * dy.shape[3], dy.shape[1]
    rows = torch.empty(m, dtype=torch.int32, device=dy.device)
    count = torch.empty(1, dtype=torch.int32, device=dy.device)
    work = torch.empty(_ROWS.call("rr_active_rows_work_bytes", m) // 4, dtype=torch.int32, device=dy.device)
    _ROWS.call("rr_active_rows", dy, m, k, rows, count, work)
    return rows, count, work


def active_targets(listed, x_shape, r, s, pad):
    """active_rows' result for a dy -> (targets int32[N*H*W], count int32[1]): the pixels of dx [x_shape] a listed pixel reaches through a tap."""
    n, _, h, wd = x_shape
    dev = listed[0].device
    targets = torch.empty(n * h * wd, dtype=torch.int32, device=dev)
    count = torch.empty(1, dtype=torch.int32, device=dev)
    work = torch.empty(_ROWS.call("rr_active_rows_work_bytes", n * h * wd) // 4, dtype=torch.int32, device=dev)
    _ROWS.call("rr_active_targets", listed[2], n, h, wd, r, s, pad[0], pad[1], targets, count, work)
    return targets, count


def _rows_shape_ok(dy, x_shape, w_shape, stride):
    """The shapes the pair (rows entry point + _unless entry point) takes: stride 1, a filter with more than one tap on a map of at
    least 64 pixels (the plain forward kernel is the dense side), C and K multiples of 4, every tensor below 2 GiB."""
    n, c, h, wd = x_shape
    k, _, r, s = w_shape
    return (_CONV_ROWS and stride == 1 and _mode() == MATH_F32 and c % 4 == 0 and k % 4 == 0 and 1 < r * s <= 64 and h * wd >= 64
            and tuple(dy.shape[2:]) == (h, wd) and max(n * h * wd * max(c, k), k * c * r * s) * 4 < (1 << 31))


def _dgrad_rows_pair(dy, w, out, geo, wt, listed):
    """Both sides of the gate on the same (count, max_rows): the rows kernel on the dx pixels the listed dy pixels reach, the forward kernel on
    the flipped filter unless that list is short.  Timer keys of their own with no FLOPs: the one that returns at its gate must not enter a
    roofline figure."""
    rows, count = active_targets(listed, geo[:1] + (geo[3],) + geo[1:3], geo[5], geo[6], geo[7:9])
    max_rows = geo[0] * geo[1] * geo[2] // _TARGETS_MAX_SHARE
    wt = _flipped_filter(w, wt, None, False)[0]
    _launch("conv_dgrad<rows>", 0.0, "rr_conv_dgrad_s1_rows", (dy, w, out) + geo + (rows, count, max_rows), geo[:7] + (1,), call=_ROWS.call)
    _launch("conv_dgrad<dense>", 0.0, "rr_conv_dgrad_s1_unless", (dy, wt, out) + geo + (count, max_rows), geo[:7] + (1,), call=_ROWS.call)


def conv_dgrad(dy, w, x_shape, stride=1, pad=(0, 0), out=None, accumulate=False, bnsum=None, bnsum_z=None, wt=None, wt16=None,
               wt_split=None):
    """dy [N,K,P,Q], w [K,C,R,S] -> dx [N,C,H,W]; with `out` and accumulate adds into it.  The kernel is dgrad_route's choice.
    wt: the flipped / transposed filter (rr_weight_flip_transpose of w) when the caller keeps one (FlatParams.wt_view).
    bnsum (BnLink of the layer that produced the convolution's input): when the launch can carry them, the producer's BatchNorm-backward
    sums are computed in the epilogue and left in bnsum.sums / bnsum.dz.  bnsum_z: the convolution's input itself, needed when bnsum.use_z."""
    _C.require_cuda(dy, w)
    assert (is_nhwc(dy) or is_phantom(dy)) and is_nhwc(w)     # (phantom: a bf16-only gradient, see phantom_f32)
    n, c, h, wd = x_shape
    k, c2, r, s = w.shape
    assert c == c2 and dy.shape[1] == k
    if out is None:
        out = empty_nhwc(n, c, h, wd, dy.device)
        accumulate = False
    else:
        amax_drop(out)                # an existing tensor rewritten / added into through its pointer
    assert is_nhwc(out)
    link, link_b16, have_z = link_facts(bnsum, bnsum_z, x_shape)
    if link_b16 and link != "bn":
        bnsum_z = f32_of(bnsum_z)     # a ReLU / bias producer whose output is a bf16 image only: its mask is read from the widened copy
    route, bf = dgrad_route(tuple(dy.shape), tuple(w.shape), x_shape, stride, pad, link, link_b16, have_z, dy.is_cuda)
    if is_phantom(dy) and route not in _DGRAD_DY16:
        dy = f32_of(dy)               # (relumask included: it rounds the widened copy again — exact, but two passes too many)
    geo = (n, h, wd, c, k, r, s, pad[0], pad[1], int(accumulate))
    flops = 2.0 * dy.shape[0] * dy.shape[2] * dy.shape[3] * k * c * r * s
    listed = rows_side.now(dy) if route in ("fprop", "fprop_bnsum") and bf == MATH_F32 else None
    if listed is not None and _rows_shape_ok(dy, x_shape, w.shape, stride):
        # the pair carries no link: a launch that may return at its gate cannot produce the producer's sums (its own pass runs)
        _dgrad_rows_pair(dy, w, out, geo, wt, listed)
    elif (route in ("fprop", "fprop_bnsum") and bf == MATH_F32
          and wino_takes(n, h, wd, k, c, r, s, stride, (r - 1 - pad[0], s - 1 - pad[1]), accumulate=accumulate, link=route == "fprop_bnsum")):
        _dgrad_wino(dy, w, out, geo, flops, wt, *((bnsum, bnsum_z) if route == "fprop_bnsum" else ()))
    elif route in ("conv16_s1", "relumask"):
        _dgrad_conv16_s1(dy, w, out, geo, flops, wt, wt16, *((bnsum, bnsum_z) if route == "relumask" else ()))
    elif route in ("relubias", "head"):
        _dgrad_relubias(dy, w, out, geo, flops, bf, bnsum, bnsum_z, wt, route == "head")
    elif route in ("fprop", "fprop_bnsum"):
        _dgrad_fprop(dy, w, out, geo, flops, bf, wt, wt16, wt_split, *((bnsum, bnsum_z) if route == "fprop_bnsum" else ()))
    elif route in ("conv16_s2", "parity_s2"):
        _dgrad_s2(dy, w, out, geo, flops, bf, route == "conv16_s2")
    else:
        _dgrad_fp32(dy, w, out, geo, flops, stride)
    return out


def conv_wgrad(x, dy, dw, stride=1, pad=(0, 0), explicit_out=False, algo_c=None):
    """dw [K,C,R,S] (OHWI memory) += x (*) dy.  dw must be pre-zeroed / hold the running gradient.
    explicit_out: take the output size from dy (asymmetric padding, `pad` = leading pads)."""
    _C.require_cuda(x, dy, dw)
    assert (is_nhwc(x) or is_phantom(x)) and (is_nhwc(dy) or is_phantom(dy)) and is_nhwc(dw)
    n, c, h, wd = x.shape
    k, c2, r, s = dw.shape
    assert c == c2 and dy.shape[1] == k
    flops = 2.0 * dy.shape[0] * dy.shape[2] * dy.shape[3] * k * (c * r * s if algo_c is None else algo_c)
    if wgrad16_takes(x.shape, dy.shape, dw.shape, stride) and not explicit_out:
        x16, dy16 = bf16_of(x), bf16_of(dy)
        _launch("conv16_wgrad", flops, "rr_conv16_wgrad", (x16, dy16, dw, n, h, wd, c, k, r, s, stride, pad[0], pad[1]),
                (n, h, wd, c, k, r, s, stride))
        return dw
    listed = rows_side.now(dy) if not explicit_out and not is_phantom(x) and not is_phantom(dy) else None
    if listed is not None and _rows_shape_ok(dy, tuple(x.shape), tuple(dw.shape), stride):
        rows, count = listed[:2]
        args = (x, dy, dw, n, h, wd, c, k, r, s, pad[0], pad[1])
        max_rows = n * h * wd // _ROWS_MAX_SHARE
        _launch("conv_wgrad<rows>", 0.0, "rr_conv_wgrad_rows", args + (rows, count, max_rows), (n, h, wd, c, k, r, s, 1), call=_ROWS.call)
        _launch("conv_wgrad<dense>", 0.0, "rr_conv_wgrad_unless", args + (count, max_rows), (n, h, wd, c, k, r, s, 1), call=_ROWS.call)
        return dw
    x, dy = f32_of(x), f32_of(dy)            # (bf16-only operands in front of a layer the conv16 weight gradient does not take)
    bf = _bf16_ok(c, k, r, s, x, dy, pixels=dy.shape[0] * dy.shape[2] * dy.shape[3]) if wgrad_16bit_shape(c, k, r, s) else 0
    if bf == MATH_F32 and wino_wgrad_takes(n, h, wd, c, k, r, s, stride, pad, explicit_out):
        # the Winograd route; its timer key carries the multiplications it executes, 16 of the direct 36
        ws = _wino_ws(x.device, n, h, wd, c, k, "rr_conv_wino_wgrad_ws_bytes")
        tiles = n * ((h + 1) // 2) * ((wd + 1) // 2)
        used = 4.0 * (16 * tiles * (c + k) + 16 * k * c)        # V + W + S of this launch (the block itself is grow-only), written and read once
        _launch("conv_wgrad<wino>", flops * 16.0 / 36.0, "rr_conv_wino_wgrad", (x, dy, dw, ws, ws.numel() * 4, n, h, wd, c, k),
                (n, h, wd, c, k, r, s, stride), 4.0 * (x.numel() + dy.numel() + 2 * dw.numel()) + 2.0 * used, call=_WINO.call)
        return dw
    sfx, tag, wtail = _math_call(bf, x, dy)
    _launch("conv_wgrad<BN=%d>%s" % (128 if c > 32 else 32, tag), flops, "rr_conv_wgrad" + sfx,
            (x, dy, dw, n, h, wd, c, k, r, s, stride, pad[0], pad[1]) + ((dy.shape[2], dy.shape[3]) if explicit_out else (0, 0)) + wtail,
            (n, h, wd, c, k, r, s, stride))
    return dw


# ---------------------------------------------------------------------------------------------
# BatchNorm / elementwise
# ---------------------------------------------------------------------------------------------
def _f32(n, device):
    return torch.empty(n, dtype=torch.float32, device=device)


class _ZeroPool:
    """Pre-zeroed float64 scratch handed out in slices: the 163 BatchNorm layers of a step take their statistics
    accumulators from one zeroed chunk (one fill per ~1 MB) instead of one `torch.zeros` launch each.  A slice is
    never handed out twice; exhausted chunks stay alive as long as their slices do.
    A chunk belongs to the stream that was current when it was filled: a take() on another stream (the DCN backward's
    side stream) gets its own chunk, so every slice is ordered behind its fill.  Slices are independent tensors over
    the chunk's storage (own version counters): an in-place write into one does not invalidate siblings that
    autograd saved."""

    CHUNK = 128 * 1024      # doubles

    def __init__(self):
        self.buf = {}

    def take(self, n, device):
        n8 = (n + 1) // 2 * 2                      # keep slices 16-byte aligned
        key = (device.type, device.index, torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else 0)
        cur = self.buf.get(key)
        if cur is None or cur[1] + n8 > cur[0].numel():
            cur = [torch.zeros(max(self.CHUNK, n8), dtype=torch.float64, device=device), 0]
            self.buf[key] = cur
        out = torch.empty(0, dtype=torch.float64, device=device).set_(cur[0].untyped_storage(), cur[1], (n,))
        cur[1] += n8
        return out


_ZEROS = _ZeroPool()


def bn_reduce_slab(slab, c, extra=0, count=None):
    """slab [mtiles,2,c] doubles -> sums [2c (+extra)] doubles (extra slots zeroed: room for the
    sample count in the SyncBN exchange).  count: the local sample count, stored into sums[2c] by the same launch."""
    sums = _ZEROS.take(2 * c + extra, slab.device)
    mtiles = slab.numel() // (2 * c)
    if count is not None:
        assert extra >= 1
        _C.call("rr_bn_reduce_slab_count", slab, mtiles, c, sums, float(count), sums[2 * c:])
        return sums
    _C.call("rr_bn_reduce_slab", slab, mtiles, c, sums)
    return sums


def bn_finalize_sync(sums, count_slot, gamma, beta, running_mean, running_var, momentum, eps, num_batches_tracked=None):
    """bn_finalize for an exchanged statistics buffer: the (global) sample count is read from the device (`count_slot`, a slot of
    the buffer that went through the all-reduce) and handed back in storage of its own for the backward.
    -> mean, invstd, scale, shift, count (float64 [1])"""
    c = gamma.numel()
    buf = _f32(4 * c, gamma.device)
    mean, invstd, scale, shift = buf[0:c], buf[c:2 * c], buf[2 * c:3 * c], buf[3 * c:4 * c]
    cnt = torch.empty(1, dtype=torch.float64, device=gamma.device)
    _C.call("rr_bn_finalize_count", sums, count_slot, gamma, beta, running_mean, running_var, float(momentum), float(eps), mean,
            invstd, scale, shift, c, num_batches_tracked, cnt)
    return mean, invstd, scale, shift, cnt


def bn_affine_grad(sums, dgamma, dbeta):
    """dbeta += sums[:c], dgamma += sums[c:2c] (the LOCAL BatchNorm-backward sums, before their SyncBN exchange): one launch."""
    c = dgamma.numel()
    assert dgamma.is_contiguous() and dbeta.is_contiguous()
    _C.call("rr_bn_affine_grad", sums, dgamma, dbeta, c)


def bn_finalize(sums, count, gamma, beta, running_mean, running_var, momentum, eps, count_dev=None,
                num_batches_tracked=None):
    c = gamma.numel()
    dev = gamma.device
    buf = _f32(4 * c, dev)                       # mean | invstd | scale | shift: one allocation
    mean, invstd, scale, shift = buf[0:c], buf[c:2 * c], buf[2 * c:3 * c], buf[3 * c:4 * c]
    _C.call("rr_bn_finalize", sums, float(count), count_dev, gamma, beta, running_mean, running_var, float(momentum), float(eps),
            mean, invstd, scale, shift, c, num_batches_tracked)
    return mean, invstd, scale, shift


def bn_stats_finalize(slab, count, gamma, beta, running_mean, running_var, momentum, eps, num_batches_tracked=None):
    """bn_reduce_slab + bn_finalize in one launch (single process: nothing to exchange in between)."""
    c = gamma.numel()
    buf = _f32(4 * c, gamma.device)
    mean, invstd, scale, shift = buf[0:c], buf[c:2 * c], buf[2 * c:3 * c], buf[3 * c:4 * c]
    mtiles = slab.numel() // (2 * c)
    _C.call("rr_bn_stats_finalize", slab, mtiles, float(count), gamma, beta, running_mean, running_var, float(momentum), float(eps),
            mean, invstd, scale, shift, c, num_batches_tracked)
    return mean, invstd, scale, shift


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps):
    c = gamma.numel()
    scale, shift = _f32(c, gamma.device), _f32(c, gamma.device)
    _C.call("rr_bn_eval_coeffs", gamma, beta, running_mean, running_var, float(eps), scale, shift, c)
    return scale, shift


def _operand(t, phantom):
    """-> (fp32 tensor, image) of an operand the `_b16` entry points read in either form: one of the two is None (NULL)."""
    return (None, image_of(t)) if phantom else (t, None)


def _produced(n, c, h, w, device, f32, image):
    """-> (fp32 tensor | None, bf16 image | None) for a producer to write."""
    return (empty_nhwc(n, c, h, w, device) if f32 else None, empty_nhwc(n, c, h, w, device, torch.bfloat16) if image else None)


def _published(out, out16, word=None):
    """What the producer returns: its fp32 tensor with the sidecars it wrote in the same pass — or, bf16-only, the phantom handle."""
    if out is None:
        return phantom_f32(tuple(out16.shape), out16.device, out16)
    if out16 is not None:
        b16_side.attach(out, out16)     # the bf16 image the consuming convolution (csrc/conv16.hip) reads
    if word is not None:
        amax_side.attach(out, word)     # split-operand convolutions: the consumer's operand scale (see amax_of)
    return out


def bn_apply(y, scale, shift, residual=None, relu=False, res_scale=None, res_shift=None, bf16_only=False):
    """bf16_only (conv16, ops.phantom_scope): the output is written as a bf16 image only and returned as a memory-less fp32
    handle (phantom_f32).  A bf16-only residual is read from its image."""
    res_ph, y_ph = is_phantom(residual), is_phantom(y)
    assert (is_nhwc(y) or y_ph) and (residual is None or ((is_nhwc(residual) or res_ph) and residual.shape == y.shape))
    n, c, h, w = y.shape
    mixed = bool((bf16_only or res_ph or y_ph) and y.is_cuda and c % 4 == 0)       # an operand or the output exists as an image only
    only16 = mixed and bf16_only
    out, out16 = _produced(n, c, h, w, y.device, not only16, only16 or image_wanted(c, n * h * w, y.device))
    if mixed or out16 is not None:
        _C.call("rr_bn_apply_b16", *_operand(y, y_ph), scale, shift, *_operand(residual, res_ph), res_scale, res_shift, out, out16,
                y.numel(), c, int(relu))
        return _published(out, out16)
    head = (y, scale, shift, residual, res_scale, res_shift, out, y.numel(), c, int(relu))
    if amax_wanted(c, n * h * w, y.device):
        word = _amax_word(y.device)
        _C.call("rr_bn_apply_amax", *head, word)
        return _published(out, None, word)
    _C.call("rr_bn_apply", *head)
    return out


def bn_bwd_reduce(dz, z, y, mean, invstd, extra=0, mask_scale=None, mask_shift=None):
    n, c, h, w = y.shape
    sums = _ZEROS.take(2 * c + extra, y.device)            # pre-zeroed pool slice: no memset launch per layer
    z_ph, y_ph = is_phantom(z), is_phantom(y)
    if z_ph or y_ph:                                        # the layer's output / pre-BN output exist only as bf16 images
        _C.call("rr_bn_bwd_reduce_b16", dz, *_operand(z, z_ph), *_operand(y, y_ph), mean, invstd, mask_scale, mask_shift, sums,
                n * h * w, c)
        return sums
    _C.call("rr_bn_bwd_reduce", dz, z, y, mean, invstd, mask_scale, mask_shift, sums, n * h * w, c, 1)
    return sums


def bn_bwd_apply(dz, z, y, mean, invstd, gamma, sums, count, want_g=False, dgamma=None, dbeta=None, count_dev=None,
                 mask_scale=None, mask_shift=None, g_into=None, bf16_only=False):
    """-> (dx, g).  g_into: an existing gradient buffer of y's shape that the masked gradient is ADDED to (returned as g).
    bf16_only (conv16): dx is written as a bf16 image only — the caller knows that its data and weight gradient both read
    that image; the returned dx is a memory-less fp32 handle (phantom_f32)."""
    n, c, h, w = y.shape
    z_ph, y_ph = is_phantom(z), is_phantom(y)
    only16 = bool(bf16_only and _CONV16 and _mode() == MATH_BF16 and y.is_cuda and c % 4 == 0)
    if g_into is not None:
        assert is_nhwc(g_into) and g_into.shape == y.shape
        amax_drop(g_into)             # added into through its pointer
        g = g_into
    else:
        g = empty_nhwc(n, c, h, w, y.device) if want_g else None
    dx, dx16 = _produced(n, c, h, w, y.device, not only16, only16 or image_wanted(c, n * h * w, y.device))
    mid = (mean, invstd, gamma, mask_scale, mask_shift, sums, float(count), count_dev)
    if z_ph or y_ph or dx16 is not None:
        _C.call("rr_bn_bwd_apply_b16", dz, *_operand(z, z_ph), *_operand(y, y_ph), *mid, dx, dx16, g, int(g_into is not None),
                dgamma, dbeta, y.numel(), c)
        return _published(dx, dx16), g
    if amax_wanted(c, n * h * w, y.device):
        # split-operand convolutions: dx is the operand of the data / weight gradient launched next — its maximum comes out
        # of this pass.  (dx is a fresh tensor that nothing adds into later: the remembered maximum cannot go stale.)
        word = _amax_word(y.device)
        _C.call("rr_bn_bwd_apply_amax", dz, z, y, *mid, dx, g, int(g_into is not None), dgamma, dbeta, y.numel(), c, word)
        return _published(dx, None, word), g
    _C.call("rr_bn_bwd_apply_gacc" if g_into is not None else "rr_bn_bwd_apply", dz, z, y, *mid, dx, g, dgamma, dbeta, y.numel(), c)
    return dx, g


def relu_fwd(x):
    out = torch.empty_like(x)
    assert out.stride() == x.stride()
    _C.call("rr_relu_fwd", x, out, x.numel())
    return out


def sum_n(grads, z=None):
    """(sum of same-layout tensors) * (z > 0 if z is given) in one pass."""
    import ctypes
    g0 = grads[0]
    for g in grads:
        assert g.shape == g0.shape and g.stride() == g0.stride() and g.is_cuda
    out = torch.empty_like(g0)
    assert out.stride() == g0.stride()
    arr = (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])
    _C.call("rr_sum_n", ctypes.cast(arr, ctypes.c_void_p), len(grads), z, out, g0.numel())
    return out


def bias_relu_bwd(dy, z, dbias):
    """dy NHWC-memory [*, c]; returns dy*(z>0) (or dy itself when z is None) and adds column sums to dbias."""
    c = dbias.numel()
    npix = dy.numel() // c
    masked = torch.empty_like(dy) if z is not None else None
    _C.call("rr_bias_relu_bwd", dy, z, masked, dbias, npix, c)
    return masked if z is not None else dy


def upsample_add_fwd(up1, low, bf16_only=False):
    """up1 + nearest-2x(low) (bilinear-align-corners resize for odd sizes).  Either operand may be a bf16-only activation;
    bf16_only: the sum is written as a bf16 image only (phantom_f32)."""
    n, c, h, w = up1.shape
    fast = (2 * low.shape[2] == h and 2 * low.shape[3] == w and c % 4 == 0 and up1.is_cuda)
    if fast and (bf16_only or is_phantom(up1) or is_phantom(low)):
        u_ph, l_ph = is_phantom(up1), is_phantom(low)
        out, out16 = _produced(n, c, h, w, up1.device, not bf16_only, bf16_only or image_wanted(c, n * h * w, up1.device))
        _C.call("rr_upsample2x_add_b16", *_operand(up1, u_ph), *_operand(low, l_ph), out, out16, n, h, w, c)
        return _published(out, out16)
    up1, low = f32_of(up1), f32_of(low)
    out = empty_nhwc(n, c, h, w, up1.device)
    _C.call("rr_upsample_add_fwd", up1, low, out, n, h, w, low.shape[2], low.shape[3], c)
    return out


def upsample_add_bwd(dout, low_shape):
    n, c, h, w = dout.shape
    dlow = empty_nhwc(n, c, low_shape[2], low_shape[3], dout.device)
    _C.call("rr_upsample_add_bwd", dout, dlow, n, h, w, low_shape[2], low_shape[3], c)
    return dlow


def resize_bilinear_ac(x, scale_factor):
    """F.interpolate(x, scale_factor=s, mode='bilinear', align_corners=True) on an NHWC tensor."""
    import math
    x = to_nhwc(x)
    n, c, h, w = x.shape
    oh, ow = int(math.floor(h * scale_factor)), int(math.floor(w * scale_factor))
    out = empty_nhwc(n, c, oh, ow, x.device)
    _C.call("rr_resize_bilinear_ac", x, out, n, h, w, oh, ow, c)
    return out


def avgpool_fwd(x):
    r, c, h, w = x.shape
    out = empty_nhwc(r, c, 1, 1, x.device)
    _C.call("rr_avgpool_fwd", x, out, r, h * w, c)
    return out


def bn_res_relu_avgpool(y, scale, shift, res):
    """[R,C,h,w] (NHWC) x2 -> [R,C,1,1]: mean_p relu(y*scale + shift + res), one pass (inference)."""
    assert is_nhwc(y) and is_nhwc(res) and y.shape == res.shape
    r, c, h, w = y.shape
    out = empty_nhwc(r, c, 1, 1, y.device)
    _C.call("rr_bn_res_relu_avgpool", y, scale, shift, res, out, r, h * w, c)
    return out


def conv1x1_bn_res_relu_avgpool(h, w, scale, shift, res):
    """h [R,K,ph,pw], w [N,K,1,1], res [R,N,ph,pw] (all NHWC) -> [R,N,1,1]: mean_p relu(conv1x1(h)*scale + shift + res),
    one kernel, the convolution's output stays in LDS (inference)."""
    assert is_nhwc(h) and is_nhwc(res) and is_nhwc(w)
    r, k, ph, pw = h.shape
    n = w.shape[0]
    assert tuple(w.shape[1:]) == (k, 1, 1) and tuple(res.shape) == (r, n, ph, pw)
    out = empty_nhwc(r, n, 1, 1, h.device)
    _C.call("rr_conv1x1_bn_res_relu_avgpool", h, w, scale, shift, res, out, r, ph * pw, k, n)
    return out


def avgpool_bwd(dout, shape):
    r, c, h, w = shape
    dx = empty_nhwc(r, c, h, w, dout.device)
    _C.call("rr_avgpool_bwd", dout, dx, r, h * w, c)
    return dx


def wh_shift_sum_fwd(t, bias_w, bias_h, k):
    n, c, h, w = t.shape
    assert c >= 2 * k and is_nhwc(t)
    out = empty_nhwc(n, 2, h, w, t.device)
    _C.call("rr_wh_shift_sum_fwd", t, bias_w, bias_h, out, n, h, w, k, c)
    return out


def wh_shift_sum_bwd(dout, k, ct):
    n, _, h, w = dout.shape
    dt = empty_nhwc(n, ct, h, w, dout.device)
    _C.call("rr_wh_shift_sum_bwd", dout, dt, n, h, w, k, ct)
    return dt


def adam_step(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, grad_scale=1.0):
    assert param.numel() % 4 == 0
    _C.call("rr_adam_step", param, grad, exp_avg, exp_avg_sq, param.numel(), float(lr), float(beta1), float(beta2), float(eps),
            int(step), float(grad_scale))


GUARD_CTL_WORDS = 20                # RR_GUARD_CTL_WORDS of include/rrnet_hip.h
GUARD_CTL_SLOTS = ("applied", "skipped", "clipped", "beta1_pow", "beta2_pow", "norm", "norm_max", "bad", "skip", "scale",
                   "step_size", "bc2_sqrt", "ema_d", "ema_omd", "reserved0", "reserved1", "b1", "omb1", "b2", "omb2")


def guard_ctl_fresh():
    """A fresh control record of the guarded step as a host float64 tensor: all zero, the two running products 1."""
    ctl = torch.zeros(GUARD_CTL_WORDS, dtype=torch.float64)
    ctl[3] = ctl[4] = 1.0
    return ctl


def grad_norm_blocks(n):
    """rr_grad_norm_blocks: the workgroups (= partial sums) of rr_grad_norm over n words; a function of n alone."""
    return int(_C.call("rr_grad_norm_blocks", int(n)))


def _flat_f32(what, name, t, n=None):
    if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 1 or (n is not None and t.numel() != n):
        raise _C.RRNetHipError("%s: %s must be a flat contiguous float32 tensor%s" % (what, name, "" if n is None else " of %d words" % n))


def grad_norm(grad, partial=None, bad=None):
    """rr_grad_norm on the current stream -> (partial float64 [blocks], bad int32 [blocks]): per workgroup the sum of
    squares of the finite words of `grad` and the count of its NaN / Inf words.  `partial` / `bad`: preallocated outputs."""
    _C.require_cuda(grad, partial, bad)
    _flat_f32("grad_norm", "grad", grad)
    n = grad.numel()
    if n % 4:
        raise _C.RRNetHipError("grad_norm: n = %d is not a multiple of 4 (pad the flat buffer)" % n)
    blocks = grad_norm_blocks(n)
    if partial is None:
        partial = torch.empty(blocks, dtype=torch.float64, device=grad.device)
    if bad is None:
        bad = torch.empty(blocks, dtype=torch.int32, device=grad.device)
    if partial.dtype != torch.float64 or not partial.is_contiguous() or partial.numel() != blocks or partial.device != grad.device:
        raise _C.RRNetHipError("grad_norm: partial must be a contiguous float64 [%d] tensor on %s" % (blocks, grad.device))
    if bad.dtype != torch.int32 or not bad.is_contiguous() or bad.numel() != blocks or bad.device != grad.device:
        raise _C.RRNetHipError("grad_norm: bad must be a contiguous int32 [%d] tensor on %s" % (blocks, grad.device))
    _C.call("rr_grad_norm", grad, n, partial, bad)
    return partial, bad


def _check_ctl(what, ctl, device):
    if ctl.dtype != torch.float64 or not ctl.is_contiguous() or ctl.numel() != GUARD_CTL_WORDS or ctl.device != device:
        raise _C.RRNetHipError("%s: ctl must be a contiguous float64 [%d] tensor on %s" % (what, GUARD_CTL_WORDS, device))


def guard_decide(partial, bad, ctl, grad_scale=1.0, max_norm=float("inf"), skip_nonfinite=False, lr=1e-3, beta1=0.9,
                 beta2=0.999, ema_decay=0.0, ema_warmup=False):
    """rr_guard_decide on the current stream: adds up what grad_norm left, decides skip / clip and advances the control
    record `ctl` (float64 [GUARD_CTL_WORDS] on the device, layout in include/rrnet_hip.h) in place.  Nothing is read back."""
    if partial.dtype != torch.float64 or not partial.is_contiguous() or bad.dtype != torch.int32 or not bad.is_contiguous() \
            or partial.numel() != bad.numel():
        raise _C.RRNetHipError("guard_decide: partial (float64) and bad (int32) must be contiguous and equally long")
    _check_ctl("guard_decide", ctl, partial.device)
    _C.call("rr_guard_decide", partial, bad, partial.numel(), float(grad_scale), float(max_norm), int(bool(skip_nonfinite)),
            float(lr), float(beta1), float(beta2), float(ema_decay), int(bool(ema_warmup)), ctl)
    return ctl


def adam_step_guarded(param, grad, exp_avg, exp_avg_sq, ema, eps, ctl):
    """rr_adam_step_guarded on the current stream: the fused Adam step with its constants read from `ctl`; does nothing when
    ctl says skip; `ema` (None: no averaged weights) is updated in the same pass."""
    _flat_f32("adam_step_guarded", "param", param)
    n = param.numel()
    if n % 4:
        raise _C.RRNetHipError("adam_step_guarded: n = %d is not a multiple of 4 (pad the flat buffer)" % n)
    for name, t in (("grad", grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq), ("ema", ema)):
        if t is not None:
            _flat_f32("adam_step_guarded", name, t, n)
    _check_ctl("adam_step_guarded", ctl, param.device)
    _C.call("rr_adam_step_guarded", param, grad, exp_avg, exp_avg_sq, ema, n, float(eps), ctl)


def state_snapshot(src, dst=None, chunk=65536, n=None, out=None):
    """rr_state_snapshot on the current stream: copies the fp32 words of `src` into `dst` (None: no copy) as bits and
    returns the digest, int64 [ceil(n / chunk), 3] holding the uint64 records (d0, d1, d2) of include/rrnet_hip.h.
    `n` defaults to src.numel(); `out`: a preallocated digest tensor of that shape (a checkpoint writer keeps one)."""
    _C.require_cuda(src, dst)
    if src.dtype != torch.float32 or not src.is_contiguous() or src.dim() != 1:
        raise _C.RRNetHipError("state_snapshot: src must be a flat contiguous float32 tensor")
    n = src.numel() if n is None else int(n)
    if n > src.numel():
        raise _C.RRNetHipError("state_snapshot: n = %d exceeds src (%d words)" % (n, src.numel()))
    if dst is not None and (dst.dtype != torch.float32 or not dst.is_contiguous() or dst.numel() < n):
        raise _C.RRNetHipError("state_snapshot: dst must be a contiguous float32 tensor of at least n words")
    chunk = int(chunk)
    nchunks = (n + chunk - 1) // chunk if n > 0 and chunk > 0 else 0
    if out is not None:
        if out.dtype != torch.int64 or not out.is_contiguous() or tuple(out.shape) != (nchunks, 3) or out.device != src.device:
            raise _C.RRNetHipError("state_snapshot: out must be a contiguous int64 [%d, 3] tensor on %s" % (nchunks, src.device))
    digest = out if out is not None and nchunks else \
        torch.empty((max(nchunks, 1), 3), dtype=torch.int64, device=src.device)        # never a NULL pointer, also for n == 0
    _C.call("rr_state_snapshot", src, dst, n, chunk, digest)
    return digest[:nchunks]


# ---------------------------------------------------------------------------------------------
# losses
# ---------------------------------------------------------------------------------------------
def focal_fwd(logits, gt):
    sums = torch.empty(3, dtype=torch.float64, device=logits.device)
    _C.call("rr_focal_loss_fwd", logits, gt, logits.numel(), sums)
    return sums


def focal_bwd(logits, gt, sums, gout, gscale=1.0):
    d = torch.empty_like(logits)
    assert d.stride() == logits.stride()
    _C.call("rr_focal_loss_bwd", logits, gt, logits.numel(), sums, gout, float(gscale), d)
    return d


def regl1_fwd(pred, mask, ind, target):
    b, c, h, w = pred.shape
    m = ind.shape[1]
    sums = torch.empty(3, dtype=torch.float64, device=pred.device)
    _C.call("rr_regl1_fwd", pred, mask, ind, target, b, m, c, h * w, sums)
    return sums


def regl1_bwd(pred, mask, ind, target, sums, gout, gscale=1.0):
    b, c, h, w = pred.shape
    m = ind.shape[1]
    d = empty_nhwc(b, c, h, w, pred.device)
    _C.call("rr_regl1_bwd", pred, mask, ind, target, b, m, c, h * w, sums, gout, float(gscale), d)
    return d


def stage2_loss(rois, reg, gt_xyxy, scale, want_droi=False):
    """rois [R,5], reg [R,4], gt [B,G,>=4] (xyxy) -> loss (double[3], [0] is the loss), dreg_unit [R,4], tgt, pos,
    npos, droi_unit [R,4] | None."""
    r = rois.shape[0]
    b, g, gs = gt_xyxy.shape
    dev = rois.device
    tgt = torch.empty((max(r, 1), 4), dtype=torch.float32, device=dev)
    pos = torch.zeros(max(r, 1), dtype=torch.int32, device=dev)
    npos = torch.empty(b, dtype=torch.int32, device=dev)
    loss = torch.empty(3, dtype=torch.float64, device=dev)
    dreg = torch.zeros((r, 4), dtype=torch.float32, device=dev)
    droi = torch.zeros((r, 4), dtype=torch.float32, device=dev) if want_droi else None
    _C.call("rr_stage2_loss", rois, reg, r, gt_xyxy, b, g, gs, float(scale), tgt, pos, npos, loss, dreg, droi)
    return loss, dreg, tgt[:r], pos[:r], npos, droi


# ---------------------------------------------------------------------------------------------
# decode / NMS / RoIAlign
# ---------------------------------------------------------------------------------------------
def decode_topk(hm, wh, off, k, is_logits=True, want_pix=False, peak_filter=False, spread=True, box_mode=0, scale=1.0):
    """spread=False keeps the whole decode in one workgroup per frame (no workspace): the A/B of the two paths.
    box_mode 0: RRNet rows x1,y1,x2,y2,score,cls (feature coordinates, wh clamped at 0); 1: CenterNet rows
    (x,y,w,h)*scale,score,cls+1 (no clamp)."""
    assert is_nhwc(hm) and is_nhwc(wh) and is_nhwc(off)
    b, c, h, w = hm.shape
    out = torch.empty((b, k, 6), dtype=torch.float32, device=hm.device)
    pix = torch.empty((b, k), dtype=torch.int32, device=hm.device) if want_pix else None
    ws, ws_bytes = None, 0
    if spread and h * w * c >= 65536:
        ws_bytes = _C.call("rr_decode_workspace_bytes", b)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=hm.device)
    _C.call("rr_decode_topk", hm, int(is_logits), int(peak_filter), wh, off, b, h, w, c, k, int(box_mode), float(scale), out, pix,
            ws, ws_bytes)
    return (out, pix) if want_pix else out


def roi_provenance(rois, scores, clses, decoded, pix):
    r = rois.shape[0]
    roi_pix = torch.full((max(r, 1),), -1, dtype=torch.int32, device=rois.device)
    _C.call("rr_roi_provenance", rois, scores, clses, r, decoded, pix, decoded.shape[1], roi_pix)
    return roi_pix[:r]


def proposal_bwd(droi, rois, roi_pix, wh):
    b, _, h, w = wh.shape
    dwh, doff = empty_nhwc(b, 2, h, w, wh.device), empty_nhwc(b, 2, h, w, wh.device)
    _C.call("rr_proposal_bwd", droi, rois, roi_pix, rois.shape[0], wh, b, h, w, dwh, doff)
    return dwh, doff


def peak3x3(hm, is_logits=True):
    """`_ctnet_nms` score map: sigmoid(hm) (or hm itself when is_logits=False) where it equals its 3x3 maximum, else 0."""
    b, c, h, w = hm.shape
    out = empty_nhwc(b, c, h, w, hm.device)
    _C.call("rr_peak3x3", hm, int(is_logits), out, b, h, w, c)
    return out


def group_by_class(boxes, num_classes, cls_base=0):
    """boxes [B,K,6] -> grouped [B,K,6], seg_off int32 [B*num_classes+1], seg_len int32 [B*num_classes].
    Rows whose class lies outside [cls_base, cls_base+num_classes) are dropped (a gap of uninitialised rows at the
    end of the image's block): hand seg_len, not offset differences, to the NMS entries."""
    b, k, _ = boxes.shape
    grouped = torch.empty_like(boxes)
    seg_off = torch.empty(b * num_classes + 1, dtype=torch.int32, device=boxes.device)
    seg_len = torch.empty(b * num_classes, dtype=torch.int32, device=boxes.device)
    _C.call("rr_group_by_class", boxes, b, k, num_classes, cls_base, grouped, seg_off, seg_len)
    return grouped, seg_off, seg_len


def hard_nms_segments(boxes6, seg_off, max_seg, thresh, seg_len=None):
    nseg = seg_off.numel() - 1
    n_out = torch.zeros(nseg, dtype=torch.int32, device=boxes6.device)
    _C.call("rr_hard_nms_segments", boxes6, seg_off, seg_len, nseg, int(max_seg), float(thresh), n_out)
    return n_out


WBF_CONF_TYPES = {"avg": 0, "max": 1}


def wbf_plan(nseg, max_seg):
    """rr_wbf_plan -> list of RR_WBF_PLAN_INTS ints (include/rrnet_hip.h); a bound the kernel refuses raises RRNetHipError."""
    import ctypes
    buf = (ctypes.c_int * 32)()
    _C.call("rr_wbf_plan", int(nseg), int(max_seg), buf, 32)
    return list(buf)


def wbf_segments(rows, seg_off, max_seg, iou_thr, conf_type, weight_sum, seg_len=None, out=None):
    """rr_wbf_segments: weighted boxes fusion of score-sorted segments.  rows [R,6] float32 x1,y1,x2,y2,score,cls,
    seg_off int32 [nseg+1] (seg_len int32 [nseg] where the offsets leave gaps) -> (out [R,6], members int32 [R],
    n_out int32 [nseg]): segment s's clusters are out[seg_off[s] : seg_off[s]+n_out[s]], rows beyond are not written.
    conf_type 0 / "avg" or 1 / "max".  `out`: a caller's [R,6] buffer to write into."""
    _C.require_cuda(rows, seg_off, seg_len, out)
    if rows.dtype != torch.float32 or rows.dim() != 2 or rows.shape[1] != 6 or not rows.is_contiguous():
        raise ValueError("wbf_segments: rows must be contiguous float32 [R,6], got %s %s" % (rows.dtype, tuple(rows.shape)))
    if seg_off.dtype != torch.int32 or (seg_len is not None and seg_len.dtype != torch.int32):
        raise ValueError("wbf_segments: seg_off and seg_len must be int32")
    conf_type = WBF_CONF_TYPES.get(conf_type, conf_type)
    nseg = seg_off.numel() - 1
    if seg_len is not None and seg_len.numel() != nseg:
        raise ValueError("wbf_segments: seg_len has %d entries for %d segments" % (seg_len.numel(), nseg))
    dev = rows.device
    if out is None:
        out = torch.empty_like(rows)
    elif out.shape != rows.shape or out.dtype != torch.float32 or not out.is_contiguous() or out.data_ptr() == rows.data_ptr():
        raise ValueError("wbf_segments: out must be another contiguous float32 tensor of rows' shape")
    members = torch.zeros(rows.shape[0], dtype=torch.int32, device=dev)
    n_out = torch.zeros(max(nseg, 0), dtype=torch.int32, device=dev)
    nbytes = _C.call("rr_wbf_workspace_bytes", nseg, int(max_seg))
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
    _C.call("rr_wbf_segments", rows, seg_off, seg_len, nseg, int(max_seg), float(iou_thr), int(conf_type), float(weight_sum), out,
            members, n_out, ws, nbytes)
    return out, members, n_out


TEXT_LAYOUTS = {"rrnet": 0, "centernet": 1, "retinanet": 2}
TEXT_LINE_FLAGGED, TEXT_LINE_SURPLUS = 1, 2
TEXT_MAX_ROW = 165                                    # RR_TEXT_MAX_ROW


def _exclusive_sum(counts):
    off = torch.zeros(counts.numel() + 1, dtype=torch.int64, device=counts.device)
    torch.cumsum(counts, 0, dtype=torch.int64, out=off[1:])
    return off


def text_lines(text, file_off):
    """rr_text_line_counts + rr_text_lines: text uint8 [N] (files back to back, each non-empty one ending in '\\n'), file_off
    int64 [F+1] -> (line_pos int64 [L], file_line_off int64 [F+1]).  One host sync to learn L."""
    _C.require_cuda(text, file_off)
    if text.dtype != torch.uint8 or text.dim() != 1 or file_off.dtype != torch.int64 or file_off.numel() < 1:
        raise ValueError("text_lines: text must be uint8 [N] and file_off int64 [F+1]")
    if not file_off.is_contiguous():
        raise ValueError("text_lines: file_off must be contiguous")
    n, dev = text.numel(), text.device
    nblocks = _C.call("rr_text_line_blocks", n)
    counts = torch.empty(nblocks, dtype=torch.int32, device=dev)
    _C.call("rr_text_line_counts", text, n, counts)
    block_off = _exclusive_sum(counts)
    nlines = int(block_off[-1].item())
    line_pos = torch.empty(nlines, dtype=torch.int64, device=dev)
    file_line_off = torch.empty(file_off.numel(), dtype=torch.int64, device=dev)
    _C.call("rr_text_lines", text, n, file_off, file_off.numel() - 1, block_off, nlines, line_pos, file_line_off)
    return line_pos, file_line_off


def text_parse(text, line_pos, ncol=8):
    """rr_text_parse: -> (rows float64 [L,ncol], line_flag int32 [L]: 0, TEXT_LINE_SURPLUS or TEXT_LINE_FLAGGED)."""
    _C.require_cuda(text, line_pos)
    if text.dtype != torch.uint8 or line_pos.dtype != torch.int64 or not line_pos.is_contiguous():
        raise ValueError("text_parse: text must be uint8 and line_pos contiguous int64")
    nlines, dev = line_pos.numel(), text.device
    rows = torch.empty((nlines, ncol), dtype=torch.float64, device=dev)
    flags = torch.empty(nlines, dtype=torch.int32, device=dev)
    _C.call("rr_text_parse", text, text.numel(), line_pos, nlines, int(ncol), rows, flags)
    return rows, flags


def _check_rows6(who, rows6):
    if rows6.dtype != torch.float32 or rows6.dim() != 2 or rows6.shape[1] != 6 or not rows6.is_contiguous():
        raise ValueError("%s: rows must be contiguous float32 [R,6], got %s %s" % (who, rows6.dtype, tuple(rows6.shape)))


def text_format_len(rows6, layout, clamp):
    """rr_text_format_len: -> (len int32 [R], row_flag int32 [R], byte_off int64 [R+1] = the exclusive sum of len)."""
    _C.require_cuda(rows6)
    _check_rows6("text_format_len", rows6)
    r, dev = rows6.shape[0], rows6.device
    length = torch.empty(r, dtype=torch.int32, device=dev)
    flag = torch.empty(r, dtype=torch.int32, device=dev)
    _C.call("rr_text_format_len", rows6, r, int(TEXT_LAYOUTS.get(layout, layout)), int(bool(clamp)), length, flag)
    return length, flag, _exclusive_sum(length)


def text_format(rows6, layout, clamp, byte_off, out):
    """rr_text_format: writes row r to out[byte_off[r] : byte_off[r+1]] (uint8 device buffer) and returns out."""
    _check_rows6("text_format", rows6)
    if byte_off.dtype != torch.int64 or byte_off.numel() != rows6.shape[0] + 1 or not byte_off.is_contiguous():
        raise ValueError("text_format: byte_off must be contiguous int64 [R+1]")
    if out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("text_format: out must be a contiguous uint8 buffer")
    _C.call("rr_text_format", rows6, rows6.shape[0], int(TEXT_LAYOUTS.get(layout, layout)), int(bool(clamp)), byte_off, out,
            out.numel())
    return out


def _np_ptr(a):
    return _C.c_void_p(a.ctypes.data)


def text_parse_host(text, file_off, ncol=8):
    """The codec's host loops (rr_text_lines_host + rr_text_parse_host) on numpy buffers, no device: text uint8 [N], file_off
    int64 [F+1] -> (rows float64 [L,ncol], line_flag int32 [L], line_pos int64 [L], file_line_off int64 [F+1])."""
    import ctypes
    import numpy as np
    text = np.ascontiguousarray(text, np.uint8)
    file_off = np.ascontiguousarray(file_off, np.int64)
    nfiles = file_off.size - 1
    file_line_off = np.zeros(nfiles + 1, np.int64)
    nlines = ctypes.c_long(0)
    _C.call("rr_text_lines_host", _np_ptr(text), text.size, _np_ptr(file_off), nfiles, 0, None, _np_ptr(file_line_off), ctypes.byref(nlines))
    line_pos = np.zeros(nlines.value, np.int64)
    _C.call("rr_text_lines_host", _np_ptr(text), text.size, _np_ptr(file_off), nfiles, line_pos.size, _np_ptr(line_pos),
            _np_ptr(file_line_off), ctypes.byref(nlines))
    rows = np.zeros((line_pos.size, ncol), np.float64)
    flags = np.zeros(line_pos.size, np.int32)
    _C.call("rr_text_parse_host", _np_ptr(text), text.size, _np_ptr(line_pos), line_pos.size, int(ncol), _np_ptr(rows),
            _np_ptr(flags))
    return rows, flags, line_pos, file_line_off


def text_format_host(rows6, layout, clamp, pad=0, fill=0):
    """The codec's host loop (rr_text_format_host) on a numpy [R,6] float32 array, no device -> (out uint8 [total + pad],
    byte_off int64 [R+1], row_flag int32 [R]); `pad` bytes of `fill` follow the text (the tests look at them)."""
    import numpy as np
    rows6 = np.ascontiguousarray(rows6, np.float32).reshape(-1, 6)
    layout = int(TEXT_LAYOUTS.get(layout, layout))
    r = rows6.shape[0]
    length, flag = np.zeros(r, np.int32), np.zeros(r, np.int32)
    _C.call("rr_text_format_host", _np_ptr(rows6), r, layout, int(bool(clamp)), _np_ptr(length), _np_ptr(flag), None, None, 0)
    byte_off = np.zeros(r + 1, np.int64)
    np.cumsum(length, out=byte_off[1:])
    out = np.full(int(byte_off[-1]) + pad, fill, np.uint8)
    _C.call("rr_text_format_host", _np_ptr(rows6), r, layout, int(bool(clamp)), None, None, _np_ptr(byte_off), _np_ptr(out),
            int(byte_off[-1]))
    return out, byte_off, flag


def seg_prefix(n_out):
    """Exclusive prefix of per-segment counts -> int32 [nseg+1] (last entry = total)."""
    nseg = n_out.numel()
    out_off = torch.empty(nseg + 1, dtype=torch.int32, device=n_out.device)
    _C.call("rr_pack_segments", None, None, n_out, nseg, 1, out_off, None, None, None, None, 0)
    return out_off


def pack_segments(grouped, seg_off, n_out, segs_per_image, want_rois=True, want_rows=False, want_offsets=False):
    """-> (rois [R,5], scores [R], clses [R]) and/or rows [R,6]; one host sync to learn R."""
    nseg = n_out.numel()
    dev = grouped.device
    out_off = seg_prefix(n_out)
    import time as _time
    t0 = _time.perf_counter()
    r = int(out_off[-1].item())              # the step's one device -> host read: the RoI count sizes the head's tensors
    global SYNC_WAIT_S
    SYNC_WAIT_S += _time.perf_counter() - t0
    rois = torch.empty((r, 5), dtype=torch.float32, device=dev) if want_rois else None
    scores = torch.empty(r, dtype=torch.float32, device=dev) if want_rois else None
    clses = torch.empty(r, dtype=torch.float32, device=dev) if want_rois else None
    rows = torch.empty((r, 6), dtype=torch.float32, device=dev) if want_rows else None
    _C.call("rr_pack_segments", grouped, seg_off, n_out, nseg, segs_per_image, out_off, rois, scores, clses, rows, 1)
    if want_offsets:
        return rois, scores, clses, rows, out_off
    return rois, scores, clses, rows


def ctnet_targets(annos, counts, img_h, img_w, scale_factor=4, num_classes=10):
    """annos [B,M,>=6] cuda float32 (padded), counts [B] cuda int32 -> hm (logical [B,C,Hf,Wf], NHWC memory),
    wh [B,M,2], ind [B,M,1], offset [B,M,2], reg_mask [B,M,1]  (collate_fn_ctnet contract)."""
    _C.require_cuda(annos, counts)
    assert annos.is_contiguous()
    b, m, st = annos.shape
    hf, wf = img_h // scale_factor, img_w // scale_factor
    dev = annos.device
    hm = empty_nhwc(b, num_classes, hf, wf, dev)
    wh = torch.empty((b, m, 2), dtype=torch.float32, device=dev)
    ind = torch.empty((b, m, 1), dtype=torch.float32, device=dev)
    off = torch.empty((b, m, 2), dtype=torch.float32, device=dev)
    mask = torch.empty((b, m, 1), dtype=torch.float32, device=dev)
    _C.call("rr_ctnet_targets", annos, counts, b, m, st, img_h, img_w, scale_factor, num_classes, hm, wh, ind, off, mask)
    return hm, wh, ind, off, mask


AUGMENT_PARAMS = 16        # RR_AUGMENT_PARAMS: int32 words of rr_augment_frames' per-image record


def _jitter_args(jitter, b):
    """jitter: None or (factors float32 [B,3], gray_mean int32 [B]) -> the two extra arguments of a _jitter entry."""
    if jitter is None:
        return ()
    factors, gray_mean = jitter
    assert factors.is_contiguous() and factors.shape == (b, 3)
    assert gray_mean.is_contiguous() and gray_mean.numel() == b
    return (factors, gray_mean)


def augment_frames(src, params, rects, rect_off, taps, mean, std, out_h, out_w, jitter=None):
    """rr_augment_frames: packed uint8 source windows + per-image records -> the normalised network input, logical
    [B,3,out_h,out_w] in NHWC memory.  src uint8 [bytes], params int32 [B,16], rects int32 [R,4] (None or empty: no
    ignore region), rect_off int32 [B+1], taps int32 [T,3], mean / std float32 [3]; all on the device.  The records
    are built (and checked against the window and table sizes) by rrnet_amd.datasets.augment.pack_batch.  `jitter`
    (factors, gray_mean) selects rr_augment_frames_jitter: see augment_frames_jitter."""
    _C.require_cuda(src, params, rects, rect_off, taps, mean, std)
    assert src.is_contiguous() and src.dim() == 1
    assert params.is_contiguous() and params.shape[1] == AUGMENT_PARAMS
    assert rect_off.numel() == params.shape[0] + 1
    assert taps.is_contiguous() and taps.shape[1] == 3
    assert mean.numel() == 3 and std.numel() == 3
    if rects is not None and rects.numel() == 0:
        rects = None
    assert rects is None or (rects.is_contiguous() and rects.shape[1] == 4)
    b = params.shape[0]
    out = empty_nhwc(b, 3, out_h, out_w, src.device)
    _C.call("rr_augment_frames_jitter" if jitter is not None else "rr_augment_frames", src, src.numel(), params, rects, rect_off,
            taps, taps.shape[0], mean, std, *_jitter_args(jitter, b), out, b, out_h, out_w)
    return out


PASTE_WORDS = 12           # RR_PASTE_WORDS: int32 words of one row of a paste table


def paste_workspace(b, canvas_pix, scratch_pix, device):
    """(canvas [b, canvas_pix rounded up to 4, 3], scratch [b, scratch_pix, 3]) for augment_frames_pasted."""
    return (torch.empty((b, (max(int(canvas_pix), 1) + 3) // 4 * 4, 3), dtype=torch.float32, device=device),
            torch.empty((b, max(int(scratch_pix), 1), 3), dtype=torch.float32, device=device))


def augment_frames_pasted(src, params, rects, rect_off, taps, pastes, paste_off, mean, std, out_h, out_w,
                          canvas_pix=None, scratch_pix=None, stages=7, work=None, jitter=None):
    """rr_augment_frames_pasted: rr_augment_frames with FillDuck's ordered pastes between the ignore step and the flip.
    Arguments as augment_frames, plus pastes int32 [K,12] (None or empty: none) and paste_off int32 [B+1]; a frame with
    pastes ships its whole source frame as its window.  canvas_pix / scratch_pix: the largest scaled frame (dst_h*dst_w)
    and the largest pasted object (out_h*out_w) of the batch in pixels; left None they are read back from the device
    records (a synchronisation the loader avoids by passing them).  The canvas and the scratch come from the caching
    allocator, which hands the same blocks back batch after batch.  `stages` / `work` (a paste_workspace kept between
    calls) exist for timing one stage.  `jitter` (factors, gray_mean) selects rr_augment_frames_pasted_jitter: see
    augment_frames_pasted_jitter.  -> [B,3,out_h,out_w] in NHWC memory."""
    _C.require_cuda(src, params, rects, rect_off, taps, pastes, paste_off, mean, std)
    assert src.is_contiguous() and src.dim() == 1
    assert params.is_contiguous() and params.shape[1] == AUGMENT_PARAMS
    b = params.shape[0]
    assert rect_off.numel() == b + 1
    assert paste_off.numel() == b + 1 and paste_off.is_contiguous()
    assert taps.is_contiguous() and taps.shape[1] == 3
    assert mean.numel() == 3 and std.numel() == 3
    if rects is not None and rects.numel() == 0:
        rects = None
    assert rects is None or (rects.is_contiguous() and rects.shape[1] == 4)
    if pastes is None or pastes.numel() == 0:
        pastes = torch.zeros((1, PASTE_WORDS), dtype=torch.int32, device=src.device)
    assert pastes.is_contiguous() and pastes.shape[1] == PASTE_WORDS
    if work is None and canvas_pix is None:
        host = params.cpu()
        canvas_pix = int((host[:, 6].long() * host[:, 7].long()).max())
    if work is None and scratch_pix is None:
        host = pastes.cpu()
        scratch_pix = int((host[:, 6].long() * host[:, 7].long()).max())
    canvas, scratch = work if work is not None else paste_workspace(b, canvas_pix, scratch_pix, src.device)
    canvas_pix, scratch_pix = canvas.shape[1], scratch.shape[1]
    assert canvas.shape == (b, canvas_pix, 3) and scratch.shape == (b, scratch_pix, 3) and canvas_pix % 4 == 0
    assert canvas.is_contiguous() and scratch.is_contiguous()
    out = empty_nhwc(b, 3, out_h, out_w, src.device)
    _C.call("rr_augment_frames_pasted_jitter" if jitter is not None else "rr_augment_frames_pasted", src, src.numel(), params, rects,
            rect_off, taps, taps.shape[0], pastes, paste_off, mean, std, *_jitter_args(jitter, b), canvas, canvas_pix, scratch,
            scratch_pix, out, b, out_h, out_w, int(stages))
    return out


def jitter_workspace(b, device):
    """(sums int64 [b], gray_mean int32 [b]) for jitter_gray_mean."""
    return (torch.empty(b, dtype=torch.int64, device=device), torch.empty(b, dtype=torch.int32, device=device))


def jitter_gray_mean(src, params, factors, max_pixels=None, work=None):
    """rr_jitter_gray_mean: ColorJitter's one whole-frame quantity.  src, params as augment_frames, every frame shipped
    WHOLE (rrnet_amd.datasets.augment.pack_batch / pack_jitter check that on the host records); factors float32 [B,3] =
    brightness, contrast, saturation per frame.  max_pixels: the largest frame of the batch in pixels; left None it is
    read back from the device records (a synchronisation the loader avoids by passing it).  -> (gray_mean int32 [B] =
    int(mean(L) + 0.5) of each brightness-adjusted frame, sums int64 [B] = the integer sums of L)."""
    _C.require_cuda(src, params, factors)
    assert src.is_contiguous() and src.dim() == 1
    assert params.is_contiguous() and params.shape[1] == AUGMENT_PARAMS
    b = params.shape[0]
    assert factors.is_contiguous() and factors.shape == (b, 3)
    if max_pixels is None:
        host = params.cpu()
        max_pixels = int((host[:, 4].long() * host[:, 5].long()).max())
    sums, gray = work if work is not None else jitter_workspace(b, src.device)
    assert sums.numel() == b and gray.numel() == b
    _C.call("rr_jitter_gray_mean", src, src.numel(), params, factors, sums, gray, b, int(max_pixels))
    return gray, sums


def augment_frames_jitter(src, params, rects, rect_off, taps, factors, gray_mean, mean, std, out_h, out_w):
    """rr_augment_frames_jitter: augment_frames with ColorJitter applied to the source taps.  factors float32 [B,3],
    gray_mean int32 [B] from jitter_gray_mean on the same src / params / factors; every frame shipped whole."""
    return augment_frames(src, params, rects, rect_off, taps, mean, std, out_h, out_w, jitter=(factors, gray_mean))


def augment_frames_pasted_jitter(src, params, rects, rect_off, taps, pastes, paste_off, factors, gray_mean, mean, std,
                                 out_h, out_w, **kw):
    """rr_augment_frames_pasted_jitter: augment_frames_pasted on the colour-jittered frame (the canvas stage jitters the
    source taps; pasted objects read the jittered canvas).  factors, gray_mean as augment_frames_jitter; everything
    else, keywords included, as augment_frames_pasted."""
    return augment_frames_pasted(src, params, rects, rect_off, taps, pastes, paste_off, mean, std, out_h, out_w,
                                 jitter=(factors, gray_mean), **kw)


def refine_boxes(rois, reg, scores, clses, seg_off, scale, score_thr):
    """generate_bbox + score filter + xywh->xyxy for every (frame, class) segment of the packed RoI list.
    -> boxes6 [R,6] (kept rows at the front of each segment's range), seg_len int32 [nseg]."""
    _C.require_cuda(rois, reg, scores, clses, seg_off)
    r = rois.shape[0]
    nseg = seg_off.numel() - 1
    out6 = torch.empty((r, 6), dtype=torch.float32, device=rois.device)
    seg_len = torch.zeros(max(nseg, 0), dtype=torch.int32, device=rois.device)
    _C.call("rr_refine_boxes", rois, reg.contiguous(), scores, clses, seg_off, nseg, float(scale), float(score_thr), out6, seg_len)
    return out6, seg_len


def finalize_frames(boxes6, seg_off, n_out, nframes, segs_per_frame, max_frame_boxes):
    """Per frame: concatenate kept segment rows, xyxy->xywh, sort by score descending.
    -> out6 [R,6] (R = upper bound rows; frame f occupies rows [frame_off[f], frame_off[f+1])), frame_off int32
    [nframes+1] (device)."""
    out_off = seg_prefix(n_out)
    out6 = torch.empty_like(boxes6)
    _C.call("rr_finalize_frames", boxes6, seg_off, n_out, out_off, nframes, segs_per_frame, int(max_frame_boxes), out6)
    return out6, out_off[::segs_per_frame]


def sort_rows_by_score(rows6):
    """[n,6] device rows -> a new tensor ordered by score descending (ties keep their input order)."""
    rows6 = rows6.contiguous()
    out = torch.empty_like(rows6)
    _C.call("rr_sort_rows_by_score", rows6, rows6.shape[0], out)
    return out


DETECT_MAX_ROWS = 16384       # RR_DETECT_MAX_ROWS: merged rows of one frame the LDS sort holds


def _prepare_frames(symbol, copies, frames_u8, mean, std, scale_factor):
    """The body of prepare_frames (copies = 1) and prepare_frames_pair (copies = 2): `copies` output images per frame."""
    import math
    _C.require_cuda(frames_u8, mean, std)
    assert frames_u8.is_contiguous() and frames_u8.dim() == 4 and frames_u8.shape[3] == 3
    assert mean.numel() == 3 and std.numel() == 3
    assert mean.is_contiguous() and std.is_contiguous()
    b, h, w, _ = frames_u8.shape
    oh, ow = int(math.floor(h * scale_factor)), int(math.floor(w * scale_factor))
    out = empty_nhwc(copies * b, 3, oh, ow, frames_u8.device)
    _C.call(symbol, frames_u8, mean, std, out, b, h, w, oh, ow)
    return out


def prepare_frames(frames_u8, mean, std, scale_factor):
    """rr_prepare_frames: frames uint8 [B,H,W,3] (RGB) -> ToTensor -> Normalize -> F.interpolate(scale_factor, bilinear,
    align_corners=True) -> logical [B,3,floor(H*s),floor(W*s)] float32 in NHWC memory.  mean / std float32 [3] on the
    device.  Same bits as resize_bilinear_ac on the host-normalised frame."""
    return _prepare_frames("rr_prepare_frames", 1, frames_u8, mean, std, scale_factor)


def merge_buffers(nframes, k, device):
    """(merged [nframes,k,6] with every class -1, count int32 [nframes] zeros): the state rr_merge_scales appends to."""
    if not 0 < k <= DETECT_MAX_ROWS:
        raise ValueError("merge_buffers: %d rows per frame (limit %d)" % (k, DETECT_MAX_ROWS))
    merged = torch.full((nframes, k, 6), -1.0, dtype=torch.float32, device=device)
    return merged, torch.zeros(nframes, dtype=torch.int32, device=device)


def merge_scales(rois, reg, scores, clses, frame_off, div, merged, count, scale=4, score_thr=None):
    """rr_merge_scales: one scale's stage-2 inputs (rois [R,5], reg [R,4], scores / clses [R]; frame_off int32 [B+1] row
    ranges) -> generate_bbox rows (x,y,w,h,score,cls+1), kept when score_thr is None or score > score_thr, x,y,w,h / div
    (IEEE), appended to merged [B,K,6] at count [B] (both updated in place, see merge_buffers)."""
    r = rois.shape[0]
    b, k, six = merged.shape
    assert six == 6 and merged.is_contiguous() and 0 < k <= DETECT_MAX_ROWS
    assert count.numel() == b and count.is_contiguous()
    assert frame_off.numel() == b + 1 and frame_off.is_contiguous()
    assert rois.is_contiguous() and tuple(rois.shape) == (r, 5)
    assert tuple(reg.shape) == (r, 4)
    assert scores.is_contiguous() and scores.numel() == r
    assert clses.is_contiguous() and clses.numel() == r
    _C.call("rr_merge_scales", rois, reg.contiguous(), scores, clses, frame_off, b, r, float(scale), float(div),
            int(score_thr is not None), float(score_thr if score_thr is not None else 0.0), merged, count, k)


def prepare_frames_pair(frames_u8, mean, std, scale_factor):
    """rr_prepare_frames_pair: prepare_frames into logical [2B,3,oh,ow] (NHWC memory): images 0..B-1 are prepare_frames'
    output, images B..2B-1 the same pixels mirrored in x (`flip_img` after the resize: the bits of the plain image)."""
    return _prepare_frames("rr_prepare_frames_pair", 2, frames_u8, mean, std, scale_factor)


def merge_ctnet(rows, nframes, img_w, div, merged, count, pair=True, score_thr=0.01):
    """rr_merge_ctnet: one scale's CenterNet rows [(2 if pair else 1)*nframes, k_in, 6] (decode_topk, box_mode=1) -> per
    frame the flipped image's rows (image nframes+f, x <- (img_w - x) - w) then the plain image's, kept when score >
    score_thr, x,y,w,h / div (IEEE), appended to merged [nframes,K,6] at count [nframes] (in place, see merge_buffers)."""
    b, k, six = merged.shape
    assert b == nframes and six == 6 and merged.is_contiguous() and 0 < k <= DETECT_MAX_ROWS
    assert count.numel() == b and count.is_contiguous()
    assert rows.is_contiguous() and rows.dim() == 3 and rows.shape[2] == 6
    assert rows.shape[0] == (2 if pair else 1) * nframes
    _C.call("rr_merge_ctnet", rows, nframes, rows.shape[1], int(bool(pair)), float(img_w), float(div), float(score_thr), merged,
            count, k)


def check_tiles(tiles, sizes, tile):
    """The host's check of a tile table before it is uploaded.  tiles: T rows (frame, y0, x0); sizes: (H, W) of every frame;
    tile = (th, tw).  Every tile must name a frame and lie inside it, and the rows must be sorted by frame (a frame's tiles
    back to back, which is what rr_merge_tiles' ranges need).
    -> (table int32 [T,3] numpy, tile_off int32 [F+1] numpy); ValueError naming the first offending row."""
    import numpy as np
    table = np.ascontiguousarray(np.asarray(tiles, dtype=np.int64).reshape(-1, 3))
    th, tw = int(tile[0]), int(tile[1])
    if th <= 0 or tw <= 0:
        raise ValueError("tiles: tile %dx%d" % (th, tw))
    nframes = len(sizes)
    per_frame = [0] * nframes
    last = 0
    for t, (f, y0, x0) in enumerate(table.tolist()):
        if not 0 <= f < nframes:
            raise ValueError("tiles: row %d names frame %d of %d" % (t, f, nframes))
        h, w = int(sizes[f][0]), int(sizes[f][1])
        if y0 < 0 or x0 < 0 or y0 + th > h or x0 + tw > w:
            raise ValueError("tiles: row %d: tile %dx%d at (%d, %d) leaves frame %d (%dx%d)" % (t, th, tw, y0, x0, f, h, w))
        if f < last:
            raise ValueError("tiles: row %d: frame %d after frame %d (rows must be sorted by frame)" % (t, f, last))
        last = f
        per_frame[f] += 1
    tile_off = np.concatenate([[0], np.cumsum(per_frame)]).astype(np.int32)
    return table.astype(np.int32), tile_off


def _frame_sizes(frames):
    if torch.is_tensor(frames):
        if frames.dim() != 4 or frames.shape[3] != 3:
            raise ValueError("tiles: frames must be [B,H,W,3] or a list of [H,W,3], got %s" % (tuple(frames.shape),))
        return [(int(frames.shape[1]), int(frames.shape[2]))] * int(frames.shape[0])
    sizes = []
    for i, fr in enumerate(frames):
        if not torch.is_tensor(fr) or fr.dim() != 3 or fr.shape[2] != 3:
            raise ValueError("tiles: frame %d must be a [H,W,3] tensor" % i)
        sizes.append((int(fr.shape[0]), int(fr.shape[1])))
    return sizes


def prepare_tiles(frames, tiles, tile, zoom, mean, std, out=None):
    """rr_prepare_tiles: T equal-size tiles cut out of F frames of any sizes -> ToTensor -> Normalize -> bilinear resize
    (align_corners=True) by `zoom`, one launch.  frames: a list of uint8 [H_i,W_i,3] device tensors (packed here into one
    byte buffer) or one uint8 [B,H,W,3] tensor; tiles: T host rows (frame, y0, x0), checked by check_tiles; tile = (th, tw).
    -> logical [T,3,floor(th*zoom),floor(tw*zoom)] float32 in NHWC memory; tile t carries the bits prepare_frames gives for
    frames[f][y0:y0+th, x0:x0+tw] at that factor.  out (optional): the NHWC buffer to write into."""
    import math
    import numpy as np
    sizes = _frame_sizes(frames)
    if not sizes:
        raise ValueError("prepare_tiles: no frames")
    th, tw = int(tile[0]), int(tile[1])
    table, _ = check_tiles(tiles, sizes, (th, tw))
    if torch.is_tensor(frames):
        packed = frames.contiguous()
    else:
        packed = torch.cat([fr.contiguous().view(-1) for fr in frames]) if len(frames) > 1 else frames[0].contiguous()
    _C.require_cuda(packed, mean, std, out)
    assert mean.numel() == 3 and std.numel() == 3
    assert mean.is_contiguous() and std.is_contiguous()
    oh, ow = int(math.floor(th * zoom)), int(math.floor(tw * zoom))
    if oh <= 0 or ow <= 0:
        raise ValueError("prepare_tiles: tile %dx%d at zoom %g is empty" % (th, tw, zoom))
    t = table.shape[0]
    dev = packed.device
    if out is None:
        out = empty_nhwc(t, 3, oh, ow, dev)
    assert tuple(out.shape) == (t, 3, oh, ow) and out.dtype == torch.float32 and (t == 0 or is_nhwc(out))
    if t == 0:
        return out
    base = np.concatenate([[0], np.cumsum([h * w * 3 for h, w in sizes])[:-1]]).astype(np.int64)
    frame_base = torch.from_numpy(base).to(dev)
    frame_hw = torch.tensor(sizes, dtype=torch.int32).to(dev)
    tiles_dev = torch.from_numpy(table).to(dev)
    _C.call("rr_prepare_tiles", packed, frame_base, frame_hw, len(sizes), tiles_dev, t, th, tw, oh, ow, mean, std, out)
    return out


def merge_tiles(rows, count_in, tiles, sizes, tile, in_size, div, margin, merged, count):
    """rr_merge_tiles: per-tile rows [T,k_in,6] (x,y,w,h,score,cls in the model's input coordinates, in_size = (oh, ow)) and
    count_in int32 [T] -> per frame, its tiles in table order and of each its first min(max(count_in[t], 0), k_in) rows:
    the margin test (margin > 0: a row leaves when it comes within `margin` input pixels of a tile side that is not on the
    frame's border — the box a tile edge has cut; the neighbouring tile sees it whole as long as the tiles' overlap exceeds
    margin / div plus the object size), x / div + x0, y / div + y0, w / div, h / div (float32, IEEE), appended to merged
    [F,K,6] at count [F] (in place, see merge_buffers).  count[f] ends as the true number of kept rows, also above K; rows
    beyond K are not written.  tiles: T host rows (frame, y0, x0) sorted by frame, sizes: (H, W) per frame."""
    import numpy as np
    th, tw = int(tile[0]), int(tile[1])
    table, tile_off = check_tiles(tiles, sizes, (th, tw))
    _C.require_cuda(rows, count_in, merged, count)
    f, k, six = merged.shape
    t = table.shape[0]
    assert f == len(sizes) and six == 6 and merged.is_contiguous() and 0 < k <= DETECT_MAX_ROWS
    assert count.numel() == f and count.is_contiguous()
    assert rows.is_contiguous() and rows.dim() == 3 and rows.shape[0] == t and rows.shape[2] == 6
    assert count_in.numel() == t and count_in.is_contiguous()
    div, margin = float(np.float32(div)), float(np.float32(margin))
    if not div > 0 or not margin >= 0:
        raise ValueError("merge_tiles: zoom %r, margin %r" % (div, margin))
    if f == 0:
        return
    dev = merged.device
    # an empty table still needs addresses the kernel may name
    tiles_dev = torch.from_numpy(table if t else np.zeros((1, 3), np.int32)).to(dev)
    off_dev = torch.from_numpy(tile_off).to(dev)
    hw_dev = torch.tensor([(int(h), int(w)) for h, w in sizes], dtype=torch.int32).to(dev)
    cin = count_in if t else torch.zeros(1, dtype=torch.int32, device=dev)
    _C.call("rr_merge_tiles", rows, cin, tiles_dev, off_dev, hw_dev, f, rows.shape[1], th, tw, int(in_size[0]), int(in_size[1]),
            div, margin, merged, count, k)


def sort_frames_by_score(rows6, count, out_off=None, xyxy=False):
    """rr_sort_frames_by_score: rows6 [B,K,6], count int32 [B] -> every frame's first count[f] rows by score descending
    (ties keep row order).  out_off None: [B,K,6], padding (class -1) behind the sorted rows.  out_off int32 [B+1]
    (ops.seg_prefix(count)): packed [B*K,6] with frame f at row out_off[f].  xyxy: columns 2,3 become x+w, y+h."""
    _C.require_cuda(rows6, count, out_off)
    b, k, six = rows6.shape
    if k > DETECT_MAX_ROWS:
        raise ValueError("sort_frames_by_score: %d rows per frame (limit %d)" % (k, DETECT_MAX_ROWS))
    assert six == 6 and rows6.is_contiguous()
    assert count.numel() == b and count.is_contiguous()
    assert out_off is None or (out_off.numel() == b + 1 and out_off.is_contiguous())
    out = torch.empty((b * k, 6) if out_off is not None else (b, k, 6), dtype=torch.float32, device=rows6.device)
    _C.call("rr_sort_frames_by_score", rows6, count, out_off, b, k, int(bool(xyxy)), out, b * k)
    return out


EVAL_MAX_GT = 2048            # RR_EVAL_MAX_GT: ground truths of one frame that rr_eval_match keeps in LDS
EVAL_MAX_THRESHOLDS = 16      # RR_EVAL_MAX_THRESHOLDS


def eval_match(dets, det_len, gts, gt_len, thresholds, cls_num=11):
    """rr_eval_match: `get_tp` of utils/metrics/metrics.py for F frames in one launch.  dets float32 [F,Dmax,6] =
    x,y,w,h,score,cls in evaluation order, det_len int32 [F]; gts float32 [F,Gmax,6] (cls 0 = ignored region), gt_len
    int32 [F]; thresholds float32 [T] (the host's tensor, moved to the device, not recomputed); all on the device.
    -> flag_bits int32 [F,Dmax] (bit t: true positive at threshold t), counted uint8 [F,Dmax], target_count int32
    [F,cls_num-1]."""
    assert dets.dim() == 3 and dets.shape[2] == 6 and gts.dim() == 3 and gts.shape[2] == 6
    f, dmax, gmax, t = dets.shape[0], dets.shape[1], gts.shape[1], thresholds.numel()
    if gmax > EVAL_MAX_GT:
        raise ValueError("eval_match: at most %d ground truths per frame (Gmax), got %d" % (EVAL_MAX_GT, gmax))
    if not 1 <= t <= EVAL_MAX_THRESHOLDS:
        raise ValueError("eval_match: 1..%d thresholds, got %d" % (EVAL_MAX_THRESHOLDS, t))
    _C.require_cuda(dets, det_len, gts, gt_len, thresholds)
    assert dets.is_contiguous() and gts.is_contiguous()
    assert gts.shape[0] == f and det_len.numel() == f and gt_len.numel() == f
    assert det_len.is_contiguous() and gt_len.is_contiguous()
    assert thresholds.is_contiguous()
    dev = dets.device
    flag_bits = torch.empty((f, dmax), dtype=torch.int32, device=dev)
    counted = torch.empty((f, dmax), dtype=torch.uint8, device=dev)
    target_count = torch.empty((f, cls_num - 1), dtype=torch.int32, device=dev)
    _C.call("rr_eval_match", dets, det_len, gts, gt_len, thresholds, f, dmax, gmax, t, int(cls_num), flag_bits, counted,
            target_count)
    return flag_bits, counted, target_count


def eval_ap(flag_bits, seg_off, target_count, in_img_count, t):
    """rr_eval_ap: `calculate_ap_rc`.  flag_bits int32 [N]: the counted detections' words class by class, each class
    sorted by confidence descending; seg_off int32 [C+1]; target_count, in_img_count int32 [C] summed over the frames.
    -> ap float32 [t], rc float32 [] on the device."""
    _C.require_cuda(flag_bits, seg_off, target_count, in_img_count)
    c = target_count.numel()
    assert flag_bits.is_contiguous() and flag_bits.dim() == 1
    assert seg_off.is_contiguous() and seg_off.numel() == c + 1
    assert in_img_count.numel() == c
    assert target_count.is_contiguous() and in_img_count.is_contiguous()
    dev = flag_bits.device
    work = torch.empty(2 * c * int(t), dtype=torch.float32, device=dev)
    ap = torch.empty(int(t), dtype=torch.float32, device=dev)
    rc = torch.empty((), dtype=torch.float32, device=dev)
    _C.call("rr_eval_ap", flag_bits, flag_bits.numel(), seg_off, target_count, in_img_count, c, int(t), work, ap, rc)
    return ap, rc


def roi_spatial_order(rois, frame_off):
    """Per-frame spatial processing order of the packed RoI list (frame_off int32 [B+1], device) -> int32 [R]."""
    r = rois.shape[0]
    order = torch.empty(max(r, 1), dtype=torch.int32, device=rois.device)
    _C.call("rr_roi_spatial_order", rois, frame_off, frame_off.numel() - 1, order)
    return order[:r]


def roi_align_fwd(feat, rois, out_size, spatial_scale=1.0, sampling_ratio=-1, order=None):
    assert is_nhwc(feat)
    b, c, h, w = feat.shape
    r = rois.shape[0]
    ph, pw = out_size
    out = empty_nhwc(r, c, ph, pw, feat.device)
    _C.call("rr_roi_align_fwd", feat, rois, r, h, w, c, ph, pw, float(spatial_scale), int(sampling_ratio), order, out)
    return out


def roi_align_bwd(dout, rois, feat_shape, out_size, spatial_scale=1.0, sampling_ratio=-1):
    b, c, h, w = feat_shape
    r = rois.shape[0]
    ph, pw = out_size
    dfeat = empty_nhwc(b, c, h, w, dout.device)
    _C.call("rr_roi_align_bwd", dout, rois, r, b, h, w, c, ph, pw, float(spatial_scale), int(sampling_ratio), dfeat)
    return dfeat


# ---------------------------------------------------------------------------------------------
# DCNv2
# ---------------------------------------------------------------------------------------------
_DCN_WPACK = True       # False: rr_dcn_dgrad_bf16_ws (test_dcn_gpu.py::test_dcn_bf16_dgrad_equals_fp32_dgrad_on_rounded_operands)


def dcn_fwd(x, offset, mask, w, bias, stride, pad, dilation, dg, bf16=False):
    assert is_nhwc(x) and is_nhwc(offset) and is_nhwc(mask) and is_nhwc(w)
    n, c, h, wd = x.shape
    k, _, r, s = w.shape
    p, q = offset.shape[2], offset.shape[3]
    y = empty_nhwc(n, k, p, q, x.device)
    if bf16 and _DCN_WPACK:
        # weights re-packed to bf16 inside the call (one small kernel): the B operand then reaches LDS by DMA
        wpack = torch.empty(_C.call("rr_dcn_wpack_bytes", c, k, r, s), dtype=torch.uint8, device=x.device)
        _C.call("rr_dcn_fwd_bf16_packed", x, offset, mask, w, bias, y, n, h, wd, c, k, r, s, stride, pad[0], pad[1], dilation, dg,
                wpack)
        return y
    name = "rr_dcn_fwd_bf16" if bf16 else "rr_dcn_fwd"
    _C.call(name, x, offset, mask, w, bias, y, n, h, wd, c, k, r, s, stride, pad[0], pad[1], dilation, dg)
    return y


def dcn_im2col(x, offset, mask, r, s, stride, pad, dilation, dg):
    n, c, h, wd = x.shape
    m = offset.shape[0] * offset.shape[2] * offset.shape[3]
    col = torch.empty((1, m, 1, r * s * c), dtype=torch.float32, device=x.device).permute(0, 3, 1, 2)
    _C.call("rr_dcn_im2col", x, offset, mask, col, n, h, wd, c, r, s, stride, pad[0], pad[1], dilation, dg)
    return col                                           # logical [1, r*s*c, M, 1], memory [M][r*s*c]


def dcn_col2im(x, offset, mask, dcol, r, s, stride, pad, dilation, dg):
    n, c, h, wd = x.shape
    dx = empty_nhwc(n, c, h, wd, x.device)
    doff = torch.empty_like(offset)
    dmask = torch.empty_like(mask)
    assert doff.stride() == offset.stride() and dmask.stride() == mask.stride()
    _C.call("rr_dcn_col2im", x, offset, mask, dcol, dx, doff, dmask, n, h, wd, c, r, s, stride, pad[0], pad[1], dilation, dg)
    return dx, doff, dmask


def dcn_fused_bwd_supported(c, k, r, s, stride, dg, dilation=1):
    """Whether rr_dcn_wgrad / rr_dcn_dgrad take a layer of this shape (else: the column path)."""
    return bool(_C.call("rr_dcn_fused_bwd_supported_dil", c, k, r, s, stride, dilation, dg))


def dcn_wgrad(x, offset, mask, dy, dw, stride, pad, dilation, dg, bf16=False, dy_img=None):
    """dw [K,C,R,S] (OHWI memory, pre-zeroed or the running gradient) += dY^T x deformed columns; no column buffer.
    bf16: bf16 matrix operands (dY, samples), input window in LDS (rr_dcn_wgrad_bf16); dy_img: dY's bf16 image, complete on
    the current stream — the dY operand then reaches LDS by DMA (rr_dcn_wgrad_bf16_img)."""
    assert is_nhwc(x) and is_nhwc(offset) and is_nhwc(mask) and is_nhwc(dy) and is_nhwc(dw)
    n, c, h, wd = x.shape
    k, _, r, s = dw.shape
    if bf16 and dy_img is not None:
        _C.call("rr_dcn_wgrad_bf16_img", x, offset, mask, dy, dy_img, dw, n, h, wd, c, k, r, s, stride, pad[0], pad[1], dilation,
                dg)
        return dw
    name = "rr_dcn_wgrad_bf16" if bf16 else "rr_dcn_wgrad"
    _C.call(name, x, offset, mask, dy, dw, n, h, wd, c, k, r, s, stride, pad[0], pad[1], dilation, dg)
    return dw


def dcn_dgrad_accumulates(bf16):
    """True when dcn_dgrad(..., out=buf) adds into buf inside the kernel (the LDS-DMA data gradient of the bf16 path)."""
    return bool(bf16 and _DCN_WPACK)


def dcn_dgrad(x, offset, mask, w, dy, stride, pad, dilation, dg, bf16=False, out=None):
    """-> dx, doffset, dmask; the column gradient never leaves the MFMA accumulators / LDS.  bf16: bf16 matrix operands
    (dY, W) and d input pre-summed in an LDS window before the global atomics (rr_dcn_dgrad_bf16)."""
    assert is_nhwc(x) and is_nhwc(offset) and is_nhwc(mask) and is_nhwc(dy) and is_nhwc(w)
    n, c, h, wd = x.shape
    k, _, r, s = w.shape
    # out: a buffer that already holds another consumer's gradient of x — d input is ADDED to it (dcn_dgrad_accumulates only)
    assert out is None or (dcn_dgrad_accumulates(bf16) and is_nhwc(out) and tuple(out.shape) == tuple(x.shape))
    dx = out if out is not None else empty_nhwc(n, c, h, wd, x.device)
    if out is not None:
        amax_drop(out)                # an existing tensor added into through its pointer
    doff = torch.empty_like(offset)
    dmask = torch.empty_like(mask)
    assert doff.stride() == offset.stride() and dmask.stride() == mask.stride()
    img = b16_side.now(dy) if bf16 else None
    if bf16 and _DCN_WPACK:
        # both sweep operands by LDS-DMA: weights packed to bf16 inside the call; dY = its producer's bf16 image when there is
        # one (the heads' 1x1 data gradient), else rounded once into the workspace
        ws = torch.empty(_C.call("rr_dcn_dgrad_ws_bytes", dy.shape[0], dy.shape[2], dy.shape[3], c, k, r, s, int(img is not None)),
                         dtype=torch.uint8, device=x.device)
        _C.call("rr_dcn_dgrad_bf16_packed", x, offset, mask, w, dy, img, dx, doff, dmask, n, h, wd, c, k, r, s, stride, pad[0], pad[1],
                dilation, dg, int(out is not None), ws)
        return dx, doff, dmask
    if img is not None:
        # dY's producer already left its bf16 image (the heads' 1x1 data gradient): no conversion pass
        _C.call("rr_dcn_dgrad_bf16_img", x, offset, mask, w, dy, img, dx, doff, dmask, n, h, wd, c, k, r, s, stride, pad[0], pad[1],
                dilation, dg)
        return dx, doff, dmask
    if bf16:
        # dY rounded to bf16 once per call (caller scratch): the sweep's eight re-reads of a block's dY tile stay in L2
        dyb = torch.empty(_C.call("rr_dcn_dyb_bytes", dy.shape[0], dy.shape[2], dy.shape[3], k), dtype=torch.uint8, device=x.device)
        _C.call("rr_dcn_dgrad_bf16_ws", x, offset, mask, w, dy, dx, doff, dmask, n, h, wd, c, k, r, s, stride, pad[0], pad[1],
                dilation, dg, dyb)
        return dx, doff, dmask
    _C.call("rr_dcn_dgrad", x, offset, mask, w, dy, dx, doff, dmask, n, h, wd, c, k, r, s, stride, pad[0], pad[1], dilation, dg)
    return dx, doff, dmask


def dcn_split_fwd(om):
    """om [N, 3t, P, Q] (NHWC memory) -> offset [N, 2t, P, Q], mask [N, t, P, Q] = sigmoid(last third)."""
    assert is_nhwc(om) and om.shape[1] % 3 == 0
    n, ch, p, q = om.shape
    t = ch // 3
    offset, mask = empty_nhwc(n, 2 * t, p, q, om.device), empty_nhwc(n, t, p, q, om.device)
    _C.call("rr_dcn_split_fwd", om, n * p * q, t, offset, mask)
    return offset, mask


def dcn_split_bwd(doffset, dmask, mask):
    n, t, p, q = mask.shape
    dom = empty_nhwc(n, 3 * t, p, q, mask.device)
    _C.call("rr_dcn_split_bwd", doffset, dmask, mask, n * p * q, t, dom)
    return dom


def dcn_psroi_fwd(x, rois, trans, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size, sample_per_part,
                  trans_std):
    """Deformable PS-RoI pooling.  x NHWC; rois [n,5]; trans [n,2*classes,part,part] (contiguous NCHW) or None.
    -> out, count: logical [n, output_dim, pooled, pooled], NHWC memory."""
    assert is_nhwc(x)
    b, c, h, w = x.shape
    n = rois.shape[0]
    out = empty_nhwc(n, output_dim, pooled_size, pooled_size, x.device)
    count = empty_nhwc(n, output_dim, pooled_size, pooled_size, x.device)
    tc = 0 if no_trans else trans.shape[1]
    _C.call("rr_dcn_psroi_fwd", x, rois, None if no_trans else trans, n, h, w, c, int(no_trans), float(spatial_scale), output_dim,
            group_size, pooled_size, part_size, sample_per_part, float(trans_std), tc, out, count)
    return out, count


def dcn_psroi_bwd(dout, x, rois, trans, count, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
                  sample_per_part, trans_std):
    assert is_nhwc(x) and is_nhwc(dout)
    b, c, h, w = x.shape
    n = rois.shape[0]
    dx = empty_nhwc(b, c, h, w, x.device)
    dtrans = None if no_trans else torch.empty_like(trans)
    tc = 0 if no_trans else trans.shape[1]
    _C.call("rr_dcn_psroi_bwd", dout, x, rois, None if no_trans else trans, count, n, b, h, w, c, int(no_trans),
            float(spatial_scale), output_dim, group_size, pooled_size, part_size, sample_per_part, float(trans_std), tc, dx, dtrans)
    return dx, dtrans


# ---------------------------------------------------------------------------------------------
# RetinaNet (csrc/retina.hip)
# ---------------------------------------------------------------------------------------------
def maxpool3x3s2_fwd(x):
    """x NHWC [n,c,h,w] -> (y, idx): MaxPool2d(3, 2, 1) and the winning tap (uint8, 0..8) of every output element."""
    _C.require_cuda(x)
    assert is_nhwc(x)
    n, c, h, w = x.shape
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    y = empty_nhwc(n, c, oh, ow, x.device)
    idx = empty_nhwc(n, c, oh, ow, x.device, dtype=torch.uint8)
    _C.call("rr_maxpool3x3s2_fwd", x, y, idx, n, h, w, c)
    return y, idx


def maxpool3x3s2_bwd(dy, idx, x_shape):
    n, c, h, w = x_shape
    assert is_nhwc(dy) and is_nhwc(idx) and dy.shape == idx.shape
    assert tuple(dy.shape) == (n, c, (h - 1) // 2 + 1, (w - 1) // 2 + 1)
    dx = empty_nhwc(n, c, h, w, dy.device)
    _C.call("rr_maxpool3x3s2_bwd", dy, idx, dx, n, h, w, c)
    return dx


def bilinear_add_fwd(x, y):
    """y + F.interpolate(x, size(y), mode='bilinear', align_corners=False); both NHWC."""
    _C.require_cuda(x, y)
    assert is_nhwc(x) and is_nhwc(y) and x.shape[:2] == y.shape[:2]
    n, c, ih, iw = x.shape
    oh, ow = y.shape[2], y.shape[3]
    out = empty_nhwc(n, c, oh, ow, x.device)
    _C.call("rr_bilinear_add_fwd", x, y, out, n, ih, iw, oh, ow, c)
    return out


def bilinear_add_bwd(dout, x_shape):
    n, c, ih, iw = x_shape
    assert is_nhwc(dout) and dout.shape[0] == n and dout.shape[1] == c
    dx = empty_nhwc(n, c, ih, iw, dout.device)
    _C.call("rr_bilinear_add_bwd", dout, dx, n, ih, iw, dout.shape[2], dout.shape[3], c)
    return dx


def retina_assign(annos, anchors, num_classes):
    """annos [B,M,8] xywh rows (zero rows = padding), anchors [A,4] xyxy ->
    dict(state int8 [B,A], argmax int32, max_iou, cls int32, target [B,A,4], npos int32 [B])."""
    _C.require_cuda(annos, anchors)
    assert annos.dim() == 3 and annos.shape[2] == 8 and anchors.dim() == 2 and anchors.shape[1] == 4
    annos = annos.contiguous().float()
    anchors = anchors.contiguous().float()
    b, m, a = annos.shape[0], annos.shape[1], anchors.shape[0]
    if m == 0:                                  # an all-padding image list: one zero row wins nothing
        annos, m = annos.new_zeros((b, 1, 8)), 1
    dev = annos.device
    out = {
        "state": torch.empty((b, a), dtype=torch.int8, device=dev),
        "argmax": torch.empty((b, a), dtype=torch.int32, device=dev),
        "max_iou": torch.empty((b, a), dtype=torch.float32, device=dev),
        "cls": torch.empty((b, a), dtype=torch.int32, device=dev),
        "target": torch.empty((b, a, 4), dtype=torch.float32, device=dev),
        "npos": torch.empty((b,), dtype=torch.int32, device=dev),
    }
    _C.call("rr_retina_assign", annos, anchors, b, m, a, int(num_classes), out["state"], out["argmax"], out["max_iou"], out["cls"],
            out["target"], out["npos"])
    return out


def _retina_loss_args(logits, loc, asg):
    assert logits.dim() == 3 and loc.dim() == 3 and loc.shape[2] == 4 and logits.shape[:2] == loc.shape[:2]
    assert logits.is_contiguous() and loc.is_contiguous()
    b, a, c = logits.shape
    assert tuple(asg["state"].shape) == (b, a) and tuple(asg["target"].shape) == (b, a, 4)
    return b, a, c


def retina_loss_fwd(logits, loc, asg):
    """-> losses [2] = (classification, regression) of the criterion, bit-identical run to run."""
    _C.require_cuda(logits, loc)
    b, a, c = _retina_loss_args(logits, loc, asg)
    nblk = _C.call("rr_retina_loss_blocks", a, c)
    partial = torch.empty((b, nblk, 2), dtype=torch.float64, device=logits.device)
    losses = torch.empty(2, dtype=torch.float32, device=logits.device)
    _C.call("rr_retina_loss_fwd", logits, loc, asg["state"], asg["cls"], asg["target"], asg["npos"], b, a, c, partial, losses)
    return losses


def retina_loss_bwd(logits, loc, asg, gout):
    """gout [2] (device) -> (d logits [B,A,C], d loc [B,A,4])."""
    b, a, c = _retina_loss_args(logits, loc, asg)
    assert gout.numel() == 2 and gout.is_contiguous()
    dlogits, dloc = torch.empty_like(logits), torch.empty_like(loc)
    _C.call("rr_retina_loss_bwd", logits, loc, asg["state"], asg["cls"], asg["target"], asg["npos"], gout, b, a, c, dlogits, dloc)
    return dlogits, dloc


def retina_decode(logits, loc, anchors, score_thr=0.1):
    """logits [B,A,C], loc [B,A,4], anchors [A,4] -> (rows [B,A,6] = x,y,w,h,prob,cls+1 in anchor order, count int32 [B])."""
    _C.require_cuda(logits, loc, anchors)
    logits, loc, anchors = logits.contiguous().float(), loc.contiguous().float(), anchors.contiguous().float()
    b, a, c = logits.shape
    assert tuple(loc.shape) == (b, a, 4) and tuple(anchors.shape) == (a, 4)
    rows = torch.zeros((b, a, 6), dtype=torch.float32, device=logits.device)
    count = torch.zeros((b,), dtype=torch.int32, device=logits.device)
    if a > 0:
        _C.call("rr_retina_decode", logits, loc, anchors, b, a, c, float(score_thr), rows, count)
    return rows, count


RETINA_DECODE_CHUNK = 256     # RR_RETINA_DECODE_CHUNK: anchors of one workgroup of rr_retina_decode_frames


def retina_decode_frames(logits, loc, anchors, score_thr=0.1, k=None, rows=None):
    """rr_retina_decode_frames: retina_decode with an image's anchors spread over workgroups.  logits [B,A,C], loc [B,A,4],
    anchors [A,4] -> (rows [B,k,6], count int32 [B]); k defaults to A.  The first min(count[f], k) rows of a frame are
    retina_decode's; count[f] is the true number of candidates also above k.  rows (optional): the buffer to write into —
    what lies behind min(count[f], k) stays as it was (a fresh buffer is zero-filled)."""
    _C.require_cuda(logits, loc, anchors, rows)
    logits, loc, anchors = logits.contiguous().float(), loc.contiguous().float(), anchors.contiguous().float()
    b, a, c = logits.shape
    assert tuple(loc.shape) == (b, a, 4) and tuple(anchors.shape) == (a, 4)
    k = a if k is None else int(k)
    if rows is None:
        rows = torch.zeros((b, k, 6), dtype=torch.float32, device=logits.device)
    assert tuple(rows.shape) == (b, k, 6) and rows.is_contiguous()
    count = torch.zeros((b,), dtype=torch.int32, device=logits.device)
    if a > 0 and b > 0:
        ws = torch.empty(_C.call("rr_retina_decode_frames_workspace_bytes", b, a), dtype=torch.uint8, device=logits.device)
        _C.call("rr_retina_decode_frames", logits, loc, anchors, b, a, c, float(score_thr), rows, k, count, ws)
    return rows, count


def nms_frames(rows6, frame_off, max_rows, thresh, inclusive=False):
    """rr_nms_frames: the reference's hard NMS ("+1" IoU; suppression at IoU > thresh, with inclusive at IoU >= thresh) for
    every frame of a batch.  rows6 [R,6] = packed score-descending x,y,w,h,score,cls rows (sort_frames_by_score with
    out_off), frame_off int32 [B+1], max_rows >= the longest frame, R >= B * max_rows.
    -> (keep int32 [R]: keep[frame_off[f] + j] = j-th kept row of frame f, local to the frame; kept int32 [B])."""
    _C.require_cuda(rows6, frame_off)
    assert rows6.dim() == 2 and rows6.shape[1] == 6 and rows6.is_contiguous()
    assert frame_off.dim() == 1 and frame_off.numel() >= 1 and frame_off.is_contiguous()
    b, max_rows = frame_off.numel() - 1, int(max_rows)
    if not 0 <= max_rows <= DETECT_MAX_ROWS:
        raise ValueError("nms_frames: %d rows per frame (limit %d)" % (max_rows, DETECT_MAX_ROWS))
    assert rows6.shape[0] >= b * max_rows
    dev = rows6.device
    keep = torch.empty(rows6.shape[0], dtype=torch.int32, device=dev)
    kept = torch.zeros(b, dtype=torch.int32, device=dev)
    ws = torch.empty(_C.call("rr_nms_frames_workspace_bytes", b, max_rows), dtype=torch.uint8, device=dev)
    _C.call("rr_nms_frames", rows6, frame_off, b, max_rows, float(thresh), int(bool(inclusive)), ws, keep, kept)
    return keep, kept


def pack_frames(rows6, frame_off, keep, kept, max_rows, out_rows=None):
    """rr_pack_frames: the rows nms_frames kept, frames back to back, each in its score order -> (out6 [out_rows,6], out_off
    int32 [B+1] = exclusive prefix of kept).  out_rows defaults to rows6's row count; the caller slices by out_off[-1]."""
    _C.require_cuda(rows6, frame_off, keep, kept)
    b, max_rows = frame_off.numel() - 1, int(max_rows)
    assert rows6.dim() == 2 and rows6.shape[1] == 6 and rows6.is_contiguous()
    assert keep.numel() == rows6.shape[0] and keep.is_contiguous()
    assert kept.numel() == b and kept.is_contiguous()
    assert frame_off.is_contiguous() and rows6.shape[0] >= b * max_rows
    out_rows = rows6.shape[0] if out_rows is None else int(out_rows)
    out6 = torch.empty((out_rows, 6), dtype=torch.float32, device=rows6.device)
    out_off = torch.empty(b + 1, dtype=torch.int32, device=rows6.device)
    _C.call("rr_pack_frames", rows6, frame_off, keep, kept, b, max_rows, out6, out_rows, out_off)
    return out6, out_off


KMEANS_MAX_K, KMEANS_MAX_M, KMEANS_MAX_R = 64, 4, 64      # RR_KMEANS_MAX_K / _M / _R


def kmeans_lloyd(X, init, tol=1e-4, max_iter=10000, check_every=16):
    """rr_kmeans_steps: Lloyd's algorithm for R restarts side by side.  X [N,M] float32, init [R,k,M] float32 (device) ->
    (labels int32 [R,N], centres float32 [R,k,M], counts int32 [R,k], inertia float64 [R], iters int32 [R], converged bool
    [R]).  Labels, counts and inertia refer to the centres before the last update, as the reference's labels do; an empty
    cluster keeps its centre; a restart ends when shift^2 < tol (converged) or at max_iter.  `check_every` steps are
    enqueued on the current stream between two reads of the R done flags; the result does not depend on it.  Shapes
    outside 1 <= k <= 64, 1 <= M <= 4, 1 <= R <= 64, N >= 1 raise ValueError before anything is launched."""
    if not (torch.is_tensor(X) and torch.is_tensor(init)):
        raise ValueError("kmeans_lloyd: X and init must be tensors")
    if X.dim() != 2 or init.dim() != 3:
        raise ValueError("kmeans_lloyd: X must be [N,M] and init [R,k,M], got %s and %s" % (tuple(X.shape), tuple(init.shape)))
    if X.dtype != torch.float32 or init.dtype != torch.float32:
        raise ValueError("kmeans_lloyd: X and init must be float32, got %s and %s" % (X.dtype, init.dtype))
    (n, m), (r, k, m2) = X.shape, init.shape
    if m2 != m:
        raise ValueError("kmeans_lloyd: init has %d columns, X has %d" % (m2, m))
    if not (n >= 1 and 1 <= m <= KMEANS_MAX_M and 1 <= k <= KMEANS_MAX_K and 1 <= r <= KMEANS_MAX_R):
        raise ValueError("kmeans_lloyd: N=%d M=%d k=%d R=%d outside N >= 1, 1 <= M <= %d, 1 <= k <= %d, 1 <= R <= %d"
                         % (n, m, k, r, KMEANS_MAX_M, KMEANS_MAX_K, KMEANS_MAX_R))
    max_iter, check_every = int(max_iter), int(check_every)
    if max_iter < 1 or check_every < 1:
        raise ValueError("kmeans_lloyd: max_iter=%d and check_every=%d must be at least 1" % (max_iter, check_every))
    _C.require_cuda(X, init)
    dev = X.device
    X = X.contiguous()
    if X.data_ptr() % 16:
        X = X.clone()
    centres = init.to(dev).clone(memory_format=torch.contiguous_format)
    labels = torch.empty((r, n), dtype=torch.int32, device=dev)
    counts = torch.zeros((r, k), dtype=torch.int32, device=dev)
    inertia = torch.zeros((r,), dtype=torch.float64, device=dev)
    iters = torch.zeros((r,), dtype=torch.int32, device=dev)
    flags = torch.zeros((r,), dtype=torch.int32, device=dev)
    ws = torch.empty(_C.call("rr_kmeans_workspace_bytes", n, m, k, r), dtype=torch.uint8, device=dev)
    left = max_iter
    while left > 0:
        ns = min(check_every, left)
        _C.call("rr_kmeans_steps", X, n, m, k, r, centres, labels, counts, inertia, iters, flags, float(tol), max_iter, ns, ws)
        left -= ns
        if bool(flags.cpu().numpy().all()):                  # the one host read per `check_every` steps
            break
    return labels, centres, counts, inertia, iters, flags == 1


# ---------------------------------------------------------------------------------------------
# SE hourglass (csrc/se.hip): squeeze-and-excitation tail of the residual block, the stem's 2x2 max-pool
# ---------------------------------------------------------------------------------------------
_SE = _C.Family("rrnet_hip_se.h")       # the family's own header beside include/rrnet_hip.h
SE_MIN_CHUNK_ROWS = 128       # rows of the map one workgroup of the two reductions sums ...
SE_MAX_CHUNKS = 256           # ... and at most this many chunks per sample (the per-sample kernels finish them one by one)


def se_chunk_rows(hw):
    """Rows per workgroup of rr_se_squeeze / rr_se_bwd_reduce for a map of hw pixels -> (chunk_rows, chunks)."""
    rows = max(SE_MIN_CHUNK_ROWS, -(-hw // SE_MAX_CHUNKS))
    return rows, -(-hw // rows)


def _se_dims(u):
    assert is_nhwc(u) and u.dtype == torch.float32
    n, c, h, w = u.shape
    return n, c, h * w


def se_squeeze(u):
    """u NHWC [n,c,h,w] -> partial sums over the map, [n, chunks, c] float64."""
    n, c, hw = _se_dims(u)
    rows, chunks = se_chunk_rows(hw)
    part = torch.empty((n, chunks, c), dtype=torch.float64, device=u.device)
    _SE.call("rr_se_squeeze", u, part, n, hw, c, rows)
    return part


def se_excite_fwd(part, w1, w2, hw):
    """part of se_squeeze, w1 [c/r, c], w2 [c, c/r] -> (m [n,c] mean, h [n,c/r] = relu(w1 m), s [n,c] = sigmoid(w2 h))."""
    n, chunks, c = part.shape
    cr = w1.shape[0]
    assert tuple(w1.shape) == (cr, c) and tuple(w2.shape) == (c, cr) and w1.is_contiguous() and w2.is_contiguous()
    m = torch.empty((n, c), dtype=torch.float32, device=part.device)
    h = torch.empty((n, cr), dtype=torch.float32, device=part.device)
    s = torch.empty((n, c), dtype=torch.float32, device=part.device)
    _SE.call("rr_se_excite_fwd", part, w1, w2, m, h, s, n, chunks, c, cr, hw)
    return m, h, s


def se_scale_res_relu_fwd(u, s, skip):
    """relu(u * s[n, c] + skip), one pass."""
    n, c, hw = _se_dims(u)
    assert is_nhwc(skip) and skip.shape == u.shape and tuple(s.shape) == (n, c)
    out = empty_nhwc(*u.shape, device=u.device)
    _SE.call("rr_se_scale_res_relu_fwd", u, s, skip, out, n, hw, c)
    return out


def se_bwd_reduce(dout, out, u):
    """partial sums over the map of dout * (out > 0) * u, [n, chunks, c] float64."""
    n, c, hw = _se_dims(u)
    assert is_nhwc(dout) and is_nhwc(out) and dout.shape == u.shape == out.shape
    rows, chunks = se_chunk_rows(hw)
    part = torch.empty((n, chunks, c), dtype=torch.float64, device=u.device)
    _SE.call("rr_se_bwd_reduce", dout, out, u, part, n, hw, c, rows)
    return part


def se_excite_bwd(part, s, h, m, w1, w2, dw1, dw2):
    """part of se_bwd_reduce -> dm [n,c] (the gradient of the mean); ADDS the weight gradients into dw1 [c/r, c] / dw2 [c, c/r]."""
    n, chunks, c = part.shape
    cr = w1.shape[0]
    assert dw1.shape == w1.shape and dw2.shape == w2.shape and dw1.is_contiguous() and dw2.is_contiguous()
    dm = torch.empty((n, c), dtype=torch.float32, device=part.device)
    ws = torch.empty((n, c + cr), dtype=torch.float32, device=part.device)
    _SE.call("rr_se_excite_bwd", part, s, h, m, w1, w2, dm, dw1, dw2, ws, n, chunks, c, cr)
    return dm


def se_bwd_apply(dout, out, s, dm, dskip_into=None):
    """-> (du, dskip): du = g * s[n, c] + dm[n, c] / hw, dskip = g = dout * (out > 0).  dskip_into: g is added into that
    tensor instead (a fan-in buffer that already holds another consumer's gradient) and dskip comes back None."""
    n, c, hw = _se_dims(out)
    assert is_nhwc(dout) and dout.shape == out.shape
    du = empty_nhwc(*out.shape, device=out.device)
    dskip = None
    if dskip_into is None:
        dskip = empty_nhwc(*out.shape, device=out.device)
    else:
        assert is_nhwc(dskip_into) and dskip_into.shape == out.shape and dskip_into.dtype == torch.float32
    _SE.call("rr_se_bwd_apply", dout, out, s, dm, du, dskip, dskip_into, n, hw, c)
    return du, dskip


def maxpool2x2_fwd(x):
    """x NHWC [n,c,h,w] -> (y, idx): MaxPool2d(2) (floor on odd sizes) and the winning tap (uint8, 0..3) of every output element."""
    _C.require_cuda(x)
    assert is_nhwc(x)
    n, c, h, w = x.shape
    y = empty_nhwc(n, c, h // 2, w // 2, x.device)
    idx = empty_nhwc(n, c, h // 2, w // 2, x.device, dtype=torch.uint8)
    _SE.call("rr_maxpool2x2_fwd", x, y, idx, n, h, w, c)
    return y, idx


def maxpool2x2_bwd(dy, idx, x_shape):
    n, c, h, w = x_shape
    assert is_nhwc(dy) and is_nhwc(idx) and dy.shape == idx.shape and tuple(dy.shape) == (n, c, h // 2, w // 2)
    dx = empty_nhwc(n, c, h, w, dy.device)
    _SE.call("rr_maxpool2x2_bwd", dy, idx, dx, n, h, w, c)
    return dx


# ---------------------------------------------------------------------------------------------
# Dilated-window attention (csrc/attn.hip): the unfold / softmax / weighted-sum chain of modules/self_attention.py
# ---------------------------------------------------------------------------------------------
_ATTN = _C.Family("rrnet_hip_attn.h")   # the family's own header beside include/rrnet_hip.h
ATTN_MAX_TAPS = 64


def _pair(v):
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def window_attention_geometry(h, w, kernel_size, dilation, padding):
    """-> ((kh, kw), (dh, dw), (ph, pw), (oh, ow), (cy, cx)): the output size of the stride-1 window and the offset of an
    output's query position (modules/self_attention.py:58-60, :84)."""
    k, d, p = _pair(kernel_size), _pair(dilation), _pair(padding)
    out = tuple(s + 2 * p[i] - d[i] * (k[i] - 1) for i, s in enumerate((h, w)))
    centre = tuple(d[i] * (k[i] // 2) - p[i] for i in range(2))
    return k, d, p, out, centre


def _attn_launch(entry, flops, nbytes, *args):
    return _launch(entry[3:], flops, entry, args, nbytes=nbytes, call=_ATTN.call)


def _attn_dims(q, k, v, kernel_size, dilation, padding):
    assert is_nhwc(q) and is_nhwc(k) and is_nhwc(v) and q.dtype == k.dtype == v.dtype == torch.float32
    n, ck, h, w = q.shape
    cv = v.shape[1]
    assert k.shape == q.shape and tuple(v.shape) == (n, cv, h, w)
    kk, d, p, out, _ = window_attention_geometry(h, w, kernel_size, dilation, padding)
    return (n, h, w, ck, cv) + kk + d + p, out, kk[0] * kk[1]


def window_attention_fwd(q, k, v, kernel_size, dilation, padding):
    """q, k NHWC [n,ck,h,w], v NHWC [n,cv,h,w] -> (ctx NHWC [n,cv,oh,ow], p [n,oh,ow,T]): the softmax over a pixel's T window
    taps of q . k (a padded tap: logit 0, value 0) and the context it weighs out of v."""
    _C.require_cuda(q, k, v)
    dims, (oh, ow), taps = _attn_dims(q, k, v, kernel_size, dilation, padding)
    n, h, w, ck, cv = dims[:5]
    # (a geometry the entry refuses gets placeholders of one element: the refusal comes from the library, before any launch)
    ok = oh >= 1 and ow >= 1
    ctx = empty_nhwc(n, cv, max(oh, 1), max(ow, 1), q.device)
    p = torch.empty((n, max(oh, 1), max(ow, 1), taps), dtype=torch.float32, device=q.device)
    px = n * oh * ow if ok else 0
    _attn_launch("rr_attn_fwd", 2.0 * px * taps * (ck + cv), 4.0 * (n * h * w * (2 * ck + cv) + px * (cv + taps)),
                 q, k, v, ctx, p, *dims)
    return ctx, p


def window_attention_bwd(dctx, q, k, v, p, kernel_size, dilation, padding):
    """-> (dq, dk, dv), each written whole (a query position no output reads: 0)."""
    dims, (oh, ow), taps = _attn_dims(q, k, v, kernel_size, dilation, padding)
    n, h, w, ck, cv = dims[:5]
    assert is_nhwc(dctx) and dctx.dtype == torch.float32 and tuple(dctx.shape) == (n, cv, oh, ow)
    assert tuple(p.shape) == (n, oh, ow, taps) and p.is_contiguous() and p.dtype == torch.float32
    ds = torch.empty_like(p)
    dq, dk, dv = empty_nhwc(*q.shape, device=q.device), empty_nhwc(*k.shape, device=q.device), empty_nhwc(*v.shape, device=q.device)
    px, mp = n * oh * ow, n * h * w
    _attn_launch("rr_attn_bwd_q", 2.0 * px * taps * (ck + cv), 4.0 * (mp * (2 * ck + cv) + px * (cv + 2 * taps)),
                 dctx, v, k, p, ds, dq, *dims)
    _attn_launch("rr_attn_bwd_kv", 2.0 * px * taps * (ck + cv), 4.0 * (mp * (2 * ck + cv) + px * (cv + 2 * taps)),
                 ds, p, q, dctx, dk, dv, *dims)
    return dq, dk, dv


# ---------------------------------------------------------------------------------------------
# ShuffleNetV2 (csrc/depthwise.hip): the depthwise 3x3 convolution and the channel shuffle with its split / join copies
# ---------------------------------------------------------------------------------------------
_DW = _C.Family("rrnet_hip_dw.h")       # the family's own header beside include/rrnet_hip.h
DW_SLAB_PIXELS = 64           # RR_DW_SLAB_PIXELS of the header: output pixels per workgroup of the forward = per slab tile
DW_MIN_TILE_PIXELS = 128      # output pixels one workgroup of the weight gradient's first stage sums ...
DW_MAX_TILES = 256            # ... and at most this many tiles (the second stage adds them one by one)


def _dw_launch(entry, flops, nbytes, *args):
    return _launch(entry[3:], flops, entry, args, nbytes=nbytes, call=_DW.call)


def dw_out_hw(h, w, stride):
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def dw_tile_pixels(pixels):
    """Output pixels per workgroup of rr_dwconv3x3_bwd_weight's first stage -> (tile_pixels, tiles)."""
    tile = max(DW_MIN_TILE_PIXELS, -(-pixels // DW_MAX_TILES))
    return tile, -(-pixels // tile)


def _dw_filter(w, c):
    """The parameter [c, 1, 3, 3] (any of its layouts: one input channel) as the [c, 3, 3] block the kernels read."""
    assert tuple(w.shape) == (c, 1, 3, 3) and w.dtype == torch.float32, (tuple(w.shape), c)
    f = w.permute(0, 2, 3, 1)
    if not f.is_contiguous():
        f = f.contiguous()
    return f


def dwconv3x3_fwd(x, w, bias=None, stride=1, want_stats=False):
    """x NHWC [n,c,h,w], w [c,1,3,3] -> y NHWC [n,c,P,Q] (padding 1), or (y, slab) with the BatchNorm partial sums
    [mtiles,2,c] float64 of y in rr_conv_fprop's layout (bn_stats_finalize / bn_reduce_slab read it)."""
    _C.require_cuda(x, w, bias)
    assert is_nhwc(x) and x.dtype == torch.float32
    n, c, h, wd = x.shape
    if stride not in (1, 2):
        raise ValueError("dwconv3x3_fwd: stride %r (1 or 2)" % (stride,))
    p, q = dw_out_hw(h, wd, stride)
    y = empty_nhwc(n, c, p, q, x.device)
    slab = None
    if want_stats:
        slab = torch.empty((-(-(n * p * q) // DW_SLAB_PIXELS), 2, c), dtype=torch.float64, device=x.device)
    _dw_launch("rr_dwconv3x3_fwd", 18.0 * n * p * q * c, 4.0 * c * (n * h * wd + n * p * q), x, _dw_filter(w, c), bias, y, slab,
               n, h, wd, c, stride)
    return (y, slab) if want_stats else y


def dwconv3x3_bwd_data(dy, w, x_shape, stride=1):
    """-> dx NHWC of x_shape, written whole."""
    n, c, h, wd = x_shape
    p, q = dw_out_hw(h, wd, stride)
    assert is_nhwc(dy) and dy.dtype == torch.float32 and tuple(dy.shape) == (n, c, p, q)
    dx = empty_nhwc(n, c, h, wd, dy.device)
    _dw_launch("rr_dwconv3x3_bwd_data", 18.0 * n * p * q * c, 4.0 * c * (n * h * wd + n * p * q), dy, _dw_filter(w, c), dx,
               n, h, wd, c, stride)
    return dx


def dwconv3x3_bwd_weight(x, dy, dw, stride=1, accumulate=False):
    """dw [c,1,3,3] = (accumulate: dw +) the filter gradient; dw is written in place (a parameter's gradient target)."""
    n, c, h, wd = x.shape
    p, q = dw_out_hw(h, wd, stride)
    assert is_nhwc(x) and is_nhwc(dy) and tuple(dy.shape) == (n, c, p, q) and x.dtype == dy.dtype == torch.float32
    assert tuple(dw.shape) == (c, 1, 3, 3) and dw.permute(0, 2, 3, 1).is_contiguous() and dw.dtype == torch.float32
    tile, tiles = dw_tile_pixels(n * p * q)
    partial = torch.empty((tiles, c, 9), dtype=torch.float64, device=x.device)
    _dw_launch("rr_dwconv3x3_bwd_weight", 18.0 * n * p * q * c, 4.0 * c * (n * h * wd + n * p * q), x, dy, partial, dw,
               int(bool(accumulate)), n, h, wd, c, stride, tile)
    return dw


def pixel_rows(t):
    """An NHWC tensor or a channel slice of one -> (pixels, channels, pixel stride in floats).  The pixels must lie one
    stride apart in n, h, w order; the channels densely."""
    assert t.dim() == 4 and t.dtype == torch.float32
    n, c, h, w = t.shape
    sn, sc, sh, sw = t.stride()
    stride = step = None
    ok = sc == 1 or c == 1
    for size, st in ((w, sw), (h, sh), (n, sn)):          # (a dimension of one element has no stride to speak of)
        if size == 1:
            continue
        if stride is None:
            stride = st
        elif st != step:
            ok = False
        step = st * size
    if stride is None:
        stride = c
    if not ok or stride < c:
        raise ValueError("not a channel slice of an NHWC tensor: shape %s strides %s" % (tuple(t.shape), tuple(t.stride())))
    return n * h * w, c, stride


def shuffle_interleave(a, b):
    """channel_shuffle(cat(a, b), 2): out[:, 2i] = a[:, i], out[:, 2i+1] = b[:, i].  a, b: NHWC tensors or channel slices."""
    _C.require_cuda(a, b)
    pa, half, sa = pixel_rows(a)
    pb, hb, sb = pixel_rows(b)
    assert a.shape == b.shape
    n, _, h, w = a.shape
    out = empty_nhwc(n, 2 * half, h, w, a.device)
    _dw_launch("rr_shuffle_interleave", 0.0, 16.0 * pa * half, a, sa, b, sb, out, 2 * half, pa, half)
    return out


def shuffle_deinterleave(g, da=None, db=None):
    """The inverse: -> (da, db) with da[:, i] = g[:, 2i], db[:, i] = g[:, 2i+1]; either may be given (a channel slice to fill)."""
    pg, c2, sg = pixel_rows(g)
    n, _, h, w = g.shape
    half = c2 // 2
    assert c2 % 2 == 0
    if da is None:
        da = empty_nhwc(n, half, h, w, g.device)
    if db is None:
        db = empty_nhwc(n, half, h, w, g.device)
    _, ha, sa = pixel_rows(da)
    _, hb, sb = pixel_rows(db)
    assert ha == hb == half and da.shape == db.shape and tuple(da.shape) == (n, half, h, w)
    _dw_launch("rr_shuffle_deinterleave", 0.0, 16.0 * pg * half, g, sg, da, sa, db, sb, pg, half)
    return da, db


def channel_copy(src, dst=None):
    """src (a channel slice of an NHWC tensor) -> dst (a fresh NHWC tensor, or the slice given)."""
    _C.require_cuda(src)
    ps, ch, ss = pixel_rows(src)
    if dst is None:
        dst = empty_nhwc(src.shape[0], ch, src.shape[2], src.shape[3], src.device)
    _, cd, sd = pixel_rows(dst)
    assert dst.shape == src.shape
    _dw_launch("rr_channel_copy", 0.0, 8.0 * ps * ch, src, ss, dst, sd, ps, ch)
    return dst


def channel_join(lo, hi):
    """cat(lo, hi) along the channels in one launch -> a fresh NHWC tensor."""
    pl, half, sl = pixel_rows(lo)
    _, hh, sh = pixel_rows(hi)
    assert lo.shape == hi.shape
    n, _, h, w = lo.shape
    out = empty_nhwc(n, 2 * half, h, w, lo.device)
    _dw_launch("rr_channel_join", 0.0, 16.0 * pl * half, lo, sl, hi, sh, out, 2 * half, pl, half)
    return out


class _OpsModule(types.ModuleType):
    """`ops.BF16` (read / assign) = this thread's arithmetic switch."""

    @property
    def BF16(self):
        return _MODE.value

    @BF16.setter
    def BF16(self, v):
        _MODE.value = int(v or 0)


sys.modules[__name__].__class__ = _OpsModule
