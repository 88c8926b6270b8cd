"""GPU: the gradient fan-in sum, the stand-alone ReLU, the hourglass up path (nearest-2x up-sample + bilinear resize + add, forward
and backward), the channel padding and the two bf16 conversions of csrc/elementwise.hip against float64 / exact references.

Bounds, derived from the arithmetic (u = helpers.U32 = 2^-24):
 - sum_n adds g_0 .. g_{n-1} one after the other in float32: n - 1 roundings, each at most u times a partial sum that does not
   exceed sum|g_i|: (n - 1) u sum|g_i| per element; the mask (z > 0) is a select: where z <= 0 (-0.0 and 0 included) the result
   is exactly 0.  relu_fwd is a select: EQUAL to torch.relu on finite data.
 - up path, sizes 2 LH x 2 LW: out = up1 + low[h / 2, w / 2], one rounding: u |a + b|, asserted at 2 u |a + b|; bf16 images as in
   tests/test_bn_forward_gpu.py (EQUAL to the rounded float32 output where both exist; against float64 half a bfloat16 ulp on top of the float32
   bound).  Backward: dlow = the sum of a 2x2 block in float32, three additions: 3 u sum|terms|.
 - up path, general kernel: sample (h, w) of the output reads the nearest-2x image U (UH = 2 LH rows) at fy = sy h with
   sy = fl((UH - 1) / (H - 1)) and the product rounded again: |fy - exact| <= 3 u (UH - 1) (the division is not assumed to be
   correctly rounded); fy - floor(fy) is exact in float32.  The interpolant is continuous and piecewise linear with slope
   at most the largest difference of two neighbouring samples, so the position error moves the value by at most
   3 u ((UH - 1) Dy + (UW - 1) Dx), Dy / Dx the largest neighbour differences in the footprint (taken over the 2x2 cell
   widened by one sample on every side: a position within rounding of an integer may land in the next cell).  The arithmetic:
   1 - ly, 1 - lx (u each), two products and a sum per row (3 u), times the row weight, the sum of the rows and the final
   add of up1: at most 8 roundings on any path: 8 u (|up1| + sum w_i |v_i|).
   Backward: every output adds g * wy * wx to four elements of dlow with float atomics (arbitrary order): K contributions meet
   in an element in K - 1 roundings, K u sum|terms|.  For the shapes below sy and sx are 1 or 1.25: every weight is a multiple of
   1/4 and exact, the position error is zero, and only the accumulation rounds.
 - rr_pad_channels, rr_to_bf16 (round to nearest even), rr_from_bf16: exact."""
import functools

import numpy as np
import pytest
import torch

from helpers import U32, bf16_crafted_vector, bf16_exact, bf16_half_ulp, upsample_add_ref64
from test_split_model_gpu import _Calls

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
AUDIT_TOL = 2e-5
BIG = 4 * (4096 * 256 + 1)          # one quad more than the grid cap of ew_blocks covers in one pass: the grid-stride loop wraps


def _nhwc(a):
    """[n, h, w, c] array -> device tensor of logical shape [n, c, h, w] over that memory."""
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().permute(0, 3, 1, 2)


def _rows(t):
    """NHWC-memory tensor [n, c, h, w] -> host [n, h, w, c]."""
    return t.permute(0, 2, 3, 1).contiguous().cpu()


# --------------------------------------------------------------------------------------------------------------------
# sum_n, relu_fwd
# --------------------------------------------------------------------------------------------------------------------
SUM_SHAPES = {"4d-4": (1, 1, 1, 4), "4d-1020": (1, 5, 17, 12), "flat-1020": (1020,), "flat-wrap": (BIG,)}


@functools.lru_cache(maxsize=1)
def _sum_inputs(shape):
    rng = np.random.default_rng(int(np.prod(shape)))
    gs = [(rng.normal(0.0, 1.0, shape) * 10.0 ** rng.integers(-2, 3)).astype(np.float32) for _ in range(8)]
    z = rng.normal(0.0, 1.0, shape).astype(np.float32)
    pick = rng.random(shape)
    z[pick < 0.1] = 0.0
    z[pick < 0.05] = -0.0
    return gs, z


@pytest.mark.parametrize("with_z", [False, True], ids=["noz", "z"])
@pytest.mark.parametrize("n", [1, 2, 3, 8])
@pytest.mark.parametrize("shape", sorted(SUM_SHAPES))
def test_sum_n_vs_fp64(shape, n, with_z):
    from rrnet_amd import ops
    shp = SUM_SHAPES[shape]
    gs, z = _sum_inputs(shp)
    dev = (lambda a: _nhwc(a)) if len(shp) == 4 else (lambda a: torch.from_numpy(a).cuda())
    gd, zd = [dev(g) for g in gs[:n]], (dev(z) if with_z else None)
    keep, zkeep = [g.clone() for g in gd], (zd.clone() if with_z else None)
    with _Calls() as calls:
        out = ops.sum_n(gd, zd)
    assert calls.n == {"rr_sum_n": 1} and out.shape == gd[0].shape and out.stride() == gd[0].stride()
    assert all(torch.equal(g, was) for g, was in zip(gd, keep)) and (zd is None or torch.equal(zd, zkeep))
    got = (_rows(out) if len(shp) == 4 else out.cpu()).double().numpy()
    ref = np.sum([g.astype(np.float64) for g in gs[:n]], axis=0)
    mag = np.sum([np.abs(g.astype(np.float64)) for g in gs[:n]], axis=0)
    if with_z:
        dead = ~(z > 0)
        assert dead.sum() > 0 and (got[dead] == 0.0).all(), "an element with z <= 0 is not exactly zero"
        ref, mag = np.where(dead, 0.0, ref), np.where(dead, 0.0, mag)
    bound = (n - 1) * U32 * mag
    err = np.abs(got - ref)
    assert (err <= bound).all(), (shape, n, with_z, float((err - bound).max()))
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if n > 1 else 0.0
    norm = float(bound.max() / max(np.abs(ref).max(), 1e-300))
    assert ref.size < 256 or norm <= AUDIT_TOL, norm
    print("sum_n %s n=%d z=%d: worst %.3f of the (n-1) u sum|g_i| bound%s (bound / max|ref| %.1e)"
          % (shape, n, with_z, ratio, ", n = 1 is a copy: exact" if n == 1 else "", norm))


def test_sum_n_refuses_nine_inputs():
    from rrnet_amd import _C, ops
    gs = [torch.ones(8, device="cuda") for _ in range(9)]
    with pytest.raises(_C.RRNetHipError):
        ops.sum_n(gs)
    assert float(ops.sum_n(gs[:8]).sum()) == 64.0


@pytest.mark.parametrize("shape", sorted(SUM_SHAPES))
def test_relu_fwd_equals_torch_relu(shape):
    from rrnet_amd import ops
    shp = SUM_SHAPES[shape]
    gs, z = _sum_inputs(shp)
    x = _nhwc(z) if len(shp) == 4 else torch.from_numpy(z).cuda()
    keep = x.clone()
    with _Calls() as calls:
        out = ops.relu_fwd(x)
    assert calls.n == {"rr_relu_fwd": 1} and out.stride() == x.stride() and torch.equal(x, keep)
    assert torch.equal(out, torch.relu(x)) and torch.equal(out.cpu(), torch.relu(x.cpu()))
    assert not bool(torch.signbit(out[x == 0]).any())                 # -0.0 comes out as +0.0, as before
    print("relu_fwd %s: %d elements equal torch.relu (%d zeros in, -0.0 among them)" % (shape, out.numel(), int((x == 0).sum())))


# --------------------------------------------------------------------------------------------------------------------
# up path, exact 2x sizes: rr_upsample_add_fwd's fast kernel and rr_upsample2x_add_b16
# --------------------------------------------------------------------------------------------------------------------
F32, BF16 = 0, 1
UP_FAST_SHAPES = [(1, 4, 2, 2), (2, 12, 6, 10), (1, 128, 64, 64)]
# (up1 bf16-only, low bf16-only, output kind)
UP_FAST_KINDS = [(False, False, "f32"), (True, False, "f32"), (False, True, "f32"), (True, True, "f32"), (False, False, "only16"),
                 (True, True, "only16")]
UP_FAST_CASES = [(s, k) for s in UP_FAST_SHAPES for k in UP_FAST_KINDS] + [((2, 128, 64, 64), (True, False, "f32+image")),
                                                                           ((2, 128, 64, 64), (False, True, "f32+image"))]


def _phantom(ops, a):
    img = _nhwc(a).to(torch.bfloat16)
    assert torch.equal(img.float().cpu(), torch.from_numpy(a).permute(0, 3, 1, 2))
    return ops.phantom_f32(tuple(img.shape), img.device, img)


@pytest.mark.parametrize("shape,kind", UP_FAST_CASES, ids=lambda v: "%s-u%d-l%d" % (v[2], v[0], v[1]) if isinstance(v[0], bool) else "x".join(map(str, v)))
def test_upsample_add_fwd_fast_path_vs_fp64(shape, kind):
    from rrnet_amd import ops
    n, c, h, w = shape
    u16, l16, outkind = kind
    rng = np.random.default_rng(n * c * h * w)
    up1, low = rng.normal(0.0, 1.0, (n, h, w, c)).astype(np.float32), rng.normal(0.3, 1.0, (n, h // 2, w // 2, c)).astype(np.float32)
    up1, low = (bf16_exact(up1) if u16 else up1), (bf16_exact(low) if l16 else low)
    ud, ld = (_phantom(ops, up1) if u16 else _nhwc(up1)), (_phantom(ops, low) if l16 else _nhwc(low))
    with ops.bf16_scope(BF16 if outkind == "f32+image" else F32, force=True), _Calls() as calls:
        out = ops.upsample_add_fwd(ud, ld, bf16_only=outkind == "only16")
    entry = "rr_upsample_add_fwd" if not (u16 or l16 or outkind == "only16") else "rr_upsample2x_add_b16"
    assert calls.n == {entry: 1}, calls.n
    ref = up1.astype(np.float64) + np.repeat(np.repeat(low.astype(np.float64), 2, axis=1), 2, axis=2)
    ref_t = upsample_add_ref64(torch.from_numpy(up1).permute(0, 3, 1, 2), torch.from_numpy(low).permute(0, 3, 1, 2))
    assert torch.equal(ref_t.permute(0, 2, 3, 1), torch.from_numpy(ref)), "the composition is not the plain 2x copy at these sizes"
    bound = 2 * U32 * np.abs(ref)
    assert float(bound.max() / np.abs(ref).max()) <= AUDIT_TOL
    img = ops.image_of(out) if outkind == "only16" else ops.b16_carry(out)
    assert ops.is_phantom(out) == (outkind == "only16") and (img is not None) == (outkind != "f32")
    fig = []
    if outkind != "only16":
        got = _rows(out).double().numpy()
        err = np.abs(got - ref)
        assert (err <= bound).all()
        fig.append("fp32 worst %.3f of 2u|a+b|" % float((err[bound > 0] / bound[bound > 0]).max()))
    if img is not None:
        if outkind != "only16":
            assert torch.equal(img, out.to(torch.bfloat16)), "the image is not the float32 output rounded to nearest even"
            fig.append("image == RNE(out)")
        b16 = bf16_half_ulp(np.abs(ref) + bound) + bound
        e16 = np.abs(_rows(img).double().numpy() - ref)
        assert (e16 <= b16).all()
        fig.append("image worst %.3f of its bound" % float((e16[b16 > 0] / b16[b16 > 0]).max()))
    print("upsample_add_fwd %s up1 %s low %s -> %s via %s: %s" % (shape, "bf16" if u16 else "fp32", "bf16" if l16 else "fp32", outkind, entry, ", ".join(fig)))


@pytest.mark.parametrize("shape", UP_FAST_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_upsample_add_bwd_fast_path_vs_fp64(shape):
    from rrnet_amd import ops
    n, c, h, w = shape
    rng = np.random.default_rng(7 + n * c * h * w)
    dout = rng.normal(0.0, 1.0, (n, h, w, c)).astype(np.float32)
    dd = _nhwc(dout)
    with _Calls() as calls:
        dlow = ops.upsample_add_bwd(dd, (n, c, h // 2, w // 2))
    assert calls.n == {"rr_upsample_add_bwd": 1} and tuple(dlow.shape) == (n, c, h // 2, w // 2)
    low = torch.zeros(n, c, h // 2, w // 2, dtype=torch.float64, requires_grad=True)
    upsample_add_ref64(torch.zeros(n, c, h, w, dtype=torch.float64), low).backward(torch.from_numpy(dout).permute(0, 3, 1, 2).double())
    ref = low.grad.permute(0, 2, 3, 1).numpy()
    a = np.abs(dout.astype(np.float64))
    mag = a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2]
    err, bound = np.abs(_rows(dlow).double().numpy() - ref), 3 * U32 * mag
    assert (err <= bound).all() and float(bound.max() / np.abs(ref).max()) <= AUDIT_TOL
    print("upsample_add_bwd fast %s: worst %.3f of 3u sum|terms|" % (shape, float((err / bound).max())))


# --------------------------------------------------------------------------------------------------------------------
# up path, general kernel (odd sizes, or C % 4 != 0)
# --------------------------------------------------------------------------------------------------------------------
# name -> (N, C, LH, LW, H, W, backward too).  The last one has inexact scales (7/6): forward only, see the module docstring
UP_GENERAL = {"odd-3x3-to-5x5": (2, 8, 3, 3, 5, 5, True), "mixed-3x3-to-6x5": (2, 8, 3, 3, 6, 5, True),
              "identity-c6-3x4-to-6x8": (2, 6, 3, 4, 6, 8, True), "inexact-scale-4x4-to-7x7": (1, 4, 4, 4, 7, 7, False)}


def _general_inputs(name):
    n, c, lh, lw, h, w, _ = UP_GENERAL[name]
    rng = np.random.default_rng(len(name) + c * h * w)
    return rng.normal(0.0, 1.0, (n, h, w, c)).astype(np.float32), rng.normal(0.3, 1.0, (n, lh, lw, c)).astype(np.float32)


def _position_term(low, h, w):
    """3 u ((UH - 1) Dy + (UW - 1) Dx) per output [n, h, w, c]: module docstring."""
    n, lh, lw, c = low.shape
    up = np.repeat(np.repeat(low.astype(np.float64), 2, axis=1), 2, axis=2)
    uh, uw = 2 * lh, 2 * lw
    out = np.zeros((n, h, w, c))
    for i in range(h):
        y0 = int(np.floor(i * (uh - 1) / (h - 1))) if h > 1 else 0
        ys = slice(max(y0 - 1, 0), min(y0 + 3, uh))
        for j in range(w):
            x0 = int(np.floor(j * (uw - 1) / (w - 1))) if w > 1 else 0
            win = up[:, ys, max(x0 - 1, 0):min(x0 + 3, uw), :]
            dy = np.abs(np.diff(win, axis=1)).max(axis=(1, 2)) if win.shape[1] > 1 else 0.0
            dx = np.abs(np.diff(win, axis=2)).max(axis=(1, 2)) if win.shape[2] > 1 else 0.0
            out[:, i, j, :] = 3 * U32 * ((uh - 1) * dy + (uw - 1) * dx)
    return out


@pytest.mark.parametrize("name", sorted(UP_GENERAL))
def test_upsample_add_fwd_general_path_vs_fp64(name):
    from rrnet_amd import ops
    n, c, lh, lw, h, w, _ = UP_GENERAL[name]
    up1, low = _general_inputs(name)
    t = lambda a: torch.from_numpy(a).permute(0, 3, 1, 2)
    with _Calls() as calls:
        out = ops.upsample_add_fwd(_nhwc(up1), _nhwc(low))
    assert calls.n == {"rr_upsample_add_fwd": 1}
    ref = upsample_add_ref64(t(up1), t(low)).permute(0, 2, 3, 1).numpy()
    mag = upsample_add_ref64(t(np.abs(up1)), t(np.abs(low))).permute(0, 2, 3, 1).numpy()         # weights >= 0: |up1| + sum w_i |v_i|
    arith, pos = 8 * U32 * mag, _position_term(low, h, w)
    bound = arith + pos
    err = np.abs(_rows(out).double().numpy() - ref)
    assert float(bound.max() / np.abs(ref).max()) <= AUDIT_TOL
    print("upsample_add_fwd general %s: worst %.3f of bound (arithmetic term up to %.1e, position term up to %.1e)"
          % (name, float((err / bound).max()), float(arith.max()), float(pos.max())))
    assert (err <= bound).all()
    if name.startswith("identity"):           # the bilinear resize is the identity at equal sizes: the plain 2x copy, one rounding
        plain = up1.astype(np.float64) + np.repeat(np.repeat(low.astype(np.float64), 2, axis=1), 2, axis=2)
        assert (np.abs(_rows(out).double().numpy() - plain) <= U32 * np.abs(plain)).all()


def _contributions(lh, lw, h, w):
    """How many of the kernel's atomics land in each element of dlow [lh, lw]: four per output, zero weights included.  (Exact
    floors: the scales of the shapes that use this are 1 or 1.25.)"""
    uh, uw = 2 * lh, 2 * lw
    k = np.zeros((lh, lw))
    for i in range(h):
        y0 = i * (uh - 1) // (h - 1)
        y1 = y0 + (1 if y0 < uh - 1 else 0)
        for j in range(w):
            x0 = j * (uw - 1) // (w - 1)
            x1 = x0 + (1 if x0 < uw - 1 else 0)
            for yy in (y0, y1):
                for xx in (x0, x1):
                    k[yy // 2, xx // 2] += 1
    return k


@pytest.mark.parametrize("name", sorted(k for k, v in UP_GENERAL.items() if v[6]))
def test_upsample_add_bwd_general_path_vs_fp64(name):
    """Against the float64 autograd of the composition; run twice into a dirty dlow: the result must not depend on what the
    buffer held (the entry zero-fills it before the atomics)."""
    from rrnet_amd import _C, ops
    n, c, lh, lw, h, w, _ = UP_GENERAL[name]
    rng = np.random.default_rng(3 + len(name))
    dout = rng.normal(0.0, 1.0, (n, h, w, c)).astype(np.float32)
    g64 = torch.from_numpy(dout).permute(0, 3, 1, 2).double()

    def autograd(g):
        low = torch.zeros(n, c, lh, lw, dtype=torch.float64, requires_grad=True)
        upsample_add_ref64(torch.zeros(n, c, h, w, dtype=torch.float64), low).backward(g)
        return low.grad.permute(0, 2, 3, 1).numpy()
    ref, mag = autograd(g64), autograd(g64.abs())                                    # weights >= 0: sum|terms|
    contrib = _contributions(lh, lw, h, w)[None, :, :, None]
    dd = _nhwc(dout)
    with _Calls() as calls:
        first = ops.upsample_add_bwd(dd, (n, c, lh, lw))
    assert calls.n == {"rr_upsample_add_bwd": 1}
    store = torch.full((n * lh * lw * c + 16,), SENTINEL, dtype=torch.float32, device="cuda")
    dirty = store[8:8 + n * lh * lw * c]
    results = [_rows(first).double().numpy()]
    for fill in (SENTINEL, float("nan")):
        dirty.fill_(fill)
        _C.check(_C.fn("rr_upsample_add_bwd")(_C.ptr(dd), _C.ptr(dirty), n, h, w, lh, lw, c, _C.stream()), "rr_upsample_add_bwd")
        results.append(dirty.view(n, lh, lw, c).cpu().double().numpy())
        assert bool((store[:8] == SENTINEL).all()) and bool((store[8 + n * lh * lw * c:] == SENTINEL).all())
    bound = contrib * U32 * mag
    assert float(bound.max() / np.abs(ref).max()) <= AUDIT_TOL
    worst = max(float((np.abs(r - ref) / bound).max()) for r in results)
    print("upsample_add_bwd general %s: worst %.3f of K u sum|terms| over three runs (K up to %d)" % (name, worst, int(contrib.max())))
    for r in results:
        assert np.isfinite(r).all() and (np.abs(r - ref) <= bound).all()


# --------------------------------------------------------------------------------------------------------------------
# rr_pad_channels
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npix", [1, 513, 70001])
@pytest.mark.parametrize("k", [1, 2, 10, 34, 36])
def test_pad_channels_copies_and_zero_fills(k, npix):
    from rrnet_amd import _C
    kp = (k + 3) // 4 * 4
    rng = np.random.default_rng(k * npix)
    src = torch.from_numpy(rng.normal(0.0, 1.0, (npix, k)).astype(np.float32)).cuda()
    src[0, 0] = -0.0
    keep = src.clone()
    guard = 12
    store = torch.full((npix * kp + guard,), SENTINEL, dtype=torch.float32, device="cuda")
    with _Calls() as calls:
        _C.check(_C.fn("rr_pad_channels")(_C.ptr(src), _C.ptr(store), npix, k, kp, _C.stream()), "rr_pad_channels")
    assert calls.n == {"rr_pad_channels": 1}
    dst = store[:npix * kp].view(npix, kp)
    assert torch.equal(dst[:, :k].view(torch.int32), keep.view(torch.int32)), "not a bit copy"
    assert torch.equal(src, keep) and bool((dst[:, k:] == 0).all()) and not bool(torch.signbit(dst[:, k:]).any())
    assert bool((store[npix * kp:] == SENTINEL).all()), "wrote past the destination"
    print("pad_channels k=%d -> %d, %d pixels: exact copy, %d zero tail elements, guard intact" % (k, kp, npix, npix * (kp - k)))


# --------------------------------------------------------------------------------------------------------------------
# bf16_of / f32_of
# --------------------------------------------------------------------------------------------------------------------
def test_bf16_conversions_round_to_nearest_even_like_torch():
    """ops.bf16_of (rr_to_bf16) == torch's CPU .to(bfloat16) and ops.f32_of (rr_from_bf16) == .float() on ties (kept mantissa even
    and odd), one float32 ulp either side of them, +-0, +-Inf, NaN (stays NaN), the largest finite float32 (rounds to Inf) and
    random normals of three magnitudes.  float32 SUBNORMALS are left out: whether they are flushed is a mode setting of the
    device, not a property of these kernels."""
    from rrnet_amd import ops
    v = bf16_crafted_vector()
    assert v.size % 4 == 0 and np.isnan(v).sum() >= 3 and np.isinf(v).sum() >= 2
    x = torch.from_numpy(v)
    want = x.to(torch.bfloat16)
    assert bool(torch.isinf(want[x == torch.finfo(torch.float32).max]).all())
    xd = x.cuda().view(1, 1, v.size // 4, 4).permute(0, 3, 1, 2)
    with _Calls() as calls:
        img = ops.bf16_of(xd)
        again = ops.bf16_of(xd)
    assert calls.n == {"rr_to_bf16": 1} and again is img and img.dtype == torch.bfloat16 and img.stride() == xd.stride()
    got = img.permute(0, 2, 3, 1).reshape(-1).cpu()
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan) and int(nan.sum()) == int(np.isnan(v).sum())
    assert torch.equal(got[~nan].view(torch.int16), want[~nan].view(torch.int16)), "not the round-to-nearest-even image, bit for bit"
    ph = ops.phantom_f32(tuple(img.shape), img.device, img)
    with _Calls() as calls:
        back = ops.f32_of(ph)
    assert calls.n == {"rr_from_bf16": 1} and back.dtype == torch.float32
    b = back.permute(0, 2, 3, 1).reshape(-1).cpu()
    assert torch.equal(torch.isnan(b), nan) and torch.equal(b[~nan].view(torch.int32), want.float()[~nan].view(torch.int32))
    # bf16-exact data survives the round trip unchanged
    e = bf16_exact(v[np.isfinite(v)][: np.isfinite(v).sum() // 4 * 4])
    ed = torch.from_numpy(e).cuda().view(1, 1, e.size // 4, 4).permute(0, 3, 1, 2)
    rt = ops.f32_of(ops.phantom_f32(tuple(ed.shape), ed.device, ops.bf16_of(ed)))
    assert torch.equal(rt.view(torch.int32), ed.view(torch.int32))
    print("bf16_of / f32_of: %d crafted values (%d NaN, %d Inf) equal torch's conversions; round trip of %d bf16 values is the identity"
          % (v.size, int(nan.sum()), int(np.isinf(v).sum()), e.size))
