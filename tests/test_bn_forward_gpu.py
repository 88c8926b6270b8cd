"""GPU: the forward half of the BatchNorm chain (csrc/elementwise.hip: bn_apply through rr_bn_apply / rr_bn_apply_amax /
rr_bn_apply_b16, bn_stats_finalize, bn_eval_coeffs) against float64 on the host, the ReLU-mask agreement between the forward,
the two backward passes that recompute the mask from y and the data-gradient epilogues that carry the BatchNorm sums, and the
fate of non-finite values in the forward ReLU.

Bounds are derived from the arithmetic, never read off the kernels (u = helpers.U32 = 2^-24):
 - bn_apply: v = fma(y, scale, shift) is ONE rounding, u |v| <= u (|y scale| + |shift|); the residual add is one more,
   u |v + r| <= u (|y scale| + |shift| + |r|) (1 + u); ReLU is 1-Lipschitz and exact.  Per element
   |out - ref| <= 2 u (|y scale| + |shift|) + u |r| + O(u^2) <= 3 u (|y scale| + |shift| + |r|) — asserted per ELEMENT, not as a
   global relative error.  Normalised as tests/kernel_audit.py does (max bound / max |ref|) it must not exceed the audit's
   2e-5, which is asserted for every case of at least 256 elements (a four-element ReLU output may be all zero).
 - a bf16 image is the float32 value rounded to nearest even: EQUAL to out.to(bfloat16) where the float32 output exists;
   against float64 |image - ref| <= half a bfloat16 ulp of out32 + |out32 - ref|.  bfloat16 keeps 8 significant bits: its ulp at
   v is 2^(floor(log2 |v|) - 7), so half an ulp is between 2^-9 |v| (just below a power of two) and 2^-8 |v| (just above one: 1 +
   2^-8 is a tie and rounds to 1).  A flat 2^-9 |v| is missed by a correct conversion by up to a factor 2 (measured 1.94 at the
   first run); the test asserts the half ulp itself, taken at |ref| + the float32 bound: helpers.bf16_half_ulp.
 - the word rr_bn_apply_amax publishes is the maximum of |out| itself (a maximum does not round): compared exactly.
 - ReLU edge (helpers.bn_mask_edge_inputs): the reference is exact, one fma returns its float32 rounding, the mask is its
   sign: every comparison is an equality; the sums over the masked gradient get tests/test_syncbn_gpu.py's bound for
   rr_bn_bwd_reduce (float32 partials over 8 pixels, double from there: 9 u sum|d| and 12 u sum|d xhat| + 2 u |mean| invstd
   sum|d|).  |dz| >= 0.5, so ONE element with the wrong mask moves sum d by at least 0.5: 4e5 times the bound.
 - bn_stats_finalize: the slab is summed in double in a fixed order ((mtiles + 8) 2^-53 of the sums of magnitudes, carried
   through var's cancellation and invstd's derivative like the convolution terms of test_syncbn_gpu._fwd_bounds); every
   output is then a float32 rounding of double arithmetic: mean u |m|, invstd u istd (both asserted at 2 u), scale =
   fl(gamma * fl(istd)): 2 u |scale|; shift = fl(beta - fl(fl(m) * scale32)): the product carries scale32's 2 u, fl(m)'s u and
   its own u, the subtraction u (|beta| + |m scale|): u |beta| + 5 u |m scale|; the running statistics 4 u per term
   (fl(1 - momentum), the float32 momentum, fl(m), the product and the final add).
 - bn_eval_coeffs: fl(var + eps) u, sqrtf and the division not assumed correctly rounded: 6 u |scale|, and
   6 u (|beta| + |mean scale|) for the shift.
Each test prints its figures (pytest -s)."""
import functools

import numpy as np
import pytest
import torch

from helpers import U32, bf16_exact, bf16_half_ulp, bn_apply_ref64, bn_mask_edge_inputs, nhwc_from_rows
from test_split_model_gpu import _Calls

pytestmark = pytest.mark.gpu
F32, BF16, F16X3 = 0, 1, 2
AUDIT_TOL = 2e-5
SENTINEL = -12345.0


def _h(t):
    return torch.as_tensor(t).detach().cpu().double()


class _Placed:
    """Operands as slices of larger sentinel-filled buffers: after the launch every buffer must be what it was."""

    def __init__(self):
        self.bufs = []

    def rows(self, a, as_image=False, off=8, tail=24):
        """[pixels, c] float32 array -> NHWC tensor [1, c, 1, pixels] inside a larger buffer (float32, or its bf16 image)."""
        dt = torch.bfloat16 if as_image else torch.float32
        big = torch.full((off + a.size + tail,), SENTINEL, dtype=dt, device="cuda")
        src = torch.from_numpy(np.ascontiguousarray(a)).cuda().to(dt).view(-1)
        big[off:off + a.size] = src
        self.bufs.append((big, big.clone()))
        p, c = a.shape
        return big[off:off + a.size].view(1, 1, p, c).permute(0, 3, 1, 2)

    def vec(self, a, off=4, tail=12):
        big = torch.full((off + a.size + tail,), SENTINEL, dtype=torch.float32, device="cuda")
        big[off:off + a.size] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.bufs.append((big, big.clone()))
        return big[off:off + a.size]

    def operand(self, a, phantom):
        from rrnet_amd import ops
        if not phantom:
            return self.rows(a)
        img = self.rows(a, as_image=True)
        assert torch.equal(img.float().cpu(), nhwc_from_rows(a))           # the values ARE bfloat16 values
        return ops.phantom_f32(tuple(img.shape), img.device, img)

    def untouched(self):
        # (bit patterns: a NaN planted in an operand must compare equal to itself)
        return all(torch.equal(big.view(torch.int16 if big.dtype == torch.bfloat16 else torch.int32),
                               was.view(torch.int16 if was.dtype == torch.bfloat16 else torch.int32)) for big, was in self.bufs)


def _rows_of(t):
    """NHWC tensor [1, c, 1, pixels] -> host [pixels, c] (dtype kept)."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).cpu()


# --------------------------------------------------------------------------------------------------------------------
# 1a. bn_apply against float64, every launch form
# --------------------------------------------------------------------------------------------------------------------
# shapes: (C, pixels).  plain: 1 quad / one pixel, one partial workgroup (< 256 quads), and more than 4096 x 256 quads (the grid
# cap of ew_blocks: the grid-stride loop wraps); amax / b16: both sides of ops._SPLIT_MIN_PIXELS / ops._CONV16_MIN_PIXELS
_B16 = "rr_bn_apply_b16"
APPLY_FORMS = {
    "plain": dict(mode=F32, entry=lambda px: "rr_bn_apply",
                  shapes=[(4, 1), (4, 77), (4, 1048583), (12, 1), (12, 67), (12, 349527), (64, 1), (64, 7), (64, 65603),
                          (384, 1), (384, 2), (384, 10930)]),
    "amax": dict(mode=F16X3, entry=lambda px: "rr_bn_apply_amax" if px >= 2048 else "rr_bn_apply", shapes=[(12, 2047), (12, 2048), (12, 2049)]),
    "b16": dict(mode=BF16, entry=lambda px: _B16 if px >= 8192 else "rr_bn_apply", shapes=[(128, 8191), (128, 8192)]),
    "only16": dict(mode=F32, entry=lambda px: _B16, shapes=[(12, 333), (128, 129)], only16=True),
    "y16": dict(mode=F32, entry=lambda px: _B16, shapes=[(12, 333), (128, 129)], y16=True),
    "res16": dict(mode=F32, entry=lambda px: _B16, shapes=[(12, 333), (128, 129)], r16=True),
    "y16-res16": dict(mode=F32, entry=lambda px: _B16, shapes=[(12, 333), (128, 129)], y16=True, r16=True),
    "y16-only16": dict(mode=BF16, entry=lambda px: _B16, shapes=[(20, 333)], y16=True, only16=True),
}
APPLY_CASES = [(form, c, px, relu, res) for form, cfg in APPLY_FORMS.items() for c, px in cfg["shapes"]
               for relu in (False, True) for res in (False, True) if res or not cfg.get("r16")]


@functools.lru_cache(maxsize=2)
def _apply_inputs(c, px, y16, r16):
    rng = np.random.default_rng(1000 * c + px)
    q = bf16_exact
    y = rng.normal(0.4, 1.3, (px, c)).astype(np.float32)
    r = rng.normal(0.0, 1.0, (px, c)).astype(np.float32)
    return (q(y) if y16 else y, q(r) if r16 else r, rng.normal(1.0, 0.3, c).astype(np.float32), rng.normal(0.0, 0.5, c).astype(np.float32))


def _check_against(tag, out32, img, ref, bound):
    """out32 / img: host [pixels, c] tensors (or None); ref, bound: float64 arrays.  -> printed figures."""
    fig = []
    ref_t, b_t = torch.from_numpy(ref), torch.from_numpy(bound)
    if ref.size >= 256:
        norm = float(b_t.max()) / float(ref_t.abs().max())
        assert norm <= AUDIT_TOL, (tag, norm)                      # no looser than the audit, normalised its way
        fig.append("bound/max|ref| %.1e" % norm)
    if out32 is not None:
        ratio = float(((out32.double() - ref_t).abs() / b_t).max())
        fig.append("fp32 worst %.3f of bound" % ratio)
        assert ratio <= 1.0, (tag, ratio)
    if img is not None:
        if out32 is not None:
            assert torch.equal(img, out32.to(torch.bfloat16)), tag + ": the image is not the float32 output rounded to nearest even"
            fig.append("image == RNE(out)")
        b16 = torch.from_numpy(bf16_half_ulp(np.abs(ref) + bound)) + b_t
        ratio = float(((img.double() - ref_t).abs() / b16).max())
        fig.append("image worst %.3f of its bound" % ratio)
        assert ratio <= 1.0, (tag, ratio)
    return fig


@pytest.mark.parametrize("form,c,px,relu,res", APPLY_CASES, ids=lambda v: str(int(v)) if isinstance(v, bool) else str(v))
def test_bn_apply_vs_fp64(form, c, px, relu, res):
    from rrnet_amd import ops
    cfg = APPLY_FORMS[form]
    y16, r16, only16 = cfg.get("y16", False), cfg.get("r16", False), cfg.get("only16", False)
    y, r, sc, sh = _apply_inputs(c, px, y16, r16)
    ref, mag = bn_apply_ref64(y, sc, sh, r if res else None, relu)
    place = _Placed()
    yd, rd = place.operand(y, y16), (place.operand(r, r16) if res else None)
    scd, shd = place.vec(sc), place.vec(sh)
    with ops.bf16_scope(cfg["mode"], force=True), _Calls() as calls:
        out = ops.bn_apply(yd, scd, shd, rd, relu, bf16_only=only16)
    torch.cuda.synchronize()
    entry = cfg["entry"](px)
    assert calls.n == {entry: 1}, (calls.n, entry)
    assert place.untouched(), "an operand buffer changed"
    assert ops.is_phantom(out) == only16 and tuple(out.shape) == (1, c, 1, px)
    img = ops.image_of(out) if only16 else ops.b16_carry(out)
    assert (img is not None) == (only16 or (form == "b16" and px >= 8192))
    tag = "%s C=%d pixels=%d relu=%d res=%d via %s" % (form, c, px, relu, res, entry)
    fig = _check_against(tag, None if only16 else _rows_of(out), None if img is None else _rows_of(img), ref, 3.0 * U32 * mag)
    if entry == "rr_bn_apply_amax":
        word = ops.amax_carry(out).view(torch.float32)[0]
        assert float(word) == float(out.abs().max()), (float(word), float(out.abs().max()))
        fig.append("published max|out| %.6e" % float(word))
    else:
        assert ops.amax_carry(out) is None
    print(tag + ": " + ", ".join(fig))


@pytest.mark.parametrize("relu", [False, True], ids=["norelu", "relu"])
@pytest.mark.parametrize("form,c,px", [("plain", 12, 333), ("plain", 64, 65603), ("res16", 128, 129)])
def test_bn_apply_residual_affine_vs_fp64(form, c, px, relu):
    """ops.bn_apply's res_scale / res_shift (no layer of rrnet_amd/ passes them, the audit's reference ignores them): out =
    relu?(y * scale + shift + (res * res_scale + res_shift)).  The residual's affine is a multiply and an add that the compiler
    may or may not contract: at most 2 u (|res res_scale| + |res_shift|); with the fma of y (u) and the final add (u of the
    sum): 3 u (|y scale| + |shift| + |res res_scale| + |res_shift|), second order carried by the factor 1 + 8 u."""
    from rrnet_amd import ops
    r16 = form == "res16"
    y, r, sc, sh = _apply_inputs(c, px, False, r16)
    rng = np.random.default_rng(c + px)
    rs, rh = rng.normal(1.0, 0.3, c).astype(np.float32), rng.normal(0.0, 0.5, c).astype(np.float32)
    r64 = r.astype(np.float64) * rs.astype(np.float64)[None, :]
    ref0, mag0 = bn_apply_ref64(y, sc, sh, None, False)
    ref = ref0 + r64 + rh.astype(np.float64)[None, :]
    ref = np.maximum(ref, 0.0) if relu else ref
    mag = mag0 + np.abs(r64) + np.abs(rh.astype(np.float64))[None, :]
    place = _Placed()
    yd, rd = place.rows(y), place.operand(r, r16)
    scd, shd, rsd, rhd = (place.vec(a) for a in (sc, sh, rs, rh))
    with ops.bf16_scope(F32, force=True), _Calls() as calls:
        out = ops.bn_apply(yd, scd, shd, rd, relu, rsd, rhd)
    entry = _B16 if r16 else "rr_bn_apply"
    assert calls.n == {entry: 1} and place.untouched()
    tag = "residual affine / %s C=%d pixels=%d relu=%d via %s" % (form, c, px, relu, entry)
    fig = _check_against(tag, _rows_of(out), None, ref, 3.0 * U32 * (1.0 + 8.0 * U32) * mag)
    plain, _ = bn_apply_ref64(y, sc, sh, r, relu)
    assert float(np.abs(plain - ref).max()) > 0.1             # the affine matters: ignoring it is far outside the bound
    print(tag + ": " + ", ".join(fig))


# --------------------------------------------------------------------------------------------------------------------
# 1b. ReLU-mask agreement on inputs that sit on the edge
# --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def _edge(c, px, bf16=False):
    return bn_mask_edge_inputs(7, c, px, bf16=bf16)


MASK_FWD_FORMS = {
    "plain": dict(mode=F32, c=64, px=4096, entry="rr_bn_apply"),
    "amax": dict(mode=F16X3, c=64, px=4096, entry="rr_bn_apply_amax"),
    "b16": dict(mode=BF16, c=128, px=8192, entry=_B16),
    "y16": dict(mode=BF16, c=64, px=4096, entry=_B16, y16=True),
    "y16-only16": dict(mode=BF16, c=64, px=4096, entry=_B16, y16=True, only16=True),
}


@pytest.mark.parametrize("form", sorted(MASK_FWD_FORMS))
def test_relu_edge_forward_is_the_rounded_exact_value(form):
    """bn_apply(relu=True) == float32(max(exact, 0)) element for element; its bf16 image is the RNE of that."""
    from rrnet_amd import ops
    cfg = MASK_FWD_FORMS[form]
    d = _edge(cfg["c"], cfg["px"], cfg.get("y16", False))
    want = torch.from_numpy(np.maximum(d["exact"], 0.0).astype(np.float32))          # one rounding to nearest even, as one fma
    place = _Placed()
    yd, scd, shd = place.operand(d["y"], cfg.get("y16", False)), place.vec(d["sc"]), place.vec(d["sh"])
    with ops.bf16_scope(cfg["mode"], force=True), _Calls() as calls:
        out = ops.bn_apply(yd, scd, shd, None, True, bf16_only=cfg.get("only16", False))
    assert calls.n == {cfg["entry"]: 1} and place.untouched()
    img = ops.image_of(out) if cfg.get("only16") else ops.b16_carry(out)
    assert (img is not None) == (form in ("b16", "y16-only16"))
    fig = []
    if not cfg.get("only16"):
        got = _rows_of(out)
        bad = int((got != want).sum())
        fig.append("%d of %d elements differ from float32(max(exact, 0)); %d are positive" % (bad, want.numel(), int((got > 0).sum())))
        assert bad == 0 and torch.equal(got > 0, torch.from_numpy(d["mask"]))
    if img is not None:
        bad = int((_rows_of(img).float() != want.to(torch.bfloat16).float()).sum())
        fig.append("image: %d differ from RNE of that" % bad)
        assert bad == 0
    if form == "amax":
        assert float(ops.amax_carry(out).view(torch.float32)[0]) == float(want.max())
    print("relu edge forward / %s via %s: %s" % (form, cfg["entry"], ", ".join(fig)))


MASK_BWD_FORMS = {
    "plain": dict(mode=F32, c=64, px=4096, entry="rr_bn_bwd_apply"),
    "gacc": dict(mode=F32, c=64, px=4096, entry="rr_bn_bwd_apply_gacc", g_into=True),
    "amax": dict(mode=F16X3, c=64, px=4096, entry="rr_bn_bwd_apply_amax"),
    "b16": dict(mode=BF16, c=128, px=8192, entry="rr_bn_bwd_apply_b16"),
    "image-input": dict(mode=BF16, c=64, px=4096, entry="rr_bn_bwd_apply_b16", y16=True),
    "image-input-c384": dict(mode=BF16, c=384, px=700, entry="rr_bn_bwd_apply_b16", y16=True),      # the un-hoisted loop of the HOIST kernel
}


def _stats_for(d, seed=3):
    rng = np.random.default_rng(seed)
    c = d["sc"].size
    return (rng.normal(0.0, 0.1, c).astype(np.float32), (1.0 / np.sqrt(rng.uniform(0.5, 1.5, c))).astype(np.float32),
            rng.normal(1.0, 0.3, c).astype(np.float32))


@pytest.mark.parametrize("form", sorted(MASK_BWD_FORMS))
def test_relu_edge_bwd_apply_masks_as_the_forward_did(form):
    """bn_bwd_apply(..., mask_scale, mask_shift, want_g) returns g EQUAL to dz * (exact > 0) (added to the fan-in buffer in the gacc
    form: one float32 addition, reproduced on the host)."""
    from rrnet_amd import ops
    cfg = MASK_BWD_FORMS[form]
    y16 = cfg.get("y16", False)
    d = _edge(cfg["c"], cfg["px"], y16)
    c, px = cfg["c"], cfg["px"]
    mean, invstd, gamma = _stats_for(d)
    place = _Placed()
    yd, dzd = place.operand(d["y"], y16), place.rows(d["dz"])
    scd, shd, md, isd, gd = (place.vec(a) for a in (d["sc"], d["sh"], mean, invstd, gamma))
    sums = torch.zeros(2 * c, dtype=torch.float64, device="cuda")
    base = np.random.default_rng(5).normal(0.0, 1.0, (px, c)).astype(np.float32) if cfg.get("g_into") else None
    g_into = nhwc_from_rows(base.copy()).cuda() if base is not None else None
    with ops.bf16_scope(cfg["mode"], force=True), _Calls() as calls:
        dx, g = ops.bn_bwd_apply(dzd, None, yd, md, isd, gd, sums, float(px), g_into is None, None, None, None, scd, shd, g_into=g_into)
    assert calls.n == {cfg["entry"]: 1}, calls.n
    assert place.untouched()
    masked = np.where(d["mask"], d["dz"], np.float32(0.0)).astype(np.float32)
    want = torch.from_numpy(masked if base is None else base + masked)
    got = _rows_of(g)
    bad = int((got != want).sum())
    print("relu edge bwd_apply / %s via %s: %d of %d elements of g differ from dz * (exact > 0); mask keeps %d"
          % (form, cfg["entry"], bad, want.numel(), int(d["mask"].sum())))
    assert bad == 0
    assert g_into is None or g.data_ptr() == g_into.data_ptr()
    assert bool(torch.isfinite(dx).all())


def _bwd_sums_check(tag, got, d64, y, mean, invstd):
    """got [2c] device doubles against the float64 sums of d64 [pixels, c] and d64 * xhat, at tests/test_syncbn_gpu.py's bound."""
    c = mean.size
    xh = (y.astype(np.float64) - mean.astype(np.float64)[None, :]) * invstd.astype(np.float64)[None, :]
    s1, s2 = d64.sum(0), (d64 * xh).sum(0)
    a1, a2 = np.abs(d64).sum(0), np.abs(d64 * xh).sum(0)
    b1 = 9 * U32 * a1
    b2 = 12 * U32 * a2 + 2 * U32 * np.abs(mean.astype(np.float64)) * invstd.astype(np.float64) * a1
    g = got.cpu().numpy()
    e1 = float((np.abs(g[:c] - s1) / np.maximum(b1, 1e-300)).max())
    e2 = float((np.abs(g[c:2 * c] - s2) / np.maximum(b2, 1e-300)).max())
    print("%s: sum d worst %.3f of bound, sum d*xhat worst %.3f of bound (the smallest |d| is %.3g times the largest bound of sum d)"
          % (tag, e1, e2, float(np.abs(d64[d64 != 0]).min()) / float(b1.max())))
    assert e1 <= 1.0 and e2 <= 1.0, (tag, e1, e2)


# img: 33001 pixels x 64 channels: 16 pixel lanes, the grid capped at 256 workgroups, so the first pass over 8 x 4096 pixels takes
# the batched eight-pixel branch in every lane and the second pass (232 pixels left) the tail branch
@pytest.mark.parametrize("inst,c,px", [("f32", 64, 4096), ("f32", 384, 700), ("img", 64, 4096), ("img", 64, 33001)])
def test_relu_edge_bwd_reduce_sums(inst, c, px):
    from rrnet_amd import ops
    y16 = inst == "img"
    d = _edge(c, px, y16)
    mean, invstd, _ = _stats_for(d)
    place = _Placed()
    yd, dzd = place.operand(d["y"], y16), place.rows(d["dz"])
    scd, shd, md, isd = (place.vec(a) for a in (d["sc"], d["sh"], mean, invstd))
    with ops.bf16_scope(BF16 if y16 else F32, force=True), _Calls() as calls:
        sums = ops.bn_bwd_reduce(dzd, None, yd, md, isd, mask_scale=scd, mask_shift=shd)
    assert calls.n == {"rr_bn_bwd_reduce_b16" if y16 else "rr_bn_bwd_reduce": 1} and place.untouched()
    d64 = np.where(d["mask"], d["dz"].astype(np.float64), 0.0)
    _bwd_sums_check("relu edge bwd_reduce / %s C=%d pixels=%d" % (inst, c, px), sums[:2 * c], d64, d["y"], mean, invstd)


# (n, c = k, h, w, lowered threshold): the first is the small layer, which reaches rr_conv_dgrad_s1_bnsum only with
# ops._DGRAD_VIA_FPROP_MIN_PIXELS lowered and there takes split-K, so the ENTRY's sums come from its reduce pass; the second fills
# 256 tiles of 128 rows: the sums come out of the convolution's epilogue itself (conv.hip, `rr_bn_affine(yv[q], ...) > 0`)
@pytest.mark.parametrize("n,c,h,w,lower", [(2, 64, 16, 16, True), (2, 64, 128, 128, False)], ids=["2x64x16x16-reduce-pass", "2x64x128x128-epilogue"])
def test_relu_edge_dgrad_epilogue_sums_fp32(n, c, h, w, lower):
    from rrnet_amd import ops
    _dgrad_edge(ops, n, c, h, w, c, F32, "rr_conv_dgrad_s1_bnsum", lower)


def test_relu_edge_dgrad_epilogue_sums_bf16():
    """The shape of test_conv_bf16_gpu.py::test_bf16_dgrad_carries_the_bn_backward_sums, on the kernel whose epilogue carries the sums."""
    from rrnet_amd import ops
    saved = ops._CONV16
    try:
        ops._CONV16 = False
        _dgrad_edge(ops, 2, 256, 64, 64, 256, BF16, "rr_conv_dgrad_s1_bnsum_bf16", False)
    finally:
        ops._CONV16 = saved


def _dgrad_edge(ops, n, c, h, w, k, mode, entry, lower):
    px = n * h * w
    d = _edge(c, px)
    mean, invstd, _ = _stats_for(d)
    g = torch.Generator().manual_seed(c + px)
    dy = ops.to_nhwc(torch.randn(n, k, h, w, generator=g).cuda())
    wt = ops.to_nhwc((torch.randn(k, c, 3, 3, generator=g) / np.sqrt(k * 9.0)).cuda())
    y = torch.from_numpy(d["y"]).cuda().view(n, h, w, c).permute(0, 3, 1, 2)
    link = ops.BnLink()
    link.y, link.mean, link.invstd = y, torch.from_numpy(mean).cuda(), torch.from_numpy(invstd).cuda()
    link.msc, link.msh = torch.from_numpy(d["sc"]).cuda(), torch.from_numpy(d["sh"]).cuda()
    saved = ops._DGRAD_VIA_FPROP_MIN_PIXELS
    try:
        if lower:
            ops._DGRAD_VIA_FPROP_MIN_PIXELS = 0
        with ops.bf16_scope(mode, force=True), _Calls() as calls:
            dx = ops.conv_dgrad(dy, wt, (n, c, h, w), 1, (1, 1), bnsum=link, bnsum_z=None)
    finally:
        ops._DGRAD_VIA_FPROP_MIN_PIXELS = saved
    assert calls.n.get(entry) == 1, calls.n
    assert link.sums is not None and link.dz is dx
    dx_rows = dx.permute(0, 2, 3, 1).reshape(px, c).cpu().double().numpy()
    assert np.isfinite(dx_rows).all() and float(np.abs(dx_rows).max()) > 0.1
    d64 = np.where(d["mask"], dx_rows, 0.0)            # the kernel's own gradient times the exact mask
    _bwd_sums_check("relu edge dgrad sums / %s %dx%dx%dx%d" % (entry, n, c, h, w), link.sums[:2 * c], d64, d["y"], mean, invstd)


# --------------------------------------------------------------------------------------------------------------------
# 1c. non-finite values stay visible
# --------------------------------------------------------------------------------------------------------------------
def _planted(c, px):
    rng = np.random.default_rng(17)
    clean = rng.normal(0.4, 1.3, (px, c)).astype(np.float32)
    flat = clean.copy().reshape(-1)
    n = flat.size
    spots = {}
    for base, vals in ((0, (np.nan, np.inf, -np.inf, np.nan)), (n - 4, (-np.inf, np.nan, np.inf, np.inf)), (n // 2 // 4 * 4 + 1, (np.nan, -np.inf, np.inf))):
        for i, v in enumerate(vals):
            flat[base + i] = v
            spots[base + i] = v
    return clean, flat.reshape(px, c), spots


def _check_planted(tag, got, clean_out, spots):
    got, clean_out = got.reshape(-1).float(), clean_out.reshape(-1).float()
    idx = torch.tensor(sorted(spots))
    for i, v in spots.items():
        o = float(got[i])
        assert (np.isnan(o) if np.isnan(v) else o == (np.inf if v > 0 else 0.0)), (tag, i, v, o)
    keep = torch.ones(got.numel(), dtype=torch.bool)
    keep[idx] = False
    assert torch.equal(got[keep], clean_out[keep]), tag + ": a planted value leaked into another element"
    print("%s: %d planted NaN stay NaN, %d +Inf stay +Inf, %d -Inf become 0; the other %d elements are unchanged"
          % (tag, sum(np.isnan(v) for v in spots.values()), sum(v == np.inf for v in spots.values()),
             sum(v == -np.inf for v in spots.values()), int(keep.sum())))


@pytest.mark.parametrize("form", ["plain", "amax", "only16", "b16"])
def test_bn_apply_relu_keeps_nan_and_inf(form):
    from rrnet_amd import ops
    c, px = (128, 8192) if form == "b16" else (12, 2500)
    clean, dirty, spots = _planted(c, px)
    rng = np.random.default_rng(2)
    sc, sh = (np.abs(rng.normal(1.0, 0.3, c)) + 0.1).astype(np.float32), rng.normal(0.0, 0.5, c).astype(np.float32)
    mode = {"plain": F32, "amax": F16X3, "only16": F32, "b16": BF16}[form]
    outs = []
    for a in (clean, dirty):
        place = _Placed()
        with ops.bf16_scope(mode, force=True), _Calls() as calls:
            out = ops.bn_apply(place.rows(a), place.vec(sc), place.vec(sh), None, True, bf16_only=form == "only16")
        assert calls.n == {{"plain": "rr_bn_apply", "amax": "rr_bn_apply_amax"}.get(form, _B16): 1} and place.untouched()
        outs.append(out)
    if form != "only16":
        _check_planted("bn_apply(relu) / " + form, _rows_of(outs[1]), _rows_of(outs[0]), spots)
    if form in ("only16", "b16"):
        imgs = [ops.image_of(o) if form == "only16" else ops.b16_carry(o) for o in outs]
        _check_planted("bn_apply(relu) bf16 image / " + form, _rows_of(imgs[1]), _rows_of(imgs[0]), spots)


def test_bn_apply_relu_keeps_a_nan_of_the_residual_and_of_the_statistics():
    """A NaN in one channel's scale / shift (a poisoned batch statistic) makes that whole channel NaN, not zero; a NaN of the
    residual stays where it is."""
    from rrnet_amd import ops
    c, px = 12, 300
    rng = np.random.default_rng(4)
    y, r = rng.normal(0.4, 1.3, (px, c)).astype(np.float32), rng.normal(0.0, 1.0, (px, c)).astype(np.float32)
    sc, sh = rng.normal(1.0, 0.3, c).astype(np.float32), rng.normal(0.0, 0.5, c).astype(np.float32)
    place = _Placed()
    clean = _rows_of(ops.bn_apply(place.rows(y), place.vec(sc), place.vec(sh), place.rows(r), True))
    r2, sc2, sh2 = r.copy(), sc.copy(), sh.copy()
    r2[7, 3] = np.nan
    sc2[5] = sh2[5] = np.nan
    got = _rows_of(ops.bn_apply(place.rows(y), place.vec(sc2), place.vec(sh2), place.rows(r2), True))
    assert bool(torch.isnan(got[:, 5]).all()) and bool(torch.isnan(got[7, 3]))
    keep = torch.ones(px, c, dtype=torch.bool)
    keep[:, 5] = False
    keep[7, 3] = False
    assert torch.equal(got[keep], clean[keep]) and place.untouched()
    print("bn_apply(relu): a NaN statistic poisons its %d-element channel visibly, a NaN of the residual stays" % px)


@pytest.mark.parametrize("c,px", [(4, 1), (12, 2500)])
def test_relu_fwd_keeps_nan_and_inf(c, px):
    from rrnet_amd import ops
    clean, dirty, spots = _planted(c, max(px, 3))
    if px == 1:               # one quad: NaN, +Inf, -Inf and a finite value
        clean = clean[:1].copy()
        clean[0, 3] = 0.75
        dirty, spots = np.array([[np.nan, np.inf, -np.inf, 0.75]], np.float32), {0: np.nan, 1: np.inf, 2: -np.inf}
    place = _Placed()
    with _Calls() as calls:
        outs = [ops.relu_fwd(place.rows(a)) for a in (clean, dirty)]
    assert calls.n == {"rr_relu_fwd": 2} and place.untouched()
    _check_planted("relu_fwd %d elements" % dirty.size, _rows_of(outs[1]), _rows_of(outs[0]), spots)


# --------------------------------------------------------------------------------------------------------------------
# 1d. bn_stats_finalize on synthetic slabs
# --------------------------------------------------------------------------------------------------------------------
EPS = 1e-5
EPS32 = float(np.float32(EPS))          # the entry point takes eps as a float: that is the value the kernel adds


def _finalize_ref_and_bounds(slab, count, gamma, beta, rm0, rv0, mom):
    """slab [mtiles, 2, C] float64, the rest float32 arrays.  -> (ref, bound) dicts of float64 arrays (module docstring)."""
    mt, _, c = slab.shape
    g, b = gamma.astype(np.float64), beta.astype(np.float64)
    s1, s2 = slab[:, 0, :].sum(0), slab[:, 1, :].sum(0)
    m = s1 / count
    var = np.maximum(s2 / count - m * m, 0.0)
    istd = 1.0 / np.sqrt(var + EPS32)
    sc = g * istd
    unb = var * count / (count - 1.0) if count > 1 else var
    ref = dict(mean=m, invstd=istd, scale=sc, shift=b - m * sc, running_mean=(1.0 - mom) * rm0.astype(np.float64) + mom * m,
               running_var=(1.0 - mom) * rv0.astype(np.float64) + mom * unb)
    dd = (mt + 8) * 2.0 ** -53                                      # the double summation and the few double operations behind it
    em = dd * np.abs(slab[:, 0, :]).sum(0) / count
    ev = dd * np.abs(slab[:, 1, :]).sum(0) / count + 2 * np.abs(m) * em + em * em + dd * m * m
    rel = ev / (var + EPS32)
    assert float(rel.max()) < 0.5
    d_istd = istd * 0.5 * rel * (1.0 - rel) ** -1.5
    fac = count / (count - 1.0) if count > 1 else 1.0
    bound = dict(mean=em + 2 * U32 * np.abs(m), invstd=d_istd + 2 * U32 * istd,
                 scale=np.abs(g) * d_istd + 2 * U32 * np.abs(sc),
                 shift=U32 * (np.abs(b) + 5 * np.abs(m * sc)) * (1 + 8 * U32) + np.abs(sc) * em + np.abs(m * g) * d_istd,
                 running_mean=4 * U32 * (np.abs((1 - mom) * rm0) + np.abs(mom * m)) + mom * em,
                 running_var=4 * U32 * (np.abs((1 - mom) * rv0) + mom * unb) + mom * ev * fac)
    return ref, bound


def _check_finalize(tag, got, ref, bound):
    worst = {}
    for name in ref:
        gv = _h(got[name]).numpy()
        assert np.isfinite(gv).all(), (tag, name)
        err = np.abs(gv - ref[name])
        worst[name] = float((err / np.maximum(bound[name], 1e-300)).max())
        norm = float(bound[name].max() / max(np.abs(ref[name]).max(), 1e-300))
        assert norm <= AUDIT_TOL, (tag, name, norm)
    print("%s: " % tag + ", ".join("%s %.2f of bound" % kv for kv in worst.items()))
    for name, ratio in worst.items():
        assert ratio <= 1.0, (tag, name, ratio)


def _finalize_twice(tag, slab, count, c, seed):
    from rrnet_amd import ops
    rng = np.random.default_rng(seed)
    gamma, beta = rng.normal(1.0, 0.3, c).astype(np.float32), rng.normal(0.0, 0.5, c).astype(np.float32)
    rm0, rv0 = rng.normal(0.0, 1.0, c).astype(np.float32), rng.uniform(0.5, 2.0, c).astype(np.float32)
    guard = 6
    store = torch.full((2, c + guard), SENTINEL, dtype=torch.float32, device="cuda")
    store[0, :c], store[1, :c] = torch.from_numpy(rm0).cuda(), torch.from_numpy(rv0).cuda()
    rm, rv = store[0, :c], store[1, :c]
    big = torch.full((slab.size + 10,), SENTINEL, dtype=torch.float64, device="cuda")
    big[4:4 + slab.size] = torch.from_numpy(slab.reshape(-1)).cuda()
    big0 = big.clone()
    sl = big[4:4 + slab.size]
    gd, bd = torch.from_numpy(gamma).cuda(), torch.from_numpy(beta).cuda()
    nbt = torch.tensor(41, dtype=torch.int64, device="cuda")
    prev_rm, prev_rv = rm0, rv0
    for call, mom in enumerate((0.1, 0.37)):
        with _Calls() as calls:
            mean, invstd, scale, shift = ops.bn_stats_finalize(sl, count, gd, bd, rm, rv, mom, EPS, nbt)
        assert calls.n == {"rr_bn_stats_finalize": 1}
        assert int(nbt) == 42 + call, int(nbt)
        assert torch.equal(big, big0) and bool((store[:, c:] == SENTINEL).all())
        got = dict(mean=mean, invstd=invstd, scale=scale, shift=shift, running_mean=rm.clone(), running_var=rv.clone())
        ref, bound = _finalize_ref_and_bounds(slab, count, gamma, beta, prev_rm, prev_rv, float(np.float32(mom)))
        _check_finalize("%s momentum %.2f" % (tag, mom), got, ref, bound)
        prev_rm, prev_rv = rm.cpu().numpy().copy(), rv.cpu().numpy().copy()
    return got, ref


@pytest.mark.parametrize("c", [1, 3, 12, 200])
@pytest.mark.parametrize("mtiles", [1, 31, 32, 33, 1000])
def test_bn_stats_finalize_on_synthetic_slabs(mtiles, c):
    """Random double slabs (tiles of 128 samples: sum y and sum y^2 of a channel of mean ~0.3 and variance in [0.5, 2]), no
    convolution in front; two calls (momentum 0.1, then 0.37 on the updated running statistics)."""
    rng = np.random.default_rng(100 * mtiles + c)
    mu, var = rng.normal(0.3, 0.5, c), rng.uniform(0.5, 2.0, c)
    slab = np.empty((mtiles, 2, c))
    slab[:, 0, :] = 128.0 * (mu[None, :] + rng.normal(0.0, 0.1, (mtiles, c)))
    slab[:, 1, :] = 128.0 * (mu[None, :] ** 2 + var[None, :] * rng.uniform(0.9, 1.1, (mtiles, c)) + 0.05)
    _finalize_twice("stats_finalize mtiles=%d C=%d" % (mtiles, c), slab, 128.0 * mtiles, c, mtiles + c)


def test_bn_stats_finalize_count_one_and_negative_variance():
    """count = 1: the unbiased factor count / (count - 1) is guarded (running_var moves towards the biased variance, 0).
    A channel whose sum y^2 / n - mean^2 comes out negative in float64 is clamped: invstd = 1 / sqrt(eps), not NaN."""
    c = 12
    rng = np.random.default_rng(9)
    yv = rng.normal(0.3, 1.0, c)
    slab = np.stack([yv, yv * yv])[None]                            # one tile, one sample
    got, ref = _finalize_twice("stats_finalize count=1", slab, 1.0, c, 1)
    assert np.array_equal(ref["invstd"], np.full(c, 1.0 / np.sqrt(EPS32)))
    assert torch.equal(got["invstd"].cpu(), torch.full((c,), float(np.float32(1.0 / np.sqrt(EPS32)))))
    n, mt = 4096.0, 32
    mu = rng.normal(2.0, 0.5, c)
    slab = np.empty((mt, 2, c))
    slab[:, 0, :] = (n / mt) * mu[None, :]
    slab[:, 1, :] = (n / mt) * (mu[None, :] ** 2) * (1.0 - 1e-9)    # sum y^2 / n - mean^2 = -1e-9 mean^2 < 0
    slab[:, 1, 0] = (n / mt) * (mu[0] ** 2 + 1.0)                   # (channel 0: an ordinary one next to them)
    raw = slab[:, 1, :].sum(0) / n - (slab[:, 0, :].sum(0) / n) ** 2
    assert (raw[1:] < 0).all() and raw[0] > 0.9
    got, ref = _finalize_twice("stats_finalize negative variance", slab, n, c, 2)
    assert torch.equal(got["invstd"].cpu()[1:], torch.full((c - 1,), float(np.float32(1.0 / np.sqrt(EPS32)))))


# --------------------------------------------------------------------------------------------------------------------
# 1e. bn_eval_coeffs
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 12, 200, 1024])
def test_bn_eval_coeffs_vs_fp64(c):
    from rrnet_amd import ops
    rng = np.random.default_rng(c)
    gamma, beta = rng.normal(1.0, 0.3, c).astype(np.float32), rng.normal(0.0, 0.5, c).astype(np.float32)
    rm = rng.normal(0.0, 1.0, c).astype(np.float32)
    rv = (10.0 ** rng.uniform(-6.0, 3.0, c)).astype(np.float32)
    rv[0] = np.float32(1e-6)
    rv[-1] = np.float32(1e3)
    place = _Placed()
    with _Calls() as calls:
        scale, shift = ops.bn_eval_coeffs(place.vec(gamma), place.vec(beta), place.vec(rm), place.vec(rv), EPS)
    assert calls.n == {"rr_bn_eval_coeffs": 1} and place.untouched() and scale.numel() == shift.numel() == c
    sc = gamma.astype(np.float64) / np.sqrt(rv.astype(np.float64) + EPS32)
    sf = beta.astype(np.float64) - rm.astype(np.float64) * sc
    b_sc, b_sf = 6 * U32 * np.abs(sc), 6 * U32 * (np.abs(beta.astype(np.float64)) + np.abs(rm.astype(np.float64) * sc))
    e1 = float((np.abs(_h(scale).numpy() - sc) / b_sc).max())
    e2 = float((np.abs(_h(shift).numpy() - sf) / b_sf).max())
    assert float(b_sc.max() / np.abs(sc).max()) <= AUDIT_TOL and float(b_sf.max() / np.abs(sf).max()) <= AUDIT_TOL
    print("bn_eval_coeffs C=%d (running_var %.1e .. %.1e): scale worst %.3f of 6u|scale|, shift worst %.3f of 6u(|beta| + |mean scale|)"
          % (c, float(rv.min()), float(rv.max()), e1, e2))
    assert e1 <= 1.0 and e2 <= 1.0
