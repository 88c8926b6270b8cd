"""GPU: the tile epilogue of conv_igemm_kernel (rrnet_amd/csrc/conv.hip) — store, accumulate, split-K atomics, the parity
and position-major pixel mappings, the fused statistics — through the library's entry points, on shapes with ragged row
and column tiles.

The epilogue addresses the destination through a buffer descriptor and lets the hardware drop the lanes outside the tensor,
so every destination here lies INSIDE a larger allocation, between two sentinel bands of at least one tile (128 rows x DC
floats) that must come back bit for bit.  Values are judged by the rule of tests/test_conv_fp64_gpu.py (conv_error_ratios /
conv_accepts with CONV_MARGIN against conv_ref64); a slab or `sums` against the float64 column sums of the kernel's own
output, by the bounds of that file's _check_slab.

Shapes (reduction below 16 K-steps except SPLIT: pick_ksplit keeps split-K off, every launch costs milliseconds at most).
For the tile cases `cin` is the reduction's channel count and `cols` the GEMM's N = the destination's channel count, in the
forward pass AND in the data gradients (there the forward layer runs cols -> cin channels):
  T128   8 -> 136 columns on one 79 x 81 map: 6399 rows = 50 row tiles with a ragged last one, a second column tile of 8
  T72    8 -> 72 columns on one 37 x 35 map: 11 ragged row tiles; 11 tiles <= small_tiles(), so the host narrows the tile to 32
  T40    8 -> 40 columns on one 9 x 13 map: one ragged row tile; 33..64 columns take the 64-column tile
  T72M   8 -> 72 columns on one 53 x 51 map: 22 row tiles <= mid_tiles(): the 128-column tile narrowed to 64, ragged second tile
  SPLIT  tests/test_conv_fp64_gpu.py's SHAPE_A: split-K atomics in both passes
  PARITY that file's SHAPE_B (stride 2, odd 7 x 9 map) and its mirror with 24 destination columns
  POSM   2048 maps of 3 x 3, 64 -> 64: position-major tiles"""
import functools

import numpy as np
import pytest
import torch

from helpers import (CONV_MARGIN, U32, conv_accepts, conv_bias_clear_of_zero, conv_error_ratios, conv_ref64, conv_routes,
                     conv_sample_positions, conv_terms, conv_yardstick)

pytestmark = pytest.mark.gpu

SENTINEL_BITS = 0x7B8D5EA7                       # a finite float32 no kernel here produces
BAND_ROWS = 128                                  # one tile of rows before and after the destination
TILES = {"T128": (8, 136, 79, 81), "T72": (8, 72, 37, 35), "T40": (8, 40, 9, 13), "T72M": (8, 72, 53, 51)}
TILE_ROUTE = {"T128": "bn128", "T72": "bn32", "T40": "bn64", "T72M": "bn64"}
WHOLE = (8, 136, 64, 100)                        # T128's columns on 6400 rows = 50 whole tiles: the fused BatchNorm-backward sums
SHAPE_A = (1, 256, 16, 16, 256, 3, 3, 1, 1, 1)
SHAPE_B = (2, 16, 7, 9, 24, 3, 3, 2, 1, 1)
SHAPE_B_MIRROR = (2, 24, 7, 9, 16, 3, 3, 2, 1, 1)
SHAPE_POSM = (2048, 64, 3, 3, 64, 3, 3, 1, 1, 1)


def _nhwc(t):
    """CPU [N,C,H,W] -> contiguous float32 [N,H,W,C] on the device (filters: OHWI)."""
    return torch.as_tensor(t).float().permute(0, 2, 3, 1).contiguous().cuda()


class _Dest:
    """A [N,H,W,C] float32 destination between two sentinel bands inside one allocation."""

    def __init__(self, n, h, w, c, fill=None):
        self.shape, self.size, self.band = (n, h, w, c), n * h * w * c, BAND_ROWS * c
        self.buf = torch.full((self.size + 2 * self.band,), SENTINEL_BITS, dtype=torch.int32, device="cuda").view(torch.float32)
        self.t = self.buf[self.band:self.band + self.size]
        if fill is not None:
            self.t.copy_(_nhwc(fill).reshape(-1))

    def result(self, tag):
        """The destination as CPU float64 [N,C,H,W]; asserts both bands untouched and every element written."""
        torch.cuda.synchronize()
        bits = self.buf.view(torch.int32)
        lo, hi = bits[:self.band], bits[self.band + self.size:]
        assert bool((lo == SENTINEL_BITS).all()) and bool((hi == SENTINEL_BITS).all()), \
            "%s: %d words of the band before and %d of the band after the destination were overwritten" \
            % (tag, int((lo != SENTINEL_BITS).sum()), int((hi != SENTINEL_BITS).sum()))
        assert bool((bits[self.band:self.band + self.size] != SENTINEL_BITS).all()), "%s: destination elements left unwritten" % tag
        n, h, w, c = self.shape
        return self.t.view(n, h, w, c).permute(0, 3, 1, 2).cpu().double()


def _judge(tag, got, ref_all, idx, ref_s, max_seq, rms_seq):
    got, ref_all = got.numpy(), ref_all.numpy()
    assert np.abs(ref_s - ref_all[idx]).max() <= 1e-11 * max(np.abs(ref_s).max(), 1e-30), tag
    ratios = conv_error_ratios(got[idx], ref_s, max_seq, rms_seq, got, ref_all)
    print("%s: max %.2f rms %.2f whole-tensor rms %.2f of the chained-fp32 yardstick, margin %g" % ((tag,) + ratios + (CONV_MARGIN,)))
    assert conv_accepts(ratios), (tag, ratios)


def _call(name, *args):
    from rrnet_amd import _C
    _C.check(_C.fn(name)(*[_C.ptr(a) if (a is None or torch.is_tensor(a)) else a for a in args], _C.stream()), name)


def _slab(rows, k):
    return torch.full((-(-rows // 128) * 2 * k,), -7.25e300, dtype=torch.float64, device="cuda")


def _check_slab(tag, slab, y, k):
    """tests/test_conv_fp64_gpu.py's bounds for the fused slab: s1 / s2 chain at most 64 rows per lane in fp32, then all is
    double: |err| <= 65 u sum|y| and 66 u sum y^2 against the float64 column sums of the kernel's own y [N,K,P,Q]."""
    rows = slab.view(-1, 2, k)
    assert bool((rows != -7.25e300).all()), tag                      # every tile row, every column written
    yd = y.permute(0, 2, 3, 1).reshape(-1, k)
    s1, s2, a1 = yd.sum(0), (yd * yd).sum(0), yd.abs().sum(0)
    got = rows.sum(0).cpu()
    e1, e2 = (got[0] - s1).abs(), (got[1] - s2).abs()
    b1, b2 = 65 * U32 * a1, 66 * U32 * s2
    print("%s: slab (%d rows) error over bound: sum y %.3f, sum y^2 %.3f" % (tag, rows.shape[0], float((e1 / (b1 + 1e-300)).max()),
          float((e2 / (b2 + 1e-300)).max())))
    assert bool((e1 <= b1).all()) and bool((e2 <= b2).all()), tag


def _flipped(wd, k, c, r, s):
    """The flipped, transposed filter rr_conv_dgrad_s1 takes, from the OHWI filter on the device."""
    wt = torch.empty_like(wd)
    _call("rr_weight_flip_transpose", wd, wt, k, c, r, s)
    return wt


@functools.lru_cache(maxsize=None)
def _fwd_case(name):
    """Forward pass cin -> cols, 3x3, pad 1: inputs and float64 references (plain, bias, bias + ReLU), computed once."""
    cin, cols, h, w = TILES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    x = torch.from_numpy(rng.standard_normal((1, cin, h, w)).astype(np.float32))
    wt = torch.from_numpy((rng.standard_normal((cols, cin, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32))
    y0 = conv_ref64(x, wt, None, 1, (1, 1), False)[0]
    # |bias| around 2.5 standard deviations of y: a channel keeps a few elements on the other side of the ReLU, and a gap
    # around 0 that no element falls into exists within conv_bias_clear_of_zero's reach even at 6399 elements per channel
    b0 = rng.choice([-2.5, 2.5], cols) + 0.3 * rng.standard_normal(cols)
    b = torch.from_numpy(conv_bias_clear_of_zero(y0.numpy(), b0.astype(np.float32)))
    return dict(x=x, w=wt, b=b, plain=y0, bias=conv_ref64(x, wt, b, 1, (1, 1), False)[0], bias_relu=conv_ref64(x, wt, b, 1, (1, 1), True)[0])


@functools.lru_cache(maxsize=None)
def _bwd_case(name, hw=None):
    """Data gradient whose destination has `cols` channels: the forward layer cols -> cin, 3x3, pad 1."""
    cin, cols, h, w = TILES[name] if hw is None else TILES[name][:2] + hw
    rng = np.random.default_rng(sum(map(ord, name)) + 7 * h)
    wt = torch.from_numpy((rng.standard_normal((cin, cols, 3, 3)) / np.sqrt(cin * 9)).astype(np.float32))
    gy = torch.from_numpy(rng.standard_normal((1, cin, h, w)).astype(np.float32))
    base = torch.from_numpy(rng.standard_normal((1, cols, h, w)).astype(np.float32))
    dx = conv_ref64(torch.zeros(1, cols, h, w), wt, None, 1, (1, 1), False, gy)[1]
    idx = conv_sample_positions((1, cols, h, w), 11 * h + 1)
    yard = conv_yardstick(conv_terms("dgrad", idx, None, wt, gy, 1, (1, 1)), head=base.double().numpy()[idx])
    return dict(w=wt, gy=gy, base=base, dx=dx, idx=idx, yard=yard, dims=(1, h, w, cols, cin))


def test_the_tile_cases_reach_the_three_tile_widths():
    for name, (cin, cols, h, w) in TILES.items():
        fwd = conv_routes(1, cin, h, w, cols, 3, 3, 1, (1, 1), True, False, True)["fprop"]
        via = conv_routes(1, cols, h, w, cin, 3, 3, 1, (1, 1), False, False, False)["dgrad_via_fprop"]
        assert fwd == {TILE_ROUTE[name]} and via == {TILE_ROUTE[name]}, (name, fwd, via)


@pytest.mark.parametrize("mode", ["plain", "bias", "bias_relu"])
@pytest.mark.parametrize("name", list(TILES))
def test_fprop_tiles_with_slab(name, mode):
    cin, cols, h, w = TILES[name]
    cs = _fwd_case(name)
    bias = None if mode == "plain" else cs["b"]
    idx = conv_sample_positions((1, cols, h, w), 3)
    yard = conv_yardstick(conv_terms("fprop", idx, cs["x"], cs["w"], None, 1, (1, 1), bias=bias), relu=mode == "bias_relu")
    tag = "fprop %s %s" % (name, mode)
    dst, slab = _Dest(1, h, w, cols), _slab(h * w, cols)
    _call("rr_conv_fprop", _nhwc(cs["x"]), _nhwc(cs["w"]), None if bias is None else bias.cuda(), dst.t, slab, 1, h, w, cin, cols, 3, 3, 1, 1, 1,
          int(mode == "bias_relu"))
    y = dst.result(tag)
    _judge(tag, y, cs[mode], idx, *yard)
    _check_slab(tag, slab, y, cols)


@pytest.mark.parametrize("name", list(TILES))
def test_dgrad_s1_tiles_plain_and_accumulating(name):
    cs = _bwd_case(name)
    n, h, w, c, k = cs["dims"]
    wt = _flipped(_nhwc(cs["w"]), k, c, 3, 3)
    for acc in (0, 1):
        tag = "dgrad_s1 %s accumulate=%d" % (name, acc)
        dst = _Dest(n, h, w, c, cs["base"] if acc else None)
        _call("rr_conv_dgrad_s1", _nhwc(cs["gy"]), wt, dst.t, n, h, w, c, k, 3, 3, 1, 1, acc)
        _judge(tag, dst.result(tag), cs["dx"] + (cs["base"].double() if acc else 0), cs["idx"], *cs["yard"][3 * acc:3 * acc + 3])


def _check_sums(tag, sums, d, xhat, c, both=True):
    """`sums` [2][C] against the float64 column sums of d and d * xhat, d from the kernel's own dx.  Bounds as _check_slab's:
    chains of at most 64 rows per lane in fp32, everything after them double.  sum d: 64 additions + 1 -> 65 u sum|d|.
    sum d*xhat: each term carries the roundings of y - mean, of (.) * invstd and of the product on top -> 68 u sum|d*xhat|."""
    d2, x2 = d.permute(0, 2, 3, 1).reshape(-1, c), xhat.permute(0, 2, 3, 1).reshape(-1, c)
    got = sums.view(2, c).cpu()
    e1, b1 = (got[0] - d2.sum(0)).abs(), 65 * U32 * d2.abs().sum(0)
    print("%s: sum d error over bound %.3f" % (tag, float((e1 / (b1 + 1e-300)).max())))
    assert bool((e1 <= b1).all()), tag
    if both:
        e2, b2 = (got[1] - (d2 * x2).sum(0)).abs(), 68 * U32 * (d2 * x2).abs().sum(0)
        print("%s: sum d*xhat error over bound %.3f" % (tag, float((e2 / (b2 + 1e-300)).max())))
        assert bool((e2 <= b2).all()), tag


@pytest.mark.parametrize("hw", [None, WHOLE[2:]], ids=["ragged79x81", "whole64x100"])
@pytest.mark.parametrize("mask", ["z", "scale_shift"])
@pytest.mark.parametrize("acc", [0, 1], ids=["store", "accumulate"])
def test_dgrad_s1_bnsum(hw, mask, acc):
    """T128's columns: dx as rr_conv_dgrad_s1's, `sums` = column sums of d = dx * mask and of d * xhat.  Whole tiles take the
    fused epilogue; the ragged map the separate reduce pass behind the plain epilogue."""
    cs = _bwd_case("T128", hw)
    n, h, w, c, k = cs["dims"]
    rng = np.random.default_rng(5 + h)
    py = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))          # the producer's pre-BN output
    mean = torch.from_numpy((0.1 * rng.standard_normal(c)).astype(np.float32))
    invstd = torch.from_numpy(rng.uniform(0.5, 2.0, c).astype(np.float32))
    msc = torch.from_numpy(rng.uniform(0.5, 2.0, c).astype(np.float32) * rng.choice([-1.0, 1.0], c).astype(np.float32))
    msh = torch.from_numpy((0.3 * rng.standard_normal(c)).astype(np.float32))
    if mask == "z":
        pz = torch.from_numpy(np.maximum(rng.standard_normal((n, c, h, w)), 0).astype(np.float32))
        on = pz > 0
    else:
        pz = None
        sc64, sh64 = msc.double().view(1, -1, 1, 1), msh.double().view(1, -1, 1, 1)
        py = torch.where((py.double() * sc64 + sh64).abs() < 1e-3, py + 0.01 / msc.view(1, -1, 1, 1), py)   # y*scale + shift clear of 0:
        aff64 = py.double() * sc64 + sh64                                                                 # fp32 and fp64 agree on the mask
        assert float(aff64.abs().min()) > 1e-4
        on = aff64 > 0
    tag = "dgrad_s1_bnsum %dx%d mask=%s accumulate=%d" % (h, w, mask, acc)
    dst = _Dest(n, h, w, c, cs["base"] if acc else None)
    sums = torch.zeros(2 * c, dtype=torch.float64, device="cuda")
    _call("rr_conv_dgrad_s1_bnsum", _nhwc(cs["gy"]), _flipped(_nhwc(cs["w"]), k, c, 3, 3), dst.t, n, h, w, c, k, 3, 3, 1, 1, acc, _nhwc(py),
          None if pz is None else _nhwc(pz), mean.cuda(), invstd.cuda(), None if pz is not None else msc.cuda(),
          None if pz is not None else msh.cuda(), _slab(h * w, c), sums)
    dx = dst.result(tag)
    _judge(tag, dx, cs["dx"] + (cs["base"].double() if acc else 0), cs["idx"], *cs["yard"][3 * acc:3 * acc + 3])
    xhat = ((py - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)).double()          # as the kernel forms it: float32
    _check_sums(tag, sums, dx * on, xhat, c)


@pytest.mark.parametrize("acc", [0, 1], ids=["store", "accumulate"])
def test_dgrad_s1_relubias(acc):
    """T128's columns on whole tiles (the entry point refuses others): the MASKED gradient is stored, sums[0] = its column sums."""
    cs = _bwd_case("T128", WHOLE[2:])
    n, h, w, c, k = cs["dims"]
    rng = np.random.default_rng(9)
    pz = torch.from_numpy(np.maximum(rng.standard_normal((n, c, h, w)), 0).astype(np.float32))
    on = (pz > 0).double()
    tag = "dgrad_s1_relubias accumulate=%d" % acc
    dst = _Dest(n, h, w, c, cs["base"] if acc else None)
    sums = torch.zeros(2 * c, dtype=torch.float64, device="cuda")
    _call("rr_conv_dgrad_s1_relubias", _nhwc(cs["gy"]), _flipped(_nhwc(cs["w"]), k, c, 3, 3), dst.t, n, h, w, c, k, 3, 3, 1, 1, acc, _nhwc(pz),
          _slab(h * w, c), sums)
    d = dst.result(tag)
    ref_s, mx, rms = cs["yard"][3 * acc:3 * acc + 3]
    ref = (cs["dx"] + (cs["base"].double() if acc else 0)) * on
    _judge(tag, d, ref, cs["idx"], ref_s * on.numpy()[cs["idx"]], mx, rms)
    _check_sums(tag, sums, d, d, c, both=False)


@functools.lru_cache(maxsize=None)
def _full_case(cfg):
    n, c, h, w, k, r, s, st, ph, pw = cfg
    rng = np.random.default_rng(n * c + h)
    x = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    wt = torch.from_numpy((rng.standard_normal((k, c, r, s)) / np.sqrt(c * r * s)).astype(np.float32))
    p, q = (h + 2 * ph - r) // st + 1, (w + 2 * pw - s) // st + 1
    gy = torch.from_numpy(rng.standard_normal((n, k, p, q)).astype(np.float32))
    base = torch.from_numpy(rng.standard_normal((n, c, h, w)).astype(np.float32))
    y, dx, _ = conv_ref64(x, wt, None, st, (ph, pw), False, gy)
    return dict(x=x, w=wt, gy=gy, base=base, y=y, dx=dx, pq=(p, q))


def _fprop_full(cfg, tag):
    n, c, h, w, k, r, s, st, ph, pw = cfg
    cs = _full_case(cfg)
    p, q = cs["pq"]
    idx = conv_sample_positions((n, k, p, q), 21)
    dst = _Dest(n, p, q, k)
    _call("rr_conv_fprop", _nhwc(cs["x"]), _nhwc(cs["w"]), None, dst.t, None, n, h, w, c, k, r, s, st, ph, pw, 0)
    _judge(tag, dst.result(tag), cs["y"], idx, *conv_yardstick(conv_terms("fprop", idx, cs["x"], cs["w"], None, st, (ph, pw))))


def _dgrad_full(cfg, tag):
    n, c, h, w, k, r, s, st, ph, pw = cfg
    cs = _full_case(cfg)
    idx = conv_sample_positions((n, c, h, w), 22)
    yard = conv_yardstick(conv_terms("dgrad", idx, None, cs["w"], cs["gy"], st, (ph, pw)), head=cs["base"].double().numpy()[idx])
    for acc in (0, 1):
        dst = _Dest(n, h, w, c, cs["base"] if acc else None)
        _call("rr_conv_dgrad", _nhwc(cs["gy"]), _nhwc(cs["w"]), dst.t, n, h, w, c, k, r, s, st, ph, pw, acc)
        t = "%s accumulate=%d" % (tag, acc)
        _judge(t, dst.result(t), cs["dx"] + (cs["base"].double() if acc else 0), idx, *yard[3 * acc:3 * acc + 3])


def test_split_k_atomics():
    rt = conv_routes(*SHAPE_A[:7], SHAPE_A[7], SHAPE_A[8:], False, False, False)
    assert "ksplit>1" in rt["fprop"] and "ksplit>1" in rt["dgrad"], rt
    _fprop_full(SHAPE_A, "split-K fprop")
    _dgrad_full(SHAPE_A, "split-K dgrad")


@pytest.mark.parametrize("cfg", [SHAPE_B, SHAPE_B_MIRROR], ids=["dx16", "dx24"])
def test_stride2_parity_classes(cfg):
    assert "parity4" in conv_routes(*cfg[:7], cfg[7], cfg[8:], False, False, False)["dgrad"]
    _dgrad_full(cfg, "parity dgrad %d columns" % cfg[1])


def test_position_major_tiles():
    assert "pos_major" in conv_routes(*SHAPE_POSM[:7], SHAPE_POSM[7], SHAPE_POSM[8:], False, False, False)["fprop"]
    _fprop_full(SHAPE_POSM, "pos_major fprop")
