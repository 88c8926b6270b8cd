"""Host (no GPU): rr_plan::wino_plan (rrnet_amd/csrc/conv_plan.h) as the library was built with it, through
rr_conv_wino_plan — what the Winograd route refuses, what it takes, and that its workspace is what the entry points demand.
The plan is additive: a launch it refuses stays with fprop_plan, whose fields tests/test_host_logic.py holds against their
mirror as before."""
import ctypes

import pytest

MATH_F32, MATH_BF16, MATH_F16X3 = 0, 1, 2
FIELDS = ("take", "floor_only", "tiles_lo", "tiles_hi", "bn", "gemm_blocks", "out_x", "out_y", "tiles_per_wg", "ws_lo", "ws_hi")
FLOOR = 8192          # the issue's lower limit of the gate's floor, in output pixels


def _plan(n, h, w, c, k, r=3, s=3, stride=1, ph=1, pw=1, math=MATH_F32, out_hw=(0, 0), bias=False, relu=False, stats=False,
          accumulate=False, strided=False, link=0):
    from rrnet_amd import _C
    buf = (ctypes.c_int * len(FIELDS))()
    flags = int(bias) | int(relu) << 1 | int(stats) << 2 | int(accumulate) << 3 | int(strided) << 4 | link << 8
    _C.Family("rrnet_hip_wino.h").call("rr_conv_wino_plan", math, n, h, w, c, k, r, s, stride, ph, pw, out_hw[0], out_hw[1], flags, buf)
    d = dict(zip(FIELDS, buf))
    d["tiles"] = d["tiles_lo"] | d["tiles_hi"] << 31
    d["ws_bytes"] = d["ws_lo"] | d["ws_hi"] << 31
    return d


HEADLINE = [(8, 256, 256, 256, 256), (8, 128, 128, 256, 256), (8, 128, 128, 256, 384),
            (8, 128, 128, 384, 384)]      # (n, h, w, c, k) of the headline step's 3x3 stride-1 layers at 256^2 and 128^2


@pytest.mark.parametrize("geo", HEADLINE, ids=lambda g: "n%dh%dw%dc%dk%d" % g)
def test_takes_the_headline_layers_with_every_epilogue_it_builds(geo):
    from rrnet_amd import _C
    n, h, w, c, k = geo
    for kw in (dict(), dict(stats=True), dict(bias=True, relu=True), dict(accumulate=True), dict(link=1), dict(link=1, accumulate=True)):
        p = _plan(n, h, w, c, k, **kw)
        assert p["take"] == 1, (geo, kw)
        assert p["tiles"] == n * (h // 2) * (w // 2) and p["bn"] == 128
        assert p["gemm_blocks"] == -(-p["tiles"] // 128) * -(-k // 128)
        assert p["out_x"] == n * h * w // 128 and p["out_y"] == -(-k // 256) and p["out_x"] * p["tiles_per_wg"] >= p["tiles"]
        # the workspace is what the entry points demand: V [16][T][c] + M [16][T][k]
        assert p["ws_bytes"] == 16 * p["tiles"] * (c + k) * 4 == _C.call("rr_conv_wino_ws_bytes", n, h, w, c, k)
        assert p["tiles"] * max(c, k) * 4 < 1 << 31          # every batch slice below 2 GiB (the whole of V or M may not be)


def test_refuses_what_the_route_does_not_cover():
    big = (8, 128, 128, 384, 384)
    assert _plan(*big)["take"] == 1
    refused = [dict(r=1, s=1, ph=0, pw=0), dict(r=5, s=5, ph=2, pw=2), dict(r=3, s=1, pw=0), dict(stride=2), dict(ph=0, pw=0), dict(ph=2, pw=2),
               dict(ph=1, pw=0), dict(math=MATH_BF16), dict(math=MATH_F16X3), dict(out_hw=(128, 128)), dict(strided=True),
               dict(link=2),                                  # the conv + bias + ReLU link is not built on this route
               dict(link=1, stats=True), dict(link=1, bias=True), dict(link=1, relu=True)]
    for kw in refused:
        assert _plan(*big, **kw)["take"] == 0, kw
    for c, k in ((382, 384), (384, 382), (3, 64), (64, 10)):
        assert _plan(8, 128, 128, c, k)["take"] == 0, (c, k)
    assert _plan(8, 128, 128, 384, 1028, link=1)["take"] == 0 and _plan(8, 128, 128, 384, 1024, link=1)["take"] == 1     # the link's channel limit
    # a tensor, or one batch slice of V / M, of 2 GiB and more
    assert _plan(8, 512, 512, 256, 256)["take"] == 0           # x and y: 2 GiB each
    assert _plan(32, 256, 256, 256, 256)["take"] == 0
    assert _plan(31, 256, 256, 256, 256)["take"] == 1
    assert _plan(0, 64, 64, 64, 64)["take"] == 0 and _plan(8, 64, 64, 0, 64)["take"] == 0


def test_refuses_every_shape_below_the_floor():
    """No launch of fewer than 8192 output pixels: the direct route there is a split-K launch of tens of microseconds, and the
    small-shape contracts of the existing tests (exact cancellation, signed zeros, a non-finite value within one tap) are the
    direct route's."""
    seen = 0
    for n in (1, 2, 3, 8, 16):
        for h, w in ((1, 5), (2, 2), (8, 8), (9, 13), (16, 16), (31, 33), (32, 32), (45, 91), (63, 65), (64, 64), (90, 91), (128, 128)):
            for c, k in ((64, 64), (256, 256), (384, 384), (512, 512)):
                p = _plan(n, h, w, c, k)
                if n * h * w < FLOOR:
                    assert p["take"] == 0 and p["floor_only"] == 1, (n, h, w, c, k)
                    seen += 1
                    # ... but the geometry is still planned: the entry points run below the floor (tests, benchmarks)
                    assert p["tiles"] == n * ((h + 1) // 2) * ((w + 1) // 2) and p["ws_bytes"] == 16 * p["tiles"] * (c + k) * 4
    assert seen > 100
    # from the limit up the floor is DESIGN 25's: existing tests pin the data gradients of 2 x 128 x 64 x 64 (tests/golden/conv_bwd_routes.json)
    # and of 2 x 64 x 128 x 128 (tests/test_bn_forward_gpu.py) to the direct entry points, so the headline's 64 x 64 level stays direct too
    for geo in ((2, 64, 64, 128, 128), (8, 32, 32, 384, 384), (2, 128, 128, 64, 64), (8, 64, 64, 384, 384)):
        p = _plan(*geo)
        assert p["take"] == 0 and p["floor_only"] == 1, geo
    assert _plan(8, 32, 32, 384, 384, stride=2)["floor_only"] == 0 and _plan(8, 128, 128, 384, 384)["floor_only"] == 0


def test_ragged_maps_have_whole_tiles_and_every_slab_row_a_workgroup():
    for n, h, w in ((8, 63, 65), (3, 127, 129), (8, 255, 257)):
        p = _plan(n, h, w, 256, 256)
        assert p["tiles"] == n * ((h + 1) // 2) * ((w + 1) // 2)
        assert p["out_x"] == -(-n * h * w // 128) and p["out_x"] * p["tiles_per_wg"] >= p["tiles"] > p["out_x"] * (p["tiles_per_wg"] - 1)
