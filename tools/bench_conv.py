"""Micro-benchmark of the conv kernels at the BASELINE config-2 layer shapes (GPU box)."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from rrnet_amd import ops

def timeit(fn, iters=10, warm=3):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters): fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / iters

SHAPES = [  # N, C, H, W, K, R, stride
    (8, 256, 256, 256, 256, 3, 1),
    (8, 256, 128, 128, 256, 3, 1),
    (8, 384, 64, 64, 384, 3, 1),
    (8, 384, 32, 32, 384, 3, 1),
    (8, 384, 16, 16, 384, 3, 1),
    (8, 512, 8, 8, 512, 3, 1),
    (8, 256, 256, 256, 256, 1, 1),
    (8, 128, 512, 512, 256, 3, 2),
    (8, 256, 256, 256, 256, 3, 2),
    (8, 256, 128, 128, 384, 3, 2),
    (8, 384, 64, 64, 384, 3, 2),
    (8, 128, 512, 512, 256, 1, 2),
    (8, 256, 256, 256, 256, 1, 2),
    (8, 3, 1024, 1024, 128, 7, 2),
]
def bench_rows(counts=(800, 8192, 32768)):
    """--rows: the rows route (csrc/conv_rows.hip) at the headline head shape, 8 x 256 x 256 x 256 -> 256, 3x3: the pair
    (rows entry point + _unless entry point, as ops launches them) for lists of `counts` active pixels against the dense data
    and weight gradient, and what each side costs when it returns at the gate."""
    from rrnet_amd import _C
    n, c, h, w, k = 8, 256, 256, 256, 256
    m = n * h * w
    x = ops.to_nhwc(torch.randn(n, c, h, w, device="cuda"))
    wt_ = ops.to_nhwc(torch.randn(k, c, 3, 3, device="cuda") * 0.02)
    flip = torch.empty(wt_.numel(), device="cuda")
    _C.call("rr_weight_flip_transpose", wt_, flip, k, c, 3, 3)
    dw = torch.zeros((k, 3, 3, c), device="cuda").permute(0, 3, 1, 2)
    dx = ops.empty_nhwc(n, c, h, w, "cuda")
    geo = (n, h, w, c, k, 3, 3, 1, 1)
    cap = m // ops._ROWS_MAX_SHARE
    g = torch.Generator(device="cuda").manual_seed(1)
    for cnt in sorted(set(counts) | {cap, cap + 1}):
        dy = ops.zeros_nhwc(n, k, h, w, "cuda")
        sel = torch.randperm(m, device="cuda", generator=g)[:cnt]
        dy.permute(0, 2, 3, 1).reshape(m, k)[sel] = torch.randn(cnt, k, device="cuda", generator=g)
        listed = ops.active_rows(dy)
        rows, count = listed[:2]
        assert int(count.item()) == cnt
        tg, tcount = ops.active_targets(listed, (n, c, h, w), 3, 3, (1, 1))      # the data gradient works from the dx pixels the list reaches
        tcnt, tcap = int(tcount.item()), m // ops._TARGETS_MAX_SHARE
        t_list = timeit(lambda: ops.active_targets(ops.active_rows(dy), (n, c, h, w), 3, 3, (1, 1)))
        d_dense = timeit(lambda: _C.call("rr_conv_dgrad_s1", dy, flip, dx, *geo, 0))
        w_dense = timeit(lambda: _C.call("rr_conv_wgrad", x, dy, dw, n, h, w, c, k, 3, 3, 1, 1, 1, 0, 0))
        d_rows = timeit(lambda: _C.call("rr_conv_dgrad_s1_rows", dy, wt_, dx, *geo, 0, tg, tcount, m))
        d_rows_acc = timeit(lambda: _C.call("rr_conv_dgrad_s1_rows", dy, wt_, dx, *geo, 1, tg, tcount, m))
        w_rows = timeit(lambda: _C.call("rr_conv_wgrad_rows", x, dy, dw, *geo, rows, count, m))
        d_pair = timeit(lambda: (_C.call("rr_conv_dgrad_s1_rows", dy, wt_, dx, *geo, 0, tg, tcount, tcap),
                                 _C.call("rr_conv_dgrad_s1_unless", dy, flip, dx, *geo, 0, tcount, tcap)))
        w_pair = timeit(lambda: (_C.call("rr_conv_wgrad_rows", x, dy, dw, *geo, rows, count, cap),
                                 _C.call("rr_conv_wgrad_unless", x, dy, dw, *geo, count, cap)))
        d_exit = timeit(lambda: _C.call("rr_conv_dgrad_s1_unless", dy, flip, dx, *geo, 0, count, m))      # dense launch returning at the gate
        w_exit = timeit(lambda: _C.call("rr_conv_wgrad_unless", x, dy, dw, *geo, count, m))
        r_exit = timeit(lambda: (_C.call("rr_conv_dgrad_s1_rows", dy, wt_, dx, *geo, 0, tg, tcount, tcnt - 1),  # rows launches returning at the gate
                                 _C.call("rr_conv_wgrad_rows", x, dy, dw, *geo, rows, count, cap if cnt > cap else 0)))
        print("rows %6d -> %6d dx pixels (max_rows %d, %d) | lists %.3f ms | dense dgrad %.3f wgrad %.3f | rows alone dgrad %.3f (accumulating %.3f) wgrad %.3f | "
              "pair dgrad %.3f wgrad %.3f | at the gate: dense dgrad %.3f wgrad %.3f, rows dgrad+wgrad %.3f ms"
              % (cnt, tcnt, cap, tcap, t_list, d_dense, w_dense, d_rows, d_rows_acc, w_rows, d_pair, w_pair, d_exit, w_exit, r_exit), flush=True)


WINO_SHAPES = [(8, 256, 256, 256, 256), (8, 256, 128, 128, 256), (8, 256, 128, 128, 384), (8, 384, 64, 64, 384),
               (8, 384, 32, 32, 384)]       # N, C, H, W, K of the headline step's 3x3 stride-1 layers, largest level first


def wino_wgrad_row(n, c, h, w, k, rounds):
    """One level of --wino: rr_conv_wino_wgrad against rr_conv_wgrad, the arms alternating `rounds` times (mean, spread = max - min), and
    the route's stages: single measurements taken once before the rounds, not alternated, no spread; the input transform and the zero
    fill are the remainder."""
    from rrnet_amd import _C
    W = ops._WINO
    tiles = n * ((h + 1) // 2) * ((w + 1) // 2)
    x = ops.to_nhwc(torch.randn(n, c, h, w, device="cuda"))
    dy = ops.to_nhwc(torch.randn(n, k, h, w, device="cuda"))
    dw = ops.zeros_nhwc(k, c, 3, 3, "cuda")
    wws = ops._wino_ws(x.device, n, h, w, c, k, "rr_conv_wino_wgrad_ws_bytes")
    v_, w_, s_ = wws, wws[16 * tiles * c:], wws[16 * tiles * (c + k):]
    W.call("rr_wino_input", x, v_, n, h, w, c)
    t_dy = timeit(lambda: W.call("rr_wino_dy", dy, w_, n, h, w, k))
    t_wg = timeit(lambda: W.call("rr_wino_wgrad_gemm", v_, w_, s_, tiles, c, k))
    t_dw = timeit(lambda: W.call("rr_wino_dw", s_, dw, k, c))
    td, tw = [], []
    for _ in range(rounds):
        td.append(timeit(lambda: _C.call("rr_conv_wgrad", x, dy, dw, n, h, w, c, k, 3, 3, 1, 1, 1, 0, 0)))
        tw.append(timeit(lambda: W.call("rr_conv_wino_wgrad", x, dy, dw, wws, wws.numel() * 4, n, h, w, c, k)))
    md, mw = sum(td) / rounds, sum(tw) / rounds
    sd, sw = max(td) - min(td), max(tw) - min(tw)
    verdict = "wino wins" if md - mw > 2 * max(sd, sw) else ("direct wins" if mw - md > 2 * max(sd, sw) else "inside the spread")
    gf = 2.0 * 16 * tiles * c * k / 1e9
    print("N%d C%d %dx%d K%d (%d pixels) wgrad | direct %.3f ms (spread %.3f, %.1f TF) | wino %.3f ms (spread %.3f) | %+.3f ms: %s | stages: "
          "dy transform %.3f ms (%.2f TB/s), GEMMs %.3f ms (%.1f TF), dw transform %.3f ms; input transform + zero fill: the rest %.3f ms"
          % (n, c, h, w, k, n * h * w, md, sd, 2.0 * 9 * n * h * w * c * k / 1e9 / md, mw, sw, mw - md, verdict, t_dy,
             (n * h * w * k + 16.0 * tiles * k) * 4 / t_dy / 1e9, t_wg, gf / t_wg, t_dw, mw - t_dy - t_wg - t_dw), flush=True)


def bench_wino(rounds=3, wgrad_only=False):
    """--wino: the Winograd route (csrc/conv_wino.hip) against the direct kernel at the headline's 3x3 stride-1 levels, per pass
    (fprop with statistics, dgrad, dgrad accumulating, dgrad with the producer's BatchNorm link), the two arms alternating
    `rounds` times: mean and spread (max - min) of each, and the route's stages (input transform, GEMMs; the output transform
    is the rest).  The gate's floor (rr_plan::WINO_MIN_PIXELS) is read off this table: the smallest level at which the route wins
    by more than twice the larger spread.  The weight-gradient row (rr_conv_wino_wgrad against rr_conv_wgrad) has stages and
    a floor of its own (rr_plan::WINO_WGRAD_MIN_PIXELS); --wgrad-only prints that row alone."""
    from rrnet_amd import _C
    W = ops._WINO
    for n, c, h, w, k in WINO_SHAPES:
        wino_wgrad_row(n, c, h, w, k, rounds)
        if wgrad_only:
            continue
        x = ops.to_nhwc(torch.randn(n, c, h, w, device="cuda"))
        wt = ops.to_nhwc(torch.randn(k, c, 3, 3, device="cuda") * 0.02)
        dy = ops.to_nhwc(torch.randn(n, k, h, w, device="cuda"))
        y, dx = ops.empty_nhwc(n, k, h, w, "cuda"), ops.empty_nhwc(n, c, h, w, "cuda")
        flip = torch.empty(wt.numel(), device="cuda")
        _C.call("rr_weight_flip_transpose", wt, flip, k, c, 3, 3)
        u_f, u_d = ops._wino_filter(wt, False), ops._wino_filter(wt, True, flip)
        ws = ops._wino_ws(x.device, n, h, w, max(c, k), max(c, k))
        wsb = ws.numel() * 4
        slab = torch.empty(_C.call("rr_conv_stat_slab_bytes", n, h, w, max(c, k)) // 8, dtype=torch.float64, device="cuda")
        sums = torch.zeros(2 * c, dtype=torch.float64, device="cuda")
        py = ops.to_nhwc(torch.randn(n, c, h, w, device="cuda"))
        mean, invstd = torch.zeros(c, device="cuda"), torch.ones(c, device="cuda")
        msc, msh = torch.ones(c, device="cuda"), torch.zeros(c, device="cuda")
        geo = (n, h, w, c, k, 3, 3, 1, 1)
        arms = {
            "fprop+stats": (lambda: _C.call("rr_conv_fprop", x, wt, None, y, slab, n, h, w, c, k, 3, 3, 1, 1, 1, 0),
                            lambda: W.call("rr_conv_wino_fprop", x, u_f, None, y, slab, ws, wsb, n, h, w, c, k, 0, 0)),
            "dgrad": (lambda: _C.call("rr_conv_dgrad_s1", dy, flip, dx, *geo, 0),
                      lambda: W.call("rr_conv_wino_fprop", dy, u_d, None, dx, None, ws, wsb, n, h, w, k, c, 0, 0)),
            "dgrad accumulating": (lambda: _C.call("rr_conv_dgrad_s1", dy, flip, dx, *geo, 1),
                                   lambda: W.call("rr_conv_wino_fprop", dy, u_d, None, dx, None, ws, wsb, n, h, w, k, c, 0, 1)),
            "dgrad+bnsum": (lambda: _C.call("rr_conv_dgrad_s1_bnsum", dy, flip, dx, *geo, 0, py, None, mean, invstd, msc, msh, slab, sums),
                            lambda: W.call("rr_conv_wino_dgrad_bnsum", dy, u_d, dx, ws, wsb, n, h, w, c, k, 0, py, None, mean, invstd, msc, msh,
                                           slab, sums)),
        }
        tiles = n * ((h + 1) // 2) * ((w + 1) // 2)
        t_in = timeit(lambda: W.call("rr_wino_input", x, ws, n, h, w, c))
        t_gemm = timeit(lambda: W.call("rr_wino_gemm", ws, u_f, ws[16 * tiles * c:], tiles, c, k))
        t_filt = timeit(lambda: W.call("rr_wino_filter", wt, u_f, k, c))
        gflop = 2.0 * 16 * tiles * c * k / 1e9
        print("N%d C%d %dx%d K%d (%d output pixels) | stages: input transform %.3f ms (%.2f TB/s), GEMMs %.3f ms (%.1f TF), filter transform %.3f ms"
              % (n, c, h, w, k, n * h * w, t_in, (n * h * w * c + 16.0 * tiles * c) * 4 / t_in / 1e9, t_gemm, gflop / t_gemm, t_filt), flush=True)
        for name, (direct, wino) in arms.items():
            td, tw = [], []
            for _ in range(rounds):
                td.append(timeit(direct))
                tw.append(timeit(wino))
            md, mw = sum(td) / rounds, sum(tw) / rounds
            sd, sw = max(td) - min(td), max(tw) - min(tw)
            verdict = "wino wins" if md - mw > 2 * max(sd, sw) else ("direct wins" if mw - md > 2 * max(sd, sw) else "inside the spread")
            extra = "" if name != "fprop+stats" else " | output transform %.3f ms" % (mw - t_in - t_gemm)
            print("   %-20s direct %.3f ms (spread %.3f) | wino %.3f ms (spread %.3f) | %+.3f ms: %s%s"
                  % (name, md, sd, mw, sw, mw - md, verdict, extra), flush=True)


if "--rows" in sys.argv:
    bench_rows()
    sys.exit(0)
if "--wino" in sys.argv:
    bench_wino(wgrad_only="--wgrad-only" in sys.argv)
    sys.exit(0)
only = [int(a) for a in sys.argv[1:]]
for i, (n, c, h, w, k, r, st) in enumerate(SHAPES):
    if only and i not in only: continue
    pad = r // 2
    x = ops.to_nhwc(torch.randn(n, c, h, w, device="cuda"))
    wt = ops.to_nhwc(torch.randn(k, c, r, r, device="cuda") * 0.02)
    p, q = ops.out_hw(h, w, r, r, st, pad, pad)
    dy = ops.to_nhwc(torch.randn(n, k, p, q, device="cuda"))
    dw = torch.zeros((k, r, r, c), device="cuda").permute(0, 3, 1, 2)
    dx = ops.empty_nhwc(n, c, h, w, "cuda")
    flops = 2.0 * n * p * q * k * c * r * r
    t1 = timeit(lambda: ops.conv_fprop(x, wt, None, st, (pad, pad), False, want_stats=os.environ.get("RR_BENCH_NOSTATS") != "1"))
    t2 = timeit(lambda: ops.conv_dgrad(dy, wt, (n, c, h, w), st, (pad, pad), out=dx))
    t3 = timeit(lambda: ops.conv_wgrad(x, dy, dw, st, (pad, pad)))
    if st == 2:
        t4 = timeit(lambda: ops.conv_dgrad(dy, wt, (n, c, h, w), st, (pad, pad), out=dx, accumulate=True))
        print("   dgrad accumulating into dx: %.3f ms %.1f TF" % (t4, flops / t4 / 1e9), flush=True)
    print("N%d C%d %dx%d K%d r%d s%d | fprop %.3f ms %.1f TF | dgrad %.3f ms %.1f TF | wgrad %.3f ms %.1f TF" % (
        n, c, h, w, k, r, st, t1, flops / t1 / 1e9, t2, flops / t2 / 1e9, t3, flops / t3 / 1e9), flush=True)
