"""The rows route of the heads' 3x3 gradients (csrc/conv_rows.hip, include/rrnet_hip_rows.h) against fp64:
rr_active_rows, rr_conv_dgrad_s1_rows / rr_conv_wgrad_rows, the gate they share with rr_conv_dgrad_s1_unless /
rr_conv_wgrad_unless, and the route inside one train step of the tiny RRNet.

Reference: torch.nn.grad.conv2d_input / conv2d_weight in fp64 on the DENSE dy.  Tolerances: the kernel audit's own
(tests/kernel_audit.audit defaults), relative to the reference's maximum: 2e-5 data gradient, 2e-4 weight gradient.
Shapes: N=2, 12x20 map, 3x3 pad 1; C=80 K=96 (partial tiles both ways) and C=K=128 (exact tiles).

Run as a script (`python tests/test_conv_rows_gpu.py OUT`) it is the model test's child process: one train step, flat
gradient written to OUT (the switch RR_CONV_ROWS is read at import, so the other arm needs a fresh interpreter)."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CL = torch.channels_last
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, H, W = 2, 12, 20
M = N * H * W
SHAPES = [(80, 96), (128, 128)]
TOL_DGRAD, TOL_WGRAD = 2e-5, 2e-4


def _pix(n, p, q):
    return (n * H + p) * W + q


def _pattern(name):
    """-> sorted pixel indices of the rows that hold a gradient."""
    if name == "none":
        return []
    if name == "single":
        return [_pix(0, 5, 7)]
    if name == "border":        # four corners and one pixel on each edge: dropped scatter targets, zero-read taps
        return sorted(_pix(0, p, q) for p, q in [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 9), (H - 1, 9), (5, 0), (5, W - 1)])
    if name == "block":         # a 2x2 block and a diagonal neighbour: overlapping scatters
        return sorted(_pix(1, p, q) for p, q in [(4, 4), (4, 5), (5, 4), (5, 5), (6, 6)])
    if name == "tail33":        # 33 rows: one more than a 32-row K-step of the weight gradient
        return sorted(np.random.default_rng(5).choice(H * W, 33, replace=False).tolist())
    if name == "both":          # rows in both images
        rng = np.random.default_rng(6)
        return sorted(rng.choice(H * W, 9, replace=False).tolist() + (H * W + rng.choice(H * W, 11, replace=False)).tolist())
    raise KeyError(name)


PATTERNS = ["none", "single", "border", "block", "tail33", "both"]


def _nhwc_rows(t):
    """NHWC memory of a channels_last [N,C,H,W] tensor as [pixels][channels]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


@functools.lru_cache(maxsize=None)
def _case(c, k, pattern):
    """Operands (host) and the fp64 gradients of the dense dy, computed once per case and shared."""
    g = torch.Generator().manual_seed(1000 * c + k + len(pattern))
    x = torch.randn(N, c, H, W, generator=g).contiguous(memory_format=CL)
    w = (torch.randn(k, c, 3, 3, generator=g) * 0.05).contiguous(memory_format=CL)
    dy = torch.zeros(N, k, H, W).contiguous(memory_format=CL)
    rows = _pattern(pattern)
    if rows:
        _nhwc_rows(dy)[rows] = torch.randn(len(rows), k, generator=g)
    dx = torch.nn.grad.conv2d_input((N, c, H, W), w.double(), dy.double(), 1, 1)
    dw = torch.nn.grad.conv2d_weight(x.double(), (k, c, 3, 3), dy.double(), 1, 1)
    base_x = torch.randn(N, c, H, W, generator=g).contiguous(memory_format=CL)
    base_w = torch.randn(k, c, 3, 3, generator=g).contiguous(memory_format=CL)
    return SimpleNamespace(x=x, w=w, dy=dy, rows=rows, dx=dx, dw=dw, base_x=base_x, base_w=base_w)


def _rel(got, ref):
    return float((got.double().cpu() - ref).abs().max() / max(float(ref.abs().max()), 1e-30))


def _list(dy):
    from rrnet_amd import ops
    return ops.active_rows(dy)[:2]


@pytest.mark.parametrize("k", [2, 34, 96])
def test_active_rows_lists_the_nonzero_rows_in_ascending_order(k):
    """Every pattern, a row holding only a NaN in one channel, a row holding only -0.0 (not listed): ascending order and the
    exact count against torch.nonzero.  m = 480 rows: a full workgroup of 256 and a partial one; k = 2 and 34 are no
    multiples of 4 (the partial workgroup's scalar tail), 34 is the wh head's tap count."""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(k)
    for name in PATTERNS + ["nan"]:
        dy = torch.zeros(N, k, H, W).contiguous(memory_format=CL)
        flat = _nhwc_rows(dy)
        if name == "nan":
            flat[_pix(1, 3, 3), k - 1] = float("nan")
            flat[_pix(0, 2, 2), 0] = float("inf")
        else:
            rows = _pattern(name)
            if rows:
                flat[rows, int(torch.randint(k, (1,), generator=g))] = 1.5     # one channel only
        flat[_pix(1, 11, 19), 0] = -0.0                                          # the very last row: -0 is zero
        want = torch.nonzero((flat != 0).any(1)).flatten().to(torch.int32)
        rows_d, count_d = _list(dy.to(dev))
        torch.cuda.synchronize()
        cnt = int(count_d.item())
        assert cnt == want.numel(), (name, cnt, want.numel())
        assert torch.equal(rows_d[:cnt].cpu(), want), name
        if name == "nan":
            assert cnt == 2


def _dgrad(entry, cs, dx, accumulate, tail):
    from rrnet_amd import _C
    k, c = cs.w.shape[:2]
    _C.call(entry, cs.dy_d, cs.wt_d if entry.endswith("unless") else cs.w_d, dx, N, H, W, c, k, 3, 3, 1, 1, int(accumulate), *tail)


def _wgrad(entry, cs, dw, tail):
    from rrnet_amd import _C
    k, c = cs.w.shape[:2]
    _C.call(entry, cs.x_d, cs.dy_d, dw, N, H, W, c, k, 3, 3, 1, 1, *tail)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("c,k", SHAPES)
def test_rows_and_dense_entry_points_share_one_gate(c, k, pattern):
    """Both gradients (the data gradient gated on its list of dx pixels, the weight gradient on the list of dy pixels), with and
    without a running destination.  count == max_rows: the rows entry point alone gives the
    reference, the _unless entry point alone leaves a sentinel-filled destination bit for bit; count == max_rows + 1: the
    roles are reversed (not for the empty list: no max_rows >= 0 lies below a count of 0); in every case the pair
    together gives the reference exactly once (applied twice it misses the tolerance by the size of the gradient)."""
    from rrnet_amd import _C
    dev = torch.device("cuda", 0)
    cs = _case(c, k, pattern)
    cs.x_d, cs.w_d, cs.dy_d = cs.x.to(dev), cs.w.to(dev), cs.dy.to(dev)
    cs.wt_d = torch.empty(cs.w.numel(), dtype=torch.float32, device=dev)
    _C.call("rr_weight_flip_transpose", cs.w_d, cs.wt_d, k, c, 3, 3)
    from rrnet_amd import ops
    listed = ops.active_rows(cs.dy_d)
    rows, count = listed[:2]
    cnt = int(count.item())
    assert cnt == len(cs.rows)
    # the data gradient's list: the dx pixels a listed dy pixel reaches through one of the nine taps, ascending
    targets, tcount = ops.active_targets(listed, (N, c, H, W), 3, 3, (1, 1))
    tcnt = int(tcount.item())
    ind = torch.zeros(M)
    ind[cs.rows] = 1.0
    reach = torch.nn.functional.conv2d(ind.view(N, 1, H, W), torch.ones(1, 1, 3, 3), padding=1) > 0
    want_t = torch.nonzero(reach.flatten()).flatten().to(torch.int32)
    assert tcnt == want_t.numel() and torch.equal(targets[:tcnt].cpu(), want_t), (tcnt, want_t.numel())
    sentinel_x = torch.full((N, c, H, W), 7.0, device=dev).contiguous(memory_format=CL)
    figures = []
    for delta, rows_act in [(0, True)] + ([(-1, False)] if cnt > 0 else []):
        for accumulate in (False, True):
            max_rows = tcnt + delta
            # ---- data gradient
            start = cs.base_x.to(dev) if accumulate else sentinel_x.clone()
            ref = cs.dx + cs.base_x.double() if accumulate else cs.dx
            for who, acts in (("rows", rows_act), ("unless", not rows_act), ("pair", True)):
                dx = start.clone()
                if who in ("rows", "pair"):
                    _dgrad("rr_conv_dgrad_s1_rows", cs, dx, accumulate, (targets, tcount, max_rows))
                if who in ("unless", "pair"):
                    _dgrad("rr_conv_dgrad_s1_unless", cs, dx, accumulate, (tcount, max_rows))
                if acts:
                    figures.append(("dgrad", who, delta, accumulate, _rel(dx, ref), TOL_DGRAD))
                else:
                    assert torch.equal(dx.view(torch.int32), start.view(torch.int32)), ("dgrad", who, max_rows, accumulate)
            # ---- weight gradient (always adds into dw: "accumulate" = a running gradient in it)
            max_rows = cnt + delta
            start = cs.base_w.to(dev) if accumulate else torch.zeros(k, c, 3, 3, device=dev).contiguous(memory_format=CL)
            ref = cs.dw + cs.base_w.double() if accumulate else cs.dw
            for who, acts in (("rows", rows_act), ("unless", not rows_act), ("pair", True)):
                dw = start.clone() if (acts or accumulate) else torch.full_like(start, 7.0)
                keep = dw.clone()
                if who in ("rows", "pair"):
                    _wgrad("rr_conv_wgrad_rows", cs, dw, (rows, count, max_rows))
                if who in ("unless", "pair"):
                    _wgrad("rr_conv_wgrad_unless", cs, dw, (count, max_rows))
                if acts:
                    figures.append(("wgrad", who, delta, accumulate, _rel(dw, ref), TOL_WGRAD))
                else:
                    assert torch.equal(dw.view(torch.int32), keep.view(torch.int32)), ("wgrad", who, max_rows, accumulate)
    torch.cuda.synchronize()
    print("\n".join("%s %-6s max_rows-count %+d accumulate %d: %.2e (tol %.0e)" % f for f in figures))
    bad = [f for f in figures if not f[4] <= f[5]]
    assert not bad, bad


# ---- model level -------------------------------------------------------------------------------------------------
def _cfg():
    return SimpleNamespace(num_classes=10, Model=SimpleNamespace(num_stacks=2, backbone="hourglass_tiny", nms_type_for_stage1="nms",
                           nms_per_class_for_stage1=True), Train=SimpleNamespace(scale_factor=4))


def _train_step():
    """One train step (forward, criterion, backward) of the tiny RRNet on 2 seeded 256x256 frames -> the FlatAdam whose
    flat buffer holds the gradient.  64x64 head maps: 4096 pixels per image, the smallest map whose 3x3 head layers take
    the forward-kernel data gradient (ops._DGRAD_VIA_FPROP_MIN_PIXELS)."""
    from rrnet_amd import functional as RF
    from rrnet_amd.datasets.synthetic import synth_batch
    from rrnet_amd.flat import FlatAdam
    from rrnet_amd.models.rrnet import RRNet
    torch.manual_seed(219)
    model = RRNet(_cfg()).cuda().to(memory_format=CL).train()
    opt = FlatAdam(model, lr=2.5e-4)
    imgs, annos, hms, whs, inds, offs, masks, _ = [t.cuda() if torch.is_tensor(t) else t
                                                   for t in synth_batch(2, 256, 256, boxes_per_image=12, seed=219)]
    opt.zero_grad()
    outs = model(imgs, k=100)
    hm_l = sum(RF.focal_loss_hm_from_logits(outs[0][i], hms) / 2 for i in range(2))
    wh_l = sum(RF.reg_l1_loss(outs[1][i], masks, inds, whs) / 2 for i in range(2))
    off_l = sum(RF.reg_l1_loss(outs[2][i], masks, inds, offs) / 2 for i in range(2))
    a = annos.clone()
    a[:, :, 2:4] += a[:, :, 0:2]
    s2_l = RF.stage2_reg_loss(outs[3], outs[4], a, 4.0)
    (hm_l + 0.1 * wh_l + off_l + s2_l).backward()
    torch.cuda.synchronize()
    return opt


def test_train_step_takes_the_rows_route_for_the_regression_heads(tmp_path):
    """Under the kernel audit with a timer on: the audit is green; the 3x3 layers of the wh and offset heads (2 stacks each: 4)
    show up under the pair's timer keys, the two hm layers do not; and the flat gradient agrees, per parameter and
    relative to the parameter's largest gradient, within the audit's weight-gradient tolerance with the gradient of the
    same step under RR_CONV_ROWS=0 in a fresh process."""
    from kernel_audit import audit
    from rrnet_amd import ops
    assert ops._CONV_ROWS, "this test runs with the route switched on (RR_CONV_ROWS unset)"
    ops.TIMER = ops.KernelTimer()
    try:
        with audit() as rec:
            opt = _train_step()
        summary = ops.TIMER.summary()
    finally:
        ops.TIMER = None
    assert not rec.bad, rec.bad
    for key in ("conv_dgrad<rows>", "conv_dgrad<dense>", "conv_wgrad<rows>", "conv_wgrad<dense>"):
        assert key in summary and summary[key]["launches"] == 4 and summary[key]["flops"] == 0.0, (key, summary.get(key))
    grad = opt.fp.grad.detach().cpu()
    out = str(tmp_path / "grad_dense.bin")
    env = dict(os.environ, RR_CONV_ROWS="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=env, cwd=ROOT, timeout=600)
    dense = torch.from_numpy(np.fromfile(out, dtype=np.float32))
    assert dense.numel() == grad.numel() and bool(torch.isfinite(dense).all())
    base = opt.fp.grad.data_ptr()
    worst = (0.0, None)
    names = {id(p): n for n, p in opt.fp.module.named_parameters()} if hasattr(opt.fp, "module") else {}
    for p in opt.fp.params:
        o, n = (p._rr_grad.data_ptr() - base) // 4, p.numel()
        scale = float(dense[o:o + n].abs().max())
        err = float((grad[o:o + n] - dense[o:o + n]).abs().max())
        rel = err / scale if scale > 0 else (0.0 if err == 0 else float("inf"))
        if rel > worst[0]:
            worst = (rel, names.get(id(p), "param@%d" % o))
    print("flat gradient, rows route against RR_CONV_ROWS=0: worst per-parameter deviation %.2e (%s)" % worst)
    assert worst[0] <= TOL_WGRAD, worst


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from rrnet_amd import ops as _ops
    assert not _ops._CONV_ROWS, "the child process is the RR_CONV_ROWS=0 arm"
    _train_step().fp.grad.detach().cpu().numpy().tofile(sys.argv[1])
