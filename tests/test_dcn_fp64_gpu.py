"""GPU: every deformable-convolution kernel of csrc/dcn.hip against FLOAT64 (helpers.dcn_ref64: oracle/dcn.py in float64 on the
float32 inputs, the sample position formed by one float32 add), on every route of the launch plans (csrc/dcn_plan.h) and through
every entry point of helpers.DCN_ENTRY_FLAGS.

The bound is not a tolerance chosen by hand: per tensor, the error at 4096 sampled outputs (max-abs and RMS) and over the whole
tensor (RMS) is divided by the error of the same definition evaluated in float32 with every reduction chained in plain loop order
(helpers.dcn_terms), and no ratio may exceed helpers.DCN_MARGIN.  Two allowances are restated from reference quantities only: the
fixed-point window of the window data-gradient routes (helpers.dcn_fixed_point_allowance; its share of the bound is printed as
`fx=`, the largest ratio without it as `raw=`) and bf16 columns that lie within a float32 blend's error of a rounding boundary
(helpers.dcn_tie_*).

helpers.DCN64_GRID holds the smallest shapes that still split; helpers.DCN64_EDGE_CASES (one window route, one gather route per
pass) run every edge class of helpers.DCN_EDGE_CLASSES in both operand precisions.  Every case asks rr_dcn_plan which route it
took.  The L2-gather weight- and data-gradient kernels (route `gather`) multiply fp32 operands also behind the bf16 entry points:
there the reference is the fp32 definition.  One line per (case, entry point, tensor) is printed: profiles/dcn_fp64_ratios.txt is
that output of an MI355X run."""
import os

import numpy as np
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

CASES = [(name, "gauss") for name in H.DCN64_GRID] + [(name, cls) for name in H.DCN64_EDGE_CASES for cls in H.DCN_EDGE_CLASSES[1:]]
_OWN_MARGIN = int(os.environ.get("RR_DCN_WINDOW", "3"))


def _plan(pas, bf16, geo, flags):
    """rr_dcn_plan at the library's own margin -> {field: int} or None where it refuses."""
    import ctypes
    from rrnet_amd import _C
    buf = (ctypes.c_int * H.DCN_PLAN_INTS)(*([0] * H.DCN_PLAN_INTS))
    n, c, h, w, k, r, s, stride, ph, pw, dil, dg = geo
    if _C.fn("rr_dcn_plan")(pas, bf16, n, h, w, c, k, r, s, stride, ph, pw, dil, dg, -1, flags, buf, H.DCN_PLAN_INTS) != 0:
        return None
    return dict(zip(H.DCN_PLAN_FIELDS[pas], list(buf)))


def _nchw(t):
    return t.detach().float().cpu().contiguous().numpy()


def _call_fwd(entry, dev, geo):
    from rrnet_amd import ops
    x, off, mask, wt, bias = dev[:5]
    saved = ops._DCN_WPACK
    ops._DCN_WPACK = entry == "rr_dcn_fwd_bf16_packed"
    try:
        return ops.dcn_fwd(x, off, mask, wt, bias, geo[7], (geo[8], geo[9]), geo[10], geo[11], bf16=entry != "rr_dcn_fwd")
    finally:
        ops._DCN_WPACK = saved


def _call_wgrad(entry, dev, geo, base):
    from rrnet_amd import ops
    x, off, mask, _, _, dy = dev
    dw = ops.to_nhwc(base.cuda())
    img = dy.to(torch.bfloat16) if entry == "rr_dcn_wgrad_bf16_img" else None
    assert img is None or img.stride() == dy.stride()
    ops.dcn_wgrad(x, off, mask, dy, dw, geo[7], (geo[8], geo[9]), geo[10], geo[11], bf16=entry != "rr_dcn_wgrad", dy_img=img)
    return dw


def _call_dgrad(entry, dev, geo, base_dx):
    """Every data-gradient entry point through the C ABI, with the arguments rrnet_amd.ops.dcn_dgrad hands them."""
    from rrnet_amd import _C, ops
    x, off, mask, wt, _, dy = dev
    n, c, h, w, k, r, s, stride, ph, pw, dil, dg = geo
    acc, ready = entry.endswith("+acc"), "img" in entry
    dx = ops.to_nhwc(base_dx.cuda()).clone(memory_format=torch.preserve_format) if acc else ops.empty_nhwc(n, c, h, w, x.device)
    assert ops.is_nhwc(dx)
    doff, dmask = torch.empty_like(off), torch.empty_like(mask)
    assert doff.stride() == off.stride() and dmask.stride() == mask.stride()
    img = dy.to(torch.bfloat16) if ready else None
    assert img is None or img.stride() == dy.stride()
    head = (_C.ptr(x), _C.ptr(off), _C.ptr(mask), _C.ptr(wt), _C.ptr(dy))
    outs = (_C.ptr(dx), _C.ptr(doff), _C.ptr(dmask))
    dims = (n, h, w, c, k, r, s, stride, ph, pw, dil, dg)
    keep = None
    if entry.startswith("rr_dcn_dgrad_bf16_packed"):
        keep = torch.empty(_C.fn("rr_dcn_dgrad_ws_bytes")(n, dy.shape[2], dy.shape[3], c, k, r, s, int(ready)), dtype=torch.uint8, device=x.device)
        rc = _C.fn("rr_dcn_dgrad_bf16_packed")(*head, _C.ptr(img) if ready else None, *outs, *dims, int(acc), _C.ptr(keep), _C.stream())
        name = "rr_dcn_dgrad_bf16_packed"
    elif entry == "rr_dcn_dgrad_bf16_img":
        rc, name = _C.fn(entry)(*head, _C.ptr(img), *outs, *dims, _C.stream()), entry
    elif entry == "rr_dcn_dgrad_bf16_ws":
        keep = torch.empty(_C.fn("rr_dcn_dyb_bytes")(n, dy.shape[2], dy.shape[3], k), dtype=torch.uint8, device=x.device)
        rc, name = _C.fn(entry)(*head, *outs, *dims, _C.ptr(keep), _C.stream()), entry
    else:
        assert entry in ("rr_dcn_dgrad", "rr_dcn_dgrad_bf16"), entry
        rc, name = _C.fn(entry)(*head, *outs, *dims, _C.stream()), entry
    _C.check(rc, name)
    torch.cuda.synchronize()
    return dx, doff, dmask


@pytest.fixture(autouse=True)
def _stop_after_a_device_error():
    """A device error (as opposed to a failed comparison) ends the session: nothing more is launched on a device that has faulted."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as exc:
        pytest.exit("device error, no further GPU tests: %s" % exc, returncode=3)


_CASES = {}


def _case(geo, cls, bf16, accumulate):
    """The reference of one (shape, edge class, operand precision, accumulating or not); the "beyond the margin" class is built for
    the window margin the data-gradient plan reports for the shape."""
    key = (geo, cls, bf16, accumulate)
    if key not in _CASES:
        if len(_CASES) >= 4:                             # the references of one (shape, class): the entries of a case come in a row
            _CASES.clear()
        plan = _plan(H.DCN_DGRAD, 0, geo, 0)
        margin = plan["margin"] if plan is not None and plan["window"] else 3
        _CASES[key] = H.DcnCase(geo, cls, bf16, margin=margin, accumulate=accumulate)
    return _CASES[key]


@pytest.mark.parametrize("name,cls", CASES, ids=["%s-%s" % c for c in CASES])
def test_dcn_kernels_vs_float64(name, cls):
    from rrnet_amd import ops
    geo = H.DCN64_GRID[name]
    n, c, h, w, k, r, s, stride, ph, pw, dil, dg = geo
    failed, ran = [], []
    for bf16 in (0, 1):
        entries = [e for e in H.dcn64_entries(name) if e[2] == bf16]
        for accumulate in (False, True):
            todo = [e for e in entries if e[1].endswith("+acc") == accumulate]
            if not todo:
                continue
            for pas, entry, _, flags, labels in todo:
                plan = _plan(pas, bf16, geo, flags)
                assert plan is not None, (name, entry)
                # the L2-gather gradient kernels multiply fp32 operands whatever the entry point: their reference is the fp32 definition
                cs = _case(geo, cls, int(bf16 and (pas == H.DCN_FWD or bool(plan["window"]))), accumulate)
                dev = [ops.to_nhwc(t.cuda()) if t.dim() == 4 else t.cuda() for t in cs.inputs]
                if _OWN_MARGIN == 3:
                    mirror = H.dcn_plan_mirror(pas, bf16, geo, 3, flags)
                    assert all(plan[f] == mirror[f] for f in H.DCN_PLAN_FIELDS[pas]) and mirror["labels"] == labels, (name, entry, plan, mirror)
                if pas == H.DCN_FWD:
                    got = {"out": _nchw(_call_fwd(entry, dev, geo))}
                elif pas == H.DCN_WGRAD:
                    got = {"dw": _nchw(_call_wgrad(entry, dev, geo, cs.base_dw)).reshape(k, c, r * s)}
                else:
                    got = dict(zip(("dx", "doffset", "dmask"), (_nchw(t) for t in _call_dgrad(entry, dev, geo, cs.base_dx))))
                for tensor, val in got.items():
                    window = bool(plan["window"]) and pas == H.DCN_DGRAD
                    ratios, share, ok = cs.check(tensor, val, window=window)
                    raw = cs.check(tensor, val)[0][0] if window and tensor == "dx" else ratios[0]      # without the allowance
                    line = ("%-8s %-9s %-5s %-32s %-22s %-8s max %.3f rms %.3f all %.3f fx=%.2f raw=%.3f"
                            % (name, cls, ("fp32", "bf16")[bf16], entry, "+".join(sorted(labels)), tensor, *ratios, share, raw))
                    print(line)
                    ran.append(line)
                    if not ok:
                        failed.append(line)
    assert ran and not failed, "\n".join(failed)


@pytest.mark.parametrize("name,cls", [(n_, c_) for n_ in ("k36", "stride2", "g2", "dil3g2") for c_ in ("gauss",)] +
                         [("edge", c_) for c_ in H.DCN_EDGE_CLASSES[1:]])
def test_dcn_column_path_vs_float64(name, cls):
    """rr_dcn_im2col and rr_dcn_col2im directly: the columns against the float64 columns (yardstick: the float32 oracle's columns),
    and d input / d offset / d mask of a GIVEN column gradient (the float32 chain over k of dY x W, so that only the kernel under
    test separates the result from the reference) against the float64 model of the same column gradient.  Float atomics: no
    fixed-point allowance."""
    from rrnet_amd import ops
    geo = H.DCN64_GRID[name]
    n, c, h, w, k, r, s, stride, ph, pw, dil, dg = geo
    cs = _case(geo, cls, 0, False)
    dev = [ops.to_nhwc(t.cuda()) if t.dim() == 4 else t.cuda() for t in cs.inputs]
    p, q = cs.ref["out"].shape[2:]
    col = ops.dcn_im2col(dev[0], dev[1], dev[2], r, s, stride, (ph, pw), dil, dg)                    # memory [M][tap][c]
    got_col = col.permute(0, 2, 3, 1).reshape(n, p, q, r * s, c).permute(0, 4, 3, 1, 2)
    failed = []
    ratios, _, ok = cs.check("cols", _nchw(got_col))
    print("%-8s %-9s fp32  %-32s %-22s %-8s max %.3f rms %.3f all %.3f fx=0.00" % (name, cls, "rr_dcn_im2col", "columns", "cols", *ratios))
    failed += [] if ok else [("cols", ratios)]
    dcol32 = cs.y["dcol"]                                                                           # [n, c, T, P, Q] float32
    ref = H.dcn_model(*cs.inputs[:5], stride, (ph, pw), dil, dg, dcol=dcol32.astype(np.float64))
    dcol_dev = torch.from_numpy(np.ascontiguousarray(dcol32.transpose(0, 3, 4, 2, 1))).reshape(1, n * p * q, 1, r * s * c).permute(0, 3, 1, 2).cuda()
    outs = ops.dcn_col2im(dev[0], dev[1], dev[2], dcol_dev, r, s, stride, (ph, pw), dil, dg)
    for tensor, val in zip(("dx", "doffset", "dmask"), outs):
        idx, yd = cs.yard(tensor)
        yd = H.dcn_yardstick(tensor, idx, cs.y, ref[tensor][idx])
        rt, _ = H.dcn_error_ratios(_nchw(val), ref[tensor], idx, yd)
        print("%-8s %-9s fp32  %-32s %-22s %-8s max %.3f rms %.3f all %.3f fx=0.00" % (name, cls, "rr_dcn_col2im", "columns", tensor, *rt))
        failed += [] if H.conv_accepts(rt, H.DCN_MARGIN) else [(tensor, rt)]
    assert not failed, failed


def test_dcn_split_kernels_vs_float64():
    """rr_dcn_split_fwd (offset = the first two thirds, mask = sigmoid of the last) and rr_dcn_split_bwd against float64.  Bound: the
    sigmoid is one exp, one add and one division in float32 — 4 roundings of a value in (0, 1), so |error| <= 4 x 2^-24, taken times
    DCN_MARGIN for the library's exp; its derivative m (1 - m) g adds three more roundings relative to |g| / 4."""
    from rrnet_amd import ops
    g = torch.Generator().manual_seed(3)
    n, t, p, q = 2, 9, 9, 17
    om = torch.randn(n, 3 * t, p, q, generator=g) * 3.0
    om[0, 2 * t:, 0, :4] = torch.tensor([0.0, -30.0, 30.0, 88.0])
    off, mask = ops.dcn_split_fwd(ops.to_nhwc(om.cuda()))
    assert torch.equal(off.cpu(), om[:, :2 * t])
    m64 = torch.sigmoid(om[:, 2 * t:].double())
    err = (mask.cpu().double() - m64).abs().max().item()
    print("split_fwd mask err / 2^-24 = %.3f" % (err / H.U32))
    assert err <= 4 * H.U32 * H.DCN_MARGIN
    doff, dmask = torch.randn(n, 2 * t, p, q, generator=g), torch.randn(n, t, p, q, generator=g)
    dom = ops.dcn_split_bwd(ops.to_nhwc(doff.cuda()), ops.to_nhwc(dmask.cuda()), mask).cpu()
    assert torch.equal(dom[:, :2 * t], doff)
    mk = mask.cpu().double()                               # the kernel differentiates at ITS mask
    want = dmask.double() * mk * (1 - mk)
    err = ((dom[:, 2 * t:].double() - want).abs() / (dmask.double().abs() / 4 + 1e-300)).max().item()
    print("split_bwd err / (|g| / 4 x 2^-24) = %.3f" % (err / H.U32))
    assert err <= 3 * H.U32 * H.DCN_MARGIN


def test_dcn_far_and_exact_samples_contribute_nothing():
    """Samples exactly at -1 / H / W and far outside (1e4, 3e9 beyond int32, 1e30) give exactly zero d offset and d mask on a window
    and on a gather route, in both precisions (the strict inside test)."""
    from rrnet_amd import ops
    for name in H.DCN64_EDGE_CASES:
        geo = H.DCN64_GRID[name]
        n, c, h, w, k, r, s, stride, ph, pw, dil, dg = geo
        for cls in ("far", "exact"):
            cs = _case(geo, cls, 0, False)
            out = ~cs.m64["geo"]["inside"]                                                            # [n, dg, T, P, Q]
            assert out.sum() > 20
            dev = [ops.to_nhwc(t.cuda()) if t.dim() == 4 else t.cuda() for t in cs.inputs]
            for entry in ("rr_dcn_dgrad", "rr_dcn_dgrad_bf16_packed"):
                _, doff, dmask = _call_dgrad(entry, dev, geo, None)
                dm = _nchw(dmask).reshape(out.shape)
                do = _nchw(doff).reshape(n, dg, r * s, 2, *out.shape[-2:])
                assert (dm[out] == 0).all() and (do[:, :, :, 0][out] == 0).all() and (do[:, :, :, 1][out] == 0).all(), (name, cls, entry)
