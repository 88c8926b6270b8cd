"""ShuffleNetV2's kernels on the MI355X (csrc/depthwise.hip).

Depthwise 3x3, cases tests/shufflenet_cases.DW_CASES: forward (with and without bias), data gradient and weight gradient (with and
without `accumulate`) against the float64 oracle, judged by the error of the same sums chained in float32
(shufflenet_cases.*(dtype=float32)) with the margin 4; every output buffer starts as NaN; two runs are bitwise equal.  One line
per (case, tensor) is printed: profiles/dw_fp64_ratios.txt is that output of an MI355X run.  The slab equals the float64 sums
of the kernel's own y.  The shuffle family is bit-exact against torch indexing, sliced operands included, and each backward is
the exact inverse.  Every refusal returns its status.

The two units of tests/golden/shufflenet.npz (the reference's own InvertedResidual in float64): train-mode output, input and
parameter gradients, BatchNorm buffers and the eval-mode output, judged by the golden's own float32 run with the margin 4.
One RetinaNet train step on shufflenet_v2_x0_5, and its folded eval forward against the network with its BatchNorm layers left
unfolded on the running statistics."""
import numpy as np
import pytest
import torch

import shufflenet_cases as sc

pytestmark = pytest.mark.gpu
CL = torch.channels_last
_REF = {}


def _reference(case):
    """(inputs, float64 oracle, chained float32) of a case, computed once."""
    if case not in _REF:
        n, h, w, c, s = case
        x, f, bias, dy, df0 = sc.dw_inputs(case)
        both = []
        for dtype in (np.float64, np.float32):
            both.append(dict(y=sc.dw_fwd(x, f, s, dtype=dtype), y_bias=sc.dw_fwd(x, f, s, bias, dtype=dtype),
                             dx=sc.dw_bwd_data(dy, f, s, h, w, dtype=dtype), df=sc.dw_bwd_weight(x, dy, s, dtype=dtype),
                             df_acc=sc.dw_bwd_weight(x, dy, s, df0, dtype=dtype)))
        _REF[case] = ((x, f, bias, dy, df0), both[0], both[1])
    return _REF[case]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _nan(*shape, dtype=torch.float32):
    return torch.full(shape, float("nan"), dtype=dtype, device="cuda")


def _raw(case, x, f, bias, dy, df0):
    """The three entries on NaN-filled outputs (NHWC device tensors) -> dict."""
    from rrnet_amd import _C, ops
    fam = _C.Family("rrnet_hip_dw.h")
    n, h, w, c, s = case
    p, q = sc.out_hw(h, w, s)
    tile, tiles = ops.dw_tile_pixels(n * p * q)
    mtiles = -(-(n * p * q) // ops.DW_SLAB_PIXELS)
    out = dict(y=_nan(n, p, q, c), y_bias=_nan(n, p, q, c), y_stats=_nan(n, p, q, c), slab=_nan(mtiles, 2, c, dtype=torch.float64),
               dx=_nan(n, h, w, c), df=_nan(c, 3, 3), df_acc=df0.clone(), tiles=tiles, mtiles=mtiles)
    fam.call("rr_dwconv3x3_fwd", x, f, None, out["y"], None, n, h, w, c, s)
    fam.call("rr_dwconv3x3_fwd", x, f, bias, out["y_bias"], None, n, h, w, c, s)
    fam.call("rr_dwconv3x3_fwd", x, f, None, out["y_stats"], out["slab"], n, h, w, c, s)
    fam.call("rr_dwconv3x3_bwd_data", dy, f, out["dx"], n, h, w, c, s)
    fam.call("rr_dwconv3x3_bwd_weight", x, dy, _nan(tiles, c, 9, dtype=torch.float64), out["df"], 0, n, h, w, c, s, tile)
    fam.call("rr_dwconv3x3_bwd_weight", x, dy, _nan(tiles, c, 9, dtype=torch.float64), out["df_acc"], 1, n, h, w, c, s, tile)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("case", sc.DW_CASES, ids=str)
def test_depthwise_kernels_against_the_float64_oracle(case):
    from rrnet_amd import functional as RF, ops
    (x, f, bias, dy, df0), ref, seq = _reference(case)
    n, h, w, c, s = case
    dev = [_dev(a) for a in (x, f, bias, dy, df0)]
    got = _raw(case, *dev)
    again = _raw(case, *dev)
    if case == (2, 33, 65, 88, 1):
        assert got["tiles"] > 1 and got["mtiles"] > 1
    bad = []
    for t in ("y", "y_bias", "dx", "df", "df_acc"):
        g = got[t].cpu().numpy()
        assert np.isfinite(g).all(), (case, t)                    # written whole (the buffers started as NaN)
        assert torch.equal(got[t], again[t]), (case, t)          # two runs: the same bits
        ratios = sc.error_ratios(g, ref[t], seq[t])
        print("dw64 %-18s %-6s max-abs ratio %6.3f rms ratio %6.3f   (chained float32: max-abs %.3e)"
              % ("%dx%dx%dx%d/s%d" % case, t, ratios[0], ratios[1], float(np.abs(seq[t] - ref[t]).max())))
        if not sc.accepts(ratios):
            bad.append((t, ratios))
    assert not bad, (case, bad)
    # the slab: float64 sums of the kernel's own y, tile by tile and in total; asking for it does not change y
    assert torch.equal(got["y_stats"], got["y"]) and torch.equal(got["slab"], again["slab"])
    y64 = got["y"].double().reshape(-1, c)
    slab = got["slab"]
    assert bool(torch.isfinite(slab).all())
    pad = torch.zeros((got["mtiles"] * ops.DW_SLAB_PIXELS - y64.shape[0], c), dtype=torch.float64, device="cuda")
    tiles = torch.cat([y64, pad]).reshape(got["mtiles"], ops.DW_SLAB_PIXELS, c)
    for row, vals in ((0, tiles), (1, tiles * tiles)):
        assert bool(((slab[:, row] - vals.sum(1)).abs() <= 1e-12 * vals.abs().sum(1)).all()), (case, row)
        assert bool(((slab[:, row].sum(0) - vals.sum((0, 1))).abs() <= 1e-12 * vals.abs().sum((0, 1))).all()), (case, row)
    # the wrappers launch the same kernels on the same memory
    xd, fd, bd, dyd, df0d = dev
    xn, dyn, wp = xd.permute(0, 3, 1, 2), dyd.permute(0, 3, 1, 2), fd.reshape(c, 1, 3, 3)
    y, slab2 = ops.dwconv3x3_fwd(xn, wp, None, s, want_stats=True)
    assert ops.is_nhwc(y) and torch.equal(y.permute(0, 2, 3, 1), got["y"]) and torch.equal(slab2, slab)
    assert torch.equal(ops.dwconv3x3_fwd(xn, wp, bd, s).permute(0, 2, 3, 1), got["y_bias"])
    assert torch.equal(ops.dwconv3x3_bwd_data(dyn, wp, tuple(xn.shape), s).permute(0, 2, 3, 1), got["dx"])
    assert torch.equal(ops.dwconv3x3_bwd_weight(xn, dyn, torch.empty_like(wp), s).reshape(c, 3, 3), got["df"])
    assert torch.equal(ops.dwconv3x3_bwd_weight(xn, dyn, df0d.clone().reshape(c, 1, 3, 3), s, accumulate=True).reshape(c, 3, 3),
                       got["df_acc"])


def test_timer_sees_the_launches():
    from rrnet_amd import ops
    case = (2, 7, 9, 8, 1)
    x, f, bias, dy, df0 = (_dev(a) for a in _reference(case)[0])
    xn, dyn, wp = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2), f.reshape(8, 1, 3, 3)
    ops.TIMER = ops.KernelTimer()
    try:
        ops.dwconv3x3_fwd(xn, wp)
        ops.dwconv3x3_bwd_data(dyn, wp, tuple(xn.shape))
        ops.dwconv3x3_bwd_weight(xn, dyn, torch.empty_like(wp))
        ops.shuffle_deinterleave(ops.shuffle_interleave(xn[:, :4], xn[:, 4:]))
        seen = ops.TIMER.summary()
    finally:
        ops.TIMER = None
    assert {"dwconv3x3_fwd", "dwconv3x3_bwd_data", "dwconv3x3_bwd_weight", "shuffle_interleave", "shuffle_deinterleave"} <= set(seen)


# ---- the shuffle family -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 8, 1, 1), (2, 48, 5, 6), (3, 96, 7, 3), (2, 976, 3, 5), (2, 176, 33, 65)], ids=str)
def test_shuffle_family_is_bit_exact_and_its_backward_the_inverse(shape):
    from rrnet_amd import functional as RF, ops
    n, c, h, w = shape
    half = c // 2
    g = torch.Generator(device="cuda").manual_seed(c)
    x = torch.randn((n, h, w, c), device="cuda", generator=g).permute(0, 3, 1, 2)          # NHWC memory
    o = torch.randn((n, h, w, half), device="cuda", generator=g).permute(0, 3, 1, 2)

    def shuffled(a, b):                                        # the reference's channel_shuffle(cat(a, b), 2), by indexing
        cat = torch.cat([a, b], 1)
        return cat.reshape(n, 2, half, h, w).transpose(1, 2).reshape(n, c, h, w)

    # sliced operands: the lower half of x in place, a tensor of its own beside it; and both halves of x in place
    for a, b in ((x[:, :half], o), (o, x[:, half:]), (x[:, :half], x[:, half:])):
        out = ops.shuffle_interleave(a, b)
        assert ops.is_nhwc(out) and torch.equal(out, shuffled(a, b))
        da, db = ops.shuffle_deinterleave(out)
        assert ops.is_nhwc(da) and ops.is_nhwc(db) and torch.equal(da, a) and torch.equal(db, b)
    # the de-interleave into slices of one tensor (da straight into the lower half of a unit's dx)
    into = torch.full((n, h, w, c), float("nan"), device="cuda").permute(0, 3, 1, 2)
    ops.shuffle_deinterleave(shuffled(x[:, :half], x[:, half:]).contiguous(memory_format=CL), into[:, :half], into[:, half:])
    assert torch.equal(into, x)
    # the two copies of a stride-1 unit: the upper half out, two halves back into one tensor
    hi = ops.channel_copy(x[:, half:])
    assert ops.is_nhwc(hi) and torch.equal(hi, x[:, half:]) and hi.data_ptr() != x.data_ptr()
    assert torch.equal(ops.channel_join(x[:, :half], hi), x) and torch.equal(ops.channel_join(o, x[:, :half]), torch.cat([o, x[:, :half]], 1))
    back = torch.full((n, h, w, c), float("nan"), device="cuda").permute(0, 3, 1, 2)
    ops.channel_copy(hi, back[:, half:])
    ops.channel_copy(x[:, :half], back[:, :half])
    assert torch.equal(back, x)
    # the autograd nodes: split -> shuffle is a permutation of x, its backward the inverse permutation of the gradient
    leaf = x.clone().requires_grad_()
    lo, up = RF.split_halves(leaf)
    assert lo.data_ptr() == leaf.data_ptr() and up.data_ptr() != leaf.data_ptr()         # the passthrough half is not copied
    y = RF.shuffle_cat(lo, up)
    assert torch.equal(y, shuffled(x[:, :half], x[:, half:]))
    gy = torch.randn((n, h, w, c), device="cuda", generator=g).permute(0, 3, 1, 2)
    y.backward(gy)
    assert torch.equal(leaf.grad, torch.cat([gy[:, 0::2], gy[:, 1::2]], 1))
    two = [t.clone().requires_grad_() for t in (o, o * 2)]
    RF.shuffle_cat(*two).backward(gy)
    assert torch.equal(two[0].grad, gy[:, 0::2]) and torch.equal(two[1].grad, gy[:, 1::2])


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_status():
    from rrnet_amd import _C
    fam = _C.Family("rrnet_hip_dw.h")
    t = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    big = t(1, 16, 16, 64)                                        # roomy operands: a wrongly accepted call stays inside them
    bigd = torch.zeros(4096, dtype=torch.float64, device="cuda")
    off = t(1, 16, 16, 64 + 1).reshape(-1)[1:]                    # 4 bytes past a 16-byte boundary

    def dw(dims, swap=None):
        """The three entries on `dims`; swap = (position among the entry's required pointers, replacement)."""
        fwd, bwd, wg = [big, big, big, big, bigd], [big, big, big], [big, big, bigd, big, 0]
        if swap is not None:
            k, value = swap
            fwd[(0, 1, 3)[k]], bwd[k], wg[(0, 1, 3)[k]] = value, value, value            # (x, f, y) / (dy, f, dx) / (x, dy, df)
        return (("rr_dwconv3x3_fwd", fwd, dims), ("rr_dwconv3x3_bwd_data", bwd, dims), ("rr_dwconv3x3_bwd_weight", wg, dims + (64,)))

    good = (1, 4, 4, 8, 1)
    refused = [dw((1, 4, 4, 6, 1)), dw((1, 4, 4, 0, 1)),                                     # c % 4, c = 0
               dw((1, 4, 4, 8, 3)), dw((1, 4, 4, 8, 0)),                                     # s outside {1, 2}
               dw((1, 0, 4, 8, 1)), dw((1, 4, 0, 8, 2)), dw((0, 4, 4, 8, 1)),                # h, w, n below 1
               dw((1, 16384, 8192, 4, 1)), dw((16, 4096, 4096, 4, 2)),                       # 2 GiB, and more
               dw(good, (0, None)), dw(good, (1, None)), dw(good, (2, None)),                # a null required pointer
               dw(good, (0, off))]                                                           # a pointer off the 16-byte grid
    for entries in refused:
        for entry, args, dims in entries:
            with pytest.raises(_C.RRNetHipError, match=entry + " failed"):
                fam.call(entry, *args, *dims)
    with pytest.raises(_C.RRNetHipError, match="rr_dwconv3x3_bwd_weight failed"):            # the partial sums' buffer
        fam.call("rr_dwconv3x3_bwd_weight", big, big, None, big, 0, *good, 64)
    with pytest.raises(_C.RRNetHipError, match="tile_pixels"):
        fam.call("rr_dwconv3x3_bwd_weight", big, big, bigd, big, 0, 1, 4, 4, 8, 1, 0)
    shuffles = [
        ("rr_shuffle_interleave", (big, 8, big, 8, big, 16, 4, 6)),                          # half % 4
        ("rr_shuffle_interleave", (big, 8, big, 6, big, 16, 4, 8)),                          # a stride that breaks the alignment
        ("rr_shuffle_interleave", (big, 8, big, 8, big, 12, 4, 8)),                          # a stride below its channels
        ("rr_shuffle_interleave", (None, 8, big, 8, big, 16, 4, 8)), ("rr_shuffle_interleave", (big, 8, big, 8, None, 16, 4, 8)),
        ("rr_shuffle_interleave", (off, 8, big, 8, big, 16, 4, 8)),
        ("rr_shuffle_interleave", (big, 8, big, 8, big, 16, 0, 8)),
        ("rr_shuffle_interleave", (big, 8, big, 8, big, 16, 1 << 26, 8)),                    # 2 GiB of output
        ("rr_shuffle_deinterleave", (big, 16, big, 8, big, 8, 4, 2)), ("rr_shuffle_deinterleave", (big, 16, big, 10, big, 8, 4, 8)),
        ("rr_shuffle_deinterleave", (big, 16, None, 8, big, 8, 4, 8)), ("rr_shuffle_deinterleave", (big, 16, big, 8, off, 8, 4, 8)),
        ("rr_shuffle_deinterleave", (big, 8, big, 8, big, 8, 4, 8)),
        ("rr_channel_copy", (big, 8, big, 8, 4, 7)), ("rr_channel_copy", (big, 9, big, 8, 4, 8)), ("rr_channel_copy", (big, 8, None, 8, 4, 8)),
        ("rr_channel_copy", (off, 8, big, 8, 4, 8)), ("rr_channel_copy", (big, 8, big, 4, 4, 8)),
        ("rr_channel_join", (big, 8, big, 8, big, 16, 4, 5)), ("rr_channel_join", (big, 8, big, 8, big, 18, 4, 8)),
        ("rr_channel_join", (big, 8, None, 8, big, 16, 4, 8)), ("rr_channel_join", (big, 8, big, 8, big, 8, 4, 8)),
    ]
    for entry, args in shuffles:
        with pytest.raises(_C.RRNetHipError, match=entry + " failed"):
            fam.call(entry, *args)
    torch.cuda.synchronize()
    assert not big.any() and not bigd.any()                       # no refused call launched anything


# ---- the units against the reference's record ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return sc.load_golden()


def _judge(name, got, g64, g32, bad):
    got, g64 = np.asarray(got, np.float64), np.asarray(g64, np.float64)
    ratios = sc.error_ratios(got, g64, np.asarray(g32, np.float64))
    print("shufflenet-units %-34s max-abs ratio %6.3f rms ratio %6.3f   (float32 run: max-abs %.3e)"
          % (name, ratios[0], ratios[1], float(np.abs(np.asarray(g32, np.float64) - g64).max())))
    if not sc.accepts(ratios):
        bad.append((name, ratios))


def test_units_against_the_golden(golden):
    from rrnet_amd.backbones.shufflenet import InvertedResidual
    m = torch.nn.Sequential(*[InvertedResidual(*u) for u in sc.UNITS])
    m.load_state_dict({k: torch.as_tensor(a).float() if a.dtype == np.float64 else torch.as_tensor(a)
                       for k, a in sc.golden_state(golden).items()}, strict=True)
    m = m.cuda().to(memory_format=CL).train()
    x = torch.from_numpy(golden["x"]).cuda().contiguous(memory_format=CL).requires_grad_()
    y = m(x)
    y.backward(torch.from_numpy(golden["gy"]).cuda().contiguous(memory_format=CL))
    torch.cuda.synchronize()
    bad = []
    _judge("y", y.detach().cpu().numpy(), golden["y"], golden["f32/y"], bad)
    _judge("dx", x.grad.cpu().numpy(), golden["dx"], golden["f32/dx"], bad)
    for name, p in m.named_parameters():
        assert p.grad is not None, name
        _judge("grad/" + name, p.grad.cpu().numpy(), golden["grad/" + name], golden["f32/grad/" + name], bad)
    for name, b in m.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(golden["buf/" + name]) == 1
        else:
            _judge("buf/" + name, b.cpu().numpy(), golden["buf/" + name], golden["f32/buf/" + name], bad)
    with torch.no_grad():
        y_eval = m.eval()(x.detach())
    _judge("y_eval", y_eval.cpu().numpy(), golden["y_eval"], golden["f32/y_eval"], bad)
    assert not bad, bad


# ---- one RetinaNet step -------------------------------------------------------------------------------------------------------
def _shufflenet_unfolded(bb, imgs):
    """ShuffleNetV2 with every BatchNorm left as a layer of its own on its running statistics (nothing folded into a filter):
    conv / depthwise conv / BatchNorm / ReLU / cat / shuffle restated with torch in float64 on the host -> (os8, os16, os32)."""
    import torch.nn.functional as F

    def seq(s, x):
        for mod in s:
            if isinstance(mod, torch.nn.Conv2d):
                x = F.conv2d(x, mod.weight, None, mod.stride, mod.padding, 1, mod.groups)
            elif isinstance(mod, torch.nn.BatchNorm2d):
                x = F.batch_norm(x, mod.running_mean, mod.running_var, mod.weight, mod.bias, False, 0.0, mod.eps)
            else:
                x = F.relu(x)
        return x

    def unit(u, x):
        if u.benchmodel == 1:
            half = x.shape[1] // 2
            out = torch.cat([x[:, :half], seq(u.banch2, x[:, half:])], 1)
        else:
            out = torch.cat([seq(u.banch1, x), seq(u.banch2, x)], 1)
        n, c, h, w = out.shape
        return out.reshape(n, 2, c // 2, h, w).transpose(1, 2).reshape(n, c, h, w)

    x = F.max_pool2d(seq(bb.conv1, imgs), 3, 2, 1)
    maps = []
    for i, u in enumerate(bb.features):
        x = unit(u, x)
        if i in (3, 11):
            maps.append(x)
    maps.append(seq(bb.conv_last, x))
    return maps


def _resnet_unfolded(bb, imgs):
    """The same for resnet10 -> (l2, l3, l4)."""
    import torch.nn.functional as F
    bn = lambda m, x: F.batch_norm(x, m.running_mean, m.running_var, m.weight, m.bias, False, 0.0, m.eps)
    conv = lambda m, x: F.conv2d(x, m.weight, None, m.stride, m.padding)
    x = F.max_pool2d(F.relu(bn(bb.bn1, conv(bb.conv1, imgs))), 3, 2, 1)
    maps = []
    for stage in (bb.layer1, bb.layer2, bb.layer3, bb.layer4):
        for blk in stage:
            out = F.relu(bn(blk.bn1, conv(blk.conv1, x)))
            out = F.relu(bn(blk.bn2, conv(blk.conv2, out)))
            res = bn(blk.downsample[1], conv(blk.downsample[0], x)) if blk.downsample is not None else x
            x = F.relu(bn(blk.bn3, conv(blk.conv3, out)) + res)
        maps.append(x)
    return maps[1:]


def test_one_retinanet_step_on_shufflenet_v2_x0_5():
    """2 x 3 x 64 x 96: finite losses, a finite gradient for every parameter, non-zero gradients for the depthwise filters; then
    the eval forward (BatchNorm folded into the filters, one launch per depthwise layer) against the network with its BatchNorm
    layers left unfolded on the same running statistics (float64), per backbone map by relative L2.  The tolerance is 4 times
    the same folded-against-unfolded figure of resnet10, measured here on the same input."""
    import copy
    import retina_cases as rc
    from rrnet_amd import functional as RF
    from rrnet_amd.models.retinanet import RetinaNet
    size = (64, 96)
    g = torch.Generator().manual_seed(7)
    imgs = torch.randn((2, 3) + size, generator=g).cuda().contiguous(memory_format=CL)
    annos = rc.criterion_batch("base")[[0, 2]]
    torch.manual_seed(31)
    model = RetinaNet(rc.retina_cfg("shufflenet_v2_x0_5", crop=size)).cuda().to(memory_format=CL).train()
    loc, cls = model(imgs)
    cl, ll = RF.retina_criterion(loc, cls, torch.from_numpy(annos).cuda(), rc.anchors_of(size).cuda(), 10)
    (cl + ll).backward()
    torch.cuda.synchronize()
    assert loc.shape[0] == 2 and loc.shape[2] == 4 and cls.shape[:2] == loc.shape[:2]
    assert bool(torch.isfinite(cl)) and bool(torch.isfinite(ll)), (float(cl), float(ll))
    depthwise = 0
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        if p.dim() == 4 and p.shape[1] == 1 and tuple(p.shape[2:]) == (3, 3):
            depthwise += 1
            assert bool(p.grad.any()), name
    assert depthwise == 19
    for name, b in model.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b) == 1, name

    def folded_against_unfolded(net, unfolded):
        net = net.eval()
        with torch.no_grad():
            maps = net.backbone(imgs)[-3:]
            want = unfolded(copy.deepcopy(net.backbone).cpu().double(), imgs.cpu().double().contiguous())
        torch.cuda.synchronize()
        return [rc.rel_l2(m.double().cpu().numpy(), w.numpy()) for m, w in zip(maps, want)]

    torch.manual_seed(32)
    resnet = RetinaNet(rc.retina_cfg("resnet10", crop=size)).cuda().to(memory_format=CL).train()
    with torch.no_grad():
        resnet(imgs)                                             # one train-mode forward: running statistics away from 0 / 1
    yard = folded_against_unfolded(resnet, _resnet_unfolded)
    ours = folded_against_unfolded(model, _shufflenet_unfolded)
    print("\nfolded eval against the unfolded network, relative L2 per map (os8, os16, os32): resnet10 %s, shufflenet_v2_x0_5 %s"
          % (", ".join("%.3g" % v for v in yard), ", ".join("%.3g" % v for v in ours)))
    assert all(np.isfinite(v) and v > 0 for v in yard)
    assert max(ours) <= 4 * max(yard), (ours, yard)
