"""GPU tests of the dense and the SE hourglass: the kernels of csrc/se.hip, the two autograd nodes, the residual block, the
tiny networks and the models on them.

Discrete results (ReLU masks, pool taps) must equal the float64 restatement of tests/hgvariant_cases.py — test_hgvariants_host.py
proves on the CPU that float32 decides each of them as float64 does.  Values must lie within 4x the float32 restatement's own
error against float64, with a floor of 2 u max|ref| (the rule of tests/test_retina_gpu.py).  The 2x2 pool is bit-equal to
ATen's on the device.  Blocks are held to the reference's own records in tests/golden/hgvariants.npz with the tolerances of
tests/test_model_gpu.py.

No whole-tensor reference data of the tiny NETWORKS is committed: a whole record is tens of MB (11.7 M parameters in dense3),
float32 would halve that and no more.  The golden holds a compact record of them (every 64th output channel, every 4th pixel
of the input gradient, the SE weights' gradients, sum and sum of squares of every parameter gradient);
test_hgvariants_host.py holds the float64 restatement to every number of it at 1e-9 of scale, and the networks here are
compared with that restatement's whole outputs and gradients, computed once per case on the CPU, with the tolerances
tests/test_model_gpu.py applies to ctnet_tiny.npz: outputs atol = rtol = 1e-3, gradient norms rtol 5e-3 / atol 1e-5, every
gradient element max(8 x the float32 restatement's own error, 16 x the float64 gradient's movement under one float32
rounding of the input, 1e-3 of the gradient's scale) + 1e-7.  Every test prints its figures (pytest -s).
"""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import hgvariant_cases as hc
from helpers import det_fill, shapes_of

pytestmark = pytest.mark.gpu
CL = torch.channels_last
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _dev(t):
    """float64 CPU [n,c,h,w] -> float32 NHWC on the device (the cases' values are float32-representable)."""
    return t.float().cuda().contiguous(memory_format=CL)


def close(a, b, atol=1e-3, rtol=1e-3):
    np.testing.assert_allclose(_np(a) if torch.is_tensor(a) else np.asarray(a), np.asarray(b), atol=atol, rtol=rtol)


def gclose(a, b, rel=2e-3):
    b = np.asarray(b, dtype=np.float64)
    scale = max(np.abs(b).max(), 1e-6)
    assert np.abs(_np(a) - b).max() <= rel * scale + 1e-6, (np.abs(_np(a) - b).max(), scale)


# ----------------------------------------------------------------------------------------------------------------------
# squeeze, excite, scale: forward and backward
# ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _se_refs(name):
    case = hc.se_case(name)
    return case, hc.se_reference(case, torch.float64), hc.se_reference(case, torch.float32)


def _se_run(case):
    from rrnet_amd import ops
    u, skip, dout = _dev(case["u"]), _dev(case["skip"]), _dev(case["dout"])
    w1, w2 = case["w1"].float().cuda(), case["w2"].float().cuda()
    hw = u.shape[2] * u.shape[3]
    m, h, s = ops.se_excite_fwd(ops.se_squeeze(u), w1, w2, hw)
    out = ops.se_scale_res_relu_fwd(u, s, skip)
    dw1, dw2 = torch.zeros_like(w1), torch.zeros_like(w2)
    dm = ops.se_excite_bwd(ops.se_bwd_reduce(dout, out, u), s, h, m, w1, w2, dw1, dw2)
    into = _dev(case["into"]) if case["into"] is not None else None
    du, dskip = ops.se_bwd_apply(dout, out, s, dm, dskip_into=into)
    assert (dskip is None) == (into is not None)
    return dict(m=m, h=h, s=s, out=out, dm=dm, dw1=dw1, dw2=dw2, du=du, dskip=into if into is not None else dskip)


@pytest.mark.parametrize("name", sorted(hc.SE_CASES))
def test_se_kernels_against_float64(name):
    case, r64, r32 = _se_refs(name)
    got, again = _se_run(case), _se_run(case)
    torch.cuda.synchronize()
    print(name)
    for k in sorted(got):
        assert torch.equal(got[k], again[k]), "%s differs between two runs" % k             # fixed-order reductions
    assert np.array_equal(_np(got["out"]) > 0, r64["mask"])
    assert np.array_equal(_np(got["h"]) > 0, r64["hmask"])
    assert np.array_equal(_np(got["dskip"]) == (_np(_dev(case["into"])) if case["into"] is not None else 0.0), ~r64["mask"])
    for k in ("m", "h", "s", "out", "dm", "dw1", "dw2", "du", "dskip"):
        hc.judge(k, _np(got[k]), r64[k], r32[k])


def test_se_node_is_the_kernel_chain_and_hands_back_fresh_gradients():
    """functional.se_scale_res_relu on a case of the table: outputs and gradients are those of the kernels called one by one;
    the weights' gradients come back to autograd when the parameters are in no FlatParams."""
    from rrnet_amd import functional as RF
    case, r64, r32 = _se_refs("n3_hw65_c48_r16")
    want = _se_run(case)
    u, skip = _dev(case["u"]).requires_grad_(), _dev(case["skip"]).requires_grad_()
    w1, w2 = case["w1"].float().cuda().requires_grad_(), case["w2"].float().cuda().requires_grad_()
    out = RF.se_scale_res_relu(u, w1, w2, skip, 16)
    assert getattr(out, "_rr_bnlink", None) is None
    dout = _dev(case["dout"])
    out.backward(dout)
    for got, k in ((out, "out"), (u.grad, "du"), (skip.grad, "dskip"), (w1.grad, "dw1"), (w2.grad, "dw2")):
        assert torch.equal(got, want[k]), k
    assert u.grad.data_ptr() != dout.data_ptr() and skip.grad.data_ptr() != dout.data_ptr()


def test_channels_not_a_multiple_of_4_are_refused():
    from rrnet_amd import _C, ops
    u = torch.zeros(1, 6, 4, 4, device="cuda").contiguous(memory_format=CL)
    with pytest.raises(_C.RRNetHipError, match="rr_se_squeeze"):
        ops.se_squeeze(u)
    with pytest.raises(_C.RRNetHipError, match="rr_se_scale_res_relu_fwd"):
        ops.se_scale_res_relu_fwd(u, torch.zeros(1, 6, device="cuda"), u)
    with pytest.raises(_C.RRNetHipError, match="rr_maxpool2x2_fwd"):
        ops.maxpool2x2_fwd(u)


# ----------------------------------------------------------------------------------------------------------------------
# MaxPool2d(2)
# ----------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("c", hc.POOL_CHANNELS)
@pytest.mark.parametrize("h,w", hc.POOL_SIZES)
def test_maxpool2x2_bit_equal_to_aten(h, w, c):
    from rrnet_amd import _C, functional as RF, ops
    x = hc.pool_case(h, w, c).cuda().contiguous(memory_format=CL)
    if h < 2 or w < 2:                                   # ATen refuses an empty output, and so does the kernel
        with pytest.raises(RuntimeError):
            F.max_pool2d(x, 2)
        with pytest.raises(_C.RRNetHipError, match="rr_maxpool2x2_fwd"):
            ops.maxpool2x2_fwd(x)
        return
    xa = x.clone().requires_grad_()
    ya = F.max_pool2d(xa, 2)
    y, tap = ops.maxpool2x2_fwd(x)
    assert y.shape == ya.shape and torch.equal(_bits(y), _bits(ya.detach()))
    _, tap64 = hc.pool_reference(x.cpu().double())
    assert torch.equal(tap.cpu(), tap64)
    dy = torch.from_numpy(np.random.default_rng(h * 10 + w).normal(0, 1, tuple(y.shape)).astype(np.float32)).cuda().contiguous(memory_format=CL)
    ya.backward(dy)
    dx = ops.maxpool2x2_bwd(dy, tap, tuple(x.shape))
    assert torch.equal(_bits(dx), _bits(xa.grad))
    assert torch.equal(dx.cpu(), hc.pool_backward_reference(dy.cpu(), tap64, h, w))
    if h % 2:
        assert not dx[:, :, -1].any()                    # the odd last row / column: written, with zeros
    if w % 2:
        assert not dx[:, :, :, -1].any()
    xn = x.clone().requires_grad_()                      # the autograd node
    yn = RF.max_pool2x2(xn)
    yn.backward(dy)
    assert torch.equal(_bits(yn.detach()), _bits(y)) and torch.equal(_bits(xn.grad), _bits(dx))


# ----------------------------------------------------------------------------------------------------------------------
# SE residual block against the reference's records
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return np.load(os.path.join(golden_dir, "hgvariants.npz"))


@pytest.mark.parametrize("tag", sorted(hc.BLOCK_CASES))
def test_se_residual_block_vs_reference_golden(golden, tag):
    from rrnet_amd.backbones.se_hourglass import ResidualBlock
    (cin, cout, stride), shape = hc.BLOCK_CASES[tag]
    mod = ResidualBlock(cin, cout, stride)
    mod.load_state_dict(det_fill(shapes_of(mod.state_dict()), 40), strict=True)
    mod = mod.cuda().to(memory_format=CL).train()
    x = _dev(hc.det_input(shape, 41)).requires_grad_()
    y = mod(x)
    close(y, golden[tag + "/train/y"], atol=1e-4)
    y.backward(_dev(hc.det_input(tuple(y.shape), 44)))
    gclose(x.grad, golden[tag + "/train/gx"])
    for k, p in mod.named_parameters():
        gclose(p.grad, golden[tag + "/train/grad/" + k])
    for k, b in mod.named_buffers():
        if b.is_floating_point():
            close(b.float(), golden[tag + "/train/buf/" + k], atol=1e-4)
    mod.eval()
    with torch.no_grad():
        close(mod(x.detach()), golden[tag + "/eval/y"], atol=1e-4)


# ----------------------------------------------------------------------------------------------------------------------
# tiny networks against the float64 restatement (which test_hgvariants_host.py holds to the reference's records)
# ----------------------------------------------------------------------------------------------------------------------
GOLDEN = os.path.join(ROOT, "tests", "golden", "hgvariants.npz")


def _settled_state(tag, shapes):
    """det_fill's weights with the golden's settled BatchNorm biases (no ReLU input of the case within RELU_MARGIN of 0)."""
    z = np.load(GOLDEN)
    return hc.apply_nudges(det_fill(shapes, 60), z[tag + "/nudge_keys"], z[tag + "/nudge_ch"], z[tag + "/nudge_val"])


def _restated(tag, dtype, perturb=0.0):
    """The restatement's train-mode run at `dtype`, then its eval-mode run -> outputs, input / parameter gradients (float64 numpy)."""
    variant, stacks, batch = hc.NET_CASES[tag]
    net = hc.tiny_net(variant, stacks)
    net.load_state_dict(_settled_state(tag, shapes_of(net.state_dict())), strict=True)
    net = hc.full_momentum(net.to(dtype)).train()
    x = hc.det_input((batch, 3) + hc.NET_HW, 61)
    if perturb:
        x = x * (1 + perturb * torch.randn(x.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(5)))
    x = x.to(dtype).requires_grad_()
    outs = list(net(x))
    torch.autograd.backward(outs, [hc.det_input(tuple(o.shape), 77 + i).to(dtype) for i, o in enumerate(outs)])
    res = dict(outs=[_np(o) for o in outs], gx=_np(x.grad), grads={k: _np(p.grad) for k, p in net.named_parameters()})
    with torch.no_grad():
        net.eval()
        res["eval"] = [_np(o) for o in net(x.detach())]
    return res


@functools.lru_cache(maxsize=None)
def _net_refs(tag):
    """float64 truth, the same under one float32 rounding of the input, the float32 restatement."""
    return _restated(tag, torch.float64), _restated(tag, torch.float64, perturb=6e-8), _restated(tag, torch.float32)


@pytest.mark.parametrize("tag", sorted(hc.NET_CASES))
def test_tiny_network_vs_float64_restatement(tag):
    """Outputs (train and eval mode), gradient norms and every gradient element with the tolerances tests/test_model_gpu.py
    applies to ctnet_tiny.npz, unamended.  What makes them attainable is the fixture, not the bound: the cases' BatchNorm
    biases are settled (hgvariant_cases.settle_relus) so that no ReLU input lies within 1e-3 of 0 — with det_fill's weights as
    they come, ONE decision that fell the other way moved residual.0.conv1.weight's gradient of dense2 by 14 % of its scale
    on the MI355X, and float32 torch on the CPU was itself 6 % off float64 on se2 — and BatchNorm runs with momentum 1, so the
    eval pass is normalised (on the initial statistics (0, 1) the features reach 370 and four elements of dense3 missed the
    absolute 1e-3 by 1.9e-3)."""
    from rrnet_amd.utils.model_tools import get_backbone
    variant, stacks, batch = hc.NET_CASES[tag]
    truth, moved, ref32 = _net_refs(tag)
    net = get_backbone("%s_hourglass_tiny" % variant, num_stacks=stacks)
    net.load_state_dict(_settled_state(tag, shapes_of(net.state_dict())), strict=True)
    net = hc.full_momentum(net).cuda().to(memory_format=CL).train()
    x = _dev(hc.det_input((batch, 3) + hc.NET_HW, 61)).requires_grad_()
    outs = net(x)
    assert len(outs) == stacks
    for i, o in enumerate(outs):
        close(o, truth["outs"][i])
    torch.autograd.backward(list(outs), [_dev(hc.det_input(tuple(o.shape), 77 + i)) for i, o in enumerate(outs)])
    named = dict(net.named_parameters())
    keys = sorted(truth["grads"])
    assert sorted(named) == keys
    l2 = np.array([float(named[k].grad.norm()) for k in keys])
    np.testing.assert_allclose(l2, [np.sqrt((truth["grads"][k] ** 2).sum()) for k in keys], rtol=5e-3, atol=1e-5)
    worst = ("", 0.0, 0.0)
    for name, got in [(k, named[k].grad) for k in keys] + [("input", x.grad)]:
        t, m, r = ((d["grads"][name] if name != "input" else d["gx"]) for d in (truth, moved, ref32))
        scale = max(np.abs(t).max(), 1e-6)
        noise, e_ref = np.abs(m - t).max(), np.abs(r - t).max()
        bound = max(8 * e_ref, 16 * noise, 1e-3 * scale) + 1e-7
        e_mine = np.abs(_np(got) - t).max()
        if e_mine / bound > worst[1]:
            worst = (name, e_mine / bound, e_mine / scale)
        assert e_mine <= bound, (name, e_mine, e_ref, noise, scale)
    print("%s: %d gradients, worst error / bound %.3f at %s (%.2e of its scale)" % (tag, len(keys) + 1, worst[1], worst[0], worst[2]))
    net.eval()
    with torch.no_grad():
        for i, o in enumerate(net(x.detach())):
            close(o, truth["eval"][i])


# ----------------------------------------------------------------------------------------------------------------------
# the models on the new backbones
# ----------------------------------------------------------------------------------------------------------------------
def _cfg(backbone, stacks=2):
    return SimpleNamespace(num_classes=10, Model=SimpleNamespace(num_stacks=stacks, backbone=backbone, nms_type_for_stage1="nms",
                                                                 nms_per_class_for_stage1=True),
                           Train=SimpleNamespace(scale_factor=4))


def _ctnet_loss(model, batch):
    from rrnet_amd import functional as RF
    imgs, annos, hms, whs, inds, offs, masks, _ = batch
    o = model(imgs)
    n = len(o[0])
    return sum(RF.focal_loss_hm_from_logits(o[0][i], hms) + 0.1 * RF.reg_l1_loss(o[1][i], masks, inds, whs)
               + RF.reg_l1_loss(o[2][i], masks, inds, offs) for i in range(n)) / n


@pytest.mark.parametrize("backbone", ["dense_hourglass_tiny", "se_hourglass_tiny"])
def test_centernet_trains_on_the_new_backbone(backbone):
    """Three optimiser steps through FlatParams and FlatAdam: finite losses, every SE weight moved.  The first step's gradients
    equal those of the same model without FlatParams (autograd receives the gradients) to 1e-3 of the parameter's scale, the
    bound of tests/test_train_gpu.py::test_flat_grads_match_autograd_grads — on every SE weight (the node this backbone adds has
    no atomics), and on every parameter whose autograd-path gradient moves by <= 1e-5 of its scale under a 1e-7 disturbance
    of the images: the small-map convolutions' split-K atomics round differently from run to run, and a ReLU decision that
    falls the other way moves the gradients upstream of it by per cents.  The choice of parameters is made on the autograd
    path, as tests/test_dp_gpu.py::test_rccl_single_rank_step_matches_non_distributed makes it on its plain run; the
    ill-conditioned rest is only held to 0.2 of scale (a missed or doubled slot is off by 1)."""
    from rrnet_amd.datasets.synthetic import synth_batch
    from rrnet_amd.flat import FlatAdam, FlatParams
    from rrnet_amd.models.centernet import CenterNet
    batch = synth_batch(2, 128, 128, boxes_per_image=6)
    torch.manual_seed(11)
    plain = CenterNet(_cfg(backbone)).cuda().to(memory_format=CL).train()
    state = {k: v.clone() for k, v in plain.state_dict().items()}

    def fresh():
        m = CenterNet(_cfg(backbone))
        m.load_state_dict(state)
        return m.cuda().to(memory_format=CL).train()
    _ctnet_loss(plain, batch).backward()
    want = {k: p.grad.clone() for k, p in plain.named_parameters()}
    nudged = fresh()
    noise = torch.randn(batch[0].shape, generator=torch.Generator(device="cuda").manual_seed(5), device="cuda")
    _ctnet_loss(nudged, ((batch[0] * (1 + 1e-7 * noise)).contiguous(memory_format=CL),) + tuple(batch[1:])).backward()
    scale = {k: max(float(g.abs().max()), 1e-30) for k, g in want.items()}
    sens = {k: float((p.grad - want[k]).abs().max()) / scale[k] for k, p in nudged.named_parameters()}
    model = fresh()
    fp = FlatParams(model)
    opt = FlatAdam(fp, lr=1e-3)
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    losses = []
    for step in range(3):
        opt.zero_grad()
        loss = _ctnet_loss(model, batch)
        loss.backward()
        if step == 0:
            torch.cuda.synchronize()
            cross = {k: float((p._rr_grad - want[k]).abs().max()) / scale[k] for k, p in model.named_parameters()}
            good = [k for k in cross if sens[k] <= 1e-5]
            se = [k for k in cross if ".se.fc." in k]
            cv, sv = np.array(list(cross.values())), np.array(list(sens.values()))
            print("%s: FlatParams gradients against autograd's: %d of %d parameters well-conditioned, worst difference on those "
                  "%.2e of scale, on the %d SE weights %.2e; all: median %.2e worst %.2e (1e-7 image noise: median %.2e worst %.2e)"
                  % (backbone, len(good), len(cross), max([cross[k] for k in good] or [0.0]), len(se), max([cross[k] for k in se] or [0.0]),
                     np.median(cv), cv.max(), np.median(sv), sv.max()))
            assert len(good) >= 10
            for k in good + se:
                assert cross[k] <= 1e-3 + 1e-5 / scale[k], (k, cross[k], sens[k])
            # the ill-conditioned rest: two runs are two draws of the same noise (in one run of the suite the worst difference was
            # 3.5e-2 where the 1e-7 disturbance had moved a gradient by 9.7e-3), so only the coarse property is asked of them: a
            # gradient that missed its flat slot, or landed in it twice, is off by its whole scale
            assert cv.max() <= 0.2, cv.max()
        opt.step()
        losses.append(float(loss))
    assert np.all(np.isfinite(losses)), losses
    se_keys = [k for k in before if ".se.fc." in k]
    assert (len(se_keys) > 0) == backbone.startswith("se_")
    for k, p in model.named_parameters():
        if k in se_keys:
            assert bool((p.detach() != before[k]).any()), k
    print("%s: losses %s, %d SE weights moved" % (backbone, ["%.4f" % l for l in losses], len(se_keys)))


def test_one_rank_data_parallel_step_equals_the_plain_step_with_the_se_backbone(tmp_path):
    """RR_DP_FORCE=1 on one rank (a one-rank RCCL group, SyncBN's joint nodes, bucketed gradient all-reduce) with
    se_hourglass_tiny, in a child process: the step equals the non-distributed one the way
    tests/test_dp_gpu.py::test_rccl_single_rank_step_matches_non_distributed asks of the hourglass."""
    from test_streams_gpu import DET, _load, _rel, _run
    extra = ["--backbone", "se_hourglass_tiny"]
    plain = _run(tmp_path, "plain", dict(DET, RR_WGRAD_STREAM="2"), 128, 2, 2, extra + ["--perturb", "1e-7"])
    forced = _run(tmp_path, "rccl1", dict(DET, RR_WGRAD_STREAM="2", RR_DP_FORCE="1"), 128, 2, 2, extra)
    cc, nb = forced[1]["collectives"], forced[1]["buckets"]
    assert plain[1]["collectives"][0] == {}
    for c in cc:
        assert c["grads"] == nb and c["default"] == cc[0]["default"] and c["default"] > 0, (c, nb)
    assert any(".se.fc." in n for n in forced[1]["names"])
    la, lb = np.array(plain[1]["losses"][0]), np.array(forced[1]["losses"][0])
    assert np.all(np.abs(la - lb) <= 1e-4 * np.maximum(np.abs(la), 1e-3)), (la, lb)
    sl = plain[1]["slices"]
    g0 = _load(plain[0], "grad.bin")
    sens, _ = _rel(_load(plain[0], "grad2.bin"), g0, sl)              # response to 1e-7 input noise
    cross, _ = _rel(_load(forced[0], "grad.bin"), g0, sl)
    good = sens <= 1e-5
    print("one-rank RCCL step vs plain step, se_hourglass_tiny: %d of %d parameters well-conditioned, worst difference on those "
          "%.2e; all: median %.2e worst %.2e (1e-7 input noise: median %.2e worst %.2e)"
          % (int(good.sum()), good.numel(), float(cross[good].max()), float(cross.median()), float(cross.max()),
             float(sens.median()), float(sens.max())))
    assert int(good.sum()) >= 10
    assert float(cross[good].max()) <= 1e-4
    assert float(cross.median()) <= 3 * max(float(sens.median()), 1e-5)
    assert float(cross.max()) <= 3 * max(float(sens.max()), 1e-3)
    r = forced[1]["repeat_vs_first"][0]
    assert r["grad"][0] <= 1e-5 and r["buffers"] <= 2e-5, r


def test_detect_frames_centernet_runs_on_the_se_backbone():
    """The eval path: BatchNorm folded into conv2, the SE node behind it.  Random weights: the rows' shape and finiteness."""
    from rrnet_amd import inference
    from rrnet_amd.models.centernet import CenterNet
    torch.manual_seed(3)
    model = CenterNet(_cfg("se_hourglass_tiny")).cuda().to(memory_format=CL).eval()
    frames = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (2, 128, 160, 3), dtype=np.uint8)).cuda()
    boxes, frame_off = inference.detect_frames_centernet(model, frames, [1, 1.25], (0.485, 0.456, 0.406), (0.229, 0.224, 0.225),
                                                         nms=False)
    rows, fo = boxes.cpu().numpy(), frame_off.cpu().numpy()
    assert rows.ndim == 2 and rows.shape[1] == 6 and fo.shape == (3,) and fo[0] == 0 and fo[-1] == rows.shape[0]
    assert rows.shape[0] > 0 and np.all(np.isfinite(rows)) and set(np.unique(rows[:, 5])) <= set(range(1, 11))
