"""The dilated-window attention on the MI355X (csrc/attn.hip).

Kernels, cases A-E of tests/attn_cases.py: ctx, dq, dk, dv against the float64 oracle, judged by the error of the same sums
chained in float32 (attn_cases.window_rule(dtype=float32)) with the margin 4; every output buffer starts as NaN; two runs
are bitwise equal; every refusal returns its status.  One line per (case, tensor) is printed: profiles/attn_fp64_ratios.txt
is that output of an MI355X run.

SelfAttentionModule against tests/golden/self_attention.npz (the reference's own class in float64): train-mode output,
input and parameter gradients, BatchNorm buffers and the eval-mode output, judged by the golden's own float32 run with
the margin 4.  The model switch cfg.Model.attention on hourglass_tiny."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_cases as ac

pytestmark = pytest.mark.gpu
CL = torch.channels_last
_REF = {}


def _reference(name):
    """(inputs, float64 oracle, chained float32) of a case, computed once."""
    if name not in _REF:
        c = ac.CASES[name]
        inp = ac.case_inputs(name)
        geom = (c["kernel"], c["dilation"], c["padding"])
        _REF[name] = (inp, ac.window_rule(*inp[:3], *geom, dctx=inp[3]), ac.window_rule(*inp[:3], *geom, dctx=inp[3], dtype=np.float32))
    return _REF[name]


def _dev(a):
    """NHWC float64 array -> float32 device tensor, logical NCHW on NHWC memory."""
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda().permute(0, 3, 1, 2)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def _raw(name, q, k, v, dctx):
    """The three entries on NaN-filled outputs -> dict of NHWC device tensors."""
    from rrnet_amd import _C
    fam = _C.Family("rrnet_hip_attn.h")
    c = ac.CASES[name]
    n, (h, w), ck, cv = c["n"], c["hw"], c["ck"], c["cv"]
    oh, ow, _, _ = ac.geometry(h, w, c["kernel"], c["dilation"], c["padding"])
    taps = c["kernel"][0] * c["kernel"][1]
    dims = (n, h, w, ck, cv) + c["kernel"] + c["dilation"] + c["padding"]
    out = dict(ctx=_nan(n, oh, ow, cv), p=_nan(n, oh, ow, taps), ds=_nan(n, oh, ow, taps), dq=_nan(n, h, w, ck),
               dk=_nan(n, h, w, ck), dv=_nan(n, h, w, cv))
    fam.call("rr_attn_fwd", q, k, v, out["ctx"], out["p"], *dims)
    fam.call("rr_attn_bwd_q", dctx, v, k, out["p"], out["ds"], out["dq"], *dims)
    fam.call("rr_attn_bwd_kv", out["ds"], out["p"], q, dctx, out["dk"], out["dv"], *dims)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", sorted(ac.CASES))
def test_kernels_against_the_float64_oracle(name):
    from rrnet_amd import functional as RF, ops
    (q, k, v, dctx), ref, seq = _reference(name)
    dq_, dk_, dv_, dd_ = _dev(q), _dev(k), _dev(v), _dev(dctx)
    # (the entries take the NHWC memory: a logical-NCHW view of it is what ops hands them)
    got = _raw(name, dq_, dk_, dv_, dd_)
    again = _raw(name, dq_, dk_, dv_, dd_)
    bad = []
    for t in ("ctx", "p", "ds", "dq", "dk", "dv"):
        g = got[t].cpu().numpy()
        assert np.isfinite(g).all(), (name, t)                    # written whole (the buffers started as NaN), nothing overflowed
        assert torch.equal(got[t], again[t]), (name, t)          # two runs: the same bits
        ratios = ac.error_ratios(g, ref[t], seq[t])
        print("attn64 %s %-3s max-abs ratio %6.3f rms ratio %6.3f   (chained float32: max-abs %.3e)"
              % (name, t, ratios[0], ratios[1], float(np.abs(seq[t] - ref[t]).max())))
        if t in ("ctx", "dq", "dk", "dv") and not ac.accepts(ratios):
            bad.append((t, ratios))
    assert not bad, (name, bad)
    c = ac.CASES[name]
    _, _, cy, cx = ac.geometry(*c["hw"], c["kernel"], c["dilation"], c["padding"])
    if cy > 0:
        assert not got["dq"][:, :cy].any()                       # query rows no output reads: exactly 0
    # the wrappers and the autograd node launch the same kernels on the same memory
    geom = (c["kernel"], c["dilation"], c["padding"])
    ctx, p = ops.window_attention_fwd(dq_, dk_, dv_, *geom)
    grads = ops.window_attention_bwd(dd_, dq_, dk_, dv_, p, *geom)
    assert ops.is_nhwc(ctx) and torch.equal(ctx.permute(0, 2, 3, 1), got["ctx"]) and torch.equal(p, got["p"])
    for t, g in zip(("dq", "dk", "dv"), grads):
        assert ops.is_nhwc(g) and torch.equal(g.permute(0, 2, 3, 1), got[t]), t
    leaves = [t.clone().requires_grad_() for t in (dq_, dk_, dv_)]
    RF.window_attention(*leaves, *geom).backward(dd_)
    for t, leaf in zip(("dq", "dk", "dv"), leaves):
        assert torch.equal(leaf.grad.permute(0, 2, 3, 1), got[t]), t


def test_timer_sees_the_three_launches():
    from rrnet_amd import ops
    (q, k, v, dctx), _, _ = _reference("A")
    c = ac.CASES["A"]
    geom = (c["kernel"], c["dilation"], c["padding"])
    ops.TIMER = ops.KernelTimer()
    try:
        ctx, p = ops.window_attention_fwd(_dev(q), _dev(k), _dev(v), *geom)
        ops.window_attention_bwd(_dev(dctx), _dev(q), _dev(k), _dev(v), p, *geom)
        seen = ops.TIMER.summary()
    finally:
        ops.TIMER = None
    assert {"attn_fwd", "attn_bwd_q", "attn_bwd_kv"} <= set(seen) and all(seen[k]["launches"] == 1 for k in seen)


def test_every_refusal_returns_its_status():
    from rrnet_amd import _C
    fam = _C.Family("rrnet_hip_attn.h")
    t = lambda *s: torch.zeros(s, dtype=torch.float32, device="cuda")
    n, h, w = 1, 6, 6
    q, k, v = t(n, h, w, 8), t(n, h, w, 8), t(n, h, w, 8)
    big = t(n, 16, 16, 64)                                       # roomy outputs: a wrongly accepted call stays inside them

    def calls(dims, null=None):
        a = [q, k, v, big, big]
        b = [big, v, k, big, big, big]
        c = [big, big, q, big, big, big]
        if null is not None:
            a[null], b[null], c[null] = None, None, None
        return (("rr_attn_fwd", a), ("rr_attn_bwd_q", b), ("rr_attn_bwd_kv", c)), dims

    good = (n, h, w, 8, 8, 3, 3, 1, 1, 1, 1)
    refused = [
        (calls((n, h, w, 6, 8, 3, 3, 1, 1, 1, 1)), "% 4"),                                  # ck % 4
        (calls((n, h, w, 8, 10, 3, 3, 1, 1, 1, 1)), "% 4"),                                 # cv % 4
        (calls((n, h, w, 8, 8, 3, 3, 1, 1, 2, 1)), "centre"),                               # cy < 0
        (calls((n, h, w, 8, 8, 3, 3, 1, 1, 1, 2)), "centre"),                               # cx < 0
        (calls((n, h, w, 8, 8, 3, 3, 4, 1, 1, 1)), "empty"),                                # oh < 1
        (calls((n, h, w, 8, 8, 3, 3, 1, 4, 1, 1)), "empty"),                                # ow < 1
        (calls((n, h, w, 8, 8, 2, 3, 1, 1, 1, 1)), "without a query"),                      # cy + oh > h
        (calls((n, h, w, 8, 8, 9, 9, 1, 1, 4, 4)), "64 taps"),                              # above the tap limit
        (calls((0, h, w, 8, 8, 3, 3, 1, 1, 1, 1)), "below 1"),
        (calls(good, null=0), "null"), (calls(good, null=3), "null"), (calls(good, null=4), "null"),
    ]
    for (entries, dims), what in refused:
        for entry, args in entries:
            with pytest.raises(_C.RRNetHipError, match=what):
                fam.call(entry, *args, *dims)
    fam.call("rr_attn_fwd", t(1, 20, 20, 4), t(1, 20, 20, 4), t(1, 20, 20, 4), t(1, 20, 20, 4), t(1, 20, 20, 49), 1, 20, 20, 4, 4,
             7, 7, 2, 2, 6, 6)                                   # the limit admits 7x7
    torch.cuda.synchronize()
    assert not big.any()                                         # no refused call launched anything


# ---- the module against the reference's record --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return ac.load_golden()


def _judge(tag, name, got, g64, g32, bad):
    got, g64 = np.asarray(got, np.float64), np.asarray(g64, np.float64)
    ratios = ac.error_ratios(got, g64, np.asarray(g32, np.float64))
    print("attn-module %s %-28s max-abs ratio %6.3f rms ratio %6.3f   (float32 run: max-abs %.3e)"
          % (tag, name, ratios[0], ratios[1], float(np.abs(np.asarray(g32, np.float64) - g64).max())))
    if not ac.accepts(ratios):
        bad.append((name, ratios))


@pytest.mark.parametrize("tag", ["A", "B"])
def test_module_against_the_golden(golden, tag):
    """Bias gradients of the four convolutions that a train-mode BatchNorm follows are identically zero; the module produces
    none (modules/self_attention.py:_conv_bn_relu), and zero is what is judged."""
    from rrnet_amd.modules.self_attention import SelfAttentionModule
    c = ac.MODULE_CASES[tag]
    g = lambda key: golden["%s/%s" % (tag, key)]
    m = SelfAttentionModule(c["cin"], c["ck"], c["cv"], kernel_size=c["kernel"], dilation=c["dilation"], padding=c["padding"])
    m.load_state_dict({k: torch.as_tensor(a) for k, a in ac.golden_state(golden, tag).items()}, strict=True)
    m = m.float().cuda().train()
    x = torch.from_numpy(g("x")).cuda().contiguous(memory_format=CL).requires_grad_()
    y = m(x)
    assert tuple(y.shape) == tuple(g("y").shape)
    y.backward(torch.from_numpy(g("gy")).cuda().contiguous(memory_format=CL))
    bad = []
    _judge(tag, "y", y.detach().cpu().numpy(), g("y"), g("f32/y"), bad)
    _judge(tag, "dx", x.grad.cpu().numpy(), g("dx"), g("f32/dx"), bad)
    for name, p in m.named_parameters():
        grad = np.zeros(tuple(p.shape)) if p.grad is None else p.grad.cpu().numpy()
        if p.grad is None:
            assert name.endswith(".bias") and name.split(".")[0] in ("f_key", "f_query") and name.split(".")[1] in ("0", "3"), name
        _judge(tag, "grad/" + name, grad, g("grad/" + name), g("f32/grad/" + name), bad)
    for name, b in m.named_buffers():
        if name.endswith("num_batches_tracked"):
            assert int(b) == int(g("buf/" + name)) == 1
        else:
            _judge(tag, "buf/" + name, b.cpu().numpy(), g("buf/" + name), g("f32/buf/" + name), bad)
    with torch.no_grad():
        y_eval = m.eval()(x.detach())
    _judge(tag, "y_eval", y_eval.cpu().numpy(), g("y_eval"), g("f32/y_eval"), bad)
    assert not bad, (tag, bad)


# ---- the model switch ---------------------------------------------------------------------------------------------------
def _cfg(**model):
    base = dict(num_stacks=2, backbone="hourglass_tiny", nms_type_for_stage1="nms", nms_per_class_for_stage1=True)
    base.update(model)
    return SimpleNamespace(num_classes=10, Model=SimpleNamespace(**base), Train=SimpleNamespace(scale_factor=4))


def test_rrnet_with_attention_starts_as_the_plain_model_and_trains_w():
    from helpers import host_synth_batch as synth_batch
    from rrnet_amd.models.rrnet import RRNet
    from rrnet_amd.utils.model_tools import attention_kwargs
    torch.manual_seed(21)
    plain = RRNet(_cfg())
    torch.manual_seed(22)
    model = RRNet(_cfg(attention=attention_kwargs(5, 6)))
    missing = model.load_state_dict(plain.state_dict(), strict=False)
    assert missing.missing_keys and all(k.startswith("attention.") for k in missing.missing_keys) and not missing.unexpected_keys
    imgs = synth_batch(2, 128, 128, boxes_per_image=10, seed=3)[0].cuda()
    plain = plain.cuda().to(memory_format=CL).train()
    model = model.cuda().to(memory_format=CL).train()
    want = plain(imgs, k=50)
    outs = model(imgs, k=50)
    for a, b in zip(want[:3], outs[:3]):                         # W = 0: the heads read the same feature, bit for bit
        for s in range(2):
            assert torch.equal(a[s], b[s])
    gen = torch.Generator().manual_seed(4)
    sum((o * torch.randn(o.shape, generator=gen).cuda()).sum() for head in outs[:3] for o in head).backward()
    for s in range(2):
        w = model.attention[s].W
        assert torch.isfinite(w.weight.grad).all() and float(w.weight.grad.abs().sum()) > 0
        assert torch.isfinite(w.bias.grad).all() and float(w.bias.grad.abs().sum()) > 0


def test_guarded_train_step_with_attention():
    from rrnet_amd.configs.rrnet_config import Config as cfg
    from rrnet_amd.operators.rrnet_operator import RRNetOperator
    from rrnet_amd.utils.model_tools import attention_kwargs
    saved, saved_train = dict(cfg.Model), dict(cfg.Train)
    try:
        cfg.Train.batch_size, cfg.Train.crop_size = 2, (128, 128)
        cfg.Train.max_grad_norm, cfg.Train.skip_nonfinite = 35.0, True
        cfg.Model.backbone, cfg.Model.attention = "hourglass_tiny", attention_kwargs(5, 6)
        cfg.Distributed.gpu_id, cfg.Distributed.rank, cfg.Distributed.world_size = 0, 0, 1
        torch.manual_seed(cfg.seed)
        op = RRNetOperator(cfg)
        op.model.train()
        w = op.model.module.attention[1].W.weight
        assert not w.any()
        b = op.training_loader.get_batch()
        _, losses = op.train_step(2000, (b[0], b[1].clone()) + tuple(b[2:]))
        assert all(np.isfinite(float(v.detach())) for v in losses)
        assert torch.isfinite(op.model.flat.grad).all() and torch.isfinite(op.model.flat.flat).all()
        assert w.any()                                            # the zero-initialised W has moved
    finally:
        for store, old in ((cfg.Model, saved), (cfg.Train, saved_train)):
            for key in list(store):
                if key not in old:
                    del store[key]
            store.update(old)
