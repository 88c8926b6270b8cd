"""GPU: the guarded optimiser step (csrc/optim.hip) against the float64 restatement of tests/guard_cases.py:
the norm reduction at every size where the kernel takes another path, non-finite gradients, 12-step sequences with
clipping, a skip and the EMA warm-up, agreement with rr_adam_step, FlatAdam on the tiny CenterNet against torch on the
CPU, and the state-file round trip."""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import guard_cases as G
from helpers import det_fill

pytestmark = pytest.mark.gpu
CL = torch.channels_last
THREADS = G.header_define("RR_GRAD_NORM_THREADS")
ATOL, RTOL = 2e-6, 1e-5            # tests/test_train_gpu.py::test_fused_adam_matches_torch_adam


def _blocks_of(n):
    from rrnet_amd import ops
    return ops.grad_norm_blocks(n)


CASES = ("one-vector", "block-full", "block-minus-vector", "block-plus-vector", "partial-last-block", "grid-stride-wraps")
_SIZES = {}


def _size(case):
    """n of a named case (guard_cases.sizes: from the exported block count and the kernel's thread count)."""
    if not _SIZES:
        _SIZES.update(G.sizes(_blocks_of, THREADS))
        assert tuple(_SIZES) == CASES
    return _SIZES[case]


def _dev(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()


def _ctl_dev(ctl=None):
    from rrnet_amd import ops
    return (ops.guard_ctl_fresh() if ctl is None else torch.from_numpy(np.asarray(ctl, dtype=np.float64))).cuda()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _norm_and_decide(g, ctl, **kw):
    from rrnet_amd import ops
    partial, bad = ops.grad_norm(g)
    ops.guard_decide(partial, bad, ctl, **kw)
    return partial, bad


@pytest.mark.parametrize("case", CASES)
def test_norm_against_float64(case):
    """norm against the float64 sum to a relative 1e-9 (squares are exact in double; summing N <= 5e6 positive terms
    rounds at most N * 2^-53 = 5e-10); the partials equal the restated summation order bit for bit; two runs give a
    bit-equal ctl."""
    n = _size(case)
    blocks = _blocks_of(n)
    assert blocks == min(-(-n // (4 * THREADS)), _blocks_of(1 << 40))
    g = G.gradient(n, 11 + n % 1000)
    gd = _dev(g)
    ctls = []
    for _ in range(2):
        ctl = _ctl_dev()
        partial, bad = _norm_and_decide(gd, ctl, grad_scale=0.5, max_norm=1.0, lr=1e-3)
        ctls.append(ctl.cpu().numpy())
    S, B = G.sum_squares(g)
    want = math.sqrt(S) * 0.5
    got = ctls[0][G.IX["norm"]]
    print("%s: n %d blocks %d norm %.17g float64 %.17g rel %.3g" % (case, n, blocks, got, want, abs(got - want) / want))
    assert B == 0 and ctls[0][G.IX["bad"]] == 0 and ctls[0][G.IX["skip"]] == 0
    assert abs(got - want) <= 1e-9 * want
    assert np.array_equal(ctls[0].view(np.uint64), ctls[1].view(np.uint64))
    p_ref, b_ref = G.device_order_partials(g, blocks, THREADS)
    assert partial.shape == (blocks,) and np.array_equal(partial.cpu().numpy().view(np.uint64), p_ref.view(np.uint64))
    assert np.array_equal(bad.cpu().numpy(), b_ref)
    ref = G.decide(G.fresh_ctl(), G.device_order_sum(g, blocks, THREADS)[0], 0, grad_scale=0.5, max_norm=1.0, lr=1e-3)
    assert np.array_equal(ctls[0].view(np.uint64), ref.view(np.uint64))


def test_empty_gradient_launches_nothing():
    from rrnet_amd import ops
    assert _blocks_of(0) == 0
    g = torch.zeros(0, device="cuda")
    partial, bad = ops.grad_norm(g)
    assert partial.numel() == 0 and bad.numel() == 0
    ctl = ops.guard_decide(partial, bad, _ctl_dev(), max_norm=1.0).cpu().numpy()
    assert ctl[G.IX["norm"]] == 0 and ctl[G.IX["applied"]] == 1 and ctl[G.IX["scale"]] == 1
    ops.adam_step_guarded(g, g, g, g, None, 1e-8, _ctl_dev())


def _state(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(n).astype(np.float32)
    m = (rng.standard_normal(n) * 0.01).astype(np.float32)
    v = (rng.random(n) * 1e-3).astype(np.float32)
    ema = (p + rng.standard_normal(n).astype(np.float32) * 0.01).astype(np.float32)
    return p, m, v, ema


def test_nonfinite_gradient_is_counted_and_skipped():
    """NaN, +Inf and -Inf at the first word, the last word and a workgroup's first and last word: `bad` is exact per
    workgroup and in total, `skip` is set, the guarded Adam launch leaves all four buffers bit-unchanged, `applied`
    and the running products stay, `skipped` moves by one.  With skip_nonfinite = 0 the same gradient is applied."""
    from rrnet_amd import ops
    n = _size("partial-last-block")
    blocks = _blocks_of(n)
    assert blocks == 6
    g = G.gradient(n, 3)
    first_of_block2, last_of_block2 = 2 * THREADS * 4, 3 * THREADS * 4 - 1
    g[0], g[n - 1], g[first_of_block2] = np.nan, np.inf, -np.inf
    g.view(np.uint32)[last_of_block2] = 0xffc00123                  # a negative NaN with a payload
    gd = _dev(g)
    # a record with one applied step behind it, so that the products are not 1
    before = G.decide(G.fresh_ctl(), 4.0, 0, lr=1e-3, ema_decay=0.9, ema_warmup=True)
    ctl = _ctl_dev(before)
    partial, bad = _norm_and_decide(gd, ctl, skip_nonfinite=True, max_norm=1.0, lr=1e-3, ema_decay=0.9, ema_warmup=True)
    b = bad.cpu().numpy()
    assert b.tolist() == [1, 0, 2, 0, 0, 1] and ((n // 4 - 1) // THREADS) % blocks == 5
    assert np.isfinite(partial.cpu().numpy()).all()
    after = ctl.cpu().numpy()
    assert after[G.IX["bad"]] == 4 and after[G.IX["skip"]] == 1 and math.isinf(after[G.IX["norm"]])
    assert after[G.IX["skipped"]] == before[G.IX["skipped"]] + 1
    want = G.decide(before, G.device_order_sum(g, blocks, THREADS)[0], 4, skip_nonfinite=True, max_norm=1.0, lr=1e-3,
                    ema_decay=0.9, ema_warmup=True)
    assert np.array_equal(after.view(np.uint64), want.view(np.uint64))
    for slot in ("applied", "beta1_pow", "beta2_pow", "clipped", "scale", "step_size", "bc2_sqrt", "ema_d", "ema_omd"):
        assert after[G.IX[slot]] == before[G.IX[slot]], slot
    host = _state(n, 8)
    dev = [_dev(a) for a in host]
    ops.adam_step_guarded(dev[0], gd, dev[1], dev[2], dev[3], 1e-8, ctl)
    for name, a, d in zip(("param", "exp_avg", "exp_avg_sq", "ema"), host, dev):
        assert np.array_equal(_bits(d), a.view(np.uint32)), name
    # the same gradient without the skip: applied, with the gradient's own scale (a non-finite norm clips nothing)
    ctl2 = _ctl_dev(before)
    _norm_and_decide(gd, ctl2, skip_nonfinite=False, grad_scale=0.5, max_norm=1.0, lr=1e-3)
    c2 = ctl2.cpu().numpy()
    assert c2[G.IX["skip"]] == 0 and c2[G.IX["bad"]] == 4 and c2[G.IX["applied"]] == before[G.IX["applied"]] + 1
    assert c2[G.IX["scale"]] == 0.5 and c2[G.IX["skipped"]] == 0 and c2[G.IX["norm_max"]] == before[G.IX["norm_max"]]


def _sequence(n, steps=12, nan_step=6):
    grads = [G.gradient(n, 40 + t, scale=0.1 * (1 + t % 3)) for t in range(steps)]
    grads[nan_step][n // 2] = np.inf
    norms = sorted(0.5 * math.sqrt(G.sum_squares(g)[0]) for t, g in enumerate(grads) if t != nan_step)
    return grads, 0.5 * (norms[3] + norms[4])           # a bound between the norms: binds on some steps, not on others


@pytest.mark.parametrize("with_ema", [True, False])
def test_twelve_steps_against_the_restatement(with_ema):
    """12 steps, ema_decay 0.5 with the warm-up ramp (it governs the first steps, the decay the rest), grad_scale 0.5, a
    bound that clips some steps and not others, one skipped step.  After EVERY step ctl slots 0-4 and 9-13 (and the four
    beta floats) equal the restatement exactly; the norm to 1e-9; at the end the buffers within the fused Adam's
    tolerance (an EMA is a convex combination: about 2 ulp per step on top)."""
    from rrnet_amd import ops
    n, lr = _size("partial-last-block"), 1e-3
    blocks = _blocks_of(n)
    grads, max_norm = _sequence(n)
    p, m, v, ema = (a.astype(np.float64) for a in _state(n, 21))
    m[:] = 0.0
    v[:] = 0.0
    if not with_ema:
        ema = None
    dp, dm, dv = _dev(p), _dev(m), _dev(v)
    dema = _dev(ema) if with_ema else None
    ctl, dctl = G.fresh_ctl(), _ctl_dev()
    kw = dict(grad_scale=0.5, max_norm=max_norm, skip_nonfinite=True, lr=lr, beta1=0.9, beta2=0.999,
              ema_decay=0.5 if with_ema else 0.0, ema_warmup=with_ema)
    for t, g in enumerate(grads):
        gd = _dev(g)
        _norm_and_decide(gd, dctl, **kw)
        ops.adam_step_guarded(dp, gd, dm, dv, dema, 1e-8, dctl)
        S, B = G.device_order_sum(g, blocks, THREADS)
        ctl = G.decide(ctl, S, B, **kw)
        p, m, v, ema = G.adam_ema(p, m, v, ema, g, ctl)
        got = dctl.cpu().numpy()
        exact = list(G.EXACT_SLOTS) + [7, 8, 14, 15, 16, 17, 18, 19]
        assert np.array_equal(got[exact].view(np.uint64), ctl[exact].view(np.uint64)), (t, got, ctl)
        if math.isfinite(ctl[G.IX["norm"]]):
            assert abs(got[G.IX["norm"]] - ctl[G.IX["norm"]]) <= 1e-9 * ctl[G.IX["norm"]]
        else:
            assert math.isinf(got[G.IX["norm"]])
        assert abs(got[G.IX["norm_max"]] - ctl[G.IX["norm_max"]]) <= 1e-9 * ctl[G.IX["norm_max"]]
    assert ctl[G.IX["applied"]] == 11 and ctl[G.IX["skipped"]] == 1 and 3 <= ctl[G.IX["clipped"]] <= 8
    if with_ema:
        assert ctl[G.IX["ema_d"]] == 0.5
    pairs = [("param", dp, p), ("exp_avg", dm, m), ("exp_avg_sq", dv, v)] + ([("ema", dema, ema)] if with_ema else [])
    for name, d, ref in pairs:
        err = np.abs(d.cpu().numpy().astype(np.float64) - ref)
        print("%s: max abs err %.3g" % (name, err.max()))
        np.testing.assert_allclose(d.cpu().numpy(), ref, atol=ATOL, rtol=RTOL, err_msg=name)


def test_guarded_step_agrees_with_the_unguarded_kernel():
    """max_norm = inf and finite gradients: three guarded steps against rr_adam_step on the same inputs."""
    from rrnet_amd import ops
    n, lr = _size("block-plus-vector") + _size("partial-last-block"), 2.5e-4
    p, m, v, _ = _state(n, 33)
    m[:] = 0
    v[:] = 0
    a = [_dev(x) for x in (p, m, v)]
    b = [_dev(x) for x in (p, m, v)]
    ctl = _ctl_dev()
    for t in range(3):
        gd = _dev(G.gradient(n, 70 + t, scale=0.05))
        _norm_and_decide(gd, ctl, grad_scale=0.5, lr=lr)
        ops.adam_step_guarded(a[0], gd, a[1], a[2], None, 1e-8, ctl)
        ops.adam_step(b[0], gd, b[1], b[2], lr, 0.9, 0.999, 1e-8, t + 1, 0.5)
    c = ctl.cpu().numpy()
    assert c[G.IX["applied"]] == 3 and c[G.IX["clipped"]] == 0 and c[G.IX["scale"]] == 0.5
    for name, x, y in zip(("param", "exp_avg", "exp_avg_sq"), a, b):
        np.testing.assert_allclose(x.cpu().numpy(), y.cpu().numpy(), atol=ATOL, rtol=RTOL, err_msg=name)
    assert not np.array_equal(_bits(a[0]), p.view(np.uint32))


def test_argument_errors():
    from rrnet_amd import _C, ops
    g = torch.zeros(10, device="cuda")
    with pytest.raises(_C.RRNetHipError, match="multiple of 4"):
        ops.grad_norm(g)
    g = torch.zeros(8, device="cuda")
    partial, bad = ops.grad_norm(g)
    with pytest.raises(_C.RRNetHipError, match="partial"):
        ops.grad_norm(g, torch.zeros(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(_C.RRNetHipError, match="ctl"):
        ops.guard_decide(partial, bad, torch.zeros(16, dtype=torch.float64, device="cuda"))
    for kw, msg in ((dict(max_norm=0.0), "max_norm"), (dict(max_norm=float("nan")), "max_norm"), (dict(grad_scale=0.0), "grad_scale"),
                    (dict(beta1=1.0), "betas"), (dict(ema_decay=1.5), "ema_decay"), (dict(lr=float("inf")), "lr")):
        with pytest.raises(_C.RRNetHipError, match=msg):
            ops.guard_decide(partial, bad, _ctl_dev(), **kw)
    with pytest.raises(_C.RRNetHipError, match="exp_avg"):
        ops.adam_step_guarded(g, g, torch.zeros(4, device="cuda"), g, None, 1e-8, _ctl_dev())
    with pytest.raises(_C.RRNetHipError, match="float32"):
        ops.adam_step_guarded(g, g, g, g, g.double(), 1e-8, _ctl_dev())


# ---- model level ----------------------------------------------------------------------------------------------------
def _cfg():
    return SimpleNamespace(num_classes=10, Model=SimpleNamespace(num_stacks=1, backbone="hourglass_tiny",
                           nms_type_for_stage1="nms", nms_per_class_for_stage1=True))


def _model(seed=11):
    from rrnet_amd.models.centernet import CenterNet
    m = CenterNet(_cfg())
    m.load_state_dict(det_fill({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed))
    return m.cuda().to(memory_format=CL).train()


def _loss(model, x):
    hms, whs, regs = model(x)
    return (hms[0] ** 2).mean() + whs[0].abs().mean() + (regs[0] ** 2).mean()


def test_flat_adam_clip_and_ema_on_the_tiny_centernet():
    """FlatAdam(max_grad_norm, ema_decay) for 3 steps against torch.optim.Adam + clip_grad_norm_ + a per-tensor EMA on the
    CPU, fed the same gradients.  ema_state_dict has the model's keys, buffers are the live module's, and every conv weight
    equals the reference EMA in its LOGICAL layout (a wrong OHWI view would scramble it)."""
    from rrnet_amd.flat import FlatAdam
    m = _model()
    lr, max_norm, decay = 2.5e-4, 0.5, 0.9
    opt = FlatAdam(m, lr=lr, max_grad_norm=max_norm, ema_decay=decay)
    names = [k for k, _ in m.named_parameters()]
    ref_p = [p.detach().cpu().clone().requires_grad_() for p in m.parameters()]
    ref_ema = [p.detach().clone() for p in ref_p]
    ref_opt = torch.optim.Adam(ref_p, lr=lr)
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).cuda()
    norms = []
    for step in range(3):
        opt.zero_grad()
        _loss(m, x).backward()
        for rp, p in zip(ref_p, m.parameters()):
            rp.grad = p.grad.detach().cpu().clone()
        # the norm of these very gradients in float64 (clip_grad_norm_ below returns a float32 one, good to about 1e-5)
        norms.append(math.sqrt(sum(float((rp.grad.double() ** 2).sum()) for rp in ref_p)))
        torch.nn.utils.clip_grad_norm_(ref_p, max_norm)
        opt.step()
        ref_opt.step()
        d = min(decay, (2.0 + step) / (11.0 + step))
        for e, rp in zip(ref_ema, ref_p):
            e.mul_(d).add_(rp.detach() * (1.0 - d))
    stats = opt.guard_stats()
    print("norms", norms, "stats", stats)
    assert stats["applied"] == 3 and stats["skipped"] == 0 and opt.step_count == 3
    assert stats["clipped"] == sum(1 for v in norms if v > max_norm * (1 + 1e-4))
    assert all(abs(v - max_norm) > 1e-3 * max_norm for v in norms), "a norm at the bound: the count above is not decided"
    assert abs(stats["norm"] - norms[-1]) <= 1e-9 * norms[-1] and abs(stats["norm_max"] - max(norms)) <= 1e-9 * max(norms)
    for rp, p in zip(ref_p, m.parameters()):
        np.testing.assert_allclose(p.detach().cpu().numpy(), rp.detach().numpy(), atol=ATOL, rtol=RTOL)
    sd = opt.ema_state_dict(m)
    live = m.state_dict()
    assert list(sd) == list(live)
    convs = 0
    for k in sd:
        if k in names:
            want = ref_ema[names.index(k)]
            assert sd[k].shape == want.shape
            np.testing.assert_allclose(sd[k].cpu().numpy(), want.numpy(), atol=ATOL, rtol=RTOL, err_msg=k)
            convs += want.dim() == 4 and want.shape[1] > 1 and want.shape[2] > 1
        else:
            assert sd[k].data_ptr() == live[k].data_ptr(), k
    assert convs >= 3
    m2 = _model(seed=12)
    m2.load_state_dict({k: v.clone() for k, v in sd.items()})       # loadable as a checkpoint is


# ---- state files ----------------------------------------------------------------------------------------------------
def _small(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Conv2d(3, 8, 3), torch.nn.BatchNorm2d(8), torch.nn.Conv2d(8, 5, 1)).cuda()


def _synthetic_step(opt, t):
    opt.fp.grad.copy_(_dev(G.gradient(opt.fp.numel, 500 + t, scale=0.3)))
    opt.step()


def test_state_round_trip_with_ema_and_guard(tmp_path):
    """save_state / load_state with EMA and guard on: ema, ctl, the three buffers and the counters come back bit-equal, and
    one more step on identical synthetic gradients is bit-equal to the optimiser that was never interrupted."""
    from rrnet_amd import checkpoint as K
    from rrnet_amd.flat import FlatAdam
    kw = dict(lr=1e-3, max_grad_norm=2.0, skip_nonfinite=True, ema_decay=0.99)
    ma = _small(1)
    a = FlatAdam(ma, **kw)
    for t in range(3):
        _synthetic_step(a, t)
    a.fp.grad.fill_(float("nan"))
    a.step()                                           # a skipped step: step_count 4, applied 3
    w = K.StateWriter(ma, a, str(tmp_path))
    w.save_state(3)
    w.close()
    assert not w.warnings
    sd = torch.load(K.latest_state(str(tmp_path)), map_location="cpu", weights_only=False)
    assert sd["format"] == 1 and "ema" in sd and sd["guard"].dtype == torch.float64 and sd["digests"].shape[0] == 4
    mb = _small(2)
    b = FlatAdam(mb, **kw)
    assert K.load_state(K.latest_state(str(tmp_path)), mb, b) == 4
    assert b.step_count == a.step_count == 4
    ca, cb = a.ctl.cpu().numpy(), b.ctl.cpu().numpy()
    assert np.array_equal(ca.view(np.uint64), cb.view(np.uint64)) and ca[0] == 3 and ca[1] == 1
    for name in ("flat", "ema", "exp_avg", "exp_avg_sq"):
        xa, xb = (getattr(o.fp if name == "flat" else o, name) for o in (a, b))
        assert np.array_equal(_bits(xa), _bits(xb)), name
    assert not np.array_equal(_bits(a.ema), _bits(a.fp.flat))
    _synthetic_step(a, 9)
    _synthetic_step(b, 9)
    for name in ("flat", "ema", "exp_avg", "exp_avg_sq"):
        xa, xb = (getattr(o.fp if name == "flat" else o, name) for o in (a, b))
        assert np.array_equal(_bits(xa), _bits(xb)), name
    assert np.array_equal(a.ctl.cpu().numpy().view(np.uint64), b.ctl.cpu().numpy().view(np.uint64))
    assert a.guard_stats()["applied"] == 4


def test_state_without_guard_loads_into_a_guarded_optimiser(tmp_path, capsys):
    """A state taken with no option set (today's file) into FlatAdam with EMA and a guard: ema starts from the loaded
    weights with a warning, ctl is derived from step_count; the next step continues Adam's bias correction where the
    unguarded optimiser would.  And the other way round: the averaged weights of a file are ignored with a note."""
    from rrnet_amd import checkpoint as K
    from rrnet_amd.flat import FlatAdam
    ma = _small(1)
    a = FlatAdam(ma, lr=1e-3)
    for t in range(3):
        _synthetic_step(a, t)
    w = K.StateWriter(ma, a, str(tmp_path))
    w.save_state(2)
    w.close()
    path = K.latest_state(str(tmp_path))
    sd = torch.load(path, map_location="cpu", weights_only=False)
    assert "ema" not in sd and "guard" not in sd and sd["digests"].shape[0] == 3
    mb = _small(2)
    b = FlatAdam(mb, lr=1e-3, ema_decay=0.99, max_grad_norm=1e9)
    K.load_state(path, mb, b)
    assert "holds no averaged weights" in capsys.readouterr().out
    assert np.array_equal(_bits(b.ema), _bits(a.fp.flat))
    cb = b.ctl.cpu().numpy()
    assert np.array_equal(cb, K.guard_ctl_from_step_count(3, 0.9, 0.999)) and cb[0] == 3
    _synthetic_step(a, 9)
    _synthetic_step(b, 9)
    np.testing.assert_allclose(b.fp.flat.cpu().numpy(), a.fp.flat.cpu().numpy(), atol=ATOL, rtol=RTOL)
    # a file with averaged weights into an optimiser that keeps none
    w = K.StateWriter(mb, b, str(tmp_path / "ema"))
    w.save_state(3)
    w.close()
    mc = _small(3)
    c = FlatAdam(mc, lr=1e-3)
    K.load_state(K.latest_state(str(tmp_path / "ema")), mc, c)
    assert "they are not loaded" in capsys.readouterr().out and c.ema is None and c.step_count == 4
    assert np.array_equal(_bits(c.fp.flat), _bits(b.fp.flat))


def test_operator_report_line_and_ema_checkpoint(tmp_path):
    """BaseOperator.guard_report / save_ema_ckp on a small module: the print-interval suffix from one read of ctl, and
    `ckp-ema-N.pth` with the module's keys and the averaged weights; without a guard neither appears."""
    from rrnet_amd.flat import FlatAdam
    from rrnet_amd.operators.base_operator import BaseOperator
    m = _small(4)
    opt = FlatAdam(m, lr=1e-3, ema_decay=0.9, max_grad_norm=1e9)
    _synthetic_step(opt, 1)
    op = SimpleNamespace(optimizer=opt, model=SimpleNamespace(module=m))
    line = BaseOperator.guard_report(op)
    assert line.startswith("  gnorm ") and line.endswith(" clipped 0 skipped 0")
    assert float(line.split()[1]) == pytest.approx(opt.guard_stats()["norm"], rel=1e-3)
    BaseOperator.save_ema_ckp(op, 7, str(tmp_path))
    sd = torch.load(str(tmp_path / "ckp-ema-7.pth"), map_location="cpu")
    assert list(sd) == list(m.state_dict())
    views = opt.fp.views_of(opt.ema)
    for k, v in m.state_dict().items():
        want = views[k] if k in views else v
        assert torch.equal(sd[k], want.detach().cpu()), k
    assert not torch.equal(sd["0.weight"], m.state_dict()["0.weight"].cpu())
    plain = SimpleNamespace(optimizer=FlatAdam(_small(5), lr=1e-3), model=SimpleNamespace(module=m))
    assert BaseOperator.guard_report(plain) == ""
    BaseOperator.save_ema_ckp(plain, 8, str(tmp_path))
    assert sorted(p.name for p in tmp_path.iterdir()) == ["ckp-ema-7.pth"]
