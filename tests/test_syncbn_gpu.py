"""GPU: the SyncBN kernels that work with a sample count read from DEVICE memory (csrc/elementwise.hip:
rr_bn_reduce_slab_count, rr_bn_finalize_count, rr_bn_finalize / rr_bn_bwd_apply* with `count_dev`, rr_bn_affine_grad),
against training-mode BatchNorm over the CONCATENATED shards in float64 on the host (helpers.syncbn_ref64).

One process, no process group: W "virtual ranks" run the real per-rank launches on ragged shards, the test itself plays
the all-reduce (a torch sum of the ranks' float64 exchange buffers) and hands every rank the summed buffer.  A launch
that divided by the rank's own count instead of the exchanged one is invisible at world size 1 (tests/test_dp_gpu.py's
RR_DP_FORCE runs) and off by count_local / count_global here.

Bounds are derived from the arithmetic, never read off the kernels (u = 2^-24):
 - statistics: rr_conv_fprop's epilogue adds at most 64 values per thread in float32 before it goes to double
   (conv.hip: TM <= 4 fragments x 16 rows), so sum y carries <= 64 u sum|y| and sum y^2 <= 66 u sum y^2; these are
   propagated through mean, var, invstd (first derivative at the worst end of the interval) and the running statistics;
 - on top, every finalize output is a float32 rounding of float64 arithmetic: 2 u of the quantity (4 u per term of the
   two-term running updates), shift gets 3 u (|beta| + |mean * scale|) for its cancellation;
 - dx: the kernel evaluates gamma * invstd * (d - sdy - xhat * sdx) in float32 from float32 mean / invstd: <= 8
   roundings on each term's path, the backward sums carry rr_bn_bwd_reduce's float32 partials over 8 pixels (<= 12 u of
   the sums of magnitudes) and the rounded mean moves xhat by u |mean| invstd.  Normalised as tests/kernel_audit.py does
   (by max |gamma * invstd * d|) the bound must come out below the audit's 2e-5, which the test asserts;
 - bf16 images: 2^-8 of the same scale against float64, and EQUAL to the float32 result rounded to nearest even where
   both exist; g (the masked gradient) and the affine gradients are single float32 operations: compared exactly.
Each test prints its figures (pytest -s)."""
import numpy as np
import pytest
import torch

from helpers import U32, syncbn_ref64
from test_split_model_gpu import _Calls

pytestmark = pytest.mark.gpu
CL = torch.channels_last
EPS = 1e-5


def _dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t.contiguous(memory_format=CL) if t.dim() == 4 else t


def _h(t):
    return torch.as_tensor(t).detach().cpu().double()


def _ch(t):
    return t.view(1, -1, 1, 1)


# --------------------------------------------------------------------------------------------------------------------
# 1. forward: conv (statistics in the epilogue) -> slab reduction + count -> [sum over ranks] -> finalize
# --------------------------------------------------------------------------------------------------------------------
# shards: (images, H, W) of each rank's convolution OUTPUT; the BatchNorm input is [n, k, H, W]
FWD_CASES = {
    "roi-5+131": dict(shards=[(5, 3, 3), (131, 3, 3)], cin=16, k=64, r=1),          # one pixel tile / ten
    "backbone-1+3": dict(shards=[(1, 16, 16), (3, 16, 16)], cin=64, k=256, r=3),
    "three-ranks-1+2+4": dict(shards=[(1, 8, 8), (2, 8, 8), (4, 8, 8)], cin=16, k=128, r=3),
    "count-2": dict(shards=[(1, 1, 1), (1, 1, 1)], cin=8, k=4, r=1),                 # unbiased factor 2
    "many-tiles-k20": dict(shards=[(1, 96, 96), (2, 96, 96)], cin=8, k=20, r=3),     # 72 / 144 tiles: grid.y 2 / 3; 2C = 40
    "k1": dict(shards=[(1, 5, 7), (3, 5, 7)], cin=4, k=1, r=3),                      # 2C = 2, 6, 24: below / beside the
    "k3": dict(shards=[(1, 5, 7), (3, 5, 7)], cin=4, k=3, r=3),                      # reduction's 32-column blocks
    "k12": dict(shards=[(1, 5, 7), (3, 5, 7)], cin=4, k=12, r=3),
    "k200": dict(shards=[(2, 6, 6), (1, 6, 6)], cin=8, k=200, r=1),                  # finalize: 128 + 72 threads
}


def _fwd_inputs(seed, shards, cin, k, r):
    rng = np.random.default_rng(seed)
    xs = [_dev(rng.normal(0.3, 1.0, (n, cin, h, w)).astype(np.float32)) for n, h, w in shards]
    wt = _dev((rng.normal(0.0, 1.0, (k, cin, r, r)) * np.sqrt(2.0 / (cin * r * r))).astype(np.float32))
    gamma = _dev(rng.normal(1.0, 0.3, k).astype(np.float32))
    beta = _dev(rng.normal(0.0, 0.5, k).astype(np.float32))
    rm0 = rng.normal(0.0, 1.0, k).astype(np.float32)
    rv0 = rng.uniform(0.5, 2.0, k).astype(np.float32)
    return xs, wt, gamma, beta, rm0, rv0


def _fwd_bounds(ref, ys, gamma, beta, rm0, rv0, mom):
    """Per-channel bounds (float64 tensors) of mean, invstd, scale, shift, running_mean, running_var: see the module docstring."""
    n = ref["count"]
    c = gamma.numel()
    a1 = sum(_h(y).abs().sum((0, 2, 3)) for y in ys) / n
    m, var, istd, sc = ref["mean"], ref["var"], ref["invstd"], ref["scale"]
    g, b = _h(gamma).abs(), _h(beta).abs()
    em = 64 * U32 * a1
    ev = 66 * U32 * ref["sums"][c:] / n + 2 * m.abs() * em + em * em
    rel = ev / (var + EPS)
    assert float(rel.max()) < 0.5, float(rel.max())
    d_istd = istd * 0.5 * rel * (1.0 - rel) ** -1.5
    unb = var * n / (n - 1.0)
    return dict(mean=em + 2 * U32 * m.abs(),
                invstd=d_istd + 2 * U32 * istd,
                scale=g * (d_istd + 2 * U32 * istd) + 2 * U32 * sc.abs(),
                shift=3 * U32 * (b + (m * sc).abs()) + sc.abs() * em + m.abs() * g * d_istd,
                running_mean=4 * U32 * (((1 - mom) * _h(rm0)).abs() + (mom * m).abs()) + mom * em,
                running_var=4 * U32 * (((1 - mom) * _h(rv0)).abs() + mom * unb) + mom * ev * n / (n - 1.0))


def _check_fwd(tag, got, ref, bounds):
    worst = {}
    for name, bound in bounds.items():
        err = (_h(got[name]) - ref[name]).abs()
        worst[name] = (float(err.max()), float((err / bound).max()))
    print("%s: " % tag + ", ".join("%s %.2e (%.2f of bound)" % (k, v[0], v[1]) for k, v in worst.items()))
    for name, (e, ratio) in worst.items():
        assert ratio <= 1.0, (tag, name, e, ratio)


@pytest.mark.parametrize("case", sorted(FWD_CASES))
def test_forward_exchange_and_finalize_vs_fp64(case):
    """conv_fprop(want_stats) -> bn_reduce_slab(extra=1, count=) per rank -> sum of the ranks' buffers -> bn_finalize_sync on
    every rank, twice (momentum 0.1, then 0.37 on the updated running statistics)."""
    from rrnet_amd import ops
    cfg = FWD_CASES[case]
    k, shards = cfg["k"], cfg["shards"]
    xs, wt, gamma, beta, rm0, rv0 = _fwd_inputs(len(case) + k, **cfg)
    pad = (cfg["r"] // 2,) * 2
    ys, bufs, counts = [], [], []
    with _Calls() as calls:
        for x in xs:
            y, slab = ops.conv_fprop(x, wt, None, 1, pad, False, want_stats=True)
            counts.append(float(y.numel() // k))
            bufs.append(ops.bn_reduce_slab(slab, k, extra=1, count=counts[-1]))
            ys.append(y)
    assert calls.n.get("rr_bn_reduce_slab_count") == len(shards) and "rr_bn_reduce_slab" not in calls.n
    total = torch.stack(bufs).sum(0)                                    # the all-reduce
    n_glob = sum(counts)
    assert [tuple(y.shape) for y in ys] == [(n, k, h, w) for n, h, w in shards] and n_glob == sum(n * h * w for n, h, w in shards)
    for b, cnt in zip(bufs, counts):
        assert float(b[2 * k]) == cnt and b.numel() == 2 * k + 1        # the local count travels in the slot behind the sums
    assert float(total[2 * k]) == n_glob
    ref = syncbn_ref64(ys, gamma, beta, EPS)
    # the exchanged sums themselves: float32 partials in the convolution's epilogue, double from there on
    a1 = sum(_h(y).abs().sum((0, 2, 3)) for y in ys)
    e1 = float(((_h(total[:k]) - ref["sums"][:k]).abs() / (64 * U32 * a1)).max())
    e2 = float(((_h(total[k:2 * k]) - ref["sums"][k:]).abs() / (66 * U32 * ref["sums"][k:])).max())
    print("%s: exchanged sums, error over bound: sum y %.3f, sum y^2 %.3f (global count %d)" % (case, e1, e2, n_glob))
    assert e1 <= 1.0 and e2 <= 1.0
    per_rank = []
    for rank in range(len(shards)):
        rm, rv = _dev(rm0.copy()), _dev(rv0.copy())
        nbt = torch.tensor(7, dtype=torch.int64, device="cuda")
        buf = total.clone()
        with _Calls() as calls:
            mean, invstd, scale, shift, cnt = ops.bn_finalize_sync(buf[:2 * k], buf[2 * k:], gamma, beta, rm, rv, 0.1, EPS, nbt)
        assert calls.n == {"rr_bn_finalize_count": 1}
        first = dict(mean=mean.clone(), invstd=invstd.clone(), scale=scale.clone(), shift=shift.clone(),
                     running_mean=rm.clone(), running_var=rv.clone())
        assert cnt.dtype == torch.float64 and float(cnt) == n_glob and int(nbt) == 8
        assert cnt.data_ptr() != buf[2 * k:].data_ptr() and torch.equal(buf, total)          # storage of its own; buffer read only
        # the same statistics through rr_bn_finalize with a device count and a WRONG host count: the same kernel, the same bits
        rm_b, rv_b = _dev(rm0.copy()), _dev(rv0.copy())
        alt = ops.bn_finalize(buf[:2 * k], counts[rank], gamma, beta, rm_b, rv_b, 0.1, EPS, count_dev=buf[2 * k:])
        for a, b in zip(alt + (rm_b, rv_b), (mean, invstd, scale, shift, rm, rv)):
            assert torch.equal(a, b)
        # second step of the same layer: momentum 0.37 from the running statistics the first call left
        out2 = ops.bn_finalize_sync(buf[:2 * k], buf[2 * k:], gamma, beta, rm, rv, 0.37, EPS, nbt)
        assert int(nbt) == 9 and float(out2[4]) == n_glob
        second = dict(mean=out2[0], invstd=out2[1], scale=out2[2], shift=out2[3], running_mean=rm, running_var=rv)
        per_rank.append((first, second))
    for first, second in per_rank[1:]:          # every rank holds the same statistics, bit for bit
        for name in first:
            assert torch.equal(first[name], per_rank[0][0][name]) and torch.equal(second[name], per_rank[0][1][name]), name
    first, second = per_rank[0]
    r1 = syncbn_ref64(ys, gamma, beta, EPS, 0.1, rm0, rv0)
    _check_fwd(case + " momentum 0.1", first, r1, _fwd_bounds(r1, ys, gamma, beta, rm0, rv0, 0.1))
    r2 = syncbn_ref64(ys, gamma, beta, EPS, 0.37, first["running_mean"], first["running_var"])
    _check_fwd(case + " momentum 0.37", second, r2,
               _fwd_bounds(r2, ys, gamma, beta, first["running_mean"], first["running_var"], 0.37))
    if case == "count-2":
        assert n_glob == 2.0            # running_var moves by momentum * 2 * var


def test_packed_exchange_buffer_of_two_layers_vs_fp64():
    """The exchange as functional._ConvBnSyncMulti issues it: two layers on one input (3x3 stride 1 to 20 channels, 1x1
    stride 2 to 12: different k, different counts), rr_bn_reduce_slab_count writing into packed[off:off + 2k] with the
    count slots at packed[tot - L + i]; after the sum over ranks each layer is finalized from its slices.  A launch may
    write its own sums and its own count slot only: the rest of the buffer (the other layer's slices and slot, guard
    elements behind the buffer) holds sentinels that must survive."""
    from rrnet_amd import _C, ops
    rng = np.random.default_rng(11)
    shards = [(1, 16, 16), (3, 16, 16)]
    cin, layers = 8, [dict(k=20, r=3, stride=1), dict(k=12, r=1, stride=2)]
    xs = [_dev(rng.normal(0.3, 1.0, (n, cin, h, w)).astype(np.float32)) for n, h, w in shards]
    for ly in layers:
        ly["w"] = _dev((rng.normal(0.0, 1.0, (ly["k"], cin, ly["r"], ly["r"])) * 0.3).astype(np.float32))
        ly["gamma"] = _dev(rng.normal(1.0, 0.3, ly["k"]).astype(np.float32))
        ly["beta"] = _dev(rng.normal(0.0, 0.5, ly["k"]).astype(np.float32))
        ly["rm0"] = rng.normal(0.0, 1.0, ly["k"]).astype(np.float32)
        ly["rv0"] = rng.uniform(0.5, 2.0, ly["k"]).astype(np.float32)
        ly["ys"], ly["counts"] = [], []
    L, ks = len(layers), [ly["k"] for ly in layers]
    tot, guard = 2 * sum(ks) + L, 5
    offs = [0, 2 * ks[0]]
    packs = []
    for x in xs:
        store = torch.full((tot + guard,), -12345.0, dtype=torch.float64, device="cuda")
        packed = store[:tot]
        for i, ly in enumerate(layers):
            y, slab = ops.conv_fprop(x, ly["w"], None, ly["stride"], (ly["r"] // 2,) * 2, False, want_stats=True)
            k, off = ly["k"], offs[i]
            cnt = float(y.numel() // k)
            packed[off:off + 2 * k] = 0.0                  # a layer's own slice comes zeroed (the pool's pre-zeroed scratch)
            before = store.clone()
            _C.check(_C.fn("rr_bn_reduce_slab_count")(_C.ptr(slab), slab.numel() // (2 * k), k, _C.ptr(packed[off:off + 2 * k]), cnt,
                                                      _C.ptr(packed[tot - L + i:]), _C.stream()), "rr_bn_reduce_slab_count")
            own = torch.zeros(tot + guard, dtype=torch.bool, device="cuda")
            own[off:off + 2 * k] = True
            own[tot - L + i] = True
            assert torch.equal(store[~own], before[~own]), "layer %d wrote outside its slices" % i
            assert float(packed[tot - L + i]) == cnt
            ly["ys"].append(y)
            ly["counts"].append(cnt)
        packs.append(packed.clone())
    assert layers[0]["counts"] == [256.0, 768.0] and layers[1]["counts"] == [64.0, 192.0]
    total = torch.stack(packs).sum(0)
    for i, ly in enumerate(layers):
        k, off = ly["k"], offs[i]
        rm, rv = _dev(ly["rm0"].copy()), _dev(ly["rv0"].copy())
        nbt = torch.tensor(0, dtype=torch.int64, device="cuda")
        before = total.clone()
        mean, invstd, scale, shift, cnt = ops.bn_finalize_sync(total[off:off + 2 * k], total[tot - L + i:], ly["gamma"], ly["beta"],
                                                               rm, rv, 0.1, EPS, nbt)
        assert torch.equal(total, before) and int(nbt) == 1
        assert float(cnt) == sum(ly["counts"]) == float(total[tot - L + i])
        ref = syncbn_ref64(ly["ys"], ly["gamma"], ly["beta"], EPS, 0.1, ly["rm0"], ly["rv0"])
        got = dict(mean=mean, invstd=invstd, scale=scale, shift=shift, running_mean=rm, running_var=rv)
        _check_fwd("packed layer %d (k %d, global count %d)" % (i, k, int(cnt)), got, ref,
                   _fwd_bounds(ref, ly["ys"], ly["gamma"], ly["beta"], ly["rm0"], ly["rv0"], 0.1))


# --------------------------------------------------------------------------------------------------------------------
# 2. backward apply: every launch form of ops.bn_bwd_apply x the three mask modes, count read from the device
# --------------------------------------------------------------------------------------------------------------------
F32, BF16, F16X3 = 0, 1, 2
RAGGED_ROI = [(5, 3, 3), (131, 3, 3)]
# entry: which C entry point a shard of `px` pixels must take (the thresholds of rrnet_amd/ops.py: _SPLIT_MIN_PIXELS = 2048,
# _CONV16_MIN_PIXELS = 8192 — the shards sit on both sides of them)
BWD_FORMS = {
    "plain": dict(mode=F32, shards=RAGGED_ROI, c=64, entry=lambda px: "rr_bn_bwd_apply"),
    "plain-c12-three-ranks": dict(mode=F32, shards=[(1, 5, 7), (3, 5, 7), (2, 5, 7)], c=12, entry=lambda px: "rr_bn_bwd_apply"),
    "gacc": dict(mode=F32, shards=RAGGED_ROI, c=64, g_into=True, entry=lambda px: "rr_bn_bwd_apply_gacc"),
    "amax": dict(mode=F16X3, shards=[(1, 32, 32), (2, 32, 32), (3, 32, 32)], c=8,
                 entry=lambda px: "rr_bn_bwd_apply_amax" if px >= 2048 else "rr_bn_bwd_apply"),
    "b16": dict(mode=BF16, shards=[(1, 64, 64), (2, 64, 64)], c=128,
                entry=lambda px: "rr_bn_bwd_apply_b16" if px >= 8192 else "rr_bn_bwd_apply"),
    "b16-image-inputs-c12": dict(mode=BF16, shards=[(1, 5, 7), (3, 5, 7)], c=12, phantom=True, entry=lambda px: "rr_bn_bwd_apply_b16"),
    "b16-image-inputs-c128": dict(mode=BF16, shards=[(1, 64, 64), (2, 64, 64)], c=128, phantom=True,
                                  entry=lambda px: "rr_bn_bwd_apply_b16"),
    "b16-image-only-dx": dict(mode=BF16, shards=[(2, 9, 11), (5, 9, 11)], c=20, only16=True, entry=lambda px: "rr_bn_bwd_apply_b16"),
    # C / 4 = 96 does not divide the 256-thread workgroup.  64 pixels: 24 workgroups, a grid stride of 6144 quads = 64 x 96; 75 pixels:
    # 29 workgroups, 7424 quads, no multiple of 96 — in the bf16-image launches (the kernel that keeps a quad's constants in
    # registers when the stride allows) the two shards take one loop each
    "plain-c384": dict(mode=F32, shards=[(1, 8, 8), (3, 5, 5)], c=384, entry=lambda px: "rr_bn_bwd_apply"),
    "b16-image-inputs-c384": dict(mode=BF16, shards=[(1, 8, 8), (3, 5, 5)], c=384, phantom=True, entry=lambda px: "rr_bn_bwd_apply_b16"),
    # C = 1024, the launchers' upper limit: rr_bn_bwd_reduce_b16 runs ONE pixel lane per pass
    "b16-image-inputs-c1024": dict(mode=BF16, shards=[(1, 5, 7), (3, 5, 7)], c=1024, phantom=True, entry=lambda px: "rr_bn_bwd_apply_b16"),
}
APPLY_ENTRIES = ("rr_bn_bwd_apply", "rr_bn_bwd_apply_gacc", "rr_bn_bwd_apply_amax", "rr_bn_bwd_apply_b16")


def _bwd_inputs(seed, shards, c, mask, phantom):
    """Host float32 arrays per shard.  With `phantom` y and z hold bf16 values (the images ARE the data).  Mask mode
    "remask": dz is zeroed where y * mask_scale + mask_shift lies within float32 evaluation error of zero, so that the
    kernel's float32 mask and the reference's float64 mask cannot disagree on an element that counts."""
    rng = np.random.default_rng(seed)
    bf = (lambda a: torch.from_numpy(a).to(torch.bfloat16).float().numpy()) if phantom else (lambda a: a)
    ys = [bf(rng.normal(0.4, 1.3, (n, c, h, w)).astype(np.float32)) for n, h, w in shards]
    dzs = [(rng.normal(0.0, 1.0, y.shape) * 1e-2).astype(np.float32) for y in ys]
    gamma = rng.normal(1.0, 0.3, c).astype(np.float32)
    zs = msc = msh = masks = None
    if mask == "z":
        zs = [bf(np.where(rng.random(y.shape) < 0.1, 0.0, rng.normal(0.0, 1.0, y.shape)).astype(np.float32)) for y in ys]
        masks = [(z > 0).astype(np.float64) for z in zs]
    elif mask == "remask":
        msc = rng.normal(1.0, 0.3, c).astype(np.float32)
        msh = rng.normal(0.0, 0.5, c).astype(np.float32)
        masks = []
        for y, dz in zip(ys, dzs):
            a, b = y.astype(np.float64) * msc.astype(np.float64)[None, :, None, None], msh.astype(np.float64)[None, :, None, None]
            dz[np.abs(a + b) <= 1e-6 * (np.abs(a) + np.abs(b))] = 0.0
            masks.append((a + b > 0).astype(np.float64))
    return ys, dzs, gamma, zs, msc, msh, masks


def _dx_bound(ref, i, gamma, mean32, n_glob):
    """The derived bound of dx for shard i, normalised by max |gamma * invstd * d| (module docstring) -> (bound, scale)."""
    c = gamma.numel()
    a = _ch(ref["scale"].abs())
    d, xh = ref["d"][i].abs(), ref["xhat"][i].abs()
    sdy, sdx = _ch(ref["bwd_sums"][:c].abs() / n_glob), _ch(ref["bwd_sums"][c:].abs() / n_glob)
    m_d = _ch(sum(t.abs().sum((0, 2, 3)) for t in ref["d"]) / n_glob)
    m_dx = _ch(sum((t * x).abs().sum((0, 2, 3)) for t, x in zip(ref["d"], ref["xhat"])) / n_glob)
    terms = 8 * (d + sdy + xh * sdx) + 12 * (m_d + xh * m_dx) + 2 * _ch(_h(mean32).abs() * ref["invstd"]) * sdx
    scale = max(float((a * d).max()), 1e-30)
    return U32 * float((a * terms).max()) / scale, scale


@pytest.mark.parametrize("mask", ["z", "remask", "none"])
@pytest.mark.parametrize("form", sorted(BWD_FORMS))
def test_bwd_apply_divides_by_the_device_count(form, mask):
    """Ragged shards; rr_bn_bwd_reduce gives each rank's sums, the test adds them.  (a) count_dev = the global count with the
    rank's LOCAL count as the host argument must give the float64 dx (and g) of the concatenated batch; (b) count_dev =
    None with the global count on the host must give the same bits.  want_g (a residual branch) rides on the "z" mode,
    g_into on the gacc form."""
    from rrnet_amd import ops
    cfg = BWD_FORMS[form]
    c, shards, phantom, only16 = cfg["c"], cfg["shards"], cfg.get("phantom", False), cfg.get("only16", False)
    ys, dzs, gamma, zs, msc, msh, masks = _bwd_inputs(sum(map(ord, form + mask)), shards, c, mask, phantom)
    ref = syncbn_ref64(ys, gamma, np.zeros(c, np.float32), EPS, dzs=dzs, masks=masks)
    n_glob = ref["count"]
    mean, invstd, gam = _dev(ref["mean"].float().numpy()), _dev(ref["invstd"].float().numpy()), _dev(gamma)
    mscd, mshd = (_dev(msc), _dev(msh)) if msc is not None else (None, None)
    want_g = mask == "z" or cfg.get("g_into", False)
    count_dev = torch.tensor([n_glob], dtype=torch.float64, device="cuda")

    def operand(a):
        t = _dev(a)
        if not phantom:
            return t
        img = t.to(torch.bfloat16)
        assert img.stride() == t.stride() and torch.equal(img.float(), t)
        return ops.phantom_f32(tuple(t.shape), t.device, img)

    with ops.bf16_scope(cfg["mode"], force=True), _Calls() as calls:
        dev = [(_dev(dz), operand(z) if zs is not None else None, operand(y)) for dz, y, z in zip(dzs, ys, zs or [None] * len(ys))]
        local = [ops.bn_bwd_reduce(dz, z, y, mean, invstd, mask_scale=mscd, mask_shift=mshd) for dz, z, y in dev]
        total = torch.stack(local).sum(0)                               # the all-reduce
        assert calls.n.get("rr_bn_bwd_reduce_b16" if phantom else "rr_bn_bwd_reduce") == len(shards)
        for i, s in enumerate(local):        # each rank's own sums: its dbeta | dgamma
            lb = ref["local_bwd"][i]
            b1 = 9 * U32 * ref["d"][i].abs().sum((0, 2, 3))
            b2 = 12 * U32 * (ref["d"][i] * ref["xhat"][i]).abs().sum((0, 2, 3)) + \
                2 * U32 * _h(mean).abs() * ref["invstd"] * ref["d"][i].abs().sum((0, 2, 3))
            e1, e2 = float(((_h(s[:c]) - lb[:c]).abs() / b1.clamp_min(1e-300)).max()), float(((_h(s[c:2 * c]) - lb[c:]).abs() / b2.clamp_min(1e-300)).max())
            assert e1 <= 1.0 and e2 <= 1.0, (form, mask, i, e1, e2)
        expect = {}
        for i, (n, h, w) in enumerate(shards):
            dz, z, y = dev[i]
            n_loc = float(n * h * w)
            assert n_loc != n_glob
            base = _dev(np.random.default_rng(i).normal(0.0, 1e-2, ys[i].shape).astype(np.float32)) if cfg.get("g_into") else None
            ga, gb = (base.clone(), base.clone()) if base is not None else (None, None)
            name = cfg["entry"](n * h * w)
            expect[name] = expect.get(name, 0) + 2
            dxa, g_a = ops.bn_bwd_apply(dz, z, y, mean, invstd, gam, total, n_loc, want_g and ga is None, None, None, count_dev,
                                        mscd, mshd, g_into=ga, bf16_only=only16)
            dxb, g_b = ops.bn_bwd_apply(dz, z, y, mean, invstd, gam, total, n_glob, want_g and gb is None, None, None, None,
                                        mscd, mshd, g_into=gb, bf16_only=only16)
            bound, scale = _dx_bound(ref, i, gam, mean, n_glob)
            assert bound <= 2e-5, bound                                  # no looser than the audit
            img_a, img_b = (ops.image_of(dxa), ops.image_of(dxb)) if ops.is_phantom(dxa) else (ops.b16_carry(dxa), ops.b16_carry(dxb))
            assert ops.is_phantom(dxa) == ops.is_phantom(dxb) == only16 and (img_a is None) == (img_b is None)
            assert (img_a is not None) == (only16 or name == "rr_bn_bwd_apply_b16" and c % 128 == 0 and n * h * w >= 8192)
            fig = []
            if not only16:
                assert torch.equal(dxa, dxb), "count_dev and the host count disagree"
                err = float((_h(dxa) - ref["dx"][i]).abs().max()) / scale
                fig.append("dx %.2e (bound %.2e)" % (err, bound))
                assert err <= bound, (form, mask, i, err, bound)
            if img_a is not None:
                assert torch.equal(img_a, img_b)
                e16 = float((_h(img_a) - ref["dx"][i]).abs().max()) / scale
                fig.append("bf16 image %.2e (bound %.2e)" % (e16, 2.0 ** -8))
                assert e16 <= 2.0 ** -8
                if not only16:
                    assert torch.equal(img_a, dxa.to(torch.bfloat16)), "image is not the fp32 dx rounded to nearest even"
            if want_g:
                d32 = dz * _dev(masks[i].astype(np.float32)) if masks is not None else dz
                assert g_a is not None and torch.equal(g_a, g_b)
                assert torch.equal(g_a, d32 if base is None else base + d32)       # one float32 operation: exact
                if base is not None:
                    assert g_a.data_ptr() == ga.data_ptr()
            else:
                assert g_a is None and g_b is None
            if name == "rr_bn_bwd_apply_amax":
                for dx in (dxa, dxb):
                    word = ops.amax_carry(dx).view(torch.float32)[0]
                    assert float(word) == float(dx.abs().max()), (float(word), float(dx.abs().max()))
                fig.append("published max|dx| %.6e" % float(dxa.abs().max()))
            print("%s / %s, shard %d of %s (local count %d, global %d) via %s: %s" % (form, mask, i, shards, n_loc, n_glob, name, ", ".join(fig)))
        assert {k: v for k, v in calls.n.items() if k in APPLY_ENTRIES} == expect, (calls.n, expect)


# --------------------------------------------------------------------------------------------------------------------
# 3. rr_bn_affine_grad: dbeta += sums[:C], dgamma += sums[C:2C] from a slice of a larger buffer
# --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [12, 200])           # below one 128-thread block; one full block + 72 threads
def test_affine_grad_accumulates_from_an_offset_slice(c):
    from rrnet_amd import ops
    rng = np.random.default_rng(c)
    off, guard = 7, 9
    big = torch.from_numpy(rng.normal(0.0, 3.0, off + 2 * c + 5)).cuda()
    sums = big[off:off + 2 * c]
    store = torch.from_numpy(rng.normal(0.0, 1.0, (2, c + guard)).astype(np.float32)).cuda()
    dgamma, dbeta = store[0, :c], store[1, :c]
    start, big0 = store.clone(), big.clone()
    s32 = sums.float()                                        # (float) of a double: round to nearest even, as the kernel converts
    exp_b, exp_g = start[1, :c].clone(), start[0, :c].clone()
    for call in (1, 2):
        with _Calls() as calls:
            ops.bn_affine_grad(sums, dgamma, dbeta)
        assert calls.n == {"rr_bn_affine_grad": 1}
        exp_b, exp_g = exp_b + s32[:c], exp_g + s32[c:]
        assert torch.equal(dbeta, exp_b) and torch.equal(dgamma, exp_g), "call %d" % call
        assert torch.equal(store[:, c:], start[:, c:]) and torch.equal(big, big0)             # guards and the sums untouched
        r_b, r_g = _h(start[1, :c]) + call * _h(sums[:c]), _h(start[0, :c]) + call * _h(sums[c:])
        e = max(float(((_h(dbeta) - r_b).abs() / (2 * call * U32 * (_h(start[1, :c]).abs() + call * _h(sums[:c]).abs()))).max()),
                float(((_h(dgamma) - r_g).abs() / (2 * call * U32 * (_h(start[0, :c]).abs() + call * _h(sums[c:]).abs()))).max()))
        print("affine grad C=%d call %d: error over the %d u bound vs fp64: %.3f" % (c, call, 2 * call, e))
        assert e <= 1.0
    assert not torch.equal(s32[:c], s32[c:])                  # dbeta and dgamma receive different halves
