// What csrc/conv.hip, conv_bf16.hip and conv16.hip do around a launch in the same way: the work a plan (conv_plan.h) asks for in
// front of and behind a forward-kernel launch, the geometry flip of the stride-1 data gradients, the sub-filter pack and class loop of the stride-2 ones.
#pragma once
#include "common.h"
#include "conv_plan.h"
#include "rrnet_hip.h"
#include "rrnet_hip_rows.h"

// BatchNorm-backward sums of the producer of the tensor a stride-1 data gradient writes (see csrc/conv.hip ConvArgs::bs_y)
struct BnSumArgs {
    const float *y, *z, *mean, *invstd, *msc, *msh;
    double *slab;      // [ceil(M/128)][2][C] scratch
    double *sums;      // [2][C], zeroed by the caller
    int relu_bias;     // producer = conv + bias + ReLU: masked store, sums[0..C) = bias gradient
    // what the _bnsum / _relubias entry points ask of their arguments (C, K of the data gradient)
    bool bn_ok(int c) const { return y && mean && invstd && slab && sums && (!msc == !msh) && c % 4 == 0 && c <= 1024; }
    bool relu_bias_ok(int c, int k) const { return z && slab && sums && c % 4 == 0 && k % 4 == 0 && c <= 1024; }
    template <typename A> void into(A &a) const       // a ConvArgs of either file, when the sums ride in the epilogue (FpropPlan::fused)
    {
        a.stat_slab = slab; a.bs_y = y; a.bs_z = z; a.bs_mean = mean; a.bs_invstd = invstd; a.bs_msc = msc; a.bs_msh = msh; a.bs_relu_bias = relu_bias;
    }
};

// One launch: above 48 KiB of dynamic LDS the kernel's limit is raised first (per device, so on every launch).
template <typename K, typename A>
inline int rr_launch(K kern, dim3 grid, int threads, size_t lds, hipStream_t stream, const A &args, const char *name)
{
    if (lds > 48 * 1024)
        RR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds), name);
    hipLaunchKernelGGL(kern, grid, dim3(threads), lds, stream, args);
    RR_CHECK_LAUNCH(name);
    return RR_OK;
}

// a gradient plan's refusal as the error of entry point `name` (the plan's text follows the name)
inline int rr_refuse(const char *name, const rr_plan::Refusal &r)
{
    char why[256];
    snprintf(why, sizeof(why), r.why, r.a[0], r.a[1], r.a[2], r.a[3], r.a[4]);
    rr_set_error("%s: %s", name, why);
    return RR_ERR_ARG;
}

inline int rr_conv_link(const BnSumArgs *bs) { return bs == nullptr ? rr_plan::LINK_NONE : (bs->relu_bias ? rr_plan::LINK_RELU_BIAS : rr_plan::LINK_BN); }

// column sums / sums of squares of y [M][C] -> slab row 0, rows zeroed by the caller (csrc/conv.hip: colstats_kernel)
int rr_conv_colstats(const float *y, long M, int C, double *slab, hipStream_t stream, const char *name);

// the sixteen GEMMs of the Winograd route (csrc/conv_wino.hip) on conv.hip's forward kernel: m[i][t][ko] = sum_c v[i][t][c] * u[i][ko][c]
int rr_conv_wino_gemm(const float *v, const float *u, float *m, long tiles, int c, int k, hipStream_t stream, const char *name);

// the sixteen GEMMs of its weight gradient on conv.hip's weight-gradient kernel: s[ko][i][c] += sum_t w[i][t][ko] * v[i][t][c]
int rr_conv_wino_wgrad_gemm(const float *v, const float *w, float *s, long tiles, int c, int k, hipStream_t stream, const char *name);

// zero fill on one side of the rows route's gate (csrc/conv_rows.hip): runs iff (*count <= max_rows) == (when_rows != 0)
int rr_gated_zero(float *p, size_t bytes, const int *count, int max_rows, int when_rows, hipStream_t stream, const char *name);

// in front of the launch: the split-K destination and (filled by rr_conv_colstats afterwards) the statistics slab, one zero-fill launch
inline int rr_conv_before_launch(const rr_plan::FpropPlan &pl, int n, int k, float *y, double *stat_slab, hipStream_t stream, const char *name)
{
    RR_CHECK_HIP(rr_zero2(pl.zero_dst ? y : nullptr, pl.zero_dst ? sizeof(float) * (size_t)pl.M * k : 0, pl.zero_slab ? stat_slab : nullptr,
                          pl.zero_slab ? rr_conv_stat_slab_bytes(n, pl.dh, pl.dw, k) : 0, stream), name);
    return RR_OK;
}

// behind it: the link's slab reduced, or its sums in a pass of their own where the epilogue could not carry them, or the column statistics
inline int rr_conv_after_launch(const rr_plan::FpropPlan &pl, const BnSumArgs *bs, int k, const float *y, double *stat_slab, hipStream_t stream,
                                const char *name)
{
    switch (pl.after) {
    case rr_plan::AFTER_REDUCE_SLAB: return rr_bn_reduce_slab(bs->slab, rr_cdiv(pl.M, rr_plan::BM), k, bs->sums, stream);
    case rr_plan::AFTER_BWD_REDUCE: return rr_bn_bwd_reduce(y, bs->z, bs->y, bs->mean, bs->invstd, bs->msc, bs->msh, bs->sums, pl.M, k, 1, stream);
    case rr_plan::AFTER_COLSTATS: return rr_conv_colstats(y, pl.M, k, stat_slab, stream, name);
    default: return RR_OK;
    }
}

// A stride-1 data gradient IS a forward convolution of dy [n,p,q,k] with the flipped, transposed filter, leading pads r-1-pad:
// the checks every such entry point makes, then the forward geometry.  producer_ok: what the entry point asks of its own arguments.
struct DgradS1Geom { int p, q, pad_h, pad_w; };
inline int rr_dgrad_s1_geom(const char *name, int h, int wd, int r, int s, int pad_h, int pad_w, bool producer_ok, DgradS1Geom *g)
{
    RR_CHECK_ARG(pad_h < r && pad_w < s && pad_h >= 0 && pad_w >= 0, "%s: pad must be in [0, kernel)", name);
    RR_CHECK_ARG(producer_ok, "%s: bad arguments (every tensor, with a producer its tensors and the two buffers; its C, a bias producer's K %% 4 == 0, C <= 1024)", name);
    *g = {h + 2 * pad_h - r + 1, wd + 2 * pad_w - s + 1, r - 1 - pad_h, s - 1 - pad_w};
    RR_CHECK_ARG(g->p > 0 && g->q > 0, "%s: empty dy", name);
    return RR_OK;
}

// The four sub-filters of a stride-2 data gradient (rr_plan::parity_classes), packed, flipped and transposed ([c][i'][j'][k],
// i' = Rc-1-i), class blocks in the order (0,0), (0,1), (1,0), (1,1), into k*r*s*c elements of caller scratch; T = float, or unsigned short for bf16.
template <typename T>
static __global__ __launch_bounds__(256) void rr_parity_pack_kernel(const float *w, T *wsub, int K, int C, int R, int S, int pad_h, int pad_w,
                                                                    long total)
{
    using namespace rr_plan;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const int k = (int)(idx % K);
        long rest = idx / K;
        const int tap = (int)(rest % (R * S));
        const int c = (int)(rest / (R * S));
        const int r = tap / S, s = tap - r * S;
        const int ph = (r - pad_h) & 1, pw = (s - pad_w) & 1;
        const int r0 = parity_first_tap(ph, pad_h), s0 = parity_first_tap(pw, pad_w);
        const int Rc = parity_span(R, r0), Sc = parity_span(S, s0);
        long base = 0;
        for (int cl = 0; cl < ph * 2 + pw; ++cl)
            base += (long)C * parity_extent(R, parity_first_tap(cl >> 1, pad_h)) * parity_extent(S, parity_first_tap(cl & 1, pad_w)) * K;
        const int ii = Rc - 1 - (r - r0) / 2, jj = Sc - 1 - (s - s0) / 2;
        if constexpr (sizeof(T) == 2) {
            const __bf16 v = (__bf16)w[((long)k * R * S + tap) * C + c];
            wsub[base + (((long)c * Rc + ii) * Sc + jj) * K + k] = __builtin_bit_cast(unsigned short, v);
        } else {
            wsub[base + (((long)c * Rc + ii) * Sc + jj) * K + k] = w[((long)k * R * S + tap) * C + c];
        }
    }
}

template <typename T>
inline int rr_parity_pack(const float *w, T *wsub, int k, int c, int r, int s, int pad_h, int pad_w, hipStream_t stream, const char *name)
{
    const long total = (long)k * c * r * s;
    hipLaunchKernelGGL(rr_parity_pack_kernel<T>, dim3((int)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256)), dim3(256), 0, stream, w, wsub,
                       k, c, r, s, pad_h, pad_w, total);
    RR_CHECK_LAUNCH(name);
    return RR_OK;
}

// A parity-class data gradient carried out (rr_plan::dgrad_s2_plan): the sub-filters packed, dx cleared where a class with
// pixels has no tap, then launch_class(ParityClass) -> error code for every class that launches.
template <typename T, typename F>
inline int rr_dgrad_s2_run(const rr_plan::DgradS2Plan &pl, const rr_plan::ConvGeom &g, const float *w, T *wsub, float *dx, hipStream_t stream,
                           const char *name, F launch_class)
{
    if (int rc = rr_parity_pack(w, wsub, g.k, g.c, g.r, g.s, g.pad_h, g.pad_w, stream, name)) return rc;
    if (pl.zero_dst) RR_CHECK_HIP(hipMemsetAsync(dx, 0, sizeof(float) * (size_t)g.n * g.h * g.w * g.c, stream), name);
    for (int i = 0; i < pl.n_launch; ++i)
        if (int rc = launch_class(pl.cls[i])) return rc;
    return RR_OK;
}
