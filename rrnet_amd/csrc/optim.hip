// The guarded optimiser step: gradient clipping, a skip on non-finite gradients and an exponential moving
// average of the weights, decided and applied on the device.  Three launches on one stream, no host read in between:
//
//   rr_grad_norm          one streaming read of the flat gradient -> per-block sum of squares (double) + count of NaN/Inf words
//   rr_guard_decide       one workgroup: adds the partials up, decides skip / clip, advances the control record `ctl`
//   rr_adam_step_guarded  adam_kernel's arithmetic (elementwise.hip) with its constants read from `ctl`; returns at once
//                         when told to skip; folds ema = ema * d + p_new * (1 - d) into the same pass
//
// Determinism: a float squared is exact in double (24 x 24 -> 48 bits), every thread adds its squares in index order,
// the wave is reduced by an xor butterfly (every lane ends with the same value), the four waves are added in order by
// one thread, and the decide kernel adds the partials the same way.  No atomics, no block reads what another wrote in the
// same launch, the grid is a function of n alone: two runs, and two ranks holding the same all-reduced buffer, reach the
// same bits.  tests/guard_cases.py restates this order in numpy, so the record can be compared exactly.
#include <math.h>

#include "common.h"
#include "rrnet_hip.h"

typedef unsigned int opt_u32x4 __attribute__((ext_vector_type(4)));

#define OPT_THREADS RR_GRAD_NORM_THREADS
#define OPT_WAVES (OPT_THREADS / 64)
#define OPT_UNROLL 2                   // deeper would put the unrolled path beyond 8 M words, out of a quick test's reach
#define OPT_MAX_BLOCKS 2048            // 256 CUs x 8 resident workgroups, as rr_state_snapshot

static_assert(OPT_THREADS == 256, "the reductions below are written for four waves");
static_assert(RR_GUARD_CTL_WORDS == 20, "ctl layout: include/rrnet_hip.h");

namespace {

// ctl slots (include/rrnet_hip.h)
enum { C_APPLIED = 0, C_SKIPPED, C_CLIPPED, C_B1POW, C_B2POW, C_NORM, C_NORM_MAX, C_BAD, C_SKIP, C_SCALE, C_STEP_SIZE,
       C_BC2_SQRT, C_EMA_D, C_EMA_OMD, C_RES0, C_RES1, C_B1, C_OMB1, C_B2, C_OMB2 };

__device__ __forceinline__ void norm_acc(opt_u32x4 u, double &acc, int &nbad)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const bool bad = (u[e] & 0x7f800000u) == 0x7f800000u;
        const double x = bad ? 0.0 : (double)__uint_as_float(u[e]);
        nbad += bad;
        acc += x * x;                       // exact product: contracted or not, the sum rounds once
    }
}

// block-wide sum in a fixed order; the result is valid in thread 0
__device__ __forceinline__ void block_sum(double &acc, long long &cnt, double *ps, long long *pc)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    acc = wave_sum_d(acc);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {      // 64-bit integer butterfly, moved as two 32-bit halves
        const unsigned lo = (unsigned)__shfl_xor((int)(cnt & 0xffffffffLL), o, 64);
        const unsigned hi = (unsigned)__shfl_xor((int)(cnt >> 32), o, 64);
        cnt += (long long)(((unsigned long long)hi << 32) | lo);
    }
    if (lane == 0) {
        ps[wave] = acc;
        pc[wave] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = 0.0;
        long long c = 0;
#pragma unroll
        for (int w = 0; w < OPT_WAVES; ++w) {
            t += ps[w];
            c += pc[w];
        }
        acc = t;
        cnt = c;
    }
}

__global__ __launch_bounds__(OPT_THREADS) void grad_norm_kernel(const opt_u32x4 *__restrict__ g, long n4,
                                                                 double *__restrict__ partial, int *__restrict__ bad)
{
    __shared__ double ps[OPT_WAVES];
    __shared__ long long pc[OPT_WAVES];
    const long stride = (long)gridDim.x * OPT_THREADS;
    double acc = 0.0;
    int nbad = 0;
    long i = (long)blockIdx.x * OPT_THREADS + threadIdx.x;
    for (; i + (OPT_UNROLL - 1) * stride < n4; i += OPT_UNROLL * stride) {      // two 16-byte loads in flight per lane
        opt_u32x4 u[OPT_UNROLL];
#pragma unroll
        for (int k = 0; k < OPT_UNROLL; ++k) u[k] = g[i + k * stride];
#pragma unroll
        for (int k = 0; k < OPT_UNROLL; ++k) norm_acc(u[k], acc, nbad);         // the order of the plain grid-stride loop
    }
    for (; i < n4; i += stride) norm_acc(g[i], acc, nbad);
    long long cnt = nbad;
    block_sum(acc, cnt, ps, pc);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = acc;
        bad[blockIdx.x] = (int)cnt;
    }
}

__global__ __launch_bounds__(OPT_THREADS) void guard_decide_kernel(const double *__restrict__ partial,
                                                                    const int *__restrict__ bad, int blocks, double grad_scale,
                                                                    double max_norm, int skip_nonfinite, double lr, double beta1,
                                                                    double beta2, double ema_decay, int ema_warmup, double *ctl)
{
#pragma clang fp contract(off)             // the host restatement rounds every operation: no fused multiply-adds here
    __shared__ double ps[OPT_WAVES];
    __shared__ long long pc[OPT_WAVES];
    double acc = 0.0;
    long long cnt = 0;
    for (int i = threadIdx.x; i < blocks; i += OPT_THREADS) {
        acc += partial[i];
        cnt += bad[i];
    }
    block_sum(acc, cnt, ps, pc);
    if (threadIdx.x != 0) return;
    const double inf = __builtin_huge_val();
    const double norm = cnt > 0 ? inf : sqrt(acc) * grad_scale;
    const bool finite = norm < inf && norm == norm;
    const bool skip = skip_nonfinite != 0 && (cnt > 0 || !finite);
    ctl[C_BAD] = (double)cnt;
    ctl[C_NORM] = norm;
    ctl[C_SKIP] = skip ? 1.0 : 0.0;
    if (skip) {
        ctl[C_SKIPPED] += 1.0;
        return;
    }
    double coef = 1.0;
    if (max_norm < inf && finite) {
        coef = max_norm / (norm + 1e-6);
        if (coef > 1.0) coef = 1.0;
    }
    if (coef < 1.0) ctl[C_CLIPPED] += 1.0;
    const double applied = ctl[C_APPLIED] + 1.0;
    const double b1p = ctl[C_B1POW] * beta1, b2p = ctl[C_B2POW] * beta2;
    ctl[C_APPLIED] = applied;
    ctl[C_B1POW] = b1p;
    ctl[C_B2POW] = b2p;
    ctl[C_SCALE] = (double)(float)(grad_scale * coef);
    ctl[C_STEP_SIZE] = (double)(float)(lr / (1.0 - b1p));
    ctl[C_BC2_SQRT] = (double)(float)sqrt(1.0 - b2p);
    double d = ema_decay;
    if (ema_warmup) {
        const double ramp = (1.0 + applied) / (10.0 + applied);
        if (ramp < d) d = ramp;
    }
    ctl[C_EMA_D] = (double)(float)d;
    ctl[C_EMA_OMD] = (double)(float)(1.0 - d);
    ctl[C_RES0] = 0.0;
    ctl[C_RES1] = 0.0;
    ctl[C_B1] = (double)(float)beta1;
    ctl[C_OMB1] = (double)(float)(1.0 - beta1);
    ctl[C_B2] = (double)(float)beta2;
    ctl[C_OMB2] = (double)(float)(1.0 - beta2);
    if (finite && norm > ctl[C_NORM_MAX]) ctl[C_NORM_MAX] = norm;
}

// adam_kernel of elementwise.hip, constants from ctl (values that are floats already: the conversions are exact)
template <bool EMA>
__global__ __launch_bounds__(OPT_THREADS) void adam_guarded_kernel(rr_f32x4 *__restrict__ p, const rr_f32x4 *__restrict__ g,
                                                                    rr_f32x4 *__restrict__ m, rr_f32x4 *__restrict__ v,
                                                                    rr_f32x4 *__restrict__ ema, long n4, float eps,
                                                                    const double *__restrict__ ctl)
{
    if (ctl[C_SKIP] != 0.0) return;
    const float grad_scale = (float)ctl[C_SCALE], step_size = (float)ctl[C_STEP_SIZE], bc2_sqrt = (float)ctl[C_BC2_SQRT];
    const float b1 = (float)ctl[C_B1], omb1 = (float)ctl[C_OMB1], b2 = (float)ctl[C_B2], omb2 = (float)ctl[C_OMB2];
    const float ema_d = (float)ctl[C_EMA_D], ema_omd = (float)ctl[C_EMA_OMD];
    for (long i = (long)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * OPT_THREADS) {
        const rr_f32x4 gg = g[i] * grad_scale;
        rr_f32x4 mm = m[i], vv = v[i], pp = p[i];
        rr_f32x4 ee;
        if (EMA) ee = ema[i];
        mm = mm * b1 + gg * omb1;
        vv = vv * b2 + gg * gg * omb2;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float denom = sqrtf(vv[e]) / bc2_sqrt + eps;
            pp[e] -= step_size * (mm[e] / denom);
        }
        m[i] = mm; v[i] = vv; p[i] = pp;
        if (EMA) ema[i] = ee * ema_d + pp * ema_omd;
    }
}

inline bool aligned16(const void *p) { return reinterpret_cast<size_t>(p) % 16 == 0; }
inline bool is_finite(double x) { return x == x && x < HUGE_VAL && x > -HUGE_VAL; }

}  // namespace

extern "C" int rr_grad_norm_blocks(long n)
{
    if (n <= 0) return 0;
    const long n4 = (n + 3) / 4;
    const long b = (n4 + OPT_THREADS - 1) / OPT_THREADS;
    return (int)(b > OPT_MAX_BLOCKS ? OPT_MAX_BLOCKS : b);
}

extern "C" int rr_grad_norm(const float *grad, long n, double *partial, int *bad, hipStream_t stream)
{
    RR_CHECK_ARG(n >= 0 && n % 4 == 0, "rr_grad_norm: n = %ld must be non-negative and a multiple of 4 (pad the flat buffer)", n);
    if (n == 0) return RR_OK;
    RR_CHECK_ARG(grad != nullptr && partial != nullptr && bad != nullptr, "rr_grad_norm: grad, partial or bad is NULL");
    RR_CHECK_ARG(aligned16(grad), "rr_grad_norm: grad must be 16-byte aligned");
    RR_CHECK_ARG(reinterpret_cast<size_t>(partial) % 8 == 0 && reinterpret_cast<size_t>(bad) % 4 == 0,
                 "rr_grad_norm: partial must be 8-byte and bad 4-byte aligned");
    hipLaunchKernelGGL(grad_norm_kernel, dim3(rr_grad_norm_blocks(n)), dim3(OPT_THREADS), 0, stream,
                       reinterpret_cast<const opt_u32x4 *>(grad), n / 4, partial, bad);
    RR_CHECK_LAUNCH("rr_grad_norm");
    return RR_OK;
}

extern "C" int rr_guard_decide(const double *partial, const int *bad, int blocks, double grad_scale, double max_norm,
                               int skip_nonfinite, double lr, double beta1, double beta2, double ema_decay, int ema_warmup,
                               double *ctl, hipStream_t stream)
{
    RR_CHECK_ARG(blocks >= 0 && blocks <= OPT_MAX_BLOCKS, "rr_guard_decide: blocks = %d outside [0, %d]", blocks, OPT_MAX_BLOCKS);
    RR_CHECK_ARG(blocks == 0 || (partial != nullptr && bad != nullptr), "rr_guard_decide: partial or bad is NULL");
    RR_CHECK_ARG(ctl != nullptr && reinterpret_cast<size_t>(ctl) % 8 == 0, "rr_guard_decide: ctl is NULL or not 8-byte aligned");
    RR_CHECK_ARG(is_finite(grad_scale) && grad_scale > 0.0, "rr_guard_decide: grad_scale = %g must be finite and positive", grad_scale);
    RR_CHECK_ARG(max_norm > 0.0, "rr_guard_decide: max_norm = %g must be positive (+inf: no clipping)", max_norm);
    RR_CHECK_ARG(is_finite(lr), "rr_guard_decide: lr = %g is not finite", lr);
    RR_CHECK_ARG(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, "rr_guard_decide: betas (%g, %g) outside [0, 1)",
                 beta1, beta2);
    RR_CHECK_ARG(ema_decay >= 0.0 && ema_decay <= 1.0, "rr_guard_decide: ema_decay = %g outside [0, 1]", ema_decay);
    hipLaunchKernelGGL(guard_decide_kernel, dim3(1), dim3(OPT_THREADS), 0, stream, partial, bad, blocks, grad_scale, max_norm,
                       skip_nonfinite, lr, beta1, beta2, ema_decay, ema_warmup, ctl);
    RR_CHECK_LAUNCH("rr_guard_decide");
    return RR_OK;
}

extern "C" int rr_adam_step_guarded(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *ema, long n,
                                    float eps, const double *ctl, hipStream_t stream)
{
    RR_CHECK_ARG(n >= 0 && n % 4 == 0, "rr_adam_step_guarded: n = %ld must be non-negative and a multiple of 4 (pad the flat buffer)", n);
    RR_CHECK_ARG(ctl != nullptr && reinterpret_cast<size_t>(ctl) % 8 == 0, "rr_adam_step_guarded: ctl is NULL or not 8-byte aligned");
    if (n == 0) return RR_OK;
    RR_CHECK_ARG(param != nullptr && grad != nullptr && exp_avg != nullptr && exp_avg_sq != nullptr,
                 "rr_adam_step_guarded: param, grad, exp_avg or exp_avg_sq is NULL");
    RR_CHECK_ARG(aligned16(param) && aligned16(grad) && aligned16(exp_avg) && aligned16(exp_avg_sq) && aligned16(ema),
                 "rr_adam_step_guarded: every buffer must be 16-byte aligned");
    const long n4 = n / 4;
    long blocks = (n4 + OPT_THREADS - 1) / OPT_THREADS;
    if (blocks > 4096) blocks = 4096;                   // the grid of rr_adam_step (ew_blocks)
    if (ema != nullptr)
        hipLaunchKernelGGL(adam_guarded_kernel<true>, dim3((int)blocks), dim3(OPT_THREADS), 0, stream, (rr_f32x4 *)param,
                           (const rr_f32x4 *)grad, (rr_f32x4 *)exp_avg, (rr_f32x4 *)exp_avg_sq, (rr_f32x4 *)ema, n4, eps, ctl);
    else
        hipLaunchKernelGGL(adam_guarded_kernel<false>, dim3((int)blocks), dim3(OPT_THREADS), 0, stream, (rr_f32x4 *)param,
                           (const rr_f32x4 *)grad, (rr_f32x4 *)exp_avg, (rr_f32x4 *)exp_avg_sq, (rr_f32x4 *)ema, n4, eps, ctl);
    RR_CHECK_LAUNCH("rr_adam_step_guarded");
    return RR_OK;
}
