// Weighted boxes fusion (Solovyev, Wang, Gabruseva 2021) of score-sorted (frame, class) segments for gfx950.  The contract —
// the float32 IoU, the choice of the cluster, the double sums — stands in include/rrnet_hip.h; tests/wbf_cases.py restates it.
//
// One workgroup per segment.  Cluster c belongs to thread c % T for the whole run: that thread alone reads its fused box in the
// scan of every step, and that thread alone rewrites it when the cluster wins (or is opened).  So a step needs no ordering
// between threads except the arg-max itself:
//   1. every lane scans its clusters against the step's row (float32 IoU; the row's five values sit at a uniform address and the
//      next row is fetched before the reduction), keeping (IoU bits, ~index) — IoU >= 0, so its bits order like the value;
//   2. a DPP wave maximum of the IoU, and, where more than one lane holds it, a second one over ~index (lowest index wins);
//   3. with more than one wave, one LDS exchange behind ONE barrier (double-buffered slots, as in softnms.hip);
//   4. every lane knows the winner; its owner adds the row to the double sums and rewrites the fused box, or the owner of the
//      next free index opens a cluster.  The cluster count lives redundantly in every lane.
// A segment of at most 64 rows cannot open more than 64 clusters: it runs on the first wave alone, one lane per cluster, with
// no barrier at all.  At the end every lane writes its own clusters.  No atomics; nothing waits on another workgroup.
// Which launches a call gets is wbf_plan.h's decision.  Compiled with -ffp-contract=off.
//
// Latency-bound: the step is a chain of one LDS read, ~15 float operations with one IEEE division, the wave reduction, the
// exchange, and — on a join — the owner's four double divisions.  tools/bench_wbf.py quotes its time per row beside Soft-NMS.
#include "common.h"
#include "rrnet_hip.h"
#include "wbf_plan.h"

namespace {

// the wave maximum of softnms.hip: row_shr 1, 2, 4, 8 inside the 16-lane rows, row_bcast 15 / 31 across them; lane 63 ends
// with the maximum.  Lanes without a source keep their own value; max is idempotent, so no bank masks are needed.
__device__ __forceinline__ unsigned dpp_max_u32(unsigned v)
{
    unsigned o;
#define RR_DPP_STEP(ctrl, rmask)                                                  \
    o = (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, ctrl, rmask, 0xf, false); \
    v = o > v ? o : v;
    RR_DPP_STEP(0x111, 0xf) RR_DPP_STEP(0x112, 0xf) RR_DPP_STEP(0x114, 0xf) RR_DPP_STEP(0x118, 0xf)
    RR_DPP_STEP(0x142, 0xa) RR_DPP_STEP(0x143, 0xc)
#undef RR_DPP_STEP
    return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}

// a segment's clusters: the fused boxes (LDS, SoA) and the running sums (LDS, or the workgroup's slice of the workspace)
struct Clusters {
    float *x1, *y1, *x2, *y2;
    double *ax1, *ay1, *ax2, *ay2, *S;
    int *cnt;
    float *mx, *cls;
};

template <int T>
__device__ __forceinline__ void wbf_segment(const float *__restrict__ rows, const int n, const float thr, const int conf_type,
                                            const double wsum, const Clusters c, unsigned *slots /* [2][16][2] */,
                                            float *__restrict__ out6, int *__restrict__ members, int *__restrict__ n_out)
{
    constexpr int W = T / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int nc = 0, xbuf = 0;
    float rx1 = 0.f, ry1 = 0.f, rx2 = 0.f, ry2 = 0.f, rs = 0.f, rc = 0.f;
    if (n > 0) { rx1 = rows[0]; ry1 = rows[1]; rx2 = rows[2]; ry2 = rows[3]; rs = rows[4]; rc = rows[5]; }
    for (int j = 0; j < n; ++j) {
        // ---- the next row, ahead of the reduction (the last step reads its own row again)
        const float *nr = rows + (size_t)(j + 1 < n ? j + 1 : j) * 6;
        const float qx1 = nr[0], qy1 = nr[1], qx2 = nr[2], qy2 = nr[3], qs = nr[4], qc = nr[5];
        // ---- 1. my clusters against the row
        const float rarea = (rx2 - rx1) * (ry2 - ry1);
        unsigned key = 0u, ikey = 0u;              // ikey 0: no candidate (~index of a cluster is never 0)
        for (int k = tid; k < nc; k += T) {
            const float fx1 = c.x1[k], fy1 = c.y1[k], fx2 = c.x2[k], fy2 = c.y2[k];
            const float iw = __builtin_fminf(fx2, rx2) - __builtin_fmaxf(fx1, rx1);
            const float ih = __builtin_fminf(fy2, ry2) - __builtin_fmaxf(fy1, ry1);
            float iou = 0.0f;
            if (iw > 0.0f && ih > 0.0f) {
                const float inter = iw * ih;
                const float u = ((fx2 - fx1) * (fy2 - fy1) + rarea) - inter;
                iou = u > 0.0f ? inter / u : 0.0f;
            }
            const unsigned kb = __float_as_uint(iou);
            if (kb > key || ikey == 0u) {          // k ascends: strict `>` keeps the lowest index among equals
                key = kb;
                ikey = ~(unsigned)k;
            }
        }
        // ---- 2. wave maximum, the lowest index among equal maxima
        unsigned ms = dpp_max_u32(key), mi;
        {
            const unsigned long long tie = __ballot(key == ms && ikey != 0u);
            if (__popcll(tie) > 1) mi = dpp_max_u32(key == ms ? ikey : 0u);
            else if (tie != 0ull) mi = (unsigned)__builtin_amdgcn_readlane((int)ikey, __ffsll((long long)tie) - 1);
            else mi = 0u;
        }
        // ---- 3. across the waves
        if (W > 1) {
            typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
            u32x2 *sl = reinterpret_cast<u32x2 *>(slots) + xbuf * 16;
            if (lane == 0) sl[wave] = u32x2{ms, mi};
            __syncthreads();
            xbuf ^= 1;                             // the other set of slots next time: no second barrier per step
            u32x2 h[W];
#pragma unroll
            for (int w = 0; w < W; ++w) h[w] = sl[w];
            ms = h[0][0];
            mi = h[0][1];
#pragma unroll
            for (int w = 1; w < W; ++w) {
                const bool better = h[w][1] != 0u && (mi == 0u || h[w][0] > ms || (h[w][0] == ms && h[w][1] > mi));
                ms = better ? h[w][0] : ms;
                mi = better ? h[w][1] : mi;
            }
        }
        // ---- 4. join the winner or open a cluster; the owner lane alone touches the cluster
        const bool join = mi != 0u && __uint_as_float(ms) > thr;
        const int k = join ? (int)~mi : nc;
        if (tid == (k & (T - 1))) {
            const double s = (double)rs;
            if (join) {
                const double a1 = c.ax1[k] + s * (double)rx1, b1 = c.ay1[k] + s * (double)ry1;
                const double a2 = c.ax2[k] + s * (double)rx2, b2 = c.ay2[k] + s * (double)ry2;
                const double S = c.S[k] + s;
                c.ax1[k] = a1; c.ay1[k] = b1; c.ax2[k] = a2; c.ay2[k] = b2; c.S[k] = S;
                c.cnt[k] += 1;
                const float m = c.mx[k];
                c.mx[k] = m >= rs ? m : rs;
                c.x1[k] = (float)(a1 / S); c.y1[k] = (float)(b1 / S); c.x2[k] = (float)(a2 / S); c.y2[k] = (float)(b2 / S);
            } else {
                c.x1[k] = rx1; c.y1[k] = ry1; c.x2[k] = rx2; c.y2[k] = ry2;
                c.ax1[k] = s * (double)rx1; c.ay1[k] = s * (double)ry1; c.ax2[k] = s * (double)rx2; c.ay2[k] = s * (double)ry2;
                c.S[k] = s;
                c.cnt[k] = 1;
                c.mx[k] = rs;
                c.cls[k] = rc;
            }
        }
        nc += join ? 0 : 1;
        rx1 = qx1; ry1 = qy1; rx2 = qx2; ry2 = qy2; rs = qs; rc = qc;
    }
    // ---- every lane writes its own clusters
    for (int k = tid; k < nc; k += T) {
        const int cnt = c.cnt[k];
        const double base = conf_type == 1 ? (double)c.mx[k] : c.S[k] / (double)cnt;
        const double m = (double)cnt < wsum ? (double)cnt : wsum;
        float *o = out6 + (size_t)k * 6;
        o[0] = c.x1[k]; o[1] = c.y1[k]; o[2] = c.x2[k]; o[3] = c.y2[k];
        o[4] = (float)(base * m / wsum);
        o[5] = c.cls[k];
        if (members) members[k] = cnt;
    }
    if (tid == 0) *n_out = nc;
}

// dynamic LDS: the fused boxes, and for WS == false the running sums behind them (sums first: they are doubles)
template <int T, bool WS>
__global__ __launch_bounds__(T) void wbf_kernel(const float *__restrict__ rows6, const int *__restrict__ seg_off,
                                                const int *__restrict__ seg_len, const int nseg, const float thr,
                                                const int conf_type, const double wsum, float *__restrict__ out6,
                                                int *__restrict__ members, int *__restrict__ n_out, unsigned char *workspace,
                                                const int cap, const int n_lo, const int n_hi)
{
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ __align__(8) unsigned slots[2 * 16 * 2];
    Clusters c;
    unsigned char *sums = WS ? workspace + (size_t)blockIdx.x * cap * rr_plan::WBF_CLUSTER_WS_BYTES : smem;
    c.ax1 = reinterpret_cast<double *>(sums);
    c.ay1 = c.ax1 + cap; c.ax2 = c.ax1 + 2 * cap; c.ay2 = c.ax1 + 3 * cap; c.S = c.ax1 + 4 * cap;
    c.cnt = reinterpret_cast<int *>(c.ax1 + 5 * cap);
    c.mx = reinterpret_cast<float *>(c.cnt + cap);
    c.cls = c.mx + cap;
    c.x1 = WS ? reinterpret_cast<float *>(smem) : c.cls + cap;
    c.y1 = c.x1 + cap; c.x2 = c.x1 + 2 * cap; c.y2 = c.x1 + 3 * cap;
    // (WS: the workgroup walks segments blockIdx.x, + gridDim.x, ...; otherwise gridDim.x == nseg and this loop runs once)
    for (int seg = blockIdx.x; seg < nseg; seg += gridDim.x) {
        const int off = seg_off[seg];
        const int n = seg_len ? seg_len[seg] : seg_off[seg + 1] - off;
        if (n <= n_lo || n > n_hi || n > cap) {    // another launch's segment (n > cap: beyond the caller's bound, not taken)
            if (n > cap && n <= n_hi && threadIdx.x == 0) n_out[seg] = 0;
            continue;
        }
        const float *rows = rows6 + (size_t)off * 6;
        float *o = out6 + (size_t)off * 6;
        int *mem = members ? members + off : nullptr;
        if (!WS && T > 64 && n <= rr_plan::WBF_ONE_WAVE) {
            if (threadIdx.x < 64) wbf_segment<64>(rows, n, thr, conf_type, wsum, c, slots, o, mem, &n_out[seg]);
            return;                                // (never in the walking launch: its segments are long)
        }
        wbf_segment<T>(rows, n, thr, conf_type, wsum, c, slots, o, mem, &n_out[seg]);
        if (WS) __syncthreads();                   // the slots and the parity start over with the next segment
    }
}

template <int T, bool WS>
int launch_wbf(const rr_plan::WbfLaunch &l, const float *rows6, const int *seg_off, const int *seg_len, int nseg, float thr,
               int conf_type, double wsum, float *out6, int *members, int *n_out, void *workspace, hipStream_t stream)
{
    if (l.raise_lds_limit)
        RR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(wbf_kernel<T, WS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                         l.lds), "rr_wbf_segments");
    const int grid = l.grid > 0 && l.grid < nseg ? l.grid : nseg;
    hipLaunchKernelGGL((wbf_kernel<T, WS>), dim3(grid), dim3(T), (size_t)l.lds, stream, rows6, seg_off, seg_len, nseg, thr, conf_type,
                       wsum, out6, members, n_out, static_cast<unsigned char *>(workspace), l.cap, l.lo, l.hi);
    return RR_OK;
}

}  // namespace

extern "C" size_t rr_wbf_workspace_bytes(int nseg, int max_seg_boxes)
{
    const rr_plan::WbfPlan p = rr_plan::wbf_plan(nseg, max_seg_boxes);
    return p.refuse == nullptr && p.use_workspace ? (size_t)p.workspace_bytes : 0;
}

// the plan of wbf_plan.h as rr_wbf_segments asks it, with the kernel's per-segment constants, for the tests
extern "C" int rr_wbf_plan(int nseg, int max_seg_boxes, int *out, int n_out)
{
    using namespace rr_plan;
    RR_CHECK_ARG(out != nullptr && n_out >= RR_WBF_PLAN_INTS, "rr_wbf_plan: bad arguments");
    const WbfPlan p = wbf_plan(nseg, max_seg_boxes);
    RR_CHECK_ARG(p.refuse == nullptr, p.refuse, p.a0);
    for (int i = 0; i < RR_WBF_PLAN_INTS; ++i) out[i] = 0;
    out[0] = p.launches; out[1] = p.use_workspace;
    out[2] = WBF_ONE_WAVE; out[3] = WBF_SHORT; out[4] = WBF_LDS_MAX; out[5] = WBF_MAX_SEG; out[6] = WBF_WS_GRID;
    for (int i = 0; i < p.launches; ++i) {
        const WbfLaunch &l = p.launch[i];
        const int v[7] = {l.T, l.lds, l.cap, l.lo, l.hi, l.ws, l.grid};
        for (int q = 0; q < 7; ++q) out[8 + 7 * i + q] = v[q];
    }
    return RR_OK;
}

extern "C" int rr_wbf_segments(const float *rows6, const int *seg_off, const int *seg_len, int nseg, int max_seg_boxes,
                               float iou_thr, int conf_type, double weight_sum, float *out6, int *members, int *n_out,
                               void *workspace, size_t workspace_bytes, hipStream_t stream)
{
    using namespace rr_plan;
    const WbfPlan p = wbf_plan(nseg, max_seg_boxes);
    RR_CHECK_ARG(p.refuse == nullptr, p.refuse, p.a0);
    if (p.launches == 0) return RR_OK;         // an empty batch
    RR_CHECK_ARG(rows6 != nullptr && seg_off != nullptr && out6 != nullptr && n_out != nullptr, "rr_wbf_segments: null pointer");
    RR_CHECK_ARG(static_cast<const void *>(rows6) != static_cast<const void *>(out6), "rr_wbf_segments: out6 may not alias rows6");
    RR_CHECK_ARG(conf_type == 0 || conf_type == 1, "rr_wbf_segments: conf_type %d (0 avg, 1 max)", conf_type);
    RR_CHECK_ARG(weight_sum > 0.0 && weight_sum < 1e300, "rr_wbf_segments: weight_sum %g must be positive and finite", weight_sum);
    RR_CHECK_ARG(iou_thr == iou_thr, "rr_wbf_segments: iou_thr is NaN");
    RR_CHECK_ARG(!p.use_workspace || (workspace != nullptr && workspace_bytes >= (size_t)p.workspace_bytes),
                 "rr_wbf_segments: workspace of %ld bytes required for %d-row segments", p.workspace_bytes, max_seg_boxes);
    for (int i = 0; i < p.launches; ++i) {
        const WbfLaunch &l = p.launch[i];
        int rc;
#define RR_WBF_GO(T, WS) rc = launch_wbf<T, WS>(l, rows6, seg_off, seg_len, nseg, iou_thr, conf_type, weight_sum, out6, members, n_out, \
                                                workspace, stream)
        if (l.T == 64 && !l.ws) RR_WBF_GO(64, false);
        else if (l.T == 256 && !l.ws) RR_WBF_GO(256, false);
        else if (l.T == 512 && !l.ws) RR_WBF_GO(512, false);
        else if (l.T == 512 && l.ws) RR_WBF_GO(512, true);
        else RR_CHECK_ARG(false, "rr_wbf_segments: no kernel <%d, %d>", l.T, (int)l.ws);
#undef RR_WBF_GO
        if (rc != RR_OK) return rc;
        RR_CHECK_LAUNCH("rr_wbf_segments");
    }
    return RR_OK;
}
