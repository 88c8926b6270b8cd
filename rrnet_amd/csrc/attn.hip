// Dilated-window attention of modules/self_attention.py:67-91 for gfx950, without the unfolded tensors.  NHWC fp32,
// CK % 4 == CV % 4 == 0, one 16-byte access per lane along the channels.
//
// The reference unfolds key and value into [b, c, T, h, w] (T = kh * kw taps) and runs the products, the softmax and the
// weighted sum as separate passes over them.  Here a pixel's T taps are gathered where they lie: a group of 16 lanes owns
// one pixel, lane `sub` of the group holds channels 4 sub .. 4 sub + 3 (and 64 further on, for more than 64 channels), so
// that a tap is ONE 16-byte load per lane and the group reads the tap's 256 contiguous bytes.  A workgroup is 16 such
// groups on 16 consecutive pixels of a row.  A dot product is finished with four xor-shuffles inside the group, the T
// logits of a pixel meet in LDS (4 KB per workgroup), the softmax runs over them with the group's lanes spread over the
// taps, and the weighted sum gathers the taps a second time.
//
// The halo is left to the caches: a 5x5 window at dilation 6 spans 25x25 pixels, i.e. 160 KB of key and value at 64
// channels per pixel row segment a workgroup would have to stage; no channel chunk of it that fits LDS is reused by more
// than the 16 pixels that sit in the workgroup anyway, while in L2 every key / value row is reused by the kh output rows
// and kw columns that read it.  The arithmetic (4 T (CK + CV) flop per pixel) is negligible beside those reads.
//
// Three launches: forward (ctx and the stashed P), backward over the query positions (dS and dq), backward over the
// key / value positions (dk, dv as gathers over the outputs that read a position).  No floating-point atomics; every sum
// has a fixed order (channels ascending in a lane, the shuffle tree, taps ascending); every output is written whole.
#include "common.h"
#include "rrnet_hip.h"
#include "rrnet_hip_attn.h"

namespace {

constexpr int TPB = 256;
constexpr int GROUP = 16;                    // lanes of one pixel
constexpr int PIX = TPB / GROUP;             // pixels of one workgroup
constexpr int MAX_TAPS = 64;                 // a pixel's row of logits in LDS; admits 7x7 (and 8x8)

// The window's index rule, stated once for the three kernels.
struct Window {
    int H, W, OH, OW, KH, KW, DH, DW, PH, PW, CY, CX;

    // source (y, x) of tap (a, b) of output (i, j) -> inside the map?  Outside, (y, x) comes back clamped into the map: an
    // address that exists, for a load whose value the caller drops.
    __device__ __forceinline__ bool source(int i, int j, int a, int b, int &y, int &x) const
    {
        const int sy = i - PH + a * DH, sx = j - PW + b * DW;
        y = min(max(sy, 0), H - 1);
        x = min(max(sx, 0), W - 1);
        return sy == y && sx == x;
    }
    // the output (i, j) whose tap (a, b) reads the source (y, x) -> does it exist?  (clamped likewise where it does not)
    __device__ __forceinline__ bool reader(int y, int x, int a, int b, int &i, int &j) const
    {
        const int ri = y + PH - a * DH, rj = x + PW - b * DW;
        i = min(max(ri, 0), OH - 1);
        j = min(max(rj, 0), OW - 1);
        return ri == i && rj == j;
    }
    // query position of output (i, j)
    __device__ __forceinline__ void centre(int i, int j, int &qy, int &qx) const
    {
        qy = i + CY;
        qx = j + CX;
    }
    // the output whose query position is (qy, qx) -> does it exist?
    __device__ __forceinline__ bool centre_of(int qy, int qx, int &i, int &j) const
    {
        i = qy - CY;
        j = qx - CX;
        return i >= 0 && i < OH && j >= 0 && j < OW;
    }
};

__device__ __forceinline__ rr_f32x4 ld4(const float *p) { return *reinterpret_cast<const rr_f32x4 *>(p); }
__device__ __forceinline__ void st4(float *p, rr_f32x4 v) { *reinterpret_cast<rr_f32x4 *>(p) = v; }

// One DPP row is 16 lanes = one group: quad swaps, then the mirrored half rows, then the mirrored row.  Every level adds the
// sums of two disjoint sets of lanes, and a + b == b + a bit for bit, so all 16 lanes end with the same value.
#define RR_ATTN_DPP(v, ctrl) __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), ctrl, 0xf, 0xf, false))
__device__ __forceinline__ float group_sum(float v)
{
    v += RR_ATTN_DPP(v, 0xB1);       // quad_perm [1,0,3,2]
    v += RR_ATTN_DPP(v, 0x4E);       // quad_perm [2,3,0,1]
    v += RR_ATTN_DPP(v, 0x141);      // row_half_mirror: lane i <- lane 7 - i
    v += RR_ATTN_DPP(v, 0x140);      // row_mirror: lane i <- lane 15 - i
    return v;
}
__device__ __forceinline__ float group_max(float v)
{
    v = fmaxf(v, RR_ATTN_DPP(v, 0xB1));
    v = fmaxf(v, RR_ATTN_DPP(v, 0x4E));
    v = fmaxf(v, RR_ATTN_DPP(v, 0x141));
    v = fmaxf(v, RR_ATTN_DPP(v, 0x140));
    return v;
}

// The tap loops below are free of branches: a tap outside the map is loaded from the clamped position and dropped by a select
// (never multiplied by 0: the clamped position may hold an Inf), so that the loads of several taps are in flight together.

// row[t] = a . src[y, x, :] for the taps of output (i, j) inside the map, 0 for the others.  a: the pixel's own vector of C
// channels, src: the image [H, W, C] the taps are gathered from.  A pixel that is not valid stands on pixel 0 of image 0 (its
// addresses exist) and gets zeros.  Every lane of the workgroup runs the reductions.
__device__ __forceinline__ void window_dots(const Window &g, bool valid, int i, int j, const float *__restrict__ a,
                                            const float *__restrict__ src, int C, int sub, float *row)
{
    const int C4 = C / 4, T = g.KH * g.KW;
    const bool own = valid && sub < C4;
    const int q0 = sub < C4 ? sub : 0;
    const rr_f32x4 a0 = ld4(a + q0 * 4);
    int ta = 0, tb = 0;
#pragma unroll 4
    for (int t = 0; t < T; ++t) {
        int y, x;
        const bool inside = g.source(i, j, ta, tb, y, x);
        const float *s = src + ((long)y * g.W + x) * C;
        const rr_f32x4 b0 = ld4(s + q0 * 4);
        float part = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) part = __builtin_fmaf(a0[e], b0[e], part);
        for (int cq = sub + GROUP; cq < C4; cq += GROUP) {
            const rr_f32x4 av = ld4(a + cq * 4), bv = ld4(s + cq * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) part = __builtin_fmaf(av[e], bv[e], part);
        }
        part = group_sum(own && inside ? part : 0.f);
        if (sub == 0) row[t] = part;
        if (++tb == g.KW) {
            tb = 0;
            ++ta;
        }
    }
}

// out[:] = sum over the taps of output (i, j) inside the map, ascending, of row[t] * src[y, x, :]; zeros for a pixel that
// is not valid.  out: the pixel's own vector of C channels, or null (a lane past the last pixel: nothing is written).
__device__ __forceinline__ void window_gather(const Window &g, bool valid, int i, int j, const float *row,
                                              const float *__restrict__ src, int C, int sub, float *__restrict__ out)
{
    const int C4 = C / 4, T = g.KH * g.KW;
    for (int cq = sub; cq < C4; cq += GROUP) {
        rr_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        int ta = 0, tb = 0;
#pragma unroll 4
        for (int t = 0; t < T; ++t) {
            int y, x;
            const bool inside = g.source(i, j, ta, tb, y, x) && valid;
            const float wgt = row[t];
            const rr_f32x4 s = ld4(src + ((long)y * g.W + x) * C + cq * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = inside ? __builtin_fmaf(wgt, s[e], acc[e]) : acc[e];
            if (++tb == g.KW) {
                tb = 0;
                ++ta;
            }
        }
        if (out) st4(out + cq * 4, acc);
    }
}

// forward: one group per output pixel
__global__ __launch_bounds__(TPB) void attn_fwd_kernel(const float *__restrict__ q, const float *__restrict__ k,
                                                       const float *__restrict__ v, float *__restrict__ ctx, float *__restrict__ p,
                                                       Window g, int CK, int CV, long pixels)
{
    __shared__ float sh[PIX][MAX_TAPS];
    const int sub = threadIdx.x % GROUP, pl = threadIdx.x / GROUP;
    const int T = g.KH * g.KW;
    const long pix = (long)blockIdx.x * PIX + pl;
    const bool valid = pix < pixels;
    const long per = (long)g.OH * g.OW;
    const long n = valid ? pix / per : 0;
    const int r = valid ? (int)(pix - n * per) : 0;
    const int i = r / g.OW, j = r - i * g.OW;
    int qy, qx;
    g.centre(i, j, qy, qx);
    const long img = n * g.H * g.W;
    float *row = sh[pl];
    window_dots(g, valid, i, j, q + ((img + (long)qy * g.W + qx) * CK), k + img * CK, CK, sub, row);
    __syncthreads();
    float m = -INFINITY;
    for (int t = sub; t < T; t += GROUP) m = fmaxf(m, row[t]);
    m = group_max(m);
    float s = 0.f;
    for (int t = sub; t < T; t += GROUP) {
        const float e = expf(row[t] - m);
        row[t] = e;                              // (lane sub owns the taps sub, sub + 16, ..: nobody else reads them before the barrier)
        s += e;
    }
    s = group_sum(s);
    for (int t = sub; t < T; t += GROUP) {
        const float w = row[t] / s;
        row[t] = w;
        if (valid) p[pix * T + t] = w;
    }
    __syncthreads();
    window_gather(g, valid, i, j, row, v + img * CV, CV, sub, valid ? ctx + pix * CV : nullptr);
}

// backward over the query positions: one group per pixel of the map
__global__ __launch_bounds__(TPB) void attn_bwd_q_kernel(const float *__restrict__ dctx, const float *__restrict__ v,
                                                         const float *__restrict__ k, const float *__restrict__ p,
                                                         float *__restrict__ ds, float *__restrict__ dq, Window g, int CK, int CV,
                                                         long pixels)
{
    __shared__ float sh[PIX][MAX_TAPS];
    const int sub = threadIdx.x % GROUP, pl = threadIdx.x / GROUP;
    const int T = g.KH * g.KW;
    const long pix = (long)blockIdx.x * PIX + pl;             // over [n, H, W]
    const bool in_map = pix < pixels;
    const long per = (long)g.H * g.W;
    const long n = in_map ? pix / per : 0;
    const int r = in_map ? (int)(pix - n * per) : 0;
    const int qy = r / g.W, qx = r - qy * g.W;
    int i, j;
    const bool valid = g.centre_of(qy, qx, i, j) && in_map;   // an output reads this query
    const long opix = valid ? (n * g.OH + i) * g.OW + j : 0;
    const long img = n * per;
    float *row = sh[pl];
    window_dots(g, valid, i, j, dctx + opix * CV, v + img * CV, CV, sub, row);
    __syncthreads();
    float s = 0.f;
    for (int t = sub; t < T; t += GROUP) {
        const float w = valid ? p[opix * T + t] : 0.f;
        s = __builtin_fmaf(w, row[t], s);
    }
    s = group_sum(s);
    for (int t = sub; t < T; t += GROUP) {
        if (valid) {
            const float d = p[opix * T + t] * (row[t] - s);
            row[t] = d;
            ds[opix * T + t] = d;
        }
    }
    __syncthreads();
    window_gather(g, valid, i, j, row, k + img * CK, CK, sub, in_map ? dq + pix * CK : nullptr);
}

// backward over the key / value positions: one group per pixel of the map, a gather over the outputs that read it
__global__ __launch_bounds__(TPB) void attn_bwd_kv_kernel(const float *__restrict__ ds, const float *__restrict__ p,
                                                          const float *__restrict__ q, const float *__restrict__ dctx,
                                                          float *__restrict__ dk, float *__restrict__ dv, Window g, int CK, int CV,
                                                          long pixels)
{
    const int sub = threadIdx.x % GROUP, pl = threadIdx.x / GROUP;
    const int T = g.KH * g.KW;
    const long pix = (long)blockIdx.x * PIX + pl;             // over [n, H, W]
    if (pix >= pixels) return;
    const long per = (long)g.H * g.W;
    const long n = pix / per;
    const int r = (int)(pix - n * per);
    const int y = r / g.W, x = r - y * g.W;
    const long oimg = n * g.OH * g.OW;
    const int CK4 = CK / 4, CV4 = CV / 4;
    for (int cq = sub; cq < CK4; cq += GROUP) {
        rr_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        int ta = 0, tb = 0;
#pragma unroll 4
        for (int t = 0; t < T; ++t) {
            int i, j, qy, qx;
            const bool reads = g.reader(y, x, ta, tb, i, j);
            g.centre(i, j, qy, qx);
            const float wgt = ds[(oimg + (long)i * g.OW + j) * T + t];
            const rr_f32x4 s = ld4(q + (n * per + (long)qy * g.W + qx) * CK + cq * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = reads ? __builtin_fmaf(wgt, s[e], acc[e]) : acc[e];
            if (++tb == g.KW) {
                tb = 0;
                ++ta;
            }
        }
        st4(dk + pix * CK + cq * 4, acc);
    }
    for (int cq = sub; cq < CV4; cq += GROUP) {
        rr_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        int ta = 0, tb = 0;
#pragma unroll 4
        for (int t = 0; t < T; ++t) {
            int i, j;
            const bool reads = g.reader(y, x, ta, tb, i, j);
            const long o = oimg + (long)i * g.OW + j;
            const float wgt = p[o * T + t];
            const rr_f32x4 s = ld4(dctx + o * CV + cq * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[e] = reads ? __builtin_fmaf(wgt, s[e], acc[e]) : acc[e];
            if (++tb == g.KW) {
                tb = 0;
                ++ta;
            }
        }
        st4(dv + pix * CV + cq * 4, acc);
    }
}

constexpr long MAX_BLOCKS = 2147483647L;

// the geometry checks the three entries share -> the message of the first one that fails, or nullptr
inline const char *window_of(Window &g, int n, int h, int w, int ck, int cv, int kh, int kw, int dh, int dw, int ph, int pw)
{
    if (n < 1 || h < 1 || w < 1 || ck < 1 || cv < 1 || kh < 1 || kw < 1 || dh < 1 || dw < 1 || ph < 0 || pw < 0)
        return "a size below 1 or a negative padding";
    if (ck % 4 != 0 || cv % 4 != 0) return "ck % 4 == 0 and cv % 4 == 0 are required";
    if ((long)kh * kw > MAX_TAPS) return "more than 64 taps";
    const long oh = (long)h + 2L * ph - (long)dh * (kh - 1), ow = (long)w + 2L * pw - (long)dw * (kw - 1);
    const long cy = (long)dh * (kh / 2) - ph, cx = (long)dw * (kw / 2) - pw;
    if (cy < 0 || cx < 0) return "the padding exceeds dilation * (kernel / 2): the centre would lie outside the map";
    if (oh < 1 || ow < 1) return "the output is empty";
    if (cy + oh > h || cx + ow > w) return "outputs without a query position (centre + output size exceeds the map)";
    if (((long)n * h * w + PIX - 1) / PIX > MAX_BLOCKS) return "tensor too large";
    g = Window{h, w, (int)oh, (int)ow, kh, kw, dh, dw, ph, pw, (int)cy, (int)cx};
    return nullptr;
}

#define RR_ATTN_DIMS "n=%d h=%d w=%d ck=%d cv=%d kernel=(%d,%d) dilation=(%d,%d) padding=(%d,%d)"

}  // namespace

extern "C" int rr_attn_fwd(const float *q, const float *k, const float *v, float *ctx, float *p, int n, int h, int w, int ck,
                           int cv, int kh, int kw, int dh, int dw, int ph, int pw, hipStream_t stream)
{
    Window g;
    RR_CHECK_ARG(q && k && v && ctx && p, "rr_attn_fwd: null pointer");
    const char *why = window_of(g, n, h, w, ck, cv, kh, kw, dh, dw, ph, pw);
    RR_CHECK_ARG(!why, "rr_attn_fwd: %s (" RR_ATTN_DIMS ")", why, n, h, w, ck, cv, kh, kw, dh, dw, ph, pw);
    const long pixels = (long)n * g.OH * g.OW;
    hipLaunchKernelGGL(attn_fwd_kernel, dim3(rr_cdiv(pixels, PIX)), dim3(TPB), 0, stream, q, k, v, ctx, p, g, ck, cv, pixels);
    RR_CHECK_LAUNCH("rr_attn_fwd");
    return RR_OK;
}

extern "C" int rr_attn_bwd_q(const float *dctx, const float *v, const float *k, const float *p, float *ds, float *dq, int n,
                             int h, int w, int ck, int cv, int kh, int kw, int dh, int dw, int ph, int pw, hipStream_t stream)
{
    Window g;
    RR_CHECK_ARG(dctx && v && k && p && ds && dq, "rr_attn_bwd_q: null pointer");
    const char *why = window_of(g, n, h, w, ck, cv, kh, kw, dh, dw, ph, pw);
    RR_CHECK_ARG(!why, "rr_attn_bwd_q: %s (" RR_ATTN_DIMS ")", why, n, h, w, ck, cv, kh, kw, dh, dw, ph, pw);
    const long pixels = (long)n * h * w;
    hipLaunchKernelGGL(attn_bwd_q_kernel, dim3(rr_cdiv(pixels, PIX)), dim3(TPB), 0, stream, dctx, v, k, p, ds, dq, g, ck, cv,
                       pixels);
    RR_CHECK_LAUNCH("rr_attn_bwd_q");
    return RR_OK;
}

extern "C" int rr_attn_bwd_kv(const float *ds, const float *p, const float *q, const float *dctx, float *dk, float *dv, int n,
                              int h, int w, int ck, int cv, int kh, int kw, int dh, int dw, int ph, int pw, hipStream_t stream)
{
    Window g;
    RR_CHECK_ARG(ds && p && q && dctx && dk && dv, "rr_attn_bwd_kv: null pointer");
    const char *why = window_of(g, n, h, w, ck, cv, kh, kw, dh, dw, ph, pw);
    RR_CHECK_ARG(!why, "rr_attn_bwd_kv: %s (" RR_ATTN_DIMS ")", why, n, h, w, ck, cv, kh, kw, dh, dw, ph, pw);
    const long pixels = (long)n * h * w;
    hipLaunchKernelGGL(attn_bwd_kv_kernel, dim3(rr_cdiv(pixels, PIX)), dim3(TPB), 0, stream, ds, p, q, dctx, dk, dv, g, ck, cv,
                       pixels);
    RR_CHECK_LAUNCH("rr_attn_bwd_kv");
    return RR_OK;
}
