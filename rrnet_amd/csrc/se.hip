// Squeeze-and-excitation tail of the SE hourglass' residual block (backbones/se_hourglass.py:12-27,50-60) and the stem's
// 2x2 max-pool (:164) for gfx950.  NHWC fp32, C % 4 == 0, one 16-byte access per lane along C.
//
// All of them are bandwidth-bound (no MFMA).  The two reductions over the map (the squeeze and the backward's sum of
// g * u) run on a grid of samples x row chunks, so that a small batch still fills the chip; a chunk's workgroup lays
// its lanes over [rows, C / 4], every lane adds its rows in ascending order into doubles, and the rows of a workgroup
// meet in LDS in ascending order.  The per-sample kernels finish the chunks in ascending order, again in double.  No
// floating-point atomics anywhere: two runs give the same bits.  The partial sums are doubles because they cost
// nothing here (four adds per 16 bytes loaded) and leave the mean and ds rounded once.
#include <algorithm>

#include "common.h"
#include "rrnet_hip.h"
#include "rrnet_hip_se.h"

namespace {

typedef unsigned char u8;
typedef u8 u8x4 __attribute__((ext_vector_type(4)));

constexpr int TPB = 256;
constexpr int MAX_ROWS_PER_PASS = 32;        // lanes over rows of one pass: at most this many (tiny C would take all 256)
constexpr int MAX_C = 2048;                  // the per-sample kernels keep [C + C/r] doubles in LDS (at most 32 KB)

// Partial sums over a chunk of rows.  MUL: of (out > 0 ? dout : 0) * u, else of u.
//   grid (chunks, N); lanes: cv = t % LC, row = t / LC, LC = min(C / 4, TPB); channel tiles of LC when C / 4 > TPB.
template <bool MUL>
__global__ __launch_bounds__(TPB) void se_rows_kernel(const float *__restrict__ u, const float *__restrict__ dout,
                                                      const float *__restrict__ out, double *__restrict__ part, int HW, int C,
                                                      int chunk_rows)
{
    __shared__ double sh[TPB][4];
    const int CV = C / 4;
    const int LC = CV < TPB ? CV : TPB;
    int R = TPB / LC;
    if (R > MAX_ROWS_PER_PASS) R = MAX_ROWS_PER_PASS;
    const int n = blockIdx.y, chunk = blockIdx.x;
    const int r0 = chunk * chunk_rows;
    const int r1 = min(r0 + chunk_rows, HW);
    const int lane_c = threadIdx.x % LC, lane_r = threadIdx.x / LC;
    const bool active = lane_r < R;
    const long base = (long)n * HW * C;
    for (int cv0 = 0; cv0 < CV; cv0 += LC) {
        const int cv = cv0 + lane_c;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        if (active && cv < CV) {
            for (int r = r0 + lane_r; r < r1; r += R) {
                const long o = base + (long)r * C + (long)cv * 4;
                const rr_f32x4 a = *reinterpret_cast<const rr_f32x4 *>(u + o);
                if (MUL) {
                    const rr_f32x4 d = *reinterpret_cast<const rr_f32x4 *>(dout + o);
                    const rr_f32x4 z = *reinterpret_cast<const rr_f32x4 *>(out + o);
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (z[e] > 0.f) acc[e] += (double)d[e] * (double)a[e];
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[e] += (double)a[e];
                }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) sh[threadIdx.x][e] = acc[e];
        __syncthreads();
        if (lane_r == 0 && cv < CV) {
            double s[4] = {0.0, 0.0, 0.0, 0.0};
            for (int r = 0; r < R; ++r)
#pragma unroll
                for (int e = 0; e < 4; ++e) s[e] += sh[r * LC + lane_c][e];
            double *p = part + ((long)n * gridDim.x + chunk) * C + (long)cv * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) p[e] = s[e];
        }
        __syncthreads();
    }
}

// one workgroup per sample: partial sums -> m = mean, h = relu(W1 m), s = sigmoid(W2 h)
__global__ __launch_bounds__(TPB) void se_excite_fwd_kernel(const double *__restrict__ part, const float *__restrict__ w1,
                                                            const float *__restrict__ w2, float *__restrict__ m,
                                                            float *__restrict__ h, float *__restrict__ s, int nchunk, int C,
                                                            int CR, int HW)
{
    extern __shared__ double lds[];
    double *m_s = lds, *h_s = lds + C;
    const int n = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += TPB) {
        double a = 0.0;
        for (int k = 0; k < nchunk; ++k) a += part[((long)n * nchunk + k) * C + c];
        const float mf = (float)(a / (double)HW);
        m[(long)n * C + c] = mf;
        m_s[c] = (double)mf;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = wave; j < CR; j += TPB / 64) {
        double a = 0.0;
        for (int c = lane; c < C; c += 64) a += (double)w1[(long)j * C + c] * m_s[c];
        a = wave_sum_d(a);
        const float hf = a > 0.0 ? (float)a : 0.f;
        if (lane == 0) {
            h[(long)n * CR + j] = hf;
            h_s[j] = (double)hf;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += TPB) {
        double a = 0.0;
        for (int j = 0; j < CR; ++j) a += (double)w2[(long)c * CR + j] * h_s[j];
        s[(long)n * C + c] = (float)(1.0 / (1.0 + exp(-a)));
    }
}

// one workgroup per sample: ds -> d(W2 h) -> dh -> d(W1 m) -> dm; leaves dz2 [C] and dz1 [C/r] of the sample in `ws`
__global__ __launch_bounds__(TPB) void se_excite_bwd_kernel(const double *__restrict__ part, const float *__restrict__ s,
                                                            const float *__restrict__ h, const float *__restrict__ w1,
                                                            const float *__restrict__ w2, float *__restrict__ dm,
                                                            float *__restrict__ ws, int nchunk, int C, int CR)
{
    extern __shared__ double lds[];
    double *dz2_s = lds, *dz1_s = lds + C;
    const int n = blockIdx.x;
    float *ws_n = ws + (long)n * (C + CR);
    for (int c = threadIdx.x; c < C; c += TPB) {
        double a = 0.0;
        for (int k = 0; k < nchunk; ++k) a += part[((long)n * nchunk + k) * C + c];
        const double sv = (double)s[(long)n * C + c];
        const float d = (float)(a * sv * (1.0 - sv));
        ws_n[c] = d;
        dz2_s[c] = (double)d;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int j = wave; j < CR; j += TPB / 64) {
        double a = 0.0;
        for (int c = lane; c < C; c += 64) a += (double)w2[(long)c * CR + j] * dz2_s[c];
        a = wave_sum_d(a);
        const float d = h[(long)n * CR + j] > 0.f ? (float)a : 0.f;
        if (lane == 0) {
            ws_n[C + j] = d;
            dz1_s[j] = (double)d;
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += TPB) {
        double a = 0.0;
        for (int j = 0; j < CR; ++j) a += (double)w1[(long)j * C + c] * dz1_s[j];
        dm[(long)n * C + c] = (float)a;
    }
}

// dW1 [CR, C] += sum_n dz1[n, j] m[n, c];  dW2 [C, CR] += sum_n dz2[n, c] h[n, j]: one lane per element of each, samples in
// ascending order
__global__ __launch_bounds__(TPB) void se_excite_wgrad_kernel(const float *__restrict__ ws, const float *__restrict__ m,
                                                              const float *__restrict__ h, float *__restrict__ dw1,
                                                              float *__restrict__ dw2, int N, int C, int CR)
{
    const int t = blockIdx.x * TPB + threadIdx.x;
    const int per = C * CR;
    if (t >= 2 * per) return;
    const int stride = C + CR;
    double a = 0.0;
    if (t < per) {                                  // dW1[j, c]
        const int j = t / C, c = t - j * C;
        for (int n = 0; n < N; ++n) a += (double)ws[(long)n * stride + C + j] * (double)m[(long)n * C + c];
        dw1[t] += (float)a;
    } else {                                        // dW2[c, j]
        const int q = t - per;
        const int c = q / CR, j = q - c * CR;
        for (int n = 0; n < N; ++n) a += (double)ws[(long)n * stride + c] * (double)h[(long)n * CR + j];
        dw2[q] += (float)a;
    }
}

// out = relu(u * s[n, c] + skip)
__global__ __launch_bounds__(TPB) void se_scale_fwd_kernel(const float *__restrict__ u, const float *__restrict__ s,
                                                           const float *__restrict__ skip, float *__restrict__ out, long total,
                                                           long per_sample, int CV)
{
    const long stride = (long)gridDim.x * TPB;
    for (long t = (long)blockIdx.x * TPB + threadIdx.x; t < total; t += stride) {
        const long n = t / per_sample;
        const int cv = (int)(t % CV);
        const rr_f32x4 a = *reinterpret_cast<const rr_f32x4 *>(u + t * 4);
        const rr_f32x4 k = *reinterpret_cast<const rr_f32x4 *>(skip + t * 4);
        const rr_f32x4 sc = *reinterpret_cast<const rr_f32x4 *>(s + (n * CV + cv) * 4);
        rr_f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float v = __builtin_fmaf(a[e], sc[e], k[e]);
            r[e] = v < 0.f ? 0.f : v;               // (a NaN stays)
        }
        *reinterpret_cast<rr_f32x4 *>(out + t * 4) = r;
    }
}

// g = dout * (out > 0);  du = g * s[n, c] + dm[n, c] / HW;  dskip = g, or dskip_into += g
template <bool INTO>
__global__ __launch_bounds__(TPB) void se_apply_bwd_kernel(const float *__restrict__ dout, const float *__restrict__ out,
                                                           const float *__restrict__ s, const float *__restrict__ dm,
                                                           float *__restrict__ du, float *__restrict__ dskip, long total,
                                                           long per_sample, int CV, float hw)
{
    const long stride = (long)gridDim.x * TPB;
    for (long t = (long)blockIdx.x * TPB + threadIdx.x; t < total; t += stride) {
        const long n = t / per_sample;
        const int cv = (int)(t % CV);
        const rr_f32x4 d = *reinterpret_cast<const rr_f32x4 *>(dout + t * 4);
        const rr_f32x4 z = *reinterpret_cast<const rr_f32x4 *>(out + t * 4);
        const rr_f32x4 sc = *reinterpret_cast<const rr_f32x4 *>(s + (n * CV + cv) * 4);
        const rr_f32x4 mm = *reinterpret_cast<const rr_f32x4 *>(dm + (n * CV + cv) * 4);
        rr_f32x4 g, x;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            g[e] = z[e] > 0.f ? d[e] : 0.f;
            x[e] = __builtin_fmaf(g[e], sc[e], mm[e] / hw);
        }
        *reinterpret_cast<rr_f32x4 *>(du + t * 4) = x;
        if (INTO) {
            const rr_f32x4 old = *reinterpret_cast<const rr_f32x4 *>(dskip + t * 4);
            g += old;
        }
        *reinterpret_cast<rr_f32x4 *>(dskip + t * 4) = g;
    }
}

// MaxPool2d(2): window rows 2*oy, 2*oy+1, columns 2*ox, 2*ox+1; tap = ky * 2 + kx
__global__ __launch_bounds__(TPB) void maxpool2_fwd_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                           u8 *__restrict__ idx, long total, int H, int W, int OH, int OW, int CV)
{
    const long t = (long)blockIdx.x * TPB + threadIdx.x;
    if (t >= total) return;
    const int cv = (int)(t % CV);
    long p = t / CV;
    const int ox = (int)(p % OW);
    p /= OW;
    const int oy = (int)(p % OH);
    const long n = p / OH;
    const long C = (long)CV * 4;
    rr_f32x4 m;
    u8x4 tap = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int iy = 2 * oy + (k >> 1), ix = 2 * ox + (k & 1);         // inside the map: OH = H / 2, OW = W / 2
        const rr_f32x4 v = *reinterpret_cast<const rr_f32x4 *>(x + ((n * H + iy) * W + ix) * C + (long)cv * 4);
        if (k == 0) {
            m = v;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (v[e] > m[e] || v[e] != v[e]) {      // strictly larger, or a NaN (ATen's rule): the first maximum keeps the tap
                    m[e] = v[e];
                    tap[e] = (u8)k;
                }
        }
    }
    *reinterpret_cast<rr_f32x4 *>(y + t * 4) = m;
    *reinterpret_cast<u8x4 *>(idx + t * 4) = tap;
}

// dx written whole: an element of a window receives dy where the window's tap names it, the odd last row / column zeros
__global__ __launch_bounds__(TPB) void maxpool2_bwd_kernel(const float *__restrict__ dy, const u8 *__restrict__ idx,
                                                           float *__restrict__ dx, long total, int H, int W, int OH, int OW, int CV)
{
    const long t = (long)blockIdx.x * TPB + threadIdx.x;
    if (t >= total) return;
    const int cv = (int)(t % CV);
    long p = t / CV;
    const int ix = (int)(p % W);
    p /= W;
    const int iy = (int)(p % H);
    const long n = p / H;
    const long C = (long)CV * 4;
    rr_f32x4 r = {0.f, 0.f, 0.f, 0.f};
    const int oy = iy >> 1, ox = ix >> 1;
    if (oy < OH && ox < OW) {
        const long o = ((n * OH + oy) * OW + ox) * C + (long)cv * 4;
        const rr_f32x4 g = *reinterpret_cast<const rr_f32x4 *>(dy + o);
        const u8x4 k = *reinterpret_cast<const u8x4 *>(idx + o);
        const u8 want = (u8)((iy & 1) * 2 + (ix & 1));
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (k[e] == want) r[e] = g[e];
    }
    *reinterpret_cast<rr_f32x4 *>(dx + t * 4) = r;
}

constexpr long MAX_BLOCKS = 2147483647L;
inline int stream_blocks(long total) { return (int)std::min<long>((total + TPB - 1) / TPB, 256L * 16); }

// the shape checks the chunked reductions share; nchunk = ceil(hw / chunk_rows)
inline bool rows_ok(int n, int hw, int c, int chunk_rows)
{
    return n > 0 && n <= 65535 && hw > 0 && c > 0 && c % 4 == 0 && chunk_rows > 0 && (long)n * hw * c / 4 <= MAX_BLOCKS * TPB;
}

}  // namespace

extern "C" int rr_se_squeeze(const float *u, double *part, int n, int hw, int c, int chunk_rows, hipStream_t stream)
{
    RR_CHECK_ARG(u && part && rows_ok(n, hw, c, chunk_rows), "rr_se_squeeze: bad dims n=%d hw=%d c=%d (c %% 4 == 0) chunk_rows=%d",
                 n, hw, c, chunk_rows);
    const int nchunk = rr_cdiv(hw, chunk_rows);
    hipLaunchKernelGGL(se_rows_kernel<false>, dim3(nchunk, n), dim3(TPB), 0, stream, u, nullptr, nullptr, part, hw, c, chunk_rows);
    RR_CHECK_LAUNCH("rr_se_squeeze");
    return RR_OK;
}

extern "C" int rr_se_excite_fwd(const double *part, const float *w1, const float *w2, float *m, float *h, float *s, int n,
                                int nchunk, int c, int cr, int hw, hipStream_t stream)
{
    RR_CHECK_ARG(part && w1 && w2 && m && h && s && n > 0 && nchunk > 0 && c > 0 && c % 4 == 0 && c <= MAX_C && cr > 0 && cr <= c &&
                     hw > 0,
                 "rr_se_excite_fwd: bad dims n=%d nchunk=%d c=%d (c %% 4 == 0, <= %d) cr=%d hw=%d", n, nchunk, c, MAX_C, cr, hw);
    hipLaunchKernelGGL(se_excite_fwd_kernel, dim3(n), dim3(TPB), (size_t)(c + cr) * sizeof(double), stream, part, w1, w2, m, h, s,
                       nchunk, c, cr, hw);
    RR_CHECK_LAUNCH("rr_se_excite_fwd");
    return RR_OK;
}

extern "C" int rr_se_scale_res_relu_fwd(const float *u, const float *s, const float *skip, float *out, int n, int hw, int c,
                                        hipStream_t stream)
{
    RR_CHECK_ARG(u && s && skip && out && rows_ok(n, hw, c, 1), "rr_se_scale_res_relu_fwd: bad dims n=%d hw=%d c=%d (c %% 4 == 0)",
                 n, hw, c);
    const long per = (long)hw * (c / 4), total = per * n;
    hipLaunchKernelGGL(se_scale_fwd_kernel, dim3(stream_blocks(total)), dim3(TPB), 0, stream, u, s, skip, out, total, per, c / 4);
    RR_CHECK_LAUNCH("rr_se_scale_res_relu_fwd");
    return RR_OK;
}

extern "C" int rr_se_bwd_reduce(const float *dout, const float *out, const float *u, double *part, int n, int hw, int c,
                                int chunk_rows, hipStream_t stream)
{
    RR_CHECK_ARG(dout && out && u && part && rows_ok(n, hw, c, chunk_rows),
                 "rr_se_bwd_reduce: bad dims n=%d hw=%d c=%d (c %% 4 == 0) chunk_rows=%d", n, hw, c, chunk_rows);
    const int nchunk = rr_cdiv(hw, chunk_rows);
    hipLaunchKernelGGL(se_rows_kernel<true>, dim3(nchunk, n), dim3(TPB), 0, stream, u, dout, out, part, hw, c, chunk_rows);
    RR_CHECK_LAUNCH("rr_se_bwd_reduce");
    return RR_OK;
}

extern "C" int rr_se_excite_bwd(const double *part, const float *s, const float *h, const float *m, const float *w1,
                                const float *w2, float *dm, float *dw1, float *dw2, float *ws, int n, int nchunk, int c, int cr,
                                hipStream_t stream)
{
    RR_CHECK_ARG(part && s && h && m && w1 && w2 && dm && dw1 && dw2 && ws && n > 0 && nchunk > 0 && c > 0 && c % 4 == 0 &&
                     c <= MAX_C && cr > 0 && cr <= c,
                 "rr_se_excite_bwd: bad dims n=%d nchunk=%d c=%d (c %% 4 == 0, <= %d) cr=%d", n, nchunk, c, MAX_C, cr);
    hipLaunchKernelGGL(se_excite_bwd_kernel, dim3(n), dim3(TPB), (size_t)(c + cr) * sizeof(double), stream, part, s, h, w1, w2, dm,
                       ws, nchunk, c, cr);
    RR_CHECK_LAUNCH("rr_se_excite_bwd");
    hipLaunchKernelGGL(se_excite_wgrad_kernel, dim3(rr_cdiv(2L * c * cr, TPB)), dim3(TPB), 0, stream, ws, m, h, dw1, dw2, n, c, cr);
    RR_CHECK_LAUNCH("rr_se_excite_bwd");
    return RR_OK;
}

extern "C" int rr_se_bwd_apply(const float *dout, const float *out, const float *s, const float *dm, float *du, float *dskip,
                               float *dskip_into, int n, int hw, int c, hipStream_t stream)
{
    RR_CHECK_ARG(dout && out && s && dm && du && ((dskip != nullptr) != (dskip_into != nullptr)) && rows_ok(n, hw, c, 1),
                 "rr_se_bwd_apply: bad dims n=%d hw=%d c=%d (c %% 4 == 0), or not exactly one of dskip / dskip_into", n, hw, c);
    const long per = (long)hw * (c / 4), total = per * n;
    if (dskip_into)
        hipLaunchKernelGGL(se_apply_bwd_kernel<true>, dim3(stream_blocks(total)), dim3(TPB), 0, stream, dout, out, s, dm, du,
                           dskip_into, total, per, c / 4, (float)hw);
    else
        hipLaunchKernelGGL(se_apply_bwd_kernel<false>, dim3(stream_blocks(total)), dim3(TPB), 0, stream, dout, out, s, dm, du, dskip,
                           total, per, c / 4, (float)hw);
    RR_CHECK_LAUNCH("rr_se_bwd_apply");
    return RR_OK;
}

extern "C" int rr_maxpool2x2_fwd(const float *x, float *y, unsigned char *idx, int n, int h, int w, int c, hipStream_t stream)
{
    RR_CHECK_ARG(x && y && idx && n > 0 && h >= 2 && w >= 2 && c > 0 && c % 4 == 0,
                 "rr_maxpool2x2_fwd: bad dims %d %d %d %d (h, w >= 2: the output would be empty; c %% 4 == 0)", n, h, w, c);
    const int oh = h / 2, ow = w / 2;
    const long total = (long)n * oh * ow * (c / 4);
    RR_CHECK_ARG((total + TPB - 1) / TPB <= MAX_BLOCKS, "rr_maxpool2x2_fwd: tensor too large");
    hipLaunchKernelGGL(maxpool2_fwd_kernel, dim3(rr_cdiv(total, TPB)), dim3(TPB), 0, stream, x, y, idx, total, h, w, oh, ow, c / 4);
    RR_CHECK_LAUNCH("rr_maxpool2x2_fwd");
    return RR_OK;
}

extern "C" int rr_maxpool2x2_bwd(const float *dy, const unsigned char *idx, float *dx, int n, int h, int w, int c,
                                 hipStream_t stream)
{
    RR_CHECK_ARG(dy && idx && dx && n > 0 && h >= 2 && w >= 2 && c > 0 && c % 4 == 0,
                 "rr_maxpool2x2_bwd: bad dims %d %d %d %d (h, w >= 2; c %% 4 == 0)", n, h, w, c);
    const int oh = h / 2, ow = w / 2;
    const long total = (long)n * h * w * (c / 4);
    RR_CHECK_ARG((total + TPB - 1) / TPB <= MAX_BLOCKS, "rr_maxpool2x2_bwd: tensor too large");
    hipLaunchKernelGGL(maxpool2_bwd_kernel, dim3(rr_cdiv(total, TPB)), dim3(TPB), 0, stream, dy, idx, dx, total, h, w, oh, ow, c / 4);
    RR_CHECK_LAUNCH("rr_maxpool2x2_bwd");
    return RR_OK;
}
