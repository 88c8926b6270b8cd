// ShuffleNetV2's kernel family for gfx950 (backbones/shufflenet.py): the depthwise 3x3 convolution (forward with the
// BatchNorm partial sums, data gradient, weight gradient) and the channel shuffle with its split / join copies.
// NHWC fp32, C % 4 == 0, one 16-byte access per lane along C.
//
// A depthwise convolution has no reduction over channels: 9 multiply-adds per output element against 4 bytes written and
// (with the taps of neighbouring pixels served by the caches) about 4 bytes read.  Nothing here goes near the matrix cores;
// all of it is bound by memory, and at the batch sizes RetinaNet trains with by the number of workgroups a layer offers.
// The forward and the weight gradient run one workgroup per (tile of output pixels, group of 64 channels), lanes laid over
// [pixels of a pass, C / 4 of the group]: every lane adds its pixels in ascending order into doubles, the lanes of a workgroup
// meet in LDS in ascending order, and the tiles are added in ascending order by a second kernel (the weight gradient) or by
// the BatchNorm statistics kernels (the slab).  No floating-point atomics: two runs give the same bits.
//
// Compiled with -ffp-contract=off (build.py): the forward and the data gradient are the chain "round every product, add it to
// the running sum, taps ascending", which is what their float32 yardstick in tests/shufflenet_cases.py computes.
#include <algorithm>

#include "common.h"
#include "rrnet_hip.h"
#include "rrnet_hip_dw.h"

namespace {

constexpr int TPB = 256;
constexpr int SLAB_PIXELS = RR_DW_SLAB_PIXELS;  // output pixels per forward workgroup = per slab tile
constexpr int MAX_ROWS = 32;                    // lanes over pixels of one pass: at most this many (tiny C would take all 256)
constexpr int GROUP_CV = 16;                    // channel vectors (of 4 channels) one workgroup covers
constexpr long MAX_BYTES = 1L << 31;            // a tensor of 2 GiB or more is refused

// the 36 filter values of a lane's four channels: f[(4 cv + e) * 9 + t] = wr[e * 9 + t], 144 contiguous bytes
struct Taps {
    float wr[36];
    __device__ __forceinline__ void load(const float *__restrict__ f, int cv)
    {
        const rr_f32x4 *p = reinterpret_cast<const rr_f32x4 *>(f + (long)cv * 36);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const rr_f32x4 v = p[k];
#pragma unroll
            for (int e = 0; e < 4; ++e) wr[k * 4 + e] = v[e];
        }
    }
    __device__ __forceinline__ float at(int e, int t) const { return wr[e * 9 + t]; }
};

// lanes of a workgroup over [rows, channel vectors].  blockIdx.y names a group of LC = min(CV, GROUP_CV) channel vectors (so that
// a small map with many channels still spreads over the chip), R = min(TPB / LC, MAX_ROWS) rows of lanes share them.
struct Lanes {
    int LC, R, lane_c, lane_r, cv;
    __device__ __forceinline__ Lanes(int CV)
    {
        LC = CV < GROUP_CV ? CV : GROUP_CV;
        R = TPB / LC;
        if (R > MAX_ROWS) R = MAX_ROWS;
        lane_c = threadIdx.x % LC;
        lane_r = threadIdx.x / LC;
        cv = blockIdx.y * LC + lane_c;
    }
    __device__ __forceinline__ bool active(int CV) const { return lane_r < R && cv < CV; }
};
inline int channel_groups(int c) { return rr_cdiv(c / 4, std::min(c / 4, GROUP_CV)); }

// grid: (tiles of SLAB_PIXELS output pixels, channel groups).  STATS: slab[tile][0][c] = sum of the tile's y, slab[tile][1][c] = sum of y * y.
template <int S, bool STATS>
__global__ __launch_bounds__(TPB) void dw_fwd_kernel(const float *__restrict__ x, const float *__restrict__ f,
                                                     const float *__restrict__ bias, float *__restrict__ y,
                                                     double *__restrict__ slab, int H, int W, int P, int Q, int C, long pixels)
{
    __shared__ double sh[STATS ? TPB : 1][8];
    const int CV = C / 4;
    const Lanes L(CV);
    const long p0 = (long)blockIdx.x * SLAB_PIXELS;
    const long p1 = p0 + SLAB_PIXELS < pixels ? p0 + SLAB_PIXELS : pixels;
    {
        const int cv = L.cv;
        const bool on = L.active(CV);
        double sum[4] = {0.0, 0.0, 0.0, 0.0}, sq[4] = {0.0, 0.0, 0.0, 0.0};
        if (on) {
            Taps w;
            w.load(f, cv);
            rr_f32x4 b = {0.f, 0.f, 0.f, 0.f};
            if (bias) b = *reinterpret_cast<const rr_f32x4 *>(bias + (long)cv * 4);
            for (long p = p0 + L.lane_r; p < p1; p += L.R) {
                const int j = (int)(p % Q);
                const long pi = p / Q;
                const int i = (int)(pi % P);
                const long n = pi / P;
                rr_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int iy = i * S - 1 + a;
                    if (iy < 0 || iy >= H) continue;
#pragma unroll
                    for (int bb = 0; bb < 3; ++bb) {
                        const int ix = j * S - 1 + bb;
                        if (ix < 0 || ix >= W) continue;
                        const rr_f32x4 v = *reinterpret_cast<const rr_f32x4 *>(x + ((n * H + iy) * W + ix) * C + (long)cv * 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[e] = acc[e] + w.at(e, a * 3 + bb) * v[e];
                    }
                }
                if (bias) acc = acc + b;
                *reinterpret_cast<rr_f32x4 *>(y + p * C + (long)cv * 4) = acc;
                if (STATS) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double d = (double)acc[e];
                        sum[e] += d;
                        sq[e] += d * d;
                    }
                }
            }
        }
        if (STATS) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                sh[threadIdx.x][e] = sum[e];
                sh[threadIdx.x][4 + e] = sq[e];
            }
            __syncthreads();
            if (L.lane_r == 0 && cv < CV) {
                double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                for (int r = 0; r < L.R; ++r)
#pragma unroll
                    for (int e = 0; e < 8; ++e) s[e] += sh[r * L.LC + L.lane_c][e];
                double *o = slab + (long)blockIdx.x * 2 * C + (long)cv * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    o[e] = s[e];
                    o[C + e] = s[4 + e];
                }
            }
        }
    }
}

// one lane per four channels of an input pixel: the gather over the outputs that read it
template <int S>
__global__ __launch_bounds__(TPB) void dw_bwd_data_kernel(const float *__restrict__ dy, const float *__restrict__ f,
                                                          float *__restrict__ dx, int H, int W, int P, int Q, int CV, long total)
{
    const long stride = (long)gridDim.x * TPB;
    const long C = (long)CV * 4;
    for (long t = (long)blockIdx.x * TPB + threadIdx.x; t < total; t += stride) {
        const int cv = (int)(t % CV);
        long p = t / CV;
        const int xx = (int)(p % W);
        p /= W;
        const int yy = (int)(p % H);
        const long n = p / H;
        Taps w;
        w.load(f, cv);
        rr_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const int ty = yy + 1 - a;
            if (ty < 0 || ty % S != 0 || ty / S >= P) continue;
#pragma unroll
            for (int bb = 0; bb < 3; ++bb) {
                const int tx = xx + 1 - bb;
                if (tx < 0 || tx % S != 0 || tx / S >= Q) continue;
                const rr_f32x4 g = *reinterpret_cast<const rr_f32x4 *>(dy + ((n * P + ty / S) * Q + tx / S) * C + (long)cv * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[e] = acc[e] + w.at(e, a * 3 + bb) * g[e];
            }
        }
        *reinterpret_cast<rr_f32x4 *>(dx + t * 4) = acc;
    }
}

// stage one of the weight gradient; grid: (tiles of tile_pixels output pixels, channel groups) -> partial[tile][c][9]
template <int S>
__global__ __launch_bounds__(TPB) void dw_wgrad_tile_kernel(const float *__restrict__ x, const float *__restrict__ dy,
                                                            double *__restrict__ partial, int H, int W, int P, int Q, int C,
                                                            long pixels, int tile_pixels)
{
    __shared__ double sh[TPB][4];
    const int CV = C / 4;
    const Lanes L(CV);
    const long p0 = (long)blockIdx.x * tile_pixels;
    const long p1 = p0 + tile_pixels < pixels ? p0 + tile_pixels : pixels;
    {
        const int cv = L.cv;
        const bool on = L.active(CV);
        double acc[9][4];
#pragma unroll
        for (int t = 0; t < 9; ++t)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[t][e] = 0.0;
        if (on) {
            for (long p = p0 + L.lane_r; p < p1; p += L.R) {
                const int j = (int)(p % Q);
                const long pi = p / Q;
                const int i = (int)(pi % P);
                const long n = pi / P;
                const rr_f32x4 g = *reinterpret_cast<const rr_f32x4 *>(dy + p * C + (long)cv * 4);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int iy = i * S - 1 + a;
                    if (iy < 0 || iy >= H) continue;
#pragma unroll
                    for (int bb = 0; bb < 3; ++bb) {
                        const int ix = j * S - 1 + bb;
                        if (ix < 0 || ix >= W) continue;
                        const rr_f32x4 v = *reinterpret_cast<const rr_f32x4 *>(x + ((n * H + iy) * W + ix) * C + (long)cv * 4);
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[a * 3 + bb][e] += (double)v[e] * (double)g[e];
                    }
                }
            }
        }
        double *o = partial + (long)blockIdx.x * C * 9 + (long)cv * 36;
#pragma unroll
        for (int t = 0; t < 9; ++t) {
#pragma unroll
            for (int e = 0; e < 4; ++e) sh[threadIdx.x][e] = acc[t][e];
            __syncthreads();
            if (L.lane_r == 0 && cv < CV) {
                double s[4] = {0.0, 0.0, 0.0, 0.0};
                for (int r = 0; r < L.R; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) s[e] += sh[r * L.LC + L.lane_c][e];
#pragma unroll
                for (int e = 0; e < 4; ++e) o[e * 9 + t] = s[e];
            }
            __syncthreads();
        }
    }
}

// stage two: one lane per filter value, the tiles in ascending order
__global__ __launch_bounds__(TPB) void dw_wgrad_final_kernel(const double *__restrict__ partial, float *__restrict__ df, int tiles,
                                                             int count, int accumulate)
{
    const int t = blockIdx.x * TPB + threadIdx.x;
    if (t >= count) return;
    double a = 0.0;
    for (int k = 0; k < tiles; ++k) a += partial[(long)k * count + t];
    if (accumulate) a += (double)df[t];
    df[t] = (float)a;
}

// ---- the shuffle family: one lane per four channels of each operand ------------------------------------------------------
__global__ __launch_bounds__(TPB) void interleave_kernel(const float *__restrict__ a, long as, const float *__restrict__ b, long bs,
                                                         float *__restrict__ out, long os, int HV, long total)
{
    const long stride = (long)gridDim.x * TPB;
    for (long t = (long)blockIdx.x * TPB + threadIdx.x; t < total; t += stride) {
        const long p = t / HV;
        const long i = (t % HV) * 4;
        const rr_f32x4 va = *reinterpret_cast<const rr_f32x4 *>(a + p * as + i);
        const rr_f32x4 vb = *reinterpret_cast<const rr_f32x4 *>(b + p * bs + i);
        const rr_f32x4 lo = {va[0], vb[0], va[1], vb[1]};
        const rr_f32x4 hi = {va[2], vb[2], va[3], vb[3]};
        rr_f32x4 *o = reinterpret_cast<rr_f32x4 *>(out + p * os + 2 * i);
        o[0] = lo;
        o[1] = hi;
    }
}

__global__ __launch_bounds__(TPB) void deinterleave_kernel(const float *__restrict__ g, long gs, float *__restrict__ da, long as,
                                                           float *__restrict__ db, long bs, int HV, long total)
{
    const long stride = (long)gridDim.x * TPB;
    for (long t = (long)blockIdx.x * TPB + threadIdx.x; t < total; t += stride) {
        const long p = t / HV;
        const long i = (t % HV) * 4;
        const rr_f32x4 *src = reinterpret_cast<const rr_f32x4 *>(g + p * gs + 2 * i);
        const rr_f32x4 lo = src[0], hi = src[1];
        const rr_f32x4 va = {lo[0], lo[2], hi[0], hi[2]};
        const rr_f32x4 vb = {lo[1], lo[3], hi[1], hi[3]};
        *reinterpret_cast<rr_f32x4 *>(da + p * as + i) = va;
        *reinterpret_cast<rr_f32x4 *>(db + p * bs + i) = vb;
    }
}

// dst[p, i] = src[p, i]; with a second source: dst[p, off2 + i] = src2[p, i] as well (the join)
__global__ __launch_bounds__(TPB) void channel_copy_kernel(const float *__restrict__ src, long ss, const float *__restrict__ src2,
                                                           long s2, float *__restrict__ dst, long ds, long off2, int HV, long total)
{
    const long stride = (long)gridDim.x * TPB;
    for (long t = (long)blockIdx.x * TPB + threadIdx.x; t < total; t += stride) {
        const long p = t / HV;
        const long i = (t % HV) * 4;
        *reinterpret_cast<rr_f32x4 *>(dst + p * ds + i) = *reinterpret_cast<const rr_f32x4 *>(src + p * ss + i);
        if (src2) *reinterpret_cast<rr_f32x4 *>(dst + p * ds + off2 + i) = *reinterpret_cast<const rr_f32x4 *>(src2 + p * s2 + i);
    }
}

inline int stream_blocks(long total) { return (int)std::min<long>((total + TPB - 1) / TPB, 256L * 16); }
inline bool aligned16(const void *p) { return reinterpret_cast<size_t>(p) % 16 == 0; }

// the shape rules the three depthwise entries share; P, Q: the output sizes
inline bool dw_dims_ok(int n, int h, int w, int c, int s, int *P, int *Q)
{
    if (!(n >= 1 && h >= 1 && w >= 1 && c >= 4 && c % 4 == 0 && (s == 1 || s == 2))) return false;
    *P = (h - 1) / s + 1;
    *Q = (w - 1) / s + 1;
    const long plane = (long)h * w;                                  // (three steps: none can leave 63 bits)
    return plane < MAX_BYTES && plane * n < MAX_BYTES && plane * n * c * 4 < MAX_BYTES;
}

// an operand of the shuffle family: [pixels, ch] floats at a pixel stride
inline bool operand_ok(const void *p, int stride, int ch, int pixels)
{
    return p && aligned16(p) && stride >= ch && stride % 4 == 0 && (long)pixels * stride * 4 < MAX_BYTES;
}

}  // namespace

#define DW_BAD "%s: bad arguments n=%d h=%d w=%d c=%d s=%d (non-null 16-byte aligned pointers; n, h, w >= 1; c %% 4 == 0; s 1 or 2; tensors under 2 GiB)"

extern "C" int rr_dwconv3x3_fwd(const float *x, const float *f, const float *bias, float *y, double *slab, int n, int h, int w,
                                int c, int s, hipStream_t stream)
{
    int P = 0, Q = 0;
    RR_CHECK_ARG(x && f && y && aligned16(x) && aligned16(f) && aligned16(y) && aligned16(bias) && dw_dims_ok(n, h, w, c, s, &P, &Q),
                 DW_BAD, "rr_dwconv3x3_fwd", n, h, w, c, s);
    const long pixels = (long)n * P * Q;
    const dim3 grid(rr_cdiv(pixels, SLAB_PIXELS), channel_groups(c));
#define DW_FWD(S, STATS) \
    hipLaunchKernelGGL((dw_fwd_kernel<S, STATS>), grid, dim3(TPB), 0, stream, x, f, bias, y, slab, h, w, P, Q, c, pixels)
    if (s == 1) {
        if (slab) DW_FWD(1, true); else DW_FWD(1, false);
    } else {
        if (slab) DW_FWD(2, true); else DW_FWD(2, false);
    }
#undef DW_FWD
    RR_CHECK_LAUNCH("rr_dwconv3x3_fwd");
    return RR_OK;
}

extern "C" int rr_dwconv3x3_bwd_data(const float *dy, const float *f, float *dx, int n, int h, int w, int c, int s,
                                     hipStream_t stream)
{
    int P = 0, Q = 0;
    RR_CHECK_ARG(dy && f && dx && aligned16(dy) && aligned16(f) && aligned16(dx) && dw_dims_ok(n, h, w, c, s, &P, &Q), DW_BAD,
                 "rr_dwconv3x3_bwd_data", n, h, w, c, s);
    const long total = (long)n * h * w * (c / 4);
    if (s == 1)
        hipLaunchKernelGGL(dw_bwd_data_kernel<1>, dim3(stream_blocks(total)), dim3(TPB), 0, stream, dy, f, dx, h, w, P, Q, c / 4, total);
    else
        hipLaunchKernelGGL(dw_bwd_data_kernel<2>, dim3(stream_blocks(total)), dim3(TPB), 0, stream, dy, f, dx, h, w, P, Q, c / 4, total);
    RR_CHECK_LAUNCH("rr_dwconv3x3_bwd_data");
    return RR_OK;
}

extern "C" int rr_dwconv3x3_bwd_weight(const float *x, const float *dy, double *partial, float *df, int accumulate, int n, int h,
                                       int w, int c, int s, int tile_pixels, hipStream_t stream)
{
    int P = 0, Q = 0;
    RR_CHECK_ARG(x && dy && partial && df && aligned16(x) && aligned16(dy) && dw_dims_ok(n, h, w, c, s, &P, &Q), DW_BAD,
                 "rr_dwconv3x3_bwd_weight", n, h, w, c, s);
    RR_CHECK_ARG(tile_pixels >= 1, "rr_dwconv3x3_bwd_weight: tile_pixels = %d", tile_pixels);
    const long pixels = (long)n * P * Q;
    const int tiles = rr_cdiv(pixels, tile_pixels);
    if (s == 1)
        hipLaunchKernelGGL(dw_wgrad_tile_kernel<1>, dim3(tiles, channel_groups(c)), dim3(TPB), 0, stream, x, dy, partial, h, w, P, Q, c, pixels, tile_pixels);
    else
        hipLaunchKernelGGL(dw_wgrad_tile_kernel<2>, dim3(tiles, channel_groups(c)), dim3(TPB), 0, stream, x, dy, partial, h, w, P, Q, c, pixels, tile_pixels);
    RR_CHECK_LAUNCH("rr_dwconv3x3_bwd_weight");
    hipLaunchKernelGGL(dw_wgrad_final_kernel, dim3(rr_cdiv(9L * c, TPB)), dim3(TPB), 0, stream, partial, df, tiles, 9 * c,
                       accumulate ? 1 : 0);
    RR_CHECK_LAUNCH("rr_dwconv3x3_bwd_weight");
    return RR_OK;
}

#define SH_BAD "%s: bad arguments pixels=%d half=%d strides %d %d %d (non-null 16-byte aligned pointers; pixels >= 1; half %% 4 == 0; every stride %% 4 == 0 and >= its channels; tensors under 2 GiB)"

extern "C" int rr_shuffle_interleave(const float *a, int a_stride, const float *b, int b_stride, float *out, int out_stride,
                                     int pixels, int half, hipStream_t stream)
{
    RR_CHECK_ARG(pixels >= 1 && half >= 4 && half % 4 == 0 && operand_ok(a, a_stride, half, pixels) &&
                     operand_ok(b, b_stride, half, pixels) && operand_ok(out, out_stride, 2 * half, pixels),
                 SH_BAD, "rr_shuffle_interleave", pixels, half, a_stride, b_stride, out_stride);
    const long total = (long)pixels * (half / 4);
    hipLaunchKernelGGL(interleave_kernel, dim3(stream_blocks(total)), dim3(TPB), 0, stream, a, (long)a_stride, b, (long)b_stride, out,
                       (long)out_stride, half / 4, total);
    RR_CHECK_LAUNCH("rr_shuffle_interleave");
    return RR_OK;
}

extern "C" int rr_shuffle_deinterleave(const float *g, int g_stride, float *da, int da_stride, float *db, int db_stride, int pixels,
                                       int half, hipStream_t stream)
{
    RR_CHECK_ARG(pixels >= 1 && half >= 4 && half % 4 == 0 && operand_ok(g, g_stride, 2 * half, pixels) &&
                     operand_ok(da, da_stride, half, pixels) && operand_ok(db, db_stride, half, pixels),
                 SH_BAD, "rr_shuffle_deinterleave", pixels, half, g_stride, da_stride, db_stride);
    const long total = (long)pixels * (half / 4);
    hipLaunchKernelGGL(deinterleave_kernel, dim3(stream_blocks(total)), dim3(TPB), 0, stream, g, (long)g_stride, da, (long)da_stride,
                       db, (long)db_stride, half / 4, total);
    RR_CHECK_LAUNCH("rr_shuffle_deinterleave");
    return RR_OK;
}

extern "C" int rr_channel_copy(const float *src, int src_stride, float *dst, int dst_stride, int pixels, int ch, hipStream_t stream)
{
    RR_CHECK_ARG(pixels >= 1 && ch >= 4 && ch % 4 == 0 && operand_ok(src, src_stride, ch, pixels) &&
                     operand_ok(dst, dst_stride, ch, pixels),
                 SH_BAD, "rr_channel_copy", pixels, ch, src_stride, dst_stride, 0);
    const long total = (long)pixels * (ch / 4);
    hipLaunchKernelGGL(channel_copy_kernel, dim3(stream_blocks(total)), dim3(TPB), 0, stream, src, (long)src_stride,
                       (const float *)nullptr, 0L, dst, (long)dst_stride, 0L, ch / 4, total);
    RR_CHECK_LAUNCH("rr_channel_copy");
    return RR_OK;
}

extern "C" int rr_channel_join(const float *lo, int lo_stride, const float *hi, int hi_stride, float *out, int out_stride,
                               int pixels, int half, hipStream_t stream)
{
    RR_CHECK_ARG(pixels >= 1 && half >= 4 && half % 4 == 0 && operand_ok(lo, lo_stride, half, pixels) &&
                     operand_ok(hi, hi_stride, half, pixels) && operand_ok(out, out_stride, 2 * half, pixels),
                 SH_BAD, "rr_channel_join", pixels, half, lo_stride, hi_stride, out_stride);
    const long total = (long)pixels * (half / 4);
    hipLaunchKernelGGL(channel_copy_kernel, dim3(stream_blocks(total)), dim3(TPB), 0, stream, lo, (long)lo_stride, hi, (long)hi_stride,
                       out, (long)out_stride, (long)half, half / 4, total);
    RR_CHECK_LAUNCH("rr_channel_join");
    return RR_OK;
}
