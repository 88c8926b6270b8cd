// rr_jitter_gray_mean: the one whole-frame quantity of ColorJitter (datasets/transforms/transforms.py:120-130,
// functional.py:159-174).  PIL's ImageEnhance.Contrast blends towards  m = int(mean(L) + 0.5)  of the frame it is given,
// which is the brightness-adjusted frame; everything else of the jitter is per pixel and rides on the tap reads of
// augment.hip / augment_paste.hip (jitter.h).  Two launches:
//   sum   grid (chunk, frame): every workgroup sums L over JIT_CHUNK pixels of one frame (brightness applied first), wave
//         shuffle -> LDS -> ONE 64-bit integer atomic per workgroup.  Integer addition commutes: the word does not
//         depend on the order of arrival.
//   mean  one thread per frame: m = (2*S + N) / (2*N) in 64-bit integers, which equals int(S/N + 0.5) of PIL's double
//         expression (S/N is either a half exactly or at least 1/(2N) away from one, far above double rounding).
// Frames sit back to back at any byte offset and a pixel is three bytes, so a group of four pixels (12 bytes) is read as
// the aligned dwords that cover it and shifted into place; a group whose covering dwords would leave [src, src+src_bytes)
// or that is the ragged end of its frame is read byte by byte.  This file is compiled with -ffp-contract=off.
#include "common.h"
#include "rrnet_hip.h"
#include "jitter.h"

#define JIT_THREADS 256
#define JIT_GROUPS 4                                  // groups of four pixels per thread
#define JIT_CHUNK (JIT_THREADS * JIT_GROUPS * 4)      // pixels per workgroup

// int32 fields of the per-image record (RR_AUGMENT_PARAMS of them), as in augment.hip
enum { P_SRC_H, P_SRC_W, P_WIN_Y0, P_WIN_X0, P_WIN_H, P_WIN_W, P_DST_H, P_DST_W, P_FLIP, P_CROP_Y0, P_CROP_X0, P_OFF_LO,
       P_OFF_HI, P_YTAB, P_XTAB, P_RESERVED };

__device__ __forceinline__ int jit_gray_of(int r, int g, int b, float fb)
{
    jit_brightness(r, g, b, fb);
    return jit_gray(r, g, b);
}

__global__ __launch_bounds__(JIT_THREADS) void jitter_gray_sum_kernel(
    const uint8_t *__restrict__ src, long src_bytes, const int *__restrict__ params, const float *__restrict__ factors,
    unsigned long long *__restrict__ sums)
{
    __shared__ int part[JIT_THREADS / 64];
    const int b = blockIdx.y;
    const int *P = params + (long)b * RR_AUGMENT_PARAMS;
    const int win_h = P[P_WIN_H], win_w = P[P_WIN_W];
    const long n = (long)win_h * win_w;
    const long c0 = (long)blockIdx.x * JIT_CHUNK;
    if (win_h <= 0 || win_w <= 0 || c0 >= n) return;         // uniform over the workgroup
    const long base = ((long)(unsigned)P[P_OFF_LO]) | ((long)P[P_OFF_HI] << 32);
    const long last = src_bytes - 3;
    const float fb = factors[(long)b * 3];
    int acc = 0;                                             // at most 16 pixels of at most 255 each
#pragma unroll
    for (int it = 0; it < JIT_GROUPS; ++it) {
        const long p = c0 + ((long)it * JIT_THREADS + threadIdx.x) * 4;
        if (p < n) {
            const long a = base + p * 3;
            bool wide = n - p >= 4 && a >= 0 && a + 12 <= src_bytes;
            const size_t u = reinterpret_cast<size_t>(src + (wide ? a : 0));
            const unsigned sh = (unsigned)(u & 3) * 8;
            const uint8_t *w8 = reinterpret_cast<const uint8_t *>(u & ~(size_t)3);
            // the covering dwords: three when the group is aligned, four otherwise; all of them inside the buffer?
            wide = wide && w8 >= src && w8 + (sh ? 16 : 12) <= src + src_bytes;
            if (wide) {
                const uint32_t *w = reinterpret_cast<const uint32_t *>(w8);
                const uint64_t d0 = w[0], d1 = w[1], d2 = w[2], d3 = sh ? w[3] : 0u;
                const uint32_t e0 = (uint32_t)(((d1 << 32) | d0) >> sh);
                const uint32_t e1 = (uint32_t)(((d2 << 32) | d1) >> sh);
                const uint32_t e2 = (uint32_t)(((d3 << 32) | d2) >> sh);
                acc += jit_gray_of(e0 & 255, (e0 >> 8) & 255, (e0 >> 16) & 255, fb);
                acc += jit_gray_of(e0 >> 24, e1 & 255, (e1 >> 8) & 255, fb);
                acc += jit_gray_of((e1 >> 16) & 255, e1 >> 24, e2 & 255, fb);
                acc += jit_gray_of((e2 >> 8) & 255, (e2 >> 16) & 255, e2 >> 24, fb);
            } else {
                for (int k = 0; k < 4 && p + k < n; ++k) {
                    long ak = a + (long)k * 3;
                    ak = ak < 0 ? 0 : (ak > last ? last : ak);
                    acc += jit_gray_of(src[ak], src[ak + 1], src[ak + 2], fb);
                }
            }
        }
    }
    acc = wave_sum_i(acc);                                   // 64 * 16 * 255 fits an int with room
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
#pragma unroll
        for (int i = 0; i < JIT_THREADS / 64; ++i) s += part[i];
        atomicAdd(sums + b, (unsigned long long)s);
    }
}

__global__ __launch_bounds__(JIT_THREADS) void jitter_gray_mean_kernel(
    const int *__restrict__ params, const unsigned long long *__restrict__ sums, int *__restrict__ gray_mean, int b)
{
    const int i = blockIdx.x * JIT_THREADS + threadIdx.x;
    if (i >= b) return;
    const int *P = params + (long)i * RR_AUGMENT_PARAMS;
    const int win_h = P[P_WIN_H], win_w = P[P_WIN_W];
    int m = 0;
    if (win_h > 0 && win_w > 0) {
        const unsigned long long n = (unsigned long long)win_h * (unsigned long long)win_w;
        const unsigned long long q = (2ull * sums[i] + n) / (2ull * n);    // one 64-bit division per FRAME
        m = q > 255ull ? 255 : (int)q;
    }
    gray_mean[i] = m;
}

extern "C" int rr_jitter_gray_mean(const unsigned char *src, long src_bytes, const int *params, const float *factors,
                                   unsigned long long *sums, int *gray_mean, int b, long max_pixels, hipStream_t stream)
{
    RR_CHECK_ARG(b > 0 && b <= 65535 && src_bytes >= 3 && max_pixels > 0, "rr_jitter_gray_mean: bad dims");
    RR_CHECK_ARG(src && params && factors && sums && gray_mean, "rr_jitter_gray_mean: null pointer");
    RR_CHECK_ARG((reinterpret_cast<size_t>(sums) & 7) == 0, "rr_jitter_gray_mean: sums must be 8-byte aligned");
    const long chunks = (max_pixels + JIT_CHUNK - 1) / JIT_CHUNK;
    RR_CHECK_ARG(chunks <= 0x7fffffffL, "rr_jitter_gray_mean: frame too large");
    RR_CHECK_HIP(hipMemsetAsync(sums, 0, (size_t)b * sizeof(unsigned long long), stream), "rr_jitter_gray_mean");
    hipLaunchKernelGGL(jitter_gray_sum_kernel, dim3((unsigned)chunks, (unsigned)b), dim3(JIT_THREADS), 0, stream, src,
                       src_bytes, params, factors, sums);
    RR_CHECK_LAUNCH("rr_jitter_gray_mean (sum)");
    hipLaunchKernelGGL(jitter_gray_mean_kernel, dim3((unsigned)((b + JIT_THREADS - 1) / JIT_THREADS)), dim3(JIT_THREADS), 0,
                       stream, params, sums, gray_mean, b);
    RR_CHECK_LAUNCH("rr_jitter_gray_mean (mean)");
    return RR_OK;
}
