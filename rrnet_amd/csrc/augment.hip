// rr_augment_frames: the pixel half of the training chain of configs/rrnet_config.py:40-49 (MultiScale -> ToTensor ->
// MaskIgnore -> HorizontalFlip -> RandomCrop -> Normalize; frames FillDuck pastes into go through augment_paste.hip) as ONE
// gather per output pixel.  The host decodes the JPEG and decides (scale, flip, crop origin); this kernel reads the uint8
// source window and writes the normalised fp32 NHWC network input.  Bit-exact with the host chain:
//   * PIL's 8-bit bilinear resize is two separable fixed-point passes (Resample.c): horizontal first, rounded to uint8,
//     then vertical; an up-scale has at most two taps per output coordinate.  The per-axis tables (first tap, k0, k1)
//     come from the host (datasets/transforms/functional.py pil_bilinear_taps), so the kernel does integer work only.
//   * uint8 -> /255 -> (x - mean) / std has 256 x 3 possible results: a table in LDS built with the same three float32
//     operations torch performs (this file is compiled with -ffp-contract=off; fp32 division is correctly rounded).
// Order per pixel (datasets/transforms/transforms.py:60-72, functional.py:290-313): crop -> padding (0, normalised; the
// reference pads right/bottom after the flip and before Normalize) -> un-flip -> ignore rectangle (mean, normalised:
// +0.0) -> bilinear sample.
// rr_augment_frames_jitter is the same gather with ColorJitter (jitter.h) applied to each of the four source taps before
// the resize: the jitter is the first transform of the chain, so the resize reads jittered uint8 pixels.  It is a second
// instantiation of the same body; the unjittered kernel compiles to what it was without it.
#include "common.h"
#include "rrnet_hip.h"
#include "jitter.h"
#include "rowkit.h"

#define AUG_THREADS 256
#define AUG_PIX 4                 // pixels per thread: 12 floats = three 16-byte stores
#define AUG_PREC 22               // PIL's PRECISION_BITS for 8-bit channels

// int32 fields of the per-image record (RR_AUGMENT_PARAMS of them)
enum { P_SRC_H, P_SRC_W, P_WIN_Y0, P_WIN_X0, P_WIN_H, P_WIN_W, P_DST_H, P_DST_W, P_FLIP, P_CROP_Y0, P_CROP_X0, P_OFF_LO,
       P_OFF_HI, P_YTAB, P_XTAB, P_RESERVED };

__device__ __forceinline__ int aug_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int aug_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// one jittered source tap
__device__ __forceinline__ void aug_tap(const uint8_t *__restrict__ src, long a, float fb, float fc, float fs, int m, int *t)
{
    t[0] = src[a], t[1] = src[a + 1], t[2] = src[a + 2];
    jit_pixel(t[0], t[1], t[2], fb, fc, fs, m);
}

// what the jittered instantiation takes on top: nothing in the unjittered one, whose arguments stay what they were
template <bool JIT> struct AugJitter {};
template <> struct AugJitter<true> {
    const float *factors;          // [b,3] brightness, contrast, colour
    const int *gray_mean;          // [b] rr_jitter_gray_mean
};

template <bool JIT>
__global__ __launch_bounds__(AUG_THREADS) void augment_frames_kernel(
    const uint8_t *__restrict__ src, long src_bytes, const int *__restrict__ params, const int *__restrict__ rects,
    const int *__restrict__ rect_off, const int *__restrict__ taps, int ntaps, const float *__restrict__ mean,
    const float *__restrict__ stdv, float *__restrict__ out, long npix, int OH, int OW, AugJitter<JIT> jit)
{
    __shared__ float lut[256 * 3];                       // lut[v*3 + c]
    rr_norm_lut_fill<AUG_THREADS>(lut, mean, stdv);
    const long p0 = ((long)blockIdx.x * AUG_THREADS + threadIdx.x) * AUG_PIX;
    if (p0 >= npix) return;
    const long per_img = (long)OH * OW;
    float vals[AUG_PIX * 3];
#pragma unroll
    for (int k = 0; k < AUG_PIX; ++k) {
        const long p = p0 + k;
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
        if (p < npix) {
            const int b = (int)(p / per_img);
            const int rem = (int)(p - (long)b * per_img);
            const int oy = rem / OW, ox = rem - oy * OW;
            const int *P = params + (long)b * RR_AUGMENT_PARAMS;
            const int dst_h = P[P_DST_H], dst_w = P[P_DST_W];
            const int sy = P[P_CROP_Y0] + oy, sxp = P[P_CROP_X0] + ox;
            if (sy >= dst_h || sxp >= dst_w) {           // padding: 0, normalised
                r0 = lut[0], r1 = lut[1], r2 = lut[2];
            } else {
                const int sx = P[P_FLIP] ? dst_w - 1 - sxp : sxp;
                bool ign = false;
                for (int r = rect_off[b]; r < rect_off[b + 1]; ++r) {
                    const int *R = rects + (long)r * 4;  // y0, y1, x0, x1 (half-open, scaled pre-flip coordinates)
                    ign |= (sy >= R[0]) & (sy < R[1]) & (sx >= R[2]) & (sx < R[3]);
                }
                if (!ign) {                              // ignore region: (mean - mean) / std = +0.0
                    const int win_h = P[P_WIN_H], win_w = P[P_WIN_W];
                    const int *ty = taps + (long)aug_clampi(P[P_YTAB] + sy, 0, ntaps - 1) * 3;
                    const int *tx = taps + (long)aug_clampi(P[P_XTAB] + sx, 0, ntaps - 1) * 3;
                    const int ky0 = ty[1], ky1 = ty[2], kx0 = tx[1], kx1 = tx[2];
                    // the second tap of a one-tap row/column has weight 0; the clamp keeps its address inside the window
                    const int y0 = aug_clampi(ty[0] - P[P_WIN_Y0], 0, win_h - 1);
                    const int y1 = aug_clampi(ty[0] + 1 - P[P_WIN_Y0], 0, win_h - 1);
                    const int x0 = aug_clampi(tx[0] - P[P_WIN_X0], 0, win_w - 1);
                    const int x1 = aug_clampi(tx[0] + 1 - P[P_WIN_X0], 0, win_w - 1);
                    const long base = ((long)(unsigned)P[P_OFF_LO]) | ((long)P[P_OFF_HI] << 32);
                    long a00 = base + ((long)y0 * win_w + x0) * 3, a01 = base + ((long)y0 * win_w + x1) * 3;
                    long a10 = base + ((long)y1 * win_w + x0) * 3, a11 = base + ((long)y1 * win_w + x1) * 3;
                    const long last = src_bytes - 3;
                    a00 = a00 < 0 ? 0 : (a00 > last ? last : a00);
                    a01 = a01 < 0 ? 0 : (a01 > last ? last : a01);
                    a10 = a10 < 0 ? 0 : (a10 > last ? last : a10);
                    a11 = a11 < 0 ? 0 : (a11 > last ? last : a11);
                    int v[3];
                    if constexpr (!JIT) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const int h0 = aug_clip8(((int)src[a00 + c] * kx0 + (int)src[a01 + c] * kx1 + (1 << (AUG_PREC - 1))) >> AUG_PREC);
                            const int h1 = aug_clip8(((int)src[a10 + c] * kx0 + (int)src[a11 + c] * kx1 + (1 << (AUG_PREC - 1))) >> AUG_PREC);
                            v[c] = aug_clip8((h0 * ky0 + h1 * ky1 + (1 << (AUG_PREC - 1))) >> AUG_PREC);
                        }
                    } else {                             // the same resize on jittered taps
                        const float *f = jit.factors + (long)b * 3;
                        const float fb = f[0], fc = f[1], fs = f[2];
                        const int gm = aug_clampi(jit.gray_mean[b], 0, 255);
                        int t00[3], t01[3], t10[3], t11[3];
                        aug_tap(src, a00, fb, fc, fs, gm, t00);
                        aug_tap(src, a01, fb, fc, fs, gm, t01);
                        aug_tap(src, a10, fb, fc, fs, gm, t10);
                        aug_tap(src, a11, fb, fc, fs, gm, t11);
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const int h0 = aug_clip8((t00[c] * kx0 + t01[c] * kx1 + (1 << (AUG_PREC - 1))) >> AUG_PREC);
                            const int h1 = aug_clip8((t10[c] * kx0 + t11[c] * kx1 + (1 << (AUG_PREC - 1))) >> AUG_PREC);
                            v[c] = aug_clip8((h0 * ky0 + h1 * ky1 + (1 << (AUG_PREC - 1))) >> AUG_PREC);
                        }
                    }
                    r0 = lut[v[0] * 3], r1 = lut[v[1] * 3 + 1], r2 = lut[v[2] * 3 + 2];
                }
            }
        }
        vals[k * 3] = r0, vals[k * 3 + 1] = r1, vals[k * 3 + 2] = r2;
    }
    float *o = out + p0 * 3;
    if (p0 + AUG_PIX <= npix) {                          // p0 is a multiple of 4 pixels = 48 bytes: 16-byte aligned
        rr_f32x4 *o4 = reinterpret_cast<rr_f32x4 *>(o);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            rr_f32x4 w = {vals[q * 4], vals[q * 4 + 1], vals[q * 4 + 2], vals[q * 4 + 3]};
            o4[q] = w;
        }
    } else {
        for (long i = 0; i < (npix - p0) * 3; ++i) o[i] = vals[i];
    }
}

extern "C" int rr_augment_frames(const unsigned char *src, long src_bytes, const int *params, const int *rects,
                                 const int *rect_off, const int *taps, int ntaps, const float *mean, const float *stdv,
                                 float *out, int b, int out_h, int out_w, hipStream_t stream)
{
    RR_CHECK_ARG(b > 0 && out_h > 0 && out_w > 0 && src_bytes >= 3 && ntaps > 0, "rr_augment_frames: bad dims");
    RR_CHECK_ARG(src && params && rect_off && taps && mean && stdv && out, "rr_augment_frames: null pointer");
    RR_CHECK_ARG((reinterpret_cast<size_t>(out) & 15) == 0, "rr_augment_frames: out must be 16-byte aligned");
    const long npix = (long)b * out_h * out_w;
    const long blocks = (npix + (long)AUG_THREADS * AUG_PIX - 1) / ((long)AUG_THREADS * AUG_PIX);
    RR_CHECK_ARG(blocks <= 0x7fffffffL, "rr_augment_frames: too many pixels");
    hipLaunchKernelGGL(augment_frames_kernel<false>, dim3((unsigned)blocks), dim3(AUG_THREADS), 0, stream, src, src_bytes,
                       params, rects, rect_off, taps, ntaps, mean, stdv, out, npix, out_h, out_w, AugJitter<false>{});
    RR_CHECK_LAUNCH("rr_augment_frames");
    return RR_OK;
}

extern "C" int rr_augment_frames_jitter(const unsigned char *src, long src_bytes, const int *params, const int *rects,
                                        const int *rect_off, const int *taps, int ntaps, const float *mean,
                                        const float *stdv, const float *factors, const int *gray_mean, float *out, int b,
                                        int out_h, int out_w, hipStream_t stream)
{
    RR_CHECK_ARG(b > 0 && out_h > 0 && out_w > 0 && src_bytes >= 3 && ntaps > 0, "rr_augment_frames_jitter: bad dims");
    RR_CHECK_ARG(src && params && rect_off && taps && mean && stdv && factors && gray_mean && out,
                 "rr_augment_frames_jitter: null pointer");
    RR_CHECK_ARG((reinterpret_cast<size_t>(out) & 15) == 0, "rr_augment_frames_jitter: out must be 16-byte aligned");
    const long npix = (long)b * out_h * out_w;
    const long blocks = (npix + (long)AUG_THREADS * AUG_PIX - 1) / ((long)AUG_THREADS * AUG_PIX);
    RR_CHECK_ARG(blocks <= 0x7fffffffL, "rr_augment_frames_jitter: too many pixels");
    hipLaunchKernelGGL(augment_frames_kernel<true>, dim3((unsigned)blocks), dim3(AUG_THREADS), 0, stream, src, src_bytes,
                       params, rects, rect_off, taps, ntaps, mean, stdv, out, npix, out_h, out_w,
                       AugJitter<true>{factors, gray_mean});
    RR_CHECK_LAUNCH("rr_augment_frames_jitter");
    return RR_OK;
}
