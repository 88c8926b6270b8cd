// rr_augment_frames_pasted: the pixel half of the FULL training chain of configs/rrnet_config.py:40-49 (MultiScale ->
// ToTensor -> MaskIgnore -> FillDuck -> HorizontalFlip -> RandomCrop -> Normalize) for frames that FillDuck pastes into.
// FillDuck (datasets/transforms/functional.py:356-523) copies objects inside the scaled, masked, un-flipped frame, so the
// one-gather form of rr_augment_frames (augment.hip) does not hold: a pasted pixel depends on a rectangle of other
// pixels, possibly on earlier pastes.  Three stages on a float canvas in HBM:
//   canvas  the scaled frame as fp32 NHWC, (float)v / 255.0f from PIL's fixed-point two-tap resize (the same integer
//           work as augment.hip), the float32 mean inside ignore rectangles; no flip, no normalisation.  A frame
//           without pastes gets only the pixels its crop reads.
//   paste   one workgroup per frame walks the frame's paste list in order.  Each paste is torch's
//           upsample_bilinear2d(align_corners=True) of the source rectangle (functional.py:440-445), staged in a
//           per-frame scratch and copied to the destination rectangle after a workgroup barrier: all reads of a paste
//           come before any of its writes (source and destination may overlap), and a later paste sees what earlier
//           ones wrote.
//   finish  crop origin, right/bottom padding with 0, un-flip, (x - mean) / std.
// This file is compiled with -ffp-contract=off.  Unpasted pixels go through exactly the three float32 operations of
// augment.hip's table ((float)v / 255.0f, subtract, correctly rounded divide) and are bit-identical to it.  A pasted
// pixel is  l0*(m0*a + m1*b) + l1*(m0*c + m1*d)  with r = rheight*(float)oy, y0 = (int)r, l1 = r - y0, l0 = 1 - l1
// (likewise along x): torch's source indices exactly, its value within float32 rounding of the blend.
// Every address is clamped into the frame's canvas / scratch slab; a record that does not fit its slab is skipped.
// rr_augment_frames_pasted_jitter: the canvas stage, the one place that reads src, applies ColorJitter (jitter.h) to each
// source tap before the resize; pasted objects then read the jittered canvas, as the reference's order implies.  The
// unjittered canvas kernel compiles to what it was without it.
#include "common.h"
#include "rrnet_hip.h"
#include "jitter.h"

#define AUG_THREADS 256
#define AUG_PIX 4                 // pixels per thread: 12 floats = three 16-byte stores
#define AUG_PREC 22               // PIL's PRECISION_BITS for 8-bit channels
#define PASTE_THREADS 1024

// int32 fields of the per-image record (RR_AUGMENT_PARAMS of them), as in augment.hip
enum { P_SRC_H, P_SRC_W, P_WIN_Y0, P_WIN_X0, P_WIN_H, P_WIN_W, P_DST_H, P_DST_W, P_FLIP, P_CROP_Y0, P_CROP_X0, P_OFF_LO,
       P_OFF_HI, P_YTAB, P_XTAB, P_RESERVED };
// int32 fields of one paste (RR_PASTE_WORDS of them)
enum { T_SRC_Y, T_SRC_X, T_SRC_H, T_SRC_W, T_DST_Y, T_DST_X, T_OUT_H, T_OUT_W, T_RHEIGHT, T_RWIDTH };

__device__ __forceinline__ int pst_clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ int pst_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ bool pst_frame_fits(const int *P, long canvas_stride)
{
    return P[P_DST_H] > 0 && P[P_DST_W] > 0 && (long)P[P_DST_H] * P[P_DST_W] <= canvas_stride;
}

// one jittered source tap
__device__ __forceinline__ void pst_tap(const uint8_t *__restrict__ src, long a, float fb, float fc, float fs, int m, int *t)
{
    t[0] = src[a], t[1] = src[a + 1], t[2] = src[a + 2];
    jit_pixel(t[0], t[1], t[2], fb, fc, fs, m);
}

// what the jittered instantiation takes on top: nothing in the unjittered one, whose arguments stay what they were
template <bool JIT> struct PstJitter {};
template <> struct PstJitter<true> {
    const float *factors;          // [b,3] brightness, contrast, colour
    const int *gray_mean;          // [b] rr_jitter_gray_mean
};

template <bool JIT>
__global__ __launch_bounds__(AUG_THREADS) void paste_canvas_kernel(
    const uint8_t *__restrict__ src, long src_bytes, const int *__restrict__ params, const int *__restrict__ rects,
    const int *__restrict__ rect_off, const int *__restrict__ taps, int ntaps, const int *__restrict__ paste_off,
    const float *__restrict__ mean, float *__restrict__ canvas, long canvas_stride, int OH, int OW, PstJitter<JIT> jit)
{
    const int b = blockIdx.y;
    const int *P = params + (long)b * RR_AUGMENT_PARAMS;
    if (!pst_frame_fits(P, canvas_stride)) return;
    const int dst_h = P[P_DST_H], dst_w = P[P_DST_W];
    const long npix = (long)dst_h * dst_w;
    const long p0 = ((long)blockIdx.x * AUG_THREADS + threadIdx.x) * AUG_PIX;
    if (p0 >= npix) return;
    const bool whole = paste_off[b + 1] > paste_off[b];     // a pasted frame may read any pixel of its canvas
    const int flip = P[P_FLIP], cy0 = P[P_CROP_Y0], cx0 = P[P_CROP_X0];
    const int win_h = P[P_WIN_H], win_w = P[P_WIN_W];
    const long base = ((long)(unsigned)P[P_OFF_LO]) | ((long)P[P_OFF_HI] << 32);
    const long last = src_bytes - 3;
    float vals[AUG_PIX * 3];
    bool any = false;
#pragma unroll
    for (int k = 0; k < AUG_PIX; ++k) {
        const long p = p0 + k;
        float r0 = 0.f, r1 = 0.f, r2 = 0.f;
        if (p < npix) {
            const int sy = (int)(p / dst_w), sx = (int)(p - (long)sy * dst_w);
            const int sxp = flip ? dst_w - 1 - sx : sx;    // the column of the flipped frame this pixel lands in
            const bool need = whole || (sy >= cy0 && sy < cy0 + OH && sxp >= cx0 && sxp < cx0 + OW);
            if (need) {
                any = true;
                bool ign = false;
                for (int r = rect_off[b]; r < rect_off[b + 1]; ++r) {
                    const int *R = rects + (long)r * 4;     // y0, y1, x0, x1 (half-open, scaled pre-flip coordinates)
                    ign |= (sy >= R[0]) & (sy < R[1]) & (sx >= R[2]) & (sx < R[3]);
                }
                if (ign) {                                  // MaskIgnore writes the float32 mean
                    r0 = mean[0], r1 = mean[1], r2 = mean[2];
                } else {
                    const int *ty = taps + (long)pst_clampi(P[P_YTAB] + sy, 0, ntaps - 1) * 3;
                    const int *tx = taps + (long)pst_clampi(P[P_XTAB] + sx, 0, ntaps - 1) * 3;
                    const int ky0 = ty[1], ky1 = ty[2], kx0 = tx[1], kx1 = tx[2];
                    const int y0 = pst_clampi(ty[0] - P[P_WIN_Y0], 0, win_h - 1);
                    const int y1 = pst_clampi(ty[0] + 1 - P[P_WIN_Y0], 0, win_h - 1);
                    const int x0 = pst_clampi(tx[0] - P[P_WIN_X0], 0, win_w - 1);
                    const int x1 = pst_clampi(tx[0] + 1 - P[P_WIN_X0], 0, win_w - 1);
                    long a00 = base + ((long)y0 * win_w + x0) * 3, a01 = base + ((long)y0 * win_w + x1) * 3;
                    long a10 = base + ((long)y1 * win_w + x0) * 3, a11 = base + ((long)y1 * win_w + x1) * 3;
                    a00 = a00 < 0 ? 0 : (a00 > last ? last : a00);
                    a01 = a01 < 0 ? 0 : (a01 > last ? last : a01);
                    a10 = a10 < 0 ? 0 : (a10 > last ? last : a10);
                    a11 = a11 < 0 ? 0 : (a11 > last ? last : a11);
                    float v[3];
                    if constexpr (!JIT) {
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const int h0 = pst_clip8(((int)src[a00 + c] * kx0 + (int)src[a01 + c] * kx1 + (1 << (AUG_PREC - 1))) >> AUG_PREC);
                            const int h1 = pst_clip8(((int)src[a10 + c] * kx0 + (int)src[a11 + c] * kx1 + (1 << (AUG_PREC - 1))) >> AUG_PREC);
                            v[c] = (float)pst_clip8((h0 * ky0 + h1 * ky1 + (1 << (AUG_PREC - 1))) >> AUG_PREC) / 255.0f;
                        }
                    } else {                                // the same resize on jittered taps
                        const float *f = jit.factors + (long)b * 3;
                        const float fb = f[0], fc = f[1], fs = f[2];
                        const int gm = pst_clampi(jit.gray_mean[b], 0, 255);
                        int t00[3], t01[3], t10[3], t11[3];
                        pst_tap(src, a00, fb, fc, fs, gm, t00);
                        pst_tap(src, a01, fb, fc, fs, gm, t01);
                        pst_tap(src, a10, fb, fc, fs, gm, t10);
                        pst_tap(src, a11, fb, fc, fs, gm, t11);
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            const int h0 = pst_clip8((t00[c] * kx0 + t01[c] * kx1 + (1 << (AUG_PREC - 1))) >> AUG_PREC);
                            const int h1 = pst_clip8((t10[c] * kx0 + t11[c] * kx1 + (1 << (AUG_PREC - 1))) >> AUG_PREC);
                            v[c] = (float)pst_clip8((h0 * ky0 + h1 * ky1 + (1 << (AUG_PREC - 1))) >> AUG_PREC) / 255.0f;
                        }
                    }
                    r0 = v[0], r1 = v[1], r2 = v[2];
                }
            }
        }
        vals[k * 3] = r0, vals[k * 3 + 1] = r1, vals[k * 3 + 2] = r2;
    }
    if (!any) return;
    float *o = canvas + ((long)b * canvas_stride + p0) * 3;  // canvas_stride is a multiple of 4 pixels: 16-byte aligned
    if (p0 + AUG_PIX <= npix) {
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

__global__ __launch_bounds__(PASTE_THREADS) void paste_objects_kernel(
    const int *__restrict__ params, const int *__restrict__ pastes, const int *__restrict__ paste_off, float *canvas,
    long canvas_stride, float *scratch, long scratch_stride)
{
    const int b = blockIdx.x;
    const int *P = params + (long)b * RR_AUGMENT_PARAMS;
    if (!pst_frame_fits(P, canvas_stride)) return;          // uniform over the workgroup, like every exit below
    const int dst_h = P[P_DST_H], dst_w = P[P_DST_W];
    float *cv = canvas + (long)b * canvas_stride * 3;
    float *sc = scratch + (long)b * scratch_stride * 3;
    for (int k = paste_off[b]; k < paste_off[b + 1]; ++k) {
        const int *T = pastes + (long)k * RR_PASTE_WORDS;
        const int sy = T[T_SRC_Y], sx = T[T_SRC_X], sh = T[T_SRC_H], sw = T[T_SRC_W];
        const int dy = T[T_DST_Y], dx = T[T_DST_X], oh = T[T_OUT_H], ow = T[T_OUT_W];
        if (sh <= 0 || sw <= 0 || oh <= 0 || ow <= 0) continue;
        const long n = (long)oh * ow;
        if (n > scratch_stride) continue;
        const float rheight = __int_as_float(T[T_RHEIGHT]), rwidth = __int_as_float(T[T_RWIDTH]);
        // read phase: the resized object, from the canvas as the earlier pastes left it
        for (long i = threadIdx.x; i < n; i += PASTE_THREADS) {
            const int oy = (int)(i / ow), ox = (int)(i - (long)oy * ow);
            const float r = rheight * (float)oy, c = rwidth * (float)ox;
            int y0 = (int)r, x0 = (int)c;
            y0 = y0 > sh - 1 ? sh - 1 : y0;
            x0 = x0 > sw - 1 ? sw - 1 : x0;
            const int y1 = y0 + 1 > sh - 1 ? sh - 1 : y0 + 1;
            const int x1 = x0 + 1 > sw - 1 ? sw - 1 : x0 + 1;
            const float l1 = r - (float)y0, l0 = 1.0f - l1;
            const float m1 = c - (float)x0, m0 = 1.0f - m1;
            const long ry0 = (long)pst_clampi(sy + y0, 0, dst_h - 1) * dst_w, ry1 = (long)pst_clampi(sy + y1, 0, dst_h - 1) * dst_w;
            const int cx0 = pst_clampi(sx + x0, 0, dst_w - 1), cx1 = pst_clampi(sx + x1, 0, dst_w - 1);
            const float *pa = cv + (ry0 + cx0) * 3, *pb = cv + (ry0 + cx1) * 3;
            const float *pc = cv + (ry1 + cx0) * 3, *pd = cv + (ry1 + cx1) * 3;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                sc[i * 3 + ch] = l0 * (m0 * pa[ch] + m1 * pb[ch]) + l1 * (m0 * pc[ch] + m1 * pd[ch]);
        }
        __syncthreads();                                    // every read of this paste precedes every write of it
        for (long i = threadIdx.x; i < n; i += PASTE_THREADS) {
            const int oy = (int)(i / ow), ox = (int)(i - (long)oy * ow);
            const int y = dy + oy, x = dx + ox;
            if (y >= 0 && y < dst_h && x >= 0 && x < dst_w) {
                float *o = cv + ((long)y * dst_w + x) * 3;
                o[0] = sc[i * 3], o[1] = sc[i * 3 + 1], o[2] = sc[i * 3 + 2];
            }
        }
        __syncthreads();                                    // the next paste may read what this one wrote
    }
}

__global__ __launch_bounds__(AUG_THREADS) void paste_finish_kernel(
    const int *__restrict__ params, const float *__restrict__ canvas, long canvas_stride, const float *__restrict__ mean,
    const float *__restrict__ stdv, float *__restrict__ out, long npix, int OH, int OW)
{
    const long p0 = ((long)blockIdx.x * AUG_THREADS + threadIdx.x) * AUG_PIX;
    if (p0 >= npix) return;
    const long per_img = (long)OH * OW;
    const float m0 = mean[0], m1 = mean[1], m2 = mean[2], s0 = stdv[0], s1 = stdv[1], s2 = stdv[2];
    float vals[AUG_PIX * 3];
#pragma unroll
    for (int k = 0; k < AUG_PIX; ++k) {
        const long p = p0 + k;
        float x0 = 0.f, x1 = 0.f, x2 = 0.f;                 // padding: 0 before Normalize
        if (p < npix) {
            const int b = (int)(p / per_img);
            const int rem = (int)(p - (long)b * per_img);
            const int oy = rem / OW, ox = rem - oy * OW;
            const int *P = params + (long)b * RR_AUGMENT_PARAMS;
            const int dst_h = P[P_DST_H], dst_w = P[P_DST_W];
            const int sy = P[P_CROP_Y0] + oy, sxp = P[P_CROP_X0] + ox;
            if (sy >= 0 && sxp >= 0 && sy < dst_h && sxp < dst_w && pst_frame_fits(P, canvas_stride)) {
                const int sx = P[P_FLIP] ? dst_w - 1 - sxp : sxp;
                const float *c = canvas + ((long)b * canvas_stride + (long)sy * dst_w + sx) * 3;
                x0 = c[0], x1 = c[1], x2 = c[2];
            }
        }
        vals[k * 3] = (x0 - m0) / s0, vals[k * 3 + 1] = (x1 - m1) / s1, vals[k * 3 + 2] = (x2 - m2) / s2;
    }
    float *o = out + p0 * 3;
    if (p0 + AUG_PIX <= npix) {                              // p0 is a multiple of 4 pixels = 48 bytes: 16-byte aligned
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

// both entry points: factors == nullptr is the unjittered chain
static int augment_frames_pasted(const unsigned char *src, long src_bytes, const int *params, const int *rects,
                                 const int *rect_off, const int *taps, int ntaps, const int *pastes, const int *paste_off,
                                 const float *mean, const float *stdv, const float *factors, const int *gray_mean,
                                 float *canvas, long canvas_stride, float *scratch, long scratch_stride, float *out, int b,
                                 int out_h, int out_w, int stages, hipStream_t stream)
{
    RR_CHECK_ARG(b > 0 && out_h > 0 && out_w > 0 && src_bytes >= 3 && ntaps > 0, "rr_augment_frames_pasted: bad dims");
    RR_CHECK_ARG(src && params && rect_off && taps && pastes && paste_off && mean && stdv && canvas && scratch && out,
                 "rr_augment_frames_pasted: null pointer");
    RR_CHECK_ARG(canvas_stride > 0 && (canvas_stride & 3) == 0 && scratch_stride > 0,
                 "rr_augment_frames_pasted: canvas_stride must be a positive multiple of 4 pixels, scratch_stride positive");
    RR_CHECK_ARG((reinterpret_cast<size_t>(out) & 15) == 0 && (reinterpret_cast<size_t>(canvas) & 15) == 0,
                 "rr_augment_frames_pasted: out and canvas must be 16-byte aligned");
    RR_CHECK_ARG(stages > 0 && stages < 8, "rr_augment_frames_pasted: stages is a mask of 1 (canvas), 2 (paste), 4 (finish)");
    const long per_block = (long)AUG_THREADS * AUG_PIX;
    if (stages & 1) {
        const long blocks = (canvas_stride + per_block - 1) / per_block;
        RR_CHECK_ARG(blocks <= 0x7fffffffL && b <= 65535, "rr_augment_frames_pasted: canvas too large");
        if (factors)
            hipLaunchKernelGGL(paste_canvas_kernel<true>, dim3((unsigned)blocks, (unsigned)b), dim3(AUG_THREADS), 0, stream,
                               src, src_bytes, params, rects, rect_off, taps, ntaps, paste_off, mean, canvas, canvas_stride,
                               out_h, out_w, PstJitter<true>{factors, gray_mean});
        else
            hipLaunchKernelGGL(paste_canvas_kernel<false>, dim3((unsigned)blocks, (unsigned)b), dim3(AUG_THREADS), 0, stream,
                               src, src_bytes, params, rects, rect_off, taps, ntaps, paste_off, mean, canvas, canvas_stride,
                               out_h, out_w, PstJitter<false>{});
        RR_CHECK_LAUNCH("rr_augment_frames_pasted (canvas)");
    }
    if (stages & 2) {
        hipLaunchKernelGGL(paste_objects_kernel, dim3((unsigned)b), dim3(PASTE_THREADS), 0, stream, params, pastes,
                           paste_off, canvas, canvas_stride, scratch, scratch_stride);
        RR_CHECK_LAUNCH("rr_augment_frames_pasted (paste)");
    }
    if (stages & 4) {
        const long npix = (long)b * out_h * out_w;
        const long blocks = (npix + per_block - 1) / per_block;
        RR_CHECK_ARG(blocks <= 0x7fffffffL, "rr_augment_frames_pasted: too many pixels");
        hipLaunchKernelGGL(paste_finish_kernel, dim3((unsigned)blocks), dim3(AUG_THREADS), 0, stream, params, canvas,
                           canvas_stride, mean, stdv, out, npix, out_h, out_w);
        RR_CHECK_LAUNCH("rr_augment_frames_pasted (finish)");
    }
    return RR_OK;
}

extern "C" int rr_augment_frames_pasted(const unsigned char *src, long src_bytes, const int *params, const int *rects,
                                        const int *rect_off, const int *taps, int ntaps, const int *pastes,
                                        const int *paste_off, const float *mean, const float *stdv, float *canvas,
                                        long canvas_stride, float *scratch, long scratch_stride, float *out, int b,
                                        int out_h, int out_w, int stages, hipStream_t stream)
{
    return augment_frames_pasted(src, src_bytes, params, rects, rect_off, taps, ntaps, pastes, paste_off, mean, stdv, nullptr,
                                 nullptr, canvas, canvas_stride, scratch, scratch_stride, out, b, out_h, out_w, stages, stream);
}

extern "C" int rr_augment_frames_pasted_jitter(const unsigned char *src, long src_bytes, const int *params,
                                               const int *rects, const int *rect_off, const int *taps, int ntaps,
                                               const int *pastes, const int *paste_off, const float *mean,
                                               const float *stdv, const float *factors, const int *gray_mean,
                                               float *canvas, long canvas_stride, float *scratch, long scratch_stride,
                                               float *out, int b, int out_h, int out_w, int stages, hipStream_t stream)
{
    RR_CHECK_ARG(factors && gray_mean, "rr_augment_frames_pasted_jitter: null pointer");
    return augment_frames_pasted(src, src_bytes, params, rects, rect_off, taps, ntaps, pastes, paste_off, mean, stdv, factors,
                                 gray_mean, canvas, canvas_stride, scratch, scratch_stride, out, b, out_h, out_w, stages,
                                 stream);
}
