// ColorJitter (datasets/transforms/transforms.py:120-130, functional.py:159-174) on one uint8 RGB pixel, shared by
// jitter.hip (the grey-mean reduction), augment.hip and augment_paste.hip (the jittered tap reads).  The reference calls
// PIL's ImageEnhance.Brightness, Contrast and Color in this order; each is Image.blend(degenerate, image, alpha), which
// Blend.c evaluates in float32 as  t = (float)d + alpha * (float)(v - d)  (one multiply, one add, no fma: every file that
// includes this header is compiled with -ffp-contract=off), clipped to 0 at t <= 0, to 255 at t >= 255 and truncated
// otherwise.  Degenerate values: brightness 0; contrast the frame's rounded grey mean m (every channel); colour the
// pixel's own grey value L (every channel), L = (r*19595 + g*38470 + b*7471 + 0x8000) >> 16 (Convert.c L24 >> 16).
#pragma once

__device__ __forceinline__ int jit_blend(int d, int v, float alpha)
{
    const float t = (float)d + alpha * (float)(v - d);
    return !(t > 0.f) ? 0 : (t >= 255.f ? 255 : (int)t);     // a NaN factor gives 0, never an unclamped value
}

__device__ __forceinline__ int jit_gray(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// brightness alone: what the grey mean is taken over
__device__ __forceinline__ void jit_brightness(int &r, int &g, int &b, float fb)
{
    r = jit_blend(0, r, fb), g = jit_blend(0, g, fb), b = jit_blend(0, b, fb);
}

// the three stages; m = the frame's grey mean after brightness (rr_jitter_gray_mean), already clamped to 0..255
__device__ __forceinline__ void jit_pixel(int &r, int &g, int &b, float fb, float fc, float fs, int m)
{
    jit_brightness(r, g, b, fb);
    r = jit_blend(m, r, fc), g = jit_blend(m, g, fc), b = jit_blend(m, b, fc);
    const int l = jit_gray(r, g, b);
    r = jit_blend(l, r, fs), g = jit_blend(l, g, fs), b = jit_blend(l, b, fs);
}
