/* rrnet_hip_dw.h — companion header of rrnet_hip.h: ShuffleNetV2's kernel family (csrc/depthwise.hip), exported by the same
 * librrnet_hip.so.  Same conventions as rrnet_hip.h: C ABI, 0 on success, rr_last_error() holds the message of a failure,
 * every entry enqueues on `stream` and returns; pointers are device pointers.  rrnet_amd/_C.py types the bindings from
 * this file with the parser it uses for rrnet_hip.h (_C.Family). */
#ifndef RRNET_HIP_DW_H
#define RRNET_HIP_DW_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_INCLUDE_HIP_HIP_RUNTIME_API_H__
#ifndef RRNET_HIP_H
typedef struct ihipStream_t *hipStream_t;
#endif
#endif

/* ---- depthwise 3x3 convolution (backbones/shufflenet.py:65,75,89: nn.Conv2d(c, c, 3, s, 1, groups=c, bias=False)) -------- *
 * NHWC fp32.  x [n, h, w, c], filter [c, 3, 3] (the parameter's [c, 1, 3, 3]), padding 1, stride s in {1, 2}; the output is
 * [n, P, Q, c], P = (h - 1) / s + 1, Q = (w - 1) / s + 1.  No reduction over channels: a lane owns four channels of a pixel
 * (16 bytes), every sum is taken in one fixed order without atomics, every output is written whole.
 * rr_dwconv3x3_fwd: y[n, i, j, ch] = (sum over a, b ascending of f[ch, a, b] * x[n, i s - 1 + a, j s - 1 + b, ch], the taps
 *   inside the map, each product rounded and added in that order) + bias[ch].  bias may be NULL (inference hands the folded
 *   BatchNorm shift).  slab may be NULL; otherwise it receives the BatchNorm partial sums of y, [mtiles][2][c] doubles (row 0
 *   the sums, row 1 the sums of squares), mtiles = ceil(n P Q / RR_DW_SLAB_PIXELS): the layout rr_conv_fprop writes, read by
 *   rr_bn_reduce_slab / rr_bn_stats_finalize.
 * rr_dwconv3x3_bwd_data: dx[n, y, x, ch] = sum over the (a, b) ascending with (y + 1 - a) and (x + 1 - b) divisible by s and
 *   the quotients i < P, j < Q of f[ch, a, b] * dy[n, i, j, ch]; n, h, w are x's (= dx's) sizes.
 * rr_dwconv3x3_bwd_weight: df[ch, a, b] (+)= sum over n, i, j of x[n, i s - 1 + a, j s - 1 + b, ch] * dy[n, i, j, ch].
 *   Stage one: a workgroup per tile of tile_pixels output pixels leaves its sums in partial [ceil(n P Q / tile_pixels)][c][9]
 *   doubles; stage two adds the tiles in ascending order in double and rounds once.  accumulate != 0: df already holds a
 *   gradient (the parameter's slice of the flat gradient buffer) and the sum is added to it.  Two launches. */
#define RR_DW_SLAB_PIXELS 64
int rr_dwconv3x3_fwd(const float *x, const float *f, const float *bias, float *y, double *slab, int n, int h, int w, int c, int s,
                     hipStream_t stream);
int rr_dwconv3x3_bwd_data(const float *dy, const float *f, float *dx, int n, int h, int w, int c, int s, hipStream_t stream);
int rr_dwconv3x3_bwd_weight(const float *x, const float *dy, double *partial, float *df, int accumulate, int n, int h, int w,
                            int c, int s, int tile_pixels, hipStream_t stream);

/* ---- channel shuffle (backbones/shufflenet.py:31-45,97-110) ------------------------------------------------------------- *
 * channel_shuffle(cat(a, b), 2) is an interleave.  Every operand is [pixels, channels] fp32 with a pixel stride of its own
 * (in floats, >= its channels), so that a channel slice of an NHWC tensor is read or written in place.  half % 4 == 0 and
 * every stride % 4 == 0 (a lane moves 16 bytes); every pointer 16-byte aligned.
 * rr_shuffle_interleave:   out[p, 2 i] = a[p, i], out[p, 2 i + 1] = b[p, i], i < half.
 * rr_shuffle_deinterleave: da[p, i] = g[p, 2 i], db[p, i] = g[p, 2 i + 1]: the interleave's backward and exact inverse.
 * rr_channel_copy:  dst[p, i] = src[p, i], i < ch: the upper half of a stride-1 unit's input out into the branch's tensor.
 * rr_channel_join:  out[p, i] = lo[p, i], out[p, half + i] = hi[p, i]: two halves back into one gradient tensor. */
int rr_shuffle_interleave(const float *a, int a_stride, const float *b, int b_stride, float *out, int out_stride, int pixels,
                          int half, hipStream_t stream);
int rr_shuffle_deinterleave(const float *g, int g_stride, float *da, int da_stride, float *db, int db_stride, int pixels,
                            int half, hipStream_t stream);
int rr_channel_copy(const float *src, int src_stride, float *dst, int dst_stride, int pixels, int ch, hipStream_t stream);
int rr_channel_join(const float *lo, int lo_stride, const float *hi, int hi_stride, float *out, int out_stride, int pixels,
                    int half, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RRNET_HIP_DW_H */
