/* rrnet_hip_se.h — companion header of rrnet_hip.h: the SE hourglass' kernel family (csrc/se.hip), exported by the same
 * librrnet_hip.so.  Same conventions as rrnet_hip.h: C ABI, 0 on success, rr_last_error() holds the message of a failure,
 * every entry enqueues on `stream` and returns; pointers are device pointers.  rrnet_amd/_C.py types the bindings from
 * this file with the parser it uses for rrnet_hip.h (_C.Family). */
#ifndef RRNET_HIP_SE_H
#define RRNET_HIP_SE_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_INCLUDE_HIP_HIP_RUNTIME_API_H__
#ifndef RRNET_HIP_H
typedef struct ihipStream_t *hipStream_t;
#endif
#endif

/* ---- SE hourglass: squeeze-and-excitation tail and the stem's 2x2 pool (se.hip) --------------------------------- *
 * backbones/se_hourglass.py:12-27,50-60: out = relu(u * s[n, c] + skip), s = sigmoid(W2 relu(W1 mean_hw(u))), W1 [c/r, c],
 * W2 [c, c/r], no biases.  u / skip / out / dout / du / dskip are NHWC fp32 [n, hw, c]; every entry requires c % 4 == 0
 * (16 bytes per lane along c) and refuses anything else.  No floating-point atomics: every reduction has a fixed order.
 * rr_se_squeeze: part [n, nchunk, c] (double), nchunk = ceil(hw / chunk_rows) = the sums of u over each chunk of rows; grid
 *   samples x chunks.  rr_se_bwd_reduce: the same of g * u, g = dout * (out > 0).
 * rr_se_excite_fwd: one workgroup per sample; chunks summed in ascending order -> m [n, c] = mean, h [n, cr] = relu(W1 m),
 *   s [n, c] = sigmoid(W2 h); c <= 2048.
 * rr_se_excite_bwd: part (of rr_se_bwd_reduce) -> ds -> through sigmoid, W2, ReLU, W1 -> dm [n, c]; dw1 [cr, c] and dw2 [c, cr]
 *   are ADDED to, the samples in ascending order; ws: n * (c + cr) floats of scratch.
 * rr_se_bwd_apply: du = g * s[n, c] + dm[n, c] / hw; exactly one of dskip (written: g) and dskip_into (+= g) is given.
 * rr_maxpool2x2_fwd / _bwd: nn.MaxPool2d(2) (:164), x [n, h, w, c] -> y [n, h/2, w/2, c] (floor; h, w >= 2), idx (uint8, y's
 *   shape) = the winning tap ky * 2 + kx; the first maximum in row-major order wins, a NaN replaces the running maximum
 *   (ATen's rule, as rr_maxpool3x3s2_fwd).  The backward writes dx [n, h, w, c] whole: the odd last row / column get zeros. */
int rr_se_squeeze(const float *u, double *part, int n, int hw, int c, int chunk_rows, hipStream_t stream);
int rr_se_excite_fwd(const double *part, const float *w1, const float *w2, float *m, float *h, float *s, int n, int nchunk,
                     int c, int cr, int hw, hipStream_t stream);
int rr_se_scale_res_relu_fwd(const float *u, const float *s, const float *skip, float *out, int n, int hw, int c,
                             hipStream_t stream);
int rr_se_bwd_reduce(const float *dout, const float *out, const float *u, double *part, int n, int hw, int c, int chunk_rows,
                     hipStream_t stream);
int rr_se_excite_bwd(const double *part, const float *s, const float *h, const float *m, const float *w1, const float *w2,
                     float *dm, float *dw1, float *dw2, float *ws, int n, int nchunk, int c, int cr, hipStream_t stream);
int rr_se_bwd_apply(const float *dout, const float *out, const float *s, const float *dm, float *du, float *dskip,
                    float *dskip_into, int n, int hw, int c, hipStream_t stream);
int rr_maxpool2x2_fwd(const float *x, float *y, unsigned char *idx, int n, int h, int w, int c, hipStream_t stream);
int rr_maxpool2x2_bwd(const float *dy, const unsigned char *idx, float *dx, int n, int h, int w, int c, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RRNET_HIP_SE_H */
