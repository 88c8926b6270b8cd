/* rrnet_hip_rows.h — companion header of rrnet_hip.h: the rows route of the convolution gradients (csrc/conv_rows.hip and the
 * gated launches of csrc/conv.hip), exported by the same librrnet_hip.so.  Same conventions as rrnet_hip.h: C ABI, 0 on success,
 * rr_last_error() holds the message of a failure, every entry enqueues on `stream` and returns; pointers are device pointers.
 * rrnet_amd/_C.py types the bindings from this file with the parser it uses for rrnet_hip.h (_C.Family). */
#ifndef RRNET_HIP_ROWS_H
#define RRNET_HIP_ROWS_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_INCLUDE_HIP_HIP_RUNTIME_API_H__
#ifndef RRNET_HIP_H
typedef struct ihipStream_t *hipStream_t;
#endif
#endif

/* ---- The two gradients of a stride-1 convolution computed from the pixels whose
 * incoming gradient row is not all zero.  For layers behind a loss that touches few pixels (the wh / offset heads under
 * RegL1Loss: at most one pixel per object, 17 + 16 through the wh head's tap pair) the dense kernels multiply zeros.
 *
 * rr_active_rows(dy [m][k]): rows[0..*count) = the ascending indices of the rows of dy that hold a value v != 0 (+-0 counts
 *   as zero, NaN and Inf as non-zero).  rows: m ints; work: rr_active_rows_work_bytes(m) bytes of scratch.  Two launches, one
 *   pass over dy, no atomics: the order is fixed.
 * rr_active_targets(rows_work = the work buffer rr_active_rows left for dy [n,p,q,.]): targets[0..*count) = the ascending indices of
 *   the pixels t of dx [n,h,w,.] that a listed pixel of dy reaches through a tap, p = t + (pad_h - r, pad_w - s).  targets: n*h*w
 *   ints; work: rr_active_rows_work_bytes(n*h*w) bytes.  Two launches, no atomics.
 * rr_conv_dgrad_s1_rows: for the listed TARGETS t_j only, gathered like the dense kernel,
 *     dx[t_j][c] (+)= sum over taps, ko of dy[t_j + (pad_h - r, pad_w - s)][ko] * w[ko][r][s][c]       (taps outside dy read zero)
 *   one owner and one fixed summation order per element, no atomics: bit-reproducible from run to run.  accumulate == 0: dx is
 *   zero-filled first (every pixel that is no target has a zero gradient).  count / max_rows are those of the target list.
 * rr_conv_wgrad_rows: from the listed pixels p_i of dy only,
 *     dw[ko][r][s][c] += sum_i dy[p_i][ko] * x[p_i + (r - pad_h, s - pad_w)][c]   (taps outside read zero)
 *   with float atomics, as rr_conv_wgrad.  w is the filter itself (OHWI), not the flipped copy.
 *   They act iff *count <= max_rows (read on the device, no host read) and otherwise touch nothing; grids are sized for
 *   max_rows (<= the pixels of the listed tensor).  C and K multiples of 4, every tensor below 2 GiB.
 * rr_conv_dgrad_s1_unless / rr_conv_wgrad_unless: rr_conv_dgrad_s1 (wt: the flipped filter) / rr_conv_wgrad at stride 1 that act
 *   iff *count > max_rows: the dense side of the gate.  A caller enqueues the pair with the same count and max_rows; exactly
 *   one of the two does the work.  Shapes that rr_conv_dgrad_s1 would hand to another kernel family are refused.
 * Results equal the dense route's up to the fp32 summation order and the sign of zeros.  One deliberate difference: a row
 * that is exactly zero contributes nothing, where the dense kernels produce 0 * Inf = NaN from a non-finite x or w (a step
 * in that state already has non-finite forward outputs). */
size_t rr_active_rows_work_bytes(long m);
int rr_active_rows(const float *dy, long m, int k, int *rows, int *count, int *work, hipStream_t stream);
int rr_active_targets(const int *rows_work, int n, int h, int wd, int r, int s, int pad_h, int pad_w, int *targets, int *count,
                      int *work, hipStream_t stream);
int rr_conv_dgrad_s1_rows(const float *dy, const float *w, float *dx, int n, int h, int wd, int c, int k, int r, int s, int pad_h,
                          int pad_w, int accumulate, const int *targets, const int *count, int max_rows, hipStream_t stream);
int rr_conv_wgrad_rows(const float *x, const float *dy, float *dw, int n, int h, int wd, int c, int k, int r, int s, int pad_h,
                       int pad_w, const int *rows, const int *count, int max_rows, hipStream_t stream);
int rr_conv_dgrad_s1_unless(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k, int r, int s,
                            int pad_h, int pad_w, int accumulate, const int *count, int max_rows, hipStream_t stream);
int rr_conv_wgrad_unless(const float *x, const float *dy, float *dw, int n, int h, int wd, int c, int k, int r, int s,
                         int pad_h, int pad_w, const int *count, int max_rows, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif
