/* rrnet_hip_wino.h — companion header of rrnet_hip.h: the Winograd F(2x2,3x3) route of the large stride-1 fp32 convolutions
 * (csrc/conv_wino.hip; its sixteen GEMMs run conv.hip's forward kernel), exported by the same librrnet_hip.so.  Same
 * conventions as rrnet_hip.h: C ABI, 0 on success, rr_last_error() holds the message of a failure, every entry enqueues on
 * `stream` and returns; pointers are device pointers.  rrnet_amd/_C.py types the bindings from this file with the parser it
 * uses for rrnet_hip.h (_C.Family). */
#ifndef RRNET_HIP_WINO_H
#define RRNET_HIP_WINO_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef __HIP_INCLUDE_HIP_HIP_RUNTIME_API_H__
#ifndef RRNET_HIP_H
typedef struct ihipStream_t *hipStream_t;
#endif
#endif

/* ---- A 3x3, stride-1, pad-1 convolution y = x (*) w as Y = At [ (G g Gt) . (Bt d B) ] A on 2x2 output tiles: 16 instead of 36
 * multiplications per tile and channel pair.  NHWC fp32, C and K multiples of 4, every tensor below 2 GiB.  Four launches:
 *   input transform   V[16][T][C] = Bt d B        T = n * ceil(h/2) * ceil(w/2) tiles; window pixels outside x read 0
 *   sixteen GEMMs     M[i][t][ko] = sum_c V[i][t][c] * U[i][ko][c]      (one launch, the batch index in the grid)
 *   output transform  y = At M A, then the forward kernel's epilogue
 * and, once per filter and optimizer step, the filter transform U[16][K][C] = G g Gt (g = w[ko][.][.][c], OHWI).
 * The data gradient of such a layer is the same convolution of dy with the flipped / transposed filter wt
 * (rr_weight_flip_transpose): U = rr_wino_filter(wt, c, k), and c / k change places in the call.
 *
 * Results equal rr_conv_fprop's up to fp32 rounding of a DIFFERENT arithmetic (about twice its rounding error), not only of
 * another summation order: exact cancellation and the sign of zeros are not preserved, and a non-finite input element
 * reaches every output of the 2x2 tiles whose 4x4 window holds it (up to two pixels further than a tap reaches).
 * No atomics, no workgroup waits for another: bit-reproducible from run to run.
 *
 * rr_conv_wino_plan: wino_plan of csrc/conv_plan.h.  flags as rr_conv_fprop_plan (1 bias, 2 ReLU, 4 statistics, 8 accumulate,
 *   16 strided destination, bits 8-9 the link); math: ops.MATH_*; out_h / out_w > 0: an explicit output size (refused).
 *   plan[RR_WINO_PLAN_INTS] = {take (0: the direct route keeps the launch; never an error), the pixel floor is the only reason
 *   not to, tiles T (two ints: low 31 bits, high), GEMM tile width, GEMM workgroups per batch index, output-transform grid x, y, tiles per output workgroup,
 *   workspace bytes (two ints: low 31 bits, high)}.
 * rr_conv_wino_ws_bytes: V + M of one launch (16 * T * (c + k) floats).
 * rr_wino_filter: one filter; rr_wino_filter_batch: `table` holds one row of four 64-bit words per filter {source pointer,
 *   destination pointer, K, C} — all filters of a model in one launch (rrnet_amd/flat.py).
 * rr_conv_wino_fprop: y (+)= the convolution, + bias, ReLU (either may be absent); accumulate != 0 adds into y first (the data
 *   gradient's fan-in).  stat_slab (may be NULL): rr_conv_stat_slab_bytes(n, h, wd, k) bytes, [ceil(n*h*wd/128)][2][k] doubles,
 *   every row written, the rows sum to the column sums / sums of squares of the STORED y (fp32 chains of at most 32 values
 *   before they go to double); read by rr_bn_reduce_slab / rr_bn_stats_finalize.  ws: ws_bytes >= rr_conv_wino_ws_bytes.
 *   The entry points do not apply the plan's pixel floor (tests and benchmarks run below it); everything else it refuses
 *   is an error here.
 * rr_conv_wino_dgrad_bnsum: rr_conv_dgrad_s1_bnsum's contract on this route: dx [n,h,wd,c] (+)= the data gradient of dy
 *   [n,h,wd,k] (u from wt), and sums [2][c] (zeroed by the caller) receive what rr_bn_bwd_reduce(dx, prod_z, prod_y, ...) returns
 *   (same mask rule rr_bn_affine, same product order); slab: rr_conv_stat_slab_bytes(n, h, wd, c) bytes of scratch.
 * rr_wino_input / rr_wino_gemm: the first two stages alone (benchmarks: per-stage times).
 *
 * ---- The weight gradient of such a layer as F(3x3,2x2): dg = Gt [ sum over tiles (A dy_tile At) . (Bt d B) ] G, A = At^T,
 * again 16 instead of 36 multiplications per tile and channel pair.  x [n,h,wd,c], dy [n,h,wd,k], dw [k][3][3][c]; C and K
 * multiples of 4 above 32, every tensor and every slice of V and W below 2 GiB.  Five launches:
 *   input transform   V[16][T][c] = Bt d B                      (the forward route's kernel)
 *   dy transform      W[16][T][k] = A dy_tile At                pixels outside dy (ragged last tile row / column) read 0
 *   zero fill         S[k][16][c] = 0
 *   sixteen GEMMs     S[ko][i][c] += sum_t W[i][t][ko] * V[i][t][c]   (one launch of the weight-gradient kernel, the tiles split
 *                                                                     like rr_conv_wgrad splits its pixels: float atomics into S)
 *   dw transform      dw += Gt S G                              a plain read-modify-write of the running gradient
 * Results equal rr_conv_wgrad's up to fp32 rounding of a DIFFERENT arithmetic: exact cancellation and the sign of zeros are not
 * preserved; a non-finite element of dy at filter ko (of x at channel c) stays inside dw[ko] (dw[.][.][.][c]) but may reach all
 * nine taps there.  Like rr_conv_wgrad's, the sum order of the split partials varies from run to run.
 *
 * rr_conv_wino_wgrad_plan: wino_wgrad_plan of csrc/conv_plan.h; arguments as rr_conv_wino_plan, flags: 1 a gated launch
 *   (rr_conv_wgrad_unless; refused).  plan[RR_WINO_WGRAD_PLAN_INTS] = {take (0: rr_conv_wgrad keeps the launch; never an error), the
 *   pixel floor is the only reason not to, tiles T (two ints: low 31 bits, high), PIPE of the GEMM kernel (3: T % 32 == 0, else 1),
 *   splits of T, K-steps per split, GEMM workgroups, workspace bytes (two ints: low 31 bits, high)}.
 * rr_conv_wino_wgrad_ws_bytes: V + W + S of one launch (16 * T * (c + k) + 16 * k * c floats).
 * rr_conv_wino_wgrad: dw += the weight gradient; ws: ws_bytes >= rr_conv_wino_wgrad_ws_bytes.  Like the forward entry points it does
 *   not apply the plan's pixel floor.
 * rr_wino_dy / rr_wino_wgrad_gemm / rr_wino_dw: the stages alone (benchmarks: per-stage times); rr_wino_wgrad_gemm adds into s. */
#define RR_WINO_PLAN_INTS 11
int rr_conv_wino_plan(int math, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w, int out_h,
                      int out_w, int flags, int *plan);
size_t rr_conv_wino_ws_bytes(int n, int h, int wd, int c, int k);
int rr_wino_filter(const float *w, float *u, int k, int c, hipStream_t stream);
int rr_wino_filter_batch(const long long *table, int nfilters, hipStream_t stream);
int rr_conv_wino_fprop(const float *x, const float *u, const float *bias, float *y, double *stat_slab, float *ws, size_t ws_bytes,
                       int n, int h, int wd, int c, int k, int relu, int accumulate, hipStream_t stream);
int rr_conv_wino_dgrad_bnsum(const float *dy, const float *u, float *dx, float *ws, size_t ws_bytes, int n, int h, int wd, int c,
                             int k, int accumulate, const float *prod_y, const float *prod_z, const float *prod_mean,
                             const float *prod_invstd, const float *prod_mask_scale, const float *prod_mask_shift, double *slab,
                             double *sums, hipStream_t stream);
int rr_wino_input(const float *x, float *v, int n, int h, int wd, int c, hipStream_t stream);
int rr_wino_gemm(const float *v, const float *u, float *m, long tiles, int c, int k, hipStream_t stream);
#define RR_WINO_WGRAD_PLAN_INTS 10
int rr_conv_wino_wgrad_plan(int math, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w, int out_h,
                            int out_w, int flags, int *plan);
size_t rr_conv_wino_wgrad_ws_bytes(int n, int h, int wd, int c, int k);
int rr_conv_wino_wgrad(const float *x, const float *dy, float *dw, float *ws, size_t ws_bytes, int n, int h, int wd, int c, int k,
                       hipStream_t stream);
int rr_wino_dy(const float *dy, float *w, int n, int h, int wd, int k, hipStream_t stream);
int rr_wino_wgrad_gemm(const float *v, const float *w, float *s, long tiles, int c, int k, hipStream_t stream);
int rr_wino_dw(const float *s, float *dw, int k, int c, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RRNET_HIP_WINO_H */
