/*
 * rrnet_hip.h — C ABI of librrnet_hip.so: the MI355X (gfx950) implementation of RRNet's
 * detection hot path.  Every entry point is `extern "C"`, takes plain device pointers and
 * sizes plus a hipStream_t, allocates nothing (scratch comes from an explicit
 * rr_*_workspace_bytes query), is asynchronous on the given stream and returns 0 or a
 * negative error code (text via rr_last_error(), thread-local).
 *
 * Each declaration cites the reference interface it replaces (file:line under
 * /root/reference).  INTEGRATION.md shows the reference-side binding (ctypes) a maintainer
 * would add.  Layouts: activations NHWC fp32 ("channels_last"), conv weights OHWI fp32
 * (= torch channels_last of the reference's [Cout,Cin,kh,kw] parameters), boxes row-major.
 */
#ifndef RRNET_HIP_H
#define RRNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RR_ABI_VERSION 1

#ifndef __HIP_INCLUDE_HIP_HIP_RUNTIME_API_H__
typedef struct ihipStream_t *hipStream_t;
#endif

/* ---- library ------------------------------------------------------------------------ */
const char *rr_last_error(void);
int rr_abi_version(void);

/* ---- Soft-NMS ----------------------------------------------------------------------- *
 * Replaces ext/nms/nms/cpu_nms.pyx:17-120 `cpu_soft_nms(boxes, sigma, Nt, threshold, method)`
 * (bound by ext/nms/nms_wrapper.py:13-19) and its per-class drivers
 * operators/rrnet_operator.py:211-232, models/rrnet.py:56-80, utils/metrics/metrics.py:308-324.
 * `boxes` holds nseg segments back to back, `stride` floats per row (>= 5; columns 0..4 =
 * x1,y1,x2,y2,score are permuted in place, further columns are left where they are, as in
 * the reference).  Segment s = rows [seg_off[s], seg_off[s+1]).  On return rows
 * [seg_off[s], seg_off[s] + n_out[s]) are the kept detections in the reference's order,
 * bit for bit.  method: 1 linear, 2 gaussian, else hard (weight 0).  *err_flag is set to 1
 * where the reference would raise ZeroDivisionError (union area == 0); it must be zeroed by
 * the caller.  Segments above RR_SOFT_NMS_LDS_MAX boxes need `workspace`
 * (rr_soft_nms_workspace_bytes); seg_off, n_out, err_flag are device pointers. */
#define RR_SOFT_NMS_LDS_MAX 6000
size_t rr_soft_nms_workspace_bytes(int total_boxes, int max_seg_boxes);
int rr_soft_nms_segments(float *boxes, const int *seg_off, int nseg, int max_seg_boxes, int stride,
                         float sigma, float Nt, float threshold, int method, int *n_out,
                         int *err_flag, void *workspace, hipStream_t stream);
/* Same, with explicit segment lengths: segment s = rows [seg_off[s], seg_off[s] + seg_len[s]) (rows between the
 * length and the next offset are ignored) — the layout rr_refine_boxes leaves behind. */
int rr_soft_nms_ragged(float *boxes, const int *seg_off, const int *seg_len, int nseg, int max_seg_boxes, int stride,
                       float sigma, float Nt, float threshold, int method, int *n_out, int *err_flag,
                       void *workspace, hipStream_t stream);
/* Introspection, for tests: HOW a Soft-NMS call of nseg segments of up to max_seg_boxes boxes would launch, as the host plan
 * of csrc/softnms_plan.h decides it.  Launches nothing, needs no device.  out[0..10] = {launches (0: an empty batch; 2: the
 * two-launch split of the LDS loop), kernel (0 register-resident, 1 LDS loop), threads per workgroup (of the last launch),
 * boxes per lane (register kernel; else 0), dynamic LDS bytes and row capacity of the last launch (LDS loop; else 0), that
 * launch raises the function's dynamic-LDS limit first, threads and dynamic LDS bytes of the first launch of a split (else 0),
 * the caller must bring a workspace, the kernel runs on it (the LDS loop's global-workspace form)}; out[11..16] = the
 * per-segment constants of the kernels: {deaths of one step the register kernel renumbers from its list (more: the mask path),
 * longest segment that runs <256, 1> inside a wider register launch, longest segment the LDS loop runs on one wave, longest
 * segment of the split's first launch, RR_SOFT_NMS_LDS_MAX, longest segment of the register kernels (the mask's capacity)};
 * the rest 0.  n_out >= RR_SOFT_NMS_PLAN_INTS.  A bound the entry points refuse (negative, >= 65536) returns an error; they
 * also refuse stride < 5 and, where out[9] is set, a null workspace.  Scores and coordinates must be finite. */
#define RR_SOFT_NMS_PLAN_INTS 18
int rr_soft_nms_plan(int nseg, int max_seg_boxes, int *out, int n_out);


/* ---- Convolutions (NHWC fp32, implicit GEMM on v_mfma_f32_32x32x2_f32) --------------- *
 * Replace what the reference delegates to cuDNN through nn.Conv2d:
 * backbones/hourglass.py:17,21,25,48,143,167,173 (ResidualBlock / ConvBNRelu / stem / inter),
 * detectors/centernet_detector.py:62,73,85 (3x3, 17x1, 1x17, 1x1 heads),
 * detectors/fasterrcnn_detector.py:11 + backbones/resnet.py:22-28 (stage-2 Bottleneck).
 * x [n,h,w,c], w [k][r][s][c] (OHWI), y [n,p,q,k], p = (h + 2*pad_h - r)/stride + 1.
 * fprop: optional bias[k], optional fused ReLU, optional per-block BatchNorm partial sums
 *   (`stat_slab`, rr_conv_stat_slab_bytes bytes: [ceil(n*p*q/128)][2][k] doubles = column
 *   sums and sums of squares of y, reduced by rr_bn_finalize).
 * dgrad: dx [n,h,w,c] = conv-transpose of dy [n,p,q,k]; accumulate != 0 adds into dx.
 * wgrad: dw [k][r][s][c] += x (*) dy, split over the n*p*q pixels and summed with float
 *   atomics (the caller zeroes dw once per step; the flat gradient buffer is that target).
 *   out_h/out_w > 0 give dy's spatial size explicitly (asymmetric padding: pad_h/pad_w are the leading
 *   pads); 0 derives it from the symmetric formula. */
size_t rr_conv_stat_slab_bytes(int n, int p, int q, int k);
int rr_conv_fprop(const float *x, const float *w, const float *bias, float *y, double *stat_slab,
                  int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w,
                  int relu, hipStream_t stream);
int rr_conv_dgrad(const float *dy, const float *w, float *dx, int n, int h, int wd, int c, int k,
                  int r, int s, int stride, int pad_h, int pad_w, int accumulate, hipStream_t stream);
/* Stride-1 data gradient through the forward kernel (its [n][k] weight fragments are read 16 bytes at a time):
 * rr_weight_flip_transpose writes wt[c][r-1-i][s-1-j][k] = w[k][i][j][c] (k*r*s*c floats of caller scratch), then
 * rr_conv_dgrad_s1(dy [n,p,q,k], wt) = dx [n,h,w,c], p = h + 2*pad_h - r + 1.  Same result as rr_conv_dgrad
 * (different summation order inside the fp32 accumulation chain). */
int rr_weight_flip_transpose(const float *w, float *wt, int k, int c, int r, int s, hipStream_t stream);
/* The same for every filter of a flat parameter buffer in ONE launch (host layer: rrnet_amd/flat.py keeps the flipped copies
 * of all stride-1 layers in a second flat buffer, refreshed once per optimizer step): table = ntiles x int4 {element offset
 * of the filter in flat / wt_flat, (r*s) << 16 | k, c, tap << 20 | k_tile << 10 | c_tile}, one 32 x 32 tile of the (k, c)
 * plane of one tap per workgroup.  Filters of up to 65535 output channels, 1024 tiles per side, r*s < 2048. */
int rr_weight_flip_transpose_batch(const float *flat, float *wt_flat, const int *table, int ntiles, hipStream_t stream);
/* ... and, for the bf16-operand convolutions, bf16 copies of both (w16_flat: the filters as they are, wt16_flat: flipped /
 * transposed; bf16 elements at the same element offsets; either may be NULL). */
int rr_weight_flip_transpose_batch_bf16(const float *flat, float *wt_flat, unsigned short *w16_flat, unsigned short *wt16_flat,
                                        const int *table, int ntiles, hipStream_t stream);
int rr_conv_dgrad_s1(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                     int r, int s, int pad_h, int pad_w, int accumulate, hipStream_t stream);
/* Small-channel convolutions (the 7x7 stride-2 stem on a 3-channel image, backbones/hourglass.py:143): rr_conv_pack_taps
 * writes out [n,p,q,kp], out[..,k] = x[n, p*stride-pad_h+r, q*stride-pad_w+s, c] for k = (r*S+s)*c_in + c < r*s*c and 0 up
 * to kp (a multiple of 4, the caller pads to 32).  The convolution then is a 1x1 rr_conv_fprop over kp channels with the
 * OHWI weight rows zero-padded to kp, and its weight gradient a 1x1 rr_conv_wgrad — both on the vector MFMA kernels. */
int rr_conv_pack_taps(const float *x, float *out, int n, int h, int wd, int c, int r, int s, int stride, int pad_h,
                      int pad_w, int kp, hipStream_t stream);
/* rr_conv_dgrad_s1 that ALSO returns the BatchNorm-backward sums of the layer that produced the tensor whose gradient
 * it writes (the conv -> bn -> relu layer in front of this convolution, backbones/hourglass.py:31-40): the epilogue has
 * the finished gradient dz = dx in registers, reads the producer's pre-BN output prod_y [n,h,w,c] (and prod_z, its
 * post-activation output, when the ReLU mask cannot be recomputed as prod_y*mask_scale+mask_shift > 0; with neither
 * the producer has no ReLU and every element counts) and emits per
 * block sum(dz*mask) and sum(dz*mask*xhat) to `slab` (rr_conv_stat_slab_bytes(n,h,wd,c) bytes), reduced into
 * sums [2][c] (zeroed by the caller) — exactly what rr_bn_bwd_reduce(dx, prod_z, prod_y, ...) returns, without its
 * pass over dx and y.  accumulate != 0: dx += ..., the sums are taken of the final values (the last contributor of a
 * gradient fan-in).  Layers that run split-K, and sizes with n*h*wd not a multiple of 128 (the epilogue addresses whole
 * 128-row tiles), fall back to rr_bn_bwd_reduce internally: same contract. */
int rr_conv_dgrad_s1_bnsum(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                           int r, int s, int pad_h, int pad_w, int accumulate, const float *prod_y,
                           const float *prod_z, const float *prod_mean, const float *prod_invstd,
                           const float *prod_mask_scale, const float *prod_mask_shift, double *slab,
                           double *sums, hipStream_t stream);
/* The same idea for a producer of the form conv + bias + ReLU (the heads' 3x3 layers, detectors/centernet_detector.py:62,
 * whose output prod_z [n,h,w,c] is this convolution's input): dx = relu-masked gradient (dx * (prod_z > 0) is what is
 * STORED) and sums[0..c) = its column sums = the producer's bias gradient — what rr_bias_relu_bwd computes in a pass of
 * its own.  slab: rr_conv_stat_slab_bytes(n,h,wd,c) bytes; sums [2][c] doubles, zeroed by the caller (the second row is
 * not meaningful).  K and C multiples of 4 (the host layer zero-pads a 10- or 2-channel dy to 12 / 4); n*h*wd a multiple
 * of 128 (refused otherwise: the host layer then runs rr_conv_dgrad + rr_bias_relu_bwd).
 * accumulate != 0: dx holds the gradients of the producer's other consumers; the mask is applied to the SUM (the last
 * contributor of a fan-in: the three heads' 3x3 layers behind relu(feature), models/centernet.py:20-24), which also serves
 * a bare ReLU producer (its backward then is the identity on this tensor). */
int rr_conv_dgrad_s1_relubias(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                              int r, int s, int pad_h, int pad_w, int accumulate, const float *prod_z, double *slab,
                              double *sums, hipStream_t stream);
int rr_conv_wgrad(const float *x, const float *dy, float *dw, int n, int h, int wd, int c, int k,
                  int r, int s, int stride, int pad_h, int pad_w, int out_h, int out_w, hipStream_t stream);
/* Introspection, for tests: HOW a forward-kernel convolution (rr_conv_fprop*, rr_conv_dgrad_s1*, a parity class of
 * rr_conv_dgrad_s2_*) would launch, as the one host plan of csrc/conv_plan.h decides it.  Launches nothing, needs no device.
 * math: 0 fp32, 1 bf16, 2 f16x3.  out_h / out_w > 0: the output grid given explicitly (pads are leading pads).  flags: 1 bias,
 * 2 relu, 4 statistics wanted, 8 accumulate, 16 strided parity-class destination, (link << 8): 1 a BatchNorm producer (_bnsum),
 * 2 a conv + bias + ReLU producer (_relubias).  plan[RR_CONV_PLAN_INTS] = {row-streaming shortcut (the other fields are 0 then),
 * scalar gather, tile width, workgroups per K slice, split-K factor, position-major, one column tile per XCD, the link's sums
 * fused in the epilogue, pass afterwards (0 none, 1 rr_bn_reduce_slab, 2 rr_bn_bwd_reduce, 3 column statistics), destination
 * zero-filled, statistics slab zero-filled}.  A call the arithmetic refuses returns an error (rr_last_error says why). */
#define RR_CONV_PLAN_INTS 11
int rr_conv_fprop_plan(int math, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w,
                       int out_h, int out_w, int flags, int *plan);
/* The same for the gradient passes (dgrad_plan, dgrad_s2_plan, wgrad_plan of csrc/conv_plan.h).  pass: 0 rr_conv_dgrad (family 0),
 * 1 a parity-class data gradient (stride 2; family 1 rr_conv_dgrad_s2_bf16, 2 rr_conv_dgrad_s2_f16x3, 3 rr_conv16_dgrad_s2),
 * 2 a weight gradient (family 0 rr_conv_wgrad, 1 _bf16, 2 _f16x3, 3 rr_conv16_wgrad, which has no out_h / out_w).  out[], by pass —
 *   0: scalar gather, tile width, grid.x (workgroups of a class), grid.y (classes that launch), parity-decomposed, class order
 *      (2 bits per class, most taps first), split-K factor, dx zero-filled in front;
 *   1: dy's height, width, dx zero-filled in front, number of launches, then per launch 10 values: the class (h % 2, w % 2),
 *      sub-filter height and width, leading pads down and across, class image height and width, the sub-filter's offset in the
 *      packed filter in units of C*K elements, workgroups (family 3; 0 where rr_conv_fprop_plan decides the launch);
 *   2: dy's height, width, pixels, tile filters x channels, scalar dy loads, scalar x loads, pipeline mode (0 generic, 1, 3),
 *      tiles along K and along C, tiles, pixel splits, K-steps per split, workgroups, dynamic LDS bytes;
 * the rest 0.  n_out >= RR_CONV_GRAD_PLAN_INTS.  A call the pass refuses returns an error (rr_last_error says why). */
#define RR_CONV_GRAD_PLAN_INTS 44
int rr_conv_grad_plan(int pass, int family, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w,
                      int out_h, int out_w, int accumulate, int *out, int n_out);

/* ---- bf16-operand convolutions (BASELINE config 4, "bf16"; csrc/conv_bf16.hip) ------------------------------------- *
 * The reference is fp32-only (backbones/hourglass.py:12-61,127-199 -> nn.Conv2d), so this precision is builder-defined
 * and opt-in (cfg.Model.bf16): SAME tensors, layouts and semantics as the entry points above without the suffix — fp32
 * activations / weights / gradients in HBM — but the two operands of every product are rounded to bf16
 * (round-to-nearest-even) on their way into LDS and multiplied on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.
 * Contract: result == the fp32 entry point run on bf16-rounded operands, up to the summation order.
 * Vector shapes only (C % 4 == 0, R*S <= 64, for rr_conv_wgrad_bf16 also K % 4 == 0; every tensor < 2 GiB): the host
 * layer keeps the fp32 entry points for the rest (stride-2 data gradients, the 17-tap WH head, the 3-channel stem's
 * unpacked form).  rr_conv_dgrad_s1*_bf16 take the flipped / transposed filter of rr_weight_flip_transpose (fp32). */
/* w_bf16 / wt_bf16 (may be NULL): the same filter already rounded to bf16, same [k][r][s][c] element order (the host layer
 * keeps bf16 copies of all filters, refreshed once per optimizer step: rr_weight_flip_transpose_batch).  Used when
 * c % 8 == 0: 16-byte loads of 8 channels, no converts for the B operand; identical results. */
int rr_conv_fprop_bf16(const float *x, const float *w, const float *bias, float *y, double *stat_slab,
                       int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w,
                       int relu, const unsigned short *w_bf16, hipStream_t stream);
int rr_conv_dgrad_s1_bf16(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                          int r, int s, int pad_h, int pad_w, int accumulate, const unsigned short *wt_bf16,
                          hipStream_t stream);
int rr_conv_dgrad_s1_bnsum_bf16(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                                int r, int s, int pad_h, int pad_w, int accumulate, const float *prod_y,
                                const float *prod_z, const float *prod_mean, const float *prod_invstd,
                                const float *prod_mask_scale, const float *prod_mask_shift, double *slab,
                                double *sums, const unsigned short *wt_bf16, hipStream_t stream);
int rr_conv_dgrad_s1_relubias_bf16(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                                   int r, int s, int pad_h, int pad_w, int accumulate, const float *prod_z,
                                   double *slab, double *sums, hipStream_t stream);
int rr_conv_wgrad_bf16(const float *x, const float *dy, float *dw, int n, int h, int wd, int c, int k,
                       int r, int s, int stride, int pad_h, int pad_w, int out_h, int out_w, hipStream_t stream);

/* ---- convolutions on 16-bit ACTIVATIONS (round 5; config 4, cfg.Model.bf16; csrc/conv16.hip) ------------------------
 * Same convolutions (reference: nn.Conv2d of /root/reference/backbones/hourglass.py:12-61,127-199,
 * detectors/centernet_detector.py:80-93), same arithmetic contract as the *_bf16 entry points above (result == the fp32
 * entry point on bf16-rounded operands up to the summation order; fp32 accumulation) — but both operands are bf16 tensors
 * IN HBM: x / dy as written by their producers (rr_bn_apply_b16, rr_bn_bwd_apply_b16, rr_to_bf16), the filter's bf16
 * copy (rr_weight_flip_transpose_batch_bf16: plain for the forward, flipped / transposed for the data gradient).  They
 * reach LDS by LDS-DMA; 256 channels x 256 pixels per workgroup on v_mfma_f32_16x16x32_bf16.
 * Shapes: rr_conv16_supported (C % 64 == 0, K % 128 == 0, R*S <= 16, stride 1 or 2; input < 2 GiB); the host layer keeps
 * the *_bf16 entry points for the rest.  y / dx (fp32) and y16 / dx16 (the same values rounded to bf16, for a consumer
 * that is again a convolution): either may be NULL, not both.  stat_slab: [ceil(M / 256)][2][K] doubles
 * (rr_conv16_stat_slab_bytes), reduced by rr_bn_reduce_slab / rr_bn_stats_finalize like the fp32 kernel's. */
int rr_conv16_supported(int c, int k, int r, int s, int stride);
size_t rr_conv16_stat_slab_bytes(int n, int p, int q, int k);
int rr_conv16_fprop(const unsigned short *x, const unsigned short *w, const float *bias, float *y, unsigned short *y16,
                    double *stat_slab, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w,
                    int relu, hipStream_t stream);
int rr_conv16_dgrad_s1(const unsigned short *dy, const unsigned short *wt, float *dx, unsigned short *dx16, int n, int h,
                       int wd, int c, int k, int r, int s, int pad_h, int pad_w, int accumulate, hipStream_t stream);
/* rr_conv16_dgrad_s1 with the backward of the ReLU in front of the convolution applied in the epilogue (rr_conv_dgrad_s1_relubias without the
 * column sums: the producer is a bare ReLU, functional._ReLU): dx = (dx_conv [+ dx]) * (relu_out > 0). */
int rr_conv16_dgrad_s1_relumask(const unsigned short *dy, const unsigned short *wt, float *dx, int n, int h, int wd, int c, int k,
                                int r, int s, int pad_h, int pad_w, int accumulate, const float *relu_out, hipStream_t stream);
/* Stride-2 data gradient (rr_conv_dgrad_s2_bf16's contract: dx [n,h,w,c] = / += the gradient of a stride-2 convolution with filter
 * w [k][r][s][c] (fp32, rounded to bf16 while its parity-class sub-filters are packed into wsub: k*r*s*c bf16 of caller scratch);
 * dy bf16 [n,p,q,k]).  K % 64 == 0, C % 128 == 0, R*S <= 16, non-negative leading pads in every class (3x3 pad 1, 1x1 pad 0). */
int rr_conv16_dgrad_s2(const unsigned short *dy, const float *w, float *dx, int n, int h, int wd, int c, int k, int r, int s,
                       int pad_h, int pad_w, int accumulate, unsigned short *wsub, hipStream_t stream);
/* dw [k][r][s][c] fp32 += x (*) dy, both bf16 (rr_conv_wgrad's contract on bf16-rounded operands; fp32 atomics).
 * Shapes: rr_conv16_wgrad_supported (K % 128 == 0 — the last 256-filter tile may run half empty —, C % 128 == 0, stride 1 or 2; tensors < 2 GiB). */
int rr_conv16_wgrad_supported(int c, int k, int r, int s, int stride);
int rr_conv16_wgrad(const unsigned short *x, const unsigned short *dy, float *dw, int n, int h, int wd, int c, int k,
                    int r, int s, int stride, int pad_h, int pad_w, hipStream_t stream);

/* Producers of the bf16 images (csrc/elementwise.hip): rr_bn_apply / rr_bn_bwd_apply (reference: nn.BatchNorm2d + ReLU + residual
 * add of backbones/hourglass.py:31-40 and their autograd backward) with a second, bf16 output holding the same values
 * rounded to nearest even — written in the same pass, so the convolution that consumes the tensor never reads the fp32
 * one.  out / dx (fp32) may be NULL when nothing else reads them.  rr_to_bf16: the plain conversion, for operands that
 * come from elsewhere (fan-in sums, the up-sample add, head gradients). */
int rr_bn_apply_b16(const float *y, const unsigned short *y16, const float *scale, const float *shift, const float *res,
                    const unsigned short *res16, const float *res_scale, const float *res_shift, float *out,
                    unsigned short *out16, long total, int c, int relu, hipStream_t stream);
int rr_bn_bwd_apply_b16(const float *dz, const float *z, const unsigned short *z16, const float *y, const unsigned short *y16,
                        const float *mean, const float *invstd, const float *gamma, const float *mask_scale,
                        const float *mask_shift, const double *sums, double count, const double *count_dev, float *dx,
                        unsigned short *dx16, float *g_out, int g_accumulate, float *dgamma, float *dbeta, long total,
                        int c, hipStream_t stream);
/* y16 / res16 / z16: the convolution's pre-BN output / the residual / the layer's own output (the ReLU mask's source) when
 * it exists ONLY as its bf16 image (a tensor every consumer of which reads bf16: rrnet_amd.ops.phantom_f32); give y or
 * y16 (exactly one), res or res16, z or z16 (at most one each).
 * rr_bn_bwd_reduce_b16: rr_bn_bwd_reduce with z and / or y from their images (sums pre-zeroed).  rr_upsample2x_add_b16: the hourglass
 * up-path add (backbones/hourglass.py:121-124, even sizes) with either operand as fp32 or bf16 and the result as fp32
 * and / or bf16.  rr_from_bf16: the widening copy (a consumer without a bf16 form materialises the fp32 tensor). */
int rr_bn_bwd_reduce_b16(const float *dz, const float *z, const unsigned short *z16, const float *y, const unsigned short *y16,
                         const float *mean, const float *invstd, const float *mask_scale, const float *mask_shift,
                         double *sums, long npix, int c, hipStream_t stream);
int rr_upsample2x_add_b16(const float *up1, const unsigned short *up1_16, const float *low, const unsigned short *low_16,
                          float *out, unsigned short *out16, int n, int h, int w, int c, hipStream_t stream);
int rr_from_bf16(const unsigned short *x, float *out, long total, hipStream_t stream);
int rr_to_bf16(const float *x, unsigned short *out, long total, hipStream_t stream);

/* Data gradient of a head's narrow 1x1 convolution (K = 10 / 2 / 34 output channels behind a 3x3 conv + bias + ReLU:
 * /root/reference/detectors/centernet_detector.py:62,73,85-93), the producer's ReLU mask and bias gradient in the same
 * pass — rr_conv_dgrad_s1_relubias's contract for r = s = 1 without the channel padding:
 *   dx[m][c] = (prod_z[m][c] > 0) * ([dx[m][c] +] sum_k dy[m][k] * w[k][c]);  sums[c] += sum_m dx[m][c]  (doubles, pre-zeroed).
 * dy [m][k], w [k][c] (the layer's own OHWI filter), k <= 36, c a divisor of 1024; dx16 (may be NULL): bf16 image of dx.
 * HBM-bound element-wise kernel (csrc/elementwise.hip). */
int rr_head_dgrad_relubias(const float *dy, const float *w, float *dx, unsigned short *dx16, const float *prod_z,
                           double *sums, long m, int c, int k, int accumulate, hipStream_t stream);

/* ---- split-operand convolutions ("f16x3", cfg.Model.conv_math; csrc/conv_bf16.hip) -------------------------------
 * fp32 in, fp32 out, fp32 accumulation, as rr_conv_fprop / rr_conv_dgrad / rr_conv_wgrad (reference: nn.Conv2d in
 * /root/reference/backbones/hourglass.py:12-61); inside the kernel each operand is the sum of two fp16 values (22
 * significant bits, after a power-of-two scaling taken from the tensor's largest magnitude) and the three products
 * hi*hi + hi*lo + lo*hi run on the 16-bit matrix instructions.  amax_*: DEVICE words holding the bit pattern of
 * max|tensor|, produced by rr_absmax_bits (atomicMax into a word the caller zeroed; several calls may share a word to
 * take the maximum over several tensors).  Shapes as the _bf16 entry points.  w_split / wt_split (optional; C % 8 == 0,
 * K > 64): the filter (for the data gradients: the flipped / transposed one) already split into its two fp16 parts by
 * rr_weight_split_f16 with the SAME amax word — 2*k*r*s*c halves, hi image then lo image — instead of tile by tile inside
 * the convolution (48 of its 149 vector instructions per K-step and thread). */
int rr_weight_split_f16(const float *w, long n, const unsigned *amax_w, unsigned short *out, hipStream_t stream);
int rr_absmax_bits(const float *x, long n, unsigned *out, hipStream_t stream);
int rr_conv_fprop_f16x3(const float *x, const float *w, const float *bias, float *y, double *stat_slab,
                        int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h,
                        int pad_w, int relu, const unsigned *amax_x, const unsigned *amax_w,
                        const unsigned short *w_split, hipStream_t stream);
int rr_conv_dgrad_s1_f16x3(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                           int r, int s, int pad_h, int pad_w, int accumulate, const unsigned *amax_dy,
                           const unsigned *amax_w, const unsigned short *wt_split, hipStream_t stream);
int rr_conv_dgrad_s1_bnsum_f16x3(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                                 int r, int s, int pad_h, int pad_w, int accumulate, const float *prod_y,
                                 const float *prod_z, const float *prod_mean, const float *prod_invstd,
                                 const float *prod_mask_scale, const float *prod_mask_shift, double *slab,
                                 double *sums, const unsigned *amax_dy, const unsigned *amax_w,
                                 const unsigned short *wt_split, hipStream_t stream);
int rr_conv_dgrad_s1_relubias_f16x3(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                                    int r, int s, int pad_h, int pad_w, int accumulate, const float *prod_z,
                                    double *slab, double *sums, const unsigned *amax_dy, const unsigned *amax_w,
                                    hipStream_t stream);
int rr_conv_dgrad_s2_f16x3(const float *dy, const float *w, float *dx, int n, int h, int wd, int c, int k,
                           int r, int s, int pad_h, int pad_w, int accumulate, float *wsub, const unsigned *amax_dy,
                           const unsigned *amax_w, hipStream_t stream);
int rr_conv_wgrad_f16x3(const float *x, const float *dy, float *dw, int n, int h, int wd, int c, int k,
                        int r, int s, int stride, int pad_h, int pad_w, int out_h, int out_w, const unsigned *amax_x,
                        const unsigned *amax_dy, hipStream_t stream);

/* Stride-2 data gradient (rr_conv_dgrad with stride 2) on the bf16 forward kernel: one launch per output parity class
 * (h % 2, w % 2) with that class's sub-filter (1 / 2 / 2 / 4 taps of a 3x3), written to every second pixel of dx
 * [n,h,w,c]; classes no tap reaches are zeroed (unless accumulating).  w OHWI fp32; wsub: k*r*s*c floats of caller
 * scratch (the packed sub-filters).  C, K multiples of 4. */
int rr_conv_dgrad_s2_bf16(const float *dy, const float *w, float *dx, int n, int h, int wd, int c, int k,
                          int r, int s, int pad_h, int pad_w, int accumulate, float *wsub, hipStream_t stream);

/* ---- BatchNorm / ReLU / residual / up-path / Adam (HBM-bound NHWC elementwise) -------- *
 * Replace nn.BatchNorm2d (SyncBatchNorm via operators/rrnet_operator.py:27) + ReLU + residual
 * add of backbones/hourglass.py:18-19,22,26,34-40,51,59-60 and backbones/resnet.py:23-50;
 * nn.Upsample x2 + bilinear(align_corners) resize + add of backbones/hourglass.py:113,121-124;
 * F.adaptive_avg_pool2d of detectors/fasterrcnn_detector.py:15; optim.Adam of
 * operators/rrnet_operator.py:29,138.  `total` = element count, `c` = channels (NHWC inner).
 * Training statistics: rr_conv_fprop's slab -> rr_bn_reduce_slab (adds into a zeroed) sums[2][c] (the SyncBN
 * exchange all-reduces exactly this buffer plus the sample count) -> rr_bn_finalize ->
 * mean/invstd (saved for backward), scale/shift (for rr_bn_apply), running stats updated with
 * `momentum` and the unbiased variance, num_batches_tracked (optional int64 counter) incremented.
 * rr_bn_apply: out = relu?(y*scale+shift [+ res | + res*res_scale+res_shift]).
 *   Its ReLU hands a NaN on (v <= 0 ? 0 : v), as ATen's does: a poisoned statistic stays visible in the activation.
 * rr_bn_bwd_reduce: sums[2][c] = per-channel sum(dy), sum(dy*xhat), dy = dz*(z>0) if z; with z NULL and
 *   mask_scale/mask_shift given the ReLU mask is recomputed as (y*scale+shift > 0) — layers without a
 *   residual input need not re-read their output.  sums_zeroed != 0: the caller hands in zeroed sums (the host
 *   layer takes them from one pre-zeroed pool: 163 memset launches per step less).
 * rr_bn_bwd_apply: dx = gamma*invstd*(dy - sums0/count - xhat*sums1/count); g_out (optional)
 *   receives dy for the residual branch; dgamma/dbeta (optional) are accumulated from sums.
 *   `count_dev` (optional, both finalize and bwd_apply): sample count read from device memory
 *   instead of `count` — the SyncBN exchange all-reduces it next to the sums.
 * rr_sum_n: out = (sum of n<=8 tensors) * (z>0 if z): gradient fan-in of a multiply-used tensor.
 * rr_bias_relu_bwd: dy_masked = dy*(z>0) (if z), dbias += column sums (conv+bias+ReLU heads,
 *   detectors/centernet_detector.py:85-93).
 * rr_upsample_add: out[n,h,w] = up1[n,h,w] + bilinear_ac(nearest2x(low))[h,w]; the exact 2x
 *   case never builds the intermediate image. */
int rr_bn_reduce_slab(const double *slab, int mtiles, int c, double *sums, hipStream_t stream);
int rr_bn_finalize(const double *sums, double count, const double *count_dev, const float *gamma, const float *beta,
                   float *running_mean, float *running_var, float momentum, float eps, float *mean,
                   float *invstd, float *scale, float *shift, int c, long *num_batches_tracked, hipStream_t stream);
/* SyncBN (data parallel; /root/reference/operators/distributed_wrapper.py:40-61 converts every BatchNorm): the three small steps
 * around a statistics exchange without extra launches.  rr_bn_reduce_slab_count = rr_bn_reduce_slab that also stores the local
 * sample count into *count_slot (a slot of the buffer that goes through the all-reduce);  rr_bn_finalize_count = rr_bn_finalize
 * with the (exchanged) count read from the device and copied to *count_out for the backward;  rr_bn_affine_grad adds the LOCAL
 * BatchNorm-backward sums into dbeta / dgamma before they are exchanged. */
int rr_bn_reduce_slab_count(const double *slab, int mtiles, int c, double *sums, double count, double *count_slot,
                            hipStream_t stream);
int rr_bn_finalize_count(const double *sums, const double *count_dev, const float *gamma, const float *beta,
                         float *running_mean, float *running_var, float momentum, float eps, float *mean,
                         float *invstd, float *scale, float *shift, int c, long *num_batches_tracked,
                         double *count_out, hipStream_t stream);
int rr_bn_affine_grad(const double *sums, float *dgamma, float *dbeta, int c, hipStream_t stream);
/* rr_bn_reduce_slab + rr_bn_finalize in one launch, for the single-process case (no SyncBN exchange of the sums in
 * between); fixed summation order (no atomics). */
int rr_bn_stats_finalize(const double *slab, int mtiles, double count, const float *gamma, const float *beta,
                         float *running_mean, float *running_var, float momentum, float eps, float *mean,
                         float *invstd, float *scale, float *shift, int c, long *num_batches_tracked,
                         hipStream_t stream);
int rr_bn_eval_coeffs(const float *gamma, const float *beta, const float *running_mean,
                      const float *running_var, float eps, float *scale, float *shift, int c,
                      hipStream_t stream);
int rr_bn_apply(const float *y, const float *scale, const float *shift, const float *res,
                const float *res_scale, const float *res_shift, float *out, long total, int c, int relu,
                hipStream_t stream);
/* rr_bn_apply that also leaves max |out| (bit pattern, atomicMax into the zeroed word *amax_out): the operand scale of
 * the split-operand convolution that consumes `out` (rr_conv_*_f16x3) without a pass of rr_absmax_bits. */
int rr_bn_apply_amax(const float *y, const float *scale, const float *shift, const float *res,
                     const float *res_scale, const float *res_shift, float *out, long total, int c, int relu,
                     unsigned *amax_out, hipStream_t stream);
/* c % 4 == 0; up to 1024 channels one workgroup covers every channel of its pixels, wider layers (backbones/resnet.py:69, the
 * 2048-channel stage) run in chunks of 1024 channels. */
int rr_bn_bwd_reduce(const float *dz, const float *z, const float *y, const float *mean,
                     const float *invstd, const float *mask_scale, const float *mask_shift, double *sums,
                     long npix, int c, int sums_zeroed, hipStream_t stream);
int rr_bn_bwd_apply(const float *dz, const float *z, const float *y, const float *mean,
                    const float *invstd, const float *gamma, const float *mask_scale, const float *mask_shift,
                    const double *sums, double count,
                    const double *count_dev, float *dx, float *g_out, float *dgamma, float *dbeta, long total,
                    int c, hipStream_t stream);
/* rr_bn_bwd_apply whose masked gradient (the residual branch's share, g) is ADDED into g_acc — the fan-in buffer of the
 * residual's fan-out when another consumer already left its gradient there (one read-modify-write instead of a write,
 * an add kernel and its three passes). */
int rr_bn_bwd_apply_gacc(const float *dz, const float *z, const float *y, const float *mean,
                    const float *invstd, const float *gamma, const float *mask_scale, const float *mask_shift,
                    const double *sums, double count,
                    const double *count_dev, float *dx, float *g_acc, float *dgamma, float *dbeta, long total,
                    int c, hipStream_t stream);
/* rr_bn_bwd_apply / rr_bn_bwd_apply_gacc (g_accumulate) that also leave max |dx| in the zeroed word *amax_dx (see
 * rr_bn_apply_amax): dx is the operand of the data / weight gradients of the convolution in front of the BatchNorm. */
int rr_bn_bwd_apply_amax(const float *dz, const float *z, const float *y, const float *mean,
                         const float *invstd, const float *gamma, const float *mask_scale, const float *mask_shift,
                         const double *sums, double count, const double *count_dev, float *dx, float *g_out,
                         int g_accumulate, float *dgamma, float *dbeta, long total, int c, unsigned *amax_dx,
                         hipStream_t stream);
int rr_relu_fwd(const float *x, float *out, long total, hipStream_t stream);
/* [npix][k] -> [npix][kp], channels k..kp-1 zero (kp a multiple of 4): the 10- / 2-channel gradients of the hm / offset
 * heads' last 1x1 convolutions (detectors/centernet_detector.py:14-16) enter the vector data-gradient kernel as 12 / 4
 * channels.  (A strided torch copy into a channel slice took 3.6 ms per head at 8x256x256 — 10.8 ms of a 457 ms step.) */
int rr_pad_channels(const float *src, float *dst, long npix, int k, int kp, hipStream_t stream);
int rr_sum_n(const float *const *grads, int n, const float *z, float *out, long total, hipStream_t stream);
int rr_bias_relu_bwd(const float *dy, const float *z, float *dy_masked, float *dbias, long npix, int c,
                     hipStream_t stream);
int rr_upsample_add_fwd(const float *up1, const float *low, float *out, int n, int h, int w, int lh, int lw,
                        int c, hipStream_t stream);
int rr_upsample_add_bwd(const float *dout, float *dlow, int n, int h, int w, int lh, int lw, int c,
                        hipStream_t stream);
/* Bilinear resize with align_corners = True (operators/rrnet_operator.py:263, the multi-scale evaluation's
 * F.interpolate); x NHWC [n,h,w,c] -> out NHWC [n,oh,ow,c]. */
int rr_resize_bilinear_ac(const float *x, float *out, int n, int h, int w, int oh, int ow, int c, hipStream_t stream);
int rr_avgpool_fwd(const float *x, float *out, long r, int hw, int c, hipStream_t stream);
int rr_avgpool_bwd(const float *dout, float *dx, long r, int hw, int c, hipStream_t stream);
/* Inference tail of the stage-2 head (backbones/resnet.py:48-53 + detectors/fasterrcnn_detector.py:15):
 * out[r,c] = mean over the hw positions of relu(y[r,p,c]*scale[c] + shift[c] + res[r,p,c]); y, res NHWC [r,hw,c]. */
int rr_bn_res_relu_avgpool(const float *y, const float *scale, const float *shift, const float *res, float *out,
                           long r, int hw, int c, hipStream_t stream);
/* 1x1 convolution to at most 64 output channels on many rows (the stage-2 head's conv1, backbones/resnet.py:33-35 through
 * detectors/fasterrcnn_detector.py:17-18, at inference on R*9 RoI rows): y[m][n] = relu?(x[m][:] . w[n][:] + bias[n]), x [M][K]
 * (K = 128 or 256, M*K*4 < 2 GiB), w [N][K], y [M][N].  Weights live in registers, rows stream through persistent workgroups. */
int rr_conv1x1_rows(const float *x, const float *w, const float *bias, float *y, long m, int k, int n, int relu,
                    hipStream_t stream);
/* The same tail with the 1x1 convolution in front of it fused in (inference): out [r, n] = mean over the hw rows of a
 * RoI of relu((h [r*hw, k] x w [n, k]^T) * scale + shift + res [r*hw, n]); the convolution's output never reaches
 * HBM.  k = 32 or 64, n a multiple of 4 and <= 256 (backbones/resnet.py:46-53 with planes = 64,
 * fasterrcnn_detector.py:15). */
int rr_conv1x1_bn_res_relu_avgpool(const float *h, const float *w, const float *scale, const float *shift,
                                   const float *res, float *out, long r, int hw, int k, int n, hipStream_t stream);
/* WH head, detectors/centernet_detector.py:26-77 (HCov k x 1 and WCov 1 x k to one channel each,
 * interleaved [W,H]): t [n,h,w,ct] (ct >= 2k, a multiple of 4 keeps the vector conv paths) = 1x1
 * convolution of the 256-channel map with the 2k tap vectors (rows 0..k-1 = HCov taps, k..2k-1 = WCov
 * taps, the rest zero; computed by rr_conv_fprop); out [n,h,w,2]:
 * out[..,0] = bias_w + sum_s t[h, w+s-k/2, k+s], out[..,1] = bias_h + sum_r t[h+r-k/2, w, r]. */
int rr_wh_shift_sum_fwd(const float *t, const float *bias_w, const float *bias_h, float *out, int n, int h,
                        int w, int k, int ct, hipStream_t stream);
int rr_wh_shift_sum_bwd(const float *dout, float *dt, int n, int h, int w, int k, int ct, hipStream_t stream);
/* torch.optim.Adam's fp32 update: lr, betas in double; 1 - beta and the bias corrections 1 - beta^step are formed in
 * double and rounded once (step counts from 1). */
int rr_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, long n, double lr,
                 double beta1, double beta2, float eps, int step, float grad_scale, hipStream_t stream);
/* Copy and fingerprint of a training-state buffer in one pass (full-state checkpoints, rrnet_amd/checkpoint.py).
 * src: n fp32 words; dst: n words, or NULL = digest only; chunk: elements per digest record, positive and a multiple of
 * 4; digest: ceil(n / chunk) records of three 64-bit words, written, not accumulated.  With u_j the bit pattern
 * (unsigned 32-bit) of element c*chunk + j, the record of chunk c is
 *   d0 = sum u_j mod 2^64,   d1 = sum (j+1) * u_j mod 2^64,   d2 = #{ j : (u_j & 0x7f800000) == 0x7f800000 } (NaN, +-Inf).
 * Integer sums: the digest is the same for every grid and wave layout; d1 makes it sensitive to position.
 * dst receives the bits of src unchanged (copied as integers: NaN payloads, -0.0, denormals); words of dst beyond n
 * are not written.  src and dst must be 16-byte aligned.  n >= 0; n == 0 launches nothing and succeeds. */
int rr_state_snapshot(const float *src, float *dst, long n, long chunk, unsigned long long *digest, hipStream_t stream);
/* The guarded optimiser step (csrc/optim.hip): gradient-norm clipping, a skip on non-finite gradients and an
 * exponential moving average (EMA) of the weights, decided and applied on the device; the host never reads `ctl` to run a
 * step.  Three launches on one stream: rr_grad_norm, rr_guard_decide, rr_adam_step_guarded.
 *
 * rr_grad_norm: grad holds n fp32 words, n % 4 == 0, 16-byte aligned; n == 0 launches nothing.  The grid is
 *   rr_grad_norm_blocks(n) workgroups of RR_GRAD_NORM_THREADS lanes, a function of n alone and capped: the host sizes
 *   partial [blocks] (double) and bad [blocks] (int) from it.  Global lane t of T = blocks * RR_GRAD_NORM_THREADS visits the
 *   16-byte vectors t, t + T, t + 2T, ... and adds the squares of their words, in index order, in double (a float squared
 *   is exact in double); a word with (bits & 0x7f800000) == 0x7f800000 (NaN, +-Inf) is counted and adds 0, so the sum
 *   stays finite.  Lanes are added by an xor butterfly over the wave (offsets 32, 16, ..., 1), the four waves in order.
 *   partial[b] and bad[b] are written, not accumulated.  No atomics: a run repeats bit for bit.
 * rr_guard_decide: one workgroup.  Lane t adds partial[t], partial[t + RR_GRAD_NORM_THREADS], ... in order, then the same
 *   butterfly -> S; B = sum of bad.  blocks <= the cap of rr_grad_norm_blocks; blocks == 0 means S = 0, B = 0.  ctl holds
 *   RR_GUARD_CTL_WORDS doubles (a fresh record: all 0 except beta1_pow = beta2_pow = 1):
 *     0 applied     steps applied so far              10 step_size  lr / (1 - beta1_pow)
 *     1 skipped     steps skipped so far              11 bc2_sqrt   sqrt(1 - beta2_pow)
 *     2 clipped     steps clipped so far              12 ema_d      EMA decay of this step
 *     3 beta1_pow   running product of beta1          13 ema_omd    1 - that decay
 *     4 beta2_pow   running product of beta2          14, 15        zero
 *     5 norm        this step's gradient norm         16 b1         (float)beta1
 *     6 norm_max    largest finite norm seen          17 omb1       (float)(1 - beta1)
 *     7 bad         non-finite words of this step     18 b2         (float)beta2
 *     8 skip        0 or 1                            19 omb2       (float)(1 - beta2)
 *     9 scale       factor applied to the gradient
 *   Slots 9-13 and 16-19 hold values already rounded to float (the record was widened from 16 words for the four beta
 *   floats that rr_adam_step_guarded needs).  All in double, every operation rounded on its own (no fused multiply-add):
 *     norm = sqrt(S) * grad_scale, or +inf when B > 0;   skip = skip_nonfinite && (B > 0 || !isfinite(norm)).
 *     skip: skipped += 1; bad, norm and skip are written; nothing else changes.
 *     otherwise: coef = 1 when max_norm is +inf or norm is not finite, else min(1, max_norm / (norm + 1e-6))
 *       (torch.nn.utils.clip_grad_norm_); clipped += (coef < 1); scale = (float)(grad_scale * coef); applied += 1;
 *       beta1_pow *= beta1; beta2_pow *= beta2 (running products: a skipped step does not advance Adam's bias correction,
 *       and a host restatement is exact); step_size = (float)(lr / (1 - beta1_pow)); bc2_sqrt = (float)sqrt(1 - beta2_pow);
 *       d = ema_decay, or with ema_warmup min(ema_decay, (1 + applied) / (10 + applied)) with the new `applied`;
 *       ema_d = (float)d; ema_omd = (float)(1 - d); norm_max = max(norm_max, norm) when norm is finite.
 *   grad_scale finite and > 0; max_norm > 0 (+inf: no clipping); betas in [0, 1); ema_decay in [0, 1].
 * rr_adam_step_guarded: every lane reads ctl with ordinary loads.  skip != 0: returns with param, exp_avg, exp_avg_sq and
 *   ema untouched bit for bit.  Otherwise rr_adam_step's arithmetic with scale, step_size, bc2_sqrt and the four beta
 *   floats from ctl, and with ema != NULL  ema = ema * ema_d + param_new * ema_omd  in the same pass.  n % 4 == 0, every
 *   buffer 16-byte aligned. */
#define RR_GUARD_CTL_WORDS 20
#define RR_GRAD_NORM_THREADS 256
int rr_grad_norm_blocks(long n);
int rr_grad_norm(const float *grad, long n, double *partial, int *bad, hipStream_t stream);
int rr_guard_decide(const double *partial, const int *bad, int blocks, double grad_scale, double max_norm,
                    int skip_nonfinite, double lr, double beta1, double beta2, double ema_decay, int ema_warmup,
                    double *ctl, hipStream_t stream);
int rr_adam_step_guarded(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, float *ema,
                         long n, float eps, const double *ctl, hipStream_t stream);

/* ---- losses --------------------------------------------------------------------------- *
 * rr_focal_loss_fwd/bwd: clamp(sigmoid(x),1e-4,1-1e-4) + focal_loss_for_hm of
 *   operators/rrnet_operator.py:55-57 + modules/loss/functional.py:25-51.  logits and gt share
 *   one layout; sums[3] (double, device) = { sum log(p)(1-p)^2 [g==1], sum log(1-p)p^2(1-g)^4
 *   [g<1], #(g==1) }; loss = -(s0+s1)/s2, or -s1 when s2 == 0.  bwd: dlogits = *gout * gscale *
 *   dloss/dlogits (gout: device scalar).
 * rr_regl1_fwd/bwd: modules/loss/regl1loss.py:9-17.  pred NHWC [b,hw,c]; mask, ind [b,m] float;
 *   target [b,m,c]; sums = { sum|pred*m - t*m|, sum of the expanded mask }; loss = s0/(s1+1e-4).
 *   bwd zeroes dpred [b,hw,c] and scatters with float atomics.
 * rr_stage2_loss: operators/rrnet_operator.py:63-102 — per RoI max IoU (torchvision box_iou
 *   definition) against gt [b,g,gstride>=4] xyxy, positives IoU > 0.5, Faster-RCNN targets with
 *   the +1 width convention, smooth-L1 mean per image / b; images without positives add 0.
 *   rois [r,5] = (image, x1,y1,x2,y2) in feature coords, scaled by `scale`.  Outputs: tgt [r,4],
 *   pos [r], npos [b], loss[0] (double), dreg_unit [r,4] = dloss/dreg, droi_unit [r,4] (optional) =
 *   dloss/droi — the reference's smooth-L1 also differentiates its TARGETS, which depend on the boxes
 *   (rrnet_operator.py:82 with the hard-NMS-selected boxes of models/rrnet.py:70). */
int rr_focal_loss_fwd(const float *logits, const float *gt, long n, double *sums, hipStream_t stream);
int rr_focal_loss_bwd(const float *logits, const float *gt, long n, const double *sums, const float *gout,
                      float gscale, float *dlogits, hipStream_t stream);
int rr_regl1_fwd(const float *pred, const float *mask, const float *ind, const float *target, int b, int m,
                 int c, long hw, double *sums, hipStream_t stream);
int rr_regl1_bwd(const float *pred, const float *mask, const float *ind, const float *target, int b, int m,
                 int c, long hw, const double *sums, const float *gout, float gscale, float *dpred,
                 hipStream_t stream);
int rr_stage2_loss(const float *rois, const float *reg, int r, const float *gt, int b, int g, int gstride,
                   float scale, float *tgt, int *pos, int *npos, double *loss, float *dreg_unit,
                   float *droi_unit, hipStream_t stream);

/* ---- decode / NMS plumbing ------------------------------------------------------------ *
 * rr_decode_topk: models/rrnet.py:93-138 (_topk + gathers + transform_bbox).  hm NHWC
 *   [b,h,w,c] logits (is_logits=1: sigmoid applied) or ready scores (0); wh, off NHWC [b,h,w,2];
 *   out [b,k,6] = x1,y1,x2,y2,score,cls in feature coordinates, score-descending, ties by the
 *   reference's flat index; pix_out (optional) [b,k] = y*w+x of every row.  rr_roi_provenance maps
 *   packed RoIs back to that pixel; rr_proposal_bwd is the backward of the box assembly (d wh, d off maps
 *   from d roi).  k <= min(4096, c*h*w).  peak_filter=1 applies operators/centernet_operator.py:204-210
 *   (`_ctnet_nms`: keep a score only where it equals its 3x3 window maximum, dead code in the reference, named by
 *   north_star) INSIDE the scan: only the candidates above the sampled threshold are tested, no extra pass over
 *   the map; rr_peak3x3 writes the filtered score map itself (is_logits=0: hm holds
 *   ready scores, the reference's call form `_ctnet_nms(heat)`).  workspace (optional, rr_decode_workspace_bytes(b)
 *   bytes of device memory): with it, maps of >= 64 K elements are scanned by all CUs (threshold kernel -> streaming
 *   candidate scan -> one workgroup per frame for sort + box assembly); without it one workgroup per frame does
 *   everything.  Both give identical rows.  box_mode 0: RRNet rows as above (scale unused); box_mode 1: CenterNet
 *   rows of operators/centernet_operator.py:152-178 = (x, y, w, h) * scale, score, cls+1, wh NOT clamped.
 * rr_group_by_class: stable regrouping of each image's k rows by class (classes ascending =
 *   torch.unique order of models/rrnet.py:59); seg_off [b*num_classes+1] row offsets.  Rows whose class lies
 *   outside [cls_base, cls_base+num_classes) are dropped and leave a gap at the end of the image's k-row block, so
 *   seg_off[s+1]-seg_off[s] over-counts the image's last class by the gap: seg_len (optional, [b*num_classes]) holds
 *   the exact lengths and is what the NMS entries should be given (rr_hard_nms_segments, rr_soft_nms_ragged).
 * rr_hard_nms_segments: torchvision.ops.nms as called at models/rrnet.py:69,78; rows of a
 *   segment score-descending, 6 floats per row; kept rows are compacted to the segment front.  seg_len NULL:
 *   lengths from consecutive offsets.
 * rr_pack_segments: phase 0 -> out_off [nseg+1] exclusive prefix of n_out (out_off[nseg] = R);
 *   phase 1 -> rois [R,5], scores [R], clses [R] (models/rrnet.py:37-49) and/or rows6 [R,6]. */
size_t rr_decode_workspace_bytes(int b);
int rr_decode_topk(const float *hm, int is_logits, int peak_filter, const float *wh, const float *off, int b,
                   int h, int w, int c, int k, int box_mode, float scale, float *out, int *pix_out, void *workspace,
                   size_t workspace_bytes, hipStream_t stream);
int rr_roi_provenance(const float *rois, const float *scores, const float *clses, int r, const float *decoded,
                      const int *pix, int k, int *roi_pix, hipStream_t stream);
int rr_proposal_bwd(const float *droi, const float *rois, const int *roi_pix, int r, const float *wh, int b, int h,
                    int w, float *dwh, float *doff, hipStream_t stream);
int rr_peak3x3(const float *hm, int is_logits, float *scores, int b, int h, int w, int c, hipStream_t stream);
int rr_group_by_class(const float *boxes, int b, int k, int num_classes, int cls_base, float *grouped,
                      int *seg_off, int *seg_len, hipStream_t stream);
int rr_hard_nms_segments(float *boxes, const int *seg_off, const int *seg_len, int nseg, int max_seg_boxes,
                         float thresh, int *n_out, hipStream_t stream);

/* ---- the reference's own hard-NMS family: ext/nms/nms/nms_kernel.cu (`_nms`), cpu_nms.pyx:129-176, py_cpu_nms.py,
 * bound by ext/nms/nms_wrapper.py:23-33 `nms(dets, thresh, gpu_id)`.  Legacy "+1" IoU; boxes [n,stride>=4] on the
 * device, already score-descending; inclusive = 0 suppresses at IoU > thresh (nms_kernel.cu:71, py_cpu_nms.py:29),
 * 1 at IoU >= thresh (cpu_nms.pyx:170).  keep [n] (device) receives the kept row indices in order, *num_out their
 * count; workspace = rr_nms_workspace_bytes(n) bytes (the n x ceil(n/64) suppression bit matrix).
 * `_nms` is the reference's C entry itself (gpu_nms.hpp:1-2): host pointers, synchronous, own scratch. */
size_t rr_nms_workspace_bytes(int n);
int rr_nms_sorted(const float *boxes, int n, int stride, float thresh, int inclusive, void *workspace,
                  int *keep, int *num_out, hipStream_t stream);
void _nms(int *keep_out, int *num_out, const float *boxes_host, int boxes_num, int boxes_dim,
          float nms_overlap_thresh, int device_id);
/* rr_nms_frames: rr_nms_sorted for all frames of a batch, no host read in between.  rows6 = the packed, score-descending
 *   x,y,w,h,score,cls rows of rr_sort_frames_by_score(out_off, xyxy = 0); frame f occupies rows frame_off[f] ..
 *   frame_off[f+1] (int32 [nframes+1], device).  The kernel forms x2 = x + w, y2 = y + h in float32 itself.
 *   keep[frame_off[f] + j] = the j-th kept row index, local to the frame and ascending: the indices rr_nms_sorted returns
 *   for that frame alone; kept[f] their number.  rows6 and keep hold at least nframes * max_rows rows; max_rows <=
 *   RR_DETECT_MAX_ROWS is checked on the host, a frame length outside [0, max_rows] or a first row outside that space is
 *   clamped on the device.  workspace = rr_nms_frames_workspace_bytes(nframes, max_rows) bytes: one max_rows x
 *   ceil(max_rows / 64) word suppression matrix per frame.
 * rr_pack_frames: the kept rows back to back: out6[out_off[f] + j] = row keep[frame_off[f] + j] of frame f, j < kept[f];
 *   out_off [nframes+1] = exclusive prefix of kept, written by the same launch; rows beyond out_rows are not written. */
size_t rr_nms_frames_workspace_bytes(int nframes, int max_rows);
int rr_nms_frames(const float *rows6, const int *frame_off, int nframes, int max_rows, float thresh, int inclusive,
                  void *workspace, int *keep, int *kept, hipStream_t stream);
int rr_pack_frames(const float *rows6, const int *frame_off, const int *keep, const int *kept, int nframes, int max_rows,
                   float *out6, long out_rows, int *out_off, hipStream_t stream);
int rr_pack_segments(const float *grouped, const int *seg_off, const int *n_out, int nseg, int segs_per_image,
                     int *out_off, float *rois, float *scores, float *clses, float *rows6, int phase,
                     hipStream_t stream);

/* ---- training targets ------------------------------------------------------------ *
 * rr_ctnet_targets: datasets/transforms/functional.py:177-262 (gaussian_radius, gaussian2d, draw_umich_gaussian,
 *   to_heatmap) + the zero padding of datasets/drones_det.py:70-94 (collate_fn_ctnet) for a whole batch.
 *   annos [b,m,anno_stride>=6] = x,y,w,h,score,cls(1-based),.. in image pixels (rows >= counts[i] are padding),
 *   counts [b] int32.  Outputs: hm NHWC [b,img_h/sf,img_w/sf,num_classes] (zeroed here), wh [b,m,2] = (w,h)/sf,
 *   ind [b,m] = cy_int*(img_w/4)+cx_int as float, offset [b,m,2], reg_mask [b,m] (0/1 floats). */
int rr_ctnet_targets(const float *annos, const int *counts, int b, int m, int anno_stride, int img_h, int img_w,
                     int scale_factor, int num_classes, float *hm, float *wh, float *ind, float *offset,
                     float *reg_mask, hipStream_t stream);

/* ---- training input: device-side augmentation ------------------------------------------------- *
 * rr_augment_frames: the pixel half of the training chain of configs/rrnet_config.py:40-49 for frames FillDuck does not
 *   paste into (those go through rr_augment_frames_pasted below), one gather per output pixel: MultiScale (datasets/transforms/functional.py:72-82, PIL `Image.resize(..., BILINEAR)` for scale
 *   factors >= 1), ToTensor (:32-38), MaskIgnore (:290-313), HorizontalFlip (:13-19), RandomCrop's padding and crop
 *   (datasets/transforms/transforms.py:60-72, functional.py:104-111) and Normalize (functional.py:135-143).  Bit-exact
 *   with that chain on the host.
 *   src [src_bytes] uint8: one HWC RGB source WINDOW per image, back to back (only the rows and columns a crop reads).
 *   params [b, RR_AUGMENT_PARAMS] int32 per image: source height, width; window origin y, x; window height, width;
 *     scaled height, width = int(h*s), int(w*s); flip flag; crop origin y, x in the scaled, flipped, padded frame; byte
 *     offset of the window in src (low, high word); first row of the vertical and of the horizontal tap table in taps;
 *     one reserved word.
 *   rects [*,4] int32 = y0, y1, x0, x1: ignore rectangles in scaled, pre-flip coordinates (half open);
 *     rect_off [b+1] int32: image i owns rows [rect_off[i], rect_off[i+1]).  rects may be NULL when there is none.
 *   taps [ntaps,3] int32 = first tap, k0, k1 per output coordinate: PIL's fixed-point coefficients (22 bits) of one
 *     resize pass, source coordinates in the FULL frame.
 *   mean, stdv [3] float.  out [b,out_h,out_w,3] float NHWC, 16-byte aligned.  Pixels right of / below the scaled
 *   frame are padding: (0 - mean) / std. */
#define RR_AUGMENT_PARAMS 16
int rr_augment_frames(const unsigned char *src, long src_bytes, const int *params, const int *rects,
                      const int *rect_off, const int *taps, int ntaps, const float *mean, const float *stdv,
                      float *out, int b, int out_h, int out_w, hipStream_t stream);

/* rr_augment_frames_pasted: the same chain WITH FillDuck between MaskIgnore and HorizontalFlip (datasets/transforms/
 *   transforms.py:173-179, functional.py:356-523: crop an object, F.interpolate(mode='bilinear', align_corners=True),
 *   slice-assign it elsewhere in the frame, :438-452 and :486-501).  The host decides every paste (datasets/transforms/
 *   functional.py fill_duck_decide here); the device does the pixels in three stages: `canvas` (the scaled, masked,
 *   un-flipped frame as fp32 = (float)v / 255.0f; the float32 mean inside ignore rectangles), `paste` (one workgroup per
 *   frame walks its list in order; all reads of a paste come before its writes, later pastes see earlier ones) and
 *   `finish` (crop, 0 padding, un-flip, (x - mean) / std).  Pixels no paste wrote are bit-identical to rr_augment_frames;
 *   a pasted pixel is l0*(m0*a + m1*b) + l1*(m0*c + m1*d) with torch's source indices and weights (r = rheight*(float)oy,
 *   y0 = (int)r, l1 = r - y0, l0 = 1 - l1; likewise x), within float32 rounding of torch's value.
 *   src, params, rects, rect_off, taps, mean, stdv, out, b, out_h, out_w: as rr_augment_frames, except that a frame
 *     with pastes ships a window that covers every source pixel (the whole frame).
 *   pastes [*, RR_PASTE_WORDS] int32 = source rectangle y, x, h, w; destination y, x; object h, w (all inside the scaled
 *     frame); the float32 bit patterns of rheight = (h-1)/(object h-1) and rwidth (0 for a 1-pixel object axis); two
 *     reserved words.  paste_off [b+1] int32: frame i owns rows [paste_off[i], paste_off[i+1]).
 *   canvas [b, canvas_stride, 3] float, 16-byte aligned, canvas_stride (pixels, a multiple of 4) >= every frame's
 *     scaled height * width; scratch [b, scratch_stride, 3] float, scratch_stride (pixels) >= every object's h * w.  A
 *     frame or object that does not fit is skipped, never written out of bounds.
 *   stages: mask of 1 (canvas), 2 (paste), 4 (finish); 7 is the whole chain (the others exist to time one stage). */
#define RR_PASTE_WORDS 12
int rr_augment_frames_pasted(const unsigned char *src, long src_bytes, const int *params, const int *rects,
                             const int *rect_off, const int *taps, int ntaps, const int *pastes, const int *paste_off,
                             const float *mean, const float *stdv, float *canvas, long canvas_stride, float *scratch,
                             long scratch_stride, float *out, int b, int out_h, int out_w, int stages,
                             hipStream_t stream);

/* ColorJitter in front of the chain (datasets/transforms/transforms.py:120-130, functional.py:159-174: PIL's
 *   ImageEnhance.Brightness, Contrast, Color on the uint8 frame, before MultiScale).  Each stage is PIL's Image.blend,
 *   float32  t = (float)d + alpha*(float)(v - d)  (a multiply, then an add), 0 at t <= 0, 255 at t >= 255, truncated
 *   otherwise, with d = 0 (brightness), d = m, the rounded grey mean of the brightness-adjusted WHOLE frame (contrast),
 *   d = L of the pixel itself (colour); L = (r*19595 + g*38470 + b*7471 + 0x8000) >> 16.  Bit-exact with PIL.
 *   PRECONDITION of all three entries: every frame ships its whole source frame as its window (window origin 0, 0;
 *   window height, width = source height, width), because m is a mean over the whole frame.
 * rr_jitter_gray_mean: for every frame i, sums[i] = the integer sum of L over the frame after brightness factors[i,0]
 *   (zeroed here on the stream, one 64-bit integer atomic per workgroup: the same words run to run) and
 *   gray_mean[i] = (2*sums[i] + N) / (2*N), N the frame's pixels = int(mean + 0.5) as PIL forms it.
 *   src, src_bytes, params: as rr_augment_frames.  factors [b,3] float = brightness, contrast, colour factor per frame.
 *   sums [b] 64-bit words (workspace, 8-byte aligned), gray_mean [b] int32.  max_pixels >= every frame's height * width
 *   (it sizes the grid; pixels beyond it would not be summed).  b <= 65535.
 * rr_augment_frames_jitter, rr_augment_frames_pasted_jitter: rr_augment_frames and rr_augment_frames_pasted with the
 *   jitter applied to each of the four source taps before PIL's fixed-point resize (exact, since the jitter precedes the
 *   resize).  factors as above; gray_mean [b] int32 from rr_jitter_gray_mean (clamped to 0..255 where it is read).
 *   Ignore rectangles and padding are what they were: the chain writes them after ToTensor.  Pasted objects read the
 *   jittered canvas.  With factors (1, 1, 1) the results equal the unjittered entries bit for bit. */
int rr_jitter_gray_mean(const unsigned char *src, long src_bytes, const int *params, const float *factors,
                        unsigned long long *sums, int *gray_mean, int b, long max_pixels, hipStream_t stream);
int rr_augment_frames_jitter(const unsigned char *src, long src_bytes, const int *params, const int *rects,
                             const int *rect_off, const int *taps, int ntaps, const float *mean, const float *stdv,
                             const float *factors, const int *gray_mean, float *out, int b, int out_h, int out_w,
                             hipStream_t stream);
int rr_augment_frames_pasted_jitter(const unsigned char *src, long src_bytes, const int *params, const int *rects,
                                    const int *rect_off, const int *taps, int ntaps, const int *pastes,
                                    const int *paste_off, const float *mean, const float *stdv, const float *factors,
                                    const int *gray_mean, float *canvas, long canvas_stride, float *scratch,
                                    long scratch_stride, float *out, int b, int out_h, int out_w, int stages,
                                    hipStream_t stream);

/* ---- inference post-process (config 5: decode -> re-regression -> Soft-NMS) ------------------ *
 * rr_refine_boxes: operators/rrnet_operator.py:188-209 `generate_bbox` (stage-2 boxes from the packed RoIs
 *   [r,5] = image,x1,y1,x2,y2 in feature coordinates, the regression [r,4], scores, classes), the score filter
 *   `pred_bbox[:, 4] > score_thr` (:266-267) and the xywh -> xyxy step of `_ext_nms` (:222-223), for all
 *   (frame, class) segments of a batch in one launch.  seg_off [nseg+1] = row offsets of the stage-1 segments in
 *   the packed list (rr_pack_segments phase 0).  out6 rows = x1,y1,x2,y2,score,cls+1, order preserved, written
 *   to the front of each segment's row range; seg_len [nseg] = rows kept.  Feed to rr_soft_nms_ragged.
 * rr_finalize_frames: `np.concatenate` of the per-class results (:225), xyxy -> xywh (:231) and the final
 *   `torch.sort(score, descending)` (:278-279; ties keep concatenation order) per frame.  out_off [nseg+1] =
 *   exclusive prefix of n_out (rr_pack_segments phase 0); frame f's rows land at out6[out_off[f*segs_per_frame]]. */
int rr_refine_boxes(const float *rois, const float *reg, const float *scores, const float *clses,
                    const int *seg_off, int nseg, float scale, float score_thr, float *out6, int *seg_len,
                    hipStream_t stream);
int rr_finalize_frames(const float *boxes6, const int *seg_off, const int *n_out, const int *out_off,
                       int nframes, int segs_per_frame, int max_frame_boxes, float *out6, hipStream_t stream);
/* rows6 [n,6] -> out6 ordered by score (column 4) descending, ties in input order (operators/rrnet_operator.py:272,
 * 278: the torch.sort calls around _ext_nms in the multi-scale evaluation); n <= 16384, out6 != rows6. */
int rr_sort_rows_by_score(const float *rows6, int n, float *out6, hipStream_t stream);

/* ---- detection on raw frames: the multi-scale evaluation body (operators/rrnet_operator.py:256-279), batched ---- *
 * rr_prepare_frames: frames [n,h,w,3] uint8 RGB -> ToTensor -> Normalize(mean, stdv [3]) -> F.interpolate(bilinear,
 *   align_corners=True) to oh x ow, out [n,oh,ow,3] float NHWC.  Bit-identical to rr_resize_bilinear_ac on the host-
 *   normalised frame ((u8 / 255 - mean) / std in float32).
 * rr_merge_scales: one scale's stage-2 inputs (rois [r,5], reg [r,4], scores, clses [r] as the model returns them;
 *   frame_off [nframes+1] = row range of every frame) -> rows (x, y, w, h, score, cls+1) of `generate_bbox` (scale =
 *   the model's stride, 4), kept when !filter or score > score_thr, x,y,w,h divided by div (IEEE), appended in row
 *   order to frame f's block of merged [nframes,k,6] at count[f]; count [nframes] int32 is advanced on the device.
 *   The caller zeroes count and fills merged's class column with a value outside the class range before the first
 *   scale; one launch per scale, in the order of the concatenation.  k <= RR_DETECT_MAX_ROWS.
 * rr_sort_frames_by_score: per frame, the first count[f] rows of rows6 [nframes,k,6] by score descending, ties in row
 *   order (rr_sort_rows_by_score's keys and network, one workgroup per frame).  out_off NULL: out6 [nframes,k,6],
 *   out_rows = nframes*k, rows behind count[f] are written as padding (class -1).  out_off [nframes+1] (exclusive
 *   prefix of count): out6 [out_rows,6] packed, frame f at row out_off[f].  xyxy != 0 writes x2 = x + w, y2 = y + h
 *   (the step in front of Soft-NMS, :222-223).  out6 != rows6.
 * CenterNet's evaluation body (operators/centernet_operator.py:262-285: every scale once flipped, once plain):
 * rr_prepare_frames_pair: rr_prepare_frames into out [2n,oh,ow,3]: images 0..n-1 are what rr_prepare_frames writes,
 *   images n..2n-1 the same pixels mirrored in x, out[n+i][y][ow-1-x] = out[i][y][x] — the reference resizes first and
 *   flips afterwards (:268-272), so the mirrored image carries the bits of the plain one.
 * rr_merge_ctnet: rows6 [(pair ? 2 : 1)*nframes, k_in, 6] = CenterNet rows (x,y,w,h,score,cls+1) as rr_decode_topk
 *   (box_mode 1) writes them.  Per frame f, appended in order at count[f] as rr_merge_scales does: with pair the rows of
 *   image nframes+f (the flipped one) with x <- (img_w - x) - w (`flip_annos`, two fp32 subtractions; img_w = ow), then
 *   the rows of image f.  A row is kept iff score > score_thr (`transform_bbox` always filters; NaN leaves); x,y,w,h
 *   are each divided by div (IEEE) after the flip; w, h are not clamped.  Rows beyond k are dropped, count[f] <= k.
 *   k <= RR_DETECT_MAX_ROWS; count[f] is clamped to [0,k] before it addresses anything. */
#define RR_DETECT_MAX_ROWS 16384
int rr_prepare_frames(const unsigned char *frames, const float *mean, const float *stdv, float *out, int n, int h,
                      int w, int oh, int ow, hipStream_t stream);
int rr_merge_scales(const float *rois, const float *reg, const float *scores, const float *clses,
                    const int *frame_off, int nframes, int r, float scale, float div, int filter, float score_thr,
                    float *merged, int *count, int k, hipStream_t stream);
int rr_sort_frames_by_score(const float *rows6, const int *count, const int *out_off, int nframes, int k, int xyxy,
                            float *out6, long out_rows, hipStream_t stream);
int rr_prepare_frames_pair(const unsigned char *frames, const float *mean, const float *stdv, float *out, int n, int h,
                           int w, int oh, int ow, hipStream_t stream);
int rr_merge_ctnet(const float *rows6, int nframes, int k_in, int pair, float img_w, float div, float score_thr,
                   float *merged, int *count, int k, hipStream_t stream);
/* Tiled inference (no counterpart in the reference): equal-size overlapping tiles cut out of frames of any size, detected
 * as a batch, and their rows brought back into per-frame blocks.
 * rr_prepare_tiles: frames = one packed byte buffer; frame f is [H_f, W_f, 3] uint8 at byte frame_base[f] (any byte
 *   address), frame_hw [nframes,2] = H_f, W_f.  tiles [ntiles,3] = frame, y0, x0: the th x tw window of that frame at
 *   (y0, x0), which the caller has checked to lie inside it.  Tile t of out [ntiles,oh,ow,3] (float NHWC) equals, bit for
 *   bit, what rr_prepare_frames writes for the host-cropped array frame[y0:y0+th, x0:x0+tw] at output size oh x ow: the taps
 *   are the tile's (sy = (th-1)/(oh-1) or 0, likewise sx) and the "+1" tap stops at the tile's last row / column, not the
 *   frame's.  The kernel clamps the frame index, the origin and every tap to the frame the table names.
 * rr_merge_tiles: rows6 [T,k_in,6] = (x, y, w, h, score, cls) rows per tile in the model's input coordinates (oh x ow),
 *   count_in [T]; tiles as above, sorted by frame, tile_off [nframes+1] = the tile range of every frame (built and
 *   checked by the caller; column 0 of tiles is not read).  Per frame its tiles in table order, of each its first
 *   min(max(count_in[t], 0), k_in) rows in row order; float32 throughout, every operation its own rounding:
 *   margin test (only when margin > 0): a tile side is interior when it is not on the frame's border (left x0 > 0, top
 *     y0 > 0, right x0 + tw < W_f, bottom y0 + th < H_f); the row leaves iff left is interior and x < margin, or top is
 *     interior and y < margin, or right is interior and x + w > (float)ow - margin, or bottom is interior and
 *     y + h > (float)oh - margin.  A NaN makes every comparison false: the row stays.
 *   move: x <- x / div + (float)x0, y <- y / div + (float)y0, w <- w / div, h <- h / div (IEEE division); score and class
 *     are unchanged.
 *   append: the row goes to frame f's block of merged [nframes,k,6] at count[f] (the caller zeroes count); count[f] ends
 *     as the true number of kept rows, also above k; rows at and beyond k are not written, rows between count[f] and k are
 *     left as they were.  k <= RR_DETECT_MAX_ROWS.  One workgroup per frame, no atomics, no dependence on dispatch order. */
int rr_prepare_tiles(const unsigned char *frames, const long long *frame_base, const int *frame_hw, int nframes,
                     const int *tiles, int ntiles, int th, int tw, int oh, int ow, const float *mean, const float *stdv,
                     float *out, hipStream_t stream);
int rr_merge_tiles(const float *rows6, const int *count_in, const int *tiles, const int *tile_off, const int *frame_hw,
                   int nframes, int k_in, int th, int tw, int oh, int ow, float div, float margin, float *merged,
                   int *count, int k, hipStream_t stream);

/* ---- evaluation: VisDrone AP / AR on the device ------------------------------------------------ *
 * rr_eval_match: utils/metrics/metrics.py:51-131 (`get_tp` with its `bbox_iou` calls) for f frames in one launch, one
 *   workgroup per frame.
 *   dets [f,dmax,6] = x,y,w,h,score,cls rows already in evaluation order (score descending) and cut to max_det_num,
 *   det_len [f]; gts [f,gmax,6] = the first six columns of the VisDrone rows (cls == 0: ignored region), gt_len [f];
 *   thresholds [t] (the host's own tensor values, t <= RR_EVAL_MAX_THRESHOLDS).  Lengths are clamped to dmax / gmax.
 *   1. with an ignored region in the frame, a ground truth leaves unless every inter/area(gt) over the ignored regions
 *      is < 0.5 (0.5 leaves; zero area gives 0/0 = NaN and leaves);  2. a detection leaves by the same rule on
 *      inter/area(det);  3. target_count [f,cls_num-1] = ground truths left per class 1..cls_num-1; counted [f,dmax] = 1
 *      for a detection that stayed, has a class in 1..cls_num-1 and meets a ground truth of that class in its frame
 *      (detections of a class the frame does not hold are dropped, not false positives: the reference's rule);
 *   4. greedy matching per class in row order, independently per threshold: the detection takes the ground truth of
 *      largest IoU among those of its class with iou - thr >= 0 not yet taken at that threshold, ties to the lowest
 *      ground-truth index; flag_bits [f,dmax] bit t = true positive at threshold t (0 for rows not counted).
 *   IoU in fp32 in bbox_iou's operation order (:10-49), correctly rounded division, no fused multiply-add: the flags
 *   equal the host's.  gmax <= RR_EVAL_MAX_GT (the frame's ground truth lives in LDS), cls_num <= RR_EVAL_MAX_CLASSES.
 * rr_eval_ap: utils/metrics/metrics.py:133-174 (`calculate_ap_rc`).  flag_bits [nrows]: the counted detections' words
 *   class by class, each class sorted by confidence descending; seg_off [c+1] its row offsets; target_count,
 *   in_img_count [c] summed over the frames.  Per (class, threshold): cumulative true positives, prec = cum/(i+1), rec =
 *   cum/max(count,1) as fp32 quotients, the precision envelope (reverse running maximum, trailing sentinel 0), the sum of
 *   (rec_i - rec_{i-1}) * env_i where recall rises (fp32 terms, summed in double) and the largest recall; then the
 *   in_img_count weighting.  ap [t], rc [1]; classes with target_count 0 are skipped, no class at all gives NaN.
 *   work: 2*c*t floats of device scratch. */
#define RR_EVAL_MAX_GT 2048
#define RR_EVAL_MAX_THRESHOLDS 16
#define RR_EVAL_MAX_CLASSES 64
int rr_eval_match(const float *dets, const int *det_len, const float *gts, const int *gt_len, const float *thresholds,
                  int f, int dmax, int gmax, int t, int cls_num, int *flag_bits, unsigned char *counted,
                  int *target_count, hipStream_t stream);
int rr_eval_ap(const int *flag_bits, long nrows, const int *seg_off, const int *target_count, const int *in_img_count,
               int c, int t, float *work, float *ap, float *rc, hipStream_t stream);

/* ---- RetinaNet: stem pool, FPN upsample-add, anchor criterion, decode (retina.hip) ---------------- *
 * rr_maxpool3x3s2_fwd / _bwd: nn.MaxPool2d(kernel_size=3, stride=2, padding=1) of backbones/resnet.py:65 on NHWC fp32.
 *   x [n,h,w,c] -> y [n,oh,ow,c], oh = (h-1)/2+1, ow = (w-1)/2+1; idx (uint8, y's shape) = the winning tap ky*3+kx of the
 *   window (input row 2*oy-1+ky, column 2*ox-1+kx).  Padding counts as -inf; the first maximum in row-major window order
 *   wins; a NaN replaces the running maximum (ATen's rule).  The backward is a gather: dx [n,h,w,c] = the sum, in window
 *   order, of dy over the at most 4 windows whose tap names the element.  No atomics.
 * rr_bilinear_add_fwd / _bwd: modules/fpn.py:39-40, out = y + F.interpolate(x, size(y), 'bilinear', align_corners=False).
 *   x NHWC [n,ih,iw,c], y and out NHWC [n,oh,ow,c], any sizes.  Source coordinate (dst + 0.5) * in/out - 0.5 (in/out as
 *   one float quotient) clamped at 0, second tap clamped at in-1.  d y is dout itself; _bwd writes d x [n,ih,iw,c] as a
 *   gather over the bounded range of output pixels that read the input pixel, weights recomputed.  No atomics.
 * rr_retina_assign: operators/retinanet_operator.py:51-62,67,76-97.  annos [b,m,8] (x,y,w,h,.,cls,.,.; zero rows are
 *   padding), anchors [a,4] xyxy.  Per (image, anchor): float32 IoU of utils/metrics/metrics.py:29-44 against every row
 *   (x2 = x + w as the criterion's in-place add; union clamped at 1e-8; IEEE division), max_iou / argmax (lowest index on
 *   ties), state int8 = 1 (IoU >= 0.5), 0 (IoU < 0.4), -1 (between), cls = the assigned class of a positive (0 otherwise),
 *   target [b,a,4] = the regression target of a positive (0 otherwise): centres from the unclamped w/h, w/h clamped at 1,
 *   log, divided by (0.1, 0.1, 0.2, 0.2).  npos [b] int32 = positives per image (zeroed inside, integer atomics).
 *   Deviation: a class outside [1, num_classes] gives cls 0, i.e. no target bit (the reference indexes -1 or raises).
 * rr_retina_loss_fwd / _bwd: modules/loss/functional.py:6-22 and retinanet_operator.py:64-72,99-113.  logits [b,a,c],
 *   loc [b,a,4].  losses[0] = mean over images of sum over (state >= 0 anchors x classes) of the focal term (p =
 *   clamp(sigmoid, 1e-7, 1-1e-7), alpha 0.75 on the target bit, 0.25 elsewhere, gamma 2) / max(1, npos); losses[1] =
 *   mean over images of the smooth-L1 (knee 1/9) mean over npos*4 values, 0 for npos == 0.  Two stages: partial
 *   [b, rr_retina_loss_blocks(a,c), 2] doubles written per workgroup, then one workgroup: bit-identical run to run.
 *   _bwd: gout [2] (device) = the two upstream scalars; dlogits [b,a,c] and dloc [b,a,4] are written whole: zero for
 *   ignored anchors, for non-positives in loc and where the probability clamp is active.  npos is clamped to [0,a].
 * rr_retina_decode: retinanet_operator.py:179-213 for a batch.  Per image: sigmoid, max over classes (first maximum),
 *   kept when prob > score_thr (NaN leaves), decoded against the anchors (std 0.1/0.2, exp); rows (x,y,w,h,prob,cls+1)
 *   appended in anchor order to rows [b,a,6], count [b] int32 written on the device.  One workgroup per image. */
int rr_maxpool3x3s2_fwd(const float *x, float *y, unsigned char *idx, int n, int h, int w, int c, hipStream_t stream);
int rr_maxpool3x3s2_bwd(const float *dy, const unsigned char *idx, float *dx, int n, int h, int w, int c,
                        hipStream_t stream);
int rr_bilinear_add_fwd(const float *x, const float *y, float *out, int n, int ih, int iw, int oh, int ow, int c,
                        hipStream_t stream);
int rr_bilinear_add_bwd(const float *dout, float *dx, int n, int ih, int iw, int oh, int ow, int c, hipStream_t stream);
int rr_retina_assign(const float *annos, const float *anchors, int b, int m, int a, int num_classes,
                     signed char *state, int *argmax, float *max_iou, int *cls, float *target, int *npos,
                     hipStream_t stream);
int rr_retina_loss_blocks(int a, int c);
int rr_retina_loss_fwd(const float *logits, const float *loc, const signed char *state, const int *cls,
                       const float *target, const int *npos, int b, int a, int c, double *partial, float *losses,
                       hipStream_t stream);
int rr_retina_loss_bwd(const float *logits, const float *loc, const signed char *state, const int *cls,
                       const float *target, const int *npos, const float *gout, int b, int a, int c, float *dlogits,
                       float *dloc, hipStream_t stream);
int rr_retina_decode(const float *logits, const float *loc, const float *anchors, int b, int a, int c, float score_thr,
                     float *rows, int *count, hipStream_t stream);
/* rr_retina_decode_frames: rr_retina_decode with the anchors of an image spread over workgroups of RR_RETINA_DECODE_CHUNK
 *   anchors.  rows [b,k,6], 0 < k <= a: the first min(count[f], k) rows of frame f are bit for bit the rows rr_retina_decode
 *   writes for that image, in anchor order; count[f] is the true number of candidates also when it exceeds k; rows at and
 *   beyond k are not written, rows between count[f] and k are left untouched.  Two launches ordered by the stream (per-chunk
 *   counts and per-anchor probability / class into the workspace; then every workgroup sums the counts of the chunks in
 *   front of it and writes its rows): no workgroup waits on another.  workspace =
 *   rr_retina_decode_frames_workspace_bytes(b, a) bytes. */
#define RR_RETINA_DECODE_CHUNK 256
size_t rr_retina_decode_frames_workspace_bytes(int b, int a);
int rr_retina_decode_frames(const float *logits, const float *loc, const float *anchors, int b, int a, int c,
                            float score_thr, float *rows, int k, int *count, void *workspace, hipStream_t stream);

/* ---- RoIAlign --------------------------------------------------------------------------- *
 * torchvision.ops.roi_align(feat, rois, (ph,pw)) at models/rrnet.py:51 (spatial_scale 1,
 * sampling_ratio -1, legacy coordinates).  feat NHWC [b,h,w,c]; out NHWC [r,ph,pw,c]. */
int rr_roi_align_fwd(const float *feat, const float *rois, int r, int h, int w, int c, int ph, int pw,
                     float spatial_scale, int sampling_ratio, const int *order, float *out, hipStream_t stream);
/* order (optional, 3x3 bins): processing position -> RoI index; rr_roi_spatial_order builds it per frame (rois of
 * frame f = rows [frame_off[f], frame_off[f+1]) of the packed list) by (8-pixel row band, x centre), so that RoIs with
 * overlapping footprints run back to back on one XCD and share its L2.  Outputs stay in RoI order. */
int rr_roi_spatial_order(const float *rois, const int *frame_off, int nframes, int *order, hipStream_t stream);
int rr_roi_align_bwd(const float *dout, const float *rois, int r, int b, int h, int w, int c, int ph, int pw,
                     float spatial_scale, int sampling_ratio, float *dfeat, hipStream_t stream);

/* ---- Modulated deformable convolution (DCNv2) -- BASELINE config 4 ------------------------- *
 * Replaces ext/dcn: `dcn_v2_forward` / `dcn_v2_backward` of src/vision.cpp:3-8 (src/cuda/dcn_v2_cuda.cu:42-172,
 * 206-335, kernels src/cuda/dcn_v2_im2col_cuda.cu:125-327), bound by ext/dcn/dcn_v2.py:25,40.
 * x NHWC [n,h,w,c]; offset NHWC [n,p,q,2*dg*r*s] (per deformable group: interleaved (dh,dw) per tap);
 * mask NHWC [n,p,q,dg*r*s]; w OHWI [k][r][s][c]; y NHWC [n,p,q,k].
 * rr_dcn_fwd is one fused gather-GEMM (no column buffer).  The backward is assembled by the host layer:
 *   col  = rr_dcn_im2col(x, offset, mask)            [M, r*s*c], M = n*p*q   (rr_dcn_col_bytes)
 *   dw  += rr_conv_wgrad(col as [1,M,1,r*s*c], dy as [1,M,1,k])              (1x1 layer)
 *   dcol = rr_conv_dgrad(dy, w as [k, r*s*c, 1, 1])
 *   rr_dcn_col2im(x, offset, mask, dcol) -> dx (zeroed + float atomics), doffset, dmask
 * Requires c % 4 == 0, c % dg == 0 and (dg == 1 or (c/dg) % 32 == 0).
 * Layers with stride 1, c % 32 == 0 and k > 32 (3x3 for the two gradients) run on kernels that stage the input block an
 * 8x16 pixel tile can reach in LDS (margin RR_DCN_WINDOW, default 3 pixels; offsets beyond it go to global memory);
 * the others on the kernels that gather the bilinear corners from L2.  Same results either way. */
int rr_dcn_fwd(const float *x, const float *offset, const float *mask, const float *w, const float *bias, float *y,
               int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w, int dilation,
               int deformable_groups, hipStream_t stream);
/* Same operation with bf16 matrix operands (samples and weights rounded to bf16 in the kernel, fp32 accumulation on
 * v_mfma_f32_32x32x16_bf16): inputs and outputs stay fp32 tensors.  BASELINE config 4. */
int rr_dcn_fwd_bf16(const float *x, const float *offset, const float *mask, const float *w, const float *bias, float *y,
                    int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w, int dilation,
                    int deformable_groups, hipStream_t stream);
/* rr_dcn_fwd_bf16 with caller scratch for the weights re-packed to bf16 [tap][32-channel chunk][filter][32]
 * (rr_dcn_wpack_bytes(c,k,r,s) bytes, filled inside by one small kernel per call): on the LDS-window kernel with 256-filter
 * tiles the weight operand then goes global -> LDS by buffer_load ... lds (no staging registers, converts or ds_writes).
 * Layers that kernel does not take run exactly as rr_dcn_fwd_bf16. */
size_t rr_dcn_wpack_bytes(int c, int k, int r, int s);
int rr_dcn_fwd_bf16_packed(const float *x, const float *offset, const float *mask, const float *w, const float *bias,
                           float *y, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w,
                           int dilation, int deformable_groups, void *wpack, hipStream_t stream);
size_t rr_dcn_col_bytes(int n, int h, int wd, int c, int r, int s, int stride, int pad_h, int pad_w, int dilation);
int rr_dcn_im2col(const float *x, const float *offset, const float *mask, float *col, int n, int h, int wd, int c,
                  int r, int s, int stride, int pad_h, int pad_w, int dilation, int deformable_groups,
                  hipStream_t stream);
int rr_dcn_col2im(const float *x, const float *offset, const float *mask, const float *dcol, float *dx,
                  float *doffset, float *dmask, int n, int h, int wd, int c, int r, int s, int stride, int pad_h,
                  int pad_w, int dilation, int deformable_groups, hipStream_t stream);

/* Fused backward (no column buffers): rr_dcn_wgrad adds dY^T x (deformed columns produced in registers) into dw
 * (float atomics; dw pre-zeroed or holding the running gradient); rr_dcn_dgrad keeps the column gradient in the MFMA
 * accumulators and writes dx (zeroed inside; window kernels: contributions pre-summed per pixel block in an LDS image
 * in fixed point, one power-of-two scale per block and channel, then one global float atomic per window element;
 * otherwise float atomics on the bilinear corners), doffset and dmask (plain stores).
 * Replace ext/dcn/src/cuda/dcn_v2_cuda.cu:206-335 + dcn_v2_im2col_cuda.cu:197-327.  Layers they do not take
 * (rr_dcn_fused_bwd_supported == 0) go through the column path above. */
/* rr_dcn_wgrad_bf16 with dY's bf16 image (same element order as dy; its producer's image or one rr_to_bf16 pass): the dY
 * operand reaches LDS by buffer_load ... lds, no conversion inside (round 5).  Same results as rr_dcn_wgrad_bf16.
 * Replaces the dW GEMM of dcn_v2_cuda_backward (ext/dcn/src/cuda/dcn_v2_cuda.cu:283-301). */
int rr_dcn_wgrad_bf16_img(const float *x, const float *offset, const float *mask, const float *dy, const unsigned short *dy_bf16,
                          float *dw, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w,
                          int dilation, int deformable_groups, hipStream_t stream);

/* 1 when rr_dcn_wgrad / rr_dcn_dgrad (and their _bf16 forms) take a layer of this shape, 0 when the host layer has to
 * run the column path (rr_dcn_im2col / rr_dcn_col2im + the conv GEMMs). */
int rr_dcn_fused_bwd_supported(int c, int k, int r, int s, int stride, int deformable_groups);      /* dilation 1 */
/* The same query with the dilation: deformable groups of 32 / 64 / 96 channels exist on the LDS-window kernels only, and a
 * dilated filter's window may not fit (3x3 with dilation >= 3: the data-gradient window exceeds 160 KB). */
int rr_dcn_fused_bwd_supported_dil(int c, int k, int r, int s, int stride, int dilation, int deformable_groups);
int rr_dcn_wgrad(const float *x, const float *offset, const float *mask, const float *dy, float *dw, int n, int h,
                 int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w, int dilation,
                 int deformable_groups, hipStream_t stream);
int rr_dcn_dgrad(const float *x, const float *offset, const float *mask, const float *w, const float *dy, float *dx,
                 float *doffset, float *dmask, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h,
                 int pad_w, int dilation, int deformable_groups, hipStream_t stream);
/* rr_dcn_dgrad_bf16 with caller scratch for dY rounded to bf16 (rr_dcn_dyb_bytes(n,p,q,k) bytes, written inside by one
 * pass per call): the K sweep re-reads a block's dY tile once per 32-channel chunk — as bf16 those re-reads stay in L2
 * (64 KB per workgroup instead of 128 KB) and the operand staging needs no convert.  Same results bit for bit. */
size_t rr_dcn_dyb_bytes(int n, int p, int q, int k);
int rr_dcn_dgrad_bf16_ws(const float *x, const float *offset, const float *mask, const float *w, const float *dy, float *dx,
                         float *doffset, float *dmask, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h,
                         int pad_w, int dilation, int deformable_groups, void *dyb, hipStream_t stream);
/* ... with dY's bf16 image already in HBM (written by dY's producer: rr_head_dgrad_relubias / rr_to_bf16): no conversion
 * inside the call.  dy (fp32) is still read by the d offset / d mask side where the column path is taken. */
int rr_dcn_dgrad_bf16_img(const float *x, const float *offset, const float *mask, const float *w, const float *dy,
                          const unsigned short *dy_bf16, float *dx, float *doffset, float *dmask, int n, int h, int wd,
                          int c, int k, int r, int s, int stride, int pad_h, int pad_w, int dilation,
                          int deformable_groups, hipStream_t stream);
/* rr_dcn_dgrad_bf16 with BOTH operands of the column-gradient sweep fed by LDS-DMA (round 5): the weights are packed to
 * bf16 inside the call (the forward's [tap][chunk][filter][32] layout), dY comes as the caller's bf16 image (dy_bf16) or is
 * rounded once into the workspace (dy_bf16 NULL).  ws: rr_dcn_dgrad_ws_bytes(n,p,q,c,k,r,s, dy_bf16 != NULL) bytes.
 * Layers the DMA kernel does not take (K % 32 != 0, other filter sizes ...) run rr_dcn_dgrad_bf16_ws's kernel: same results.
 * accumulate != 0: dx holds another consumer's gradient of x and is added to (the kernels scatter with float atomics; the
 * zero fill is skipped) — the host layer's shared fan-in buffer, no separate sum pass.
 * Replaces modulated_deformable_col2im(_coord)_cuda + the dcol GEMM (ext/dcn/src/cuda/dcn_v2_cuda.cu:214-259). */
size_t rr_dcn_dgrad_ws_bytes(int n, int p, int q, int c, int k, int r, int s, int have_dy_bf16);
int rr_dcn_dgrad_bf16_packed(const float *x, const float *offset, const float *mask, const float *w, const float *dy,
                             const unsigned short *dy_bf16, float *dx, float *doffset, float *dmask, int n, int h, int wd, int c,
                             int k, int r, int s, int stride, int pad_h, int pad_w, int dilation, int deformable_groups, int accumulate,
                             void *ws, hipStream_t stream);

/* rr_dcn_dgrad with bf16 matrix operands (dY, W rounded to bf16; fp32 accumulation and scatter): the backward of
 * rr_dcn_fwd_bf16.  Layers the window kernel does not take run rr_dcn_dgrad's fp32 kernel. */
int rr_dcn_dgrad_bf16(const float *x, const float *offset, const float *mask, const float *w, const float *dy, float *dx,
                      float *doffset, float *dmask, int n, int h, int wd, int c, int k, int r, int s, int stride,
                      int pad_h, int pad_w, int dilation, int deformable_groups, hipStream_t stream);

/* rr_dcn_wgrad with bf16 matrix operands (dY and the masked bilinear samples rounded to bf16; fp32 accumulation): a
 * workgroup keeps the [256 filters][9 taps x 32 channels] block of dW in its accumulators and walks over 8x16 pixel
 * blocks whose input window is staged in LDS as in rr_dcn_fwd_bf16.  3x3, stride 1, c % 32 == 0; other layers take the
 * rr_dcn_wgrad kernel. */
int rr_dcn_wgrad_bf16(const float *x, const float *offset, const float *mask, const float *dy, float *dw, int n, int h,
                      int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w, int dilation,
                      int deformable_groups, hipStream_t stream);

/* Introspection, for tests: HOW a deformable convolution would launch, as the host plans of csrc/dcn_plan.h decide it.  Launches
 * nothing, needs no device.  pass: 0 forward, 1 weight gradient, 2 data gradient.  margin: the window margin asked for
 * (RR_DCN_WINDOW), < 0: the library's.  flags, what the entry points of a pass differ by: 1 a workspace for packed weights
 * (_packed), 2 a buffer for dY's bf16 image (_ws, _img, _packed), 4 that image is complete (_img, _packed with dy_bf16),
 * 8 accumulate.  out[0..7] = {window kernel (0: L2-gather), margin, window height, window width, pixel blocks down / across an
 * image, workgroups, dynamic LDS bytes}; out[8..] by pass —
 *   forward: window tile width, L2-gather tile width, weights packed in front and fed by LDS-DMA;
 *   weight gradient: dY by LDS-DMA, 256-filter tiles, workgroups per pixel split, pixel splits, input window by LDS-DMA, and for
 *     the L2-gather kernel 128-filter tiles, 128-channel tiles, K-steps per split;
 *   data gradient: dx zero-filled in front, the sweep reads dY's bf16 image, a pass in front writes that image, both sweep
 *     operands by LDS-DMA (weights packed in front), byte offset of the window-pixel offset table;
 * the rest 0.  n_out >= RR_DCN_PLAN_INTS.  A call the pass refuses returns an error (rr_last_error says why). */
#define RR_DCN_PLAN_INTS 16
int rr_dcn_plan(int pass, int bf16, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w,
                int dilation, int deformable_groups, int margin, int flags, int *out, int n_out);

/* DCN module glue (ext/dcn/dcn_v2.py:117-121): om NHWC [m, 3*third] -> offset [m, 2*third] (first two thirds,
 * unchanged = cat(o1, o2)) and mask [m, third] = sigmoid(last third); backward: dom from doffset, dmask and mask. */
int rr_dcn_split_fwd(const float *om, long m, int third, float *offset, float *mask, hipStream_t stream);
int rr_dcn_split_bwd(const float *doffset, const float *dmask, const float *mask, long m, int third, float *dom,
                     hipStream_t stream);

/* ---- deformable PS-RoI pooling (ext/dcn/src/cuda/dcn_v2_psroi_pooling_cuda.cu:59-290; dcn_v2.py:130-300) ------ *
 * x NHWC [b,h,w,c], c = output_dim * group_size^2; rois [n,5] = (image, x1,y1,x2,y2); trans NCHW
 * [n, trans_channels = 2*num_classes, part, part] (ignored when no_trans); out / count NHWC [n, pooled, pooled,
 * output_dim].  Backward: dx (zeroed inside, float atomics) and dtrans (REQUIRED unless no_trans; zeroed inside).
 * A RoI whose image index is negative (backward: or >= b, the batch size it is told) pools nothing: out = count = 0. */
int rr_dcn_psroi_fwd(const float *x, const float *rois, const float *trans, int n, int h, int w, int c,
                     int no_trans, float spatial_scale, int output_dim, int group_size, int pooled_size,
                     int part_size, int sample_per_part, float trans_std, int trans_channels, float *out,
                     float *count, hipStream_t stream);
int rr_dcn_psroi_bwd(const float *dout, const float *x, const float *rois, const float *trans, const float *count,
                     int n, int b, int h, int w, int c, int no_trans, float spatial_scale, int output_dim,
                     int group_size, int pooled_size, int part_size, int sample_per_part, float trans_std,
                     int trans_channels, float *dx, float *dtrans, hipStream_t stream);

/* ---- k-means (ext/kmeans/kmeans.py:13-36 `lloyd`, the anchor statistics of scripts/kmeans.py) ------------------- *
 * rr_kmeans_steps enqueues `nsteps` Lloyd steps for r independent restarts over the same points x [n,m] float32, each
 * with its own centres [r,k,m] float32 (updated in place).  One step, per restart whose flag is 0:
 *   d[n,j] = sum_m (x[n,m] - c[j,m])^2, every difference, product and sum rounded to float32, m ascending, no FMA;
 *   labels[n] = the lowest j of the minimum; sum[j,m] and count[j] over the members in double, through per-workgroup
 *   partials added in a fixed order (no floating-point atomics: a run repeats bit for bit);
 *   c'[j,m] = (float)(sum[j,m] / count[j]); where count[j] == 0 the centre STAYS (the reference writes NaN there and then
 *   never returns); shift = sum_j sqrt(sum_m (c'[j,m] - c[j,m])^2) in double on the float32 values, j and m ascending;
 *   iters += 1; inertia = sum_n d[n, labels[n]] in double (like the labels, against the centres before the update);
 *   flags = 1 (done, converged) when shift^2 < tol, else 2 (done, not converged) when iters >= max_iter.
 * A restart whose flag is set is skipped: labels [r,n], centres, counts [r,k], inertia [r], iters [r] stay as its last
 * step left them.  The caller zeroes iters and flags before the first call and reads flags [r] whenever it likes; the
 * result does not depend on how the steps are split over calls.  Limits: k <= RR_KMEANS_MAX_K, m <= RR_KMEANS_MAX_M,
 * r <= RR_KMEANS_MAX_R, n >= 1 (n < k is legal); x 16-byte aligned.  The grid is rr_kmeans_blocks(n) workgroups of 256
 * points per restart, capped at RR_KMEANS_MAX_BLOCKS (the loop strides); workspace = rr_kmeans_workspace_bytes bytes. */
#define RR_KMEANS_MAX_K 64
#define RR_KMEANS_MAX_M 4
#define RR_KMEANS_MAX_R 64
#define RR_KMEANS_MAX_BLOCKS 512
int rr_kmeans_blocks(long n);
size_t rr_kmeans_workspace_bytes(long n, int m, int k, int r);
int rr_kmeans_steps(const float *x, long n, int m, int k, int r, float *centres, int *labels, int *counts,
                    double *inertia, int *iters, int *flags, double tol, int max_iter, int nsteps, void *workspace,
                    hipStream_t stream);

/* ---- Weighted boxes fusion (Solovyev, Wang, Gabruseva 2021; the project's own feature, rrnet_amd/ensemble.py) ---- *
 * rr_wbf_segments fuses each segment's rows into clusters.  rows6 = x1,y1,x2,y2,score,cls, finite, score > 0; segment s is
 * rows seg_off[s] .. +n with n = seg_len[s], or seg_off[s+1]-seg_off[s] when seg_len is NULL.  Rows are taken in the order
 * given (the caller sorts them score-descending); classes are not compared.  Clusters are numbered in creation order.  For
 * every row r, in order:
 *   IoU of a cluster's fused box F against r, in float32 with every operation rounded on its own (no FMA):
 *     iw = min(F.x2, r.x2) - max(F.x1, r.x1), ih likewise; !(iw > 0 && ih > 0) -> 0; inter = iw*ih;
 *     u = ((F.x2-F.x1)*(F.y2-F.y1) + (r.x2-r.x1)*(r.y2-r.y1)) - inter; IoU = u > 0 ? inter/u : 0.
 *   The cluster of the largest IoU is chosen, the lowest index among equals.  r joins it iff a cluster exists and that IoU
 *   is strictly greater than iou_thr: acc_k += (double)score*(double)coord_k, S += (double)score, cnt += 1,
 *   mx = max(mx, score), F_k = (float)(acc_k / S).  Otherwise r opens a cluster: F = r's coordinates (bits unchanged),
 *   acc_k = (double)score*(double)coord_k, S = (double)score, cnt = 1, mx = score, and the cluster takes r's cls.
 * At the end cluster c goes to out6[seg_off[s]+c] = F, conf, cls; members[seg_off[s]+c] = cnt (members may be NULL);
 * n_out[s] = clusters.  conf = (float)(base * min((double)cnt, weight_sum) / weight_sum), left to right in double, with
 * base = S/cnt for conf_type 0 ("avg") and (double)mx for conf_type 1 ("max").  Rows of out6 at and beyond n_out[s] are not
 * written; out6 may not alias rows6.  No atomics and no workgroup waits on another: a run repeats bit for bit.
 * Segments of up to RR_WBF_MAX_SEG rows; a bound above RR_WBF_LDS_MAX needs `workspace` of rr_wbf_workspace_bytes bytes.
 * max_seg_boxes sizes the kernel's LDS: a segment longer than the bound the caller gave is not fused, its n_out is 0.
 * rr_wbf_plan shows what a call would launch (csrc/wbf_plan.h), for the tests: out[0] = launches (0 for an empty batch),
 * out[1] = a workspace is needed, out[2..6] = {longest segment that runs on one wave, longest segment of a split's first
 * launch, RR_WBF_LDS_MAX, RR_WBF_MAX_SEG, workgroups of the workspace launch}, out[7] = 0, then seven ints per launch i at
 * out[8+7i]: {threads, dynamic LDS bytes, clusters the LDS holds, lo, hi (the launch takes segments of lo < n <= hi rows),
 * running sums in the workspace, grid (0: one workgroup per segment)}; the rest 0.  n_out >= RR_WBF_PLAN_INTS. */
#define RR_WBF_LDS_MAX 2048
#define RR_WBF_MAX_SEG 8192
#define RR_WBF_PLAN_INTS 32
size_t rr_wbf_workspace_bytes(int nseg, int max_seg_boxes);
int rr_wbf_plan(int nseg, int max_seg_boxes, int *out, int n_out);
int rr_wbf_segments(const float *rows6, const int *seg_off, const int *seg_len, int nseg, int max_seg_boxes,
                    float iou_thr, int conf_type, double weight_sum, float *out6, int *members, int *n_out,
                    void *workspace, size_t workspace_bytes, hipStream_t stream);

/* ---- VisDrone text files: parse and format (utils/metrics/metrics.py `_read` = pandas.read_csv(float_precision='high'); the
 * writers operators/rrnet_operator.py, centernet_operator.py, retinanet_operator.py `write_results`, ensemble.format_rows) ---- *
 * Both directions are exact in 64-bit integer arithmetic (csrc/textcodec.h, shared by the kernels and the *_host loops); what
 * they cannot decide is FLAGGED and left to the host functions, never approximated.  No atomics, nothing depends on the
 * dispatch order: a run repeats bit for bit.  Limits: a text buffer of at most 2^40 bytes, fewer than 2^31 lines / rows.
 *
 * PARSE.  `text` holds nfiles files back to back, file f = bytes [file_off[f], file_off[f+1]); the caller makes every
 * non-empty file end in '\n'.  Any byte address works (byte loads only).  A line starts at byte 0 and behind every '\n'; a
 * blank line (nothing, or only '\r', in front of its '\n') is skipped, as pandas skips it.
 *   rr_text_line_counts: block_count[b] = lines that start in bytes [b, b+1) * RR_TEXT_BLOCK_BYTES, b < rr_text_line_blocks.
 *   rr_text_lines: with block_off = the exclusive sum of block_count and nlines = its total, line_pos[l] = the start of line
 *     l, ascending, and file_line_off[f] = the lines that start before file_off[f], f = 0..nfiles: file f holds lines
 *     [file_line_off[f], file_line_off[f+1]).
 *   rr_text_parse: rows[l, 0..ncol) = the first ncol fields of line l, line_flag[l] = 0, RR_TEXT_LINE_SURPLUS (the line has
 *     exactly one surplus field and it is empty: the trailing comma of some annotation files) or RR_TEXT_LINE_FLAGGED.
 *     A field is [+-]? digit* ('.' digit*)? with at least one digit, ended by ',' '\r' '\n' or the buffer's end; its value is
 *     (double)D / 10^k, D the integer of all its digits and k the digits behind the point, ONE IEEE division.  Flagged:
 *     D >= 2^53, k > 22, more than 17 digit characters (leading zeros count: pandas' parser reads 17 digits of a field and
 *     drops the rest, so beyond them it is no longer float()), anything outside the grammar (exponents, blanks, nan, inf, an empty field), a zero written with a
 *     minus sign (pandas answers 0 or -0.0 by the column's dtype), fewer than ncol fields, any other surplus, a '\r' that no
 *     '\n' follows.  Fields of a flagged line that were not reached are 0.  pandas fixes the column count by the first line:
 *     a file in which only some lines carry the surplus field belongs to the host as well (rrnet_amd/textio.py sees to it).
 *
 * FORMAT.  rows6 [nrows,6] float32 = x,y,w,h (layout 1, 2: the four values the writer is given), score, cls.  clamp 1 applies
 * v < 0 ? 0 : v to all six in float32 (NaN and -0.0 pass, as np.where(rows < 0, 0, rows) lets them).  A row's bytes:
 *   layout 0 (RRNet):     '%f,%f,%f,%f,%.4f,%d,-1,-1\n' % (x, y, w, h, score, int(cls))
 *   layout 1 (CenterNet): a..d = int(rintf(.)) of the four, then '%d,%d,%d,%d,%.4f,%d,-1,-1\n' % (a, b, c-a, d-b, score, int(cls))
 *   layout 2 (RetinaNet): '%d,%d,%d,%d,%.4f,%d,-1,-1\n' % (int(x), int(y), int(w), int(h), score, int(cls))
 * with Python's meaning of % on the float32 value: '%f' rounds the exact binary value half to even (|v| = m*2^e, the digits are
 * (m*10^6) >> -e in integers), a set sign bit prints '-' (also in front of 0.000000), infinity prints inf / -inf, NaN nan;
 * int() truncates towards zero and -0.0 gives 0.  Flagged: a finite |v| >= 2^63 anywhere, NaN or infinity under %d, and in
 * layout 1 a rounded corner at or beyond 2^62 (the difference of two must fit 64 bits).
 *   rr_text_format_len: len[r] = the row's bytes (0 for a flagged row), row_flag[r] = 0 / 1.
 *   rr_text_format: with byte_off [nrows+1] = the exclusive sum of len (int64), writes row r to out[byte_off[r] ..
 *     byte_off[r+1]).  A row whose slot is not exactly its length, or leaves [0, out_bytes), is not written; nothing else of
 *     `out` is touched.  The bytes of rows [a, b) are out[byte_off[a] .. byte_off[b]).
 * A row is at most RR_TEXT_MAX_ROW bytes: four '%f' of 27 (sign, 19 digits of 2^63, point, 6 decimals), '%.4f' of 25, '%d' of
 * 20, five commas and ",-1,-1\n" (static_assert in csrc/textio.hip against the layouts).
 *
 * rr_text_lines_host / rr_text_parse_host / rr_text_format_host run the same codec in plain loops on host pointers, so that
 * the digit logic can be tested without a device: lines_host counts (*nlines) and, where line_pos is not NULL, writes the first
 * max_lines positions; format_host fills len / row_flag where they are not NULL and writes the bytes where `out` is not NULL. */
#define RR_TEXT_BLOCK_BYTES 4096
#define RR_TEXT_MAX_ROW 165
#define RR_TEXT_MAX_COLS 64
#define RR_TEXT_LINE_FLAGGED 1
#define RR_TEXT_LINE_SURPLUS 2
int rr_text_line_blocks(long nbytes);
int rr_text_line_counts(const unsigned char *text, long nbytes, int *block_count, hipStream_t stream);
int rr_text_lines(const unsigned char *text, long nbytes, const long *file_off, int nfiles, const long *block_off,
                  long nlines, long *line_pos, long *file_line_off, hipStream_t stream);
int rr_text_parse(const unsigned char *text, long nbytes, const long *line_pos, long nlines, int ncol, double *rows,
                  int *line_flag, hipStream_t stream);
int rr_text_format_len(const float *rows6, long nrows, int layout, int clamp, int *len, int *row_flag, hipStream_t stream);
int rr_text_format(const float *rows6, long nrows, int layout, int clamp, const long *byte_off, unsigned char *out,
                   long out_bytes, hipStream_t stream);
int rr_text_lines_host(const unsigned char *text, long nbytes, const long *file_off, int nfiles, long max_lines,
                       long *line_pos, long *file_line_off, long *nlines);
int rr_text_parse_host(const unsigned char *text, long nbytes, const long *line_pos, long nlines, int ncol, double *rows,
                       int *line_flag);
int rr_text_format_host(const float *rows6, long nrows, int layout, int clamp, int *len, int *row_flag,
                        const long *byte_off, unsigned char *out, long out_bytes);

#ifdef __cplusplus
}
#endif
#endif /* RRNET_HIP_H */
