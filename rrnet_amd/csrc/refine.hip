// Inference post-process of RRNet for gfx950: re-regressed boxes, score filter and the final per-frame
// ordering, batched over frames and (frame, class) segments.
//
// Replaces, for a whole batch of frames per launch,
//   operators/rrnet_operator.py:188-209  generate_bbox  (stage-2 boxes from RoIs + regression)
//   operators/rrnet_operator.py:266-267  `pred_bbox[pred_bbox[:, 4] > 0.01]`
//   operators/rrnet_operator.py:222-223  xywh -> xyxy in front of soft_nms
//   operators/rrnet_operator.py:231      xyxy -> xywh behind it
//   operators/rrnet_operator.py:272-279  sort by score (descending) before and after _ext_nms
// The reference runs these as ~20 small torch kernels + a D2H copy + Python loops per frame and class.
// Built with -ffp-contract=off: every arithmetic step is a separate fp32 rounding like the eager torch ops.
// HBM traffic is R*(5+4+2)*4 B in and R*6*4 B out per call: latency-bound, not bandwidth-bound.
#include "common.h"
#include "rrnet_hip.h"
#include "rowkit.h"

namespace {

// One workgroup per stage-1 (frame, class) segment: rows [seg_off[s], seg_off[s+1]) of the packed RoI list.
// out rows (x1, y1, x2, y2, score, cls+1) of the boxes passing `score > thr` are written, order preserved, to the
// front of the same row range; seg_len[s] = how many.
__global__ __launch_bounds__(256) void refine_boxes_kernel(const float *rois, const float *reg, const float *scores,
                                                           const float *clses, const int *seg_off, float scale, float thr,
                                                           float *out6, int *seg_len)
{
    __shared__ int wave_cnt[4];
    const int s = blockIdx.x;
    const int r0 = seg_off[s], n = seg_off[s + 1] - r0;
    int run = 0;
    for (int base = 0; base < n; base += 256) {
        const int i = base + threadIdx.x;
        bool keep = false;
        float o0 = 0.f, o1 = 0.f, ow = 0.f, oh = 0.f, sc = 0.f, cl = 0.f;
        if (i < n) {
            const long r = r0 + i;
            rr_generate_bbox(rois + r * 5, reg + r * 4, scale, o0, o1, ow, oh);
            sc = scores[r];
            cl = clses[r] + 1.0f;
            keep = sc > thr;
        }
        int total;
        const int pos = run + rr_block_rank<4>(keep, wave_cnt, total);
        if (keep) rr_store_row6(out6 + (long)(r0 + pos) * 6, o0, o1, o0 + ow, o1 + oh, sc, cl);   // _ext_nms: x2 = x + w
        run += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) seg_len[s] = run;
}

// One workgroup per frame: the kept rows of the frame's segments (class order, as np.concatenate at
// rrnet_operator.py:225 leaves them) -> xywh -> stable sort by score descending -> out rows at
// frame_off = out_off[frame * segs_per_frame].
__global__ __launch_bounds__(256) void finalize_frames_kernel(const float *boxes6, const int *seg_off, const int *n_out,
                                                              const int *out_off, int segs_per_frame, int KP, float *out6)
{
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem);   // [KP]
    const int f = blockIdx.x;
    const int s0 = f * segs_per_frame;
    const int o0 = out_off[s0];
    const int total = out_off[s0 + segs_per_frame] - o0;
    for (int i = threadIdx.x; i < KP; i += 256) keys[i] = 0ull;
    __syncthreads();
    for (int s = s0; s < s0 + segs_per_frame; ++s) {
        const int n = n_out[s], src0 = seg_off[s], dst0 = out_off[s] - o0;
        // position = the row's place in the frame's concatenation
        for (int i = threadIdx.x; i < n; i += 256)
            keys[dst0 + i] = rr_score_key(boxes6[(long)(src0 + i) * 6 + 4], (unsigned int)(dst0 + i));
    }
    __syncthreads();
    rr_bitonic_sort<256, true>(keys, KP);
    for (int k = threadIdx.x; k < total; k += 256) {
        const int pos = (int)rr_key_pos(keys[k]);
        // segment holding that position: segs_per_frame is small (classes), linear search
        int s = s0;
        while (s + 1 < s0 + segs_per_frame && out_off[s + 1] - o0 <= pos) ++s;
        const float *r = boxes6 + (long)(seg_off[s] + (pos - (out_off[s] - o0))) * 6;
        rr_store_row6(out6 + (long)(o0 + k) * 6, r[0], r[1], r[2] - r[0], r[3] - r[1], r[4], r[5]);
    }
}

// rows [n,6] -> out [n,6] ordered by score (column 4) descending, equal scores in input order: the two
// `torch.sort(pred_bbox[:, 4], descending=True)` of operators/rrnet_operator.py:272-279 on the device (one workgroup,
// LDS bitonic sort of (score, ~position) keys; n <= 16384).
__global__ __launch_bounds__(1024) void sort_rows_kernel(const float *rows, int n, int KP, float *out)
{
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem);
    rr_sort_rows6_keys<1024>(rows, n, keys, KP);
    for (int k = threadIdx.x; k < n; k += 1024) {
        const float *r = rows + (long)rr_key_pos(keys[k]) * 6;
        rr_store_row6(out + (long)k * 6, r[0], r[1], r[2], r[3], r[4], r[5]);
    }
}

}  // namespace

extern "C" int rr_sort_rows_by_score(const float *rows6, int n, float *out6, hipStream_t stream)
{
    RR_CHECK_ARG(n >= 0 && n <= 16384, "rr_sort_rows_by_score: %d rows (limit 16384)", n);
    if (n == 0) return RR_OK;
    int kp = 2;
    while (kp < n) kp <<= 1;
    const size_t lds = (size_t)kp * 8;
    if (lds > 48 * 1024)
        RR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(sort_rows_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                     "rr_sort_rows_by_score");
    hipLaunchKernelGGL(sort_rows_kernel, dim3(1), dim3(1024), lds, stream, rows6, n, kp, out6);
    RR_CHECK_LAUNCH("rr_sort_rows_by_score");
    return RR_OK;
}

extern "C" int rr_refine_boxes(const float *rois, const float *reg, const float *scores, const float *clses,
                               const int *seg_off, int nseg, float scale, float score_thr, float *out6, int *seg_len,
                               hipStream_t stream)
{
    RR_CHECK_ARG(nseg >= 0, "rr_refine_boxes: negative segment count");
    if (nseg == 0) return RR_OK;
    hipLaunchKernelGGL(refine_boxes_kernel, dim3(nseg), dim3(256), 0, stream, rois, reg, scores, clses, seg_off, scale,
                       score_thr, out6, seg_len);
    RR_CHECK_LAUNCH("rr_refine_boxes");
    return RR_OK;
}

extern "C" int rr_finalize_frames(const float *boxes6, const int *seg_off, const int *n_out, const int *out_off,
                                  int nframes, int segs_per_frame, int max_frame_boxes, float *out6, hipStream_t stream)
{
    RR_CHECK_ARG(nframes >= 0 && segs_per_frame > 0, "rr_finalize_frames: bad dims");
    RR_CHECK_ARG(max_frame_boxes >= 0 && max_frame_boxes <= 16384, "rr_finalize_frames: %d boxes per frame (limit 16384)",
                 max_frame_boxes);
    if (nframes == 0) return RR_OK;
    int kp = 2;
    while (kp < max_frame_boxes) kp <<= 1;
    const size_t lds = (size_t)kp * 8;
    if (lds > 48 * 1024)
        RR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(finalize_frames_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                     "rr_finalize_frames");
    hipLaunchKernelGGL(finalize_frames_kernel, dim3(nframes), dim3(256), lds, stream, boxes6, seg_off, n_out, out_off,
                       segs_per_frame, kp, out6);
    RR_CHECK_LAUNCH("rr_finalize_frames");
    return RR_OK;
}
