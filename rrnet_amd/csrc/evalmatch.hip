// rr_eval_match / rr_eval_ap: the VisDrone evaluator of utils/metrics/metrics.py (get_tp :51-131, calculate_ap_rc
// :133-174) on the device.  The host versions are a Python loop over every detection of every (file, class) pair and a
// handful of whole-list tensor passes per class; here one workgroup owns a frame (matching) or a (class, threshold)
// pair (AP).
//
// rr_eval_match, one 256-thread workgroup per frame:
//   load    ground truth corners (x, y, x+w, y+h) and class into LDS; the ignored regions (class == 0) into an index list.
//   step 1  a ground truth stays iff it is an ignored region or EVERY inter/area(gt) over the ignored regions is < 0.5
//           (0.5 itself fails, 0/0 = NaN fails: torch's max propagates NaN and NaN < 0.5 is false); skipped without an
//           ignored region.  Survivors are counted per class.
//   bucket  the surviving ground truths of each class as a list of LDS indices in input order (counting pass, prefix,
//           ballot compaction), so "lowest list position" is "lowest ground-truth index", torch.max's tie rule.
//   step 2  a detection survives iff every inter/area(det) over the ignored regions is < 0.5; `counted` = survived, class
//           in 1..cls_num-1, and the frame holds a ground truth of that class.  flag_bits is zeroed.
//   match   the classes are dealt to the four waves.  A wave walks the detections 64 at a time, picks those of its class
//           with a ballot and handles them in row order: lanes stride over the class's ground truths, compute the IoU
//           once, keep a (IoU, lowest position) key per threshold among the ground truths that clear it and are not yet
//           taken at it, and one wave max per threshold that has a candidate finds the winner, whose owner lane sets the
//           taken bit.  A ground truth is always visited by the same lane of the same wave: no barrier in this phase.
// This file is compiled with -ffp-contract=off and the IoU is metrics.py's bbox_iou operation for operation (fp32,
// correctly rounded division, no reciprocal), so a flag never differs from the host's by a rounding at a threshold.
// det_len / gt_len come from the device and are clamped to dmax / gmax before any address is formed.
//
// rr_eval_ap: per (class, threshold) workgroup one reduction for the true-positive total, then ONE backward walk over
// the confidence-sorted list in chunks: the cumulative count of a row is the total minus what lies behind it, the
// precision envelope is the running maximum carried from the chunks already walked (trailing sentinel 0), and the sum
// takes (rec_i - rec_{i-1}) * env_i where recall rises, every rec as the fp32 quotient cum / max(count, 1) the host
// forms.  The per-row products are fp32 as on the host; they are accumulated in double.  A second one-workgroup kernel
// applies the in_img_count weights in class order.
#include "common.h"
#include "rrnet_hip.h"

#define EV_THREADS 256
#define EV_WAVES (EV_THREADS / 64)
#define EV_GMAX RR_EVAL_MAX_GT
#define EV_TMAX RR_EVAL_MAX_THRESHOLDS
#define EV_CMAX RR_EVAL_MAX_CLASSES
#define AP_ROWS 4                           // consecutive rows per thread in one chunk of the backward walk

struct ev_box { float x1, y1, x2, y2; };

__device__ __forceinline__ float ev_area(const ev_box &b) { return (b.x2 - b.x1) * (b.y2 - b.y1); }
__device__ __forceinline__ float ev_inter(const ev_box &a, const ev_box &b)
{
    const float iw = fmaxf(fminf(a.x2, b.x2) - fmaxf(a.x1, b.x1), 0.0f);
    const float ih = fmaxf(fminf(a.y2, b.y2) - fmaxf(a.y1, b.y1), 0.0f);
    return iw * ih;
}

// class of a row as `.long()` gives it, folded to: 1..cls_num-1 a class, anything else -1 (matches nothing)
__device__ __forceinline__ int ev_class(float c, int cls_num)
{
    return (c >= 1.0f && c < (float)cls_num) ? (int)c : -1;
}

__global__ __launch_bounds__(EV_THREADS) void eval_match_kernel(
    const float *__restrict__ dets, const int *__restrict__ det_len, int dmax, const float *__restrict__ gts,
    const int *__restrict__ gt_len, int gmax, const float *__restrict__ thresholds, int T, int cls_num,
    int *__restrict__ flag_bits, unsigned char *__restrict__ counted, int *__restrict__ target_count)
{
    __shared__ ev_box s_box[EV_GMAX];
    __shared__ short s_cls[EV_GMAX];            // 0 ignored region, 1..cls_num-1 class, -1 neither; -2 removed in step 1
    __shared__ unsigned short s_ign[EV_GMAX];   // indices of the ignored regions
    __shared__ unsigned short s_list[EV_GMAX];  // surviving ground truths, class by class, input order inside a class
    __shared__ unsigned short s_taken[EV_GMAX]; // per list position: bit t = taken at threshold t
    __shared__ int s_cnt[EV_CMAX + 1];
    __shared__ int s_off[EV_CMAX + 1];
    __shared__ int s_nign;

    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int nd = det_len[f], ng = gt_len[f];
    nd = nd < 0 ? 0 : (nd > dmax ? dmax : nd);
    ng = ng < 0 ? 0 : (ng > gmax ? gmax : ng);
    const float *D = dets + (long)f * dmax * 6;
    const float *G = gts + (long)f * gmax * 6;
    int *FB = flag_bits + (long)f * dmax;
    unsigned char *CT = counted + (long)f * dmax;

    if (tid <= EV_CMAX) s_cnt[tid] = 0;
    if (tid == 0) s_nign = 0;
    __syncthreads();
    for (int g = tid; g < ng; g += EV_THREADS) {
        const float *r = G + (long)g * 6;
        ev_box b;
        b.x1 = r[0], b.y1 = r[1], b.x2 = r[0] + r[2], b.y2 = r[1] + r[3];
        s_box[g] = b;
        const float c = r[5];
        const bool ign = c == 0.0f;
        s_cls[g] = (short)(ign ? 0 : ev_class(c, cls_num));
        s_taken[g] = 0;
        if (ign) s_ign[atomicAdd(&s_nign, 1)] = (unsigned short)g;   // order is irrelevant: only "every ratio < 0.5" is asked
    }
    __syncthreads();
    const int nign = s_nign;

    // step 1: ground truths mostly inside an ignored region leave; survivors are counted per class
    for (int g = tid; g < ng; g += EV_THREADS) {
        int c = s_cls[g];
        if (c == 0) continue;
        const ev_box b = s_box[g];
        const float area = ev_area(b);
        bool keep = true;
        for (int i = 0; i < nign; ++i) keep &= (ev_inter(b, s_box[s_ign[i]]) / area) < 0.5f;
        if (!keep) s_cls[g] = -2;
        else if (c > 0) atomicAdd(&s_cnt[c], 1);
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int c = 1; c < cls_num; ++c) { s_off[c] = run; run += s_cnt[c]; }
        s_off[cls_num] = run;
    }
    if (tid >= 1 && tid < cls_num) target_count[(long)f * (cls_num - 1) + tid - 1] = s_cnt[tid];
    __syncthreads();

    // bucket: wave w lists the ground truths of its classes in input order
    for (int c = 1 + wave; c < cls_num; c += EV_WAVES) {
        int pos = s_off[c];
        for (int g0 = 0; g0 < ng; g0 += 64) {
            const int g = g0 + lane;
            const bool mine = g < ng && s_cls[g] == c;
            const unsigned long long m = __ballot(mine);
            if (mine) s_list[pos + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)g;
            pos += __popcll(m);
        }
    }

    // step 2: detections mostly inside an ignored region leave; `counted` and a zeroed flag word for every row
    for (int d = tid; d < dmax; d += EV_THREADS) {
        unsigned char cnt = 0;
        if (d < nd) {
            const float *r = D + (long)d * 6;
            ev_box b;
            b.x1 = r[0], b.y1 = r[1], b.x2 = r[0] + r[2], b.y2 = r[1] + r[3];
            const int c = ev_class(r[5], cls_num);
            const float area = ev_area(b);
            bool keep = true;
            for (int i = 0; i < nign; ++i) keep &= (ev_inter(b, s_box[s_ign[i]]) / area) < 0.5f;
            cnt = (keep && c > 0 && s_cnt[c] > 0) ? 1 : 0;
        }
        CT[d] = cnt;
        FB[d] = 0;
    }
    __syncthreads();                            // the lists, `counted` and the zeroed flags are visible to every wave

    float thr[EV_TMAX];
#pragma unroll
    for (int t = 0; t < EV_TMAX; ++t) thr[t] = t < T ? thresholds[t] : 0.0f;

    for (int c = 1 + wave; c < cls_num; c += EV_WAVES) {
        const int g_lo = s_off[c], g_hi = s_off[c + 1];
        if (g_hi == g_lo) continue;
        for (int d0 = 0; d0 < nd; d0 += 64) {
            const int d = d0 + lane;
            ev_box mine = {0.f, 0.f, 0.f, 0.f};
            bool sel = false;
            if (d < nd && CT[d]) {
                const float *r = D + (long)d * 6;
                sel = ev_class(r[5], cls_num) == c;
                mine.x1 = r[0], mine.y1 = r[1], mine.x2 = r[0] + r[2], mine.y2 = r[1] + r[3];
            }
            unsigned long long todo = __ballot(sel);
            while (todo) {                      // wave-uniform: the selected detections in row order
                const int j = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                ev_box a;
                a.x1 = __shfl(mine.x1, j, 64), a.y1 = __shfl(mine.y1, j, 64);
                a.x2 = __shfl(mine.x2, j, 64), a.y2 = __shfl(mine.y2, j, 64);
                const float a_area = ev_area(a);
                unsigned long long best[EV_TMAX];
#pragma unroll
                for (int t = 0; t < EV_TMAX; ++t) best[t] = 0ull;
                for (int p = g_lo + lane; p < g_hi; p += 64) {
                    const ev_box b = s_box[s_list[p]];
                    const float inter = ev_inter(a, b);
                    const float uni = fmaxf((a_area + ev_area(b)) - inter, 1e-8f);
                    const float iou = inter / uni;
                    const unsigned tk = s_taken[p];
                    // a larger IoU wins, then the lower position: IoU > 0 here, so its bit pattern orders like the value
                    const unsigned long long key =
                        ((unsigned long long)__float_as_uint(iou) << 32) | (unsigned)(0xffffffffu - (unsigned)p);
#pragma unroll
                    for (int t = 0; t < EV_TMAX; ++t) {
                        const bool cand = t < T && (iou - thr[t]) >= 0.0f && iou > 0.0f && !((tk >> t) & 1u);
                        if (cand && key > best[t]) best[t] = key;
                    }
                }
                int bits = 0;
#pragma unroll
                for (int t = 0; t < EV_TMAX; ++t) {
                    if (t >= T || __ballot(best[t] != 0ull) == 0ull) continue;     // wave-uniform
                    unsigned long long k = best[t];
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const unsigned long long other = __shfl_xor(k, o, 64);
                        k = other > k ? other : k;
                    }
                    const int p = (int)(0xffffffffu - (unsigned)(k & 0xffffffffull));
                    if (p >= g_lo && p < g_hi && ((p - g_lo) & 63) == lane) s_taken[p] |= (unsigned short)(1u << t);
                    bits |= 1 << t;
                }
                if (lane == 0) FB[d0 + j] = bits;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ int ev_wave_incl_sum(int v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_up(v, o, 64);
        if (lane >= o) v += u;
    }
    return v;
}
// inclusive maximum over this lane and every HIGHER lane
__device__ __forceinline__ float ev_wave_suffix_max(float v, int lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float u = __shfl_down(v, o, 64);
        if (lane + o < 64) v = fmaxf(v, u);
    }
    return v;
}

__global__ __launch_bounds__(EV_THREADS) void eval_ap_kernel(
    const int *__restrict__ flags, long nrows, const int *__restrict__ seg_off, const int *__restrict__ target_count,
    int C, int T, float *__restrict__ work)
{
    __shared__ int s_sum[EV_WAVES];
    __shared__ float s_max[EV_WAVES];
    __shared__ double s_acc[EV_WAVES];
    const int c = blockIdx.x / T, t = blockIdx.x - c * T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *ap_out = work + (long)c * T + t, *rc_out = work + (long)C * T + (long)c * T + t;
    long lo = seg_off[c], hi = seg_off[c + 1];
    lo = lo < 0 ? 0 : (lo > nrows ? nrows : lo);
    hi = hi < lo ? lo : (hi > nrows ? nrows : hi);
    const int count = target_count[c];
    const long n = hi - lo;
    if (count <= 0 || n == 0) {                 // a class without ground truth is skipped; an empty list integrates to 0
        if (tid == 0) *ap_out = 0.0f, *rc_out = 0.0f;
        return;
    }
    const int *F = flags + lo;
    const float fcount = (float)count;          // count >= 1 here: clamp(min=1) is the identity

    int part = 0;
    for (long i = tid; i < n; i += EV_THREADS) part += (F[i] >> t) & 1;
    part = wave_sum_i(part);
    if (lane == 0) s_sum[wave] = part;
    __syncthreads();
    int cum_end = 0;                            // true positives in rows [0, chunk end)
#pragma unroll
    for (int w = 0; w < EV_WAVES; ++w) cum_end += s_sum[w];
    const float max_rec = (float)cum_end / fcount;      // recall never falls: its maximum is the last row's
    __syncthreads();

    const long chunk = (long)EV_THREADS * AP_ROWS;
    float env_tail = 0.0f;                      // envelope of everything behind the chunk; the sentinel row holds 0
    double acc = 0.0;
    for (long base = (n - 1) / chunk * chunk; base >= 0; base -= chunk) {
        const long r0 = base + (long)tid * AP_ROWS;
        int fl[AP_ROWS], mysum = 0;
#pragma unroll
        for (int k = 0; k < AP_ROWS; ++k) {
            fl[k] = (r0 + k < n) ? ((F[r0 + k] >> t) & 1) : 0;
            mysum += fl[k];
        }
        const int wincl = ev_wave_incl_sum(mysum, lane);
        if (lane == 63) s_sum[wave] = wincl;
        __syncthreads();
        int before = wincl - mysum, chunk_sum = 0;      // true positives of the chunk in front of this thread's rows
#pragma unroll
        for (int w = 0; w < EV_WAVES; ++w) {
            if (w < wave) before += s_sum[w];
            chunk_sum += s_sum[w];
        }
        const int cum_base = cum_end - chunk_sum + before;
        float prec[AP_ROWS], mymax = 0.0f;
        int cum[AP_ROWS];
        int run = cum_base;
#pragma unroll
        for (int k = 0; k < AP_ROWS; ++k) {
            run += fl[k];
            cum[k] = run;
            prec[k] = (r0 + k < n) ? (float)run / (float)(r0 + k + 1) : 0.0f;
            mymax = fmaxf(mymax, prec[k]);
        }
        const float wsuf = ev_wave_suffix_max(mymax, lane);
        if (lane == 0) s_max[wave] = wsuf;
        __syncthreads();
        float behind = env_tail, chunk_max = env_tail;  // maximum over the threads behind this one, and the tail
#pragma unroll
        for (int w = 0; w < EV_WAVES; ++w) {
            if (w > wave) behind = fmaxf(behind, s_max[w]);
            chunk_max = fmaxf(chunk_max, s_max[w]);
        }
        const float next = __shfl_down(wsuf, 1, 64);
        if (lane < 63) behind = fmaxf(behind, next);
        float env = behind;
#pragma unroll
        for (int k = AP_ROWS - 1; k >= 0; --k) {
            env = fmaxf(env, prec[k]);
            if (r0 + k < n) {
                const float rec = (float)cum[k] / fcount, rec_prev = (float)(cum[k] - fl[k]) / fcount;
                const float step = rec - rec_prev;
                if (step > 0.0f) acc += (double)(step * env);
            }
        }
        env_tail = chunk_max;
        cum_end -= chunk_sum;
        __syncthreads();                        // s_sum / s_max are rewritten by the next chunk
    }
    acc = wave_sum_d(acc);
    if (lane == 0) s_acc[wave] = acc;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int w = 0; w < EV_WAVES; ++w) s += s_acc[w];
        *ap_out = (float)s;
        *rc_out = max_rec;
    }
}

// total_ap / total_rc of calculate_ap_rc in its class order and fp32; 0/0 = NaN when no class occurs in any image
__global__ __launch_bounds__(64) void eval_ap_finish_kernel(
    const float *__restrict__ work, const int *__restrict__ target_count, const int *__restrict__ in_img_count, int C,
    int T, float *__restrict__ ap, float *__restrict__ rc)
{
    const int t = threadIdx.x;
    float total_ap = 0.0f, total_rc = 0.0f, imgs = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float w = (float)in_img_count[c];
        imgs += w;
        if (target_count[c] == 0 || t >= T) continue;
        total_ap += work[(long)c * T + t] * w;
        total_rc += work[(long)C * T + (long)c * T + t] * w;
    }
    const float r = t < T ? total_rc / imgs : 0.0f;
    if (t < T) ap[t] = total_ap / imgs;
    float sum = 0.0f;
    for (int i = 0; i < T; ++i) sum += __shfl(r, i, 64);       // torch's mean over T <= 16 values: a plain running sum
    if (t == 0) *rc = sum / (float)T;
}

extern "C" int rr_eval_match(const float *dets, const int *det_len, const float *gts, const int *gt_len,
                             const float *thresholds, int f, int dmax, int gmax, int t, int cls_num, int *flag_bits,
                             unsigned char *counted, int *target_count, hipStream_t stream)
{
    RR_CHECK_ARG(f >= 0 && dmax >= 0 && gmax >= 0, "rr_eval_match: negative dims");
    RR_CHECK_ARG(gmax <= RR_EVAL_MAX_GT, "rr_eval_match: at most %d ground truths per frame (got %d)", RR_EVAL_MAX_GT, gmax);
    RR_CHECK_ARG(t >= 1 && t <= RR_EVAL_MAX_THRESHOLDS, "rr_eval_match: 1..%d thresholds (got %d)",
                 RR_EVAL_MAX_THRESHOLDS, t);
    RR_CHECK_ARG(cls_num >= 2 && cls_num <= RR_EVAL_MAX_CLASSES, "rr_eval_match: cls_num in 2..%d (got %d)",
                 RR_EVAL_MAX_CLASSES, cls_num);
    if (f == 0) return RR_OK;
    RR_CHECK_ARG(det_len && gt_len && thresholds && target_count && (dmax == 0 || (dets && flag_bits && counted)) &&
                 (gmax == 0 || gts), "rr_eval_match: null pointer");
    hipLaunchKernelGGL(eval_match_kernel, dim3((unsigned)f), dim3(EV_THREADS), 0, stream, dets, det_len, dmax, gts, gt_len,
                       gmax, thresholds, t, cls_num, flag_bits, counted, target_count);
    RR_CHECK_LAUNCH("rr_eval_match");
    return RR_OK;
}

extern "C" int rr_eval_ap(const int *flag_bits, long nrows, const int *seg_off, const int *target_count,
                          const int *in_img_count, int c, int t, float *work, float *ap, float *rc, hipStream_t stream)
{
    RR_CHECK_ARG(nrows >= 0 && c >= 1 && c < RR_EVAL_MAX_CLASSES, "rr_eval_ap: bad dims");
    RR_CHECK_ARG(t >= 1 && t <= RR_EVAL_MAX_THRESHOLDS, "rr_eval_ap: 1..%d thresholds (got %d)", RR_EVAL_MAX_THRESHOLDS, t);
    RR_CHECK_ARG(seg_off && target_count && in_img_count && work && ap && rc && (nrows == 0 || flag_bits),
                 "rr_eval_ap: null pointer");
    hipLaunchKernelGGL(eval_ap_kernel, dim3((unsigned)(c * t)), dim3(EV_THREADS), 0, stream, flag_bits, nrows, seg_off,
                       target_count, c, t, work);
    RR_CHECK_LAUNCH("rr_eval_ap");
    hipLaunchKernelGGL(eval_ap_finish_kernel, dim3(1), dim3(64), 0, stream, work, target_count, in_img_count, c, t, ap, rc);
    RR_CHECK_LAUNCH("rr_eval_ap (finish)");
    return RR_OK;
}
