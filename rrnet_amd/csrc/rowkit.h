// Device helpers shared by the detection post-processing kernels (refine, detect, retina, hardnms, decode, roialign,
// augment): the ordered score key, the LDS bitonic network, the ordered compaction rank, the six-float row store, the
// generate_bbox arithmetic and the normalisation table.  One copy each: a fix to a barrier, a clamp or a rounding is made
// here once.  Everything is __device__ __forceinline__ and templated on compile-time facts only, so every kernel compiles
// to what it was with the code written out.
//
// Floating point: rr_generate_bbox and rr_norm_lut_fill must round every step on its own (they are held bit for bit to
// the reference's eager float32 ops).  They switch contraction off for their own bodies, so they do not depend on the
// including file's -ffp-contract flag; every file that uses them today is built with -ffp-contract=off anyway.  The other
// helpers are integer only (decode.hip and roialign.hip, built with the default contraction, take just those).
#pragma once
#include "common.h"

// Order-preserving map float -> u32 (a < b as floats <=> ord(a) < ord(b) as unsigned; -0 < +0, NaNs at the ends) and back.
__device__ __forceinline__ unsigned int rr_f2ord(float f)
{
    const unsigned int u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float rr_ord2f(unsigned int o)
{
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// Sort key of a scored row: high word the score's order, low word ~position, so that a DESCENDING sort of the keys is a
// stable descending sort by score (the earlier position wins a tie).  0 sorts behind every key: padding.
__device__ __forceinline__ unsigned long long rr_score_key(float score, unsigned int pos)
{
    return ((unsigned long long)rr_f2ord(score) << 32) | (unsigned long long)(0xffffffffu - pos);
}
__device__ __forceinline__ unsigned int rr_key_pos(unsigned long long key)
{
    return 0xffffffffu - (unsigned int)(key & 0xffffffffull);
}

// Bitonic network over keys[0..np) in LDS, np a power of two >= 2, by the NT threads of the workgroup; DESC: largest key
// first.  Barriers: the caller puts one __syncthreads() between its last write of keys and this call; the network ends
// with one, so keys may be read right after it returns.
template <int NT, bool DESC, typename K>
__device__ __forceinline__ void rr_bitonic_sort(K *keys, int np)
{
    for (int k2 = 2; k2 <= np; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < np / 2; t += NT) {
                const int lo = ((t / j) * 2 * j) + (t % j);
                const int hi = lo + j;
                const bool fwd = ((lo & k2) == 0);
                const K a = keys[lo], b = keys[hi];
                if ((DESC ? a < b : a > b) == fwd) { keys[lo] = b; keys[hi] = a; }
            }
            __syncthreads();
        }
    }
}

// keys[0..np) = the score keys of rows6[0..n) (score in column 4, position = row index), zero behind them, sorted
// descending: rr_key_pos(keys[k]) is the row that comes k-th.  Ends with the network's barrier.
template <int NT>
__device__ __forceinline__ void rr_sort_rows6_keys(const float *rows6, int n, unsigned long long *keys, int np)
{
    for (int i = threadIdx.x; i < np; i += NT) keys[i] = i < n ? rr_score_key(rows6[(long)i * 6 + 4], (unsigned int)i) : 0ull;
    __syncthreads();
    rr_bitonic_sort<NT, true>(keys, np);
}

// Ordered compaction, one pass of a workgroup of WAVES waves (one row per thread): returns the number of kept rows in
// front of this thread's row in the pass, and in `total` (every thread) the number the pass keeps.  A caller appends in
// order by writing its kept row at (rows kept by earlier passes) + rank and adding total to that count, which it holds in
// a register.  wave_cnt: WAVES ints of LDS.
// Barrier contract: every thread of the workgroup calls it (keep = false for a thread without a row); it holds ONE
// __syncthreads(), between the waves' writes of wave_cnt and the reads.  A caller that calls it again with the same
// wave_cnt puts a __syncthreads() between the two calls (a loop: at the end of each pass), so that no wave overwrites a
// count another wave has yet to read.  LDS the caller wrote before the call is visible after it.
template <int WAVES>
__device__ __forceinline__ int rr_block_rank(bool keep, int *wave_cnt, int &total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int rank = __popcll(m & ((1ull << lane) - 1ull));
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const int c = wave_cnt[w];
        if (w < wave) rank += c;
        total += c;
    }
    return rank;
}

__device__ __forceinline__ void rr_store_row6(float *o, float v0, float v1, float v2, float v3, float v4, float v5)
{
    o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3; o[4] = v4; o[5] = v5;
}

// generate_bbox (operators/rrnet_operator.py:188-209) of one RoI: roi = (frame, x1, y1, x2, y2) in feature coordinates,
// reg = the head's four outputs -> x, y, w, h in image coordinates.  xyxy * scale -> xywh -> w,h += 1 -> centre / size
// update -> xywh, every step its own fp32 rounding.
__device__ __forceinline__ void rr_generate_bbox(const float *roi, const float *reg, float scale, float &ox, float &oy,
                                                 float &ow, float &oh)
{
#pragma clang fp contract(off)
    const float x = roi[1] * scale, y = roi[2] * scale;
    const float w = (roi[3] * scale - x) + 1.0f, h = (roi[4] * scale - y) + 1.0f;
    const float cx = (reg[0] * w + x) + w / 2.0f;
    const float cy = (reg[1] * h + y) + h / 2.0f;
    ow = expf(reg[2]) * w;
    oh = expf(reg[3]) * h;
    ox = cx - ow / 2.0f;
    oy = cy - oh / 2.0f;
}

// lut[v*3 + c] = (v / 255 - mean[c]) / stdv[c] for the 256 byte values and three channels: ToTensor then Normalize with
// the three float32 operations torch performs (the division is correctly rounded).  lut: 768 floats of LDS; ends with a
// __syncthreads().
template <int NT>
__device__ __forceinline__ void rr_norm_lut_fill(float *lut, const float *mean, const float *stdv)
{
#pragma clang fp contract(off)
    for (int i = threadIdx.x; i < 256 * 3; i += NT) {
        const int v = i / 3, c = i - v * 3;
        const float x = (float)v / 255.0f;               // ToTensor: uint8.float().div(255)
        lut[i] = (x - mean[c]) / stdv[c];                // Normalize: sub, div
    }
    __syncthreads();
}
