// The host launch plan of Soft-NMS (csrc/softnms.hip), plain C++ with no HIP include, next to conv_plan.h and dcn_plan.h.
// WHICH kernel a call launches — register-resident or LDS loop, threads and boxes per lane, one launch or the two-launch split,
// dynamic LDS and its row capacity, LDS or the global workspace — and which arguments are refused is decided here and nowhere
// else: soft_nms_launch carries the plan out, and rr_soft_nms_plan (include/rrnet_hip.h) shows it to the tests together with the
// per-segment constants of the kernels (tests/softnms_cases.py writes the expected answer next to every row of its table).
// Finite scores and coordinates only: the register kernel's v_min / v_max shortcut and its sortable score key assume them, and
// the reference's ordering of NaN is not matched.
#pragma once
#include "rrnet_hip.h"

namespace rr_plan {

enum { SNMS_REGISTERS = 0, SNMS_LDS_LOOP = 1 };          // SoftNmsPlan::kernel

// ---- per-segment constants of the kernels (softnms.hip uses these, the tests read them through rr_soft_nms_plan)
constexpr int SNMS_REG_LIST = 64;          // deaths of one step the register kernel renumbers from its LDS list; more take the mask path
constexpr int SNMS_REG_SHORT = 256;        // a segment of up to this many boxes in a register launch with T > 256 runs <256, 1>
constexpr int SNMS_MASK_WORDS = 288;       // 32-bit words of one dead-position mask
constexpr int SNMS_MASK_BOXES = SNMS_MASK_WORDS * 32;    // 9216: the longest segment the register kernels take
constexpr int SNMS_ONE_WAVE = 192;         // a segment of up to this many boxes runs on the first wave of an LDS-loop workgroup
constexpr int SNMS_MID_SEG = 512;          // first launch of the two-launch split: LDS for this many boxes (12.8 KB)
constexpr int SNMS_LDS_MAX = RR_SOFT_NMS_LDS_MAX;        // the LDS loop keeps segments up to this long in LDS
constexpr int SNMS_ALL = 0x7fffffff;

// dynamic LDS of the LDS loop for `cap` rows: five float columns, two 16-bit index columns, one flag byte
inline long snms_lds_bytes(int cap) { return (long)cap * 25 + 16; }

// one launch of soft_nms_kernel<T>: it takes the segments of lo < n <= hi boxes
struct SoftNmsLdsLaunch {
    int T, lds, cap, lo, hi;
    bool raise_lds_limit;      // more than 48 KB of dynamic LDS: hipFuncAttributeMaxDynamicSharedMemorySize first
};

// refuse non-null: the call is not taken (a printf format for a0).  launches 0: an empty batch, nothing to do.
struct SoftNmsPlan {
    const char *refuse;
    int a0;
    int launches;              // 0, 1, or 2 (the two-launch split of the LDS loop)
    int kernel;                // SNMS_REGISTERS: soft_nms_reg_kernel<T, NB>; SNMS_LDS_LOOP: soft_nms_kernel<T> per entry of lds_launch
    int T, NB;                 // register kernel; for the LDS loop T of the last launch, NB 0
    bool in_lds;               // the bound fits the LDS loop's LDS; otherwise the caller must bring a workspace ...
    bool use_workspace;        // ... which only the LDS loop uses (its global-workspace form)
    SoftNmsLdsLaunch lds_launch[2];
};

inline SoftNmsLdsLaunch snms_lds_launch(int T, long lds, int cap, int lo, int hi)
{
    return SoftNmsLdsLaunch{T, (int)lds, cap, lo, hi, lds > 48 * 1024};
}

inline SoftNmsPlan soft_nms_plan(int nseg, int max_seg_boxes, bool has_workspace)
{
    SoftNmsPlan p{};
    if (!(nseg >= 0 && max_seg_boxes >= 0)) { p.refuse = "rr_soft_nms_segments: negative size"; return p; }
    if (!(max_seg_boxes < 65536)) { p.refuse = "rr_soft_nms_segments: segment of %d boxes (limit 65535)"; p.a0 = max_seg_boxes; return p; }
    if (nseg == 0) return p;
    p.in_lds = max_seg_boxes <= SNMS_LDS_MAX;
    if (!(p.in_lds || has_workspace)) { p.refuse = "rr_soft_nms_segments: workspace required for %d-box segments"; p.a0 = max_seg_boxes; return p; }
    // Regime: a few segments (an image's classes at evaluation, rrnet_operator.py:246-284) are a latency problem — the
    // register-resident kernel; a batch of more long segments than two per CU is a throughput problem, where the LDS loop's
    // 256-thread workgroups (4 per CU) retire more segments per unit time (1280 x 1500 boxes: 5.5 against 6.0 ms)
    const bool throughput_regime = nseg > 512 && max_seg_boxes > 256;
    // (measured, one segment: 2500 boxes 4.97 against 5.57 ms for the LDS loop; at 5000 / 9000 boxes — six / nine boxes per
    // lane of a 1024-thread workgroup, 128 registers per lane — the register kernel spills and loses, 15.7 against 14.2 and
    // 52 against 38 ms: it takes segments of up to 3072 boxes)
    // (round 5, with the list renumbering: one 9000-box segment 29 ms in registers — 18 boxes per lane of 512 threads, 256 registers,
    // no scratch — against 38 ms for the LDS loop on its global workspace; a batch of such segments likewise: the LDS loop has no
    // LDS for them and runs out of L2)
    if (max_seg_boxes <= SNMS_MASK_BOXES && (!throughput_regime || !p.in_lds)) {
        // register-resident kernels: T x NB boxes per segment.
        // One wave alone on a SIMD issues a vector instruction every 4 cycles, two waves one every 2: the configurations put
        // (at least) two waves on every SIMD of the CU wherever the segment is long enough to feed them
        // (measured: 1024 x 2 for 1500 boxes, four waves per SIMD, is 30 % slower than 512 x 3: a 16-wave barrier and exchange)
        p.kernel = SNMS_REGISTERS;
        p.launches = 1;
        if (max_seg_boxes <= 256) { p.T = 256; p.NB = 1; }
        else if (max_seg_boxes <= 1536) { p.T = 512; p.NB = 3; }
        else if (max_seg_boxes <= 3072) { p.T = 1024; p.NB = 3; }
        else if (max_seg_boxes <= 6144) { p.T = 512; p.NB = 12; }
        else { p.T = 512; p.NB = 18; }
        return p;
    }
    // (segments of up to 256 boxes never get here: the register kernels above take them)
    p.kernel = SNMS_LDS_LOOP;
    p.use_workspace = !p.in_lds;
    const int cap = (max_seg_boxes + 3) & ~3;
    const long lds = p.in_lds ? snms_lds_bytes(cap) : 0;
    const int T = max_seg_boxes <= 2560 ? 256 : 1024;
    if (p.in_lds && max_seg_boxes > SNMS_MID_SEG) {
        // The caller's bound is the LONGEST possible segment (K = 1500 at inference: 37.5 KB of LDS per workgroup = four
        // segments per CU) while a typical (frame, class) segment holds ~150 boxes.  Two launches: the segments of up to
        // MID_SEG boxes with 12.8 KB of LDS each (all 1280 segments of a 128-frame batch are resident at once: the launch
        // lasts as long as its longest segment instead of a round and a quarter), then the larger ones with the LDS
        // they need (workgroups of the others return at once).
        p.launches = 2;
        p.lds_launch[0] = snms_lds_launch(256, snms_lds_bytes(SNMS_MID_SEG), SNMS_MID_SEG, -1, SNMS_MID_SEG);
        p.lds_launch[1] = snms_lds_launch(T, lds, cap, SNMS_MID_SEG, SNMS_ALL);
    } else {
        p.launches = 1;
        p.lds_launch[0] = snms_lds_launch(T, lds, cap, -1, SNMS_ALL);
    }
    p.T = T;
    return p;
}

}  // namespace rr_plan
