// The host launch plan of weighted boxes fusion (csrc/wbf.hip), plain C++ with no HIP include, next to softnms_plan.h.
// WHICH launches a call gets — threads, dynamic LDS and its cluster capacity, the segment lengths each launch takes, accumulators
// in LDS or in the global workspace, the grid — and which bound is refused is decided here and nowhere else: rr_wbf_segments
// carries the plan out, and rr_wbf_plan (include/rrnet_hip.h) shows it to the tests (tests/wbf_cases.py names the route of every
// row of its table).
//
// A segment of n rows opens at most n clusters.  Per cluster the kernel keeps the fused box (4 floats, read by every step) and the
// running sums (5 doubles, count, maximum, class: touched only by a join or at the end).  The caller's bound is the LONGEST
// possible segment while a typical (frame, class) segment holds ~150 rows, so — as for Soft-NMS — a call is split by segment
// length: every launch has one workgroup per segment, and the workgroups whose segment belongs to another launch return at once.
#pragma once
#include "rrnet_hip.h"

namespace rr_plan {

constexpr int WBF_ONE_WAVE = 64;           // a segment of up to this many rows runs on the first wave of its workgroup, no barriers
constexpr int WBF_SHORT = 256;             // first launch of a split: LDS for this many clusters (17 KB: nine workgroups per CU)
constexpr int WBF_LDS_MAX = 2048;          // longest segment whose running sums stay in LDS (136 KB)
constexpr int WBF_MAX_SEG = 8192;          // longest segment taken: the fused boxes alone fill 128 KB of LDS
constexpr int WBF_WS_GRID = 256;           // workgroups of the workspace launch (one per CU); each walks segments blockIdx.x, +grid, ...
constexpr int WBF_ALL = 0x7fffffff;
constexpr int WBF_CLUSTER_LDS_BYTES = 68;  // 4 floats + 5 doubles + count + maximum + class
constexpr int WBF_BOX_LDS_BYTES = 16;      // the fused box alone (workspace launch)
constexpr int WBF_CLUSTER_WS_BYTES = 52;   // 5 doubles + count + maximum + class

// one launch of wbf_kernel<T, WS>: it takes the segments of lo < n <= hi rows
struct WbfLaunch {
    int T, lds, cap, lo, hi;
    bool ws;                   // running sums in the global workspace (cap * WBF_CLUSTER_WS_BYTES per workgroup), boxes in LDS
    int grid;                  // 0: one workgroup per segment; else min(nseg, grid) workgroups that walk the segments
    bool raise_lds_limit;      // more than 48 KB of dynamic LDS: hipFuncAttributeMaxDynamicSharedMemorySize first
};

// refuse non-null: the call is not taken (a printf format for a0).  launches 0: an empty batch, nothing to do.
struct WbfPlan {
    const char *refuse;
    int a0;
    int launches;              // 0 .. 3
    bool use_workspace;
    long workspace_bytes;
    WbfLaunch launch[3];
};

inline int wbf_cap(int n) { return (n + 3) & ~3; }

inline WbfLaunch wbf_launch(int T, int cap, int lo, int hi, bool ws, int grid)
{
    const long lds = (long)cap * (ws ? WBF_BOX_LDS_BYTES : WBF_CLUSTER_LDS_BYTES);
    return WbfLaunch{T, (int)lds, cap, lo, hi, ws, grid, lds > 48 * 1024};
}

inline WbfPlan wbf_plan(int nseg, int max_seg_boxes)
{
    WbfPlan p{};
    if (!(nseg >= 0 && max_seg_boxes >= 0)) { p.refuse = "rr_wbf_segments: negative size"; return p; }
    if (!(max_seg_boxes <= WBF_MAX_SEG)) {
        p.refuse = "rr_wbf_segments: segment of %d rows (limit 8192)";
        p.a0 = max_seg_boxes;
        return p;
    }
    if (nseg == 0) return p;
    const int cap = wbf_cap(max_seg_boxes < 4 ? 4 : max_seg_boxes);
    if (max_seg_boxes <= WBF_ONE_WAVE) {
        // every segment fits one wave: one lane per cluster, the step's arg-max is a wave reduction and nothing else
        p.launches = 1;
        p.launch[0] = wbf_launch(64, cap, -1, WBF_ALL, false, 0);
        return p;
    }
    if (max_seg_boxes <= WBF_SHORT) {
        p.launches = 1;
        p.launch[0] = wbf_launch(256, cap, -1, WBF_ALL, false, 0);
        return p;
    }
    // the short segments with 17 KB of LDS each, then the longer ones with the LDS they need: 512 threads keep the scan of a
    // step at four clusters per lane for 2048 clusters, behind an eight-wave barrier
    p.launches = 2;
    p.launch[0] = wbf_launch(256, WBF_SHORT, -1, WBF_SHORT, false, 0);
    if (max_seg_boxes <= WBF_LDS_MAX) {
        p.launch[1] = wbf_launch(512, cap, WBF_SHORT, WBF_ALL, false, 0);
        return p;
    }
    // longer than the LDS holds with its sums: the fused boxes stay in LDS (the scan of every step reads them), the sums of the
    // one cluster a step changes live in a per-workgroup slice of the workspace
    p.launches = 3;
    p.launch[1] = wbf_launch(512, WBF_LDS_MAX, WBF_SHORT, WBF_LDS_MAX, false, 0);
    p.launch[2] = wbf_launch(512, cap, WBF_LDS_MAX, WBF_ALL, true, WBF_WS_GRID);
    p.use_workspace = true;
    p.workspace_bytes = (long)(nseg < WBF_WS_GRID ? nseg : WBF_WS_GRID) * cap * WBF_CLUSTER_WS_BYTES;
    return p;
}

}  // namespace rr_plan
