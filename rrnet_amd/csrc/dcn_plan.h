// The host launch plan of the deformable convolutions (csrc/dcn.hip), plain C++ with no HIP include, next to conv_plan.h.
// WHICH kernel a forward / weight-gradient / data-gradient call launches — LDS-window or L2-gather, the window's margin, tile
// widths, grids, LDS bytes, which operands travel by LDS-DMA and which helper passes run in front — is decided here and nowhere
// else: the entry points of dcn.hip fill their argument structs from a plan, rr_dcn_fused_bwd_supported_dil asks the two
// backward plans, and rr_dcn_plan (include/rrnet_hip.h) shows all three to the tests, whose Python mirror (tests/helpers.py)
// answers to it.
#pragma once
#include "conv_plan.h"

namespace rr_plan {

enum { DCN_FWD = 0, DCN_WGRAD = 1, DCN_DGRAD = 2 };                     // the pass argument of rr_dcn_plan
enum { DCN_HAS_WPACK = 1, DCN_HAS_DYB = 2, DCN_DYB_READY = 4, DCN_ACCUMULATE = 8 };   // what the entry points differ by

constexpr int DCN_TH = 8, DCN_TW = 16;              // output pixels of a window kernel's workgroup
constexpr int DCN_LDK = 36, DCN_LDKH = BK + 8;      // operand row pitch of the L2-gather forward: fp32 words / bf16 elements
constexpr long DCN_LDS_BUDGET = 160 * 1024 - 512;   // dynamic LDS a window kernel may ask for

struct DcnGeom {
    int n, h, w, c, k, r, s, stride, pad_h, pad_w, dil, dg;
};

// the fields every plan starts with.  refuse non-null: the pass does not take the call (a printf format for a0, a1) and nothing
// but P, Q, M is meaningful.  window 0: the L2-gather kernel, whose margin / WH / WW / tiles are unset.
struct DcnPlanHead {
    const char *refuse;
    int a0, a1;
    int P, Q, M;           // the output grid, n * P * Q
    int window, margin, WH, WW, tiles_y, tiles_x;
    int grid, lds;         // workgroups and dynamic LDS bytes of the GEMM kernel
};

// ---- what every pass checks first; the output grid
inline DcnPlanHead dcn_dims(const DcnGeom &g)
{
    DcnPlanHead d{};
    if (!(g.n > 0 && g.h > 0 && g.w > 0 && g.c > 0 && g.k > 0 && g.r > 0 && g.s > 0 && g.stride > 0 && g.dil > 0 && g.dg > 0)) {
        d.refuse = "rr_dcn: bad dims";
    } else if (!(g.c % 4 == 0 && g.c % g.dg == 0)) {
        d.refuse = "rr_dcn: C=%d must be a multiple of 4 and of deformable_groups=%d"; d.a0 = g.c; d.a1 = g.dg;
    } else if (!(g.dg == 1 || (g.c / g.dg) % BK == 0)) {
        d.refuse = "rr_dcn: channels per deformable group (%d) must be a multiple of 32"; d.a0 = g.c / g.dg;
    } else {
        d.P = (g.h + 2 * g.pad_h - (g.dil * (g.r - 1) + 1)) / g.stride + 1;
        d.Q = (g.w + 2 * g.pad_w - (g.dil * (g.s - 1) + 1)) / g.stride + 1;
        const long M = (long)g.n * d.P * d.Q;
        if (!(d.P > 0 && d.Q > 0)) d.refuse = "rr_dcn: empty output";
        else if (!(M < (1l << 31))) d.refuse = "rr_dcn: too many output pixels";
        else d.M = (int)M;
    }
    return d;
}

// ---- the LDS window: the pixel block, the filter's extent and a margin of m pixels for the offsets
struct DcnWindow {
    int WH, WW, npx;
};

inline DcnWindow dcn_window(int r, int s, int dil, int m)
{
    DcnWindow w;
    w.WH = DCN_TH + (r - 1) * dil + 2 * m + 1;
    w.WW = DCN_TW + (s - 1) * dil + 2 * m + 1;
    w.npx = w.WH * w.WW;
    return w;
}

// forward: the window's 32-channel chunk, the geometry tables (4 corner words + 4 weights per pixel and tap), two operand images
inline long dcn_fwd_win_lds(int r, int s, int dil, int m, int wbn)
{
    return (long)dcn_window(r, s, dil, m).npx * BK * 4 + (long)BM * r * s * 4 * 8 + 2l * 2 * (BM * DCN_LDKH + wbn * DCN_LDKH);
}

// weight gradient: window chunk, geometry, then the operands — dY as a 256 x 72 image beside the padded samples, or (dy_dma) as
// the ring of 8 waves x 6 slices of 1 KB beside the samples unpadded
inline long dcn_wgrad_win_lds(int r, int s, int dil, int m, bool dy_dma)
{
    const long operands = dy_dma ? 8 * 6 * 512 + r * s * 64 * 32 : (256 + r * s * 32) * 72;
    return 4l * (dcn_window(r, s, dil, m).npx * 32 + BM * r * s * 4) + 2l * operands;
}

// data gradient: two windows (d input in fixed point, input values) and the operand area: one image of the sweep (dY
// 128 x LDKH + weights taps x 32 x LDKH), and for the DMA sweep image 0 + the third dY image (128 x 32 + taps x 32 x 32 +
// 128 x 32) — the larger of the two
inline long dcn_dgrad_win_lds(int r, int s, int dil, int m)
{
    const int npx = dcn_window(r, s, dil, m).npx;
    const long staged = BM * DCN_LDKH + r * s * 32 * DCN_LDKH, dma = 2 * BM * 32 + r * s * 32 * 32;
    return 4l * (((npx * 33 + 3) & ~3) + BM * r * s * 7 + npx * 32) + 2l * (staged > dma ? staged : dma);
}

// the largest margin <= the requested one with which the pass's window fits, 0: none does.  variant: the forward's tile width
// (the forward also keeps the window within the 14 x 32 pixels its prefetch registers hold) / the weight gradient's dy_dma
inline int dcn_fit_margin(int pass, int r, int s, int dil, int variant, int requested)
{
    for (int m = requested; m >= 1; --m) {
        const long lds = pass == DCN_FWD ? dcn_fwd_win_lds(r, s, dil, m, variant)
                       : pass == DCN_WGRAD ? dcn_wgrad_win_lds(r, s, dil, m, variant != 0) : dcn_dgrad_win_lds(r, s, dil, m);
        if (lds <= DCN_LDS_BUDGET && (pass != DCN_FWD || dcn_window(r, s, dil, m).npx <= 14 * 32)) return m;
    }
    return 0;
}

inline void dcn_plan_window(DcnPlanHead &p, const DcnGeom &g, int margin)
{
    const DcnWindow w = dcn_window(g.r, g.s, g.dil, margin);
    p.window = 1; p.margin = margin; p.WH = w.WH; p.WW = w.WW;
    p.tiles_y = cdiv(p.P, DCN_TH); p.tiles_x = cdiv(p.Q, DCN_TW);
}

inline bool dcn_below_2g(long bytes) { return bytes < (1l << 31); }     // addressable with 32-bit buffer offsets

// ---- forward (rr_dcn_fwd, rr_dcn_fwd_bf16, rr_dcn_fwd_bf16_packed)
struct DcnFwdPlan : DcnPlanHead {
    int wbn;               // window kernel: 256 or 128 output channels per workgroup
    int bn;                // L2-gather kernel: 128 or 32
    int pack;              // bf16, 256 wide, workspace given: the weights are packed to bf16 in front and reach LDS by DMA
};

inline DcnFwdPlan dcn_fwd_plan(const DcnGeom &g, bool bf16, int flags, int margin)
{
    DcnFwdPlan p{dcn_dims(g)};
    if (p.refuse) return p;
    // stride 1 only: the window of a strided layer is not compact
    const bool takes = margin > 0 && g.stride == 1 && g.k > 32 && g.c % BK == 0 && (long)g.h * g.w < (1l << 30);
    p.wbn = (g.k % 256 == 0 || g.k > 384) ? 256 : 128;
    p.bn = g.k > 32 ? 128 : 32;
    const int m = takes ? dcn_fit_margin(DCN_FWD, g.r, g.s, g.dil, p.wbn, margin) : 0;
    if (m > 0) {
        dcn_plan_window(p, g, m);
        p.grid = g.n * p.tiles_y * p.tiles_x * cdiv(g.k, p.wbn);
        p.lds = (int)dcn_fwd_win_lds(g.r, g.s, g.dil, m, p.wbn);
        p.pack = p.wbn == 256 && bf16 && (flags & DCN_HAS_WPACK) && g.c % 32 == 0 && dcn_below_2g((long)g.k * g.r * g.s * g.c * 2);
    } else {
        p.grid = cdiv(p.M, BM) * cdiv(g.k, p.bn);
        p.lds = bf16 ? 2 * 2 * (BM * DCN_LDKH + p.bn * DCN_LDKH) : 4 * 2 * (BM * DCN_LDK + p.bn * DCN_LDK);
    }
    return p;
}

// ---- weight gradient (rr_dcn_wgrad, rr_dcn_wgrad_bf16, rr_dcn_wgrad_bf16_img)
struct DcnWgradPlan : DcnPlanHead {
    int dy_dma;            // window, bf16: dY's bf16 image feeds the operand by LDS-DMA
    int ktiles, per_split, splits;     // window: 256-filter tiles; (channel chunk, filter tile) pairs; pixel splits.  L2-gather: splits
    int dma_window;        // x is addressable with 32-bit byte offsets: the window goes global -> LDS by DMA
    int mt, nt, chunks_per_split;      // L2-gather: 128-filter / 128-channel tiles, K-steps per split
};

inline DcnWgradPlan dcn_wgrad_plan(const DcnGeom &g, bool bf16, int flags, int margin)
{
    DcnWgradPlan p{dcn_dims(g)};
    if (p.refuse) return p;
    const int cpg = g.c / g.dg;
    const bool x_below_2g = dcn_below_2g((long)g.n * g.h * g.w * g.c * 4);
    const bool takes = margin > 0 && g.stride == 1 && g.r * g.s == 9 && g.c % 32 == 0 && g.k % 4 == 0 && g.h < 32768 && g.w < 32768 &&
                       (g.dg == 1 || cpg % 32 == 0);
    const bool dy_dma = bf16 && (flags & DCN_HAS_DYB) && g.k % 32 == 0 && dcn_below_2g((long)p.M * g.k * 2) && x_below_2g;
    const int m = takes ? dcn_fit_margin(DCN_WGRAD, g.r, g.s, g.dil, dy_dma, margin) : 0;
    if (m > 0) {
        dcn_plan_window(p, g, m);
        p.dy_dma = dy_dma;
        p.lds = (int)dcn_wgrad_win_lds(g.r, g.s, g.dil, m, dy_dma);
        const int ntiles = g.n * p.tiles_y * p.tiles_x;
        p.ktiles = cdiv(g.k, 256);
        p.per_split = (g.c / 32) * p.ktiles;
        p.splits = cdiv(256, p.per_split);           // one workgroup per CU (the window leaves room for one)
        if (p.splits > 8) p.splits = p.splits / 8 * 8;
        if (p.splits > ntiles) p.splits = ntiles;
        p.grid = p.splits * p.per_split;
        p.dma_window = x_below_2g;
        return p;
    }
    // the L2-gather kernel: K % 4 == 0 and one deformable group per 128-channel tile
    if (g.k % 4 != 0) { p.refuse = "rr_dcn_wgrad: K=%d must be a multiple of 4"; p.a0 = g.k; return p; }
    if (!(g.dg == 1 || cpg % 128 == 0)) {
        p.refuse = "rr_dcn_wgrad: channels per deformable group (%d) must be a multiple of 128"; p.a0 = cpg;
        return p;
    }
    p.mt = cdiv(g.k, 128); p.nt = cdiv(g.c, 128);
    const int tiles = p.mt * p.nt * g.r * g.s;
    p.splits = pixel_splits(tiles, cdiv(p.M, BK), 512, 8, &p.chunks_per_split);
    p.grid = tiles * p.splits;
    p.lds = 4 * 2 * (BK * 128 + BK * 128);
    return p;
}

// ---- data gradient (rr_dcn_dgrad, _bf16, _bf16_ws, _bf16_img, _bf16_packed)
struct DcnDgradPlan : DcnPlanHead {
    int zero_dx;           // dx is zero-filled in front (every kernel ADDS into it); not when the caller accumulates
    int dy_image;          // window, bf16: the sweep reads dY's bf16 image ...
    int convert_dy;        // ... which a pass in front writes into the caller's buffer
    int dma_sweep;         // both sweep operands by LDS-DMA: the weights are packed to bf16 in front
    int goff_at;           // DMA sweep: byte offset of the window-pixel offset table (behind everything else; lds includes it)
};

inline DcnDgradPlan dcn_dgrad_plan(const DcnGeom &g, bool bf16, int flags, int margin)
{
    DcnDgradPlan p{dcn_dims(g)};
    if (p.refuse) return p;
    const int cpg = g.c / g.dg;
    if (g.k % 4 != 0) { p.refuse = "rr_dcn_dgrad: K=%d must be a multiple of 4"; p.a0 = g.k; return p; }
    if (!((long)g.n * g.h * g.w < (1l << 31))) { p.refuse = "rr_dcn_dgrad: input too large"; return p; }
    p.zero_dx = !(flags & DCN_ACCUMULATE);
    const bool takes = margin > 0 && g.stride == 1 && g.c % 32 == 0 && g.h < 32768 && g.w < 32768 && (g.dg == 1 || cpg % 32 == 0);
    // two windows live in LDS here: 2 pixels of margin for a 3x3 filter with dilation 1
    const int m = takes ? dcn_fit_margin(DCN_DGRAD, g.r, g.s, g.dil, 0, margin) : 0;
    if (g.r * g.s == 9 && m > 0) {
        dcn_plan_window(p, g, m);
        p.grid = g.n * p.tiles_y * p.tiles_x;
        const long lds = dcn_dgrad_win_lds(g.r, g.s, g.dil, m);
        p.lds = (int)lds;
        if (!bf16) return p;
        const long npx = (long)p.WH * p.WW;
        p.dy_image = (flags & DCN_HAS_DYB) != 0;       // the caller's (written by dY's producer), or converted here
        p.convert_dy = p.dy_image && !(flags & DCN_DYB_READY);
        p.dma_sweep = p.dy_image && (flags & DCN_HAS_WPACK) && g.k % 32 == 0 && dcn_below_2g((long)p.M * g.k * 2) &&
                      dcn_below_2g((long)g.n * g.h * g.w * g.c * 4) && npx <= 368 && lds + npx * 4 + 16 <= DCN_LDS_BUDGET &&
                      npx * 33 * 4 >= (long)(BM * 32 + 2 * g.r * g.s * 32 * 32) * 2;     // the ring's share of the d-input window
        if (p.dma_sweep) {
            p.goff_at = (int)lds;
            p.lds = (int)(lds + ((npx * 4 + 15) & ~15l));
        }
        return p;
    }
    if (!(g.dg == 1 || cpg % 128 == 0)) {
        p.refuse = "rr_dcn_dgrad: channels per deformable group (%d) must be a multiple of 128 on the L2-gather kernel"; p.a0 = cpg;
        return p;
    }
    p.grid = cdiv(p.M, BM);
    p.lds = 4 * (2 * (BM * DCN_LDK + BK * 128) + BM * 8 + BM * 4 + BM * 3);
    return p;
}

}  // namespace rr_plan
