// The host launch plan of the implicit-GEMM convolutions, plain C++ with no HIP include (it compiles with a host compiler alone).
// HOW a "forward-kernel" convolution launches — tile width, split-K, zero fill, statistics fused or in a second pass, which
// BatchNorm-backward sums ride in the epilogue — is decided in fprop_plan, for csrc/conv.hip (fp32) and csrc/conv_bf16.hip (16-bit)
// alike; rr_conv_fprop_plan (include/rrnet_hip.h) shows it to the tests, whose Python mirror (tests/helpers.py) answers to it.
// Next to it: the parity classes of a stride-2 data gradient and the pixel split of the weight gradients.
#pragma once
#include <stdlib.h>

namespace rr_plan {

enum { MATH_F32 = 0, MATH_BF16 = 1, MATH_F16X3 = 2 };                   // ops.MATH_*
enum { LINK_NONE = 0, LINK_BN = 1, LINK_RELU_BIAS = 2 };                // whose backward sums the epilogue carries (ConvArgs::bs_y)
enum { AFTER_NONE = 0, AFTER_REDUCE_SLAB = 1, AFTER_BWD_REDUCE = 2, AFTER_COLSTATS = 3 };   // FpropPlan::after

constexpr int BM = 128;   // rows of an output tile
constexpr int BK = 32;    // K-step depth

inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

inline int mid_tiles() { return 48; }       // <= 48 tiles of 128x128 (the 16x16 level): 128x64 tiles; measured worse at 192 (32x32)
inline int small_tiles() { return 16; }       // <= 16 tiles of 128x128 (the 8x8 level): 128x32 tiles give 4x the workgroups

// split-K factor for layers whose output has too few tiles to fill the chip
inline int pick_ksplit(int blocks, int nk)
{
    static int enabled = -1;
    if (enabled < 0) {
        const char *e = getenv("RR_CONV_SPLITK");
        enabled = (e && atoi(e) == 0) ? 0 : 1;
    }
    if (!enabled || blocks >= 256 || nk < 16) return 1;   // a full first wave of tiles: splitting costs more than it balances
    // Occupancy model: 256 CUs, two workgroups resident per CU.  A pair shares the MFMA pipes at ~0.87 of peak, a
    // lone workgroup reaches ~0.75 (nobody fills its issue gaps); every workgroup pays ~3 K-steps of prologue +
    // epilogue.  The busiest CU holds ceil(total / 256) workgroups; pick the split with the shortest makespan.
    int best = 1;
    float best_t = 0.f;
    for (int ks = 1; ks <= 8 && ks <= nk / 8; ++ks) {
        const int total = blocks * ks;
        const int n = (total + 255) / 256;
        const float per = (float)((nk + ks - 1) / ks) + 3.0f + (ks > 1 ? 1.0f : 0.0f);   // + atomic epilogue
        const float t = (float)(n / 2) * (2.0f * per / 0.87f) + (float)(n % 2) * (per / 0.75f);
        if (best_t == 0.f || t < best_t * 0.95f) { best = ks; best_t = t; }
    }
    return best;
}

struct ConvGeom {
    int n, h, w, c, k, r, s, stride, pad_h, pad_w;
    int out_h, out_w;      // > 0: the logical output grid given explicitly (pads are LEADING pads); 0: the symmetric formula
};

struct ConvFlags {
    bool bias, relu, stats;    // stats: the caller wants the column sums / sums of squares of y (stat_slab)
    int link;                  // LINK_*: the producer of the tensor whose gradient this launch writes
    bool accumulate, strided_dst;   // strided_dst: the destination is one parity class of a larger map (16-bit kernels, stride-2 data gradient)
};

struct FpropPlan {
    const char *refuse;   // non-null: this arithmetic does not take the call, and why; nothing else is meaningful then
    int dh, dw;           // output grid
    long M;               // n * dh * dw
    int rows;             // fp32: the row-streaming 1x1 kernel of csrc/headtail.hip takes the whole call; the rest is unset
    int scalar;           // fp32: scalar gather (channel counts not multiples of 4, or more taps than the 64-bit tap mask holds)
    int bn;               // tile width 128 / 64 / 32
    int blocks;           // workgroups per K slice
    int ks;               // split-K factor (grid.z)
    int pos_major;        // fp32: position-major M tiles (ConvArgs::pos_major)
    int xcd_n;            // 16-bit: every XCD works on one column tile (ConvArgs::xcd_n)
    int fused;            // the link's sums come out of the epilogue
    int after;            // AFTER_*: the pass behind the launch
    int zero_dst;         // split-K: the destination is zero-filled in front of the launch
    int zero_slab;        // ... and the statistics slab, which AFTER_COLSTATS then fills
};

inline FpropPlan fprop_plan(int math, const ConvGeom &g, const ConvFlags &f)
{
    FpropPlan p{};
    const bool b16 = math != MATH_F32;
    const int n = g.n, c = g.c, k = g.k, r = g.r, s = g.s;
    const long G2 = 1l << 31;
#define RR_PLAN_REFUSE(cond, why) do { if (cond) { p.refuse = why; return p; } } while (0)
    RR_PLAN_REFUSE(!(n > 0 && g.h > 0 && g.w > 0 && c > 0 && k > 0 && r > 0 && s > 0 && g.stride > 0), "bad dims");
    RR_PLAN_REFUSE(b16 && !(c % 4 == 0 && r * s <= 64), "C must be a multiple of 4 and R*S <= 64 (fp32 path for the rest)");
    RR_PLAN_REFUSE(!b16 && f.strided_dst, "a strided destination is for the 16-bit kernels");
    p.dh = g.out_h > 0 ? g.out_h : (g.h + 2 * g.pad_h - r) / g.stride + 1;
    p.dw = g.out_w > 0 ? g.out_w : (g.w + 2 * g.pad_w - s) / g.stride + 1;
    RR_PLAN_REFUSE(!(p.dh > 0 && p.dw > 0), "empty output");
    const long M = p.M = (long)n * p.dh * p.dw;
    const long src_bytes = (long)n * g.h * g.w * c * 4, w_bytes = (long)k * r * s * c * 4;
    if (b16) {
        RR_PLAN_REFUSE(!(M < G2 && src_bytes < G2 && w_bytes < G2 && M * k * 4 < G2), "tensors must stay below 2 GiB (32-bit buffer offsets)");
        RR_PLAN_REFUSE(f.strided_dst && (f.link != LINK_NONE || f.stats), "strided destination without fused sums");
    } else {
        RR_PLAN_REFUSE(!(M < G2 && src_bytes / 4 < (1l << 40)), "tensor too large");
    }
    // 1x1 to 49..64 channels (both 32-column tiles of the rows kernel in use) on very many rows without statistics — the
    // stage-2 head's conv1 at inference: the row-streaming kernel of csrc/headtail.hip (weights in registers, no per-tile
    // prologue)
    if (!b16 && r == 1 && s == 1 && g.stride == 1 && g.pad_h == 0 && g.pad_w == 0 && (c == 128 || c == 256) && k > 48 && k <= 64
        && !f.stats && f.link == LINK_NONE && !f.accumulate && M >= 64 * 1024 && M * c * 4 < G2) {
        p.rows = 1;
        return p;
    }
    const bool scalar = !b16 && ((c % 4) != 0 || r * s > 64);   // the vector path keeps a 64-bit tap mask per row
    int bn = k > 64 ? 128 : (k > 32 ? (!scalar ? 64 : 128) : 32);
    if (bn == 128 && !scalar && cdiv(M, BM) * cdiv(k, 128) <= small_tiles()) bn = 32;   // tiny layers: 4x the tiles
    else if (bn == 128 && !scalar && cdiv(M, BM) * cdiv(k, 128) <= mid_tiles()) bn = 64;
    p.scalar = scalar; p.bn = bn;
    p.blocks = cdiv(M, BM) * cdiv(k, bn);
    const int nt = cdiv(k, bn), mt = cdiv(M, BM);
    p.xcd_n = b16 && nt > 1 && 8 % nt == 0 && mt % (8 / nt) == 0;
    const int nk = scalar ? cdiv((long)r * s * c, BK) : cdiv(c, BK) * r * s;
    p.ks = (!f.bias && !f.relu && k % 4 == 0 && k <= 1024) ? pick_ksplit(p.blocks, nk) : 1;
    if (f.link == LINK_RELU_BIAS) p.ks = 1;      // the masked store needs the complete value in one workgroup
    if (f.strided_dst) p.ks = 1;                 // (the zero fill of a split-K destination would wipe the other parity classes)
    // padded filter on a tiny map, many images (the stage-2 head on 3x3 RoI maps): one output pixel per M tile, padding
    // taps skipped (ConvArgs::pos_major).  Not with statistics in the epilogue (their slab is sized by ceil(M/128) tiles).
    // The variant exists for the pipelined 128- and 64-column kernels (32-bit buffer offsets).
    if (!b16 && !scalar && !f.stats && f.link == LINK_NONE && (g.pad_h > 0 || g.pad_w > 0) && r * s > 1
        && p.dh * p.dw <= 16 && n >= 16 * BM && bn >= 64 && src_bytes < G2 && w_bytes < G2) {
        p.pos_major = p.ks = 1;
        p.blocks = p.dh * p.dw * cdiv(n, BM) * cdiv(k, bn);
    }
    // The epilogue reads the producer's tensors through buffer descriptors with the row inside the tile in the SCALAR offset,
    // which the hardware's range check does not cover: in a partial last tile it would read up to 11 rows past the end of
    // the tensor.  Fused sums therefore only for M % 128 == 0 (every size the training configurations produce); other
    // sizes take the separate reduce pass, and the masked-store mode — which has no such fallback — is refused.
    // The same epilogue reaches the destination and the producer's tensors through 32-bit offsets: below 2 GiB only.
    const bool tiles_full = M % BM == 0 && M * k * 4 < G2;
    RR_PLAN_REFUSE(f.link == LINK_RELU_BIAS && !tiles_full, "N*H*W must be a multiple of 128 and dx smaller than 2 GiB");
#undef RR_PLAN_REFUSE
    p.fused = f.link != LINK_NONE && p.ks == 1 && tiles_full;   // with split-K the complete values exist only afterwards
    p.zero_dst = p.ks > 1 && !f.accumulate;
    p.zero_slab = p.ks > 1 && f.stats && f.link == LINK_NONE;
    p.after = f.link != LINK_NONE ? (p.fused ? AFTER_REDUCE_SLAB : AFTER_BWD_REDUCE) : (p.zero_slab ? AFTER_COLSTATS : AFTER_NONE);
    return p;
}

// ---- stride-2 data gradient: four stride-1 correlations, one per output parity class (ph, pw) = (h % 2, w % 2), each with
// the sub-filter of the taps r = r0 + 2i, s = s0 + 2j that reach the class
constexpr int parity_first_tap(int parity, int pad) { return (parity + pad) & 1; }
constexpr int parity_span(int r, int r0) { return (r - r0 + 1) / 2; }                  // taps r0, r0 + 2, .. below r (r0 <= r)
constexpr int parity_extent(int r, int r0) { return r0 < r ? (r - r0 + 1) / 2 : 0; }

struct ParityClass {
    int ph, pw;            // the class, in the order (0,0), (0,1), (1,0), (1,1)
    int Rc, Sc;            // sub-filter extent; taps() == 0: no tap reaches the class, its pixels are zero
    int lead_h, lead_w;    // leading pads of the class's stride-1 correlation
    int Hc, Wc;            // class image size
    int taps_before;       // block offset in the packed filter, in units of C*K elements
    int taps() const { return Rc * Sc; }
};

// -> true if a class that has pixels has no tap
inline bool parity_classes(int h, int w, int r, int s, int pad_h, int pad_w, ParityClass (&cls)[4])
{
    bool any_empty = false;
    int before = 0;
    for (int cl = 0; cl < 4; ++cl) {
        ParityClass &p = cls[cl];
        p.ph = cl >> 1; p.pw = cl & 1;
        const int r0 = parity_first_tap(p.ph, pad_h), s0 = parity_first_tap(p.pw, pad_w);
        p.Rc = parity_extent(r, r0); p.Sc = parity_extent(s, s0);
        p.lead_h = (p.Rc - 1) - (p.ph + pad_h - r0) / 2;
        p.lead_w = (p.Sc - 1) - (p.pw + pad_w - s0) / 2;
        p.Hc = (h - p.ph + 1) / 2; p.Wc = (w - p.pw + 1) / 2;
        p.taps_before = before;
        before += p.taps();
        if (p.Hc > 0 && p.Wc > 0 && p.taps() == 0) any_empty = true;
    }
    return any_empty;
}

// ---- weight gradients: split the pixel (K) dimension so that tiles * splits fills the `slots` resident workgroups exactly once (equal-length
// workgroups in more than one round pay a whole extra round for any remainder), never fewer than `min_chunks` K-steps per split.  -> splits
inline int pixel_splits(int tiles, int total_chunks, int slots, int min_chunks, int *per_split)
{
    int splits = tiles < slots ? slots / tiles : 1;
    if (splits > cdiv(total_chunks, min_chunks)) splits = cdiv(total_chunks, min_chunks);
    if (splits < 1) splits = 1;
    *per_split = cdiv(total_chunks, splits);
    return cdiv(total_chunks, *per_split);
}

}  // namespace rr_plan
