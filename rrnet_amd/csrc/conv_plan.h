// The host launch plans of the convolutions, plain C++ with no HIP include (it compiles with a host compiler alone).
// HOW a "forward-kernel" convolution launches — tile width, split-K, zero fill, statistics fused or in a second pass, which
// BatchNorm-backward sums ride in the epilogue — is decided in fprop_plan, for csrc/conv.hip (fp32) and csrc/conv_bf16.hip (16-bit)
// alike; rr_conv_fprop_plan (include/rrnet_hip.h) shows it to the tests, whose Python mirror (tests/helpers.py) answers to it.
// The gradients have the same arrangement: dgrad_plan (rr_conv_dgrad), dgrad_s2_plan (the parity-class data gradients of
// conv_bf16.hip and conv16.hip) and wgrad_plan (the weight gradients of all three files) decide, the entry points carry out, and
// rr_conv_grad_plan shows them.  Next to them: the tile rule and shape predicates of csrc/conv16.hip.
#pragma once
#include <stdlib.h>

namespace rr_plan {

enum { MATH_F32 = 0, MATH_BF16 = 1, MATH_F16X3 = 2 };                   // ops.MATH_*
enum { FAM_CONV16 = 3 };                                                // a gradient plan's family: a MATH_*, or the 16-bit-activation kernels of csrc/conv16.hip
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

// ---- the gradient passes.  A plan's refusal: why, a printf format for a[] without the entry point's name (null: the call is taken)
struct Refusal { const char *why; int a[5]; };
enum { GRAD_DGRAD = 0, GRAD_DGRAD_S2 = 1, GRAD_WGRAD = 2 };              // the pass argument of rr_conv_grad_plan

// ---- rr_conv_dgrad (fp32, any stride): the gather kernel of csrc/conv.hip, at stride 2 over the parity classes in one launch
struct DgradPlan {
    Refusal refuse;
    long M;               // n * h * w
    int scalar;           // scalar gather
    int bn;               // tile width 128 / 64 / 32
    int blocks, gy;       // grid.x: workgroups of one class (of the whole map without parity); grid.y: the classes that have taps
    int parity;           // stride 2 on the vector kernels: parity-decomposed, 4 classes of ceil(h/2) x ceil(w/2) pixels each
    int parity_order;     // the classes by falling tap count, two bits each (ConvArgs::parity_order)
    int ks;               // split-K factor (grid.z)
    int zero_dst;         // dx is zero-filled in front: a class without taps, or split-K, and the call does not accumulate
};

inline DgradPlan dgrad_plan(const ConvGeom &g, bool accumulate)
{
    DgradPlan p{};
    const int n = g.n, h = g.h, w = g.w, c = g.c, k = g.k, r = g.r, s = g.s, stride = g.stride;
    if (!(n > 0 && h > 0 && w > 0 && c > 0 && k > 0 && r > 0 && s > 0 && stride > 0)) { p.refuse = {"bad dims"}; return p; }
    const long M = p.M = (long)n * h * w;
    if (!(M < (1l << 31))) { p.refuse = {"tensor too large"}; return p; }
    const bool scalar = (k % 4) != 0 || (c % 4) != 0 || r * s > 64 || stride > 2;
    int bn = c > 64 ? 128 : (c > 32 ? (!scalar ? 64 : 128) : 32);
    if (bn == 128 && !scalar && stride == 1 && cdiv(M, BM) * cdiv(c, 128) <= small_tiles()) bn = 32;
    else if (bn == 128 && !scalar && stride == 1 && cdiv(M, BM) * cdiv(c, 128) <= mid_tiles()) bn = 64;
    p.scalar = scalar; p.bn = bn; p.gy = 1;
    p.blocks = cdiv(M, BM) * cdiv(c, bn);
    int nk = scalar ? cdiv((long)r * s * k, BK) : cdiv(k, BK) * r * s;
    if (stride == 2 && !scalar) {
        p.parity = 1;
        ParityClass cls[4];
        parity_classes(h, w, r, s, g.pad_h, g.pad_w, cls);
        int ord[4] = {0, 1, 2, 3};
        for (int i = 0; i < 4; ++i)
            for (int j = i + 1; j < 4; ++j)
                if (cls[ord[j]].taps() > cls[ord[i]].taps()) { const int t = ord[i]; ord[i] = ord[j]; ord[j] = t; }
        p.parity_order = ord[0] | (ord[1] << 2) | (ord[2] << 4) | (ord[3] << 6);
        // classes without any tap (1x1 stride 2: three of four) produce zeros: one memset instead of workgroups
        // that run an empty K loop and store zeros element by element
        // (when accumulating they add nothing: no workgroups at all)
        p.gy = 4;
        while (p.gy > 1 && cls[ord[p.gy - 1]].taps() == 0) --p.gy;
        p.blocks = cdiv((long)n * ((h + 1) / 2) * ((w + 1) / 2), BM) * cdiv(c, bn);
        nk = cdiv(k, BK) * ((r + 1) / 2) * ((s + 1) / 2);
    }
    p.ks = p.parity ? 1 : pick_ksplit(p.blocks, nk);
    p.zero_dst = ((p.parity && p.gy < 4) || p.ks > 1) && !accumulate;
    return p;
}

// ---- csrc/conv16.hip: which shapes its kernels take, and the forward kernel's tile (fprop, stride-1 and parity-class data gradients)
inline bool conv16_supported(int c, int k, int r, int s, int stride) { return c % 64 == 0 && k % 128 == 0 && r * s <= 16 && (stride == 1 || stride == 2); }
inline bool conv16_wgrad_supported(int c, int k, int r, int s, int stride)
{
    return k % 128 == 0 && c % 128 == 0 && r * s <= 64 && (stride == 1 || stride == 2);     // (K % 256 == 128: the last 256-filter tile runs half empty)
}
struct Conv16Tile { int tch, grid, lds; };     // output channels per tile (256 pixels wide), workgroups, dynamic LDS bytes
inline Conv16Tile conv16_tile(long M, int dc)
{
    if (dc % 256 == 0) return {256, cdiv(M, 256) * (dc / 256), 2 * (256 * 128 + 256 * 128)};   // 2 buffers x (pixel image + filter image, 128-byte rows)
    return {128, cdiv(M, 256) * (dc / 128), 128 * 1024};                                         // (two buffers need 96 KiB; the statistics epilogue's table 128)
}

// ---- the parity-class data gradients rr_conv_dgrad_s2_bf16 / _f16x3 (family MATH_BF16 / MATH_F16X3) and rr_conv16_dgrad_s2
// (FAM_CONV16): one forward-kernel launch per class that has taps and pixels, into a strided destination.  How each of them
// launches is fprop_plan's decision (strided_dst) or conv16_tile's.
struct DgradS2Plan {
    Refusal refuse;
    int p, q;             // dy's grid
    int zero_dst;         // dx is zero-filled in front: a class with pixels has no tap, and the call does not accumulate
    int n_launch;
    ParityClass cls[4];   // the classes that launch, in their order
    int blocks[4];        // FAM_CONV16: workgroups of the class's launch
};

// ptrs: the scratch (and the split operands' maxima) are there — their absence shares a refusal text with the shape
inline DgradS2Plan dgrad_s2_plan(int family, const ConvGeom &g, bool accumulate, bool ptrs = true)
{
    DgradS2Plan p{};
    const int n = g.n, h = g.h, w = g.w, c = g.c, k = g.k, r = g.r, s = g.s, pad_h = g.pad_h, pad_w = g.pad_w;
#define RR_PLAN_REFUSE(cond, ...) do { if (cond) { p.refuse = {__VA_ARGS__}; return p; } } while (0)
    if (family == FAM_CONV16) {
        RR_PLAN_REFUSE(!(n > 0 && h > 0 && w > 0 && pad_h >= 0 && pad_w >= 0 && ptrs), "bad arguments");
        RR_PLAN_REFUSE(!(k % 64 == 0 && c % 128 == 0 && r * s <= 16), "unsupported shape c=%d k=%d %dx%d", {c, k, r, s});
    } else {
        RR_PLAN_REFUSE(!(n > 0 && h > 0 && w > 0 && c > 0 && k > 0 && r > 0 && s > 0), "bad dims");
        RR_PLAN_REFUSE(!(c % 4 == 0 && k % 4 == 0 && r * s <= 64 && pad_h >= 0 && pad_w >= 0 && ptrs),
                       "C, K multiples of 4, R*S <= 64, scratch of k*r*s*c floats (and, split operands, the two maxima) required");
    }
    p.p = (h + 2 * pad_h - r) / 2 + 1; p.q = (w + 2 * pad_w - s) / 2 + 1;
    if (family == FAM_CONV16) RR_PLAN_REFUSE(!(p.p > 0 && p.q > 0 && (long)n * p.p * p.q * k * 2 < (1l << 31)), "empty or oversized dy");
    else RR_PLAN_REFUSE(!(p.p > 0 && p.q > 0), "empty dy");
    ParityClass cls[4];
    const bool any_empty = parity_classes(h, w, r, s, pad_h, pad_w, cls);
    for (const ParityClass &pc : cls)
        RR_PLAN_REFUSE(!(pc.taps() == 0 || (pc.lead_h >= 0 && pc.lead_w >= 0)), "unsupported padding %d,%d", {pad_h, pad_w});
#undef RR_PLAN_REFUSE
    p.zero_dst = any_empty && !accumulate;      // parity classes no tap reaches (a 1x1 stride 2: three of four) are zero
    for (const ParityClass &pc : cls) {
        if (pc.taps() == 0 || pc.Hc <= 0 || pc.Wc <= 0) continue;
        if (family == FAM_CONV16) p.blocks[p.n_launch] = conv16_tile((long)n * pc.Hc * pc.Wc, c).grid;
        p.cls[p.n_launch++] = pc;
    }
    return p;
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

// the slots and the fewest K-steps per split of each weight-gradient kernel
struct WgradFill { int slots, min_chunks; };
constexpr WgradFill WGRAD_F32_PIPE3 = {768, 8};      // resident workgroups: 256 CUs x 3 with one LDS image,
constexpr WgradFill WGRAD_F32 = {512, 8};            // else x 2
constexpr WgradFill WGRAD_BF16 = {1024, 16};         // 256 CUs x 4, never fewer than 16 K-steps per split;
constexpr WgradFill WGRAD_F16X3 = {512, 16};         // x 2 for the split kernel's 68 KB of LDS
constexpr WgradFill WGRAD_CONV16 = {512, 32};        // the 256 CUs (one 512-thread workgroup each) about twice, never fewer than 32 K-steps per split

// rr_conv_wgrad (MATH_F32), rr_conv_wgrad_bf16 / _f16x3, rr_conv16_wgrad (FAM_CONV16, which has no out_h / out_w override)
struct WgradPlan {
    Refusal refuse;
    int P, Q;             // dy's grid.  out_h / out_w > 0 override the symmetric-padding output size (pad_h / pad_w are the LEADING pads;
                          // taps that fall past the far edge are masked), which is how asymmetric padding is expressed
    long M;               // n * P * Q
    int bm, bn;           // tile: filters x channels (fp32: 128|32 x 128|32, 16-bit: 128 x 128, conv16: 256 x 256|128)
    int a_scalar, b_scalar, pipe;    // fp32: scalar loads of dy / x (K / C not multiples of 4); PIPE of the 128x128 kernel, 0: the generic tiles
    int mt, nt, tiles;    // tiles along K and C; mt * nt * r * s
    int splits, per_split, grid, lds;
};

inline WgradPlan wgrad_plan(int family, const ConvGeom &g)
{
    WgradPlan p{};
    const int n = g.n, h = g.h, w = g.w, c = g.c, k = g.k, r = g.r, s = g.s, stride = g.stride;
    const long G2 = 1l << 31;
    const bool conv16 = family == FAM_CONV16;
#define RR_PLAN_REFUSE(cond, ...) do { if (cond) { p.refuse = {__VA_ARGS__}; return p; } } while (0)
    if (conv16) {
        RR_PLAN_REFUSE(!(n > 0 && h > 0 && w > 0), "bad arguments");
        RR_PLAN_REFUSE(!conv16_wgrad_supported(c, k, r, s, stride), "unsupported shape c=%d k=%d %dx%d stride %d", {c, k, r, s, stride});
    } else {
        RR_PLAN_REFUSE(!(n > 0 && h > 0 && w > 0 && c > 0 && k > 0 && r > 0 && s > 0 && stride > 0), "bad dims");
        RR_PLAN_REFUSE(family != MATH_F32 && !(c % 4 == 0 && k % 4 == 0), "C=%d, K=%d must be multiples of 4 (fp32 path for the rest)", {c, k});
    }
    p.P = g.out_h > 0 && !conv16 ? g.out_h : (h + 2 * g.pad_h - r) / stride + 1;
    p.Q = g.out_w > 0 && !conv16 ? g.out_w : (w + 2 * g.pad_w - s) / stride + 1;
    const long M = p.M = (long)n * p.P * p.Q, x_elems = (long)n * h * w * c;
    WgradFill fill;
    if (conv16) {
        RR_PLAN_REFUSE(!(p.P > 0 && p.Q > 0), "empty output");
        RR_PLAN_REFUSE(!(M * k * 2 < G2 && x_elems * 2 < G2), "tensor beyond 2 GiB");
        p.bm = 256; p.bn = c % 256 == 0 ? 256 : 128;
        p.mt = cdiv(k, 256); p.nt = c / p.bn;
        fill = WGRAD_CONV16;
        p.lds = 4 * (8 * 2048 + (p.bn / 32) * 2048);       // 4 stages x (dY blocks + X blocks of [32 pixels][32 channels] bf16)
    } else if (family != MATH_F32) {
        RR_PLAN_REFUSE(!(M > 0 && M < G2 && M * k * 4 < G2 && x_elems * 4 < G2), "tensors must stay below 2 GiB (32-bit buffer offsets)");
        p.bm = p.bn = 128;
        p.mt = cdiv(k, 128); p.nt = cdiv(c, 128);
        fill = family == MATH_F16X3 ? WGRAD_F16X3 : WGRAD_BF16;
        p.lds = 2 * 4 * 4 * (32 * 32 + 32) * (family == MATH_F16X3 ? 2 : 1);  // 2 operands x 2 buffers x (parts) x 4 blocks of 32 x 32 (+ pad), 16-bit
    } else {
        RR_PLAN_REFUSE(!(M > 0 && M < G2), "bad pixel count");
        p.bm = k > 32 ? 128 : 32; p.bn = c > 32 ? 128 : 32;
        p.mt = cdiv(k, p.bm); p.nt = cdiv(c, p.bn);
        p.a_scalar = (k % 4) != 0; p.b_scalar = (c % 4) != 0;
        // pipelined 128x128 variants: 32-bit buffer offsets, both tensors below 2 GiB
        const bool pipe_ok = p.bm == 128 && p.bn == 128 && !p.a_scalar && !p.b_scalar && M * k * 4 < G2 && x_elems * 4 < G2;
        p.pipe = !pipe_ok ? 0 : (p.Q % BK == 0 ? 3 : 1);
        fill = p.pipe == 3 ? WGRAD_F32_PIPE3 : WGRAD_F32;
        p.lds = 4 * (p.pipe == 3 ? 1 : 2) * (BK * p.bm + BK * p.bn);
    }
#undef RR_PLAN_REFUSE
    p.tiles = p.mt * p.nt * r * s;
    p.splits = pixel_splits(p.tiles, cdiv(M, BK), fill.slots, fill.min_chunks, &p.per_split);     // (every kernel's K-step is 32 pixels)
    p.grid = p.tiles * p.splits;
    return p;
}

// ---- the rows route of csrc/conv_rows.hip (rr_conv_dgrad_s1_rows, rr_conv_wgrad_rows): grids sized for max_rows list entries, the
// workgroups past the count the device finds leave at once
constexpr int ROWS_DGRAD_BM = 64;          // listed dx pixels of a data-gradient tile (x 128 channels)
constexpr int ROWS_WGRAD_SLOTS = 1024;     // weight gradient: 256 CUs x 4 resident workgroups (32 KiB of LDS each) ...
constexpr int ROWS_WGRAD_MIN_CHUNKS = 4;   // ... and never fewer than 4 K-steps of 32 list rows per split (WROWS_MIN_CHUNKS of the kernel)
struct RowsPlan {
    int dgrad_x, dgrad_y;     // target tiles; channel tiles
    int mt, nt, splits, wgrad_grid;
};

inline RowsPlan rows_plan(int max_rows, int c, int k, int r, int s)
{
    RowsPlan p{};
    p.dgrad_x = cdiv(max_rows, ROWS_DGRAD_BM);
    p.dgrad_y = cdiv(c, 128);
    p.mt = cdiv(k, 128); p.nt = cdiv(c, 128);
    const int tiles = p.mt * p.nt * r * s;
    p.splits = ROWS_WGRAD_SLOTS / tiles > 1 ? ROWS_WGRAD_SLOTS / tiles : 1;
    const int most = cdiv(cdiv(max_rows, BK), ROWS_WGRAD_MIN_CHUNKS);
    if (p.splits > most) p.splits = most;
    p.wgrad_grid = tiles * p.splits;          // (0 with max_rows == 0: nothing to launch)
    return p;
}

// ---- the Winograd F(2x2,3x3) route of csrc/conv_wino.hip (rr_conv_wino_fprop, rr_conv_wino_dgrad_bnsum): input transform, sixteen
// GEMMs in one launch of conv.hip's forward kernel, output transform with the forward kernel's epilogue.  Additive: a launch it
// does not take stays with fprop_plan.  g is the FORWARD geometry of the launch (a stride-1 data gradient: dy's map, c = its
// channels, k = dx's), f the forward kernel's flags.
constexpr long WINO_MIN_PIXELS = 65536;    // the gate's floor in output pixels n*p*q: above it lie the 128 x 128 and 256 x 256 levels of
                                           // the headline step.  Measured, the route also wins at 32768 and 8192 pixels (8 x 64 x 64 x 384: 0.40
                                           // against 0.62 ms; 8 x 32 x 32 x 384: 0.105 against 0.18-0.19), but the launches of fp32 data gradients of
                                           // 8192 and of 32768 pixels are pinned to the direct entry points (tests/golden/conv_bwd_routes.json,
                                           // tests/test_bn_forward_gpu.py), and below 8192 the small-shape contracts are the direct route's
constexpr int WINO_OUT_LANES = 4;          // output transform: tile lanes of a workgroup (x 64 channel quads)
struct WinoPlan {
    const char *refuse;   // non-null: the route does not take the launch, and why
    int floor_only;       // ... and the pixel floor is the only reason (the entry points run such a shape: tests, benchmarks)
    int th, tw;           // tiles along h and w
    long tiles;           // T = n * th * tw
    int bn;               // GEMM tile width (conv_igemm_kernel<bn>, 128 rows)
    int gemm_blocks;      // GEMM workgroups per batch index (grid.x; grid.y = 16)
    int out_x, out_y;     // output transform: one workgroup per statistics-slab row x 256-channel slice
    int tiles_per_wg;     // ... and the tiles each of them walks
    long ws_bytes;        // V [16][T][c] + M [16][T][k]
};

inline WinoPlan wino_plan(int math, const ConvGeom &g, const ConvFlags &f)
{
    WinoPlan p{};
    const long G2 = 1l << 31;
#define RR_PLAN_REFUSE(cond, why) do { if (cond) { p.refuse = why; return p; } } while (0)
    RR_PLAN_REFUSE(!(g.n > 0 && g.h > 0 && g.w > 0 && g.c > 0 && g.k > 0), "bad dims");
    RR_PLAN_REFUSE(math != MATH_F32, "fp32 arithmetic only");
    RR_PLAN_REFUSE(!(g.r == 3 && g.s == 3 && g.stride == 1 && g.pad_h == 1 && g.pad_w == 1), "3x3, stride 1, pad 1 only");
    RR_PLAN_REFUSE(g.out_h > 0 || g.out_w > 0, "no explicit output size");
    RR_PLAN_REFUSE(!(g.c % 4 == 0 && g.k % 4 == 0), "C and K must be multiples of 4");
    RR_PLAN_REFUSE(f.strided_dst, "no strided destination");
    RR_PLAN_REFUSE(f.link == LINK_RELU_BIAS, "the conv + bias + ReLU link is not built on this route");
    RR_PLAN_REFUSE(f.link == LINK_BN && (f.bias || f.relu || f.stats || g.k > 1024), "a BatchNorm link: plain data gradient, at most 1024 channels");
    const long M = (long)g.n * g.h * g.w;
    p.th = (g.h + 1) / 2; p.tw = (g.w + 1) / 2;
    p.tiles = (long)g.n * p.th * p.tw;
    // every tensor, and every batch slice of V and M (each addressed from its own base), through 32-bit byte offsets
    RR_PLAN_REFUSE(!(M * g.c * 4 < G2 && M * g.k * 4 < G2 && 9l * g.c * g.k * 4 < G2 && p.tiles * g.c * 4 < G2 && p.tiles * g.k * 4 < G2),
                   "tensors must stay below 2 GiB");
    p.bn = g.k > 64 ? 128 : 64;
    p.gemm_blocks = cdiv(p.tiles, BM) * cdiv(g.k, p.bn);
    p.out_x = cdiv(M, BM);
    p.out_y = cdiv(g.k / 4, 64);
    p.tiles_per_wg = cdiv(p.tiles, p.out_x);
    p.ws_bytes = 16l * p.tiles * ((long)g.c + g.k) * 4;
    if (M < WINO_MIN_PIXELS) { p.refuse = "fewer output pixels than the route's floor"; p.floor_only = 1; }
#undef RR_PLAN_REFUSE
    return p;
}

// ---- the Winograd F(3x3,2x2) weight gradient of the same layers (rr_conv_wino_wgrad): input transform of x, transform
// of dy, sixteen GEMMs S[i] = W[i]^T V[i] over the T tiles in one launch of conv.hip's weight-gradient kernel (batch mode), and
// dw += Gt S G.  Additive: a launch it does not take stays with wgrad_plan.
constexpr long WINO_WGRAD_MIN_PIXELS = 65536;     // the gate's floor in pixels n*p*q: the 128 x 128 and 256 x 256 levels of the headline step

// the GEMM launch: 128 x 128 tiles of (filters x channels) x 16 slices, the T tiles of the map split like wgrad_plan splits its pixels
struct WinoWgradGemm { int mt, nt, pipe, splits, per_split, grid, lds; };
inline WinoWgradGemm wino_wgrad_gemm_plan(long tiles, int c, int k)
{
    WinoWgradGemm p{};
    p.mt = cdiv(k, 128); p.nt = cdiv(c, 128);
    p.pipe = tiles % BK == 0 ? 3 : 1;           // PIPE 3: every K-step of 32 tiles lies inside the one "row" of T
    const WgradFill fill = p.pipe == 3 ? WGRAD_F32_PIPE3 : WGRAD_F32;
    p.splits = pixel_splits(p.mt * p.nt * 16, cdiv(tiles, BK), fill.slots, fill.min_chunks, &p.per_split);
    p.grid = p.mt * p.nt * 16 * p.splits;
    p.lds = 4 * (p.pipe == 3 ? 1 : 2) * (BK * 128 + BK * 128);
    return p;
}

struct WinoWgradPlan {
    const char *refuse;   // non-null: the route does not take the launch, and why
    int floor_only;       // ... and the pixel floor is the only reason (the entry points run such a shape: tests, benchmarks)
    int th, tw;           // tiles along h and w
    long tiles;           // T = n * th * tw
    WinoWgradGemm gemm;
    long ws_bytes;        // V [16][T][c] + W [16][T][k] + S [k][16][c]
};

// g: the layer's geometry (x's map, c / k its channels / filters); gated: the launch carries a gate (rr_conv_wgrad_unless)
inline WinoWgradPlan wino_wgrad_plan(int math, const ConvGeom &g, bool gated)
{
    WinoWgradPlan p{};
    const long G2 = 1l << 31;
#define RR_PLAN_REFUSE(cond, why) do { if (cond) { p.refuse = why; return p; } } while (0)
    RR_PLAN_REFUSE(!(g.n > 0 && g.h > 0 && g.w > 0 && g.c > 0 && g.k > 0), "bad dims");
    RR_PLAN_REFUSE(math != MATH_F32, "fp32 arithmetic only");
    RR_PLAN_REFUSE(!(g.r == 3 && g.s == 3 && g.stride == 1 && g.pad_h == 1 && g.pad_w == 1), "3x3, stride 1, pad 1 only");
    RR_PLAN_REFUSE(g.out_h > 0 || g.out_w > 0, "no explicit output size");
    RR_PLAN_REFUSE(!(g.c % 4 == 0 && g.k % 4 == 0 && g.c > 32 && g.k > 32), "C and K must be multiples of 4 above 32");
    RR_PLAN_REFUSE(gated, "no gated launch");
    const long M = (long)g.n * g.h * g.w;
    p.th = (g.h + 1) / 2; p.tw = (g.w + 1) / 2;
    p.tiles = (long)g.n * p.th * p.tw;
    // every tensor, and every slice of V and W (each addressed from its own base), through 32-bit byte offsets
    RR_PLAN_REFUSE(!(M * g.c * 4 < G2 && M * g.k * 4 < G2 && 16l * g.c * g.k * 4 < G2 && p.tiles * g.c * 4 < G2 && p.tiles * g.k * 4 < G2),
                   "tensors must stay below 2 GiB");
    p.gemm = wino_wgrad_gemm_plan(p.tiles, g.c, g.k);
    p.ws_bytes = (16l * p.tiles * ((long)g.c + g.k) + 16l * g.k * g.c) * 4;
    if (M < WINO_WGRAD_MIN_PIXELS) { p.refuse = "fewer pixels than the route's floor"; p.floor_only = 1; }
#undef RR_PLAN_REFUSE
    return p;
}

}  // namespace rr_plan
