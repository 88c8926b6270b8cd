// 16-bit-operand NHWC convolutions on the gfx950 matrix cores, fp32 accumulation.  Two arithmetics share the kernels:
//   bf16   (rr_conv_*_bf16, cfg.Model.bf16 — BASELINE config 4): each operand rounded to ONE bf16 value;
//   f16x3  (rr_conv_*_f16x3, cfg.Model.conv_math — an fp32-class arithmetic): each operand the sum of TWO fp16 values after a
//          power-of-two scaling by the tensor's maximum, three products per tile (template parameters SP = 2, F16; the
//          entry points and their contract: the "Split-operand entry points" section at the end of this file).
// The headline configuration stays on csrc/conv.hip (v_mfma_f32_32x32x2_f32).  What follows describes the bf16 form.
//
// The reference is fp32-only (/root/reference/backbones/hourglass.py:12-61,127-199 through nn.Conv2d / cuDNN), so this
// precision is builder-defined: activations, weights, gradients and every BatchNorm / loss / optimizer quantity stay
// fp32 in HBM; the two operands of a convolution are rounded to bf16 (round-to-nearest-even, v_cvt_pk_bf16_f32) on
// their way into LDS and multiplied with fp32 accumulation.  Parity contract (tests/test_conv_bf16_gpu.py): every kernel
// equals the fp32 kernel of csrc/conv.hip run on bf16-rounded operands within 1e-5 of the output scale (products of two
// bf16 values are exact in fp32: only the summation order differs).
//
// Same implicit GEMMs as csrc/conv.hip, no column matrix:
//   fprop : Y[m,ko]  = sum_{tap,c} X[pix(m,tap), c] * W[ko,tap,c]      M = N*P*Q, N = K, Kg = R*S*C
//   dgrad : stride 1 = fprop of dY with the flipped / transposed filter (rr_weight_flip_transpose), as in conv.hip
//   wgrad : dW[ko,tap,c] += sum_m dY[m,ko] * X[pix(m,tap), c]           M = K, N = C, Kg = N*P*Q (split)
// One K-step = 32 reduction indices = 2 MFMAs per 32x32 tile (16x fewer matrix instructions than fp32 for the same
// FLOPs): the kernels are bound by operand delivery (global -> registers -> LDS), not by the matrix pipe.
//   fprop: [m][k] / [n][k] LDS images of 40 bf16 per row (80-byte rows: one conflict-free ds_read_b128 = the 8 k values a
//          lane feeds to one MFMA), double buffered, one barrier per K-step, the next tile's global loads in flight
//          across it; 3 workgroups per CU cover each other's waits.
//   wgrad: both operands arrive k-major ([pixel][channel]); they are stored row-major in 32-column LDS blocks and read
//          through the hardware transpose ds_read_b64_tr_b16.
// Roofline: MFMA bf16 (2.5 PFLOP/s dense) for the FLOPs, HBM for the fp32 operands: at 256 -> 256 3x3 on 8 x 256 x 256
// the layer moves 1.07 GB for 618.5 GFLOP (ridge at 8 TB/s: 0.13 ms; MFMA at peak: 0.25 ms).
#include "conv_launch.h"
#include <type_traits>
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));

constexpr int BM = 128;
constexpr int BK = 32;
constexpr int LDK = BK + 8;          // [row][k] image row stride in bf16 (80 bytes): conflict-free ds_read_b128

__device__ __forceinline__ u16x4 f2bf4(f32x4 v) { return __builtin_bit_cast(u16x4, __builtin_convertvector(v, bf16x4)); }

__device__ __forceinline__ f32x16 mfma16(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ f32x16 mfma16(f16x8 a, f16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }

// v = parts[0] + parts[1] (+ parts[2]) + O(2^-16 / 2^-24 |v|): each part the round-to-nearest-even bf16 of what is left
// (the subtractions are exact in fp32).  Not for |v| >= 2^127.5 (the hi part rounds to infinity) or non-finite v.
// F16: the parts are fp16 (11 significant bits each: two parts carry 22 bits), v pre-multiplied by the operand's power-of-two
// scale (ConvArgs::amax_*) so that the tensor's largest magnitude sits in [2^14, 2^15) of fp16's range.
template <int SP, bool F16 = false>
__device__ __forceinline__ void split_bf4(f32x4 v, u16x4 (&parts)[SP], float scale = 1.f)
{
    if constexpr (F16) {
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        f32x2 lo2 = {v[0] * scale, v[1] * scale}, hi2 = {v[2] * scale, v[3] * scale};
#pragma unroll
        for (int i = 0; i < SP; ++i) {
            const f16x2 h0 = __builtin_convertvector(lo2, f16x2), h1 = __builtin_convertvector(hi2, f16x2);
            const u32x2 pk = {__builtin_bit_cast(unsigned, h0), __builtin_bit_cast(unsigned, h1)};
            parts[i] = __builtin_bit_cast(u16x4, pk);
            if (i + 1 < SP) {
                lo2 -= __builtin_convertvector(h0, f32x2);
                hi2 -= __builtin_convertvector(h1, f32x2);
            }
        }
        return;
    }
    // pairs: one v_cvt_pk_bf16_f32 rounds two values, shift / mask widen them again (5.5 vector instructions per element for
    // three parts; element-wise conversion, which is what __builtin_convertvector of the 4-vector compiles to, took 7.9)
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    f32x2 lo2 = {v[0], v[1]}, hi2 = {v[2], v[3]};
#pragma unroll
    for (int i = 0; i < SP; ++i) {
        const unsigned p0 = __builtin_bit_cast(unsigned, __builtin_convertvector(lo2, bf16x2));
        const unsigned p1 = __builtin_bit_cast(unsigned, __builtin_convertvector(hi2, bf16x2));
        const u32x2 pk = {p0, p1};
        parts[i] = __builtin_bit_cast(u16x4, pk);
        if (i + 1 < SP) {
            lo2[0] -= __builtin_bit_cast(float, p0 << 16);
            lo2[1] -= __builtin_bit_cast(float, p0 & 0xffff0000u);
            hi2[0] -= __builtin_bit_cast(float, p1 << 16);
            hi2[1] -= __builtin_bit_cast(float, p1 & 0xffff0000u);
        }
    }
}

__device__ __forceinline__ int xcd_remap(int bid, int nb)
{
    const int q = nb >> 3, r = nb & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_srd(const void *p, long bytes)
{   // descriptor inputs through readfirstlane: provably wave-uniform, no waterfall loop (cdna_hip_programming.md T20)
    const unsigned long long u = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    void *q = reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(q, 0, __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
}

struct ConvArgs {
    const float *src;  // X [N,H,W,C]  (or dY for the stride-1 data gradient)
    const float *w;    // [K][R][S][C] fp32
    const unsigned short *w16;   // the same filter already rounded to bf16 (B16 instantiation: read 8 channels per load, no converts)
    float *dst;        // Y [N,P,Q,K]
    const float *bias;
    double *stat_slab; // [mtiles][2][K] per-block column sums / sums of squares, or null
    // BatchNorm-backward sums / masked store of the producer (see csrc/conv.hip ConvArgs): same semantics
    const float *bs_y, *bs_z, *bs_mean, *bs_invstd, *bs_msc, *bs_msh;
    int bs_relu_bias;
    int N, SH, SW, SC, DH, DW, DC;
    int R, S, stride, pad_h, pad_w;
    int relu, accumulate;
    int M, wK, wC;
    int ksplit;
    // strided destination (stride-2 data gradient, one output parity class per launch): logical output pixel (n, h, w) of
    // the DH x DW grid lands at physical pixel (n, h * osh + oh0, w * osw + ow0) of an OH x OW map; osh == 0: dense
    int OH, OW, osh, osw, oh0, ow0;
    // F16 instantiations: bit patterns of max|src| and max|w| (rr_absmax_bits), from which the kernel derives the power-of-two
    // operand scales; null: scale 1
    const unsigned *amax_src, *amax_w;
    // workgroup -> tile map: 1 = every XCD works on ONE column tile (n_tile = xcd % ntiles): the filter rows an XCD re-reads for
    // every row tile (2.4 MB of fp16 hi + lo for 128 of 256 output channels) then stay in its 4 MiB L2; with the column tiles
    // interleaved on every XCD (4.7 MB) they do not, and every re-read goes to the memory side
    int xcd_n;
};

// Operand scale of the split-operand (f16x3) arithmetic from the word holding the bit pattern of max|tensor|: 2^(14 - floor(log2 max)),
// an exact power of two that places the maximum in [2^14, 2^15).  Exponents below 15 (max < 2^-112, zero and denormals included)
// are clamped: (268 - e) << 23 would otherwise reach the Inf / NaN encodings (e <= 13) — such a tensor is scaled by 2^126 at most
// and simply keeps fewer than 22 bits.  The epilogue undoes the two scales one after the other (each factor an exact power of two:
// their PRODUCT overflows / its inverse underflows for tiny operands).
__device__ __forceinline__ float split_scale_from_bits(unsigned bits)
{
    unsigned e = (bits >> 23) & 0xffu;
    e = e < 15u ? 15u : e;
    return __builtin_bit_cast(float, (268u - e) << 23);
}
__device__ __forceinline__ float split_scale_inv(float sc) { return __builtin_bit_cast(float, (254u << 23) - __builtin_bit_cast(unsigned, sc)); }

// 128 x BN output tile, 256 threads = 4 waves (BN 128: 2x2 waves of 64x64; BN 64: 4x1 waves of 32x64; BN 32: 4x1 of 32x32)
// B16: the filter comes as bf16 (a.w16; C % 8 == 0): half the B loads, no converts, 16-byte LDS stores for the B image.
// SO: strided destination (ConvArgs::osh; the stride-2 data gradient's parity-class launches) — its own instantiation: folded
// into the plain kernel the per-element pixel arithmetic cost 20 registers and the third workgroup per CU (585 -> 524 TFLOP/s).
// SP: operand split (csrc header of the split section below).  1: each operand rounded to ONE bf16 value.  2 / 3: each fp32
// operand is written as a sum of 2 / 3 bf16 values (hi + mid [+ lo], each the round-to-nearest of what the previous ones left)
// and the products hi*hi + (hi*mid + mid*hi) [+ hi*lo + mid*mid + lo*hi] are accumulated — 3 / 6 matrix instructions per
// product tile instead of 1, 2^-16 / 2^-24 relative per product.  The small products go to their own accumulator (added to
// the hi*hi one in the epilogue), so their rounding never touches the main sum.
// WS: always false (the wave-specialised 512-thread loop is no longer part of the kernel).
template <int BN, bool BNS, bool B16 = false, bool SO = false, int SP = 1, bool WS = false, bool F16 = false>
__global__ __launch_bounds__(256, SP == 2 ? 2 : 1) void conv_igemm_bf16_kernel(const ConvArgs a)
{
    static_assert(!WS, "conv_igemm_bf16_kernel: WS = false");
    typedef typename std::conditional<F16, f16x8, bf16x8>::type frag_t;
    // operand scales (F16): 2^(14 - floor(log2(max|tensor|))), exact powers of two; the product is undone in the epilogue
    float sc_a = 1.f, sc_b = 1.f, sc_ia = 1.f, sc_ib = 1.f;
    if constexpr (F16) {
        auto scale_of = [](const unsigned *p) {
            if (p == nullptr) return 1.f;
            return split_scale_from_bits(__builtin_amdgcn_readfirstlane(*p));                // 2^(14 - (e - 127))
        };
        sc_a = scale_of(a.amax_src);
        sc_b = scale_of(a.amax_w);
        sc_ia = split_scale_inv(sc_a);
        sc_ib = split_scale_inv(sc_b);
    }
    constexpr int WN = BN / 64 ? BN / 64 : 1;
    constexpr int WM = 4 / WN;
    constexpr int TM = BM / (WM * 32);
    constexpr int TN = BN / (WN * 32);
    constexpr int A_ELEMS = BM * LDK, B_ELEMS = BN * LDK;     // bf16 elements
    constexpr int CPR = BK / 4;                 // float4 columns per row (8)
    constexpr int RPP = 256 / CPR;              // rows per pass of the 256 threads (32)
    constexpr int AJ = BM / RPP;                // 4
    constexpr int BJ = B16 ? (BN / 64 > 0 ? BN / 64 : 1) : (BN / RPP > 0 ? BN / RPP : 1);   // B16: 4 chunks of 8 channels per row, 64 rows per pass

    extern __shared__ __align__(16) unsigned short lds16[];
    unsigned short *As = lds16;                      // [2][SP][A_ELEMS]
    unsigned short *Bs = lds16 + 2 * SP * A_ELEMS;   // [2][SP][B_ELEMS]

    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int ntiles = (a.DC + BN - 1) / BN;
    int n_tile, m_tile;
    if (a.xcd_n) {
        const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3, groups = 8 / ntiles;
        n_tile = xcd % ntiles;
        m_tile = (xcd / ntiles) * ((int)gridDim.x / ntiles / groups) + idx;
    } else {
        const int logical = xcd_remap(blockIdx.x, gridDim.x);
        n_tile = logical % ntiles;
        m_tile = logical / ntiles;
    }
    const int m0 = m_tile * BM, n0 = n_tile * BN;
    const int RS = a.R * a.S;
    const int cpt = (a.SC + BK - 1) / BK;
    const int nk_all = cpt * RS;
    int kc_lo = 0, kc_hi = nk_all;
    if (a.ksplit > 1) {
        const int per = (nk_all + a.ksplit - 1) / a.ksplit;
        kc_lo = blockIdx.z * per;
        kc_hi = kc_lo + per < nk_all ? kc_lo + per : nk_all;
        if (kc_lo >= kc_hi) return;
    }

    // ---- per-thread rows: element offset of the source pixel under tap (0,0) and a bit mask of the taps inside the image
    const int a_col = (t % CPR) * 4, a_row = t / CPR;
    int a_boff[AJ];
    unsigned long long a_mask[AJ];
    const int hw = a.DH * a.DW;
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
        const int m = m0 + a_row + RPP * j;
        int n = 0, h = 0, w = 0;
        const bool live = m < a.M;
        if (live) {
            n = m / hw;
            const int rem = m - n * hw;
            h = rem / a.DW;
            w = rem - h * a.DW;
        }
        const int ih0 = h * a.stride - a.pad_h, iw0 = w * a.stride - a.pad_w;
        unsigned long long mk = 0ull;
        if (live) {
            for (int ri = 0; ri < a.R; ++ri) {
                const int ih = ih0 + ri;
                if (ih < 0 || ih >= a.SH) continue;
                for (int si = 0; si < a.S; ++si) {
                    const int iw = iw0 + si;
                    if (iw >= 0 && iw < a.SW) mk |= 1ull << (ri * a.S + si);
                }
            }
        }
        a_mask[j] = mk;
        a_boff[j] = (int)(((((long)n * a.SH + ih0) * a.SW + iw0) * a.SC + a_col) * 4);
    }
    int b_boff[BJ];
    bool b_ok[BJ];
    const int b_row = B16 ? t / 4 : a_row, b_col = B16 ? (t % 4) * 8 : a_col, b_rpp = B16 ? 64 : RPP;
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
        const int ko = n0 + b_row + b_rpp * j;
        b_ok[j] = ko < a.wK && (b_row + b_rpp * j) < BN;
        b_boff[j] = (int)(((long)ko * RS * a.wC + b_col) * (B16 ? 2 : 4));
    }
    const __amdgpu_buffer_rsrc_t rs_src = make_srd(a.src, (long)a.N * a.SH * a.SW * a.SC * 4);
    const __amdgpu_buffer_rsrc_t rs_w = B16 ? make_srd(a.w16, (long)a.wK * RS * a.wC * 2 * SP) : make_srd(a.w, (long)a.wK * RS * a.wC * 4);
    const int w16_image = a.wK * RS * a.wC * 2;      // B16, SP > 1: the filter's hi / mid / lo images follow each other
    constexpr unsigned OOB = 0xFFFFFFF0u;       // beyond any (< 2 GiB) tensor: the hardware returns 0, no select on the data

    constexpr int NBI = B16 ? SP : 1;            // filter images fetched per K-step
    f32x4 ra[AJ], rb[NBI][BJ];
    // wave-uniform state of the K-step being fetched (tap inner, channel chunk outer: the taps re-read the same lines from L2)
    int p_cch = kc_lo / RS, p_tl = kc_lo - (kc_lo / RS) * RS;
    int p_ri = p_tl / a.S, p_si = p_tl - (p_tl / a.S) * a.S;
    int p_adelta = 0, p_wdelta = 0, p_tlc = 0;
    bool p_cok = false, p_wcok = false, p_live = true;
    auto prep = [&]() {
        const int c0 = p_cch * BK;
        p_tlc = p_tl;
        p_adelta = ((p_ri * a.SW + p_si) * a.SC + c0) * 4;
        p_cok = c0 + a_col < a.SC;                          // (SC == wC: one test serves both operands)
        p_wcok = c0 + b_col < a.wC;
        p_wdelta = (p_tl * a.wC + c0) * (B16 ? 2 : 4);
        ++p_tl;
        if (++p_si == a.S) { p_si = 0; ++p_ri; }
        if (p_tl == RS) { p_tl = 0; p_ri = 0; p_si = 0; ++p_cch; }
    };
    auto load_into = [&](f32x4 (&ra)[AJ], f32x4 (&rb)[NBI][BJ]) {
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            // (timing experiment, round 4: without this tap-mask arithmetic — wrong at the borders — the kernel runs 6 % faster)
            const unsigned ok = (unsigned)p_cok & (unsigned)((a_mask[j] >> p_tlc) & 1ull) & (unsigned)p_live;
            const unsigned off = ok ? (unsigned)(a_boff[j] + p_adelta) : OOB;
            ra[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_src, off, 0, 0));
        }
#pragma unroll
        for (int j = 0; j < BJ; ++j) {
            const unsigned ok = (unsigned)b_ok[j] & (unsigned)p_wcok & (unsigned)p_live;
#pragma unroll
            for (int sp = 0; sp < (B16 ? SP : 1); ++sp) {
                const unsigned off = ok ? (unsigned)(b_boff[j] + p_wdelta + sp * w16_image) : OOB;
                rb[sp][j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, off, 0, 0));   // B16: 8 values of 16 bits
            }
        }
    };
    auto load_all = [&]() { load_into(ra, rb); };
    auto store_from = [&](f32x4 (&ra)[AJ], f32x4 (&rb)[NBI][BJ], int buf) {
        unsigned short *A = As + buf * SP * A_ELEMS, *B = Bs + buf * SP * B_ELEMS;
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            u16x4 parts[SP];
            split_bf4<SP, F16>(ra[j], parts, sc_a);
#pragma unroll
            for (int sp = 0; sp < SP; ++sp)
                *reinterpret_cast<u16x4 *>(A + sp * A_ELEMS + (a_row + RPP * j) * LDK + a_col) = parts[sp];
        }
        if constexpr (B16) {
#pragma unroll
            for (int j = 0; j < BJ; ++j)
                if (BN >= 64 || b_row < BN)
#pragma unroll
                    for (int sp = 0; sp < SP; ++sp)
                        *reinterpret_cast<f32x4 *>(B + sp * B_ELEMS + (b_row + 64 * j) * LDK + b_col) = rb[sp][j];
        } else {
#pragma unroll
            for (int j = 0; j < BJ; ++j) {    // (a_row + RPP * j < BN always: BJ = BN / RPP, a_row < RPP — no guard, no exec-mask branch)
                u16x4 parts[SP];
                split_bf4<SP, F16>(rb[0][j], parts, sc_b);
#pragma unroll
                for (int sp = 0; sp < SP; ++sp)
                    *reinterpret_cast<u16x4 *>(B + sp * B_ELEMS + (a_row + RPP * j) * LDK + a_col) = parts[sp];
            }
        }
    };

    auto store_all = [&](int buf) { store_from(ra, rb, buf); };

    f32x16 acc[TM][TN], acl[SP > 1 ? TM : 1][SP > 1 ? TN : 1];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                acc[i][j][e] = 0.f;
                if constexpr (SP > 1) acl[i][j][e] = 0.f;
            }
    const int lr = lane & 31, lh = lane >> 5;

    if (kc_lo < kc_hi) {
        prep();
        load_all();
        store_all(0);
        p_live = kc_lo + 1 < kc_hi;
        prep();
        load_all();                         // tile kc_lo + 1 stays in registers until the first iteration stores it
    }
    __syncthreads();
    for (int kc = kc_lo; kc < kc_hi; ++kc) {
        const int buf = (kc - kc_lo) & 1;
        const unsigned short *A = As + buf * SP * A_ELEMS, *B = Bs + buf * SP * B_ELEMS;
        // SP == 1: the fragments of both 16-wide halves up front (as tuned).  SP > 1: one half at a time — half the fragment
        // registers, which keeps the split kernel within 256 registers (two workgroups per CU)
        constexpr int NKK = SP > 1 ? 1 : 2;
        frag_t fa[NKK][SP][TM], fb[NKK][SP][TN];
        auto frags = [&](int slot, int kk) {
#pragma unroll
            for (int sp = 0; sp < SP; ++sp) {
#pragma unroll
                for (int i = 0; i < TM; ++i)
                    fa[slot][sp][i] = *reinterpret_cast<const frag_t *>(A + sp * A_ELEMS + ((wm * TM + i) * 32 + lr) * LDK + kk * 16 + lh * 8);
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    fb[slot][sp][j] = *reinterpret_cast<const frag_t *>(B + sp * B_ELEMS + ((wn * TN + j) * 32 + lr) * LDK + kk * 16 + lh * 8);
            }
        };
        auto mma = [&](int slot) {
            // (product outermost, tiles inner: consecutive matrix instructions never share an accumulator)
#define RR_MM(ACC, PA, PB)                                                                                          \
    _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j)                      \
        ACC[i][j] = mfma16(fa[slot][PA][i], fb[slot][PB][j], ACC[i][j]);
            if constexpr (SP == 3) { RR_MM(acl, 0, 2) RR_MM(acl, 2, 0) RR_MM(acl, 1, 1) }
            if constexpr (SP >= 2) { RR_MM(acl, 0, 1) RR_MM(acl, 1, 0) }
            RR_MM(acc, 0, 0)
#undef RR_MM
        };
        frags(0, 0);
        if constexpr (SP == 1) frags(1, 1);
        // tile kc + 1 (loaded one iteration ago) -> the other LDS buffer, whose last readers passed the previous barrier;
        // then tile kc + 2 goes out.  (Staging BEHIND the matrix instructions instead — a whole iteration for the loads to
        // land — measured the same: the loop is bound by instruction issue, ~96 non-MFMA instructions per 8 MFMAs.)
        store_all(buf ^ 1);
        p_live = kc + 2 < kc_hi;
        prep();
        load_all();
        mma(0);
        if constexpr (SP == 1) {
            mma(1);
        } else {
            frags(0, 1);
            mma(0);
        }
        __syncthreads();
    }
    if constexpr (SP > 1) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                acc[i][j] += acl[i][j];
                if constexpr (F16) acc[i][j] = acc[i][j] * sc_ia * sc_ib;
            }
    }

    // ---- epilogue (as csrc/conv.hip).  D layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    double *sred = reinterpret_cast<double *>(lds16);   // [WM][BN][2], reuses the staging LDS
    const bool do_stats = a.stat_slab != nullptr && a.ksplit <= 1;
    const __amdgpu_buffer_rsrc_t bs_rs_y = make_srd(BNS ? a.bs_y : a.src, (long)a.M * a.DC * 4);
    const __amdgpu_buffer_rsrc_t bs_rs_z = make_srd(BNS && a.bs_z != nullptr ? a.bs_z : a.src, (long)a.M * a.DC * 4);
    const int mode_e = a.ksplit > 1 ? 2 : (a.accumulate ? 1 : 0);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int ncol = n0 + (wn * TN + j) * 32 + lr;
        const bool n_ok = ncol < a.DC;
        const float bv = (a.bias != nullptr && n_ok) ? a.bias[ncol] : 0.f;
        float s1 = 0.f, s2 = 0.f;
        float bs_m = 0.f, bs_i = 0.f, bs_sc = 0.f, bs_sh = 0.f;
        if constexpr (BNS) {
            if (n_ok && !a.bs_relu_bias) {
                bs_m = a.bs_mean[ncol]; bs_i = a.bs_invstd[ncol];
                if (a.bs_z == nullptr) {
                    if (a.bs_msc != nullptr) { bs_sc = a.bs_msc[ncol]; bs_sh = a.bs_msh[ncol]; }
                    else bs_sh = 1.f;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            if constexpr (BNS) {
                const bool use_z = a.bs_z != nullptr;
                const unsigned voff = n_ok ? (unsigned)(((m0 + (wm * TM + i) * 32 + 4 * lh) * a.DC + ncol) * 4) : 0xFFFFFFF0u;
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    float yv[8], zv[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int e = hh * 8 + q;
                        const int soff = __builtin_amdgcn_readfirstlane(((e & 3) + 8 * (e >> 2)) * a.DC * 4);
                        yv[q] = a.bs_relu_bias ? 0.f : __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(bs_rs_y, voff, soff, 0));
                        zv[q] = use_z ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(bs_rs_z, voff, soff, 0)) : 0.f;
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int e = hh * 8 + q;
                        const int m = m0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                        if (m < a.M && n_ok) {
                            float *p = a.dst + (long)m * a.DC + ncol;
                            float v = acc[i][j][e];
                            if (mode_e == 1) v += *p;
                            const bool on = use_z ? zv[q] > 0.f : rr_bn_affine(yv[q], bs_sc, bs_sh) > 0.f;
                            const float d = on ? v : 0.f;
                            *p = a.bs_relu_bias ? d : v;
                            s1 += d;
                            s2 += d * ((yv[q] - bs_m) * bs_i);
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
                continue;
            }
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                float v = acc[i][j][e] + bv;
                if (a.relu) v = v > 0.f ? v : 0.f;
                if (m < a.M && n_ok) {
                    long pix = m;
                    if constexpr (SO) {
                        const int n = m / hw, rem = m - n * hw;
                        const int h = rem / a.DW;
                        pix = ((long)n * a.OH + (h * a.osh + a.oh0)) * a.OW + ((rem - h * a.DW) * a.osw + a.ow0);
                    }
                    float *p = a.dst + pix * a.DC + ncol;
                    if (mode_e == 2) {
                        unsafeAtomicAdd(p, v);
                    } else {
                        if (mode_e == 1) v += *p;
                        *p = v;
                        s1 += v;
                        s2 += v * v;
                    }
                }
            }
        }
        if (do_stats) {
            double d1 = (double)s1, d2 = (double)s2;
            d1 += __shfl_xor(d1, 32, 64);
            d2 += __shfl_xor(d2, 32, 64);
            if (lh == 0) {
                const int cl = (wn * TN + j) * 32 + lr;
                sred[(wm * BN + cl) * 2 + 0] = d1;
                sred[(wm * BN + cl) * 2 + 1] = d2;
            }
        }
    }
    if (do_stats) {
        __syncthreads();
        if (t < BN && n0 + t < a.DC) {
            double d1 = 0.0, d2 = 0.0;
#pragma unroll
            for (int w = 0; w < WM; ++w) {
                d1 += sred[(w * BN + t) * 2 + 0];
                d2 += sred[(w * BN + t) * 2 + 1];
            }
            double *slab = a.stat_slab + (long)m_tile * 2 * a.DC;
            slab[n0 + t] = d1;
            slab[a.DC + n0 + t] = d2;
        }
    }
}

struct OutMap { int DH, DW, OH, OW, osh, osw, oh0, ow0; };   // explicit logical output grid + strided destination

// filter [K][R][S][C] fp32 -> its two fp16 parts, scaled by the power of two the convolution kernel derives from the same word:
// image 0 = hi, image 1 = lo (each K*R*S*C halves).  A 2.4 MB filter: ~5 us, against 48 of the 149 vector instructions per
// K-step and thread that splitting the filter tile inside the convolution costs.
__global__ __launch_bounds__(256) void weight_split_f16_kernel(const f32x4 *w, const unsigned *amax, unsigned short *out, long n4)
{
    const float scale = split_scale_from_bits(*amax);
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        u16x4 parts[2];
        split_bf4<2, true>(w[i], parts, scale);
        *reinterpret_cast<u16x4 *>(out + 4 * i) = parts[0];
        *reinterpret_cast<u16x4 *>(out + 4 * (n4 + i)) = parts[1];
    }
}

size_t igemm_lds(int bn, int sp = 1) { return sizeof(unsigned short) * 2 * (size_t)sp * (BM + bn) * LDK; }

// The arithmetic of a call.  split 0: bf16, filter16 = the filter already rounded to bf16, or null.  split 1: f16x3, the two
// operands' maxima, filter16 = the filter's two fp16 images (rr_weight_split_f16), or null.
struct Math16 {
    int split;
    const unsigned short *filter16;
    const unsigned *amax_src, *amax_w;
};

// name: the public entry point that was called.  How the call launches is rr_plan::fprop_plan's decision (conv_plan.h).
int fprop_impl(const char *name, const Math16 &mt, const float *x, const float *w, const float *bias, float *y, double *stat_slab, int n, int h,
               int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w, int relu, int accumulate, hipStream_t stream,
               const BnSumArgs *bs = nullptr, const OutMap *om = nullptr)
{
    RR_CHECK_ARG(!mt.split || (mt.amax_src && mt.amax_w), "%s: the operands' maxima are required", name);
    const rr_plan::FpropPlan pl = rr_plan::fprop_plan(mt.split ? rr_plan::MATH_F16X3 : rr_plan::MATH_BF16,
                                                      {n, h, wd, c, k, r, s, stride, pad_h, pad_w, om ? om->DH : 0, om ? om->DW : 0},
                                                      {bias != nullptr, relu != 0, stat_slab != nullptr, rr_conv_link(bs), accumulate != 0, om != nullptr});
    RR_CHECK_ARG(pl.refuse == nullptr, "%s: %s", name, pl.refuse);
    ConvArgs a{};
    a.src = x; a.w = w; a.dst = y; a.bias = bias; a.stat_slab = stat_slab;
    a.w16 = (!mt.split && mt.filter16 != nullptr && c % 8 == 0) ? mt.filter16 : nullptr;       // 16-byte loads of 8 channels
    RR_CHECK_ARG(w != nullptr || a.w16 != nullptr, "%s: no filter", name);
    a.N = n; a.SH = h; a.SW = wd; a.SC = c;
    a.DH = pl.dh; a.DW = pl.dw; a.DC = k;
    if (om != nullptr) {        // pads are LEADING pads; taps past the far edge are masked by the gather
        a.OH = om->OH; a.OW = om->OW; a.osh = om->osh; a.osw = om->osw; a.oh0 = om->oh0; a.ow0 = om->ow0;
    }
    a.R = r; a.S = s; a.stride = stride; a.pad_h = pad_h; a.pad_w = pad_w;
    a.relu = relu; a.accumulate = accumulate; a.ksplit = pl.ks; a.xcd_n = pl.xcd_n;
    a.M = (int)pl.M; a.wK = k; a.wC = c;
    const int bn = pl.bn, blocks = pl.blocks, ks = pl.ks;
    const bool fused = pl.fused;
    if (fused) bs->into(a);
    if (int rc = rr_conv_before_launch(pl, n, k, y, stat_slab, stream, name)) return rc;
    int rc;
#define RR_IG(BNv, BNSv, SOv)                                                                                      \
    (a.w16 ? rr_launch(conv_igemm_bf16_kernel<BNv, BNSv, true, SOv>, dim3(blocks, 1, ks), 256, igemm_lds(BNv), stream, a, name)           \
           : rr_launch(conv_igemm_bf16_kernel<BNv, BNSv, false, SOv>, dim3(blocks, 1, ks), 256, igemm_lds(BNv), stream, a, name))
    // split operands (rr_conv_*_f16x3): two fp16 parts per operand, three matrix instructions per product tile
#define RR_SX(BNv, BNSv, SOv) rr_launch(conv_igemm_bf16_kernel<BNv, BNSv, false, SOv, 2, false, true>, dim3(blocks, 1, ks), 256, igemm_lds(BNv, 2), stream, a, name)
    // the instance of launcher L for (fused sums | strided destination | plain) x tile width
#define RR_PICK(L) (fused ? RR_PICK_BN(L, true, false) : a.osh ? RR_PICK_BN(L, false, true) : RR_PICK_BN(L, false, false))
#define RR_PICK_BN(L, BNSv, SOv) (bn == 128 ? L(128, BNSv, SOv) : bn == 64 ? L(64, BNSv, SOv) : L(32, BNSv, SOv))
    if (mt.split) {
        // (A wave-specialised 512-thread form of this kernel — round 4 — measured 2.84 ms against 2.27 ms for two 256-thread
        // workgroups per CU at 256 -> 256 3x3 on 8 x 256 x 256: a SIMD does not overlap one wave's matrix instructions with another
        // wave's vector instructions (tools/coissue_probe.hip).  Its launch arm was removed in round 6.)
        a.amax_src = mt.amax_src; a.amax_w = mt.amax_w;
        if (mt.filter16 != nullptr && c % 8 == 0 && bn == 128) {
            // the filter's two fp16 images, made by rr_weight_split_f16 (once per optimizer step, outside the backward pass): the B16 instantiation
            a.w16 = mt.filter16;
#define RR_SB(BNSv, SOv) rr_launch(conv_igemm_bf16_kernel<128, BNSv, true, SOv, 2, false, true>, dim3(blocks, 1, ks), 256, igemm_lds(128, 2), stream, a, name)
            rc = fused ? RR_SB(true, false) : (a.osh ? RR_SB(false, true) : RR_SB(false, false));
#undef RR_SB
        } else
            rc = RR_PICK(RR_SX);
    } else
        rc = RR_PICK(RR_IG);
#undef RR_IG
#undef RR_SX
#undef RR_PICK
#undef RR_PICK_BN
    return rc == RR_OK ? rr_conv_after_launch(pl, bs, k, y, stat_slab, stream, name) : rc;
}

// ---------------------------------------------------------------------------------------------
// wgrad: dW[ko][tap][c] += sum over a slice of the N*P*Q pixels of dY[m][ko] * X[pix(m,tap)][c].  GEMM M = K (ko), N = C,
// reduction over pixels.  Both operands are k-major in memory ([pixel][channel]): each is stored row-major into LDS as
// 32-column blocks [block][32 pixels][32 channels] (64-byte rows) and read through ds_read_b64_tr_b16, which hands every
// lane the 8 consecutive pixels of its channel (checked lane by lane on the device: tools/tr_probe.hip).
struct WgradArgs {
    const float *x, *dy;
    float *dw;
    int N, H, W, C, K, R, S, P, Q, stride, pad_h, pad_w;
    int M, chunks_per_split, mt, nt;
    const unsigned *amax_x, *amax_dy;       // split instantiation: bit patterns of max|x|, max|dy| (rr_absmax_bits)
};

template <typename F = bf16x8>
__device__ __forceinline__ F lds_tr_frag(const unsigned short *img, int k0, int lane)
{
    const int g = lane >> 4, i = lane & 15, q = i >> 2, p = i & 3;
    const unsigned short *a = img + (k0 + 8 * (g >> 1) + q) * 32 + 16 * (g & 1) + 4 * p;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)a);
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4 *)(a + 4 * 32));
    union { s16x4 h[2]; F v; } u;
    u.h[0] = lo; u.h[1] = hi;
    return u.v;
}

// 128 (ko) x 128 (c) tile per workgroup and tap; 2x2 waves of 64x64.  K-step = 32 pixels.
// SP = 2, F16: both operands split into two fp16 parts (see conv_igemm_bf16_kernel), three matrix instructions per tile.
template <int SP = 1, bool F16 = false>
__global__ __launch_bounds__(256, SP > 1 ? 2 : 1) void conv_wgrad_bf16_kernel(const WgradArgs a)
{
    typedef typename std::conditional<F16, f16x8, bf16x8>::type frag_t;
    float sc_a = 1.f, sc_b = 1.f, sc_ia = 1.f, sc_ib = 1.f;
    if constexpr (F16) {
        auto scale_of = [](const unsigned *p) {
            if (p == nullptr) return 1.f;
            return split_scale_from_bits(__builtin_amdgcn_readfirstlane(*p));
        };
        sc_a = scale_of(a.amax_dy);
        sc_b = scale_of(a.amax_x);
        sc_ia = split_scale_inv(sc_a);
        sc_ib = split_scale_inv(sc_b);
    }
    constexpr int BLK = 32 * 32 + 32;            // one 32-column block of a K-step: [32 pixels][32 channels] (+64 B: the 8-byte
                                                 // stores of a 16-lane group go to two blocks, on disjoint banks)
    constexpr int IMG = 4 * BLK;                 // 128 channels
    extern __shared__ __align__(16) unsigned short lds16[];
    unsigned short *As = lds16;                  // [2][SP][IMG]  dY  (ko)
    unsigned short *Bs = lds16 + 2 * SP * IMG;   // [2][SP][IMG]  X   (c)

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int RS = a.R * a.S;
    int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int tap = logical % RS; logical /= RS;
    const int n_tile = logical % a.nt; logical /= a.nt;
    const int m_tile = logical % a.mt;
    const int split = logical / a.mt;
    const int r = tap / a.S, s = tap - r * a.S;
    const int ko0 = m_tile * 128, c0 = n_tile * 128;
    const int total_chunks = (a.M + BK - 1) / BK;
    const int kc_begin = split * a.chunks_per_split;
    int kc_end = kc_begin + a.chunks_per_split;
    if (kc_end > total_chunks) kc_end = total_chunks;
    if (kc_begin >= kc_end) return;

    // staging: thread = (pixel row t / 32 + 8 j, channel quad t % 32)
    const int s_col = (t & 31) * 4, s_row = t >> 5;
    const bool a_ok = ko0 + s_col < a.K, b_ok = c0 + s_col < a.C;
    const __amdgpu_buffer_rsrc_t rs_dy = make_srd(a.dy, (long)a.M * a.K * 4);
    const __amdgpu_buffer_rsrc_t rs_x = make_srd(a.x, (long)a.N * a.H * a.W * a.C * 4);
    constexpr unsigned OOB = 0xFFFFFFF0u;
    // running (n, p, q) of this thread's four pixel rows
    int bn_[4], bp_[4], bq_[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long m = (long)kc_begin * BK + s_row + 8 * j;
        const int pq = a.P * a.Q;
        bn_[j] = (int)(m / pq);
        const int rem = (int)(m - (long)bn_[j] * pq);
        bp_[j] = rem / a.Q;
        bq_[j] = rem - bp_[j] * a.Q;
    }
    f32x4 ra[4], rb[4];
    auto load_all = [&](int kc) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long m = (long)kc * BK + s_row + 8 * j;
            const unsigned ok = (unsigned)a_ok & (unsigned)(m < a.M) & (unsigned)(kc < kc_end);
            const unsigned off = ok ? (unsigned)((m * a.K + ko0 + s_col) * 4) : OOB;
            ra[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_dy, off, 0, 0));
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ih = bp_[j] * a.stride - a.pad_h + r, iw = bq_[j] * a.stride - a.pad_w + s;
            const unsigned ok = (unsigned)b_ok & (unsigned)(bn_[j] < a.N) & (unsigned)((unsigned)ih < (unsigned)a.H) &
                                (unsigned)((unsigned)iw < (unsigned)a.W) & (unsigned)(kc < kc_end);
            const unsigned off = ok ? (unsigned)((((bn_[j] * a.H + ih) * a.W + iw) * a.C + c0 + s_col) * 4) : OOB;
            rb[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, off, 0, 0));
            bq_[j] += BK;
            while (bq_[j] >= a.Q) {
                bq_[j] -= a.Q;
                if (++bp_[j] == a.P) { bp_[j] = 0; ++bn_[j]; }
            }
        }
    };
    auto store_all = [&](int buf) {
        unsigned short *A = As + buf * SP * IMG, *B = Bs + buf * SP * IMG;
        const int blk = (s_col >> 5) * BLK, cc = s_col & 31;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            u16x4 pa[SP], pb[SP];
            split_bf4<SP, F16>(ra[j], pa, sc_a);
            split_bf4<SP, F16>(rb[j], pb, sc_b);
#pragma unroll
            for (int sp = 0; sp < SP; ++sp) {
                *reinterpret_cast<u16x4 *>(A + sp * IMG + blk + (s_row + 8 * j) * 32 + cc) = pa[sp];
                *reinterpret_cast<u16x4 *>(B + sp * IMG + blk + (s_row + 8 * j) * 32 + cc) = pb[sp];
            }
        }
    };

    f32x16 acc[2][2], acl[SP > 1 ? 2 : 1][SP > 1 ? 2 : 1];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                acc[i][j][e] = 0.f;
                if constexpr (SP > 1) acl[i][j][e] = 0.f;
            }

    load_all(kc_begin);
    store_all(0);
    load_all(kc_begin + 1);
    __syncthreads();
    for (int kc = kc_begin; kc < kc_end; ++kc) {
        const int buf = (kc - kc_begin) & 1;
        const unsigned short *A = As + buf * SP * IMG, *B = Bs + buf * SP * IMG;
        // fragments of one 16-pixel half at a time (SP > 1: 32 registers instead of 64 — the split kernel must stay within 256
        // registers for its second workgroup per CU)
        frag_t fa[SP][2], fb[SP][2];
        auto frags = [&](int kk) {
#pragma unroll
            for (int sp = 0; sp < SP; ++sp) {
#pragma unroll
                for (int i = 0; i < 2; ++i) fa[sp][i] = lds_tr_frag<frag_t>(A + sp * IMG + (wm * 2 + i) * BLK, kk * 16, lane);
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[sp][j] = lds_tr_frag<frag_t>(B + sp * IMG + (wn * 2 + j) * BLK, kk * 16, lane);
            }
        };
        auto mma = [&]() {
#define RR_MM(ACC, PA, PB)                                                                                          \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) _Pragma("unroll") for (int j = 0; j < 2; ++j)                        \
        ACC[i][j] = mfma16(fa[PA][i], fb[PB][j], ACC[i][j]);
            RR_MM(acc, 0, 0)
            if constexpr (SP >= 2) { RR_MM(acl, 0, 1) RR_MM(acl, 1, 0) }
            if constexpr (SP == 3) { RR_MM(acl, 1, 1) RR_MM(acl, 0, 2) RR_MM(acl, 2, 0) }
#undef RR_MM
        };
        if constexpr (SP == 1) {
            frag_t ga[2], gb[2];       // (one part: both halves up front, as the kernel was tuned)
#pragma unroll
            for (int i = 0; i < 2; ++i) ga[i] = lds_tr_frag<frag_t>(A + (wm * 2 + i) * BLK, 16, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) gb[j] = lds_tr_frag<frag_t>(B + (wn * 2 + j) * BLK, 16, lane);
            frags(0);
            store_all(buf ^ 1);
            load_all(kc + 2);
            mma();
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(ga[i], gb[j], acc[i][j]);
        } else {
            frags(0);
            store_all(buf ^ 1);
            load_all(kc + 2);
            mma();
            frags(1);
            mma();
        }
        __syncthreads();
    }
    if constexpr (SP > 1) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                acc[i][j] += acl[i][j];
                if constexpr (F16) acc[i][j] = acc[i][j] * sc_ia * sc_ib;
            }
    }
    const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = c0 + (wn * 2 + j) * 32 + lr;
        if (c >= a.C) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ko = ko0 + (wm * 2 + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (ko < a.K) unsafeAtomicAdd(a.dw + ((long)ko * RS + tap) * a.C + c, acc[i][j][e]);
            }
    }
}

__global__ __launch_bounds__(256) void absmax_bits_kernel(const f32x4 *x, long n4, unsigned *out)
{
    float m = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const f32x4 v = x[i];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v[0]), fabsf(v[1]))), fmaxf(fabsf(v[2]), fabsf(v[3])));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    // non-negative floats order as their bit patterns; look before the same-address atomic (see bn_apply_kernel)
    if ((threadIdx.x & 63) == 0 && __builtin_bit_cast(unsigned, m) > *(volatile unsigned *)out) atomicMax(out, __builtin_bit_cast(unsigned, m));
}

}  // namespace

extern "C" int rr_absmax_bits(const float *x, long n, unsigned *out, hipStream_t stream)
{
    RR_CHECK_ARG(n % 4 == 0, "rr_absmax_bits: n must be a multiple of 4");
    if (n == 0) return RR_OK;
    long blocks = (n / 4 + 256 * 8 - 1) / (256 * 8);       // >= 8 float4 per thread; a filter takes a few workgroups, not 1024
    if (blocks > 1024) blocks = 1024;
    hipLaunchKernelGGL(absmax_bits_kernel, dim3((int)blocks), dim3(256), 0, stream, reinterpret_cast<const f32x4 *>(x), n / 4, out);
    RR_CHECK_LAUNCH("rr_absmax_bits");
    return RR_OK;
}

extern "C" int rr_conv_fprop_bf16(const float *x, const float *w, const float *bias, float *y, double *stat_slab,
                                  int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h,
                                  int pad_w, int relu, const unsigned short *w_bf16, hipStream_t stream)
{
    return fprop_impl("rr_conv_fprop_bf16", {0, w_bf16}, x, w, bias, y, stat_slab, n, h, wd, c, k, r, s, stride, pad_h, pad_w, relu, 0, stream);
}

// the stride-1 data gradients: rr_dgrad_s1_geom's checks and flip (conv_launch.h), then the forward kernel on (dy, wt)
static int dgrad_s1(const char *name, const Math16 &mt, bool producer_ok, const float *dy, const float *wt, float *dx, int n, int h, int wd,
                    int c, int k, int r, int s, int pad_h, int pad_w, int accumulate, hipStream_t stream, const BnSumArgs *bs = nullptr)
{
    DgradS1Geom g;
    if (int rc = rr_dgrad_s1_geom(name, h, wd, r, s, pad_h, pad_w, producer_ok, &g)) return rc;
    return fprop_impl(name, mt, dy, wt, nullptr, dx, nullptr, n, g.p, g.q, k, c, r, s, 1, g.pad_h, g.pad_w, 0, accumulate, stream, bs);
}

extern "C" int rr_conv_dgrad_s1_bf16(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                                     int r, int s, int pad_h, int pad_w, int accumulate, const unsigned short *wt_bf16,
                                     hipStream_t stream)
{
    return dgrad_s1("rr_conv_dgrad_s1_bf16", {0, wt_bf16}, true, dy, wt, dx, n, h, wd, c, k, r, s, pad_h, pad_w, accumulate, stream);
}

extern "C" int rr_conv_dgrad_s1_bnsum_bf16(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                                           int r, int s, int pad_h, int pad_w, int accumulate, const float *prod_y,
                                           const float *prod_z, const float *prod_mean, const float *prod_invstd,
                                           const float *prod_mask_scale, const float *prod_mask_shift, double *slab,
                                           double *sums, const unsigned short *wt_bf16, hipStream_t stream)
{
    const BnSumArgs bs{prod_y, prod_z, prod_mean, prod_invstd, prod_mask_scale, prod_mask_shift, slab, sums, 0};
    return dgrad_s1("rr_conv_dgrad_s1_bnsum_bf16", {0, wt_bf16}, bs.bn_ok(c), dy, wt, dx, n, h, wd, c, k, r, s, pad_h, pad_w, accumulate,
                    stream, &bs);
}

extern "C" int rr_conv_dgrad_s1_relubias_bf16(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                                              int r, int s, int pad_h, int pad_w, int accumulate, const float *prod_z,
                                              double *slab, double *sums, hipStream_t stream)
{
    const BnSumArgs bs{prod_z, prod_z, nullptr, nullptr, nullptr, nullptr, slab, sums, 1};
    return dgrad_s1("rr_conv_dgrad_s1_relubias_bf16", {0, nullptr}, bs.relu_bias_ok(c, k), dy, wt, dx, n, h, wd, c, k, r, s, pad_h, pad_w,
                    accumulate, stream, &bs);
}

// Stride-2 data gradient on the forward kernel: dx[n, 2a+ph, 2b+pw, c] = sum over the taps r = r0 + 2i, s = s0 + 2j that
// reach output parity class (ph, pw) (r0 = (ph + pad_h) & 1) of dY[n, a + (ph+pad_h-r0)/2 - i, ..., k] * w[k][r][s][c] — per
// class a stride-1 correlation of dY with a sub-filter of ceil / floor (R/2) x (S/2) taps, written to every second pixel
// (rr_plan::parity_classes).  The four sub-filters are packed into caller scratch of k*r*s*c floats by one kernel
// (rr_parity_pack); a 3x3 visits 1 / 2 / 2 / 4 taps instead of masking three quarters of a dilated filter.
static int dgrad_s2_impl(const char *name, const Math16 &mt, const float *dy, const float *w, float *dx, int n, int h, int wd, int c, int k,
                         int r, int s, int pad_h, int pad_w, int accumulate, float *wsub, hipStream_t stream)
{
    const rr_plan::ConvGeom g{n, h, wd, c, k, r, s, 2, pad_h, pad_w, 0, 0};
    const rr_plan::DgradS2Plan pl = rr_plan::dgrad_s2_plan(mt.split ? rr_plan::MATH_F16X3 : rr_plan::MATH_BF16, g, accumulate != 0,
                                                           wsub != nullptr && (!mt.split || (mt.amax_src && mt.amax_w)));
    if (pl.refuse.why) return rr_refuse(name, pl.refuse);
    return rr_dgrad_s2_run(pl, g, w, wsub, dx, stream, name, [&](const rr_plan::ParityClass &pc) {
        const OutMap om{pc.Hc, pc.Wc, h, wd, 2, 2, pc.ph, pc.pw};
        return fprop_impl(name, mt, dy, wsub + (long)pc.taps_before * c * k, nullptr, dx, nullptr, n, pl.p, pl.q, k, c, pc.Rc, pc.Sc, 1, pc.lead_h,
                          pc.lead_w, 0, accumulate, stream, nullptr, &om);
    });
}

extern "C" int rr_conv_dgrad_s2_bf16(const float *dy, const float *w, float *dx, int n, int h, int wd, int c, int k,
                                     int r, int s, int pad_h, int pad_w, int accumulate, float *wsub, hipStream_t stream)
{
    return dgrad_s2_impl("rr_conv_dgrad_s2_bf16", {0, nullptr}, dy, w, dx, n, h, wd, c, k, r, s, pad_h, pad_w, accumulate, wsub, stream);
}

// How it launches is rr_plan::wgrad_plan's decision (conv_plan.h); both arithmetics refuse under rr_conv_wgrad_bf16's name.
static int wgrad_impl(const float *x, const float *dy, float *dw, int n, int h, int wd, int c, int k, int r, int s, int stride,
                      int pad_h, int pad_w, int out_h, int out_w, hipStream_t stream, int split, const unsigned *amax_x,
                      const unsigned *amax_dy)
{
    const rr_plan::WgradPlan pl = rr_plan::wgrad_plan(split ? rr_plan::MATH_F16X3 : rr_plan::MATH_BF16,
                                                      {n, h, wd, c, k, r, s, stride, pad_h, pad_w, out_h, out_w});
    if (pl.refuse.why) return rr_refuse("rr_conv_wgrad_bf16", pl.refuse);
    WgradArgs a{};
    a.x = x; a.dy = dy; a.dw = dw;
    a.amax_x = amax_x; a.amax_dy = amax_dy;
    a.N = n; a.H = h; a.W = wd; a.C = c; a.K = k; a.R = r; a.S = s;
    a.P = pl.P; a.Q = pl.Q;
    a.stride = stride; a.pad_h = pad_h; a.pad_w = pad_w;
    a.M = (int)pl.M; a.mt = pl.mt; a.nt = pl.nt; a.chunks_per_split = pl.per_split;
    return split ? rr_launch(conv_wgrad_bf16_kernel<2, true>, dim3(pl.grid), 256, pl.lds, stream, a, "rr_conv_wgrad_f16x3")
                 : rr_launch(conv_wgrad_bf16_kernel<1, false>, dim3(pl.grid), 256, pl.lds, stream, a, "rr_conv_wgrad_bf16");
}

extern "C" int rr_conv_wgrad_bf16(const float *x, const float *dy, float *dw, int n, int h, int wd, int c, int k,
                                  int r, int s, int stride, int pad_h, int pad_w, int out_h, int out_w, hipStream_t stream)
{
    return wgrad_impl(x, dy, dw, n, h, wd, c, k, r, s, stride, pad_h, pad_w, out_h, out_w, stream, 0, nullptr, nullptr);
}

// ---------------------------------------------------------------------------------------------
// Split-operand entry points ("f16x3"): the same convolutions with each fp32 operand written as hi + lo, two fp16 values
// (22 significant bits), after a power-of-two scaling that puts the tensor's largest magnitude into [2^14, 2^15), and
// hi*hi + hi*lo + lo*hi accumulated in fp32 on v_mfma_f32_32x32x16_f16 — three matrix instructions at the 16-bit rate
// instead of eight v_mfma_f32_32x32x2_f32 for the same 32 x 32 x 16 block (the fp32 matrix rate of gfx950 is 1/16 of the
// 16-bit one).  amax_*: device words holding the bit pattern of max|tensor| (rr_absmax_bits), read by the kernels, no host
// synchronisation.  Error against an fp64 convolution: below the fp32-MFMA kernels' own (tests/test_conv_split_gpu.py).
extern "C" int rr_weight_split_f16(const float *w, long n, const unsigned *amax_w, unsigned short *out, hipStream_t stream)
{
    RR_CHECK_ARG(w && amax_w && out && n > 0 && n % 4 == 0, "rr_weight_split_f16: n must be a positive multiple of 4, pointers non-null");
    const long n4 = n / 4;
    long sb = (n4 + 255) / 256;
    if (sb > 1024) sb = 1024;
    hipLaunchKernelGGL(weight_split_f16_kernel, dim3((int)sb), dim3(256), 0, stream, reinterpret_cast<const f32x4 *>(w), amax_w, out, n4);
    RR_CHECK_LAUNCH("rr_weight_split_f16");
    return RR_OK;
}

extern "C" int rr_conv_fprop_f16x3(const float *x, const float *w, const float *bias, float *y, double *stat_slab,
                                   int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h,
                                   int pad_w, int relu, const unsigned *amax_x, const unsigned *amax_w,
                                   const unsigned short *w_split, hipStream_t stream)
{
    return fprop_impl("rr_conv_fprop_f16x3", {1, w_split, amax_x, amax_w}, x, w, bias, y, stat_slab, n, h, wd, c, k, r, s, stride, pad_h, pad_w,
                      relu, 0, stream);
}

extern "C" int rr_conv_dgrad_s1_f16x3(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                                      int r, int s, int pad_h, int pad_w, int accumulate, const unsigned *amax_dy,
                                      const unsigned *amax_w, const unsigned short *wt_split, hipStream_t stream)
{
    return dgrad_s1("rr_conv_dgrad_s1_f16x3", {1, wt_split, amax_dy, amax_w}, true, dy, wt, dx, n, h, wd, c, k, r, s, pad_h, pad_w, accumulate, stream);
}

extern "C" int rr_conv_dgrad_s1_bnsum_f16x3(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                                            int r, int s, int pad_h, int pad_w, int accumulate, const float *prod_y,
                                            const float *prod_z, const float *prod_mean, const float *prod_invstd,
                                            const float *prod_mask_scale, const float *prod_mask_shift, double *slab,
                                            double *sums, const unsigned *amax_dy, const unsigned *amax_w,
                                            const unsigned short *wt_split, hipStream_t stream)
{
    const BnSumArgs bs{prod_y, prod_z, prod_mean, prod_invstd, prod_mask_scale, prod_mask_shift, slab, sums, 0};
    return dgrad_s1("rr_conv_dgrad_s1_bnsum_f16x3", {1, wt_split, amax_dy, amax_w}, bs.bn_ok(c), dy, wt, dx, n, h, wd, c, k, r, s, pad_h, pad_w,
                    accumulate, stream, &bs);
}

extern "C" int rr_conv_dgrad_s1_relubias_f16x3(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                                               int r, int s, int pad_h, int pad_w, int accumulate, const float *prod_z,
                                               double *slab, double *sums, const unsigned *amax_dy, const unsigned *amax_w,
                                               hipStream_t stream)
{
    const BnSumArgs bs{prod_z, prod_z, nullptr, nullptr, nullptr, nullptr, slab, sums, 1};
    return dgrad_s1("rr_conv_dgrad_s1_relubias_f16x3", {1, nullptr, amax_dy, amax_w}, bs.relu_bias_ok(c, k), dy, wt, dx, n, h, wd, c, k, r, s,
                    pad_h, pad_w, accumulate, stream, &bs);
}

extern "C" int rr_conv_dgrad_s2_f16x3(const float *dy, const float *w, float *dx, int n, int h, int wd, int c, int k,
                                      int r, int s, int pad_h, int pad_w, int accumulate, float *wsub, const unsigned *amax_dy,
                                      const unsigned *amax_w, hipStream_t stream)
{
    return dgrad_s2_impl("rr_conv_dgrad_s2_f16x3", {1, nullptr, amax_dy, amax_w}, dy, w, dx, n, h, wd, c, k, r, s, pad_h, pad_w, accumulate, wsub,
                         stream);
}

extern "C" int rr_conv_wgrad_f16x3(const float *x, const float *dy, float *dw, int n, int h, int wd, int c, int k,
                                   int r, int s, int stride, int pad_h, int pad_w, int out_h, int out_w, const unsigned *amax_x,
                                   const unsigned *amax_dy, hipStream_t stream)
{
    RR_CHECK_ARG(amax_x && amax_dy, "rr_conv_wgrad_f16x3: the operands' maxima are required");
    return wgrad_impl(x, dy, dw, n, h, wd, c, k, r, s, stride, pad_h, pad_w, out_h, out_w, stream, 1, amax_x, amax_dy);
}
