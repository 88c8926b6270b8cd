// im2col-free NHWC fp32 convolutions on the gfx950 matrix cores (v_mfma_f32_32x32x2_f32).
//
// Replaces, for the hourglass / head / stage-2 stack of the reference, what it delegates to
// cuDNN through nn.Conv2d: /root/reference/backbones/hourglass.py:17,21,25,48,143,167,173,
// /root/reference/detectors/centernet_detector.py:62,73,85,
// /root/reference/detectors/fasterrcnn_detector.py:11 + backbones/resnet.py:22-28.
//
// One implicit-GEMM kernel family, no column matrix is ever materialised:
//   fprop : Y[m,ko]  = sum_{tap,c}  X[pix(m,tap), c]   * W[ko,tap,c]      M = N*P*Q, N = K,  Kg = R*S*C
//   dgrad : dX[m,c]  = sum_{tap,ko} dY[pix'(m,tap),ko] * W[ko,tap,c]      M = N*H*W, N = C,  Kg = R*S*K
//   wgrad : dW[ko,tap,c] += sum_m   dY[m,ko] * X[pix(m,tap), c]           M = K, N = C, Kg = N*P*Q (split)
// Activations NHWC, weights OHWI ([K][R][S][C], torch channels_last of the reference's
// parameter).  Workgroup = 256 threads = 4 waves; block tile 128 x BN (BN = 128: 2x2 waves of
// 64x64; BN = 32: 4x1 waves of 32x32) x 32 deep; operands are staged global -> registers ->
// LDS (double buffered, one barrier per K-step) with the pixel gather / zero padding done on
// the way in; every wave runs TM*TN accumulators of 32x32 (16 VGPRs each).  The [m][k] LDS
// images are padded to 36 floats per row so that one ds_read_b128 per lane feeds four
// MFMA K-steps conflict-free; [k][n] images are read with ds_read_b32.
// K-chunks run channel-chunk outer / filter-tap inner so the 9 taps of a 3x3 re-read the same
// 128-B lines from L2, and block ids are remapped so that an XCD owns a contiguous tile range.
//
// Roofline: MFMA-bound (fp32 matrix peak 157.3 TFLOP/s); algorithmic FLOPs = 2*M*N*Kg.
#include "conv_launch.h"
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// 16 zero bytes in global memory: masked lanes of the gathers load from here, so padding needs no
// select on the loaded value (a select right behind the load would pin an s_waitcnt vmcnt in the stream)
__device__ float rr_zero16[4] = {0.f, 0.f, 0.f, 0.f};

constexpr int BM = 128;
constexpr int BK = 32;   // K-step depth: 32 channels (conv_igemm_kernel's BKT), 32 pixels (conv_wgrad_kernel)

struct ConvArgs {
    const float *src;  // fprop: X [N,H,W,C]      dgrad: dY [N,P,Q,K]
    const float *w;    // [K][R][S][C]
    float *dst;        // fprop: Y [N,P,Q,K]      dgrad: dX [N,H,W,C]
    const float *bias; // fprop only, [K] or null
    double *stat_slab; // fprop only: [mtiles][2][K] per-block column sums / sums of squares, or null
    // BatchNorm-backward sums of the layer that PRODUCED the tensor whose gradient this launch writes (stride-1 data
    // gradient through the forward kernel): with bs_y set the slab receives, per block and column c, sum(d) and
    // sum(d * xhat) with d = dst * relu-mask (mask from bs_z > 0, or recomputed as bs_y*bs_msc+bs_msh > 0) and
    // xhat = (bs_y - bs_mean) * bs_invstd — what rr_bn_bwd_reduce would compute in a separate pass over dst and y.
    const float *bs_y, *bs_z, *bs_mean, *bs_invstd, *bs_msc, *bs_msh;
    // bs_relu_bias != 0: the producer is conv + bias + ReLU (a head's 3x3 layer, centernet_detector.py:62): the epilogue
    // stores the MASKED gradient dst*(bs_z > 0) and the slab's first row holds its column sums = the bias gradient
    // (what rr_bias_relu_bwd computes in a pass of its own); bs_mean / bs_invstd are not read.
    int bs_relu_bias;
    int N;
    int SH, SW, SC;    // source spatial / channels
    int DH, DW, DC;    // destination spatial / channels (DC = GEMM N)
    int R, S, stride, pad_h, pad_w;
    int relu, accumulate;
    int M;             // N*DH*DW
    int Kg;            // R*S*SC
    int wK, wC;        // weight dims K, C
    const float *zero; // 16 zero bytes (rr_zero16) for masked gather lanes
    int ksplit;        // > 1: grid.z slices the K loop and the epilogue adds with float atomics (dst pre-zeroed
                       // or holding the running sum); no bias / ReLU / statistics in that mode
    int parity_order;  // dgrad, stride 2: 4 x 2 bits, parity class handled by blockIdx.y = 0..3 (most taps first)
    int parity;        // dgrad, stride 2: blockIdx.y = output parity class (h%2, w%2); only the taps that
                       // can reach that class are visited (1/2/2/4 of a 3x3) instead of masking 3/4 of the MFMAs
    int dst32;         // destination below 2 GiB (launch_igemm): the epilogue addresses it with 32-bit buffer offsets
    int pos_major;     // fprop on tiny maps (the stage-2 head's 3x3 convolution on 3x3 RoI maps, fasterrcnn_detector.py:18
                       // -> Bottleneck.conv2): an M tile = ONE output pixel of 128 consecutive images, so the taps that
                       // fall into the padding are the same for every row of the tile and are skipped, not masked
                       // (a padded 3x3 on a 3x3 map: 49 of 81 (pixel, tap) pairs are real)
    const int *gate;   // the _unless entry points (plain forward kernel only): the launch returns when *gate <= gate_max — the rows
    int gate_max;      // route of conv_rows.hip, enqueued next to it with the opposite test, does the work then.  null: no gate
    long batch_src, batch_w, batch_dst;   // BATCH instantiations (the sixteen GEMMs of conv_wino.hip in one launch): blockIdx.y moves the
                       // three tensors on by so many elements; every slice is addressed from its own base, so each stays below 2 GiB
};

__device__ __forceinline__ int xcd_remap(int bid, int nb)
{
    const int q = nb >> 3, r = nb & 7, xcd = bid & 7, idx = bid >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// MODE 0 = fprop, 1 = dgrad.  SCALAR: source/weight channel counts not multiples of 4.
// BKT = K-step depth: 32 channels.
// PIPE: 0 plain double-buffered loop; 2 software-pipelined main loop with one LDS image per operand (global loads
// two K-steps ahead, LDS fragments one 8-deep group ahead, two barriers inside the last MFMA group) so that a wave's
// MFMA stream never waits on a barrier or on LDS latency.
// BNS: the epilogue also emits the producer's BatchNorm-backward sums (ConvArgs::bs_y); a separate instantiation so
// that the plain kernel keeps its register budget (three workgroups per CU).
// POSM: position-major M tiles (ConvArgs::pos_major); like BNS a separate instantiation — folded into the plain kernel
// the extra state cost 20 registers and the third workgroup per CU (457 -> 466 ms per train step).
// The pipelined instantiations are compiled FOR three workgroups per CU (168 registers): left to itself the allocator
// follows the epilogue's appetite (220 with the accumulators in AGPRs), not the K loop's.
// BATCH: grid.y = independent problems of one geometry (ConvArgs::batch_*): the pipelined plain forward kernel only.
template <int BN, int MODE, bool SCALAR, int BKT, int PIPE, bool BNS = false, bool POSM = false, bool BATCH = false>
__global__ __launch_bounds__(256, PIPE == 2 ? 3 : 1) void conv_igemm_kernel(const ConvArgs a)
{
    static_assert(BKT == 32 && (PIPE == 0 || PIPE == 2), "conv_igemm_kernel: K-step 32, PIPE 0 or 2");
    static_assert(!BATCH || (MODE == 0 && PIPE == 2 && !BNS && !POSM), "conv_igemm_kernel: BATCH is for the pipelined plain forward kernel");
    if constexpr (MODE == 0 && !BNS && !POSM) {
        if (a.gate != nullptr && *a.gate <= a.gate_max) return;      // wave-uniform: two scalar loads, no vector register
    }
    constexpr int WN = BN / 64 ? BN / 64 : 1;   // waves along N
    constexpr int WM = 4 / WN;                  // waves along M
    constexpr int TM = BM / (WM * 32);
    constexpr int TN = BN / (WN * 32);
    constexpr bool B_KN = (MODE == 1);          // dgrad reads W as [k][n]
    // [m][k] image row stride: padded by 4 floats for conflict-free ds_read_b128
    constexpr int LDK = BKT + 4;
    constexpr int LDB = B_KN ? BN : LDK;
    constexpr int A_ELEMS = BM * LDK;
    constexpr int B_ELEMS = B_KN ? BKT * BN : BN * LDK;
    constexpr int CPR = BKT / 4;                // float4 columns per [m][k] row
    constexpr int RPP = 256 / CPR;              // rows per pass of the 256 threads
    constexpr int AJ = BM / RPP;                // float4 per thread for the A image
    constexpr int BJ_NK = BN / RPP > 0 ? BN / RPP : 1;
    constexpr int TPR = BN / 4;                 // [k][n] image: threads per k-row
    constexpr int KRPP = 256 / TPR;             // k-rows per pass
    constexpr int BJ_KN = BKT / KRPP > 0 ? BKT / KRPP : 1;
    constexpr int BJ = B_KN ? BJ_KN : BJ_NK;

    extern __shared__ __align__(16) float lds[];
    constexpr int NBUF = PIPE == 2 ? 1 : 2;   // PIPE 2: one LDS image per operand, three workgroups per CU
    float *As = lds;                    // [NBUF][A_ELEMS]
    float *Bs = lds + NBUF * A_ELEMS;   // [NBUF][B_ELEMS]

    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int ntiles = (a.DC + BN - 1) / BN;
    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int n_tile = logical % ntiles, m_tile = logical / ntiles;
    int m0 = m_tile * BM;
    const int n0 = n_tile * BN;

    const int RS = a.R * a.S;
    // tap sub-lattice visited by this block: all taps, or (parity mode) r = r0, r0+2, ..  s = s0, s0+2, ..
    int r0 = 0, s0 = 0, tstep = 1, Rc = a.R, Sc = a.S;
    int ph = 0, pw = 0, Hc = a.DH, Wc = a.DW, Mloc = a.M;
    if (MODE == 1 && a.parity) {
        // heaviest parity class first (grid.y is the slow dispatch dimension): no long tail of 4-tap blocks
        const int pcls = (a.parity_order >> (2 * blockIdx.y)) & 3;
        ph = pcls >> 1; pw = pcls & 1;
        Hc = (a.DH - ph + 1) / 2; Wc = (a.DW - pw + 1) / 2;
        Mloc = a.N * Hc * Wc;
        if (m0 >= Mloc) return;
        r0 = (ph + a.pad_h) & 1; s0 = (pw + a.pad_w) & 1; tstep = 2;
        Rc = r0 < a.R ? (a.R - r0 + 1) / 2 : 0;
        Sc = s0 < a.S ? (a.S - s0 + 1) / 2 : 0;
    }
    int pm_pix = 0;
    if constexpr (POSM) {
        // the nine tiles of one block of images are neighbours in the launch order (same XCD: the input rows they
        // share come from its L2)
        const int hw = a.DH * a.DW;
        pm_pix = m_tile % hw;
        m0 = (m_tile / hw) * BM;
        Mloc = a.N;
        ph = pm_pix / a.DW; pw = pm_pix - ph * a.DW;
        const int h_lo = ph * a.stride - a.pad_h, w_lo = pw * a.stride - a.pad_w;   // source pixel under tap (0,0)
        r0 = h_lo < 0 ? -h_lo : 0; s0 = w_lo < 0 ? -w_lo : 0;
        const int r1 = a.SH - h_lo < a.R ? a.SH - h_lo : a.R, s1 = a.SW - w_lo < a.S ? a.SW - w_lo : a.S;
        Rc = r1 > r0 ? r1 - r0 : 0; Sc = s1 > s0 ? s1 - s0 : 0;
    }
    const int RSc = Rc * Sc;
    const int cpt = (a.SC + BKT - 1) / BKT;                // channel chunks per tap (vector mode)
    const int nk_all = SCALAR ? (a.Kg + BKT - 1) / BKT : cpt * RSc;
    // split-K (grid.z): small-spatial layers have too few output tiles for 256 CUs
    int kc_lo = 0, kc_hi = nk_all;
    if (a.ksplit > 1) {
        const int per = (nk_all + a.ksplit - 1) / a.ksplit;
        kc_lo = blockIdx.z * per;
        kc_hi = kc_lo + per < nk_all ? kc_lo + per : nk_all;
        if (kc_lo >= kc_hi) return;
    }

    // ---- per-thread A rows: destination pixel coordinates
    const int a_col = (t % CPR) * 4;
    const int a_row = t / CPR;
    int a_n[AJ], a_h[AJ], a_w[AJ];
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
        const int m = m0 + a_row + RPP * j;
        if (POSM && m < Mloc) {
            a_n[j] = m; a_h[j] = ph; a_w[j] = pw;
        } else if (m < Mloc) {
            const int hw = Hc * Wc;
            const int n = m / hw, rem = m - n * hw;
            const int h = rem / Wc;
            a_n[j] = n; a_h[j] = h * tstep + ph; a_w[j] = (rem - h * Wc) * tstep + pw;
        } else {
            a_n[j] = -1; a_h[j] = 0; a_w[j] = 0;
        }
    }

    f32x4 ra[AJ], rb[BJ];

    // ---- vector mode: branch-free gather.  Per row: element offset of the source pixel seen through
    // local tap (0,0) and a bit mask of the taps that stay inside the source image; per K-step only a
    // wave-uniform tap delta is added.  (fprop: ih = h*stride - pad + r; dgrad stride 1: ih = h + pad - r;
    // dgrad parity class: ih = hh + (ph + pad - r0)/2 - ri.)
    const int sgn = MODE == 0 ? 1 : -1;
    long a_base[AJ];
    unsigned long long a_mask[AJ];
    long b_base[BJ];
    bool b_ok[BJ];
    if (!SCALAR) {
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            int ih0, iw0;
            if (MODE == 0) {
                ih0 = a_h[j] * a.stride - a.pad_h + r0; iw0 = a_w[j] * a.stride - a.pad_w + s0;   // r0 = s0 = 0 unless pos_major
            } else if (a.parity) {
                ih0 = (a_h[j] - ph) / 2 + (ph + a.pad_h - r0) / 2; iw0 = (a_w[j] - pw) / 2 + (pw + a.pad_w - s0) / 2;
            } else {
                ih0 = a_h[j] + a.pad_h; iw0 = a_w[j] + a.pad_w;
            }
            unsigned long long mk = 0ull;
            if (a_n[j] >= 0) {
                for (int ri = 0; ri < Rc; ++ri) {
                    const int ih = ih0 + sgn * ri;
                    if (ih < 0 || ih >= a.SH) continue;
                    for (int si = 0; si < Sc; ++si) {
                        const int iw = iw0 + sgn * si;
                        if (iw >= 0 && iw < a.SW) mk |= 1ull << (ri * Sc + si);
                    }
                }
            }
            a_mask[j] = mk;
            a_base[j] = (((long)(a_n[j] < 0 ? 0 : a_n[j]) * a.SH + ih0) * a.SW + iw0) * a.SC + a_col;
        }
        if (!B_KN) {
#pragma unroll
            for (int j = 0; j < BJ; ++j) {
                const int ko = n0 + a_row + RPP * j;
                b_ok[j] = ko < a.wK && (a_row + RPP * j) < BN;
                b_base[j] = (long)ko * RS * a.wC + a_col;
            }
        } else {
#pragma unroll
            for (int j = 0; j < BJ; ++j) {
                const int c = n0 + (t % TPR) * 4;
                b_ok[j] = c < a.wC && (t / TPR + KRPP * j) < BKT;
                b_base[j] = (long)(t / TPR + KRPP * j) * RS * a.wC + c;
            }
        }
    }

    auto src_offset = [&](int j, int r, int s, long &off) -> bool {
        if (a_n[j] < 0) return false;
        int ih, iw;
        if (MODE == 0) {
            ih = a_h[j] * a.stride - a.pad_h + r;
            iw = a_w[j] * a.stride - a.pad_w + s;
            if (ih < 0 || iw < 0 || ih >= a.SH || iw >= a.SW) return false;
        } else {
            const int th = a_h[j] + a.pad_h - r, tw = a_w[j] + a.pad_w - s;
            if (th < 0 || tw < 0) return false;
            if (a.stride == 1) { ih = th; iw = tw; }
            else {
                ih = th / a.stride; iw = tw / a.stride;
                if (ih * a.stride != th || iw * a.stride != tw) return false;
            }
            if (ih >= a.SH || iw >= a.SW) return false;
        }
        off = (((long)a_n[j] * a.SH + ih) * a.SW + iw) * a.SC;
        return true;
    };

    auto load_tiles = [&](int kc) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        if (!SCALAR) {
            const int cch = kc / RSc, tl = kc - cch * RSc;
            const int ri = tl / Sc, si = tl - ri * Sc;
            const int tap = (r0 + tstep * ri) * a.S + (s0 + tstep * si);
            const int c0 = cch * BKT;
            const long a_delta = (long)sgn * ((long)ri * a.SW + si) * a.SC + c0;
            const bool c_ok = c0 + a_col < a.SC;
            // A: BM rows x BKT channels of one tap; out-of-image rows read a safe address and are zeroed
#pragma unroll
            for (int j = 0; j < AJ; ++j) {
                const bool ok = c_ok && ((a_mask[j] >> tl) & 1ull);
                const float *p = ok ? a.src + a_base[j] + a_delta : a.zero;
                ra[j] = *reinterpret_cast<const f32x4 *>(p);
            }
            if (!B_KN) {  // fprop: B[n = ko][k = (tap, c)] = w[ko][tap][c]
                const long w_delta = (long)tap * a.wC + c0;
                const bool wc_ok = c0 + a_col < a.wC;
#pragma unroll
                for (int j = 0; j < BJ; ++j) {
                    const bool ok = b_ok[j] && wc_ok;
                    const float *p = ok ? a.w + b_base[j] + w_delta : a.zero;
                    rb[j] = *reinterpret_cast<const f32x4 *>(p);
                }
            } else {      // dgrad: B[k = (tap, ko)][n = c] = w[ko][tap][c]; c0 indexes the source channels = K
                const long w_delta = ((long)c0 * RS + tap) * a.wC;
#pragma unroll
                for (int j = 0; j < BJ; ++j) {
                    const bool ok = b_ok[j] && (c0 + t / TPR + KRPP * j < a.wK);
                    const float *p = ok ? a.w + b_base[j] + w_delta : a.zero;
                    rb[j] = *reinterpret_cast<const f32x4 *>(p);
                }
            }
        } else {
            // linear k = tap * SC + c over R*S*SC; the 4 columns of this thread decode once per chunk
            int e_tap[4], e_c[4];
            bool e_ok[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = kc * BKT + a_col + e;
                e_ok[e] = k < a.Kg;
                e_tap[e] = k / a.SC;
                e_c[e] = k - e_tap[e] * a.SC;
            }
#pragma unroll
            for (int j = 0; j < AJ; ++j) {
                f32x4 v = zero;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    long off;
                    const int r = e_tap[e] / a.S, s = e_tap[e] - r * a.S;
                    if (e_ok[e] && src_offset(j, r, s, off)) v[e] = a.src[off + e_c[e]];
                }
                ra[j] = v;
            }
            if (!B_KN) {  // w[ko][k] with k linear — OHWI is already [K][R*S*C]
#pragma unroll
                for (int j = 0; j < BJ; ++j) {
                    const int ko = n0 + a_row + RPP * j;
                    f32x4 v = zero;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int k = kc * BKT + a_col + e;
                        if (ko < a.wK && (a_row + RPP * j) < BN && k < a.Kg) v[e] = a.w[(long)ko * a.Kg + k];
                    }
                    rb[j] = v;
                }
            } else {
#pragma unroll
                for (int j = 0; j < BJ; ++j) {
                    const int kl = t / TPR + KRPP * j;
                    const int k = kc * BKT + kl;                 // k = tap * K + ko
                    const int tap = k / a.SC, ko = k - tap * a.SC;
                    const int c = n0 + (t % TPR) * 4;
                    f32x4 v = zero;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (kl < BKT && k < a.Kg && c + e < a.wC) v[e] = a.w[((long)ko * RS + tap) * a.wC + c + e];
                    rb[j] = v;
                }
            }
        }
    };

    auto store_tiles = [&](int buf) {
        float *A = As + buf * A_ELEMS;
        float *B = Bs + buf * B_ELEMS;
#pragma unroll
        for (int j = 0; j < AJ; ++j)
            *reinterpret_cast<f32x4 *>(A + (a_row + RPP * j) * LDK + a_col) = ra[j];
        if (!B_KN) {
#pragma unroll
            for (int j = 0; j < BJ; ++j)
                if ((a_row + RPP * j) < BN)
                    *reinterpret_cast<f32x4 *>(B + (a_row + RPP * j) * LDK + a_col) = rb[j];
        } else {
#pragma unroll
            for (int j = 0; j < BJ; ++j)
                if ((t / TPR + KRPP * j) < BKT)
                    *reinterpret_cast<f32x4 *>(B + (t / TPR + KRPP * j) * LDB + (t % TPR) * 4) = rb[j];
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int lr = lane & 31, lh = lane >> 5;

    if constexpr (PIPE == 0) {
    if (kc_lo < kc_hi) {
        load_tiles(kc_lo);
        store_tiles(0);
    }
    __syncthreads();
    for (int kc = kc_lo; kc < kc_hi; ++kc) {
        const int buf = (kc - kc_lo) & 1;
        if (kc + 1 < kc_hi) load_tiles(kc + 1);
        const float *A = As + buf * A_ELEMS;
        const float *B = Bs + buf * B_ELEMS;
#pragma unroll
        for (int kk = 0; kk < BKT / 8; ++kk) {
            f32x4 fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                fa[i] = *reinterpret_cast<const f32x4 *>(A + ((wm * TM + i) * 32 + lr) * LDK + kk * 8 + lh * 4);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                if (!B_KN) {
                    fb[j] = *reinterpret_cast<const f32x4 *>(B + ((wn * TN + j) * 32 + lr) * LDK + kk * 8 + lh * 4);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) fb[j][e] = B[(kk * 8 + lh * 4 + e) * LDB + (wn * TN + j) * 32 + lr];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
        }
        if (kc + 1 < kc_hi) store_tiles(buf ^ 1);
        __syncthreads();
    }
    } else {
    static_assert(!SCALAR && (BN == 128 || BN == 64),
                  "pipelined loop: 4 groups of 8 per K-step, vector gather, 128x128 or 128x64 tile");
    // Each K-step = 4 groups x 4 sub-groups of 4 MFMAs.  Memory instructions are dealt out between the
    // sub-groups (never clustered): a VMEM / DS issue that would stall this wave's in-order stream then
    // overlaps the 64-cycle MFMAs already in the pipe (probe: clustered ds_write+barrier costs 5 %,
    // clustered global loads another 7 % of MFMA throughput).
    f32x4 fa0[TM], fb0[TN], fa1[TM], fb1[TN];
    auto read_frags = [&](int buf, int kk, f32x4 (&fa)[TM], f32x4 (&fb)[TN]) {
        const float *A = As + buf * A_ELEMS;
        const float *B = Bs + buf * B_ELEMS;
#pragma unroll
        for (int i = 0; i < TM; ++i)
            fa[i] = *reinterpret_cast<const f32x4 *>(A + ((wm * TM + i) * 32 + lr) * LDK + kk * 8 + lh * 4);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            if (!B_KN) {
                fb[j] = *reinterpret_cast<const f32x4 *>(B + ((wn * TN + j) * 32 + lr) * LDK + kk * 8 + lh * 4);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) fb[j][e] = B[(kk * 8 + lh * 4 + e) * LDB + (wn * TN + j) * 32 + lr];
            }
        }
    };
    auto sub = [&](const f32x4 (&fa)[TM], const f32x4 (&fb)[TN], int e) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][e], fb[j][e], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    // Buffer-addressed gathers: 32-bit byte offsets, out-of-range => hardware returns 0 (no zero-page
    // select, no 64-bit pointer arithmetic per load).  The host only takes this path when both tensors are
    // smaller than 2 GiB.
    // descriptor inputs pass through readfirstlane so that hipcc can PROVE the SRD wave-uniform; otherwise it
    // wraps every buffer_load in a waterfall loop (cdna_hip_programming.md T20)
    auto make_srd = [](const float *p, long bytes) {
        const unsigned long long u = reinterpret_cast<unsigned long long>(p);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u);
        const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
        void *q = reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo);
        return __builtin_amdgcn_make_buffer_rsrc(q, 0, __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t rs_src = make_srd(BATCH ? a.src + (long)blockIdx.y * a.batch_src : a.src, (long)a.N * a.SH * a.SW * a.SC * 4);
    const __amdgpu_buffer_rsrc_t rs_w = make_srd(BATCH ? a.w + (long)blockIdx.y * a.batch_w : a.w, (long)a.wK * RS * a.wC * 4);
    constexpr unsigned OOB = 0xFFFFFFF0u;
    int a_boff[AJ], b_boff[BJ];
#pragma unroll
    for (int j = 0; j < AJ; ++j) a_boff[j] = (int)(a_base[j] * 4);
#pragma unroll
    for (int j = 0; j < BJ; ++j) b_boff[j] = (int)(b_base[j] * 4);
    // wave-uniform state of the K-step being fetched, advanced incrementally (tap inner, channel chunk outer)
    int p_cch = kc_lo / RSc, p_tl = kc_lo - (kc_lo / RSc) * RSc;
    int p_ri = p_tl / Sc, p_si = p_tl - (p_tl / Sc) * Sc;
    int p_adelta = 0, p_wdelta = 0, p_c0 = 0, p_tlc = 0;
    bool p_cok = false, p_wcok = false, p_live = true;
    auto prep = [&]() {            // describes step (p_cch, p_ri, p_si), then advances to the next one
        const int tap = (r0 + tstep * p_ri) * a.S + (s0 + tstep * p_si);
        p_c0 = p_cch * BKT;
        p_tlc = p_tl;
        p_adelta = (sgn * (p_ri * a.SW + p_si) * a.SC + p_c0) * 4;
        p_cok = p_c0 + a_col < a.SC;
        p_wdelta = (B_KN ? (p_c0 * RS + tap) * a.wC : tap * a.wC + p_c0) * 4;
        p_wcok = p_c0 + a_col < a.wC;
        ++p_tl;
        if (++p_si == Sc) { p_si = 0; ++p_ri; }
        if (p_tl == RSc) { p_tl = 0; p_ri = 0; p_si = 0; ++p_cch; }
    };
    auto load_a = [&](int j) {
        // bitwise, not &&: a short-circuit on the per-lane p_cok becomes a divergent branch whose arms share
        // destination registers, and hipcc then parks an s_waitcnt vmcnt(0) between consecutive loads
        const unsigned ok = (unsigned)p_cok & (unsigned)((a_mask[j] >> p_tlc) & 1ull) & (unsigned)p_live;
        const unsigned off = ok ? (unsigned)(a_boff[j] + p_adelta) : OOB;
        ra[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_src, off, 0, 0));
    };
    auto load_b = [&](int j) {
        if (j >= BJ) return;           // 128x64 tile: two weight float4 per thread (j is a literal at every call site)
        const unsigned ok = (B_KN ? ((unsigned)b_ok[j] & (unsigned)(p_c0 + t / TPR + KRPP * j < a.wK))
                                  : ((unsigned)b_ok[j] & (unsigned)p_wcok)) & (unsigned)p_live;
        const unsigned off = ok ? (unsigned)(b_boff[j] + p_wdelta) : OOB;
        rb[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, off, 0, 0));
    };
    auto store_a = [&](int j, int buf) {
        *reinterpret_cast<f32x4 *>(As + buf * A_ELEMS + (a_row + RPP * j) * LDK + a_col) = ra[j];
    };
    auto store_b = [&](int j, int buf) {
        if (j >= BJ) return;
        if (!B_KN) *reinterpret_cast<f32x4 *>(Bs + buf * B_ELEMS + (a_row + RPP * j) * LDK + a_col) = rb[j];
        else *reinterpret_cast<f32x4 *>(Bs + buf * B_ELEMS + (t / TPR + KRPP * j) * LDB + (t % TPR) * 4) = rb[j];
    };
    static_assert(AJ == 4 && (BJ == 4 || BJ == 2), "piece schedule below: 4 + (4 | 2) float4 per thread");
    if (kc_lo < kc_hi) {
        prep();
#pragma unroll
        for (int j = 0; j < 4; ++j) { load_a(j); load_b(j); }
#pragma unroll
        for (int j = 0; j < 4; ++j) { store_a(j, 0); store_b(j, 0); }
        if (kc_lo + 1 < kc_hi) {      // stays in registers until the first phase's group 1
            prep();
#pragma unroll
            for (int j = 0; j < 4; ++j) { load_a(j); load_b(j); }
        }
    }
    __syncthreads();
    if (kc_lo < kc_hi) read_frags(0, 0, fa0, fb0);
    // Single LDS image, two barriers per K-step, both inside group 3: after the last fragment reads of tile kc
    // everybody waits (1), the registers holding tile kc+1 are written over it, everybody waits (2), then the
    // first fragments of kc+1 and the global loads of kc+2 go out — all under group 3's 16 MFMAs.  Half the LDS
    // of the double-buffered loop: a third workgroup fits on the CU and covers the barrier waits.
    // The body is branch-free on purpose: past the end of the K range the loads turn into out-of-range buffer reads
    // (zeros) that nobody consumes.  With `if (has_next)` arms hipcc's waitcnt pass loses track of which loads the
    // ds_writes already retired and parks s_waitcnt vmcnt(1) between consecutive load pairs, serialising them.
    for (int kc = kc_lo; kc < kc_hi; ++kc) {
        p_live = kc + 2 < kc_hi;
        read_frags(0, 1, fa1, fb1);
        sub(fa0, fb0, 0); sub(fa0, fb0, 1); sub(fa0, fb0, 2); sub(fa0, fb0, 3);
        read_frags(0, 2, fa0, fb0);
        sub(fa1, fb1, 0); sub(fa1, fb1, 1); sub(fa1, fb1, 2); sub(fa1, fb1, 3);
        read_frags(0, 3, fa1, fb1);
        sub(fa0, fb0, 0); sub(fa0, fb0, 1); sub(fa0, fb0, 2); sub(fa0, fb0, 3);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        store_a(0, 0); store_a(1, 0); store_a(2, 0); store_a(3, 0);
        sub(fa1, fb1, 0);
        store_b(0, 0); store_b(1, 0); store_b(2, 0); store_b(3, 0);
        sub(fa1, fb1, 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        read_frags(0, 0, fa0, fb0);
        prep();
        load_a(0); load_a(1); load_a(2); load_a(3);
        sub(fa1, fb1, 2);
        load_b(0); load_b(1); load_b(2); load_b(3);
        sub(fa1, fb1, 3);
    }
    }

    // ---- epilogue.  D layout: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
    double *sred = reinterpret_cast<double *>(lds);   // [WM][BN][2], reuses the staging LDS
    const bool do_stats = (MODE == 0) && a.stat_slab != nullptr && a.ksplit <= 1;
    constexpr bool bnsum = BNS;                                     // statistics = the producer's BN-backward sums
    // (the host takes the BNS variant only for destinations below 2 GiB; unused and dropped otherwise)
    auto bs_srd = [](const float *p, long bytes) {
        const unsigned long long u = reinterpret_cast<unsigned long long>(p);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u);
        const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
        void *q = reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo);
        return __builtin_amdgcn_make_buffer_rsrc(q, 0, __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t bs_rs_y = bs_srd(BNS ? a.bs_y : a.src, (long)a.M * a.DC * 4);
    const __amdgpu_buffer_rsrc_t bs_rs_z = bs_srd(BNS && a.bs_z != nullptr ? a.bs_z : a.src, (long)a.M * a.DC * 4);
    // the destination through a buffer descriptor (dst32: below 2 GiB, set by launch_igemm): 32-bit byte offsets, and a lane
    // whose row or column lies outside the tensor gets an out-of-range offset, so the buffer unit drops its store / atomic
    // and answers its load with 0 — no exec-mask branch per element, hence nothing between consecutive stores
    const __amdgpu_buffer_rsrc_t rs_dst = bs_srd(BATCH ? a.dst + (long)blockIdx.y * a.batch_dst : a.dst, a.dst32 ? (long)a.M * a.DC * 4 : 0);
    constexpr unsigned OOBD = 0xFFFFFFF0u;
    const int mode_e = a.ksplit > 1 ? 2 : (a.accumulate ? 1 : 0);   // wave-uniform: one branch around the whole epilogue
    auto put_stats = [&](int j, float s1, float s2) {
        double d1 = (double)s1, d2 = (double)s2;
        d1 += __shfl_xor(d1, 32, 64);
        d2 += __shfl_xor(d2, 32, 64);
        if (lh == 0) {
            const int cl = (wn * TN + j) * 32 + lr;
            sred[(wm * BN + cl) * 2 + 0] = d1;
            sred[(wm * BN + cl) * 2 + 1] = d2;
        }
    };
    // One 32x32 accumulator tile at the byte offsets off[0..15] (OOBD: the element is outside the tensor).  mode is a
    // literal at every call: 0 store, 1 add to the destination (its 16 loads go out first), 2 split-K float atomics.
    auto put_tile = [&](const f32x16 &c, const unsigned (&off)[16], float bv, float &s1, float &s2, int mode)
                        __attribute__((always_inline)) {
        const bool relu = MODE == 0 && a.relu;
        float v[16], old[16];
        if (mode == 1) {
#pragma unroll
            for (int e = 0; e < 16; ++e)
                old[e] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_dst, off[e], 0, 0));
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            v[e] = c[e] + bv;
            v[e] = (relu & !(v[e] > 0.f)) ? 0.f : v[e];
        }
        if (mode == 2) {
#pragma unroll
            for (int e = 0; e < 16; ++e)      // partial sums of the K slices meet in a zeroed / running dst
                __builtin_amdgcn_raw_ptr_buffer_atomic_fadd_f32(v[e], rs_dst, off[e], 0, 0);
            return;
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            if (mode == 1) v[e] += old[e];
            __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v[e]), rs_dst, off[e], 0, 0);
        }
        if (MODE == 0) {
#pragma unroll
            for (int e = 0; e < 16; ++e) {    // a dropped element adds +0 to both chains: s1, s2 never hold -0
#pragma clang fp contract(off)                // the square is rounded before it is added, as it always was: slabs keep their bits
                const float vm = off[e] != OOBD ? v[e] : 0.f;
                s1 += vm;
                s2 += vm * vm;
            }
        }
    };
    auto put_tiles = [&](int mode) __attribute__((always_inline)) {
        if constexpr (MODE == 0) {
            // consecutive rows of a tile are DC floats apart (position-major: one image apart)
            const int rstride = POSM ? a.DH * a.DW * a.DC * 4 : a.DC * 4;
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int ncol = n0 + (wn * TN + j) * 32 + lr;
                const bool n_ok = ncol < a.DC;
                const float bv = (a.bias != nullptr && n_ok) ? a.bias[ncol] : 0.f;
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int mrow = m0 + (wm * TM + i) * 32 + 4 * lh;        // first row of this lane half
                    const int lim = n_ok ? Mloc - mrow : 0;                  // its rows below lim exist
                    const unsigned base = (unsigned)(((POSM ? mrow * (a.DH * a.DW) + pm_pix : mrow) * a.DC + ncol) * 4);
                    unsigned off[16];
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int row = (e & 3) + 8 * (e >> 2);
                        off[e] = row < lim ? base + (unsigned)(row * rstride) : OOBD;
                    }
                    put_tile(acc[i][j], off, bv, s1, s2, mode);
                    __builtin_amdgcn_sched_barrier(0);      // one tile's offsets and values live at a time
                }
                if (do_stats) put_stats(j, s1, s2);
            }
        } else {
            // data gradient: no statistics, so the row tiles go outside and the pixel of every row (parity classes: two
            // divisions) is worked out once for all column tiles
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                unsigned roff[16];
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int m = m0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                    int pix = m;
                    if (a.parity) {
                        const int hw = Hc * Wc;
                        const int n = m / hw, rem = m - n * hw;
                        const int h = rem / Wc;
                        pix = (n * a.DH + (h * 2 + ph)) * a.DW + ((rem - h * Wc) * 2 + pw);
                    }
                    roff[e] = m < Mloc ? (unsigned)(pix * a.DC * 4) : OOBD;
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int ncol = n0 + (wn * TN + j) * 32 + lr;
                    const bool n_ok = ncol < a.DC;
                    unsigned off[16];
#pragma unroll
                    for (int e = 0; e < 16; ++e) off[e] = (n_ok & (roff[e] != OOBD)) ? roff[e] + (unsigned)(ncol * 4) : OOBD;
                    float s1 = 0.f, s2 = 0.f;
                    put_tile(acc[i][j], off, 0.f, s1, s2, mode);
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
        }
    };
    // BNS: the producer's pre-BN output (and, for layers with a residual, its post-activation output) is fetched for a
    // half-tile of 8 rows before the first dependent use, and with accum the destination's running values with them.  One
    // per-lane byte offset (row of this lane half, its column), the row inside the tile goes through the buffer
    // instruction's scalar offset: no 64-bit address per access, and columns past the end read 0 / drop their store.
    // (The host sends only whole tiles here: the range check does not cover the scalar offset.)
    auto put_tiles_bns = [&](bool accum) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int ncol = n0 + (wn * TN + j) * 32 + lr;
            const bool n_ok = ncol < a.DC;
            float s1 = 0.f, s2 = 0.f;
            float bs_m = 0.f, bs_i = 0.f, bs_sc = 0.f, bs_sh = 0.f;
            if (n_ok && !a.bs_relu_bias) {
                bs_m = a.bs_mean[ncol]; bs_i = a.bs_invstd[ncol];
                if (a.bs_z == nullptr) {
                    if (a.bs_msc != nullptr) { bs_sc = a.bs_msc[ncol]; bs_sh = a.bs_msh[ncol]; }
                    else bs_sh = 1.f;          // a layer without ReLU: every element counts
                }
            }
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const bool use_z = a.bs_z != nullptr;
                const unsigned voff = n_ok ? (unsigned)(((m0 + (wm * TM + i) * 32 + 4 * lh) * a.DC + ncol) * 4) : OOBD;
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {
                    float yv[8], zv[8], old[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const int e = hh * 8 + q;
                        const int soff = __builtin_amdgcn_readfirstlane(((e & 3) + 8 * (e >> 2)) * a.DC * 4);
                        yv[q] = a.bs_relu_bias ? 0.f : __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(bs_rs_y, voff, soff, 0));
                        zv[q] = use_z ? __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(bs_rs_z, voff, soff, 0)) : 0.f;
                        if (accum) old[q] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_dst, voff, soff, 0));
                    }
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
#pragma clang fp contract(off)                        // every product of the chains is rounded on its own, as it always was
                        const int e = hh * 8 + q;
                        const int soff = __builtin_amdgcn_readfirstlane(((e & 3) + 8 * (e >> 2)) * a.DC * 4);
                        float v = acc[i][j][e];
                        if (accum) v += old[q];
                        const bool on = use_z ? zv[q] > 0.f : rr_bn_affine(yv[q], bs_sc, bs_sh) > 0.f;
                        const float d = on ? v : 0.f;
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, a.bs_relu_bias ? d : v), rs_dst, voff, soff, 0);
                        s1 += d;
                        s2 += d * ((yv[q] - bs_m) * bs_i);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
            if (do_stats) put_stats(j, s1, s2);
        }
    };
    // destinations of 2 GiB and more: 64-bit addresses and a branch per element
    auto put_tiles_wide = [&]() {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int ncol = n0 + (wn * TN + j) * 32 + lr;
            const bool n_ok = ncol < a.DC;
            const float bv = (MODE == 0 && a.bias != nullptr && n_ok) ? a.bias[ncol] : 0.f;
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int row = (e & 3) + 8 * (e >> 2) + 4 * lh;
                    const int m = m0 + (wm * TM + i) * 32 + row;
                    float v = acc[i][j][e] + bv;
                    if (MODE == 0 && a.relu) v = v > 0.f ? v : 0.f;
                    if (m < Mloc && n_ok) {
                        long pix = m;
                        if constexpr (POSM) pix = (long)m * (a.DH * a.DW) + pm_pix;
                        if (MODE == 1 && a.parity) {
                            const int hw = Hc * Wc;
                            const int n = m / hw, rem = m - n * hw;
                            const int h = rem / Wc;
                            pix = ((long)n * a.DH + (h * 2 + ph)) * a.DW + ((rem - h * Wc) * 2 + pw);
                        }
                        float *p = a.dst + pix * a.DC + ncol;
                        if (mode_e == 2) {
                            unsafeAtomicAdd(p, v);        // partial sums of the K slices meet in a zeroed / running dst
                        } else {
                            if (mode_e == 1) v += *p;
                            *p = v;
                            s1 += v;
                            s2 += v * v;
                        }
                    }
                }
            }
            if (do_stats) put_stats(j, s1, s2);
        }
    };
    if constexpr (bnsum) {
        if (mode_e == 1) put_tiles_bns(true);
        else put_tiles_bns(false);
    } else if (!a.dst32) {
        put_tiles_wide();
    } else if (mode_e == 0) {
        put_tiles(0);
    } else if (mode_e == 1) {
        put_tiles(1);
    } else {
        put_tiles(2);
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

// ---------------------------------------------------------------------------------------------
// wgrad: dW[ko][tap][c] += sum over a slice of the N*P*Q pixels.  GEMM M = K (ko), N = C.
struct WgradArgs {
    const float *x;   // [N,H,W,C]
    const float *dy;  // [N,P,Q,K]
    float *dw;        // [K][R][S][C], accumulated with float atomics
    const float *zero; // 16 zero bytes for masked gather lanes
    int N, H, W, C, K, R, S, P, Q, stride, pad_h, pad_w;
    int M;            // N*P*Q
    int chunks_per_split;
    int mt, nt;       // tiles along K and C
    const int *gate;  // rr_conv_wgrad_unless: the launch returns when *gate <= gate_max (ConvArgs::gate); null: no gate
    int gate_max;
    long slice_x, slice_dy;   // BATCH instantiations (the sixteen GEMMs of the Winograd weight gradient in one launch): the "tap" moves
                      // x and dy on by so many elements; every slice is addressed from its own base, so each stays below 2 GiB
};

// BMW x BN output tile (ko x c).  128x128: 2x2 waves of 64x64; 128x32 / 32x128: 4 waves of one 32x32;
// 32x32: the 4 waves split the 32-deep K-step between them (their partial sums meet in the atomics).
// PIPE: 0 plain double-buffered loop; 1 software-pipelined (two LDS images); 3 software-pipelined for Q % BK == 0,
// where the BK pixels of a K-step lie in one output row: the row walk (n, p, q0) is wave-uniform and lives in SGPRs,
// the tensor offsets go through the buffer instruction's scalar offset, and the per-lane work per load is one add, one
// compare, one select; ONE LDS image per operand and two barriers inside the last MFMA group (three workgroups per CU,
// like conv_igemm_kernel<PIPE 2>).
// BATCH (rr_conv_wino_wgrad_gemm): sixteen independent GEMMs dw[ko][i][c] += sum_t dy_i[t][ko] * x_i[t][c] of one geometry
// (N = H = P = 1, W = Q = T, no shift, no padding): the "tap" i selects the operand slices (WgradArgs::slice_*) instead of a
// spatial shift.  The tiles of one (slice, split) are neighbours in the logical id, so that they meet in one XCD's L2.
template <int BMW, int BN, bool A_SCALAR, bool B_SCALAR, int PIPE, bool BATCH = false>
__global__ __launch_bounds__(256, PIPE == 3 ? 3 : 1) void conv_wgrad_kernel(const WgradArgs a)
{
    static_assert(PIPE == 0 || PIPE == 1 || PIPE == 3, "conv_wgrad_kernel: PIPE 0, 1 or 3");
    static_assert(!BATCH || (PIPE != 0 && BMW == 128 && BN == 128 && !A_SCALAR && !B_SCALAR), "conv_wgrad_kernel: BATCH on the pipelined 128x128 kernels");
    if (a.gate != nullptr && *a.gate <= a.gate_max) return;
    constexpr int TILES = (BMW / 32) * (BN / 32);
    constexpr int KS = TILES == 1 ? 4 : 1;                       // waves splitting K
    constexpr int WN = TILES == 16 ? 2 : (BN / 32 >= 4 ? 4 : 1);
    constexpr int WM = 4 / (WN * KS);
    constexpr int TM = BMW / (WM * 32);
    constexpr int TN = BN / (WN * 32);
    constexpr int A_ELEMS = BK * BMW, B_ELEMS = BK * BN;
    constexpr int TPR_A = BMW / 4, RPP_A = 256 / TPR_A, AJ = BMW / 32;
    constexpr int TPR_B = BN / 4, RPP_B = 256 / TPR_B, BJ = BN / 32;

    extern __shared__ __align__(16) float lds[];
    constexpr int NBUF = PIPE == 3 ? 1 : 2;
    float *As = lds, *Bs = lds + NBUF * A_ELEMS;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wk = KS > 1 ? wave : 0;
    const int wm = KS > 1 ? 0 : wave / WN, wn = KS > 1 ? 0 : wave % WN;
    const int RS = BATCH ? 16 : a.R * a.S;
    int logical = xcd_remap(blockIdx.x, gridDim.x);
    int tap, n_tile, m_tile, split;
    if constexpr (BATCH) {
        n_tile = logical % a.nt; logical /= a.nt;
        m_tile = logical % a.mt; logical /= a.mt;
        tap = logical % RS;
        split = logical / RS;
    } else {
        tap = logical % RS; logical /= RS;
        n_tile = logical % a.nt; logical /= a.nt;
        m_tile = logical % a.mt;
        split = logical / a.mt;
    }
    const int r = BATCH ? 0 : tap / a.S, s = BATCH ? 0 : tap - r * a.S;
    const int ko0 = m_tile * BMW, c0 = n_tile * BN;
    const int total_chunks = (a.M + BK - 1) / BK;
    const int kc_begin = split * a.chunks_per_split;
    int kc_end = kc_begin + a.chunks_per_split;
    if (kc_end > total_chunks) kc_end = total_chunks;
    if (kc_begin >= kc_end) return;

    f32x4 ra[AJ], rb[BJ];
    const int a_row = t / TPR_A, a_col = (t % TPR_A) * 4;
    const int b_row = t / TPR_B, b_col = (t % TPR_B) * 4;

    // running (n, p, q) of every B row: advanced by BK pixels per K-step instead of two integer
    // divisions per row per step
    int bn_[BJ], bp_[BJ], bq_[BJ];
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
        const long m = (long)kc_begin * BK + b_row + RPP_B * j;
        const int pq = a.P * a.Q;
        bn_[j] = (int)(m / pq);
        const int rem = (int)(m - (long)bn_[j] * pq);
        bp_[j] = rem / a.Q;
        bq_[j] = rem - bp_[j] * a.Q;
    }
    const bool a_ko_ok = ko0 + a_col < a.K;
    const bool b_c_ok = c0 + b_col < a.C;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

    auto load_tiles = [&](int kc) {
#pragma unroll
        for (int j = 0; j < AJ; ++j) {
            const int m = kc * BK + a_row + RPP_A * j;
            const int ko = ko0 + a_col;
            if (!A_SCALAR) {
                const bool ok = a_ko_ok && m < a.M;
                const float *p = ok ? a.dy + (long)m * a.K + ko : a.zero;
                ra[j] = *reinterpret_cast<const f32x4 *>(p);
            } else {
                f32x4 v = zero4;
                if (m < a.M) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (ko + e < a.K) v[e] = a.dy[(long)m * a.K + ko + e];
                }
                ra[j] = v;
            }
        }
#pragma unroll
        for (int j = 0; j < BJ; ++j) {
            const int c = c0 + b_col;
            const int ih = bp_[j] * a.stride - a.pad_h + r, iw = bq_[j] * a.stride - a.pad_w + s;
            const bool in = bn_[j] < a.N && ih >= 0 && iw >= 0 && ih < a.H && iw < a.W;
            const long off = (((long)bn_[j] * a.H + ih) * a.W + iw) * a.C + c;
            if (!B_SCALAR) {
                const bool ok = in && b_c_ok;
                const float *p = ok ? a.x + off : a.zero;
                rb[j] = *reinterpret_cast<const f32x4 *>(p);
            } else {
                f32x4 v = zero4;
                if (in) {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (c + e < a.C) v[e] = a.x[off + e];
                }
                rb[j] = v;
            }
            // advance this row by BK pixels
            bq_[j] += BK;
            while (bq_[j] >= a.Q) {
                bq_[j] -= a.Q;
                if (++bp_[j] == a.P) { bp_[j] = 0; ++bn_[j]; }
            }
        }
    };
    auto store_tiles = [&](int buf) {
        float *A = As + buf * A_ELEMS, *B = Bs + buf * B_ELEMS;
#pragma unroll
        for (int j = 0; j < AJ; ++j) *reinterpret_cast<f32x4 *>(A + (a_row + RPP_A * j) * BMW + a_col) = ra[j];
#pragma unroll
        for (int j = 0; j < BJ; ++j) *reinterpret_cast<f32x4 *>(B + (b_row + RPP_B * j) * BN + b_col) = rb[j];
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int lr = lane & 31, lh = lane >> 5;
    constexpr bool WPIPE = PIPE != 0 && (BMW == 128 && BN == 128 && !A_SCALAR && !B_SCALAR);
    constexpr bool ALIGNED = PIPE == 3;       // uniform row walk
    if constexpr (!WPIPE) {
    load_tiles(kc_begin);
    store_tiles(0);
    __syncthreads();
    for (int kc = kc_begin; kc < kc_end; ++kc) {
        const int buf = (kc - kc_begin) & 1;
        if (kc + 1 < kc_end) load_tiles(kc + 1);
        const float *A = As + buf * A_ELEMS, *B = Bs + buf * B_ELEMS;
#pragma unroll
        for (int k2 = 0; k2 < BK / 2 / KS; ++k2) {
            const int kr = 2 * (k2 + wk * (BK / 2 / KS)) + lh;
            float fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = A[kr * BMW + (wm * TM + i) * 32 + lr];
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = B[kr * BN + (wn * TN + j) * 32 + lr];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (kc + 1 < kc_end) store_tiles(buf ^ 1);
        __syncthreads();
    }
    } else {
    // Software-pipelined form (same scheme as conv_igemm_kernel<PIPE>): 16 sub-steps of 4 MFMAs per
    // K-step; fragments one sub-step ahead in registers, the next tile's ds_writes in sub-steps 1-4, the
    // global loads two K-steps ahead in sub-steps 6-9, the only barrier after sub-step 14.
    // fragments of one GROUP (4 sub-steps = 8 pixels of K) per register set, two sets: the reads of the next
    // group are issued a whole group (16 MFMAs) ahead, as in conv_igemm_kernel<PIPE> — with one sub-step of
    // lead the ds_read_b32 latency under load was still exposed every 4 MFMAs
    float fa0[4][TM], fb0[4][TN], fa1[4][TM], fb1[4][TN];
    auto rdg = [&](int buf, int g, float (&fa)[4][TM], float (&fb)[4][TN]) {
        const float *A = As + buf * A_ELEMS, *B = Bs + buf * B_ELEMS;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int kr = 2 * (4 * g + q) + lh;
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[q][i] = A[kr * BMW + (wm * TM + i) * 32 + lr];
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[q][j] = B[kr * BN + (wn * TN + j) * 32 + lr];
        }
    };
    auto sub = [&](const float (&fa)[4][TM], const float (&fb)[4][TN], int q) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[q][i], fb[q][j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    };
    auto make_srd = [](const float *p, long bytes) {   // provably wave-uniform descriptor (T20)
        const unsigned long long u = reinterpret_cast<unsigned long long>(p);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u);
        const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
        void *q = reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo);
        return __builtin_amdgcn_make_buffer_rsrc(q, 0, __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
    };
    const __amdgpu_buffer_rsrc_t rs_dy = make_srd(BATCH ? a.dy + (long)tap * a.slice_dy : a.dy, (long)a.M * a.K * 4);
    // Uniform row walk: the descriptor of x starts pad_w pixels BEFORE the tensor, so that the per-lane
    // offset (lq*stride + s) * C is never negative.  A negative (wrapped) lane offset is out of range for the
    // hardware's bounds check even when the scalar offset brings the address back inside the tensor — the left-most
    // tap column then silently lost the pixel in front of every K-step that does not start a row (Q > 32).  Lanes
    // whose pixel really lies outside the row are masked by the iw test below and never dereference the shifted base.
    const long x_shift = ALIGNED ? (long)a.pad_w * a.C * 4 : 0;
    const __amdgpu_buffer_rsrc_t rs_x = make_srd(reinterpret_cast<const float *>(reinterpret_cast<const char *>(BATCH ? a.x + (long)tap * a.slice_x : a.x) - x_shift),
                                                 (long)a.N * a.H * a.W * a.C * 4 + x_shift);
    constexpr unsigned OOB = 0xFFFFFFF0u;
    // A rows: byte offset of row j at K-step 0 of this split is a_off[j]; every K-step adds BK*K*4 (scalar)
    int a_off[AJ], a_m[AJ];
#pragma unroll
    for (int j = 0; j < AJ; ++j) {
        a_m[j] = a_row + RPP_A * j;
        a_off[j] = (a_m[j] * a.K + ko0 + a_col) * 4;
    }
    const int a_step = BK * a.K * 4;
    const int rr_off = r - a.pad_h, ss_off = s - a.pad_w;
    constexpr unsigned FAR = 0x80000000u;   // beyond any (< 2 GiB) tensor, no 32-bit wrap when a scalar offset is added
    // ---- aligned mode state: uniform pixel-row walk + per-lane constants
    int s_n = 0, s_p = 0, s_q0 = 0;
    unsigned a_voff[AJ], b_voff[BJ];
    int b_iw0[BJ];
    if constexpr (ALIGNED) {
        const int m0 = kc_begin * BK, pq = a.P * a.Q;
        s_n = m0 / pq;
        const int rem = m0 - s_n * pq;
        s_p = rem / a.Q;
        s_q0 = rem - s_p * a.Q;
#pragma unroll
        for (int j = 0; j < AJ; ++j) a_voff[j] = a_ko_ok ? (unsigned)a_off[j] : FAR;
#pragma unroll
        for (int j = 0; j < BJ; ++j) {
            const int lq = b_row + RPP_B * j;                     // pixel of this row inside the K-step
            b_iw0[j] = lq * a.stride + ss_off;                    // iw = q0*stride + b_iw0
            // relative to the shifted descriptor: (lq*stride + s) pixels, always >= 0
            b_voff[j] = b_c_ok ? (unsigned)(((lq * a.stride + s) * a.C + c0 + b_col) * 4) : FAR;
        }
    }
    auto load_a = [&](int j, int kc) {
        if constexpr (ALIGNED) {
            const int kcl = kc < kc_end ? kc : kc_end - 1;        // past the end: re-read the last chunk (never consumed)
            const int soff = __builtin_amdgcn_readfirstlane(kcl * a_step);
            ra[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_dy, a_voff[j], soff, 0));
        } else {
            const unsigned ok = (unsigned)a_ko_ok & (unsigned)(kc * BK + a_m[j] < a.M) & (unsigned)(kc < kc_end);
            const unsigned off = ok ? (unsigned)(a_off[j] + kc * a_step) : OOB;
            ra[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_dy, off, 0, 0));
        }
    };
    auto load_b = [&](int j) {
        if constexpr (ALIGNED) {
            const int ih = s_p * a.stride + rr_off;
            const bool s_ok = (s_n < a.N) & ((unsigned)ih < (unsigned)a.H);
            // scalar part of the address: pixel (n, ih, q0*stride), never negative
            const int sbase = s_ok ? (((s_n * a.H + ih) * a.W + s_q0 * a.stride) * a.C) * 4 : 0;
            const int iw = s_q0 * a.stride + b_iw0[j];
            const bool ok = s_ok & ((unsigned)iw < (unsigned)a.W);
            const unsigned voff = ok ? b_voff[j] : FAR;
            rb[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                  rs_x, voff, __builtin_amdgcn_readfirstlane(sbase), 0));
        } else {
            const int ih = bp_[j] * a.stride + rr_off, iw = bq_[j] * a.stride + ss_off;
            const unsigned ok = (unsigned)b_c_ok & (unsigned)(bn_[j] < a.N) & (unsigned)((unsigned)ih < (unsigned)a.H) &
                                (unsigned)((unsigned)iw < (unsigned)a.W);
            const unsigned off = ok ? (unsigned)((((bn_[j] * a.H + ih) * a.W + iw) * a.C + c0 + b_col) * 4) : OOB;
            rb[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_x, off, 0, 0));
        }
    };
    auto adv_b = [&](int j) {   // advance row j by BK pixels (kept apart from the load to keep VALU clusters short)
        if constexpr (ALIGNED) {
            if (j == BJ - 1) {                                    // one uniform step per K-step
                s_q0 += BK;
                if (s_q0 >= a.Q) { s_q0 = 0; if (++s_p == a.P) { s_p = 0; ++s_n; } }
            }
        } else {
        bq_[j] += BK;
        const bool w1 = bq_[j] >= a.Q;
        bq_[j] -= w1 ? a.Q : 0;
        bp_[j] += w1 ? 1 : 0;
        const bool w2 = bp_[j] >= a.P;
        bp_[j] = w2 ? 0 : bp_[j];
        bn_[j] += w2 ? 1 : 0;
        if (a.Q < BK) {
            while (bq_[j] >= a.Q) {
                bq_[j] -= a.Q;
                if (++bp_[j] == a.P) { bp_[j] = 0; ++bn_[j]; }
            }
        }
        }
    };
    auto st_a = [&](int j, int buf) {
        *reinterpret_cast<f32x4 *>(As + buf * A_ELEMS + (a_row + RPP_A * j) * BMW + a_col) = ra[j];
    };
    auto st_b = [&](int j, int buf) {
        *reinterpret_cast<f32x4 *>(Bs + buf * B_ELEMS + (b_row + RPP_B * j) * BN + b_col) = rb[j];
    };
#pragma unroll
    for (int j = 0; j < 4; ++j) { load_a(j, kc_begin); load_b(j); adv_b(j); }
#pragma unroll
    for (int j = 0; j < 4; ++j) { st_a(j, 0); st_b(j, 0); }
#pragma unroll
    for (int j = 0; j < 4; ++j) { load_a(j, kc_begin + 1); load_b(j); adv_b(j); }
    __syncthreads();
    rdg(0, 0, fa0, fb0);
    if constexpr (PIPE == 3) {
    for (int kc = kc_begin; kc < kc_end; ++kc) {
        rdg(0, 1, fa1, fb1);
        sub(fa0, fb0, 0); sub(fa0, fb0, 1); sub(fa0, fb0, 2); sub(fa0, fb0, 3);
        rdg(0, 2, fa0, fb0);
        sub(fa1, fb1, 0); sub(fa1, fb1, 1); sub(fa1, fb1, 2); sub(fa1, fb1, 3);
        rdg(0, 3, fa1, fb1);
        sub(fa0, fb0, 0); sub(fa0, fb0, 1); sub(fa0, fb0, 2); sub(fa0, fb0, 3);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        st_a(0, 0); st_a(1, 0); st_a(2, 0); st_a(3, 0);
        sub(fa1, fb1, 0);
        st_b(0, 0); st_b(1, 0); st_b(2, 0); st_b(3, 0);
        sub(fa1, fb1, 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        rdg(0, 0, fa0, fb0);
        load_a(0, kc + 2); load_a(1, kc + 2); load_a(2, kc + 2); load_a(3, kc + 2);
        sub(fa1, fb1, 2);
        load_b(0); load_b(1); load_b(2); load_b(3);
        adv_b(0); adv_b(1); adv_b(2); adv_b(3);
        sub(fa1, fb1, 3);
    }
    } else {
    for (int kc = kc_begin; kc < kc_end; ++kc) {
        const int buf = (kc - kc_begin) & 1;
        // branch-free body (see conv_igemm_kernel<PIPE>): past the end of this split's K range the loads are
        // out-of-range buffer reads and the stores / fragment reads touch an LDS buffer nobody consumes
        // group 0
        rdg(buf, 1, fa1, fb1);
        sub(fa0, fb0, 0); sub(fa0, fb0, 1); sub(fa0, fb0, 2); sub(fa0, fb0, 3);
        // group 1: stage the next K-step
        rdg(buf, 2, fa0, fb0);
        st_a(0, buf ^ 1); st_a(1, buf ^ 1);
        sub(fa1, fb1, 0);
        st_a(2, buf ^ 1); st_a(3, buf ^ 1);
        sub(fa1, fb1, 1);
        st_b(0, buf ^ 1); st_b(1, buf ^ 1);
        sub(fa1, fb1, 2);
        st_b(2, buf ^ 1); st_b(3, buf ^ 1);
        sub(fa1, fb1, 3);
        // group 2: refill the registers two K-steps ahead
        rdg(buf, 3, fa1, fb1);
        load_a(0, kc + 2); load_a(1, kc + 2);
        sub(fa0, fb0, 0);
        load_a(2, kc + 2); load_a(3, kc + 2);
        sub(fa0, fb0, 1);
        load_b(0); load_b(1);
        sub(fa0, fb0, 2);
        load_b(2); load_b(3);
        sub(fa0, fb0, 3);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        // group 3 overlaps the first fragment reads of the next K-step and the row bookkeeping
        rdg(buf ^ 1, 0, fa0, fb0);
        adv_b(0); adv_b(1);
        sub(fa1, fb1, 0);
        adv_b(2); adv_b(3);
        sub(fa1, fb1, 1);
        sub(fa1, fb1, 2);
        sub(fa1, fb1, 3);
    }
    }
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int c = c0 + (wn * TN + j) * 32 + lr;
        if (c >= a.C) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ko = ko0 + (wm * TM + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (ko < a.K) unsafeAtomicAdd(a.dw + ((long)ko * RS + tap) * a.C + c, acc[i][j][e]);
            }
    }
}

const float *zero_page()
{
    // a __device__ symbol has one instance per device: cache per device id
    static float *p[64] = {};
    int dev = 0;
    hipGetDevice(&dev);
    dev &= 63;
    if (!p[dev]) hipGetSymbolAddress(reinterpret_cast<void **>(&p[dev]), HIP_SYMBOL(rr_zero16));
    return p[dev];
}

// conv_igemm_kernel's dynamic LDS: nbuf images of A [BM][BK + 4] and B [bn][BK + 4] / [BK][bn]
size_t igemm_lds(int bn, bool b_kn, int nbuf)
{
    return sizeof(float) * nbuf * (BM * (BK + 4) + (b_kn ? BK * bn : bn * (BK + 4)));
}

// column sums / sums of squares of y -> slab row 0 (the other rows are zeroed by the caller); used when
// split-K keeps the statistics out of the conv epilogue.  Thread = (pixel lane, channel quad), LDS reduce
// over the pixel lanes, one double atomic per channel per workgroup.
__global__ __launch_bounds__(256) void colstats_kernel(const float *y, long M, int C, double *slab)
{
    __shared__ double red[2][256 * 4];
    const int C4 = C / 4, lanes = 256 / C4;
    const int t = threadIdx.x, cq = t % C4, pl = t / C4;
    double s1[4] = {0, 0, 0, 0}, s2[4] = {0, 0, 0, 0};
    if (pl < lanes)
        for (long p = (long)blockIdx.x * lanes + pl; p < M; p += (long)gridDim.x * lanes) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(y + p * C + cq * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { s1[e] += (double)v[e]; s2[e] += (double)v[e] * (double)v[e]; }
        }
#pragma unroll
    for (int e = 0; e < 4; ++e) { red[0][t * 4 + e] = s1[e]; red[1][t * 4 + e] = s2[e]; }
    __syncthreads();
    for (int c = t; c < C; c += 256) {
        double a1 = 0.0, a2 = 0.0;
        for (int l = 0; l < lanes; ++l) {
            a1 += red[0][(l * C4 + c / 4) * 4 + (c & 3)];
            a2 += red[1][(l * C4 + c / 4) * 4 + (c & 3)];
        }
        unsafeAtomicAdd(slab + c, a1);
        unsafeAtomicAdd(slab + C + c, a2);
    }
}

// PIPE 2 (pipelined, one LDS image) where both tensors are below 2 GiB: it addresses them through 32-bit buffer offsets
template <int MODE>
int launch_igemm(ConvArgs &a, int bn, bool scalar, int blocks, int gy, int gz, hipStream_t stream, const char *name)
{
    const bool small = (long)a.N * a.SH * a.SW * a.SC * 4 < (1l << 31) && (long)a.wK * a.R * a.S * a.wC * 4 < (1l << 31);
    a.dst32 = (long)a.M * a.DC * 4 < (1l << 31);
#define IG(BNv, SCv, PIPEv, ...)                                                                                       \
    rr_launch(conv_igemm_kernel<BNv, MODE, SCv, BK, PIPEv, ##__VA_ARGS__>, dim3(blocks, gy, gz), 256,                  \
              igemm_lds(bn, MODE == 1, PIPEv == 2 ? 1 : 2), stream, a, name)
    if constexpr (MODE == 0) {
        if (a.pos_major)             // host rule (fprop_impl): vector gather, both tensors below 2 GiB
            return bn == 128 ? IG(128, false, 2, false, true) : IG(64, false, 2, false, true);
        if (a.bs_y != nullptr) {     // producer's BatchNorm-backward sums in the epilogue: vector kernels
            RR_CHECK_ARG(!scalar, "conv: BatchNorm-backward sums need the vector kernels (C %% 4 == 0)");
            if (bn == 128) return small ? IG(128, false, 2, true) : IG(128, false, 0, true);
            if (bn == 64) return small ? IG(64, false, 2, true) : IG(64, false, 0, true);
            return IG(32, false, 0, true);
        }
    }
    if (bn == 128) {
        if (scalar) return IG(128, true, 0);
        return small ? IG(128, false, 2) : IG(128, false, 0);
    }
    if (bn == 64)     // 4 waves along M, 32x64 each: 33..64-column layers and under-filled 384-column levels
        return small ? IG(64, false, 2) : IG(64, false, 0);
    return scalar ? IG(32, true, 0) : IG(32, false, 0);
#undef IG
}

}  // namespace

extern "C" size_t rr_conv_stat_slab_bytes(int n, int p, int q, int k)
{
    const long M = (long)n * p * q;
    return (size_t)((M + BM - 1) / BM) * 2 * k * sizeof(double);
}

// The sixteen GEMMs of the Winograd route in one launch: m[i][t][ko] = sum_c v[i][t][c] * u[i][ko][c], i = blockIdx.y — the plain
// pipelined forward kernel at 1x1 geometry (one "image" of T pixels), plain stores.  The caller (rr_plan::wino_plan) keeps every
// slice below 2 GiB.
int rr_conv_wino_gemm(const float *v, const float *u, float *m, long tiles, int c, int k, hipStream_t stream, const char *name)
{
    RR_CHECK_ARG(tiles > 0 && c > 0 && k > 0 && c % 4 == 0 && k % 4 == 0 && tiles * c * 4 < (1l << 31) && tiles * k * 4 < (1l << 31)
                 && (long)k * c * 4 < (1l << 31), "%s: bad GEMM geometry", name);
    ConvArgs a{};
    a.src = v; a.w = u; a.dst = m; a.zero = zero_page();
    a.N = 1; a.SH = 1; a.SW = (int)tiles; a.SC = c;
    a.DH = 1; a.DW = (int)tiles; a.DC = k;
    a.R = 1; a.S = 1; a.stride = 1; a.ksplit = 1;
    a.M = (int)tiles; a.Kg = c; a.wK = k; a.wC = c; a.dst32 = 1;
    a.batch_src = tiles * c; a.batch_w = (long)k * c; a.batch_dst = tiles * k;
    const int bn = k > 64 ? 128 : 64;
    const dim3 grid(rr_cdiv(tiles, BM) * rr_cdiv(k, bn), 16, 1);
    if (bn == 128)
        return rr_launch(conv_igemm_kernel<128, 0, false, BK, 2, false, false, true>, grid, 256, igemm_lds(128, false, 1), stream, a, name);
    return rr_launch(conv_igemm_kernel<64, 0, false, BK, 2, false, false, true>, grid, 256, igemm_lds(64, false, 1), stream, a, name);
}

// The sixteen GEMMs of the Winograd weight gradient in one launch: s[ko][i][c] += sum_t w[i][t][ko] * v[i][t][c] — the pipelined
// weight-gradient kernel in batch mode, float atomics into s (zeroed by the caller).  rr_plan::wino_wgrad_gemm_plan sizes the launch.
int rr_conv_wino_wgrad_gemm(const float *v, const float *w, float *s, long tiles, int c, int k, hipStream_t stream, const char *name)
{
    RR_CHECK_ARG(tiles > 0 && c > 32 && k > 32 && c % 4 == 0 && k % 4 == 0 && tiles * c * 4 < (1l << 31) && tiles * k * 4 < (1l << 31)
                 && 16l * k * c * 4 < (1l << 31), "%s: bad GEMM geometry", name);
    const rr_plan::WinoWgradGemm pl = rr_plan::wino_wgrad_gemm_plan(tiles, c, k);
    WgradArgs a{};
    a.x = v; a.dy = w; a.dw = s; a.zero = zero_page();
    a.N = 1; a.H = 1; a.W = (int)tiles; a.C = c; a.K = k; a.R = 1; a.S = 1;
    a.P = 1; a.Q = (int)tiles; a.stride = 1;
    a.M = (int)tiles; a.mt = pl.mt; a.nt = pl.nt; a.chunks_per_split = pl.per_split;
    a.slice_x = tiles * c; a.slice_dy = tiles * k;
    if (pl.pipe == 3) return rr_launch(conv_wgrad_kernel<128, 128, false, false, 3, true>, dim3(pl.grid), 256, pl.lds, stream, a, name);
    return rr_launch(conv_wgrad_kernel<128, 128, false, false, 1, true>, dim3(pl.grid), 256, pl.lds, stream, a, name);
}

int rr_conv_colstats(const float *y, long M, int C, double *slab, hipStream_t stream, const char *name)
{
    const int lanes = 256 / (C / 4);
    int sblocks = rr_cdiv(M, (long)lanes * 8);
    if (sblocks > 256) sblocks = 256;
    hipLaunchKernelGGL(colstats_kernel, dim3(sblocks), dim3(256), 0, stream, y, M, C, slab);
    RR_CHECK_LAUNCH(name);
    return RR_OK;
}

// name: the public entry point that was called.  How the call launches is rr_plan::fprop_plan's decision (conv_plan.h).
static int fprop_impl(const char *name, const float *x, const float *w, const float *bias, float *y, double *stat_slab,
                      int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h,
                      int pad_w, int relu, int accumulate, hipStream_t stream, const BnSumArgs *bs = nullptr, const int *gate = nullptr,
                      int gate_max = 0)
{
    const rr_plan::FpropPlan pl = rr_plan::fprop_plan(rr_plan::MATH_F32, {n, h, wd, c, k, r, s, stride, pad_h, pad_w, 0, 0},
                                                      {bias != nullptr, relu != 0, stat_slab != nullptr, rr_conv_link(bs), accumulate != 0, false});
    RR_CHECK_ARG(pl.refuse == nullptr, "%s: %s", name, pl.refuse);
    // a gated launch is the plain forward kernel and nothing else: no other kernel family, no producer link, and its split-K zero
    // fill on the same side of the gate as itself
    RR_CHECK_ARG(gate == nullptr || (!pl.rows && !pl.pos_major && bs == nullptr && pl.after == rr_plan::AFTER_NONE && !pl.zero_slab),
                 "%s: this shape does not launch the plain forward kernel alone: no gate", name);
    if (pl.rows) return rr_conv1x1_rows(x, w, bias, y, pl.M, c, k, relu, stream);
    ConvArgs a{};
    a.gate = gate; a.gate_max = gate_max;
    a.src = x; a.w = w; a.dst = y; a.bias = bias; a.stat_slab = stat_slab;
    a.N = n; a.SH = h; a.SW = wd; a.SC = c;
    a.DH = pl.dh; a.DW = pl.dw; a.DC = k;
    a.R = r; a.S = s; a.stride = stride; a.pad_h = pad_h; a.pad_w = pad_w;
    a.relu = relu; a.accumulate = accumulate; a.ksplit = pl.ks; a.pos_major = pl.pos_major; a.zero = zero_page();
    a.M = (int)pl.M; a.Kg = r * s * c; a.wK = k; a.wC = c;
    if (pl.fused) bs->into(a);
    if (gate != nullptr && pl.zero_dst) {
        if (int rc = rr_gated_zero(y, sizeof(float) * (size_t)pl.M * k, gate, gate_max, 0, stream, name)) return rc;
    } else if (int rc = rr_conv_before_launch(pl, n, k, y, stat_slab, stream, name)) return rc;
    if (int rc = launch_igemm<0>(a, pl.bn, pl.scalar, pl.blocks, 1, pl.ks, stream, name)) return rc;
    return rr_conv_after_launch(pl, bs, k, y, stat_slab, stream, name);
}

extern "C" int rr_conv_fprop(const float *x, const float *w, const float *bias, float *y, double *stat_slab,
                             int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h,
                             int pad_w, int relu, hipStream_t stream)
{
    return fprop_impl("rr_conv_fprop", x, w, bias, y, stat_slab, n, h, wd, c, k, r, s, stride, pad_h, pad_w, relu, 0, stream);
}

// wt[c][R-1-r][S-1-s][k] = w[k][r][s][c]: 32x32 tiles of the (k, c) plane through LDS, one tap per grid.z
__global__ __launch_bounds__(256) void weight_flip_transpose_kernel(const float *w, float *wt, int K, int C, int RS)
{
    __shared__ float tile[32][33];
    const int tap = blockIdx.z, k0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int k = k0 + i, c = c0 + tx;
        tile[i][tx] = (k < K && c < C) ? w[((long)k * RS + tap) * C + c] : 0.f;
    }
    __syncthreads();
    const int ftap = RS - 1 - tap;   // (R-1-r)*S + (S-1-s)
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, k = k0 + tx;
        if (k < K && c < C) wt[((long)c * RS + ftap) * K + k] = tile[tx][i];
    }
}

extern "C" int rr_weight_flip_transpose(const float *w, float *wt, int k, int c, int r, int s, hipStream_t stream)
{
    RR_CHECK_ARG(k > 0 && c > 0 && r > 0 && s > 0 && r * s < 65536, "rr_weight_flip_transpose: bad dims");
    hipLaunchKernelGGL(weight_flip_transpose_kernel, dim3(rr_cdiv(c, 32), rr_cdiv(k, 32), r * s), dim3(256), 0, stream, w, wt,
                       k, c, r * s);
    RR_CHECK_LAUNCH("rr_weight_flip_transpose");
    return RR_OK;
}

// All filters of a model in one launch: `table` holds one int4 per 32 x 32 tile {element offset of the filter in the flat
// buffers, K, C, packed (tap << 20 | k-tile << 10 | c-tile)} (built once by the host layer, rrnet_amd/flat.py); the
// flipped / transposed copy lands at the SAME offset of `wt_flat`.  Replaces one tiny launch per layer and step on the
// critical path of backward (73 in the headline step, 153 with bf16 stride-1 data gradients at every size).
__global__ __launch_bounds__(256) void weight_flip_transpose_batch_kernel(const float *flat, float *wt_flat, const int4 *table,
                                                                          unsigned short *w16_flat, unsigned short *wt16_flat)
{
    __shared__ float tile[32][33];
    const int4 d = table[blockIdx.x];
    const int K = d.y, C = d.z;
    const int tap = d.w >> 20, k0 = ((d.w >> 10) & 1023) * 32, c0 = (d.w & 1023) * 32;
    const float *w = flat + d.x;
    float *wt = wt_flat + d.x;
    // RS travels in the top bits of K (filters have <= 4096 output channels): K = RS << 16 | K
    const int RS = K >> 16, Kk = K & 0xffff;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int k = k0 + i, c = c0 + tx;
        const bool in = k < Kk && c < C;
        const float v = in ? w[((long)k * RS + tap) * C + c] : 0.f;
        tile[i][tx] = v;
        if (in && w16_flat) w16_flat[d.x + ((long)k * RS + tap) * C + c] = __builtin_bit_cast(unsigned short, (__bf16)v);
    }
    __syncthreads();
    const int ftap = RS - 1 - tap;
    for (int i = ty; i < 32; i += 8) {
        const int c = c0 + i, k = k0 + tx;
        if (k < Kk && c < C) {
            const float v = tile[tx][i];
            wt[((long)c * RS + ftap) * Kk + k] = v;
            if (wt16_flat) wt16_flat[d.x + ((long)c * RS + ftap) * Kk + k] = __builtin_bit_cast(unsigned short, (__bf16)v);
        }
    }
}

extern "C" int rr_weight_flip_transpose_batch(const float *flat, float *wt_flat, const int *table, int ntiles, hipStream_t stream)
{
    RR_CHECK_ARG(flat && wt_flat && table && ntiles >= 0, "rr_weight_flip_transpose_batch: null argument");
    if (ntiles == 0) return RR_OK;
    hipLaunchKernelGGL(weight_flip_transpose_batch_kernel, dim3(ntiles), dim3(256), 0, stream, flat, wt_flat,
                       reinterpret_cast<const int4 *>(table), (unsigned short *)nullptr, (unsigned short *)nullptr);
    RR_CHECK_LAUNCH("rr_weight_flip_transpose_batch");
    return RR_OK;
}

extern "C" int rr_weight_flip_transpose_batch_bf16(const float *flat, float *wt_flat, unsigned short *w16_flat,
                                                   unsigned short *wt16_flat, const int *table, int ntiles, hipStream_t stream)
{
    RR_CHECK_ARG(flat && wt_flat && table && ntiles >= 0, "rr_weight_flip_transpose_batch_bf16: null argument");
    if (ntiles == 0) return RR_OK;
    hipLaunchKernelGGL(weight_flip_transpose_batch_kernel, dim3(ntiles), dim3(256), 0, stream, flat, wt_flat,
                       reinterpret_cast<const int4 *>(table), w16_flat, wt16_flat);
    RR_CHECK_LAUNCH("rr_weight_flip_transpose_batch_bf16");
    return RR_OK;
}

// the stride-1 data gradients: rr_dgrad_s1_geom's checks and flip (conv_launch.h), then the forward kernel on (dy, wt)
static int dgrad_s1(const char *name, bool producer_ok, const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                    int r, int s, int pad_h, int pad_w, int accumulate, hipStream_t stream, const BnSumArgs *bs = nullptr, const int *gate = nullptr,
                    int gate_max = 0)
{
    DgradS1Geom g;
    if (int rc = rr_dgrad_s1_geom(name, h, wd, r, s, pad_h, pad_w, producer_ok, &g)) return rc;
    return fprop_impl(name, dy, wt, nullptr, dx, nullptr, n, g.p, g.q, k, c, r, s, 1, g.pad_h, g.pad_w, 0, accumulate, stream, bs, gate, gate_max);
}

extern "C" int rr_conv_dgrad_s1(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                                int r, int s, int pad_h, int pad_w, int accumulate, hipStream_t stream)
{
    return dgrad_s1("rr_conv_dgrad_s1", true, dy, wt, dx, n, h, wd, c, k, r, s, pad_h, pad_w, accumulate, stream);
}

// the dense side of the rows route's gate (conv_rows.hip): rr_conv_dgrad_s1, returning at once when *count <= max_rows
extern "C" int rr_conv_dgrad_s1_unless(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k, int r, int s,
                                       int pad_h, int pad_w, int accumulate, const int *count, int max_rows, hipStream_t stream)
{
    RR_CHECK_ARG(count != nullptr && c % 4 == 0 && k % 4 == 0, "rr_conv_dgrad_s1_unless: a count, C and K multiples of 4");
    return dgrad_s1("rr_conv_dgrad_s1_unless", true, dy, wt, dx, n, h, wd, c, k, r, s, pad_h, pad_w, accumulate, stream, nullptr, count, max_rows);
}

// out[m][k], m = (n,p,q), k = (r*S + s)*C + c for k < R*S*C and 0 up to KP: the taps of a small-channel convolution laid
// out as one row per output pixel, so that the 7x7 stride-2 stem (C = 3: 147 -> KP = 160) becomes a 1x1 convolution on the
// vector kernels (fprop) and a 128 x KP weight-gradient GEMM over all pixels (wgrad) instead of the scalar-gather paths.
// One thread = one output float4; HBM-bound on the writes (the reads hit L2: every input pixel is wanted R*S/stride^2 times).
__global__ __launch_bounds__(256) void conv_pack_taps_kernel(const float *x, f32x4 *out, int H, int W, int C, int S, int stride,
                                                             int pad_h, int pad_w, int P, int Q, int KP4, int Kg, long total)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int k4 = (int)(i % KP4);
        long m = i / KP4;
        const int q = (int)(m % Q); m /= Q;
        const int p = (int)(m % P);
        const long n = m / P;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int k = k4 * 4 + e;
            if (k < Kg) {
                const int tap = k / C, c = k - tap * C;
                const int r = tap / S, sx = tap - r * S;
                const int ih = p * stride - pad_h + r, iw = q * stride - pad_w + sx;
                if ((unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) v[e] = x[((n * H + ih) * W + iw) * C + c];
            }
        }
        out[i] = v;
    }
}

extern "C" int rr_conv_pack_taps(const float *x, float *out, int n, int h, int wd, int c, int r, int s, int stride, int pad_h,
                                 int pad_w, int kp, hipStream_t stream)
{
    RR_CHECK_ARG(n > 0 && h > 0 && wd > 0 && c > 0 && r > 0 && s > 0 && stride > 0 && kp % 4 == 0 && kp >= r * s * c,
                 "rr_conv_pack_taps: bad dims (kp must be a multiple of 4 and >= r*s*c)");
    const int p = (h + 2 * pad_h - r) / stride + 1, q = (wd + 2 * pad_w - s) / stride + 1;
    RR_CHECK_ARG(p > 0 && q > 0, "rr_conv_pack_taps: empty output");
    const long total = (long)n * p * q * (kp / 4);
    long blocks = (total + 255) / 256;
    if (blocks > 256 * 64) blocks = 256 * 64;
    hipLaunchKernelGGL(conv_pack_taps_kernel, dim3((int)blocks), dim3(256), 0, stream, x, reinterpret_cast<f32x4 *>(out), h, wd, c,
                       s, stride, pad_h, pad_w, p, q, kp / 4, r * s * c, total);
    RR_CHECK_LAUNCH("rr_conv_pack_taps");
    return RR_OK;
}

extern "C" int rr_conv_dgrad_s1_bnsum(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                                      int r, int s, int pad_h, int pad_w, int accumulate, const float *prod_y,
                                      const float *prod_z, const float *prod_mean, const float *prod_invstd,
                                      const float *prod_mask_scale, const float *prod_mask_shift, double *slab,
                                      double *sums, hipStream_t stream)
{
    const BnSumArgs bs{prod_y, prod_z, prod_mean, prod_invstd, prod_mask_scale, prod_mask_shift, slab, sums, 0};
    return dgrad_s1("rr_conv_dgrad_s1_bnsum", bs.bn_ok(c), dy, wt, dx, n, h, wd, c, k, r, s, pad_h, pad_w, accumulate, stream, &bs);
}

extern "C" int rr_conv_dgrad_s1_relubias(const float *dy, const float *wt, float *dx, int n, int h, int wd, int c, int k,
                                         int r, int s, int pad_h, int pad_w, int accumulate, const float *prod_z, double *slab,
                                         double *sums, hipStream_t stream)
{
    const BnSumArgs bs{prod_z, prod_z, nullptr, nullptr, nullptr, nullptr, slab, sums, 1};
    return dgrad_s1("rr_conv_dgrad_s1_relubias", bs.relu_bias_ok(c, k), dy, wt, dx, n, h, wd, c, k, r, s, pad_h, pad_w, accumulate, stream, &bs);
}

// How these two launch is rr_plan::dgrad_plan's and rr_plan::wgrad_plan's decision (conv_plan.h).
extern "C" int rr_conv_dgrad(const float *dy, const float *w, float *dx, int n, int h, int wd, int c, int k,
                             int r, int s, int stride, int pad_h, int pad_w, int accumulate,
                             hipStream_t stream)
{
    const rr_plan::DgradPlan pl = rr_plan::dgrad_plan({n, h, wd, c, k, r, s, stride, pad_h, pad_w, 0, 0}, accumulate != 0);
    if (pl.refuse.why) return rr_refuse("rr_conv_dgrad", pl.refuse);
    ConvArgs a{};
    a.src = dy; a.w = w; a.dst = dx; a.bias = nullptr; a.stat_slab = nullptr;
    a.N = n;
    a.SH = (h + 2 * pad_h - r) / stride + 1; a.SW = (wd + 2 * pad_w - s) / stride + 1; a.SC = k;
    a.DH = h; a.DW = wd; a.DC = c;
    a.R = r; a.S = s; a.stride = stride; a.pad_h = pad_h; a.pad_w = pad_w;
    a.relu = 0; a.accumulate = accumulate; a.ksplit = pl.ks; a.zero = zero_page();
    a.parity = pl.parity; a.parity_order = pl.parity_order;
    a.M = (int)pl.M; a.Kg = r * s * k; a.wK = k; a.wC = c;
    if (pl.zero_dst) RR_CHECK_HIP(rr_zero2(dx, sizeof(float) * (size_t)pl.M * c, nullptr, 0, stream), "rr_conv_dgrad");
    return launch_igemm<1>(a, pl.bn, pl.scalar, pl.blocks, pl.gy, pl.ks, stream, "rr_conv_dgrad");
}

static int wgrad_impl(const char *name, const float *x, const float *dy, float *dw, int n, int h, int wd, int c, int k, int r, int s,
                      int stride, int pad_h, int pad_w, int out_h, int out_w, hipStream_t stream, const int *gate, int gate_max)
{
    const rr_plan::WgradPlan pl = rr_plan::wgrad_plan(rr_plan::MATH_F32, {n, h, wd, c, k, r, s, stride, pad_h, pad_w, out_h, out_w});
    if (pl.refuse.why) return rr_refuse(name, pl.refuse);
    WgradArgs a{};
    a.x = x; a.dy = dy; a.dw = dw; a.zero = zero_page(); a.gate = gate; a.gate_max = gate_max;
    a.N = n; a.H = h; a.W = wd; a.C = c; a.K = k; a.R = r; a.S = s;
    a.P = pl.P; a.Q = pl.Q;
    a.stride = stride; a.pad_h = pad_h; a.pad_w = pad_w;
    a.M = (int)pl.M; a.mt = pl.mt; a.nt = pl.nt; a.chunks_per_split = pl.per_split;
#define WG(BMv, BNv, ASv, BSv, PIPEv) rr_launch(conv_wgrad_kernel<BMv, BNv, ASv, BSv, PIPEv>, dim3(pl.grid), 256, pl.lds, stream, a, name)
#define WG_AB(BMv, BNv) (pl.a_scalar ? (pl.b_scalar ? WG(BMv, BNv, true, true, 0) : WG(BMv, BNv, true, false, 0))         \
                                     : (pl.b_scalar ? WG(BMv, BNv, false, true, 0) : WG(BMv, BNv, false, false, 0)))
    if (pl.pipe == 3) return WG(128, 128, false, false, 3);
    if (pl.pipe == 1) return WG(128, 128, false, false, 1);
    if (pl.bm == 128) return pl.bn == 128 ? WG_AB(128, 128) : WG_AB(128, 32);
    return pl.bn == 128 ? WG_AB(32, 128) : WG_AB(32, 32);
#undef WG
#undef WG_AB
}

extern "C" int rr_conv_wgrad(const float *x, const float *dy, float *dw, int n, int h, int wd, int c, int k,
                             int r, int s, int stride, int pad_h, int pad_w, int out_h, int out_w,
                             hipStream_t stream)
{
    return wgrad_impl("rr_conv_wgrad", x, dy, dw, n, h, wd, c, k, r, s, stride, pad_h, pad_w, out_h, out_w, stream, nullptr, 0);
}

// the dense side of the rows route's gate: rr_conv_wgrad at stride 1, returning at once when *count <= max_rows
extern "C" int rr_conv_wgrad_unless(const float *x, const float *dy, float *dw, int n, int h, int wd, int c, int k, int r, int s,
                                    int pad_h, int pad_w, const int *count, int max_rows, hipStream_t stream)
{
    RR_CHECK_ARG(count != nullptr, "rr_conv_wgrad_unless: a count");
    return wgrad_impl("rr_conv_wgrad_unless", x, dy, dw, n, h, wd, c, k, r, s, 1, pad_h, pad_w, 0, 0, stream, count, max_rows);
}

// the policy of conv_plan.h as the library was built with it, for tests/test_host_logic.py (C++ linkage, called by mangled name)
int rr_conv_pick_ksplit(int blocks, int nk) { return rr_plan::pick_ksplit(blocks, nk); }
int rr_conv_small_tiles() { return rr_plan::small_tiles(); }
int rr_conv_mid_tiles() { return rr_plan::mid_tiles(); }

extern "C" int rr_conv_fprop_plan(int math, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w,
                                  int out_h, int out_w, int flags, int *plan)
{
    RR_CHECK_ARG(math >= rr_plan::MATH_F32 && math <= rr_plan::MATH_F16X3 && ((flags >> 8) & 3) <= rr_plan::LINK_RELU_BIAS && plan != nullptr,
                 "rr_conv_fprop_plan: bad arguments");
    const rr_plan::FpropPlan pl = rr_plan::fprop_plan(math, {n, h, wd, c, k, r, s, stride, pad_h, pad_w, out_h, out_w},
                                                      {(flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags >> 8) & 3, (flags & 8) != 0,
                                                       (flags & 16) != 0});
    RR_CHECK_ARG(pl.refuse == nullptr, "rr_conv_fprop_plan: %s", pl.refuse);
    const int out[RR_CONV_PLAN_INTS] = {pl.rows, pl.scalar, pl.bn, pl.blocks, pl.ks, pl.pos_major, pl.xcd_n, pl.fused, pl.after, pl.zero_dst,
                                        pl.zero_slab};
    for (int i = 0; i < RR_CONV_PLAN_INTS; ++i) plan[i] = out[i];
    return RR_OK;
}

// the gradient plans of conv_plan.h as the entry points of conv.hip, conv_bf16.hip and conv16.hip ask them
extern "C" int rr_conv_grad_plan(int pass, int family, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w,
                                 int out_h, int out_w, int accumulate, int *out, int n_out)
{
    using namespace rr_plan;
    const bool family_ok = pass == GRAD_DGRAD ? family == MATH_F32 : pass == GRAD_DGRAD_S2 ? (family >= MATH_BF16 && family <= FAM_CONV16)
                                                                                          : (family >= MATH_F32 && family <= FAM_CONV16);
    RR_CHECK_ARG(pass >= GRAD_DGRAD && pass <= GRAD_WGRAD && family_ok && out != nullptr && n_out >= RR_CONV_GRAD_PLAN_INTS,
                 "rr_conv_grad_plan: bad arguments");
    const ConvGeom g{n, h, wd, c, k, r, s, stride, pad_h, pad_w, out_h, out_w};
    for (int i = 0; i < n_out; ++i) out[i] = 0;
    if (pass == GRAD_DGRAD) {
        const DgradPlan p = dgrad_plan(g, accumulate != 0);
        if (p.refuse.why) return rr_refuse("rr_conv_grad_plan", p.refuse);
        const int f[8] = {p.scalar, p.bn, p.blocks, p.gy, p.parity, p.parity_order, p.ks, p.zero_dst};
        for (int i = 0; i < 8; ++i) out[i] = f[i];
    } else if (pass == GRAD_DGRAD_S2) {
        const DgradS2Plan p = dgrad_s2_plan(family, g, accumulate != 0);
        if (p.refuse.why) return rr_refuse("rr_conv_grad_plan", p.refuse);
        out[0] = p.p; out[1] = p.q; out[2] = p.zero_dst; out[3] = p.n_launch;
        for (int i = 0; i < p.n_launch; ++i) {
            const ParityClass &pc = p.cls[i];
            const int f[10] = {pc.ph, pc.pw, pc.Rc, pc.Sc, pc.lead_h, pc.lead_w, pc.Hc, pc.Wc, pc.taps_before, p.blocks[i]};
            for (int j = 0; j < 10; ++j) out[4 + 10 * i + j] = f[j];
        }
    } else {
        const WgradPlan p = wgrad_plan(family, g);
        if (p.refuse.why) return rr_refuse("rr_conv_grad_plan", p.refuse);
        const int f[15] = {p.P, p.Q, (int)p.M, p.bm, p.bn, p.a_scalar, p.b_scalar, p.pipe, p.mt, p.nt, p.tiles, p.splits, p.per_split, p.grid, p.lds};
        for (int i = 0; i < 15; ++i) out[i] = f[i];
    }
    return RR_OK;
}
