// The "rows" route of a convolution's two gradients: the work of the pixels whose incoming gradient row is not all zero.
//
// The wh and offset heads are trained through RegL1Loss, which gathers its prediction at the objects' centres and nowhere
// else (losses.hip, regl1_bwd_kernel): the gradient that reaches a head's 3x3 conv + bias + ReLU layer is non-zero on a few
// hundred to a few ten thousand of the 524 288 pixels of the headline step.  The dense kernels of conv.hip multiply the
// zeros; here a list of the active pixels is made once (rr_active_rows) and
//   dgrad : dX[t_j][c] = sum_{tap,ko} dY[t_j - tap][ko] * W[ko][tap][c]    for the dx pixels t_j a listed dy pixel reaches (rr_active_targets)
//   wgrad : dW[ko][tap][c]       += sum_i  dY[p_i][ko] * X[pix(p_i, tap)][c]   GEMM  K x count  by  count x C, per tap
// with pix(p, tap) = p + (r - pad_h, s - pad_w), the input pixel the forward pass read for output pixel p through tap (r, s).
// W is read in its own OHWI layout.  fp32 MFMA (v_mfma_f32_32x32x2_f32), one LDS image per operand, registers one K-step
// ahead: these launches are short, peak rate is not their point.
//
// The gate.  Whether the list is short is known on the device only.  Every kernel here starts with
// `*count > max_rows -> return`, the dense kernels of conv.hip launched through the _unless entry points with the opposite
// test: the host enqueues both, exactly one of the two does the work, nothing is read back.  Grids are sized for max_rows;
// workgroups past the count leave at once.  No workgroup waits for another.
// The data gradient has no atomics and one owner per element: like the dense kernel it is bit-reproducible from run to run.
#include "conv_launch.h"
#include "rowkit.h"
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------------
// rr_active_rows: two launches, one pass over dy.  Pass 1: a workgroup looks at ROWS_PER_WG consecutive rows (one
// contiguous span of memory), leaves their keep bits (8 words) and its count in `work`.  Pass 2: a workgroup sums the
// counts in front of it and writes its rows at that offset in ascending order (rowkit's ordered rank, from the bits).
constexpr int ROWS_PER_WG = 256;

__global__ __launch_bounds__(256) void active_rows_flag_kernel(const float *dy, int m, int k, int nwg, int *work)
{
    __shared__ int flag[ROWS_PER_WG];
    __shared__ int wave_cnt[4];
    const int t = threadIdx.x, row0 = blockIdx.x * ROWS_PER_WG;
    const int nrows = m - row0 < ROWS_PER_WG ? m - row0 : ROWS_PER_WG;
    flag[t] = 0;
    __syncthreads();
    const float *src = dy + (long)row0 * k;        // 256 * k * 4 bytes per workgroup: 16-byte aligned
    const int n = nrows * k, n4 = n / 4;
    for (int i = t; i < n4; i += 256) {
        const f32x4 v = reinterpret_cast<const f32x4 *>(src)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (v[e] != 0.f) flag[(i * 4 + e) / k] = 1;       // (+-0 is zero, NaN and Inf are not)
    }
    for (int i = n4 * 4 + t; i < n; i += 256)
        if (src[i] != 0.f) flag[i / k] = 1;
    __syncthreads();
    const bool keep = flag[t] != 0;
    const unsigned long long bits = __ballot(keep);
    int total;
    rr_block_rank<4>(keep, wave_cnt, total);
    if ((t & 63) == 0) {
        work[nwg + blockIdx.x * 8 + (t >> 6) * 2 + 0] = (int)(unsigned)bits;
        work[nwg + blockIdx.x * 8 + (t >> 6) * 2 + 1] = (int)(unsigned)(bits >> 32);
    }
    if (t == 0) work[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void active_rows_emit_kernel(const int *work, int nwg, int *rows, int *count)
{
    __shared__ int part[4];
    __shared__ int wave_cnt[4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    int before = 0;
    for (int j = t; j < (int)blockIdx.x; j += 256) before += work[j];
    before = wave_sum_i(before);
    if (lane == 0) part[wave] = before;
    __syncthreads();
    before = part[0] + part[1] + part[2] + part[3];
    const unsigned lo = (unsigned)work[nwg + blockIdx.x * 8 + wave * 2], hi = (unsigned)work[nwg + blockIdx.x * 8 + wave * 2 + 1];
    const bool keep = ((((unsigned long long)hi << 32) | lo) >> lane) & 1ull;
    int total;
    const int rank = rr_block_rank<4>(keep, wave_cnt, total);
    if (keep) rows[before + rank] = blockIdx.x * ROWS_PER_WG + t;       // before + total <= m: every kept row is a row
    if (blockIdx.x == (unsigned)nwg - 1 && t == 0) *count = before + total;
}

// ---------------------------------------------------------------------------------------------
struct RowsArgs {
    const float *dy;   // [N,P,Q,K]
    const float *w;    // [K][R][S][C]
    const float *x;    // wgrad: [N,H,W,C]
    float *dst;        // dgrad: dX [N,H,W,C]; wgrad: dW [K][R][S][C]; float atomics
    const int *rows;   // ascending pixel indices into dy's N*P*Q
    const int *count;
    int max_rows;
    int N, H, W, C, K, R, S, P, Q, pad_h, pad_w;
    int M;             // N*P*Q
    int mt, nt;        // wgrad: tiles along K and C
};

// row i of the list -> its dy pixel and the x / dx pixel seen through tap (r, s); -1 where there is none
__device__ __forceinline__ void rows_pixel(const RowsArgs &a, int i, int cnt, int r, int s, int &pix, int &tgt)
{
    pix = tgt = -1;
    if (i >= cnt) return;
    const int p = a.rows[i];
    if ((unsigned)p >= (unsigned)a.M) return;      // (not a pixel of dy: a list this library did not make)
    const int pq = a.P * a.Q, n = p / pq, rem = p - n * pq, ph = rem / a.Q;
    const int ih = ph - a.pad_h + r, iw = rem - ph * a.Q - a.pad_w + s;
    pix = p;
    if ((unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W) tgt = (n * a.H + ih) * a.W + iw;
}

constexpr int RBM = rr_plan::ROWS_DGRAD_BM;     // dgrad: listed dx pixels per tile
constexpr int RBN = 128;    // columns per tile (channels)
constexpr int RBK = 32;     // K-step
constexpr int RLDK = RBK + 4;   // [m][k] image, padded for conflict-free ds_read_b128 (as in conv.hip)

// rr_active_targets, pass 1 (pass 2 is active_rows_emit_kernel): pixel t of dx is a target when one of the dy pixels it is fed from,
// p = t + (pad_h - r, pad_w - s), is listed — read from the bit per row that active_rows_flag_kernel left (word i / 32, bit i % 32).
__global__ __launch_bounds__(256) void active_targets_flag_kernel(const int *src_bits, int N, int H, int W, int P, int Q, int R, int S,
                                                                  int pad_h, int pad_w, int nwg, int *work)
{
    __shared__ int wave_cnt[4];
    const int t = threadIdx.x, i = blockIdx.x * ROWS_PER_WG + t;
    bool keep = false;
    if (i < N * H * W) {
        const int hw = H * W, n = i / hw, rem = i - n * hw, ih = rem / W, iw = rem - ih * W;
        for (int r = 0; r < R; ++r) {
            const int ph = ih + pad_h - r;
            if ((unsigned)ph >= (unsigned)P) continue;
            for (int s = 0; s < S; ++s) {
                const int qw = iw + pad_w - s;
                if ((unsigned)qw >= (unsigned)Q) continue;
                const int p = (n * P + ph) * Q + qw;
                keep |= ((unsigned)src_bits[p >> 5] >> (p & 31)) & 1u;
            }
        }
    }
    const unsigned long long bits = __ballot(keep);
    int total;
    rr_block_rank<4>(keep, wave_cnt, total);
    if ((t & 63) == 0) {
        work[nwg + blockIdx.x * 8 + (t >> 6) * 2 + 0] = (int)(unsigned)bits;
        work[nwg + blockIdx.x * 8 + (t >> 6) * 2 + 1] = (int)(unsigned)(bits >> 32);
    }
    if (t == 0) work[blockIdx.x] = total;
}

// The data gradient of the listed dx pixels (a.rows: the targets), gathered: dX[t][c] = sum over taps, ko of dY[t + (pad - r, pad - s)][ko] *
// W[ko][r][s][c], taps outside dy read zero.  Every element of dx has ONE owner and one fixed summation order (tap outer, ko inner): no
// atomics, bit-reproducible like the dense kernel (a scatter from the listed dy pixels would do a ninth of the products, but its float
// atomics make the data gradient — and through the backbone's ill-conditioned levels every gradient upstream — vary from run to run).
// One workgroup: 64 targets x 128 channels; 2 x 2 waves of 32 x 64.  grid = (target tiles, channel tiles).
__global__ __launch_bounds__(256) void conv_dgrad_rows_kernel(const RowsArgs a, int accumulate)
{
    const int cnt = *a.count;
    const int row0 = blockIdx.x * RBM;
    if (cnt > a.max_rows || row0 >= cnt) return;
    __shared__ __align__(16) float As[RBM * RLDK];
    __shared__ __align__(16) float Bs[RBK * RBN];
    __shared__ int stgt[RBM];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 31, lh = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int c0 = blockIdx.y * RBN;
    const int MX = a.N * a.H * a.W;
    if (t < RBM) {
        int tgt = row0 + t < cnt ? a.rows[row0 + t] : -1;
        if ((unsigned)tgt >= (unsigned)MX) tgt = -1;       // (not a pixel of dx: a list this library did not make)
        stgt[t] = tgt;
    }
    __syncthreads();

    const int a_col = (t & 7) * 4, a_row = t >> 3;        // A: 32 rows per pass, 2 passes
    const int b_col = (t & 31) * 4, b_row = t >> 5;       // B: 8 k-rows per pass, 4 passes
    int tn[2], th[2], tw[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int tgt = stgt[a_row + 32 * j];
        const int hw = a.H * a.W;
        tn[j] = tgt < 0 ? -1 : tgt / hw;
        const int rem = tgt < 0 ? 0 : tgt - tn[j] * hw;
        th[j] = rem / a.W; tw[j] = rem - th[j] * a.W;
    }
    const int RS = a.R * a.S;
    const long w_row = (long)RS * a.C;
    const float *b_ptr = c0 + b_col < a.C ? a.w + c0 + b_col : nullptr;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 ra[2], rb[4];
    const int kch = (a.K + RBK - 1) / RBK, steps = RS * kch;
    auto load_tiles = [&](int step) {
        const int tap = step / kch, k0 = (step - tap * kch) * RBK;
        const int r = tap / a.S, s = tap - r * a.S;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int ph = th[j] + a.pad_h - r, qw = tw[j] + a.pad_w - s;
            const bool ok = tn[j] >= 0 && (unsigned)ph < (unsigned)a.P && (unsigned)qw < (unsigned)a.Q && k0 + a_col < a.K;
            ra[j] = ok ? *reinterpret_cast<const f32x4 *>(a.dy + ((long)(tn[j] * a.P + ph) * a.Q + qw) * a.K + k0 + a_col) : zero4;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int ko = k0 + b_row + 8 * j;
            rb[j] = (b_ptr != nullptr && ko < a.K) ? *reinterpret_cast<const f32x4 *>(b_ptr + ko * w_row + (long)tap * a.C) : zero4;
        }
    };

    f32x16 acc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

    load_tiles(0);
    for (int step = 0; step < steps; ++step) {
#pragma unroll
        for (int j = 0; j < 2; ++j) *reinterpret_cast<f32x4 *>(As + (a_row + 32 * j) * RLDK + a_col) = ra[j];
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<f32x4 *>(Bs + (b_row + 8 * j) * RBN + b_col) = rb[j];
        __syncthreads();
        if (step + 1 < steps) load_tiles(step + 1);
#pragma unroll
        for (int kk = 0; kk < RBK / 8; ++kk) {
            const f32x4 fa = *reinterpret_cast<const f32x4 *>(As + (wm * 32 + lr) * RLDK + kk * 8 + lh * 4);
            f32x4 fb[2];
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) fb[j][e] = Bs[(kk * 8 + lh * 4 + e) * RBN + (wn * 2 + j) * 32 + lr];
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[e], fb[j][e], acc[j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = c0 + (wn * 2 + j) * 32 + lr;
        if (c >= a.C) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int tgt = stgt[wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh];
            if (tgt < 0) continue;
            float *p = a.dst + (long)tgt * a.C + c;          // the targets are distinct: this thread alone writes the element
            *p = accumulate ? *p + acc[j][e] : acc[j][e];
        }
    }
}

// One workgroup: 128 filters x 128 channels of one tap over a slice of the list; 2 x 2 waves of 64 x 64.  The slices are cut
// on the device from the count (equal shares of its 32-row chunks, never fewer than WROWS_MIN_CHUNKS) over the splits the
// grid was sized with; a slice past the end leaves.  grid = taps * channel tiles * filter tiles * splits.
constexpr int WROWS_MIN_CHUNKS = rr_plan::ROWS_WGRAD_MIN_CHUNKS;

__global__ __launch_bounds__(256) void conv_wgrad_rows_kernel(const RowsArgs a)
{
    const int cnt = *a.count;
    if (cnt > a.max_rows || cnt <= 0) return;
    const int RS = a.R * a.S;
    int id = blockIdx.x;
    const int tap = id % RS; id /= RS;
    const int n_tile = id % a.nt; id /= a.nt;
    const int m_tile = id % a.mt;
    const int split = id / a.mt, splits = gridDim.x / (RS * a.nt * a.mt);
    const int chunks = (cnt + RBK - 1) / RBK;
    int per = (chunks + splits - 1) / splits;
    if (per < WROWS_MIN_CHUNKS) per = WROWS_MIN_CHUNKS;
    const int kc0 = split * per, kc1 = kc0 + per < chunks ? kc0 + per : chunks;
    if (kc0 >= kc1) return;
    __shared__ __align__(16) float As[RBK * 128];      // [pixel][filter]
    __shared__ __align__(16) float Bs[RBK * 128];      // [pixel][channel]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, lr = lane & 31, lh = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int r = tap / a.S, s = tap - r * a.S;
    const int ko0 = m_tile * 128, c0 = n_tile * 128;
    const int col = (t & 31) * 4, row = t >> 5;          // both images: 8 pixels per pass, 4 passes
    const bool ko_ok = ko0 + col < a.K, c_ok = c0 + col < a.C;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 ra[4], rb[4];
    auto load_tiles = [&](int kc) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int pix, src;
            rows_pixel(a, kc * RBK + row + 8 * j, cnt, r, s, pix, src);
            const bool on = pix >= 0 && src >= 0;        // a tap outside the image reads zero: the row adds nothing here
            ra[j] = (on && ko_ok) ? *reinterpret_cast<const f32x4 *>(a.dy + (long)pix * a.K + ko0 + col) : zero4;
            rb[j] = (on && c_ok) ? *reinterpret_cast<const f32x4 *>(a.x + (long)src * a.C + c0 + col) : zero4;
        }
    };

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    load_tiles(kc0);
    for (int kc = kc0; kc < kc1; ++kc) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            *reinterpret_cast<f32x4 *>(As + (row + 8 * j) * 128 + col) = ra[j];
            *reinterpret_cast<f32x4 *>(Bs + (row + 8 * j) * 128 + col) = rb[j];
        }
        __syncthreads();
        if (kc + 1 < kc1) load_tiles(kc + 1);
#pragma unroll
        for (int k2 = 0; k2 < RBK / 2; ++k2) {
            const int kr = 2 * k2 + lh;
            float fa[2], fb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) fa[i] = As[kr * 128 + (wm * 2 + i) * 32 + lr];
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = Bs[kr * 128 + (wn * 2 + j) * 32 + lr];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int c = c0 + (wn * 2 + j) * 32 + lr;
        if (c >= a.C) continue;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ko = ko0 + (wm * 2 + i) * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
                if (ko < a.K) unsafeAtomicAdd(a.dst + ((long)ko * RS + tap) * a.C + c, acc[i][j][e]);
            }
    }
}

// zero fill that runs on one side of the gate: when_rows != 0 iff *count <= max_rows
__global__ __launch_bounds__(256) void gated_zero_kernel(f32x4 *p, long n, const int *count, int max_rows, int when_rows)
{
    if ((*count <= max_rows) != (when_rows != 0)) return;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) p[i] = z;
}

int rows_args(const char *name, RowsArgs &a, const float *dy, const float *w, const float *x, float *dst, const int *rows, const int *count,
              int max_rows, int n, int h, int wd, int c, int k, int r, int s, int pad_h, int pad_w)
{
    RR_CHECK_ARG(dy && dst && rows && count && n > 0 && h > 0 && wd > 0 && c > 0 && k > 0 && r > 0 && s > 0, "%s: bad arguments", name);
    RR_CHECK_ARG(c % 4 == 0 && k % 4 == 0, "%s: C=%d and K=%d must be multiples of 4", name, c, k);
    RR_CHECK_ARG(pad_h >= 0 && pad_w >= 0 && pad_h < r && pad_w < s, "%s: pad must be in [0, kernel)", name);
    const int p = h + 2 * pad_h - r + 1, q = wd + 2 * pad_w - s + 1;
    RR_CHECK_ARG(p > 0 && q > 0, "%s: empty dy", name);
    const long M = (long)n * p * q, G2 = 1l << 31;
    RR_CHECK_ARG(M * k * 4 < G2 && (long)n * h * wd * c * 4 < G2 && (long)k * r * s * c * 4 < G2, "%s: tensors must stay below 2 GiB (the dense route takes them)", name);
    RR_CHECK_ARG(max_rows >= 0 && max_rows <= (M > (long)n * h * wd ? M : (long)n * h * wd), "%s: max_rows=%d outside [0, pixels]", name, max_rows);
    a.dy = dy; a.w = w; a.x = x; a.dst = dst; a.rows = rows; a.count = count; a.max_rows = max_rows;
    a.N = n; a.H = h; a.W = wd; a.C = c; a.K = k; a.R = r; a.S = s; a.P = p; a.Q = q; a.pad_h = pad_h; a.pad_w = pad_w;
    a.M = (int)M;
    return RR_OK;
}

}  // namespace

int rr_gated_zero(float *p, size_t bytes, const int *count, int max_rows, int when_rows, hipStream_t stream, const char *name)
{
    RR_CHECK_ARG(bytes % 16 == 0 && reinterpret_cast<size_t>(p) % 16 == 0, "%s: the gated zero fill takes 16-byte multiples", name);
    if (bytes == 0) return RR_OK;
    const long n = (long)(bytes / 16);
    const long blocks = (n + 255) / 256 > 2048 ? 2048 : (n + 255) / 256;
    hipLaunchKernelGGL(gated_zero_kernel, dim3((int)blocks), dim3(256), 0, stream, reinterpret_cast<f32x4 *>(p), n, count, max_rows, when_rows);
    RR_CHECK_LAUNCH(name);
    return RR_OK;
}

extern "C" size_t rr_active_rows_work_bytes(long m) { return sizeof(int) * 9 * (size_t)rr_cdiv(m, ROWS_PER_WG); }

extern "C" int rr_active_rows(const float *dy, long m, int k, int *rows, int *count, int *work, hipStream_t stream)
{
    RR_CHECK_ARG(dy && rows && count && work && m > 0 && k > 0 && m < (1l << 31) && m * k * 4 < (1l << 40), "rr_active_rows: bad arguments");
    const int nwg = rr_cdiv(m, ROWS_PER_WG);
    hipLaunchKernelGGL(active_rows_flag_kernel, dim3(nwg), dim3(256), 0, stream, dy, (int)m, k, nwg, work);
    RR_CHECK_LAUNCH("rr_active_rows");
    hipLaunchKernelGGL(active_rows_emit_kernel, dim3(nwg), dim3(256), 0, stream, work, nwg, rows, count);
    RR_CHECK_LAUNCH("rr_active_rows");
    return RR_OK;
}

extern "C" int rr_active_targets(const int *rows_work, int n, int h, int wd, int r, int s, int pad_h, int pad_w, int *targets, int *count,
                                 int *work, hipStream_t stream)
{
    RR_CHECK_ARG(rows_work && targets && count && work && n > 0 && h > 0 && wd > 0 && r > 0 && s > 0 && pad_h >= 0 && pad_w >= 0 && pad_h < r && pad_w < s,
                 "rr_active_targets: bad arguments");
    const int p = h + 2 * pad_h - r + 1, q = wd + 2 * pad_w - s + 1;
    RR_CHECK_ARG(p > 0 && q > 0 && (long)n * h * wd < (1l << 31) && (long)n * p * q < (1l << 31), "rr_active_targets: empty or oversized map");
    const int nwg = rr_cdiv((long)n * h * wd, ROWS_PER_WG);
    hipLaunchKernelGGL(active_targets_flag_kernel, dim3(nwg), dim3(256), 0, stream, rows_work + rr_cdiv((long)n * p * q, ROWS_PER_WG), n, h, wd, p, q,
                       r, s, pad_h, pad_w, nwg, work);
    RR_CHECK_LAUNCH("rr_active_targets");
    hipLaunchKernelGGL(active_rows_emit_kernel, dim3(nwg), dim3(256), 0, stream, work, nwg, targets, count);
    RR_CHECK_LAUNCH("rr_active_targets");
    return RR_OK;
}

extern "C" int rr_conv_dgrad_s1_rows(const float *dy, const float *w, float *dx, int n, int h, int wd, int c, int k, int r, int s, int pad_h,
                                     int pad_w, int accumulate, const int *targets, const int *count, int max_rows, hipStream_t stream)
{
    RowsArgs a{};
    if (int rc = rows_args("rr_conv_dgrad_s1_rows", a, dy, w, nullptr, dx, targets, count, max_rows, n, h, wd, c, k, r, s, pad_h, pad_w)) return rc;
    RR_CHECK_ARG(w != nullptr && max_rows <= (long)n * h * wd, "rr_conv_dgrad_s1_rows: bad arguments");
    const rr_plan::RowsPlan pl = rr_plan::rows_plan(max_rows, c, k, r, s);
    if (!accumulate)
        if (int rc = rr_gated_zero(dx, sizeof(float) * (size_t)n * h * wd * c, count, max_rows, 1, stream, "rr_conv_dgrad_s1_rows")) return rc;
    if (pl.dgrad_x == 0) return RR_OK;
    hipLaunchKernelGGL(conv_dgrad_rows_kernel, dim3(pl.dgrad_x, pl.dgrad_y), dim3(256), 0, stream, a, accumulate);
    RR_CHECK_LAUNCH("rr_conv_dgrad_s1_rows");
    return RR_OK;
}

extern "C" int rr_conv_wgrad_rows(const float *x, const float *dy, float *dw, int n, int h, int wd, int c, int k, int r, int s, int pad_h,
                                  int pad_w, const int *rows, const int *count, int max_rows, hipStream_t stream)
{
    RowsArgs a{};
    if (int rc = rows_args("rr_conv_wgrad_rows", a, dy, nullptr, x, dw, rows, count, max_rows, n, h, wd, c, k, r, s, pad_h, pad_w)) return rc;
    RR_CHECK_ARG(x != nullptr, "rr_conv_wgrad_rows: bad arguments");
    const rr_plan::RowsPlan pl = rr_plan::rows_plan(max_rows, c, k, r, s);
    if (pl.wgrad_grid == 0) return RR_OK;
    a.mt = pl.mt; a.nt = pl.nt;
    hipLaunchKernelGGL(conv_wgrad_rows_kernel, dim3(pl.wgrad_grid), dim3(256), 0, stream, a);
    RR_CHECK_LAUNCH("rr_conv_wgrad_rows");
    return RR_OK;
}
