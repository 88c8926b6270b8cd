// Winograd F(2x2,3x3) route of the large stride-1 fp32 3x3 convolutions (include/rrnet_hip_wino.h).
//
//   Y = At [ (G g Gt) . (Bt d B) ] A     on 2x2 output tiles with 4x4 input windows: 16 multiplications per tile and channel
//                                         pair where the direct kernel spends 36
//   Bt = | 1  0 -1  0 |      G = | 1    0    0  |      At = | 1  1  1  0 |
//        | 0  1  1  0 |          | 1/2  1/2  1/2|           | 0  1 -1 -1 |
//        | 0 -1  1  0 |          | 1/2 -1/2  1/2|
//        | 0  1  0 -1 |          | 0    0    1  |
//
// Stages: wino_input_kernel (V[16][T][C], HBM-bound), the sixteen GEMMs M[i] = V[i] U[i]^T in one launch of conv.hip's
// pipelined forward kernel (rr_conv_wino_gemm: MFMA-bound), wino_output_kernel (At M A + the forward kernel's epilogue:
// bias, ReLU, accumulate, the statistics slab, or the producer's BatchNorm-backward sums; HBM-bound).  The filter transform
// runs once per filter and optimizer step.  A lane owns four channels (16 bytes) of a tile; no atomics, no workgroup waits
// for another: bit-reproducible.  The file is compiled with -ffp-contract=off (csrc/build.py): the filter cache is a function
// of the parameters alone and the link's product chains are rounded term by term like the direct kernel's.
// The weight gradient of the same layers (rr_conv_wino_wgrad): wino_input_kernel, wino_dy_kernel, the sixteen GEMMs over the
// tiles in one launch of conv.hip's weight-gradient kernel (rr_conv_wino_wgrad_gemm: its split partials meet in float atomics, like
// the direct weight gradient's), wino_dw_kernel.
#include "conv_launch.h"
#include "rrnet_hip_wino.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// a buffer descriptor the compiler can prove wave-uniform (csrc/conv.hip make_srd): 32-bit byte offsets, an out-of-range
// offset reads 0 / drops its store
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wino_srd(const void *p, long bytes)
{
    const unsigned long long u = reinterpret_cast<unsigned long long>(p);
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)u);
    const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)(u >> 32));
    void *q = reinterpret_cast<void *>(((unsigned long long)hi << 32) | lo);
    return __builtin_amdgcn_make_buffer_rsrc(q, 0, __builtin_amdgcn_readfirstlane((int)bytes), 0x00020000);
}
constexpr unsigned OOB = 0xFFFFFFF0u;
__device__ __forceinline__ f32x4 wino_load(__amdgpu_buffer_rsrc_t rs, unsigned off)
{
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
}

// ---- filter transform: u[i = 4a + b][ko][c] = (G g Gt)[a][b], g[r][s] = w[ko][r][s][c].  One row of `table` per filter
// (blockIdx.y), or without a table the one filter `one`.
struct WinoFilterRow { const float *w; float *u; long K, C; };

__global__ __launch_bounds__(256) void wino_filter_kernel(const WinoFilterRow *table, const WinoFilterRow one)
{
    const WinoFilterRow d = table != nullptr ? table[blockIdx.y] : one;
    const long KC = d.K * d.C;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < KC; idx += (long)gridDim.x * 256) {
        const long ko = idx / d.C, c = idx - ko * d.C;
        float g[3][3], t[4][3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int s = 0; s < 3; ++s) g[r][s] = d.w[(ko * 9 + r * 3 + s) * d.C + c];
#pragma unroll
        for (int s = 0; s < 3; ++s) {
            t[0][s] = g[0][s];
            t[1][s] = 0.5f * ((g[0][s] + g[2][s]) + g[1][s]);
            t[2][s] = 0.5f * ((g[0][s] + g[2][s]) - g[1][s]);
            t[3][s] = g[2][s];
        }
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const float u0 = t[a][0], u3 = t[a][2];
            const float u1 = 0.5f * ((t[a][0] + t[a][2]) + t[a][1]);
            const float u2 = 0.5f * ((t[a][0] + t[a][2]) - t[a][1]);
            d.u[(4 * a + 0) * KC + idx] = u0;
            d.u[(4 * a + 1) * KC + idx] = u1;
            d.u[(4 * a + 2) * KC + idx] = u2;
            d.u[(4 * a + 3) * KC + idx] = u3;
        }
    }
}

// ---- input transform: v[4a + b][t][c] = (Bt d B)[a][b], d the 4x4 window of tile t = (n, th, tw): pixels (2 th - 1 + i,
// 2 tw - 1 + j); those outside the map — the padding, and with odd h / w the ragged last tile row / column — read 0 through an
// out-of-range buffer offset.  Thread = (tile, channel quad).
__global__ __launch_bounds__(256) void wino_input_kernel(const float *x, float *v, int H, int W, int C, int TH, int TW, long tiles,
                                                         long x_bytes)
{
    const __amdgpu_buffer_rsrc_t rs = wino_srd(x, x_bytes);
    const int C4 = C / 4;
    const long total = tiles * C4;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long t = idx / C4;
        const int c = (int)(idx - t * C4) * 4;
        const int tw = (int)(t % TW);
        const long rest = t / TW;
        const int th = (int)(rest % TH);
        const int n = (int)(rest / TH);
        const int h0 = 2 * th - 1, w0 = 2 * tw - 1;
        f32x4 d[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int ih = h0 + i, iw = w0 + j;
                const bool in = (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W;
                const unsigned off = in ? (unsigned)((((n * H + ih) * W + iw) * C + c) * 4) : OOB;
                d[i][j] = wino_load(rs, off);
            }
        f32x4 m[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m[0][j] = d[0][j] - d[2][j];
            m[1][j] = d[1][j] + d[2][j];
            m[2][j] = d[2][j] - d[1][j];
            m[3][j] = d[1][j] - d[3][j];
        }
        float *vp = v + t * C + c;
        const long bs = tiles * C;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            *reinterpret_cast<f32x4 *>(vp + (4 * a + 0) * bs) = m[a][0] - m[a][2];
            *reinterpret_cast<f32x4 *>(vp + (4 * a + 1) * bs) = m[a][1] + m[a][2];
            *reinterpret_cast<f32x4 *>(vp + (4 * a + 2) * bs) = m[a][2] - m[a][1];
            *reinterpret_cast<f32x4 *>(vp + (4 * a + 3) * bs) = m[a][1] - m[a][3];
        }
    }
}

// ---- weight gradient: dg = Gt [ sum_tiles (A dy_tile At) . (Bt d B) ] G, A = At^T = rows (1,0), (1,1), (1,-1), (0,-1).
// dy transform: w[4a + b][t][ko] = (A dy_tile At)[a][b], dy_tile the 2x2 pixels (2 th + i, 2 tw + j) of tile t; those outside the map (the
// ragged last tile row / column of an odd map) read 0 through an out-of-range buffer offset.  Thread = (tile, filter quad): adds only.
__global__ __launch_bounds__(256) void wino_dy_kernel(const float *dy, float *w, int H, int W, int K, int TH, int TW, long tiles, long dy_bytes)
{
    const __amdgpu_buffer_rsrc_t rs = wino_srd(dy, dy_bytes);
    const int K4 = K / 4;
    const long total = tiles * K4;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long t = idx / K4;
        const int k = (int)(idx - t * K4) * 4;
        const int tw = (int)(t % TW);
        const long rest = t / TW;
        const int th = (int)(rest % TH);
        const int n = (int)(rest / TH);
        f32x4 d[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int oh = 2 * th + i, ow = 2 * tw + j;
                const bool in = oh < H && ow < W;
                const unsigned off = in ? (unsigned)((((n * H + oh) * W + ow) * K + k) * 4) : OOB;
                d[i][j] = wino_load(rs, off);
            }
        f32x4 m[4][2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            m[0][j] = d[0][j];
            m[1][j] = d[0][j] + d[1][j];
            m[2][j] = d[0][j] - d[1][j];
            m[3][j] = -d[1][j];
        }
        float *wp = w + t * K + k;
        const long bs = tiles * K;
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            *reinterpret_cast<f32x4 *>(wp + (4 * a + 0) * bs) = m[a][0];
            *reinterpret_cast<f32x4 *>(wp + (4 * a + 1) * bs) = m[a][0] + m[a][1];
            *reinterpret_cast<f32x4 *>(wp + (4 * a + 2) * bs) = m[a][0] - m[a][1];
            *reinterpret_cast<f32x4 *>(wp + (4 * a + 3) * bs) = -m[a][1];
        }
    }
}

// dw transform: dw[ko][r][s][c] += (Gt S G)[r][s], S[a][b] = s[ko][4a + b][c].  Thread = (filter, channel quad); a plain
// read-modify-write of the running gradient, ordered behind the GEMM on its stream.
__global__ __launch_bounds__(256) void wino_dw_kernel(const float *s, float *dw, int K, int C)
{
    const int C4 = C / 4;
    const long total = (long)K * C4;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long ko = idx / C4;
        const int c = (int)(idx - ko * C4) * 4;
        const float *sp = s + ko * 16 * C + c;
        f32x4 S[4][4], t[3][4];
#pragma unroll
        for (int i = 0; i < 16; ++i) S[i >> 2][i & 3] = *reinterpret_cast<const f32x4 *>(sp + (long)i * C);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            t[0][b] = S[0][b] + 0.5f * (S[1][b] + S[2][b]);
            t[1][b] = 0.5f * (S[1][b] - S[2][b]);
            t[2][b] = 0.5f * (S[1][b] + S[2][b]) + S[3][b];
        }
        float *dp = dw + ko * 9 * C + c;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            f32x4 *d0 = reinterpret_cast<f32x4 *>(dp + (long)(3 * r + 0) * C);
            f32x4 *d1 = reinterpret_cast<f32x4 *>(dp + (long)(3 * r + 1) * C);
            f32x4 *d2 = reinterpret_cast<f32x4 *>(dp + (long)(3 * r + 2) * C);
            *d0 += t[r][0] + 0.5f * (t[r][1] + t[r][2]);
            *d1 += 0.5f * (t[r][1] - t[r][2]);
            *d2 += 0.5f * (t[r][1] + t[r][2]) + t[r][3];
        }
    }
}

// ---- output transform + epilogue.  Workgroup (x, y) = statistics-slab row x, channels [256 y, 256 y + 256): it walks the tiles
// [x * per_wg, (x + 1) * per_wg), four at a time (tile lane = wave), a lane owning one channel quad.  Which pixels a slab row sums
// is free (its readers add the rows up); every row is written.
struct WinoOutArgs {
    const float *m;        // [16][T][K]
    float *y;              // [N,H,W,K]
    const float *bias;     // [K] or null
    double *slab;          // [gridDim.x][2][K] or null
    // LINK: the producer's BatchNorm-backward sums (csrc/conv.hip ConvArgs::bs_y): slab row = column sums of d and of d * xhat
    const float *bs_y, *bs_z, *bs_mean, *bs_invstd, *bs_msc, *bs_msh;
    int H, W, K, TH, TW;
    long tiles, y_bytes;
    int per_wg, relu, accumulate;
};

template <bool LINK>
__global__ __launch_bounds__(256) void wino_output_kernel(const WinoOutArgs a)
{
    __shared__ double sred[rr_plan::WINO_OUT_LANES][64][8];
    const int t = threadIdx.x, cl = t & 63, tl = t >> 6;
    const int c = (blockIdx.y * 64 + cl) * 4;
    const bool c_ok = c < a.K;
    const int cm = c_ok ? c : 0;          // a lane past the last channel reads column 0 of M and stores nothing
    const __amdgpu_buffer_rsrc_t rs_y = wino_srd(a.y, a.y_bytes);
    const __amdgpu_buffer_rsrc_t rs_py = wino_srd(LINK ? a.bs_y : a.y, a.y_bytes);
    const __amdgpu_buffer_rsrc_t rs_pz = wino_srd(LINK && a.bs_z != nullptr ? a.bs_z : a.y, a.y_bytes);
    const bool use_z = LINK && a.bs_z != nullptr;
    const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4 bv = zero4, bs_m = zero4, bs_i = zero4, bs_sc = zero4, bs_sh = zero4;
    if (c_ok) {
        if (a.bias != nullptr) bv = *reinterpret_cast<const f32x4 *>(a.bias + c);
        if constexpr (LINK) {
            bs_m = *reinterpret_cast<const f32x4 *>(a.bs_mean + c);
            bs_i = *reinterpret_cast<const f32x4 *>(a.bs_invstd + c);
            if (a.bs_z == nullptr) {
                if (a.bs_msc != nullptr) {
                    bs_sc = *reinterpret_cast<const f32x4 *>(a.bs_msc + c);
                    bs_sh = *reinterpret_cast<const f32x4 *>(a.bs_msh + c);
                } else {
                    bs_sh = f32x4{1.f, 1.f, 1.f, 1.f};      // a layer without ReLU: every element counts
                }
            }
        }
    }
    const bool want_sums = a.slab != nullptr;
    double d1[4] = {0, 0, 0, 0}, d2[4] = {0, 0, 0, 0};
    f32x4 s1 = zero4, s2 = zero4;
    int chain = 0;
    const long t_lo = (long)blockIdx.x * a.per_wg;
    const long t_hi = t_lo + a.per_wg < a.tiles ? t_lo + a.per_wg : a.tiles;
    const long mb = a.tiles * a.K;                 // elements of a batch slice
    for (long tile = t_lo + tl; tile < t_hi; tile += rr_plan::WINO_OUT_LANES) {
        const int tw = (int)(tile % a.TW);
        const long rest = tile / a.TW;
        const int th = (int)(rest % a.TH);
        const int n = (int)(rest / a.TH);
        const float *mp = a.m + tile * a.K + cm;       // (64-bit addresses: the whole of M may exceed 2 GiB)
        f32x4 m[4][4];
#pragma unroll
        for (int i = 0; i < 16; ++i) m[i >> 2][i & 3] = *reinterpret_cast<const f32x4 *>(mp + i * mb);
        unsigned off[2][2];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int oh = 2 * th + r, ow = 2 * tw + q;
                off[r][q] = (c_ok && oh < a.H && ow < a.W) ? (unsigned)((((n * a.H + oh) * a.W + ow) * a.K + c) * 4) : OOB;
            }
        f32x4 old[2][2], py[2][2], pz[2][2];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                old[r][q] = a.accumulate ? wino_load(rs_y, off[r][q]) : zero4;
                if constexpr (LINK) {
                    py[r][q] = wino_load(rs_py, off[r][q]);
                    pz[r][q] = use_z ? wino_load(rs_pz, off[r][q]) : zero4;
                }
            }
        f32x4 w[2][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            w[0][j] = (m[0][j] + m[1][j]) + m[2][j];
            w[1][j] = (m[1][j] - m[2][j]) - m[3][j];
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            f32x4 o[2];
            o[0] = (w[r][0] + w[r][1]) + w[r][2];
            o[1] = (w[r][1] - w[r][2]) - w[r][3];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                f32x4 v = o[q] + bv;
                if (a.relu) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : 0.f;
                }
                if (a.accumulate) v += old[r][q];
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), rs_y, off[r][q], 0, 0);
                const bool live = off[r][q] != OOB;        // a dropped element adds +0 to both chains
                if constexpr (LINK) {
                    const f32x4 aff = rr_bn_affine4(py[r][q], bs_sc, bs_sh);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const bool on = use_z ? pz[r][q][e] > 0.f : aff[e] > 0.f;
                        const float dd = (on && live) ? v[e] : 0.f;
                        s1[e] += dd;
                        s2[e] += dd * ((py[r][q][e] - bs_m[e]) * bs_i[e]);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float vm = live ? v[e] : 0.f;
                        s1[e] += vm;
                        s2[e] += vm * vm;
                    }
                }
            }
        }
        if (++chain == 8) {          // 8 tiles = 32 values per fp32 chain (the direct kernel's length), then on in double
#pragma unroll
            for (int e = 0; e < 4; ++e) { d1[e] += (double)s1[e]; d2[e] += (double)s2[e]; }
            s1 = zero4; s2 = zero4; chain = 0;
        }
    }
    if (!want_sums) return;           // (wave-uniform: a kernel argument)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        sred[tl][cl][e] = d1[e] + (double)s1[e];
        sred[tl][cl][4 + e] = d2[e] + (double)s2[e];
    }
    __syncthreads();
    if (tl == 0 && c_ok) {
        double *row = a.slab + (long)blockIdx.x * 2 * a.K;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double r1 = 0.0, r2 = 0.0;
#pragma unroll
            for (int l = 0; l < rr_plan::WINO_OUT_LANES; ++l) { r1 += sred[l][cl][e]; r2 += sred[l][cl][4 + e]; }
            row[c + e] = r1;
            row[a.K + c + e] = r2;
        }
    }
}

int grid_for(long threads)
{
    long blocks = (threads + 255) / 256;
    return (int)(blocks > 256 * 64 ? 256 * 64 : (blocks < 1 ? 1 : blocks));
}

int run_filter(const WinoFilterRow *table, const WinoFilterRow &one, int nfilters, int blocks_x, hipStream_t stream, const char *name)
{
    hipLaunchKernelGGL(wino_filter_kernel, dim3(blocks_x, nfilters), dim3(256), 0, stream, table, one);
    RR_CHECK_LAUNCH(name);
    return RR_OK;
}

int run_input(const float *x, float *v, int n, int h, int wd, int c, int th, int tw, long tiles, hipStream_t stream, const char *name)
{
    hipLaunchKernelGGL(wino_input_kernel, dim3(grid_for(tiles * (c / 4))), dim3(256), 0, stream, x, v, h, wd, c, th, tw, tiles,
                       (long)n * h * wd * c * 4);
    RR_CHECK_LAUNCH(name);
    return RR_OK;
}

int run_dy(const float *dy, float *w, int n, int h, int wd, int k, int th, int tw, long tiles, hipStream_t stream, const char *name)
{
    hipLaunchKernelGGL(wino_dy_kernel, dim3(grid_for(tiles * (k / 4))), dim3(256), 0, stream, dy, w, h, wd, k, th, tw, tiles,
                       (long)n * h * wd * k * 4);
    RR_CHECK_LAUNCH(name);
    return RR_OK;
}

int run_dw(const float *s, float *dw, int k, int c, hipStream_t stream, const char *name)
{
    hipLaunchKernelGGL(wino_dw_kernel, dim3(grid_for((long)k * (c / 4))), dim3(256), 0, stream, s, dw, k, c);
    RR_CHECK_LAUNCH(name);
    return RR_OK;
}

// the weight gradient's shape rule as the entry points apply it: wino_wgrad_plan without its pixel floor
int checked_wgrad_plan(const char *name, int n, int h, int wd, int c, int k, size_t ws_bytes, rr_plan::WinoWgradPlan *pl)
{
    *pl = rr_plan::wino_wgrad_plan(rr_plan::MATH_F32, {n, h, wd, c, k, 3, 3, 1, 1, 1, 0, 0}, false);
    RR_CHECK_ARG(pl->refuse == nullptr || pl->floor_only, "%s: %s", name, pl->refuse);
    RR_CHECK_ARG(ws_bytes >= (size_t)pl->ws_bytes, "%s: workspace of %ld bytes needed (rr_conv_wino_wgrad_ws_bytes)", name, pl->ws_bytes);
    return RR_OK;
}

// the route's shape rule as the entry points apply it: wino_plan without its pixel floor
int checked_plan(const char *name, int n, int h, int wd, int c, int k, const rr_plan::ConvFlags &f, size_t ws_bytes, rr_plan::WinoPlan *pl)
{
    *pl = rr_plan::wino_plan(rr_plan::MATH_F32, {n, h, wd, c, k, 3, 3, 1, 1, 1, 0, 0}, f);
    RR_CHECK_ARG(pl->refuse == nullptr || pl->floor_only, "%s: %s", name, pl->refuse);
    RR_CHECK_ARG(ws_bytes >= (size_t)pl->ws_bytes, "%s: workspace of %ld bytes needed (rr_conv_wino_ws_bytes)", name, pl->ws_bytes);
    return RR_OK;
}

int run_route(const char *name, const float *x, const float *u, float *y, float *ws, int n, int h, int wd, int c, int k,
              const rr_plan::WinoPlan &pl, WinoOutArgs &o, bool link, hipStream_t stream)
{
    float *v = ws, *m = ws + 16 * pl.tiles * c;
    if (int rc = run_input(x, v, n, h, wd, c, pl.th, pl.tw, pl.tiles, stream, name)) return rc;
    if (int rc = rr_conv_wino_gemm(v, u, m, pl.tiles, c, k, stream, name)) return rc;
    o.m = m; o.y = y; o.y_bytes = (long)n * h * wd * k * 4; o.H = h; o.W = wd; o.K = k; o.TH = pl.th; o.TW = pl.tw; o.tiles = pl.tiles; o.per_wg = pl.tiles_per_wg;
    if (link) hipLaunchKernelGGL(wino_output_kernel<true>, dim3(pl.out_x, pl.out_y), dim3(256), 0, stream, o);
    else hipLaunchKernelGGL(wino_output_kernel<false>, dim3(pl.out_x, pl.out_y), dim3(256), 0, stream, o);
    RR_CHECK_LAUNCH(name);
    return RR_OK;
}

}  // namespace

extern "C" int rr_conv_wino_plan(int math, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w, int out_h,
                                 int out_w, int flags, int *plan)
{
    RR_CHECK_ARG(plan != nullptr && ((flags >> 8) & 3) <= rr_plan::LINK_RELU_BIAS, "rr_conv_wino_plan: bad arguments");
    const rr_plan::WinoPlan pl = rr_plan::wino_plan(math, {n, h, wd, c, k, r, s, stride, pad_h, pad_w, out_h, out_w},
                                                    {(flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, (flags >> 8) & 3, (flags & 8) != 0,
                                                     (flags & 16) != 0});
    const int out[RR_WINO_PLAN_INTS] = {pl.refuse == nullptr, pl.floor_only, (int)(pl.tiles & 0x7fffffff), (int)(pl.tiles >> 31), pl.bn, pl.gemm_blocks, pl.out_x,
                                        pl.out_y, pl.tiles_per_wg, (int)(pl.ws_bytes & 0x7fffffff), (int)(pl.ws_bytes >> 31)};
    for (int i = 0; i < RR_WINO_PLAN_INTS; ++i) plan[i] = out[i];
    return RR_OK;
}

extern "C" size_t rr_conv_wino_ws_bytes(int n, int h, int wd, int c, int k)
{
    if (n <= 0 || h <= 0 || wd <= 0 || c <= 0 || k <= 0) return 0;
    return (size_t)16 * n * ((h + 1) / 2) * ((wd + 1) / 2) * ((size_t)c + k) * sizeof(float);
}

extern "C" int rr_wino_filter_batch(const long long *table, int nfilters, hipStream_t stream)
{
    static_assert(sizeof(WinoFilterRow) == 4 * sizeof(long long), "rr_wino_filter_batch: four 64-bit words per filter");
    RR_CHECK_ARG(table != nullptr && nfilters >= 0 && nfilters < 65536, "rr_wino_filter_batch: bad arguments");
    if (nfilters == 0) return RR_OK;
    return run_filter(reinterpret_cast<const WinoFilterRow *>(table), WinoFilterRow{}, nfilters, 64, stream, "rr_wino_filter_batch");
}

extern "C" int rr_wino_filter(const float *w, float *u, int k, int c, hipStream_t stream)
{
    RR_CHECK_ARG(w != nullptr && u != nullptr && k > 0 && c > 0, "rr_wino_filter: bad arguments");
    return run_filter(nullptr, WinoFilterRow{w, u, k, c}, 1, grid_for((long)k * c), stream, "rr_wino_filter");
}

extern "C" int rr_wino_input(const float *x, float *v, int n, int h, int wd, int c, hipStream_t stream)
{
    rr_plan::WinoPlan pl;
    if (int rc = checked_plan("rr_wino_input", n, h, wd, c, c, {}, (size_t)-1, &pl)) return rc;
    RR_CHECK_ARG(x != nullptr && v != nullptr, "rr_wino_input: null argument");
    return run_input(x, v, n, h, wd, c, pl.th, pl.tw, pl.tiles, stream, "rr_wino_input");
}

extern "C" int rr_wino_gemm(const float *v, const float *u, float *m, long tiles, int c, int k, hipStream_t stream)
{
    RR_CHECK_ARG(v != nullptr && u != nullptr && m != nullptr, "rr_wino_gemm: null argument");
    return rr_conv_wino_gemm(v, u, m, tiles, c, k, stream, "rr_wino_gemm");
}

extern "C" int rr_conv_wino_fprop(const float *x, const float *u, const float *bias, float *y, double *stat_slab, float *ws, size_t ws_bytes,
                                  int n, int h, int wd, int c, int k, int relu, int accumulate, hipStream_t stream)
{
    rr_plan::WinoPlan pl;
    if (int rc = checked_plan("rr_conv_wino_fprop", n, h, wd, c, k,
                              {bias != nullptr, relu != 0, stat_slab != nullptr, rr_plan::LINK_NONE, accumulate != 0, false}, ws_bytes, &pl))
        return rc;
    RR_CHECK_ARG(x != nullptr && u != nullptr && y != nullptr && ws != nullptr, "rr_conv_wino_fprop: null argument");
    WinoOutArgs o{};
    o.bias = bias; o.slab = stat_slab; o.relu = relu != 0; o.accumulate = accumulate != 0;
    return run_route("rr_conv_wino_fprop", x, u, y, ws, n, h, wd, c, k, pl, o, false, stream);
}

extern "C" int rr_conv_wino_dgrad_bnsum(const float *dy, const float *u, float *dx, float *ws, size_t ws_bytes, int n, int h, int wd, int c,
                                        int k, int accumulate, const float *prod_y, const float *prod_z, const float *prod_mean,
                                        const float *prod_invstd, const float *prod_mask_scale, const float *prod_mask_shift, double *slab,
                                        double *sums, hipStream_t stream)
{
    const char *name = "rr_conv_wino_dgrad_bnsum";
    const BnSumArgs bs{prod_y, prod_z, prod_mean, prod_invstd, prod_mask_scale, prod_mask_shift, slab, sums, 0};
    RR_CHECK_ARG(bs.bn_ok(c) && dy != nullptr && u != nullptr && dx != nullptr && ws != nullptr,
                 "%s: bad arguments (every tensor, the producer's tensors and the two buffers; C %% 4 == 0, C <= 1024)", name);
    rr_plan::WinoPlan pl;      // the forward geometry of the data gradient: dy's k channels in, dx's c channels out
    if (int rc = checked_plan(name, n, h, wd, k, c, {false, false, false, rr_plan::LINK_BN, accumulate != 0, false}, ws_bytes, &pl)) return rc;
    WinoOutArgs o{};
    o.slab = slab; o.accumulate = accumulate != 0;
    o.bs_y = prod_y; o.bs_z = prod_z; o.bs_mean = prod_mean; o.bs_invstd = prod_invstd; o.bs_msc = prod_mask_scale; o.bs_msh = prod_mask_shift;
    if (int rc = run_route(name, dy, u, dx, ws, n, h, wd, k, c, pl, o, true, stream)) return rc;
    return rr_bn_reduce_slab(slab, pl.out_x, c, sums, stream);
}

extern "C" int rr_conv_wino_wgrad_plan(int math, int n, int h, int wd, int c, int k, int r, int s, int stride, int pad_h, int pad_w, int out_h,
                                       int out_w, int flags, int *plan)
{
    RR_CHECK_ARG(plan != nullptr, "rr_conv_wino_wgrad_plan: bad arguments");
    const rr_plan::WinoWgradPlan pl = rr_plan::wino_wgrad_plan(math, {n, h, wd, c, k, r, s, stride, pad_h, pad_w, out_h, out_w}, (flags & 1) != 0);
    const int out[RR_WINO_WGRAD_PLAN_INTS] = {pl.refuse == nullptr, pl.floor_only, (int)(pl.tiles & 0x7fffffff), (int)(pl.tiles >> 31), pl.gemm.pipe,
                                              pl.gemm.splits, pl.gemm.per_split, pl.gemm.grid, (int)(pl.ws_bytes & 0x7fffffff), (int)(pl.ws_bytes >> 31)};
    for (int i = 0; i < RR_WINO_WGRAD_PLAN_INTS; ++i) plan[i] = out[i];
    return RR_OK;
}

extern "C" size_t rr_conv_wino_wgrad_ws_bytes(int n, int h, int wd, int c, int k)
{
    if (n <= 0 || h <= 0 || wd <= 0 || c <= 0 || k <= 0) return 0;
    return ((size_t)16 * n * ((h + 1) / 2) * ((wd + 1) / 2) * ((size_t)c + k) + (size_t)16 * k * c) * sizeof(float);
}

extern "C" int rr_wino_dy(const float *dy, float *w, int n, int h, int wd, int k, hipStream_t stream)
{
    rr_plan::WinoWgradPlan pl;
    if (int rc = checked_wgrad_plan("rr_wino_dy", n, h, wd, k, k, (size_t)-1, &pl)) return rc;
    RR_CHECK_ARG(dy != nullptr && w != nullptr, "rr_wino_dy: null argument");
    return run_dy(dy, w, n, h, wd, k, pl.th, pl.tw, pl.tiles, stream, "rr_wino_dy");
}

extern "C" int rr_wino_wgrad_gemm(const float *v, const float *w, float *s, long tiles, int c, int k, hipStream_t stream)
{
    RR_CHECK_ARG(v != nullptr && w != nullptr && s != nullptr, "rr_wino_wgrad_gemm: null argument");
    return rr_conv_wino_wgrad_gemm(v, w, s, tiles, c, k, stream, "rr_wino_wgrad_gemm");
}

extern "C" int rr_wino_dw(const float *s, float *dw, int k, int c, hipStream_t stream)
{
    RR_CHECK_ARG(s != nullptr && dw != nullptr && k > 0 && c > 0 && c % 4 == 0, "rr_wino_dw: bad arguments");
    return run_dw(s, dw, k, c, stream, "rr_wino_dw");
}

extern "C" int rr_conv_wino_wgrad(const float *x, const float *dy, float *dw, float *ws, size_t ws_bytes, int n, int h, int wd, int c, int k,
                                  hipStream_t stream)
{
    const char *name = "rr_conv_wino_wgrad";
    rr_plan::WinoWgradPlan pl;
    if (int rc = checked_wgrad_plan(name, n, h, wd, c, k, ws_bytes, &pl)) return rc;
    RR_CHECK_ARG(x != nullptr && dy != nullptr && dw != nullptr && ws != nullptr, "%s: null argument", name);
    float *v = ws, *w = v + 16 * pl.tiles * c, *s = w + 16 * pl.tiles * k;
    if (int rc = run_input(x, v, n, h, wd, c, pl.th, pl.tw, pl.tiles, stream, name)) return rc;
    if (int rc = run_dy(dy, w, n, h, wd, k, pl.th, pl.tw, pl.tiles, stream, name)) return rc;
    RR_CHECK_HIP(rr_zero2(s, sizeof(float) * 16 * (size_t)k * c, nullptr, 0, stream), name);
    if (int rc = rr_conv_wino_wgrad_gemm(v, w, s, pl.tiles, c, k, stream, name)) return rc;
    return run_dw(s, dw, k, c, stream, name);
}
