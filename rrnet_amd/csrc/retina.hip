// RetinaNet's own kernels for gfx950: the stem's max-pool, the FPN's bilinear upsample-add, the anchor criterion
// (assignment + focal / smooth-L1 losses) and the box decode (one workgroup per image, and chunked over many for frames).
//
// All of them are bandwidth-bound (no MFMA): one pass over their operands, float4 over channels / classes where the
// innermost extent is a multiple of 4, wave-level reductions, no float atomics (the only atomics are the integer adds
// of the per-image positive count).  Built with -ffp-contract=off, so the IoU, the thresholds and the decoded boxes
// round like the reference's float32 torch ops.
#include "common.h"
#include "rrnet_hip.h"
#include "rowkit.h"

namespace {

typedef unsigned char u8;
typedef signed char i8;
typedef u8 u8x4 __attribute__((ext_vector_type(4)));

constexpr int TPB = 256;

// ------------------------------------------------------------------------------------------------------------------
// max-pool 3x3, stride 2, pad 1 (NHWC)
// ------------------------------------------------------------------------------------------------------------------
template <int V>
__global__ __launch_bounds__(TPB) void maxpool_fwd_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                          u8 *__restrict__ idx, long total, int H, int W, int OH, int OW,
                                                          int CV)
{
    const long t = (long)blockIdx.x * TPB + threadIdx.x;
    if (t >= total) return;
    const int cv = (int)(t % CV);
    long p = t / CV;
    const int ox = (int)(p % OW);
    p /= OW;
    const int oy = (int)(p % OH);
    const long n = p / OH;
    const int C = CV * V;
    float m[V];
    u8 tap[V];
    bool first = true;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky;
        if (iy < 0 || iy >= H) continue;               // padding is -inf: it never wins and never addresses memory
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx;
            if (ix < 0 || ix >= W) continue;
            const float *q = x + ((n * H + iy) * W + ix) * C + (long)cv * V;
            float v[V];
            if (V == 4) {
                const rr_f32x4 r = *reinterpret_cast<const rr_f32x4 *>(q);
                v[0] = r[0]; v[1 % V] = r[1]; v[2 % V] = r[2]; v[3 % V] = r[3];
            } else {
                v[0] = q[0];
            }
#pragma unroll
            for (int e = 0; e < V; ++e) {
                // the first tap inside the map opens the window; afterwards a strictly larger value or a NaN replaces it
                if (first || v[e] > m[e] || v[e] != v[e]) {
                    m[e] = v[e];
                    tap[e] = (u8)(ky * 3 + kx);
                }
            }
            first = false;
        }
    }
    if (V == 4) {
        rr_f32x4 r = {m[0], m[1 % V], m[2 % V], m[3 % V]};
        u8x4 k = {tap[0], tap[1 % V], tap[2 % V], tap[3 % V]};
        *reinterpret_cast<rr_f32x4 *>(y + t * 4) = r;
        *reinterpret_cast<u8x4 *>(idx + t * 4) = k;
    } else {
        y[t] = m[0];
        idx[t] = tap[0];
    }
}

// gather: an input element belongs to at most 2 x 2 windows; it sums dy of those whose stored tap names it
template <int V>
__global__ __launch_bounds__(TPB) void maxpool_bwd_kernel(const float *__restrict__ dy, const u8 *__restrict__ idx,
                                                          float *__restrict__ dx, long total, int H, int W, int OH, int OW,
                                                          int CV)
{
    const long t = (long)blockIdx.x * TPB + threadIdx.x;
    if (t >= total) return;
    const int cv = (int)(t % CV);
    long p = t / CV;
    const int ix = (int)(p % W);
    p /= W;
    const int iy = (int)(p % H);
    const long n = p / H;
    const int C = CV * V;
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
#pragma unroll
    for (int ky = 2; ky >= 0; --ky) {                  // ky descending = window row ascending
        const int ty = iy + 1 - ky;
        if (ty < 0 || (ty & 1)) continue;
        const int oy = ty >> 1;
        if (oy >= OH) continue;
#pragma unroll
        for (int kx = 2; kx >= 0; --kx) {
            const int tx = ix + 1 - kx;
            if (tx < 0 || (tx & 1)) continue;
            const int ox = tx >> 1;
            if (ox >= OW) continue;
            const long o = ((n * OH + oy) * OW + ox) * C + (long)cv * V;
            const u8 want = (u8)(ky * 3 + kx);
            if (V == 4) {
                const rr_f32x4 g = *reinterpret_cast<const rr_f32x4 *>(dy + o);
                const u8x4 k = *reinterpret_cast<const u8x4 *>(idx + o);
#pragma unroll
                for (int e = 0; e < V; ++e)
                    if (k[e] == want) acc[e] += g[e];
            } else {
                if (idx[o] == want) acc[0] += dy[o];
            }
        }
    }
    if (V == 4) {
        rr_f32x4 r = {acc[0], acc[1 % V], acc[2 % V], acc[3 % V]};
        *reinterpret_cast<rr_f32x4 *>(dx + t * 4) = r;
    } else {
        dx[t] = acc[0];
    }
}

// ------------------------------------------------------------------------------------------------------------------
// out = y + bilinear(x -> size(y)), align_corners = False (NHWC)
// ------------------------------------------------------------------------------------------------------------------
struct Tap {
    int i0, i1;
    float l0, l1;
};

// ATen's source index: scale * (dst + 0.5) - 0.5 clamped at 0, second tap clamped at in - 1
__device__ __forceinline__ Tap bilinear_tap(int dst, float scale, int in)
{
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    if (s < 0.f) s = 0.f;
    int i0 = (int)s;
    if (i0 > in - 1) i0 = in - 1;
    Tap t;
    t.i0 = i0;
    t.i1 = i0 + (i0 < in - 1 ? 1 : 0);
    float l1 = s - (float)i0;
    l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
    t.l1 = l1;
    t.l0 = 1.f - l1;
    return t;
}

template <int V>
__global__ __launch_bounds__(TPB) void bilinear_add_fwd_kernel(const float *__restrict__ x, const float *__restrict__ y,
                                                               float *__restrict__ out, long total, int IH, int IW, int OH,
                                                               int OW, int CV, float sh, float sw)
{
    const long t = (long)blockIdx.x * TPB + threadIdx.x;
    if (t >= total) return;
    const int cv = (int)(t % CV);
    long p = t / CV;
    const int ox = (int)(p % OW);
    p /= OW;
    const int oy = (int)(p % OH);
    const long n = p / OH;
    const int C = CV * V;
    const Tap ty = bilinear_tap(oy, sh, IH), tx = bilinear_tap(ox, sw, IW);
    const float *b = x + n * IH * IW * C + (long)cv * V;
    const float *p00 = b + ((long)ty.i0 * IW + tx.i0) * C, *p01 = b + ((long)ty.i0 * IW + tx.i1) * C;
    const float *p10 = b + ((long)ty.i1 * IW + tx.i0) * C, *p11 = b + ((long)ty.i1 * IW + tx.i1) * C;
    if (V == 4) {
        const rr_f32x4 a = *reinterpret_cast<const rr_f32x4 *>(p00), bb = *reinterpret_cast<const rr_f32x4 *>(p01);
        const rr_f32x4 c = *reinterpret_cast<const rr_f32x4 *>(p10), d = *reinterpret_cast<const rr_f32x4 *>(p11);
        const rr_f32x4 yy = *reinterpret_cast<const rr_f32x4 *>(y + t * 4);
        rr_f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e)
            r[e] = yy[e] + (ty.l0 * (tx.l0 * a[e] + tx.l1 * bb[e]) + ty.l1 * (tx.l0 * c[e] + tx.l1 * d[e]));
        *reinterpret_cast<rr_f32x4 *>(out + t * 4) = r;
    } else {
        out[t] = y[t] + (ty.l0 * (tx.l0 * p00[0] + tx.l1 * p01[0]) + ty.l1 * (tx.l0 * p10[0] + tx.l1 * p11[0]));
    }
}

// first / last destination index that can read source index i (a superset; the weights are recomputed per candidate)
__device__ __forceinline__ void dst_range(int i, float scale, int out, int *lo, int *hi)
{
    const float inv = 1.0f / scale;
    int a = (int)floorf(((float)i - 0.5f) * inv - 0.5f) - 1;
    int b = (int)ceilf(((float)i + 1.5f) * inv - 0.5f) + 1;
    if (i == 0) a = 0;                                  // every destination whose coordinate clamps at 0 reads source 0
    *lo = a < 0 ? 0 : a;
    *hi = b > out - 1 ? out - 1 : b;
}

template <int V>
__global__ __launch_bounds__(TPB) void bilinear_add_bwd_kernel(const float *__restrict__ dout, float *__restrict__ dx,
                                                               long total, int IH, int IW, int OH, int OW, int CV, float sh,
                                                               float sw)
{
    const long t = (long)blockIdx.x * TPB + threadIdx.x;
    if (t >= total) return;
    const int cv = (int)(t % CV);
    long p = t / CV;
    const int ix = (int)(p % IW);
    p /= IW;
    const int iy = (int)(p % IH);
    const long n = p / IH;
    const int C = CV * V;
    int ylo, yhi, xlo, xhi;
    dst_range(iy, sh, OH, &ylo, &yhi);
    dst_range(ix, sw, OW, &xlo, &xhi);
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    const float *g = dout + n * OH * OW * C + (long)cv * V;
    for (int oy = ylo; oy <= yhi; ++oy) {
        const Tap ty = bilinear_tap(oy, sh, IH);
        const bool y0 = ty.i0 == iy, y1 = ty.i1 == iy;
        if (!y0 && !y1) continue;
        for (int ox = xlo; ox <= xhi; ++ox) {
            const Tap tx = bilinear_tap(ox, sw, IW);
            const bool x0 = tx.i0 == ix, x1 = tx.i1 == ix;
            if (!x0 && !x1) continue;
            const float *q = g + ((long)oy * OW + ox) * C;
            float v[V];
            if (V == 4) {
                const rr_f32x4 r = *reinterpret_cast<const rr_f32x4 *>(q);
                v[0] = r[0]; v[1 % V] = r[1]; v[2 % V] = r[2]; v[3 % V] = r[3];
            } else {
                v[0] = q[0];
            }
            // one term per (row tap, column tap) that lands here: the four products of the forward
            if (y0 && x0) {
                const float wgt = ty.l0 * tx.l0;
#pragma unroll
                for (int e = 0; e < V; ++e) acc[e] += wgt * v[e];
            }
            if (y0 && x1) {
                const float wgt = ty.l0 * tx.l1;
#pragma unroll
                for (int e = 0; e < V; ++e) acc[e] += wgt * v[e];
            }
            if (y1 && x0) {
                const float wgt = ty.l1 * tx.l0;
#pragma unroll
                for (int e = 0; e < V; ++e) acc[e] += wgt * v[e];
            }
            if (y1 && x1) {
                const float wgt = ty.l1 * tx.l1;
#pragma unroll
                for (int e = 0; e < V; ++e) acc[e] += wgt * v[e];
            }
        }
    }
    if (V == 4) {
        rr_f32x4 r = {acc[0], acc[1 % V], acc[2 % V], acc[3 % V]};
        *reinterpret_cast<rr_f32x4 *>(dx + t * 4) = r;
    } else {
        dx[t] = acc[0];
    }
}

// ------------------------------------------------------------------------------------------------------------------
// anchor assignment
// ------------------------------------------------------------------------------------------------------------------
constexpr int ANNO_CHUNK = 256;

__global__ __launch_bounds__(TPB) void retina_assign_kernel(const float *__restrict__ annos, const float *__restrict__ anchors,
                                                            int M, int A, int num_classes, i8 *__restrict__ state,
                                                            int *__restrict__ argmax, float *__restrict__ max_iou,
                                                            int *__restrict__ cls, float *__restrict__ target,
                                                            int *__restrict__ npos)
{
    __shared__ float box[ANNO_CHUNK][4];
    __shared__ float area[ANNO_CHUNK];
    const int b = blockIdx.y;
    const int a = blockIdx.x * TPB + threadIdx.x;
    const bool live = a < A;
    const float *an = annos + (long)b * M * 8;
    float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
    if (live) {
        const rr_f32x4 r = *reinterpret_cast<const rr_f32x4 *>(anchors + (long)a * 4);
        b0 = r[0]; b1 = r[1]; b2 = r[2]; b3 = r[3];
    }
    const float b_area = (b2 - b0) * (b3 - b1);
    float best = 0.f;
    int besti = -1;
    for (int m0 = 0; m0 < M; m0 += ANNO_CHUNK) {
        const int cnt = min(ANNO_CHUNK, M - m0);
        __syncthreads();
        if ((int)threadIdx.x < cnt) {
            const float *q = an + (long)(m0 + threadIdx.x) * 8;
            const float x1 = q[0], y1 = q[1];
            const float x2 = q[2] + x1, y2 = q[3] + y1;   // the criterion's in-place xywh -> xyxy
            box[threadIdx.x][0] = x1; box[threadIdx.x][1] = y1; box[threadIdx.x][2] = x2; box[threadIdx.x][3] = y2;
            area[threadIdx.x] = (x2 - x1) * (y2 - y1);
        }
        __syncthreads();
        if (live) {
            for (int j = 0; j < cnt; ++j) {
                float iw = fminf(box[j][2], b2) - fmaxf(box[j][0], b0);
                float ih = fminf(box[j][3], b3) - fmaxf(box[j][1], b1);
                iw = iw < 0.f ? 0.f : iw;
                ih = ih < 0.f ? 0.f : ih;
                float ua = area[j] + b_area - iw * ih;
                ua = ua < 1e-8f ? 1e-8f : ua;
                const float iou = (iw * ih) / ua;
                if (besti < 0 || iou > best) {           // lowest index on ties
                    best = iou;
                    besti = m0 + j;
                }
            }
        }
    }
    bool pos = false;
    if (live) {
        const long o = (long)b * A + a;
        pos = best >= 0.5f;
        const i8 st = pos ? (i8)1 : (best < 0.4f ? (i8)0 : (i8)-1);
        int c = 0;
        rr_f32x4 tg = {0.f, 0.f, 0.f, 0.f};
        if (pos) {
            const float *q = an + (long)besti * 8;        // besti < M: it came from the loop above
            const float x1 = q[0], y1 = q[1];
            const float x2 = q[2] + x1, y2 = q[3] + y1;
            const float cf = q[5];
            const int ci = (cf >= 1.0f && cf < (float)num_classes + 1.0f) ? (int)cf : 0;   // out of range (or NaN): no bit
            c = ci;
            const float aw = b2 - b0, ah = b3 - b1;
            const float acx = b0 + 0.5f * aw, acy = b1 + 0.5f * ah;
            float gw = x2 - x1, gh = y2 - y1;
            const float gcx = x1 + 0.5f * gw, gcy = y1 + 0.5f * gh;   // centres from the unclamped sizes
            gw = gw < 1.f ? 1.f : gw;
            gh = gh < 1.f ? 1.f : gh;
            tg[0] = ((gcx - acx) / aw) / 0.1f;
            tg[1] = ((gcy - acy) / ah) / 0.1f;
            tg[2] = logf(gw / aw) / 0.2f;
            tg[3] = logf(gh / ah) / 0.2f;
        }
        state[o] = st;
        argmax[o] = besti;
        max_iou[o] = best;
        cls[o] = c;
        *reinterpret_cast<rr_f32x4 *>(target + o * 4) = tg;
    }
    const unsigned long long bal = __ballot(pos);
    if ((threadIdx.x & 63) == 0 && bal) atomicAdd(npos + b, (int)__popcll(bal));
}

// ------------------------------------------------------------------------------------------------------------------
// losses
// ------------------------------------------------------------------------------------------------------------------
#define RETINA_P_LO 1e-7f
#define RETINA_P_HI ((float)(1.0 - 1e-7))

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ float focal_term(float x, bool tgt)
{
    float p = sigmoidf_(x);
    p = p < RETINA_P_LO ? RETINA_P_LO : (p > RETINA_P_HI ? RETINA_P_HI : p);
    if (tgt) {
        const float q = 1.0f - p;
        return 0.75f * (q * q) * -logf(p);
    }
    return 0.25f * (p * p) * -logf(1.0f - p);
}

// d focal / d x, 0 where the clamp is active
__device__ __forceinline__ float focal_grad(float x, bool tgt)
{
    const float p = sigmoidf_(x);
    if (!(p >= RETINA_P_LO && p <= RETINA_P_HI)) return 0.f;
    const float q = 1.0f - p;
    float dp;
    if (tgt) dp = 0.75f * (2.0f * q * logf(p) - q * q / p);
    else dp = 0.25f * (p * p / q - 2.0f * p * logf(q));
    return dp * (p * q);
}

__device__ __forceinline__ float smooth_l1(float d)
{
    return d <= (float)(1.0 / 9.0) ? (float)(0.5 * 9.0) * (d * d) : d - (float)(0.5 / 9.0);
}

// deterministic block sum of two doubles: waves by shuffles, then wave 0 over the four wave results
__device__ __forceinline__ void block_sum2(double &a, double &b, double (*sh)[2])
{
    a = wave_sum_d(a);
    b = wave_sum_d(b);
    const int wave = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) {
        sh[wave][0] = a;
        sh[wave][1] = b;
    }
    __syncthreads();
    a = ((sh[0][0] + sh[1][0]) + sh[2][0]) + sh[3][0];
    b = ((sh[0][1] + sh[1][1]) + sh[2][1]) + sh[3][1];
}

template <int V>
__global__ __launch_bounds__(TPB) void retina_loss_partial_kernel(const float *__restrict__ logits, const float *__restrict__ loc,
                                                                  const i8 *__restrict__ state, const int *__restrict__ cls,
                                                                  const float *__restrict__ target, int A, int C,
                                                                  double *__restrict__ partial)
{
    __shared__ double sh[4][2];
    const int b = blockIdx.y;
    const long base = (long)b * A;
    const int CV = C / V;
    const long nvec = (long)A * CV;
    const long stride = (long)gridDim.x * TPB;
    double s_cls = 0.0, s_reg = 0.0;
    for (long t = (long)blockIdx.x * TPB + threadIdx.x; t < nvec; t += stride) {
        const long a = t / CV;
        const int c0 = (int)(t - a * CV) * V;
        if (state[base + a] < 0) continue;               // ignored anchors take no part
        const int hot = cls[base + a] - 1;               // -1: no target bit on this row
        const float *q = logits + (base + a) * C + c0;
        if (V == 4) {
            const rr_f32x4 r = *reinterpret_cast<const rr_f32x4 *>(q);
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) s += focal_term(r[e], c0 + e == hot);
            s_cls += (double)s;
        } else {
            s_cls += (double)focal_term(q[0], c0 == hot);
        }
    }
    for (long a = (long)blockIdx.x * TPB + threadIdx.x; a < A; a += stride) {
        if (state[base + a] != 1) continue;
        const rr_f32x4 p = *reinterpret_cast<const rr_f32x4 *>(loc + (base + a) * 4);
        const rr_f32x4 g = *reinterpret_cast<const rr_f32x4 *>(target + (base + a) * 4);
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) s += smooth_l1(fabsf(g[e] - p[e]));
        s_reg += (double)s;
    }
    block_sum2(s_cls, s_reg, sh);
    if (threadIdx.x == 0) {
        double *o = partial + ((long)b * gridDim.x + blockIdx.x) * 2;
        o[0] = s_cls;
        o[1] = s_reg;
    }
}

__global__ __launch_bounds__(TPB) void retina_loss_final_kernel(const double *__restrict__ partial, const int *__restrict__ npos,
                                                                int B, int A, int nblk, float *__restrict__ losses)
{
    __shared__ double sh[4][2];
    double l_cls = 0.0, l_reg = 0.0;
    for (int b = 0; b < B; ++b) {
        double s_cls = 0.0, s_reg = 0.0;
        for (int i = threadIdx.x; i < nblk; i += TPB) {
            s_cls += partial[((long)b * nblk + i) * 2];
            s_reg += partial[((long)b * nblk + i) * 2 + 1];
        }
        block_sum2(s_cls, s_reg, sh);
        int np = npos[b];
        np = np < 0 ? 0 : (np > A ? A : np);
        l_cls += s_cls / (double)(np > 0 ? np : 1);
        if (np > 0) l_reg += s_reg / ((double)np * 4.0);
    }
    if (threadIdx.x == 0) {
        losses[0] = (float)(l_cls / (double)B);
        losses[1] = (float)(l_reg / (double)B);
    }
}

template <int V>
__global__ __launch_bounds__(TPB) void retina_loss_bwd_kernel(const float *__restrict__ logits, const float *__restrict__ loc,
                                                              const i8 *__restrict__ state, const int *__restrict__ cls,
                                                              const float *__restrict__ target, const int *__restrict__ npos,
                                                              const float *__restrict__ gout, int B, int A, int C,
                                                              float *__restrict__ dlogits, float *__restrict__ dloc)
{
    const int b = blockIdx.y;
    const long base = (long)b * A;
    const int CV = C / V;
    const long nvec = (long)A * CV;
    const long stride = (long)gridDim.x * TPB;
    int np = npos[b];
    np = np < 0 ? 0 : (np > A ? A : np);
    const float k_cls = gout[0] / ((float)B * (float)(np > 0 ? np : 1));
    const float k_reg = np > 0 ? gout[1] / ((float)B * ((float)np * 4.0f)) : 0.f;
    for (long t = (long)blockIdx.x * TPB + threadIdx.x; t < nvec; t += stride) {
        const long a = t / CV;
        const int c0 = (int)(t - a * CV) * V;
        const bool on = state[base + a] >= 0;
        const int hot = cls[base + a] - 1;
        const long o = (base + a) * C + c0;
        if (V == 4) {
            rr_f32x4 g = {0.f, 0.f, 0.f, 0.f};
            if (on) {
                const rr_f32x4 r = *reinterpret_cast<const rr_f32x4 *>(logits + o);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float d = focal_grad(r[e], c0 + e == hot);
                    g[e] = d == 0.f ? 0.f : k_cls * d;
                }
            }
            *reinterpret_cast<rr_f32x4 *>(dlogits + o) = g;
        } else {
            float d = on ? focal_grad(logits[o], c0 == hot) : 0.f;
            dlogits[o] = d == 0.f ? 0.f : k_cls * d;
        }
    }
    for (long a = (long)blockIdx.x * TPB + threadIdx.x; a < A; a += stride) {
        rr_f32x4 g = {0.f, 0.f, 0.f, 0.f};
        if (state[base + a] == 1) {
            const rr_f32x4 p = *reinterpret_cast<const rr_f32x4 *>(loc + (base + a) * 4);
            const rr_f32x4 tg = *reinterpret_cast<const rr_f32x4 *>(target + (base + a) * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float df = p[e] - tg[e];
                const float d = fabsf(df);
                const float s = df > 0.f ? 1.f : (df < 0.f ? -1.f : 0.f);
                g[e] = k_reg * (s * (d <= (float)(1.0 / 9.0) ? 9.0f * d : 1.0f));
            }
        }
        *reinterpret_cast<rr_f32x4 *>(dloc + (base + a) * 4) = g;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// decode: one workgroup per image, rows appended in anchor order (rr_block_rank).  The class scan and the box arithmetic
// are written once, for this kernel and the chunked pair below: all three must round identically.
// ------------------------------------------------------------------------------------------------------------------
// The largest class probability of one anchor's C logits and its class: the first maximum, and a NaN is the maximum wherever
// it stands (torch's max).  `best > thr` is false on a NaN: such a row leaves.
__device__ __forceinline__ float retina_best_class(const float *q, int C, int &bi)
{
    float best = sigmoidf_(q[0]);
    bi = 0;
    for (int c = 1; c < C; ++c) {
        const float p = sigmoidf_(q[c]);
        if (p > best || p != p) {
            best = p;
            bi = c;
        }
    }
    return best;
}

// anchor (x1, y1, x2, y2) + regression d -> x, y, w, h: centres move by 0.1 * d * size, sizes scale by exp(0.2 * d)
__device__ __forceinline__ void retina_anchor_decode(const float *anchor, const float *loc, float &o0, float &o1, float &o2,
                                                     float &o3)
{
    const rr_f32x4 bx = *reinterpret_cast<const rr_f32x4 *>(anchor);
    const rr_f32x4 d = *reinterpret_cast<const rr_f32x4 *>(loc);
    const float w = bx[2] - bx[0], h = bx[3] - bx[1];
    const float cx = bx[0] + 0.5f * w, cy = bx[1] + 0.5f * h;
    const float pcx = cx + (d[0] * 0.1f) * w, pcy = cy + (d[1] * 0.1f) * h;
    o2 = expf(d[2] * 0.2f) * w;
    o3 = expf(d[3] * 0.2f) * h;
    o0 = pcx - 0.5f * o2;
    o1 = pcy - 0.5f * o3;
}

__global__ __launch_bounds__(TPB) void retina_decode_kernel(const float *__restrict__ logits, const float *__restrict__ loc,
                                                            const float *__restrict__ anchors, int A, int C, float thr,
                                                            float *__restrict__ rows, int *__restrict__ count)
{
    __shared__ int wave_cnt[TPB / 64];
    const int b = blockIdx.x;
    float *dst = rows + (long)b * A * 6;
    int run = 0;
    for (int a0 = 0; a0 < A; a0 += TPB) {
        const int a = a0 + threadIdx.x;
        bool keep = false;
        float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f, sc = 0.f, cl = 0.f;
        if (a < A) {
            int bi;
            sc = retina_best_class(logits + ((long)b * A + a) * C, C, bi);
            cl = (float)(bi + 1);
            keep = sc > thr;
            if (keep) retina_anchor_decode(anchors + (long)a * 4, loc + ((long)b * A + a) * 4, o0, o1, o2, o3);
        }
        int total;
        const int pos = run + rr_block_rank<TPB / 64>(keep, wave_cnt, total);
        if (keep && pos < A) rr_store_row6(dst + (long)pos * 6, o0, o1, o2, o3, sc, cl);
        run += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) count[b] = run;
}

// ------------------------------------------------------------------------------------------------------------------
// decode for many frames: an image's anchors spread over workgroups of RR_RETINA_DECODE_CHUNK anchors, rows appended in
// anchor order across them.  Two launches ordered by the stream and nothing else: no workgroup waits on another.
//   pass 1 (score): per anchor the probability and class + 1 of retina_decode_kernel (0 = row leaves) into the scratch,
//                   per chunk the number of rows kept
//   pass 2 (write): every workgroup sums the counts of the chunks in front of it, ranks its own rows by ballot + prefix
//                   and decodes the ones that land below k; the last chunk's workgroup owns count[f]
// ------------------------------------------------------------------------------------------------------------------
constexpr int DCHUNK = RR_RETINA_DECODE_CHUNK;
static_assert(DCHUNK == TPB, "one anchor per thread of a chunk's workgroup");

struct ScoreCls { float prob; int cls; };

__global__ __launch_bounds__(TPB) void retina_score_chunks_kernel(const float *__restrict__ logits, int A, int C, float thr,
                                                                  ScoreCls *__restrict__ sc, int *__restrict__ chunk_cnt)
{
    __shared__ int wave_cnt[TPB / 64];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int a = chunk * DCHUNK + threadIdx.x;
    bool keep = false;
    if (a < A) {
        int bi;
        ScoreCls r;
        r.prob = retina_best_class(logits + ((long)b * A + a) * C, C, bi);
        keep = r.prob > thr;
        r.cls = keep ? bi + 1 : 0;
        sc[(long)b * A + a] = r;
    }
    int total;
    rr_block_rank<TPB / 64>(keep, wave_cnt, total);
    if (threadIdx.x == 0) chunk_cnt[(long)b * gridDim.x + chunk] = total;
}

__global__ __launch_bounds__(TPB) void retina_write_chunks_kernel(const ScoreCls *__restrict__ sc, const int *__restrict__ chunk_cnt,
                                                                  const float *__restrict__ loc, const float *__restrict__ anchors,
                                                                  int A, float *__restrict__ rows, int K, int *__restrict__ count)
{
    __shared__ int wave_cnt[TPB / 64];
    __shared__ int wave_sum[TPB / 64];
    const int b = blockIdx.y, chunk = blockIdx.x;
    const int *cnt = chunk_cnt + (long)b * gridDim.x;
    int part = 0;
    for (int i = threadIdx.x; i < chunk; i += TPB) part += min(max(cnt[i], 0), DCHUNK);   // a count is at most its chunk
    part = wave_sum_i(part);
    const int a = chunk * DCHUNK + threadIdx.x;
    ScoreCls r;
    r.prob = 0.f;
    r.cls = 0;
    if (a < A) r = sc[(long)b * A + a];
    const bool keep = r.cls > 0;
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = part;            // visible behind rr_block_rank's barrier
    int total;
    const int rank = rr_block_rank<TPB / 64>(keep, wave_cnt, total);
    const int base = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];     // base <= chunk * DCHUNK <= A: no overflow
    const int pos = base + rank;                                                // the chunks in front, then this one's rows
    if (keep && pos < K) {
        float o0, o1, o2, o3;
        retina_anchor_decode(anchors + (long)a * 4, loc + ((long)b * A + a) * 4, o0, o1, o2, o3);
        rr_store_row6(rows + ((long)b * K + pos) * 6, o0, o1, o2, o3, r.prob, (float)r.cls);
    }
    if (chunk == (int)gridDim.x - 1 && threadIdx.x == 0) count[b] = base + total;
}

inline int blocks_of(long total) { return (int)((total + TPB - 1) / TPB); }
constexpr long MAX_BLOCKS = 2147483647L;

}  // namespace

extern "C" int rr_maxpool3x3s2_fwd(const float *x, float *y, unsigned char *idx, int n, int h, int w, int c,
                                   hipStream_t stream)
{
    RR_CHECK_ARG(x && y && idx && n > 0 && h > 0 && w > 0 && c > 0, "rr_maxpool3x3s2_fwd: bad dims %d %d %d %d", n, h, w, c);
    const int oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1;
    const int v = c % 4 == 0 ? 4 : 1;
    const long total = (long)n * oh * ow * (c / v);
    RR_CHECK_ARG((total + TPB - 1) / TPB <= MAX_BLOCKS, "rr_maxpool3x3s2_fwd: tensor too large");
    if (v == 4)
        hipLaunchKernelGGL(maxpool_fwd_kernel<4>, dim3(blocks_of(total)), dim3(TPB), 0, stream, x, y, idx, total, h, w, oh, ow,
                           c / 4);
    else
        hipLaunchKernelGGL(maxpool_fwd_kernel<1>, dim3(blocks_of(total)), dim3(TPB), 0, stream, x, y, idx, total, h, w, oh, ow,
                           c);
    RR_CHECK_LAUNCH("rr_maxpool3x3s2_fwd");
    return RR_OK;
}

extern "C" int rr_maxpool3x3s2_bwd(const float *dy, const unsigned char *idx, float *dx, int n, int h, int w, int c,
                                   hipStream_t stream)
{
    RR_CHECK_ARG(dy && idx && dx && n > 0 && h > 0 && w > 0 && c > 0, "rr_maxpool3x3s2_bwd: bad dims %d %d %d %d", n, h, w, c);
    const int oh = (h - 1) / 2 + 1, ow = (w - 1) / 2 + 1;
    const int v = c % 4 == 0 ? 4 : 1;
    const long total = (long)n * h * w * (c / v);
    RR_CHECK_ARG((total + TPB - 1) / TPB <= MAX_BLOCKS, "rr_maxpool3x3s2_bwd: tensor too large");
    if (v == 4)
        hipLaunchKernelGGL(maxpool_bwd_kernel<4>, dim3(blocks_of(total)), dim3(TPB), 0, stream, dy, idx, dx, total, h, w, oh, ow,
                           c / 4);
    else
        hipLaunchKernelGGL(maxpool_bwd_kernel<1>, dim3(blocks_of(total)), dim3(TPB), 0, stream, dy, idx, dx, total, h, w, oh, ow,
                           c);
    RR_CHECK_LAUNCH("rr_maxpool3x3s2_bwd");
    return RR_OK;
}

extern "C" int rr_bilinear_add_fwd(const float *x, const float *y, float *out, int n, int ih, int iw, int oh, int ow, int c,
                                   hipStream_t stream)
{
    RR_CHECK_ARG(x && y && out && n > 0 && ih > 0 && iw > 0 && oh > 0 && ow > 0 && c > 0,
                 "rr_bilinear_add_fwd: bad dims %d %d %d %d %d %d", n, ih, iw, oh, ow, c);
    const int v = c % 4 == 0 ? 4 : 1;
    const long total = (long)n * oh * ow * (c / v);
    RR_CHECK_ARG((total + TPB - 1) / TPB <= MAX_BLOCKS, "rr_bilinear_add_fwd: tensor too large");
    const float sh = (float)ih / (float)oh, sw = (float)iw / (float)ow;
    if (v == 4)
        hipLaunchKernelGGL(bilinear_add_fwd_kernel<4>, dim3(blocks_of(total)), dim3(TPB), 0, stream, x, y, out, total, ih, iw,
                           oh, ow, c / 4, sh, sw);
    else
        hipLaunchKernelGGL(bilinear_add_fwd_kernel<1>, dim3(blocks_of(total)), dim3(TPB), 0, stream, x, y, out, total, ih, iw,
                           oh, ow, c, sh, sw);
    RR_CHECK_LAUNCH("rr_bilinear_add_fwd");
    return RR_OK;
}

extern "C" int rr_bilinear_add_bwd(const float *dout, float *dx, int n, int ih, int iw, int oh, int ow, int c,
                                   hipStream_t stream)
{
    RR_CHECK_ARG(dout && dx && n > 0 && ih > 0 && iw > 0 && oh > 0 && ow > 0 && c > 0,
                 "rr_bilinear_add_bwd: bad dims %d %d %d %d %d %d", n, ih, iw, oh, ow, c);
    const int v = c % 4 == 0 ? 4 : 1;
    const long total = (long)n * ih * iw * (c / v);
    RR_CHECK_ARG((total + TPB - 1) / TPB <= MAX_BLOCKS, "rr_bilinear_add_bwd: tensor too large");
    const float sh = (float)ih / (float)oh, sw = (float)iw / (float)ow;
    if (v == 4)
        hipLaunchKernelGGL(bilinear_add_bwd_kernel<4>, dim3(blocks_of(total)), dim3(TPB), 0, stream, dout, dx, total, ih, iw,
                           oh, ow, c / 4, sh, sw);
    else
        hipLaunchKernelGGL(bilinear_add_bwd_kernel<1>, dim3(blocks_of(total)), dim3(TPB), 0, stream, dout, dx, total, ih, iw,
                           oh, ow, c, sh, sw);
    RR_CHECK_LAUNCH("rr_bilinear_add_bwd");
    return RR_OK;
}

extern "C" int rr_retina_assign(const float *annos, const float *anchors, int b, int m, int a, int num_classes,
                                signed char *state, int *argmax, float *max_iou, int *cls, float *target, int *npos,
                                hipStream_t stream)
{
    RR_CHECK_ARG(annos && anchors && state && argmax && max_iou && cls && target && npos, "rr_retina_assign: null pointer");
    RR_CHECK_ARG(b > 0 && b <= 65535 && m > 0 && a > 0 && num_classes > 0, "rr_retina_assign: bad dims b=%d m=%d a=%d classes=%d",
                 b, m, a, num_classes);
    RR_CHECK_HIP(hipMemsetAsync(npos, 0, sizeof(int) * (size_t)b, stream), "rr_retina_assign");
    hipLaunchKernelGGL(retina_assign_kernel, dim3(rr_cdiv(a, TPB), b), dim3(TPB), 0, stream, annos, anchors, m, a, num_classes,
                       state, argmax, max_iou, cls, target, npos);
    RR_CHECK_LAUNCH("rr_retina_assign");
    return RR_OK;
}

extern "C" int rr_retina_loss_blocks(int a, int c)
{
    if (a <= 0 || c <= 0) return 0;
    const long nvec = (long)a * (c % 4 == 0 ? c / 4 : c);
    long blocks = (nvec + (long)TPB * 4 - 1) / ((long)TPB * 4);
    return (int)(blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks));
}

extern "C" int rr_retina_loss_fwd(const float *logits, const float *loc, const signed char *state, const int *cls,
                                  const float *target, const int *npos, int b, int a, int c, double *partial,
                                  float *losses, hipStream_t stream)
{
    RR_CHECK_ARG(logits && loc && state && cls && target && npos && partial && losses, "rr_retina_loss_fwd: null pointer");
    RR_CHECK_ARG(b > 0 && b <= 65535 && a > 0 && c > 0, "rr_retina_loss_fwd: bad dims b=%d a=%d c=%d", b, a, c);
    const int nblk = rr_retina_loss_blocks(a, c);
    if (c % 4 == 0)
        hipLaunchKernelGGL(retina_loss_partial_kernel<4>, dim3(nblk, b), dim3(TPB), 0, stream, logits, loc, state, cls, target,
                           a, c, partial);
    else
        hipLaunchKernelGGL(retina_loss_partial_kernel<1>, dim3(nblk, b), dim3(TPB), 0, stream, logits, loc, state, cls, target,
                           a, c, partial);
    RR_CHECK_LAUNCH("rr_retina_loss_fwd");
    hipLaunchKernelGGL(retina_loss_final_kernel, dim3(1), dim3(TPB), 0, stream, partial, npos, b, a, nblk, losses);
    RR_CHECK_LAUNCH("rr_retina_loss_fwd (final)");
    return RR_OK;
}

extern "C" int rr_retina_loss_bwd(const float *logits, const float *loc, const signed char *state, const int *cls,
                                  const float *target, const int *npos, const float *gout, int b, int a, int c,
                                  float *dlogits, float *dloc, hipStream_t stream)
{
    RR_CHECK_ARG(logits && loc && state && cls && target && npos && gout && dlogits && dloc, "rr_retina_loss_bwd: null pointer");
    RR_CHECK_ARG(b > 0 && b <= 65535 && a > 0 && c > 0, "rr_retina_loss_bwd: bad dims b=%d a=%d c=%d", b, a, c);
    const int nblk = rr_retina_loss_blocks(a, c);
    if (c % 4 == 0)
        hipLaunchKernelGGL(retina_loss_bwd_kernel<4>, dim3(nblk, b), dim3(TPB), 0, stream, logits, loc, state, cls, target, npos,
                           gout, b, a, c, dlogits, dloc);
    else
        hipLaunchKernelGGL(retina_loss_bwd_kernel<1>, dim3(nblk, b), dim3(TPB), 0, stream, logits, loc, state, cls, target, npos,
                           gout, b, a, c, dlogits, dloc);
    RR_CHECK_LAUNCH("rr_retina_loss_bwd");
    return RR_OK;
}

extern "C" int rr_retina_decode(const float *logits, const float *loc, const float *anchors, int b, int a, int c,
                                float score_thr, float *rows, int *count, hipStream_t stream)
{
    RR_CHECK_ARG(logits && loc && anchors && rows && count, "rr_retina_decode: null pointer");
    RR_CHECK_ARG(b > 0 && a > 0 && c > 0, "rr_retina_decode: bad dims b=%d a=%d c=%d", b, a, c);
    hipLaunchKernelGGL(retina_decode_kernel, dim3(b), dim3(TPB), 0, stream, logits, loc, anchors, a, c, score_thr, rows, count);
    RR_CHECK_LAUNCH("rr_retina_decode");
    return RR_OK;
}

extern "C" size_t rr_retina_decode_frames_workspace_bytes(int b, int a)
{
    if (b <= 0 || a <= 0) return 0;
    const size_t chunks = ((size_t)a + DCHUNK - 1) / DCHUNK;
    return (size_t)b * (size_t)a * sizeof(ScoreCls) + (size_t)b * chunks * sizeof(int);
}

extern "C" int rr_retina_decode_frames(const float *logits, const float *loc, const float *anchors, int b, int a, int c,
                                       float score_thr, float *rows, int k, int *count, void *workspace, hipStream_t stream)
{
    RR_CHECK_ARG(logits && loc && anchors && rows && count && workspace, "rr_retina_decode_frames: null pointer");
    RR_CHECK_ARG(b > 0 && b <= 65535 && a > 0 && a <= (1 << 30) && c > 0, "rr_retina_decode_frames: bad dims b=%d a=%d c=%d", b, a,
                 c);
    RR_CHECK_ARG(k > 0 && k <= a, "rr_retina_decode_frames: %d rows per frame for %d anchors", k, a);
    const int chunks = rr_cdiv(a, DCHUNK);
    ScoreCls *sc = reinterpret_cast<ScoreCls *>(workspace);                     // [b, a]
    int *chunk_cnt = reinterpret_cast<int *>(sc + (size_t)b * (size_t)a);       // [b, chunks]
    hipLaunchKernelGGL(retina_score_chunks_kernel, dim3(chunks, b), dim3(TPB), 0, stream, logits, a, c, score_thr, sc, chunk_cnt);
    RR_CHECK_LAUNCH("rr_retina_decode_frames(score)");
    hipLaunchKernelGGL(retina_write_chunks_kernel, dim3(chunks, b), dim3(TPB), 0, stream, sc, chunk_cnt, loc, anchors, a, rows, k,
                       count);
    RR_CHECK_LAUNCH("rr_retina_decode_frames(write)");
    return RR_OK;
}
