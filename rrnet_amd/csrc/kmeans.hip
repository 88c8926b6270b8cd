// Lloyd's k-means for gfx950: R independent restarts over the same points, two launches per iteration, no host round
// trip inside a run of iterations (the done flags and iteration counts live on the device).
//
// One step (the contract of DESIGN §17, restated in tests/kmeans_cases.py):
//   kmeans_assign_kernel  grid (blocks, R): float32 squared distances (difference, product and sum each rounded, m
//     ascending: the file is built with -ffp-contract=off), label = lowest index of the minimum, then per-workgroup
//     double sums / counts per cluster and the inertia, written as partials [R, P, blocks], P = k * (M + 1) + 1.
//   kmeans_update_kernel  grid (R), one workgroup: adds the partials in a fixed order, writes the new centres (an empty
//     cluster keeps its centre), the counts, the inertia, the iteration count and the done flag.
// Both return at once for a restart whose flag is set.  No floating-point atomics: a cluster's members of one wave are
// summed by a masked xor-butterfly, waves by lane 0 into LDS in loop order, workgroups by the update kernel; a run repeats
// bit for bit.  The points (a few MB) stay in L2 and the step is latency-bound, so the grid is capped and strides.
#include "common.h"
#include "rrnet_hip.h"

namespace {

constexpr int TPB = 256;
constexpr int WAVES = TPB / 64;
constexpr int MAX_K = RR_KMEANS_MAX_K;
constexpr int MAX_M = RR_KMEANS_MAX_M;
constexpr int MAX_P = MAX_K * (MAX_M + 1);          // sums and counts of one workgroup (the inertia goes beside them)

template <int M>
__device__ __forceinline__ void load_point(const float *__restrict__ X, long n, float (&x)[M])
{
    if (M == 4) {
        const rr_f32x4 r = *reinterpret_cast<const rr_f32x4 *>(X + n * 4);
        x[0] = r[0]; x[1 % M] = r[1]; x[2 % M] = r[2]; x[3 % M] = r[3];
    } else if (M == 2) {
        const float2 r = *reinterpret_cast<const float2 *>(X + n * 2);
        x[0] = r.x; x[1 % M] = r.y;
    } else {
#pragma unroll
        for (int m = 0; m < M; ++m) x[m] = X[n * M + m];
    }
}

template <int M>
__global__ __launch_bounds__(TPB) void kmeans_assign_kernel(const float *__restrict__ X, long N, int K,
                                                            const float *__restrict__ centres, const int *__restrict__ flags,
                                                            int *__restrict__ labels, double *__restrict__ partial)
{
    __shared__ float sc[MAX_K * M];
    __shared__ double acc[WAVES][MAX_P];
    __shared__ double sin_[WAVES];
    const int r = blockIdx.y;
    if (flags[r] != 0) return;                                   // a finished restart keeps its state
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nsum = K * M, nacc = K * (M + 1);
    for (int i = tid; i < nsum; i += TPB) sc[i] = centres[(long)r * nsum + i];
    for (int i = tid; i < WAVES * MAX_P; i += TPB) (&acc[0][0])[i] = 0.0;
    __syncthreads();

    int *lab = labels + (long)r * N;
    double inertia = 0.0;
    const long stride = (long)gridDim.x * TPB;
    for (long base = (long)blockIdx.x * TPB; base < N; base += stride) {     // wave-uniform bound: every lane shuffles
        const long n = base + tid;
        const bool valid = n < N;
        float x[M];
#pragma unroll
        for (int m = 0; m < M; ++m) x[m] = 0.f;
        int best_j = -1;
        if (valid) {
            load_point<M>(X, n, x);
            float best = 0.f;
            for (int j = 0; j < K; ++j) {
                float d = 0.f;
#pragma unroll
                for (int m = 0; m < M; ++m) {
                    const float t = x[m] - sc[j * M + m];
                    const float p = t * t;
                    d = d + p;
                }
                if (j == 0 || d < best) {                        // strict: the lowest index of the minimum wins
                    best = d;
                    best_j = j;
                }
            }
            lab[n] = best_j;
            inertia += (double)best;
        }
        // the clusters present in this wave, one masked reduction each
        unsigned long long rem = __ballot(valid);
        while (rem) {
            const int lead = __ffsll((long long)rem) - 1;
            const int j = __shfl(best_j, lead, 64);
            const bool mine = best_j == j;
            const unsigned long long mask = __ballot(mine);
            rem &= ~mask;
            double s[M];
#pragma unroll
            for (int m = 0; m < M; ++m) s[m] = wave_sum_d(mine ? (double)x[m] : 0.0);
            if (lane == 0) {
#pragma unroll
                for (int m = 0; m < M; ++m) acc[wave][j * M + m] += s[m];
                acc[wave][nsum + j] += (double)__popcll(mask);
            }
        }
    }
    inertia = wave_sum_d(inertia);
    if (lane == 0) sin_[wave] = inertia;
    __syncthreads();
    const long nblk = gridDim.x;
    double *out = partial + (long)r * (nacc + 1) * nblk + blockIdx.x;
    for (int e = tid; e < nacc; e += TPB) out[e * nblk] = ((acc[0][e] + acc[1][e]) + acc[2][e]) + acc[3][e];
    if (tid == 0) out[nacc * nblk] = ((sin_[0] + sin_[1]) + sin_[2]) + sin_[3];
}

// flags: 0 = running, 1 = done and converged, 2 = done at max_iter
__global__ __launch_bounds__(TPB) void kmeans_update_kernel(const double *__restrict__ partial, int nblk, int K, int M,
                                                            float *__restrict__ centres, int *__restrict__ counts,
                                                            double *__restrict__ inertia, int *__restrict__ iters,
                                                            int *__restrict__ flags, double tol, int max_iter)
{
    __shared__ double tot[MAX_P + 1];
    __shared__ double move[MAX_K];
    const int r = blockIdx.x;
    if (flags[r] != 0) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nsum = K * M, P = K * (M + 1) + 1;
    const double *in = partial + (long)r * P * nblk;
    for (int e = wave; e < P; e += WAVES) {                      // one wave per entry: lanes stride, then the butterfly
        double s = 0.0;
        for (int i = lane; i < nblk; i += 64) s += in[(long)e * nblk + i];
        s = wave_sum_d(s);
        if (lane == 0) tot[e] = s;
    }
    __syncthreads();
    if (tid < K) {
        const int j = tid;
        const double cnt = tot[nsum + j];
        float *c = centres + ((long)r * K + j) * M;
        double d2 = 0.0;
        for (int m = 0; m < M; ++m) {
            const float old = c[m];
            const float now = cnt > 0.0 ? (float)(tot[j * M + m] / cnt) : old;      // an empty cluster stays where it was
            const double t = (double)now - (double)old;
            d2 = d2 + t * t;
            c[m] = now;
        }
        move[j] = sqrt(d2);
        counts[(long)r * K + j] = (int)cnt;
    }
    __syncthreads();
    if (tid == 0) {
        double shift = 0.0;
        for (int j = 0; j < K; ++j) shift += move[j];
        const int it = iters[r] + 1;
        iters[r] = it;
        inertia[r] = tot[P - 1];
        if (shift * shift < tol) flags[r] = 1;
        else if (it >= max_iter) flags[r] = 2;
    }
}

}  // namespace

extern "C" int rr_kmeans_blocks(long n)
{
    if (n <= 0) return 0;
    const long b = (n + TPB - 1) / TPB;
    return (int)(b < RR_KMEANS_MAX_BLOCKS ? b : RR_KMEANS_MAX_BLOCKS);
}

extern "C" size_t rr_kmeans_workspace_bytes(long n, int m, int k, int r)
{
    if (n <= 0 || m <= 0 || k <= 0 || r <= 0) return 0;
    return (size_t)r * (size_t)(k * (m + 1) + 1) * (size_t)rr_kmeans_blocks(n) * sizeof(double);
}

extern "C" int rr_kmeans_steps(const float *x, long n, int m, int k, int r, float *centres, int *labels, int *counts,
                               double *inertia, int *iters, int *flags, double tol, int max_iter, int nsteps,
                               void *workspace, hipStream_t stream)
{
    RR_CHECK_ARG(x && centres && labels && counts && inertia && iters && flags && workspace, "rr_kmeans_steps: null pointer");
    RR_CHECK_ARG(n >= 1 && m >= 1 && m <= MAX_M && k >= 1 && k <= MAX_K && r >= 1 && r <= RR_KMEANS_MAX_R,
                 "rr_kmeans_steps: bad dims n=%ld m=%d k=%d r=%d (m <= %d, k <= %d, r <= %d)", n, m, k, r, MAX_M, MAX_K,
                 RR_KMEANS_MAX_R);
    RR_CHECK_ARG(max_iter >= 1 && nsteps >= 0, "rr_kmeans_steps: max_iter=%d nsteps=%d", max_iter, nsteps);
    RR_CHECK_ARG((reinterpret_cast<size_t>(x) % 16 == 0) && (reinterpret_cast<size_t>(workspace) % 8 == 0),
                 "rr_kmeans_steps: x must be 16-byte aligned, the workspace 8-byte aligned");
    const int nblk = rr_kmeans_blocks(n);
    double *partial = static_cast<double *>(workspace);
    const dim3 grid(nblk, r), block(TPB);
    for (int s = 0; s < nsteps; ++s) {
        switch (m) {
        case 1: hipLaunchKernelGGL(kmeans_assign_kernel<1>, grid, block, 0, stream, x, n, k, centres, flags, labels, partial); break;
        case 2: hipLaunchKernelGGL(kmeans_assign_kernel<2>, grid, block, 0, stream, x, n, k, centres, flags, labels, partial); break;
        case 3: hipLaunchKernelGGL(kmeans_assign_kernel<3>, grid, block, 0, stream, x, n, k, centres, flags, labels, partial); break;
        default: hipLaunchKernelGGL(kmeans_assign_kernel<4>, grid, block, 0, stream, x, n, k, centres, flags, labels, partial); break;
        }
        RR_CHECK_LAUNCH("rr_kmeans_steps (assign)");
        hipLaunchKernelGGL(kmeans_update_kernel, dim3(r), block, 0, stream, partial, nblk, k, m, centres, counts, inertia, iters,
                           flags, tol, max_iter);
        RR_CHECK_LAUNCH("rr_kmeans_steps (update)");
    }
    return RR_OK;
}
