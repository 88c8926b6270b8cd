// rr_state_snapshot: copy + fingerprint of a training-state buffer (parameters, Adam moments) in ONE streaming pass.
//
// A workgroup owns whole digest chunks (grid-stride over chunks), so a record is finished inside the workgroup that read
// its elements: no atomics, no second launch.  Every lane moves 16 bytes per load / store; the words travel as integers
// (a float move may quieten a signalling NaN).  The three sums of a chunk are integer sums mod 2^64 -- any reduction order
// gives the same record -- reduced over the wave by shuffles, then across the four waves through LDS.
// Traffic: 4n bytes read + 4n bytes written (digest only: 4n read); the integer work (two 64-bit adds, one 32x32 multiply
// per element) sits under the memory time.
#include "common.h"
#include "rrnet_hip.h"

typedef unsigned int rr_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long u64;

#define SNAP_THREADS 256
#define SNAP_WAVES (SNAP_THREADS / 64)
#define SNAP_UNROLL 4
#define SNAP_MAX_BLOCKS 2048           // 256 CUs x 8 resident workgroups

__device__ __forceinline__ u64 snap_wave_sum(u64 v)
{
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned plo = __shfl_xor(lo, o, 64), phi = __shfl_xor(hi, o, 64);
        const u64 s = (((u64)hi << 32) | lo) + (((u64)phi << 32) | plo);
        lo = (unsigned)s;
        hi = (unsigned)(s >> 32);
    }
    return ((u64)hi << 32) | lo;
}

// one 16-byte vector whose first element is element j0 of the chunk (j0 < 2^63 / 4)
__device__ __forceinline__ void snap_acc(rr_u32x4 u, u64 j0, u64 &d0, u64 &d1, unsigned &d2)
{
    const u64 s = (u64)u.x + u.y + u.z + u.w;
    d0 += s;
    d1 += (j0 + 1) * s + ((u64)u.y + 2 * (u64)u.z + 3 * (u64)u.w);      // sum (j0 + e + 1) * u_e
    d2 += ((u.x & 0x7f800000u) == 0x7f800000u) + ((u.y & 0x7f800000u) == 0x7f800000u) +
          ((u.z & 0x7f800000u) == 0x7f800000u) + ((u.w & 0x7f800000u) == 0x7f800000u);
}

template <bool COPY>
static __global__ __launch_bounds__(SNAP_THREADS) void rr_state_snapshot_kernel(const unsigned *__restrict__ src,
                                                                                unsigned *__restrict__ dst, long n, long chunk,
                                                                                long nchunks, u64 *__restrict__ digest)
{
    __shared__ u64 part[SNAP_WAVES][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const long base = c * chunk;                               // a multiple of 4: 16-byte aligned like src
        const long len = (n - base < chunk) ? (n - base) : chunk;  // 1 .. chunk
        const long nvec = len >> 2;                                // whole 16-byte vectors; [base, base + 4 nvec) lies inside n
        const rr_u32x4 *s4 = reinterpret_cast<const rr_u32x4 *>(src + base);
        rr_u32x4 *d4 = COPY ? reinterpret_cast<rr_u32x4 *>(dst + base) : nullptr;
        u64 d0 = 0, d1 = 0;
        unsigned d2 = 0;
        long v = tid;
        for (; v + (SNAP_UNROLL - 1) * SNAP_THREADS < nvec; v += SNAP_UNROLL * SNAP_THREADS) {
            rr_u32x4 u[SNAP_UNROLL];
#pragma unroll
            for (int k = 0; k < SNAP_UNROLL; ++k) u[k] = s4[v + k * SNAP_THREADS];
#pragma unroll
            for (int k = 0; k < SNAP_UNROLL; ++k) {
                if (COPY) d4[v + k * SNAP_THREADS] = u[k];
                snap_acc(u[k], (u64)(v + k * SNAP_THREADS) * 4, d0, d1, d2);
            }
        }
        for (; v < nvec; v += SNAP_THREADS) {
            const rr_u32x4 u = s4[v];
            if (COPY) d4[v] = u;
            snap_acc(u, (u64)v * 4, d0, d1, d2);
        }
        const long j = nvec * 4 + tid;                             // the n % 4 tail of the last chunk: one word per lane
        if (tid < 3 && j < len) {
            const unsigned u = src[base + j];
            if (COPY) dst[base + j] = u;
            d0 += u;
            d1 += (u64)(j + 1) * u;
            d2 += (u & 0x7f800000u) == 0x7f800000u;
        }
        d0 = snap_wave_sum(d0);
        d1 = snap_wave_sum(d1);
        const u64 cnt = snap_wave_sum((u64)d2);
        if (lane == 0) {
            part[wave][0] = d0;
            part[wave][1] = d1;
            part[wave][2] = cnt;
        }
        __syncthreads();
        if (tid < 3) {
            u64 t = 0;
#pragma unroll
            for (int w = 0; w < SNAP_WAVES; ++w) t += part[w][tid];
            digest[c * 3 + tid] = t;
        }
        __syncthreads();                                           // part[] is rewritten by the next chunk
    }
}

extern "C" int rr_state_snapshot(const float *src, float *dst, long n, long chunk, unsigned long long *digest,
                                 hipStream_t stream)
{
    RR_CHECK_ARG(n >= 0, "rr_state_snapshot: n = %ld is negative", n);
    RR_CHECK_ARG(chunk > 0 && chunk % 4 == 0, "rr_state_snapshot: chunk = %ld must be positive and a multiple of 4", chunk);
    RR_CHECK_ARG(digest != nullptr, "rr_state_snapshot: digest is NULL");
    if (n == 0) return RR_OK;
    RR_CHECK_ARG(src != nullptr, "rr_state_snapshot: src is NULL");
    RR_CHECK_ARG(reinterpret_cast<size_t>(src) % 16 == 0 && reinterpret_cast<size_t>(dst) % 16 == 0,
                 "rr_state_snapshot: src and dst must be 16-byte aligned");
    RR_CHECK_ARG(reinterpret_cast<size_t>(digest) % 8 == 0, "rr_state_snapshot: digest must be 8-byte aligned");
    const long nchunks = (n - 1) / chunk + 1;
    const int blocks = (int)(nchunks < SNAP_MAX_BLOCKS ? nchunks : SNAP_MAX_BLOCKS);
    const unsigned *s = reinterpret_cast<const unsigned *>(src);
    unsigned *d = reinterpret_cast<unsigned *>(dst);
    if (dst != nullptr)
        hipLaunchKernelGGL(rr_state_snapshot_kernel<true>, dim3(blocks), dim3(SNAP_THREADS), 0, stream, s, d, n, chunk,
                           nchunks, digest);
    else
        hipLaunchKernelGGL(rr_state_snapshot_kernel<false>, dim3(blocks), dim3(SNAP_THREADS), 0, stream, s, d, n, chunk,
                           nchunks, digest);
    RR_CHECK_LAUNCH("rr_state_snapshot");
    return RR_OK;
}
