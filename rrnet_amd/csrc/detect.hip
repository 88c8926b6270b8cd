// Batched multi-scale detection on raw frames for gfx950: what surrounds the model in the multi-scale evaluation body
// (operators/rrnet_operator.py:256-279), for B equal-size frames per launch.
//   rr_prepare_frames        uint8 RGB frames -> ToTensor -> Normalize -> F.interpolate(scale_factor, bilinear,
//                            align_corners=True) in ONE gather (:262-263), NHWC fp32 network input
//   rr_merge_scales          generate_bbox (:188-209) + `score > 0.01` (:266-267) + `pred_bbox[:, :4] / scale` (:268) of one
//                            scale, appended per frame to the cross-scale concatenation (:271)
//   rr_sort_frames_by_score  `torch.sort(pred_bbox[:, 4], descending=True)` (:272) per frame: the batched
//                            rr_sort_rows_by_score
//   rr_prepare_tiles         rr_prepare_frames for equal-size tiles cut out of frames of differing sizes (tiled inference:
//   rr_merge_tiles           the builder's own feature, the reference has none), and the way back: per-tile rows -> margin
//                            test -> frame coordinates -> per-frame blocks in table order
// Built with -ffp-contract=off like refine.hip: every step of the box arithmetic is its own fp32 rounding and the division by
// the scale is an IEEE division (the reference divides on the CPU).  The interpolation in rr_prepare_frames has to give the
// bits of rr_resize_bilinear_ac: its fused steps are written as explicit fmas (prep_taps / prep_bilinear below).
// The compaction of the merge kernels, the sort and the normalisation table come from rowkit.h.
#include "common.h"
#include "rrnet_hip.h"
#include "rowkit.h"

#define DET_THREADS 256
#define DET_SORT_THREADS 1024
#define DET_MAX_ROWS 16384          // rows of one frame the LDS sort holds (RR_DETECT_MAX_ROWS)

namespace {

// Source coordinates and the four-tap blend of resize_bilinear_ac_kernel (elementwise.hip).  That file is compiled with the
// compiler's default contraction, and what the compiler makes of `ly = sy*h - y0` and of
// `hy * (hx*v00 + lx*v01) + ly * (hx*v10 + lx*v11)` there is spelled out here with explicit fmas (this file is built with
// -ffp-contract=off, so nothing else fuses): the fraction is one fma of the un-rounded product, each row blend fuses its
// second product onto the rounded first one, and the two row terms are rounded separately before their sum.
// tests/test_detect_gpu.py holds the two kernels to the same bits.
// h / w: output row / column; H, W: source size; sy / sx: (H-1)/(OH-1), (W-1)/(OW-1) or 0.
struct PrepTaps { int y0, y1, x0, x1; float ly, lx, hy, hx; };

__device__ __forceinline__ PrepTaps prep_taps(float sy, float sx, int h, int w, int H, int W)
{
    PrepTaps t;
    const float fh = (float)h, fw = (float)w;
    const float fy = sy * fh, fx = sx * fw;
    t.y0 = (int)fy, t.x0 = (int)fx;
    t.y1 = t.y0 + (t.y0 < H - 1 ? 1 : 0), t.x1 = t.x0 + (t.x0 < W - 1 ? 1 : 0);
    t.ly = __builtin_fmaf(sy, fh, -(float)t.y0), t.lx = __builtin_fmaf(sx, fw, -(float)t.x0);
    t.hy = 1.f - t.ly, t.hx = 1.f - t.lx;
    return t;
}

__device__ __forceinline__ float prep_bilinear(const PrepTaps &t, float v00, float v01, float v10, float v11)
{
    const float r0 = __builtin_fmaf(t.lx, v01, t.hx * v00);
    const float r1 = __builtin_fmaf(t.lx, v11, t.hx * v10);
    return t.hy * r0 + t.ly * r1;
}

// Where the th x tw source window of output image n lies.
//   PrepFrames: image n is the whole of frame n, N equal-size frames back to back (th x tw = the frame).
//   PrepTiles:  image n is the window of frame tiles[n][0] at (tiles[n][1], tiles[n][2]); frame f is [H_f, W_f, 3] bytes at
//               src + frame_base[f], any byte address: byte loads, 64-bit offsets.  The table is checked on the host.
struct PrepFrames {
    static constexpr bool from_table = false;
    const uint8_t *src;
};
struct PrepTiles {
    static constexpr bool from_table = true;
    const uint8_t *src; const long long *frame_base; const int *frame_hw; int F; const int *tiles;
};

// The prepare body: N images of th x tw source pixels -> OH x OW, one thread per output pixel (three channels = 12
// contiguous bytes of the NHWC output).  The taps are those of the WINDOW (prep_taps with H = th, W = tw), so for a tile the
// "+1" tap stops at the tile's last row / column and the output carries the bits the whole-frame kernel writes for the
// host-cropped window.  The lanes of a wave hold consecutive output columns of one row, so their byte loads fall into one
// or two source rows of at most 64 * 3 * sx bytes each; a tile finds them through one table row per pixel (12 bytes that
// every lane of the wave shares: one L1 line).
// MIRROR: a second, x-mirrored copy of every image behind the N plain ones, the flip of CenterNet's test-time
// augmentation (operators/centernet_operator.py:268-272), which the reference applies AFTER the resize.  Each pixel is
// computed once, at its plain position, and stored twice: out[n][h][w] and out[N+n][h][OW-1-w].  The mirrored stores of a
// wave cover the same contiguous 64 * 12 bytes of a row as its plain ones, in descending lane order: whole cache lines
// either way, no staging in LDS.
template <class Source, bool MIRROR>
__device__ __forceinline__ void prepare_gather(const Source &from, const float *__restrict__ mean, const float *__restrict__ stdv,
                                               float *__restrict__ out, int N, int th, int tw, int OH, int OW)
{
    __shared__ float lut[256 * 3];                       // lut[v*3 + c], as augment_frames_kernel builds it
    rr_norm_lut_fill<DET_THREADS>(lut, mean, stdv);
    const long total = (long)N * OH * OW;
    const float sy = OH > 1 ? (float)(th - 1) / (float)(OH - 1) : 0.f;
    const float sx = OW > 1 ? (float)(tw - 1) / (float)(OW - 1) : 0.f;
    for (long p = (long)blockIdx.x * DET_THREADS + threadIdx.x; p < total; p += (long)gridDim.x * DET_THREADS) {
        long q = p;
        const int w = (int)(q % OW); q /= OW;
        const int h = (int)(q % OH);
        const int n = (int)(q / OH);                     // < N
        const PrepTaps t = prep_taps(sy, sx, h, w, th, tw);
        // (int)(sy*h) <= th-1 and (int)(sx*w) <= tw-1 up to one rounding of the product: clamp what addresses memory
        int y0 = min(max(t.y0, 0), th - 1), y1 = min(max(t.y1, 0), th - 1);
        int x0 = min(max(t.x0, 0), tw - 1), x1 = min(max(t.x1, 0), tw - 1);
        const uint8_t *b;
        int W;
        if constexpr (Source::from_table) {
            // what the table and frame_hw say is clamped again, inside the frame they name, before it addresses memory
            const int f = min(max(from.tiles[n * 3], 0), from.F - 1);
            const int H = max(from.frame_hw[f * 2], 1);
            W = max(from.frame_hw[f * 2 + 1], 1);
            const int oy = from.tiles[n * 3 + 1], ox = from.tiles[n * 3 + 2];
            y0 = min(max(oy + y0, 0), H - 1), y1 = min(max(oy + y1, 0), H - 1);
            x0 = min(max(ox + x0, 0), W - 1), x1 = min(max(ox + x1, 0), W - 1);
            b = from.src + from.frame_base[f];
        } else {
            W = tw;
            b = from.src + (long)n * th * tw * 3;
        }
        const uint8_t *p00 = b + ((long)y0 * W + x0) * 3, *p01 = b + ((long)y0 * W + x1) * 3;
        const uint8_t *p10 = b + ((long)y1 * W + x0) * 3, *p11 = b + ((long)y1 * W + x1) * 3;
        float *o = out + p * 3;
        float *m = out + ((((long)N + n) * OH + h) * OW + (OW - 1 - w)) * 3;      // MIRROR only; 0 <= OW-1-w < OW, N+n < 2N
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = prep_bilinear(t, lut[p00[c] * 3 + c], lut[p01[c] * 3 + c], lut[p10[c] * 3 + c], lut[p11[c] * 3 + c]);
            o[c] = v;
            if constexpr (MIRROR) m[c] = v;
        }
    }
}

__global__ __launch_bounds__(DET_THREADS) void prepare_frames_kernel(const uint8_t *__restrict__ src, const float *__restrict__ mean,
                                                                     const float *__restrict__ stdv, float *__restrict__ out, int N,
                                                                     int H, int W, int OH, int OW)
{
    prepare_gather<PrepFrames, false>(PrepFrames{src}, mean, stdv, out, N, H, W, OH, OW);
}

__global__ __launch_bounds__(DET_THREADS) void prepare_frames_pair_kernel(const uint8_t *__restrict__ src,
                                                                          const float *__restrict__ mean,
                                                                          const float *__restrict__ stdv, float *__restrict__ out,
                                                                          int N, int H, int W, int OH, int OW)
{
    prepare_gather<PrepFrames, true>(PrepFrames{src}, mean, stdv, out, N, H, W, OH, OW);
}

__global__ __launch_bounds__(DET_THREADS) void prepare_tiles_kernel(const uint8_t *__restrict__ src,
                                                                    const long long *__restrict__ frame_base,
                                                                    const int *__restrict__ frame_hw, int F,
                                                                    const int *__restrict__ tiles, int T, int TH, int TW, int OH,
                                                                    int OW, const float *__restrict__ mean,
                                                                    const float *__restrict__ stdv, float *__restrict__ out)
{
    prepare_gather<PrepTiles, false>(PrepTiles{src, frame_base, frame_hw, F, tiles}, mean, stdv, out, T, TH, TW, OH, OW);
}

// The three merge kernels below append rows in order at merged[f][count[f]...], one workgroup per frame: each pass of
// DET_THREADS rows is ranked by rr_block_rank, the rows kept so far are counted in a register.  Launches are ordered by the
// stream and no workgroup reads what another writes, so count[f] needs no atomics and the result does not depend on the
// dispatch order.

// Rows (x, y, w, h, score, cls) of the frame's tiles [tile_off[f], tile_off[f+1]), tile by tile in table order, the first
// min(max(count_in[t], 0), k_in) rows of each in row order -> margin test in the model's input coordinates ->
// x / div + x0, y / div + y0, w / div, h / div.  count[f] ends as the true number of kept rows, also above K (so the base is
// not clamped and the position is 64-bit); rows at and beyond K are not written.
__global__ __launch_bounds__(DET_THREADS) void merge_tiles_kernel(const float *rows, const int *count_in, const int *tiles,
                                                                  const int *tile_off, const int *frame_hw, int k_in, int TH,
                                                                  int TW, float fow, float foh, float div, float margin,
                                                                  float *merged, int *count, int K)
{
    __shared__ int wave_cnt[DET_THREADS / 64];
    const int f = blockIdx.x;
    const int t0 = max(tile_off[f], 0), t1 = max(tile_off[f + 1], t0);     // the host built and checked the offsets
    const int H = frame_hw[f * 2], W = frame_hw[f * 2 + 1];
    const int base0 = max(count[f], 0);
    const bool test = margin > 0.0f;
    int run = 0;
    float *dst = merged + (long)f * K * 6;
    for (int t = t0; t < t1; ++t) {
        const int n = min(max(count_in[t], 0), k_in);
        const int oy = tiles[t * 3 + 1], ox = tiles[t * 3 + 2];
        const float fy = (float)oy, fx = (float)ox;
        // a side is interior when it is not on the frame's border: only there has the tile cut what it shows
        const bool left = test && ox > 0, top = test && oy > 0;
        const bool right = test && ox + TW < W, bottom = test && oy + TH < H;
        const float *src = rows + (long)t * k_in * 6;
        for (int base = 0; base < n; base += DET_THREADS) {
            const int i = base + threadIdx.x;
            bool keep = false;
            float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f, sc = 0.f, cl = 0.f;
            if (i < n) {
                const float *q = src + (long)i * 6;
                const float x = q[0], y = q[1], w = q[2], h = q[3];
                sc = q[4];
                cl = q[5];
                // every comparison is false on a NaN: the row stays
                const bool cut = (left && x < margin) || (top && y < margin) || (right && x + w > fow - margin) ||
                                 (bottom && y + h > foh - margin);
                keep = !cut;
                o0 = x / div + fx;                       // IEEE division, then one addition: two roundings
                o1 = y / div + fy;
                o2 = w / div;
                o3 = h / div;
            }
            int total;
            const long pos = (long)base0 + run + rr_block_rank<DET_THREADS / 64>(keep, wave_cnt, total);
            if (keep && pos < K) rr_store_row6(dst + pos * 6, o0, o1, o2, o3, sc, cl);
            run += total;
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) count[f] = (int)min((long)base0 + run, 0x7fffffffl);
}

// CenterNet rows (x, y, w, h, score, cls+1) of one scale, k_in per image as rr_decode_topk (box_mode 1) writes them, ->
// `score > thr` (transform_bbox, :177) -> for the flipped image x = (img_w - x) - w (flip_annos) -> x,y,w,h / div, the
// flipped image's rows (image nframes + f) in front of the plain one's (image f): the reference's concatenation order
// (:266-285).
__global__ __launch_bounds__(DET_THREADS) void merge_ctnet_kernel(const float *rows, int nframes, int k_in, int pair, float img_w,
                                                                  float div, float thr, float *merged, int *count, int K)
{
    __shared__ int wave_cnt[DET_THREADS / 64];
    const int f = blockIdx.x;
    const int base0 = min(max(count[f], 0), K);
    int run = 0;
    float *dst = merged + (long)f * K * 6;
    for (int half = pair ? 1 : 0; half >= 0; --half) {   // 1: the flipped image, 0: the plain one
        const float *src = rows + ((long)half * nframes + f) * k_in * 6;
        for (int base = 0; base < k_in; base += DET_THREADS) {
            const int i = base + threadIdx.x;
            bool keep = false;
            float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f, sc = 0.f, cl = 0.f;
            if (i < k_in) {
                const float *q = src + (long)i * 6;
                float x = q[0];
                const float y = q[1], w = q[2], h = q[3];
                sc = q[4];
                cl = q[5];
                if (half) x = (img_w - x) - w;           // flip_annos on the undivided row: two fp32 subtractions
                o0 = x / div;                            // pred[:, :4] / scale on the host: IEEE division
                o1 = y / div;
                o2 = w / div;                            // not clamped: negative sizes pass, as in the reference
                o3 = h / div;
                keep = sc > thr;                         // NaN leaves
            }
            int total;
            const int pos = base0 + run + rr_block_rank<DET_THREADS / 64>(keep, wave_cnt, total);
            if (keep && pos < K) rr_store_row6(dst + (long)pos * 6, o0, o1, o2, o3, sc, cl);
            run += total;
            __syncthreads();
        }
    }
    if (threadIdx.x == 0) count[f] = min(base0 + run, K);
}

// Rows [frame_off[f], frame_off[f+1]) of one scale's packed stage-2 inputs -> generate_bbox rows
// (x, y, w, h, score, cls+1), optional `score > thr`, x,y,w,h / div.
__global__ __launch_bounds__(DET_THREADS) void merge_scales_kernel(const float *rois, const float *reg, const float *scores,
                                                                   const float *clses, const int *frame_off, int R, float scale,
                                                                   float div, int filter, float thr, float *merged, int *count,
                                                                   int K)
{
    __shared__ int wave_cnt[DET_THREADS / 64];
    const int f = blockIdx.x;
    const int r0 = min(max(frame_off[f], 0), R);
    const int n = min(max(frame_off[f + 1] - r0, 0), R - r0);
    const int base0 = min(max(count[f], 0), K);
    int run = 0;
    float *dst = merged + (long)f * K * 6;
    for (int base = 0; base < n; base += DET_THREADS) {
        const int i = base + threadIdx.x;
        bool keep = false;
        float o0 = 0.f, o1 = 0.f, o2 = 0.f, o3 = 0.f, sc = 0.f, cl = 0.f;
        if (i < n) {
            const long r = r0 + i;
            float x, y, w, h;
            rr_generate_bbox(rois + r * 5, reg + r * 4, scale, x, y, w, h);
            o0 = x / div;                                // pred_bbox[:, :4] / scale on the host: IEEE division
            o1 = y / div;
            o2 = w / div;
            o3 = h / div;
            sc = scores[r];
            cl = clses[r] + 1.0f;
            keep = !filter || sc > thr;
        }
        int total;
        const int pos = base0 + run + rr_block_rank<DET_THREADS / 64>(keep, wave_cnt, total);
        if (keep && pos < K) rr_store_row6(dst + (long)pos * 6, o0, o1, o2, o3, sc, cl);
        run += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) count[f] = min(base0 + run, K);
}

// One workgroup per frame: the first count[f] rows of rows[f] ordered by score descending, equal scores in input order — the
// keys and the network of sort_rows_kernel (refine.hip).  The network runs over the frame's own power of two.
//   out_off == NULL: out is [B,K,6]; the sorted rows lead frame f's block, rows behind them get class -1 (padding).
//   out_off != NULL: out is packed ([out_rows,6]); frame f's rows start at row out_off[f] (exclusive prefix of count).
//   xyxy: write (x, y, x + w, y + h, ...) — the xywh -> xyxy step in front of soft_nms (rrnet_operator.py:222-223).
__global__ __launch_bounds__(DET_SORT_THREADS) void sort_frames_kernel(const float *rows, const int *count, const int *out_off, int K,
                                                                       int KPmax, int xyxy, float *out, long out_rows)
{
    extern __shared__ __align__(16) unsigned char smem[];
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(smem);
    const int f = blockIdx.x;
    const int n = min(max(count[f], 0), K);
    int KP = 2;
    while (KP < n) KP <<= 1;
    if (KP > KPmax) KP = KPmax;                          // K <= KPmax by the launcher: never taken, keeps LDS indices bounded
    const float *src = rows + (long)f * K * 6;
    rr_sort_rows6_keys<DET_SORT_THREADS>(src, n, keys, KP);
    const long start = out_off ? min(max((long)out_off[f], 0l), out_rows) : (long)f * K;
    const int nw = (int)min((long)n, out_rows - start);  // == n whenever out_off is the prefix of count
    float *dst = out + start * 6;
    for (int k = threadIdx.x; k < nw; k += DET_SORT_THREADS) {
        const int pos = min(max((int)rr_key_pos(keys[k]), 0), n - 1);
        const float *r = src + (long)pos * 6;
        rr_store_row6(dst + (long)k * 6, r[0], r[1], xyxy ? r[0] + r[2] : r[2], xyxy ? r[1] + r[3] : r[3], r[4], r[5]);
    }
    if (!out_off) {
        for (int k = n + threadIdx.x; k < K; k += DET_SORT_THREADS) rr_store_row6(dst + (long)k * 6, 0.f, 0.f, 0.f, 0.f, 0.f, -1.0f);
    }
}

// the grid of the three prepare launchers: one thread per output pixel, capped (the kernel strides)
inline dim3 prepare_grid(int images, int oh, int ow)
{
    const long total = (long)images * oh * ow;
    long blocks = (total + DET_THREADS - 1) / DET_THREADS;
    if (blocks > 8192) blocks = 8192;
    return dim3((unsigned)blocks);
}

}  // namespace

extern "C" int rr_prepare_frames(const unsigned char *frames, const float *mean, const float *stdv, float *out, int n, int h,
                                 int w, int oh, int ow, hipStream_t stream)
{
    RR_CHECK_ARG(n > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "rr_prepare_frames: bad dims");
    RR_CHECK_ARG(frames && mean && stdv && out, "rr_prepare_frames: null pointer");
    hipLaunchKernelGGL(prepare_frames_kernel, prepare_grid(n, oh, ow), dim3(DET_THREADS), 0, stream, frames, mean, stdv, out, n, h,
                       w, oh, ow);
    RR_CHECK_LAUNCH("rr_prepare_frames");
    return RR_OK;
}

extern "C" int rr_prepare_frames_pair(const unsigned char *frames, const float *mean, const float *stdv, float *out, int n,
                                      int h, int w, int oh, int ow, hipStream_t stream)
{
    RR_CHECK_ARG(n > 0 && h > 0 && w > 0 && oh > 0 && ow > 0, "rr_prepare_frames_pair: bad dims");
    RR_CHECK_ARG(frames && mean && stdv && out, "rr_prepare_frames_pair: null pointer");
    hipLaunchKernelGGL(prepare_frames_pair_kernel, prepare_grid(n, oh, ow), dim3(DET_THREADS), 0, stream, frames, mean, stdv, out,
                       n, h, w, oh, ow);
    RR_CHECK_LAUNCH("rr_prepare_frames_pair");
    return RR_OK;
}

extern "C" int rr_prepare_tiles(const unsigned char *frames, const long long *frame_base, const int *frame_hw, int nframes,
                                const int *tiles, int ntiles, int th, int tw, int oh, int ow, const float *mean,
                                const float *stdv, float *out, hipStream_t stream)
{
    RR_CHECK_ARG(nframes > 0 && ntiles >= 0, "rr_prepare_tiles: %d frames, %d tiles", nframes, ntiles);
    RR_CHECK_ARG(th > 0 && tw > 0 && oh > 0 && ow > 0, "rr_prepare_tiles: tile %dx%d -> %dx%d", th, tw, oh, ow);
    RR_CHECK_ARG(ntiles <= 0x7fffffff / 3, "rr_prepare_tiles: %d tiles", ntiles);
    if (ntiles == 0) return RR_OK;
    RR_CHECK_ARG(frames && frame_base && frame_hw && tiles && mean && stdv && out, "rr_prepare_tiles: null pointer");
    hipLaunchKernelGGL(prepare_tiles_kernel, prepare_grid(ntiles, oh, ow), dim3(DET_THREADS), 0, stream, frames, frame_base,
                       frame_hw, nframes, tiles, ntiles, th, tw, oh, ow, mean, stdv, out);
    RR_CHECK_LAUNCH("rr_prepare_tiles");
    return RR_OK;
}

extern "C" int rr_merge_tiles(const float *rows6, const int *count_in, const int *tiles, const int *tile_off,
                              const int *frame_hw, int nframes, int k_in, int th, int tw, int oh, int ow, float div,
                              float margin, float *merged, int *count, int k, hipStream_t stream)
{
    RR_CHECK_ARG(nframes >= 0 && nframes <= 65535 && k_in >= 0, "rr_merge_tiles: %d frames, %d rows per tile", nframes, k_in);
    RR_CHECK_ARG(th > 0 && tw > 0 && oh > 0 && ow > 0, "rr_merge_tiles: tile %dx%d, input %dx%d", th, tw, oh, ow);
    RR_CHECK_ARG(k > 0 && k <= DET_MAX_ROWS, "rr_merge_tiles: %d rows per frame (limit %d)", k, DET_MAX_ROWS);
    RR_CHECK_ARG(div > 0.0f, "rr_merge_tiles: zoom %g", (double)div);
    RR_CHECK_ARG(margin >= 0.0f, "rr_merge_tiles: margin %g", (double)margin);
    if (nframes == 0) return RR_OK;
    RR_CHECK_ARG(count_in && tiles && tile_off && frame_hw && merged && count, "rr_merge_tiles: null pointer");
    RR_CHECK_ARG(k_in == 0 || rows6, "rr_merge_tiles: null pointer");
    hipLaunchKernelGGL(merge_tiles_kernel, dim3(nframes), dim3(DET_THREADS), 0, stream, rows6, count_in, tiles, tile_off, frame_hw,
                       k_in, th, tw, (float)ow, (float)oh, div, margin, merged, count, k);
    RR_CHECK_LAUNCH("rr_merge_tiles");
    return RR_OK;
}

extern "C" int rr_merge_ctnet(const float *rows6, int nframes, int k_in, int pair, float img_w, float div, float score_thr,
                              float *merged, int *count, int k, hipStream_t stream)
{
    RR_CHECK_ARG(nframes >= 0 && k_in >= 0, "rr_merge_ctnet: negative size");
    RR_CHECK_ARG(pair == 0 || pair == 1, "rr_merge_ctnet: pair %d", pair);
    RR_CHECK_ARG(k > 0 && k <= DET_MAX_ROWS, "rr_merge_ctnet: %d rows per frame (limit %d)", k, DET_MAX_ROWS);
    RR_CHECK_ARG(div > 0.0f, "rr_merge_ctnet: scale %g", (double)div);
    if (nframes == 0) return RR_OK;
    RR_CHECK_ARG(merged && count, "rr_merge_ctnet: null pointer");
    RR_CHECK_ARG(k_in == 0 || rows6, "rr_merge_ctnet: null pointer");
    hipLaunchKernelGGL(merge_ctnet_kernel, dim3(nframes), dim3(DET_THREADS), 0, stream, rows6, nframes, k_in, pair, img_w, div,
                       score_thr, merged, count, k);
    RR_CHECK_LAUNCH("rr_merge_ctnet");
    return RR_OK;
}

extern "C" int rr_merge_scales(const float *rois, const float *reg, const float *scores, const float *clses,
                               const int *frame_off, int nframes, int r, float scale, float div, int filter, float score_thr,
                               float *merged, int *count, int k, hipStream_t stream)
{
    RR_CHECK_ARG(nframes >= 0 && r >= 0, "rr_merge_scales: negative size");
    RR_CHECK_ARG(k > 0 && k <= DET_MAX_ROWS, "rr_merge_scales: %d rows per frame (limit %d)", k, DET_MAX_ROWS);
    RR_CHECK_ARG(div > 0.0f, "rr_merge_scales: scale %g", (double)div);
    if (nframes == 0) return RR_OK;
    RR_CHECK_ARG(frame_off && merged && count, "rr_merge_scales: null pointer");
    RR_CHECK_ARG(r == 0 || (rois && reg && scores && clses), "rr_merge_scales: null pointer");
    hipLaunchKernelGGL(merge_scales_kernel, dim3(nframes), dim3(DET_THREADS), 0, stream, rois, reg, scores, clses, frame_off, r,
                       scale, div, filter, score_thr, merged, count, k);
    RR_CHECK_LAUNCH("rr_merge_scales");
    return RR_OK;
}

extern "C" int rr_sort_frames_by_score(const float *rows6, const int *count, const int *out_off, int nframes, int k, int xyxy,
                                       float *out6, long out_rows, hipStream_t stream)
{
    RR_CHECK_ARG(nframes >= 0, "rr_sort_frames_by_score: negative frame count");
    RR_CHECK_ARG(k > 0 && k <= DET_MAX_ROWS, "rr_sort_frames_by_score: %d rows per frame (limit %d)", k, DET_MAX_ROWS);
    if (nframes == 0) return RR_OK;
    RR_CHECK_ARG(rows6 && count && out6 && rows6 != out6, "rr_sort_frames_by_score: null or aliased pointer");
    RR_CHECK_ARG(out_off ? out_rows >= 0 : out_rows == (long)nframes * k, "rr_sort_frames_by_score: out6 holds %ld rows", out_rows);
    int kp = 2;
    while (kp < k) kp <<= 1;
    const size_t lds = (size_t)kp * 8;
    if (lds > 48 * 1024)
        RR_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(sort_frames_kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds),
                     "rr_sort_frames_by_score");
    hipLaunchKernelGGL(sort_frames_kernel, dim3(nframes), dim3(DET_SORT_THREADS), lds, stream, rows6, count, out_off, k, kp, xyxy,
                       out6, out_rows);
    RR_CHECK_LAUNCH("rr_sort_frames_by_score");
    return RR_OK;
}
