// VisDrone result and annotation files on the device for gfx950: bytes of many files -> float64 rows (rr_text_line_counts,
// rr_text_lines, rr_text_parse) and float32 rows -> the bytes the operators' write_results write (rr_text_format_len,
// rr_text_format).  The digit logic is csrc/textcodec.h, shared with the host loops at the end of this file; the contract
// stands in include/rrnet_hip.h, tests/text_cases.py restates it.  Compiled with -ffp-contract=off (the codec holds one
// floating-point operation, an IEEE division; nothing may fuse around it).
//
// Lines: mark -> counts per block -> offsets (the caller's prefix sum) -> scatter.  A workgroup owns RR_TEXT_BLOCK_BYTES bytes,
// a thread 16 consecutive ones; a byte starts a line when the byte before it is '\n'.  The ranks inside a workgroup come from a
// wave scan and one LDS exchange, so the positions come out in byte order whatever the dispatch order.  Byte loads only.
// Parse and format run one thread per line / row: lines are ~50 bytes, the work is integer digit arithmetic and the launches
// are bound by their byte loads and stores.  rr_text_format stages the contiguous output range of a workgroup's 256 rows in
// LDS and stores it 16 bytes at a time.
#include "common.h"
#include "rrnet_hip.h"
#include "textcodec.h"

static_assert(RR_TEXT_MAX_ROW == rr_text::MAX_ROW, "RR_TEXT_MAX_ROW must be the longest row of the three layouts");
static_assert(rr_text::MAX_ROW_0 == 165 && rr_text::MAX_ROW_12 == 137, "row bounds derived from |v| < 2^63");
static_assert(RR_TEXT_LINE_FLAGGED == rr_text::LINE_FLAGGED && RR_TEXT_LINE_SURPLUS == rr_text::LINE_SURPLUS, "line_flag bits");
static_assert(RR_TEXT_BLOCK_BYTES == 256 * 16, "a workgroup of 256 threads owns 16 bytes per thread");

namespace {

constexpr int T = 256;
constexpr int PER = 16;
constexpr long TEXT_MAX = 1L << 40;
constexpr long ROWS_MAX = (1L << 31) - 1;

__device__ __forceinline__ int count_starts(const unsigned char *text, long n, long lo)
{
    int c = 0;
    for (int i = 0; i < PER; ++i)
        if (lo + i < n && rr_text::line_starts(text, n, lo + i)) ++c;
    return c;
}

__global__ __launch_bounds__(T) void line_counts_kernel(const unsigned char *text, long n, int *block_count)
{
    __shared__ int part[T / 64];
    const long lo = ((long)blockIdx.x * T + threadIdx.x) * PER;
    const int c = wave_sum_i(count_starts(text, n, lo));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(T) void line_scatter_kernel(const unsigned char *text, long n, const long *block_off, long nlines,
                                                         long *line_pos)
{
    __shared__ int part[T / 64];
    const long lo = ((long)blockIdx.x * T + threadIdx.x) * PER;
    const int c = count_starts(text, n, lo);
    int incl = c;                                   // inclusive scan inside the wave
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) part[threadIdx.x >> 6] = incl;
    __syncthreads();
    long at = block_off[blockIdx.x] + (incl - c);
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) at += part[w];
    if (c == 0) return;
    for (int i = 0; i < PER; ++i)
        if (lo + i < n && rr_text::line_starts(text, n, lo + i)) {
            if (at >= 0 && at < nlines) line_pos[at] = lo + i;
            ++at;
        }
}

// file_line_off[f] = the number of lines that start before file_off[f]: a lower bound in the sorted positions
__global__ __launch_bounds__(T) void file_lines_kernel(const long *line_pos, long nlines, const long *file_off, int nfiles,
                                                       long *file_line_off)
{
    const int f = blockIdx.x * T + threadIdx.x;
    if (f > nfiles) return;
    const long key = file_off[f];
    long lo = 0, hi = nlines;
    while (lo < hi) {
        const long mid = lo + (hi - lo) / 2;
        if (line_pos[mid] < key) lo = mid + 1;
        else hi = mid;
    }
    file_line_off[f] = lo;
}

__global__ __launch_bounds__(T) void parse_kernel(const unsigned char *text, long n, const long *line_pos, long nlines, int ncol,
                                                  double *rows, int *line_flag)
{
    const long l = (long)blockIdx.x * T + threadIdx.x;
    if (l >= nlines) return;
    const long pos = line_pos[l];
    double *row = rows + l * ncol;
    int fl = rr_text::LINE_FLAGGED;
    if (pos >= 0 && pos < n) fl = rr_text::get_line(text + pos, text + n, ncol, row);
    else
        for (int c = 0; c < ncol; ++c) row[c] = 0.0;
    line_flag[l] = fl;
}

__global__ __launch_bounds__(T) void format_len_kernel(const float *rows6, long nrows, int layout, int clamp, int *len,
                                                       int *row_flag)
{
    const long r = (long)blockIdx.x * T + threadIdx.x;
    if (r >= nrows) return;
    float v[6];
    for (int i = 0; i < 6; ++i) v[i] = rows6[r * 6 + i];
    const int n = rr_text::put_row(v, layout, clamp, nullptr);
    len[r] = n < 0 ? 0 : n;
    row_flag[r] = n < 0;
}

// the row's slot [byte_off[r], byte_off[r+1]) must be exactly the row's length and lie inside the buffer, else nothing is written
__device__ __forceinline__ int row_slot(const float *v, int layout, int clamp, const long *byte_off, long r, long lo, long hi,
                                        long *at)
{
    const int n = rr_text::put_row(v, layout, clamp, nullptr);
    const long o = byte_off[r];
    *at = o;
    return (n > 0 && o >= lo && o + n <= hi && byte_off[r + 1] - o == n) ? n : 0;
}

// A workgroup owns the contiguous output range of its 256 rows: every thread formats its row into LDS, then the range goes
// out 16 bytes at a time (bytes at its two ragged ends).  Measured against per-row byte stores straight to memory on 128 808
// rows / 7.6 MB: 0.019 ms against 0.045 ms; equal (0.019 ms) on one 9000-row frame.
__global__ __launch_bounds__(T) void format_staged_kernel(const float *rows6, long nrows, int layout, int clamp,
                                                          const long *byte_off, unsigned char *out, long out_bytes)
{
    __shared__ __attribute__((aligned(16))) unsigned char stage[T * RR_TEXT_MAX_ROW + 16];
    const long r0 = (long)blockIdx.x * T;
    const long r1 = r0 + T < nrows ? r0 + T : nrows;
    const long base = byte_off[r0], lim = byte_off[r1];
    if (base < 0 || lim < base || lim > out_bytes || lim - base > (long)T * RR_TEXT_MAX_ROW) return;   // uniform: inconsistent offsets
    const int span = (int)(lim - base);
    unsigned char *g = out + base;
    const int shift = (int)(reinterpret_cast<size_t>(g) & 15);     // LDS and global addresses agree modulo 16
    const long r = r0 + threadIdx.x;
    if (r < r1) {
        float v[6];
        for (int i = 0; i < 6; ++i) v[i] = rows6[r * 6 + i];
        long at;
        if (row_slot(v, layout, clamp, byte_off, r, base, lim, &at))
            rr_text::put_row(v, layout, clamp, reinterpret_cast<char *>(stage + shift + (at - base)));
    }
    __syncthreads();
    int head = (16 - shift) & 15;
    if (head > span) head = span;
    const int nvec = (span - head) / 16;
    const int tail = head + nvec * 16;
    if ((int)threadIdx.x < head) g[threadIdx.x] = stage[shift + threadIdx.x];
    for (int i = threadIdx.x; i < nvec; i += T)
        *reinterpret_cast<uint4 *>(g + head + 16 * i) = *reinterpret_cast<const uint4 *>(stage + shift + head + 16 * i);
    if (tail + (int)threadIdx.x < span) g[tail + threadIdx.x] = stage[shift + tail + threadIdx.x];
}

int check_format_args(const char *who, const float *rows6, long nrows, int layout, int clamp)
{
    RR_CHECK_ARG(nrows >= 0 && nrows <= ROWS_MAX, "%s: %ld rows (limit 2^31 - 1)", who, nrows);
    RR_CHECK_ARG(layout >= 0 && layout <= 2, "%s: layout %d (0 RRNet, 1 CenterNet, 2 RetinaNet)", who, layout);
    RR_CHECK_ARG(clamp == 0 || clamp == 1, "%s: clamp %d (0 or 1)", who, clamp);
    RR_CHECK_ARG(nrows == 0 || rows6 != nullptr, "%s: null pointer", who);
    return RR_OK;
}

}  // namespace

extern "C" int rr_text_line_blocks(long nbytes)
{
    return nbytes <= 0 || nbytes > TEXT_MAX ? 0 : (int)((nbytes + RR_TEXT_BLOCK_BYTES - 1) / RR_TEXT_BLOCK_BYTES);
}

extern "C" int rr_text_line_counts(const unsigned char *text, long nbytes, int *block_count, hipStream_t stream)
{
    RR_CHECK_ARG(nbytes >= 0 && nbytes <= TEXT_MAX, "rr_text_line_counts: %ld bytes (limit 2^40)", nbytes);
    if (nbytes == 0) return RR_OK;
    RR_CHECK_ARG(text != nullptr && block_count != nullptr, "rr_text_line_counts: null pointer");
    hipLaunchKernelGGL(line_counts_kernel, dim3(rr_text_line_blocks(nbytes)), dim3(T), 0, stream, text, nbytes, block_count);
    RR_CHECK_LAUNCH("rr_text_line_counts");
    return RR_OK;
}

extern "C" int rr_text_lines(const unsigned char *text, long nbytes, const long *file_off, int nfiles, const long *block_off,
                             long nlines, long *line_pos, long *file_line_off, hipStream_t stream)
{
    RR_CHECK_ARG(nbytes >= 0 && nbytes <= TEXT_MAX, "rr_text_lines: %ld bytes (limit 2^40)", nbytes);
    RR_CHECK_ARG(nlines >= 0 && nlines <= ROWS_MAX, "rr_text_lines: %ld lines (limit 2^31 - 1)", nlines);
    RR_CHECK_ARG(nfiles >= 0, "rr_text_lines: %d files", nfiles);
    RR_CHECK_ARG(file_off != nullptr && file_line_off != nullptr, "rr_text_lines: null pointer");
    if (nbytes > 0 && nlines > 0) {
        RR_CHECK_ARG(text != nullptr && block_off != nullptr && line_pos != nullptr, "rr_text_lines: null pointer");
        hipLaunchKernelGGL(line_scatter_kernel, dim3(rr_text_line_blocks(nbytes)), dim3(T), 0, stream, text, nbytes, block_off,
                           nlines, line_pos);
        RR_CHECK_LAUNCH("rr_text_lines");
    }
    hipLaunchKernelGGL(file_lines_kernel, dim3(rr_cdiv((long)nfiles + 1, T)), dim3(T), 0, stream, line_pos, nlines, file_off,
                       nfiles, file_line_off);
    RR_CHECK_LAUNCH("rr_text_lines");
    return RR_OK;
}

extern "C" int rr_text_parse(const unsigned char *text, long nbytes, const long *line_pos, long nlines, int ncol, double *rows,
                             int *line_flag, hipStream_t stream)
{
    RR_CHECK_ARG(nbytes >= 0 && nbytes <= TEXT_MAX, "rr_text_parse: %ld bytes (limit 2^40)", nbytes);
    RR_CHECK_ARG(nlines >= 0 && nlines <= ROWS_MAX, "rr_text_parse: %ld lines (limit 2^31 - 1)", nlines);
    RR_CHECK_ARG(ncol >= 1 && ncol <= RR_TEXT_MAX_COLS, "rr_text_parse: %d columns (1..%d)", ncol, RR_TEXT_MAX_COLS);
    if (nlines == 0) return RR_OK;
    RR_CHECK_ARG(text != nullptr && line_pos != nullptr && rows != nullptr && line_flag != nullptr, "rr_text_parse: null pointer");
    hipLaunchKernelGGL(parse_kernel, dim3(rr_cdiv(nlines, T)), dim3(T), 0, stream, text, nbytes, line_pos, nlines, ncol, rows,
                       line_flag);
    RR_CHECK_LAUNCH("rr_text_parse");
    return RR_OK;
}

extern "C" int rr_text_format_len(const float *rows6, long nrows, int layout, int clamp, int *len, int *row_flag,
                                  hipStream_t stream)
{
    if (int rc = check_format_args("rr_text_format_len", rows6, nrows, layout, clamp)) return rc;
    if (nrows == 0) return RR_OK;
    RR_CHECK_ARG(len != nullptr && row_flag != nullptr, "rr_text_format_len: null pointer");
    hipLaunchKernelGGL(format_len_kernel, dim3(rr_cdiv(nrows, T)), dim3(T), 0, stream, rows6, nrows, layout, clamp, len, row_flag);
    RR_CHECK_LAUNCH("rr_text_format_len");
    return RR_OK;
}

extern "C" int rr_text_format(const float *rows6, long nrows, int layout, int clamp, const long *byte_off, unsigned char *out,
                              long out_bytes, hipStream_t stream)
{
    if (int rc = check_format_args("rr_text_format", rows6, nrows, layout, clamp)) return rc;
    RR_CHECK_ARG(out_bytes >= 0 && out_bytes <= TEXT_MAX, "rr_text_format: %ld bytes (limit 2^40)", out_bytes);
    if (nrows == 0 || out_bytes == 0) return RR_OK;
    RR_CHECK_ARG(byte_off != nullptr && out != nullptr, "rr_text_format: null pointer");
    hipLaunchKernelGGL(format_staged_kernel, dim3(rr_cdiv(nrows, T)), dim3(T), 0, stream, rows6, nrows, layout, clamp, byte_off, out,
                       out_bytes);
    RR_CHECK_LAUNCH("rr_text_format");
    return RR_OK;
}

// ---- the same codec in plain host loops, for the tests that run without a device ------------------------------------

extern "C" int rr_text_lines_host(const unsigned char *text, long nbytes, const long *file_off, int nfiles, long max_lines,
                                  long *line_pos, long *file_line_off, long *nlines)
{
    RR_CHECK_ARG(nbytes >= 0 && nbytes <= TEXT_MAX, "rr_text_lines_host: %ld bytes (limit 2^40)", nbytes);
    RR_CHECK_ARG(nfiles >= 0 && file_off != nullptr && file_line_off != nullptr && nlines != nullptr && (nbytes == 0 || text != nullptr),
                 "rr_text_lines_host: bad arguments");
    long l = 0;
    int f = 0;
    for (long i = 0; i < nbytes; ++i) {
        for (; f <= nfiles && file_off[f] <= i; ++f) file_line_off[f] = l;
        if (!rr_text::line_starts(text, nbytes, i)) continue;
        if (line_pos != nullptr && l < max_lines) line_pos[l] = i;
        ++l;
    }
    for (; f <= nfiles; ++f) file_line_off[f] = l;
    *nlines = l;
    return RR_OK;
}

extern "C" int rr_text_parse_host(const unsigned char *text, long nbytes, const long *line_pos, long nlines, int ncol,
                                  double *rows, int *line_flag)
{
    RR_CHECK_ARG(nbytes >= 0 && nbytes <= TEXT_MAX, "rr_text_parse_host: %ld bytes (limit 2^40)", nbytes);
    RR_CHECK_ARG(nlines >= 0 && nlines <= ROWS_MAX, "rr_text_parse_host: %ld lines (limit 2^31 - 1)", nlines);
    RR_CHECK_ARG(ncol >= 1 && ncol <= RR_TEXT_MAX_COLS, "rr_text_parse_host: %d columns (1..%d)", ncol, RR_TEXT_MAX_COLS);
    RR_CHECK_ARG(nlines == 0 || (text != nullptr && line_pos != nullptr && rows != nullptr && line_flag != nullptr),
                 "rr_text_parse_host: null pointer");
    for (long l = 0; l < nlines; ++l) {
        const long pos = line_pos[l];
        if (pos >= 0 && pos < nbytes) {
            line_flag[l] = rr_text::get_line(text + pos, text + nbytes, ncol, rows + l * ncol);
        } else {
            for (int c = 0; c < ncol; ++c) rows[l * ncol + c] = 0.0;
            line_flag[l] = rr_text::LINE_FLAGGED;
        }
    }
    return RR_OK;
}

extern "C" int rr_text_format_host(const float *rows6, long nrows, int layout, int clamp, int *len, int *row_flag,
                                   const long *byte_off, unsigned char *out, long out_bytes)
{
    if (int rc = check_format_args("rr_text_format_host", rows6, nrows, layout, clamp)) return rc;
    RR_CHECK_ARG((len == nullptr) == (row_flag == nullptr) && (out == nullptr || byte_off != nullptr) && out_bytes >= 0,
                 "rr_text_format_host: bad arguments");
    for (long r = 0; r < nrows; ++r) {
        const int n = rr_text::put_row(rows6 + r * 6, layout, clamp, nullptr);
        if (len != nullptr) {
            len[r] = n < 0 ? 0 : n;
            row_flag[r] = n < 0;
        }
        if (out != nullptr && n > 0 && byte_off[r] >= 0 && byte_off[r] + n <= out_bytes && byte_off[r + 1] - byte_off[r] == n)
            rr_text::put_row(rows6 + r * 6, layout, clamp, reinterpret_cast<char *>(out + byte_off[r]));
    }
    return RR_OK;
}
