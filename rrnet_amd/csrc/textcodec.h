// The digit routines of the VisDrone text codec, plain C++ with no HIP include: the same functions run in the kernels of
// csrc/textio.hip, in the host loops rr_text_format_host / rr_text_parse_host, and in a host compiler alone.  Both directions
// are exact in 64-bit integer arithmetic (the contract stands in include/rrnet_hip.h, tests/text_cases.py restates it):
//   format: the bytes of Python's '%f' / '%.4f' % float(v) and '%d' % int(v) for a float32 v;
//   parse:  the double pandas.read_csv(float_precision='high') and float() give for [+-]digits[.digits].
// Every put function takes a destination that may be null: it then only counts, which is how the lengths are found.
// "flag" (-1) means: the host route decides (Python raises, needs a big integer, or pandas' answer depends on the column).
#pragma once
#include <math.h>
#include <string.h>

#if defined(__HIPCC__)
#define RR_TEXT_HD __host__ __device__ inline
#else
#define RR_TEXT_HD inline
#endif

namespace rr_text {

enum { LAYOUT_RRNET = 0, LAYOUT_CENTERNET = 1, LAYOUT_RETINANET = 2 };
enum { LINE_FLAGGED = 1, LINE_SURPLUS = 2 };       // bits of rr_text_parse's line_flag

// the longest row a layout can give, from |v| < 2^63 = 9223372036854775808 (19 digits):
constexpr int MAX_F6 = 1 + 19 + 1 + 6;             // '%f':   sign, 19 digits, point, 6 decimals
constexpr int MAX_F4 = 1 + 19 + 1 + 4;             // '%.4f'
constexpr int MAX_D = 1 + 19;                      // '%d', and the difference of two ints of layout 1 (each below 2^62)
constexpr int TAIL = 7;                            // ",-1,-1\n"
constexpr int MAX_ROW_0 = 4 * MAX_F6 + MAX_F4 + MAX_D + 5 + TAIL;
constexpr int MAX_ROW_12 = 4 * MAX_D + MAX_F4 + MAX_D + 5 + TAIL;
constexpr int MAX_ROW = MAX_ROW_0 > MAX_ROW_12 ? MAX_ROW_0 : MAX_ROW_12;

RR_TEXT_HD unsigned float_bits(float v)
{
    unsigned u;
    memcpy(&u, &v, 4);
    return u;
}

RR_TEXT_HD int put_char(char c, char *dst, int at)
{
    if (dst) dst[at] = c;
    return at + 1;
}

// decimal digits of u, at least `min_digits` (zero padded) -> the new position
RR_TEXT_HD int put_u64(unsigned long long u, int min_digits, char *dst, int at)
{
    int n = 1;
    for (unsigned long long t = u; t >= 10; t /= 10) ++n;
    if (n < min_digits) n = min_digits;
    if (dst)
        for (int i = n - 1; i >= 0; --i) {
            dst[at + i] = (char)('0' + (int)(u % 10));
            u /= 10;
        }
    return at + n;
}

RR_TEXT_HD int put_i64(long long v, char *dst, int at)
{
    unsigned long long u = (unsigned long long)v;
    if (v < 0) {
        at = put_char('-', dst, at);
        u = 0ULL - u;
    }
    return put_u64(u, 1, dst, at);
}

// |v| = m * 2^e with m < 2^24 (subnormals: e = -149); false for infinity and NaN
RR_TEXT_HD bool split_float(float v, int *sign, unsigned *m, int *e)
{
    const unsigned u = float_bits(v);
    const unsigned ex = (u >> 23) & 0xffu, mant = u & 0x7fffffu;
    *sign = (int)(u >> 31);
    if (ex == 255) return false;
    *m = ex ? (mant | 0x800000u) : mant;
    *e = ex ? (int)ex - 150 : -149;
    return true;
}

// '%.{decimals}f' % float(v), decimals 4 or 6 -> the new position, or -1
RR_TEXT_HD int put_fixed(float v, int decimals, char *dst, int at)
{
    int sign, e;
    unsigned m;
    if (!split_float(v, &sign, &m, &e)) {
        if (float_bits(v) & 0x7fffffu) {            // NaN prints without its sign
            at = put_char('n', dst, at); at = put_char('a', dst, at); return put_char('n', dst, at);
        }
        if (sign) at = put_char('-', dst, at);
        at = put_char('i', dst, at); at = put_char('n', dst, at); return put_char('f', dst, at);
    }
    const unsigned long long p10 = decimals == 4 ? 10000ULL : 1000000ULL;
    unsigned long long ip, fp;
    if (e >= 0) {
        if (e > 39) return -1;                      // |v| >= 2^63
        ip = (unsigned long long)m << e;
        fp = 0;
    } else {
        const int sh = -e;
        unsigned long long q = 0;
        if (sh < 64) {
            const unsigned long long n = (unsigned long long)m * p10;          // < 2^44
            const unsigned long long half = 1ULL << (sh - 1);
            const unsigned long long rem = n & ((half << 1) - 1ULL);           // sh <= 63: half << 1 <= 2^63
            q = n >> sh;
            if (rem > half || (rem == half && (q & 1ULL))) ++q;                // round half to even, exactly
        }
        ip = q / p10;
        fp = q % p10;
    }
    if (sign) at = put_char('-', dst, at);
    at = put_u64(ip, 1, dst, at);
    at = put_char('.', dst, at);
    return put_u64(fp, decimals, dst, at);
}

// int(v): truncation towards zero; false for NaN, infinity and |v| >= 2^63
RR_TEXT_HD bool float_to_i64(float v, long long *out)
{
    int sign, e;
    unsigned m;
    if (!split_float(v, &sign, &m, &e) || e > 39) return false;
    const unsigned long long a = e >= 0 ? (unsigned long long)m << e : (-e >= 24 ? 0ULL : (unsigned long long)(m >> -e));
    *out = sign ? -(long long)a : (long long)a;
    return true;
}

// '%d' % int(v) -> the new position, or -1
RR_TEXT_HD int put_int(float v, char *dst, int at)
{
    long long i;
    if (!float_to_i64(v, &i)) return -1;
    return put_i64(i, dst, at);
}

// One result row -> its length (the final '\n' included), or -1.  r6 = six float32; clamp: v < 0 ? 0 : v on all six
// (NaN and -0.0 pass through).  Layout 1 flags a corner at or beyond 2^62, so that the difference of two fits 64 bits.
RR_TEXT_HD int put_row(const float *r6, int layout, int clamp, char *dst)
{
    float v[6];
    for (int i = 0; i < 6; ++i) v[i] = clamp && r6[i] < 0.f ? 0.f : r6[i];
    int at = 0;
    if (layout == LAYOUT_RRNET) {
        for (int i = 0; i < 4; ++i) {
            at = put_fixed(v[i], 6, dst, at);
            if (at < 0) return -1;
            at = put_char(',', dst, at);
        }
    } else {
        long long c[4];
        for (int i = 0; i < 4; ++i) {
            if (!float_to_i64(layout == LAYOUT_CENTERNET ? rintf(v[i]) : v[i], &c[i])) return -1;
            if (layout == LAYOUT_CENTERNET && (c[i] >= (1LL << 62) || c[i] <= -(1LL << 62))) return -1;
        }
        if (layout == LAYOUT_CENTERNET) {
            c[2] -= c[0];
            c[3] -= c[1];
        }
        for (int i = 0; i < 4; ++i) {
            at = put_i64(c[i], dst, at);
            at = put_char(',', dst, at);
        }
    }
    at = put_fixed(v[4], 4, dst, at);
    if (at < 0) return -1;
    at = put_char(',', dst, at);
    at = put_int(v[5], dst, at);
    if (at < 0) return -1;
    const char tail[TAIL + 1] = ",-1,-1\n";
    for (int i = 0; i < TAIL; ++i) at = put_char(tail[i], dst, at);
    return at;
}

constexpr int MAX_DIGITS = 17;
RR_TEXT_HD bool is_digit(unsigned char c) { return c >= '0' && c <= '9'; }

// One field [+-]? digit* ('.' digit*)? with at least one digit, ended by ',', '\r', '\n' or `end` -> the bytes consumed (the
// terminator not among them), or -1.  Value = (double)D / 10^k, D the integer of all digits, k the digits behind the point:
// one IEEE division of two exact doubles (D < 2^53, k <= 22).  A zero written with a minus sign is flagged, and so is a field of
// more than MAX_DIGITS digit characters, leading zeros included: pandas' parser reads 17 of them and drops the rest.
RR_TEXT_HD long get_field(const unsigned char *p, const unsigned char *end, double *out)
{
    const unsigned char *s = p;
    bool neg = false;
    if (p < end && (*p == '+' || *p == '-')) {
        neg = *p == '-';
        ++p;
    }
    unsigned long long d = 0;
    int digits = 0, k = 0;
    for (; p < end && is_digit(*p); ++p, ++digits) {
        if (digits >= MAX_DIGITS) return -1;
        d = d * 10 + (unsigned)(*p - '0');
        if (d >= (1ULL << 53)) return -1;
    }
    if (p < end && *p == '.') {
        ++p;
        for (; p < end && is_digit(*p); ++p, ++digits, ++k) {
            if (k >= 22 || digits >= MAX_DIGITS) return -1;
            d = d * 10 + (unsigned)(*p - '0');
            if (d >= (1ULL << 53)) return -1;
        }
    }
    if (digits == 0) return -1;
    if (p < end && *p != ',' && *p != '\r' && *p != '\n') return -1;
    if (neg && d == 0) return -1;
    double p10 = 1.0;
    for (int i = 0; i < k; ++i) p10 *= 10.0;        // 10^0 .. 10^22 are exact doubles, and so is every product on the way
    const double v = (double)d / p10;
    *out = neg ? -v : v;
    return (long)(p - s);
}

// One line from p (its end of line lies before `end`): the first ncol fields -> row[ncol] -> 0, LINE_SURPLUS (one empty
// surplus field: a trailing comma), or LINE_FLAGGED: a field flagged, fewer than ncol fields, any other surplus, or a '\r'
// that no '\n' follows (pandas ends a line there).  Fields that were not parsed are 0.
RR_TEXT_HD int get_line(const unsigned char *p, const unsigned char *end, int ncol, double *row)
{
    for (int c = 0; c < ncol; ++c) row[c] = 0.0;
    for (int c = 0; c < ncol; ++c) {
        const long n = get_field(p, end, &row[c]);
        if (n < 0) return LINE_FLAGGED;
        p += n;
        const bool comma = p < end && *p == ',';
        if (comma) ++p;
        if (c + 1 < ncol) {
            if (!comma) return LINE_FLAGGED;
            continue;
        }
        if (p < end && *p == '\r') {
            if (!(p + 1 < end && p[1] == '\n')) return LINE_FLAGGED;
        } else if (p < end && *p != '\n') {
            return LINE_FLAGGED;
        }
        return comma ? LINE_SURPLUS : 0;
    }
    return LINE_FLAGGED;                            // ncol <= 0
}

// byte i starts a line that is not blank: it follows a '\n' (or starts the buffer) and is neither '\n' nor the '\r' of "\r\n"
RR_TEXT_HD bool line_starts(const unsigned char *text, long n, long i)
{
    if (i > 0 && text[i - 1] != '\n') return false;
    const unsigned char c = text[i];
    if (c == '\n') return false;
    return !(c == '\r' && i + 1 < n && text[i + 1] == '\n');
}

}  // namespace rr_text
