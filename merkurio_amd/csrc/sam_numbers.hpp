// sam_numbers.hpp -- the numbers of a SAM line as the device reads them when it turns the line into a BAM record (sam.hip).
// Compiled by hipcc for the kernels and by g++ for the CPU harness that checks it against strtoll / strtof
// (tests/helpers/sam_numbers_harness.cpp), the way codec/inflate_serial.hpp is.
//
// The host path's field_int / field_float (cli/bam_out.cpp) are strtoll-like and strtof: they take junk and wrap on overflow.  These do
// not imitate that: each converts ONE plain spelling and says "not converted" for everything else -- the window is then the host's.
//   sam_int        [+-] 1-18 digits, nothing else                      -> the value (fits a signed 64-bit integer: 10^18 < 2^63)
//   sam_cigar_len  1-9 digits                                          -> the value (999 999 999 < 2^32: no wrap to imitate)
//   sam_float      [+-] digits [. digits] [e|E [+-] digits], where the digits with the point dropped are an integer m < 2^24 and
//                  the net power of ten e (the exponent less the digits behind the point) has |e| <= 10
//                  -> (double)m * 10^e or (double)m / 10^-e, then one conversion to float.
// Why sam_float is strtof's value: m and 10^|e| (<= 10^10 < 2^53) are exact doubles, so the one multiplication or division is the
// correctly rounded 53-bit value of the decimal number; rounding a correctly rounded p-bit result of a single operation on exact
// operands to q bits gives the correctly rounded q-bit result when p >= 2q + 2 (Figueroa, "When is double rounding innocuous?",
// 1995), and 53 >= 2 * 24 + 2.  Results lie between 10^-10 and 1.7 * 10^17 or are zero: no float overflow or denormal.  The sign
// is applied last, so "-0" is -0.0f as with strtof.  field_float hands strtof the first 63 bytes of a field only, so a longer spelling
// (zeros in front, a padded exponent) is not converted either: what strtof sees of it is not what is written.
#pragma once
#include <stdint.h>

#if defined(__HIP__)  // (the HIP language: a translation unit with kernels)
#define MK_NUM_FN __host__ __device__ inline
#else
#define MK_NUM_FN inline
#endif

namespace mk {

MK_NUM_FN bool sam_int(const uint8_t *p, uint32_t n, long long *out) {
    uint32_t i = 0;
    bool neg = false;
    if (i < n && (p[i] == '+' || p[i] == '-')) neg = p[i++] == '-';
    const uint32_t digits = n - i;
    if (digits < 1 || digits > 18) return false;
    unsigned long long v = 0;
    for (; i < n; ++i) {
        const uint32_t d = (uint32_t)p[i] - '0';
        if (d > 9) return false;
        v = v * 10 + d;
    }
    *out = neg ? -(long long)v : (long long)v;
    return true;
}

MK_NUM_FN bool sam_cigar_len(const uint8_t *p, uint32_t n, uint32_t *out) {
    if (n < 1 || n > 9) return false;
    uint32_t v = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t d = (uint32_t)p[i] - '0';
        if (d > 9) return false;
        v = v * 10 + d;
    }
    *out = v;
    return true;
}

MK_NUM_FN double sam_pow10(uint32_t e) {  // e <= 10: exact
    double r = 1.0;
    for (uint32_t k = 0; k < e; ++k) r *= 10.0;  // (every partial product is an integer below 2^53)
    return r;
}

MK_NUM_FN bool sam_float(const uint8_t *p, uint32_t n, float *out) {
    if (n > 63) return false;
    uint32_t i = 0;
    bool neg = false;
    if (i < n && (p[i] == '+' || p[i] == '-')) neg = p[i++] == '-';
    uint32_t m = 0, int_digits = 0, frac_digits = 0;
    for (; i < n && (uint32_t)p[i] - '0' <= 9; ++i, ++int_digits) {
        m = m * 10 + ((uint32_t)p[i] - '0');
        if (m >= (1u << 24)) return false;
    }
    if (!int_digits) return false;
    if (i < n && p[i] == '.') {
        ++i;
        for (; i < n && (uint32_t)p[i] - '0' <= 9; ++i, ++frac_digits) {
            m = m * 10 + ((uint32_t)p[i] - '0');
            if (m >= (1u << 24)) return false;
        }
        if (!frac_digits) return false;
    }
    int e = 0;
    if (i < n && (p[i] == 'e' || p[i] == 'E')) {
        ++i;
        bool eneg = false;
        if (i < n && (p[i] == '+' || p[i] == '-')) eneg = p[i++] == '-';
        uint32_t ed = 0;
        for (; i < n && (uint32_t)p[i] - '0' <= 9; ++i, ++ed) {
            e = e * 10 + (int)((uint32_t)p[i] - '0');  // (at most 61 digits get here ...)
            if (e > 1000) return false;                // (... and no more than four of them are significant)
        }
        if (!ed) return false;
        if (eneg) e = -e;
    }
    if (i != n) return false;
    e -= (int)frac_digits;
    if (e < -10 || e > 10) return false;
    const double v = e >= 0 ? (double)m * sam_pow10((uint32_t)e) : (double)m / sam_pow10((uint32_t)-e);
    const float f = (float)v;
    *out = neg ? -f : f;
    return true;
}

// the hash of a reference name: the host builds the table of the @SQ names with it, sam.hip looks RNAME / RNEXT up with it (FNV-1a)
MK_NUM_FN uint32_t sam_name_hash(const uint8_t *p, uint32_t n) {
    uint32_t h = 2166136261u;
    for (uint32_t i = 0; i < n; ++i) h = (h ^ p[i]) * 16777619u;
    return h;
}

}  // namespace mk
