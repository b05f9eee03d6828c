// bam_numbers.hpp -- the numbers of a BAM record as the device writes them when it turns the record into a SAM line (bam.hip).
// Compiled by hipcc for the kernels and by g++ for the CPU harness that checks it against std::to_string and snprintf("%g")
// (tests/helpers/bam_numbers_harness.cpp), the way sam_numbers.hpp is.
//
// Everything goes through a BamText<kWrite>: the length pass (kWrite = false) and the writing pass (kWrite = true) run the SAME code,
// the first only advances the position -- so the sizes of pass 1 are the bytes of pass 2.
//
//   bam_put_int    plain decimal of a signed 64-bit value (std::to_string).  Digits are COUNTED by a fixed sequence of compares with
//                  powers of ten (9 for values below 2^32, which every field of a BAM record is; 19 above) and WRITTEN from the last
//                  digit forwards by dividing by the constant 10; INT64_MIN is negated as an unsigned value.
//   bam_put_float  what snprintf("%g", (double)f) gives -- six significant digits, correctly rounded from the exact binary value,
//                  ties to even, trailing zeros and a bare point removed -- for the floats where that takes 64-bit integers only:
//                    +-0                       "0" / "-0"
//                    finite, normal, and the decimal exponent X of the value ROUNDED to six digits lies in -4 ... 5 (%g's fixed notation).
//                  Such a value is m * 2^e with 2^23 <= m < 2^24 and -37 <= e <= -4 (6.1e-5 <= |v| < 2^20).  With 10^X <= |v| < 10^(X + 1) (X found
//                  by multiplying m by ten until the quotient has six digits; X >= -5, so the product stays below 2^24 * 10^10 < 2^58 and is exact),
//                    N = m * 10^(5 - X),  q = N >> -e  (six digits),  r = N mod 2^-e  against  2^(-e - 1):  above, or equal with q odd, rounds up.
//                  q = 10^6 after rounding becomes 10^5 with X + 1: 999999.5 leaves the rule (%g prints 1e+06), and the floats just below
//                  0.0001 that round up to it enter it.  Everything else -- exponent notation, inf, nan, subnormals -- is NOT formatted: the
//                  function returns false and the window is the host path's.
#pragma once
#include <stdint.h>

#if defined(__HIP__)  // (the HIP language: a translation unit with kernels)
#define MK_BNUM_FN __host__ __device__ inline
#else
#define MK_BNUM_FN inline
#endif

namespace mk {

template <bool kWrite>
struct BamText {
    uint8_t *out;  // kWrite = false: never touched
    uint64_t at;
    MK_BNUM_FN void put(uint32_t c) {
        if (kWrite) out[at] = (uint8_t)c;
        ++at;
    }
};

MK_BNUM_FN uint32_t bam_digits32(uint32_t v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
MK_BNUM_FN uint32_t bam_digits64(unsigned long long v) {
    if (v <= 0xFFFFFFFFull) return bam_digits32((uint32_t)v);
    uint32_t d = 10;  // (v >= 2^32 > 10^9)
    for (unsigned long long p = 10000000000ull; d < 20 && v >= p; p *= 10) ++d;  // (p reaches 10^19 < 2^64 at most)
    return d;
}

template <bool kWrite>
MK_BNUM_FN void bam_put_uint(BamText<kWrite> &t, unsigned long long v) {
    const uint32_t d = bam_digits64(v);
    if (kWrite) {
        uint8_t *e = t.out + t.at + d;
        if (v <= 0xFFFFFFFFull) {
            uint32_t x = (uint32_t)v;
            for (uint32_t k = 0; k < d; ++k) *--e = (uint8_t)('0' + x % 10u), x /= 10u;
        } else {
            for (uint32_t k = 0; k < d; ++k) *--e = (uint8_t)('0' + v % 10u), v /= 10u;
        }
    }
    t.at += d;
}
template <bool kWrite>
MK_BNUM_FN void bam_put_int(BamText<kWrite> &t, long long v) {
    if (v < 0) {
        t.put('-');
        bam_put_uint(t, 0ull - (unsigned long long)v);
    } else {
        bam_put_uint(t, (unsigned long long)v);
    }
}

// the float with these bits as "%g"; false: outside the rule above, nothing usable was written
template <bool kWrite>
MK_BNUM_FN bool bam_put_float(BamText<kWrite> &t, uint32_t bits) {
    const uint32_t ex = (bits >> 23) & 0xFFu, frac = bits & 0x7FFFFFu;
    if (ex == 0 && frac == 0) {
        if (bits >> 31) t.put('-');
        t.put('0');
        return true;
    }
    if (ex < 113 || ex > 146) return false;  // (e = ex - 150 outside -37 ... -4: subnormal, below 6.1e-5, 2^20 and above, inf, nan)
    const uint32_t s = 150u - ex;            // 4 ... 37
    unsigned long long N = frac | (1u << 23);
    int X = 5;
    unsigned long long q = N >> s;
    if (q >= 1000000ull) return false;
    while (q < 100000ull) {
        if (X == -5) return false;
        N *= 10, --X;
        q = N >> s;
    }
    const unsigned long long rem = N & ((1ull << s) - 1), half = 1ull << (s - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    if (q == 1000000ull) q = 100000ull, ++X;
    if (X < -4 || X > 5) return false;
    uint32_t D = (uint32_t)q, nd = 6;  // nd = digits that are left when the trailing zeros go
    for (uint32_t z = D; nd > 1 && z % 10u == 0; z /= 10u) --nd;
    if (bits >> 31) t.put('-');
    if (X < 0) {
        t.put('0'), t.put('.');
        for (int k = -1; k > X; --k) t.put('0');
    }
    uint32_t p = 100000u;
    for (int k = 0; k < 6; ++k, p /= 10u) {
        if ((uint32_t)k < nd || k <= X) t.put('0' + D / p % 10u);  // (a digit behind the nd-th is a zero of the integer part)
        if (k == X && nd > (uint32_t)X + 1) t.put('.');
    }
    return true;
}

}  // namespace mk
