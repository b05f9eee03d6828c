// crc64.hpp -- the two checks of the xz container that are CRCs, for g++ and hipcc: CRC-32 (IEEE 802.3) and CRC-64 (ECMA-182), both
// reflected, initial value and final xor all ones, as the xz file format 1.0.4 (section 6) uses them.  One template over the width:
// a byte step, a table entry, and what folds the values of pieces into the value of the whole (xz_inflate.hip: mk_xz_check_kernel;
// tests/helpers/xz_harness.cpp runs the same fold on the host).
//
// Reflected: bit W-1 of a register is x^0.  The register after a piece B that starts from register s is reg(B, 0) ^ s * x^(8 |B|) mod
// P, so the raw registers of pieces (the first one started from all ones, the others from 0) fold left to right with one
// multiplication each -- bz2_crc_mulmod's scheme (bzip2_serial.hpp), mirrored.
#pragma once
#include <stdint.h>

#include "deflate_common.hpp"

namespace mkz {

template <typename T>
struct XzCrc;
template <>
struct XzCrc<uint32_t> {
    static constexpr uint32_t poly = 0xEDB88320u;
};
template <>
struct XzCrc<uint64_t> {
    static constexpr uint64_t poly = 0xC96C5795D7870F42ull;  // x^64 + x^62 + x^57 + ... + 1 (ECMA-182), bits reversed
};

template <typename T>
MKZ_HD T xz_crc_table_entry(uint32_t i) {
    T c = i;
    for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ XzCrc<T>::poly : c >> 1;
    return c;
}
template <typename T>
MKZ_HD T xz_crc_byte(T c, uint32_t byte, const T *table) {
    return table[(uint32_t)(c & 0xff) ^ byte] ^ (c >> 8);
}
// a * b mod P
template <typename T>
MKZ_HD T xz_crc_mulmod(T a, T b) {
    constexpr int W = sizeof(T) * 8;
    T r = 0;
    for (int i = 0; i < W; ++i) {  // b's coefficient of x^i is bit W-1-i
        if (b >> (W - 1 - i) & 1) r ^= a;
        a = (a & 1) ? (a >> 1) ^ XzCrc<T>::poly : a >> 1;
    }
    return r;
}
// x^(8 n) mod P
template <typename T>
MKZ_HD T xz_crc_x_pow_bytes(uint64_t n) {
    constexpr int W = sizeof(T) * 8;
    T r = (T)1 << (W - 1), sq = (T)1 << (W - 9);
    for (; n; n >>= 1) {
        if (n & 1) r = xz_crc_mulmod<T>(r, sq);
        sq = xz_crc_mulmod<T>(sq, sq);
    }
    return r;
}
// the register after a piece of `len` bytes whose own register (started from 0) is `piece`, in front of which the register was `before`
template <typename T>
MKZ_HD T xz_crc_fold(T before, T piece, uint64_t len) {
    return xz_crc_mulmod<T>(before, xz_crc_x_pow_bytes<T>(len)) ^ piece;
}

// bytewise, for the host (the container's header, index and footer CRC-32s; the harness's reference)
template <typename T>
inline T xz_crc_bytes(const uint8_t *p, uint64_t n, T start = ~(T)0) {
    T c = start;
    for (uint64_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 1) ? (c >> 1) ^ XzCrc<T>::poly : c >> 1;
    }
    return c;
}
inline uint32_t xz_crc32(const uint8_t *p, uint64_t n) { return ~xz_crc_bytes<uint32_t>(p, n); }

}  // namespace mkz
