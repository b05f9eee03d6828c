// xxh64.hpp -- XXH64 (the xxHash specification, "XXH64 algorithm description"), fed in pieces: a zstd frame's content checksum is the
// low 32 bits of XXH64 of its text with seed 0 (RFC 8878 3.1.1).  Four accumulators take 8 bytes each of every 32-byte stripe through
// a multiply-rotate-multiply round; they are merged, the tail goes in 8, 4 and 1 bytes at a time, and the result is avalanched.  The
// four chains are serial in the text's length and do not fold like a CRC: this runs on the host, over the text as it is downloaded.
#pragma once
#include <stdint.h>
#include <string.h>

namespace mkz {

struct Xxh64 {
    static constexpr uint64_t P1 = 0x9E3779B185EBCA87ull, P2 = 0xC2B2AE3D27D4EB4Full, P3 = 0x165667B19E3779F9ull, P4 = 0x85EBCA77C2B2AE63ull,
                              P5 = 0x27D4EB2F165667C5ull;
    uint64_t v1, v2, v3, v4, total = 0;
    uint8_t held[32];
    uint32_t n_held = 0;
    explicit Xxh64(uint64_t seed = 0) : v1(seed + P1 + P2), v2(seed + P2), v3(seed), v4(seed - P1) {}
    static uint64_t rotl(uint64_t x, int r) { return x << r | x >> (64 - r); }
    static uint64_t le64(const uint8_t *p) {
        uint64_t v = 0;
        for (int i = 7; i >= 0; --i) v = v << 8 | p[i];
        return v;
    }
    static uint64_t round(uint64_t acc, uint64_t in) { return rotl(acc + in * P2, 31) * P1; }
    static uint64_t merge(uint64_t h, uint64_t v) { return (h ^ round(0, v)) * P1 + P4; }
    void stripe(const uint8_t *p) { v1 = round(v1, le64(p)), v2 = round(v2, le64(p + 8)), v3 = round(v3, le64(p + 16)), v4 = round(v4, le64(p + 24)); }
    void update(const uint8_t *p, uint64_t n) {
        total += n;
        if (n_held) {
            const uint32_t take = (uint32_t)(n < 32 - n_held ? n : 32 - n_held);
            memcpy(held + n_held, p, take);
            n_held += take, p += take, n -= take;
            if (n_held < 32) return;
            stripe(held);
            n_held = 0;
        }
        for (; n >= 32; p += 32, n -= 32) stripe(p);
        if (n) memcpy(held, p, n), n_held = (uint32_t)n;
    }
    uint64_t digest() const {
        uint64_t h;
        if (total >= 32) {
            h = rotl(v1, 1) + rotl(v2, 7) + rotl(v3, 12) + rotl(v4, 18);
            h = merge(merge(merge(merge(h, v1), v2), v3), v4);
        } else {
            h = v3 + P5;  // (v3 = the seed)
        }
        h += total;
        const uint8_t *p = held;
        uint32_t n = n_held;
        for (; n >= 8; p += 8, n -= 8) h = rotl(h ^ round(0, le64(p)), 27) * P1 + P4;
        if (n >= 4) {
            const uint64_t w = (uint64_t)p[0] | (uint64_t)p[1] << 8 | (uint64_t)p[2] << 16 | (uint64_t)p[3] << 24;
            h = rotl(h ^ w * P1, 23) * P2 + P3, p += 4, n -= 4;
        }
        for (; n; ++p, --n) h = rotl(h ^ *p * P5, 11) * P1;
        h ^= h >> 33, h *= P2, h ^= h >> 29, h *= P3, h ^= h >> 32;
        return h;
    }
};

}  // namespace mkz
