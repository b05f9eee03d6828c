// xz_kernel_edges.h -- the buffer edges of mk_xz_decode_kernel (xz_inflate.hip), one constant a line so that tests/xz_cases.py reads
// them from here and places a match source, a literal run and a chunk boundary on, one before and one after each.
#pragma once
#include <stdint.h>

namespace mkz {

constexpr uint32_t kXzRefillDwords = 64;  // compressed bytes reach the wave this many dwords at a time, one per lane (= the wave's lanes)
constexpr uint32_t kXzLitStage = 64;  // literals wait in the ring until this many are pending, then leave for device memory together
constexpr uint32_t kXzRing = 4096;  // bytes of the latest text kept in LDS (a power of two); serves a match when dist + len <= kXzRing

}  // namespace mkz
