// bgzf_cuts.hpp -- the cut rule of BGZF members that end at record ends (include/merkurio_hip.h) on the host: what
// mk_bgzf_record_cuts runs, and what the device cut kernel (bgzf_deflate.hip: mk_bgzf_cuts_kernel) is checked against.  Plain C++,
// no device, no library: tools/bgzf_cuts_check.cpp compiles it alone under the address and undefined-behaviour sanitizers.
// The rule is written once over its two constants (grid, reach); the zstd frames of mk_zstd_deflate_records use it with their own pair
// (mk_zstd_record_cuts, zstd_deflate.hip: mk_zstd_cuts_kernel).
#pragma once
#include <stdint.h>

#include <algorithm>

namespace mkz {

constexpr uint32_t kCutGrid = 49152;   // a cut is looked for at every multiple of this ...
constexpr uint32_t kCutReach = 16128;  // ... among the record ends of this many bytes from it (kCutGrid + kCutReach = 65280: the most text a member holds)
// the same for zstd frames (MK_ZSTD_CUT_GRID; grid + reach = MK_ZSTD_FRAME_TEXT_MAX = 131072, the most text a zstd block holds)
constexpr uint32_t kZsCutGrid = 114688, kZsCutReach = 16384;

// rec_end[0, n_rec): non-decreasing record ends, the last one = T.  Writes cut[0, min(cap, result)) and returns how many cuts there
// are: 0, the distinct snap(k * G) for k = 1 .. ceil(T / G) - 1, T (T = 0: the one cut 0).
template <uint32_t kGrid, uint32_t kReach>
inline uint64_t record_cuts_of(const uint64_t *rec_end, uint64_t n_rec, uint64_t *cut, uint64_t cap) {
    const uint64_t T = n_rec ? rec_end[n_rec - 1] : 0, G = kGrid;
    uint64_t k = 0, last = 0;
    auto put = [&](uint64_t x) {
        if (k && x == last) return;  // (distinct cuts only)
        if (k < cap) cut[k] = x;
        ++k, last = x;
    };
    put(0);
    for (uint64_t x = G; x < T; x += G) {
        const uint64_t e = *std::lower_bound(rec_end, rec_end + n_rec, x);  // the smallest record end >= x (there is one: x < T)
        put(e - x < kReach ? e : x);
    }
    put(T);
    return k;
}
inline uint64_t record_cuts(const uint64_t *rec_end, uint64_t n_rec, uint64_t *cut, uint64_t cap) {
    return record_cuts_of<kCutGrid, kCutReach>(rec_end, n_rec, cut, cap);
}
inline uint64_t zstd_record_cuts(const uint64_t *rec_end, uint64_t n_rec, uint64_t *cut, uint64_t cap) {
    return record_cuts_of<kZsCutGrid, kZsCutReach>(rec_end, n_rec, cut, cap);
}

#ifdef __HIPCC__
// ---- the same rule on the device: one lane per grid point (the cut kernels of bgzf_deflate.hip and zstd_deflate.hip) ----
// rec_end[0, n_rec): the ends of the records of a text of T bytes, non-decreasing (a record that is not kept repeats the end in front
// of it), rec_end[n_rec - 1] = T.  Grid point k (x = k * kGrid, k = 1 .. K - 1, K = ceil(T / kGrid)) snaps to the first record
// end e >= x if e < x + kReach, and stays at x otherwise.  One binary search for a lane's own cut and one for the cut behind it:
// snap(x) lies in [x, x + kReach) and kReach <= kGrid, so the cuts of two grid points never meet -- the only cut that can coincide
// with another is the last one with T, which is what lane K - 1 looks at.  Piece k = [cut k, cut k + 1): off[k], len[k]; *n_pieces = K,
// or K - 1 when the last grid point snapped to T.
template <uint32_t kReach>
__device__ __forceinline__ uint64_t snap_cut(const unsigned long long *__restrict__ rec_end, uint64_t n_rec, uint64_t x) {
    uint64_t lo = 0, hi = n_rec;  // the first record end >= x: there is one, x < T = rec_end[n_rec - 1]
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        if (rec_end[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    const uint64_t e = lo < n_rec ? rec_end[lo] : x;
    return e - x < kReach ? e : x;
}
template <uint32_t kGrid, uint32_t kReach>
__device__ __forceinline__ void cut_ranges(const unsigned long long *__restrict__ rec_end, uint64_t n_rec, uint64_t T, uint32_t n_grid,
                                           unsigned long long *__restrict__ off, uint32_t *__restrict__ len, uint32_t *__restrict__ n_pieces) {
    static_assert(kReach <= kGrid, "the cuts of two grid points cannot coincide");
    for (uint32_t k = blockIdx.x * blockDim.x + threadIdx.x; k < n_grid; k += gridDim.x * blockDim.x) {
        const uint64_t a = k ? snap_cut<kReach>(rec_end, n_rec, (uint64_t)k * kGrid) : 0;
        const uint64_t b = k + 1 < n_grid ? snap_cut<kReach>(rec_end, n_rec, (uint64_t)(k + 1) * kGrid) : T;
        off[k] = a;
        len[k] = (uint32_t)(b - a);
        if (k + 1 == n_grid) *n_pieces = b > a ? n_grid : n_grid - 1;
    }
}
#endif

}  // namespace mkz
