// bgzf_cuts.hpp -- the cut rule of BGZF members that end at record ends (include/merkurio_hip.h) on the host: what
// mk_bgzf_record_cuts runs, and what the device cut kernel (bgzf_deflate.hip: mk_bgzf_cuts_kernel) is checked against.  Plain C++,
// no device, no library: tools/bgzf_cuts_check.cpp compiles it alone under the address and undefined-behaviour sanitizers.
#pragma once
#include <stdint.h>

#include <algorithm>

namespace mkz {

constexpr uint32_t kCutGrid = 49152;   // a cut is looked for at every multiple of this ...
constexpr uint32_t kCutReach = 16128;  // ... among the record ends of this many bytes from it (kCutGrid + kCutReach = 65280: the most text a member holds)

// rec_end[0, n_rec): non-decreasing record ends, the last one = T.  Writes cut[0, min(cap, result)) and returns how many cuts there
// are: 0, the distinct snap(k * G) for k = 1 .. ceil(T / G) - 1, T (T = 0: the one cut 0).
inline uint64_t record_cuts(const uint64_t *rec_end, uint64_t n_rec, uint64_t *cut, uint64_t cap) {
    const uint64_t T = n_rec ? rec_end[n_rec - 1] : 0, G = kCutGrid;
    uint64_t k = 0, last = 0;
    auto put = [&](uint64_t x) {
        if (k && x == last) return;  // (distinct cuts only)
        if (k < cap) cut[k] = x;
        ++k, last = x;
    };
    put(0);
    for (uint64_t x = G; x < T; x += G) {
        const uint64_t e = *std::lower_bound(rec_end, rec_end + n_rec, x);  // the smallest record end >= x (there is one: x < T)
        put(e - x < kCutReach ? e : x);
    }
    put(T);
    return k;
}

}  // namespace mkz
