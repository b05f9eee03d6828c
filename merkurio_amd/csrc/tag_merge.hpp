// tag_merge.hpp -- the value of a record that already carries the tag (src/cmd_tag.rs:470-485), shared by bam.hip and sam.hip: the
// found patterns and the ','-separated items of the existing Z value, sort_unstable + dedup (Rust's String order = bytewise), joined
// by ','.  The kernels that size a kept record and the ones that write it enumerate that merge the same way: "the smallest item
// that is greater than the previous one", found by a scan over both lists -- quadratic in the number of items, which is a handful
// (values above kBamMergeBytes are left to the host path).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mk {

constexpr uint32_t kBamMergeBytes = 2048;

__device__ __forceinline__ int bam_cmp(const uint8_t *a, uint32_t na, const uint8_t *b, uint32_t nb) {
    const uint32_t m = min(na, nb);
    for (uint32_t k = 0; k < m; ++k)
        if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
    return na < nb ? -1 : na > nb ? 1 : 0;
}
// *best = the smallest item > prev (have_prev == false: the smallest of all); false: there is none
__device__ inline bool bam_merge_next(const uint8_t *__restrict__ ex, uint32_t nex, unsigned long long f0, unsigned long long f1,
                                      const uint32_t *__restrict__ found_pat, const uint8_t *__restrict__ pat_bytes, const uint32_t *__restrict__ pat_off,
                                      bool have_prev, const uint8_t *prev, uint32_t nprev, const uint8_t **best, uint32_t *nbest) {
    bool have = false;
    const uint8_t *bp = nullptr;
    uint32_t bn = 0;
    auto offer = [&](const uint8_t *p, uint32_t n) {
        if (have_prev && bam_cmp(p, n, prev, nprev) <= 0) return;
        if (!have || bam_cmp(p, n, bp, bn) < 0) have = true, bp = p, bn = n;
    };
    for (unsigned long long f = f0; f < f1; ++f) {
        const uint32_t pt = found_pat[f];
        offer(pat_bytes + pat_off[pt], pat_off[pt + 1] - pat_off[pt]);
    }
    for (uint32_t a = 0; a <= nex;) {  // (an empty value has been taken for "no tag" before: nex > 0; "a,,b" holds an empty item)
        uint32_t b = a;
        while (b < nex && ex[b] != ',') ++b;
        offer(ex + a, b - a);
        a = b + 1;
    }
    *best = bp, *nbest = bn;
    return have;
}

}  // namespace mk
