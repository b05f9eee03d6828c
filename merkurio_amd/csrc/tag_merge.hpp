// tag_merge.hpp -- what `tag` decides and writes per record, shared by bam.hip and sam.hip: whether the record is kept
// (src/cmd_tag.rs:457-467) and the value of its tag -- the distinct found patterns joined by ',' (:484-490; ascending pattern index =
// sort_unstable order of the sorted unique pattern list), or, for a record that already carries the tag (:470-485), the found
// patterns and the ','-separated items of the existing Z value, sort_unstable + dedup (Rust's String order = bytewise), joined by ','.
// The kernels that size a kept record (tag_value_len) and the ones that write it (tag_value_put) enumerate that merge the same way:
// "the smallest item that is greater than the previous one", found by a scan over both lists -- quadratic in the number of items,
// which is a handful (values above kBamMergeBytes are left to the host path).
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

// keep or drop: -m keeps the records with a hit, -v (without -m) the ones without, neither keeps all
__device__ __forceinline__ bool tag_keeps(uint32_t filter_matching, uint32_t invert, bool has) { return filter_matching ? has : (invert ? !has : true); }

// the length of record i's value: its found patterns [f0, f1), merged with the existing value ex[0, ex_n) when ex_n != 0
__device__ __forceinline__ uint32_t tag_value_len(const uint8_t *__restrict__ ex, uint32_t ex_n, unsigned long long f0, unsigned long long f1,
                                                  const uint32_t *__restrict__ found_pat, const uint32_t *__restrict__ pat_off,
                                                  const uint8_t *__restrict__ pat_bytes) {
    uint32_t vlen = 0;
    if (ex_n == 0) {
        for (unsigned long long k = f0; k < f1; ++k) {
            const uint32_t pt = found_pat[k];
            vlen += pat_off[pt + 1] - pat_off[pt];
        }
        if (f1 > f0) vlen += (uint32_t)(f1 - f0) - 1;
    } else {
        const uint8_t *prev = nullptr, *it;
        uint32_t nprev = 0, nit, items = 0;
        while (bam_merge_next(ex, ex_n, f0, f1, found_pat, pat_bytes, pat_off, items != 0, prev, nprev, &it, &nit)) vlen += nit, prev = it, nprev = nit, ++items;
        vlen += items - 1;
    }
    return vlen;
}

// that value's bytes at t; returns where they end (the caller's terminator goes there)
__device__ __forceinline__ uint8_t *tag_value_put(uint8_t *t, const uint8_t *__restrict__ ex, uint32_t ex_n, unsigned long long f0, unsigned long long f1,
                                                  const uint32_t *__restrict__ found_pat, const uint32_t *__restrict__ pat_off,
                                                  const uint8_t *__restrict__ pat_bytes) {
    if (ex_n == 0) {
        for (unsigned long long f = f0; f < f1; ++f) {
            if (f > f0) *t++ = ',';
            const uint32_t pt = found_pat[f];
            const uint32_t a = pat_off[pt], b = pat_off[pt + 1];
            for (uint32_t j = a; j < b; ++j) *t++ = pat_bytes[j];
        }
    } else {  // (the old field stays where it is: the merged value is appended like any other)
        const uint8_t *prev = nullptr, *it;
        uint32_t nprev = 0, nit, items = 0;
        while (bam_merge_next(ex, ex_n, f0, f1, found_pat, pat_bytes, pat_off, items != 0, prev, nprev, &it, &nit)) {
            if (items) *t++ = ',';
            for (uint32_t j = 0; j < nit; ++j) *t++ = it[j];
            prev = it, nprev = nit, ++items;
        }
    }
    return t;
}

}  // namespace mk
