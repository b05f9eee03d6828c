// bgzf_cuts_check.cpp -- the host cut rule (merkurio_amd/csrc/codec/bgzf_cuts.hpp, what mk_bgzf_record_cuts runs) as a stand-alone
// program for the address and undefined-behaviour sanitizers: host code only, no device, no library.
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o bgzf_cuts_check tools/bgzf_cuts_check.cpp && ./bgzf_cuts_check
//
// Shapes: the ones of tests/bgzf_cut_cases.py (no records, one byte, 331-byte records, ends on and around a grid point and the reach's
// edge, a 200 000-byte record between short ones, a last snap that is T) and 2 000 seeded random mixes.  Every result is written into a
// buffer of exactly its size (and once into one that is one entry short) and checked: first 0, last T, strictly increasing, gaps of
// at most 65 280, every cut a record end or inside a record longer than the reach.
#include <stdio.h>
#include <stdlib.h>

#include <random>
#include <vector>

#include "../merkurio_amd/csrc/codec/bgzf_cuts.hpp"

static int failures = 0;

static void check(const std::vector<uint64_t> &lens, const char *name) {
    std::vector<uint64_t> e(lens.size());
    uint64_t at = 0;
    for (size_t i = 0; i < lens.size(); ++i) e[i] = at += lens[i];
    const uint64_t T = at, G = mkz::kCutGrid, L = G + mkz::kCutReach;
    const uint64_t n = mkz::record_cuts(e.data(), e.size(), nullptr, 0);  // (sizing call: nothing is written)
    std::vector<uint64_t> cut(n), shorter(n ? n - 1 : 0);
    bool ok = mkz::record_cuts(e.data(), e.size(), cut.data(), cut.size()) == n && n >= 1 && n <= T / G + 2;
    ok = ok && mkz::record_cuts(e.data(), e.size(), shorter.data(), shorter.size()) == n;
    ok = ok && cut[0] == 0 && cut[n - 1] == T;
    for (uint64_t k = 1; k < n && ok; ++k) {
        ok = cut[k] > cut[k - 1] && cut[k] - cut[k - 1] <= L && shorter[k - 1] == cut[k - 1];
        if (k + 1 < n && ok) {
            const size_t r = (size_t)(std::lower_bound(e.begin(), e.end(), cut[k]) - e.begin());
            if (e[r] != cut[k]) ok = e[r] - (r ? e[r - 1] : 0) > mkz::kCutReach && cut[k] % G == 0;
        }
    }
    if (!ok) fprintf(stderr, "FAILED: %s\n", name), ++failures;
}

static std::vector<uint64_t> fill(uint64_t total, uint64_t rec = 331) {
    std::vector<uint64_t> v(total / rec, rec);
    if (total % rec) v.push_back(total % rec);
    return v;
}
static std::vector<uint64_t> join(std::vector<uint64_t> a, const std::vector<uint64_t> &b) {
    a.insert(a.end(), b.begin(), b.end());
    return a;
}

int main() {
    const uint64_t G = mkz::kCutGrid, L = G + mkz::kCutReach;
    check({}, "no records");
    check({0, 0}, "empty records");
    check({1}, "one byte");
    check(fill(3 * G + 100), "331-byte records");
    check({G, 500}, "end at G");
    check({G - 1, 500, 500}, "end at G - 1");
    check({1000, L - 1001, 700}, "end at G + reach - 1");
    check({1000, L - 1000, 700}, "end at G + reach");
    check(join(join(fill(46000), {200000}), fill(40000)), "long record");
    check(join(fill(2 * G - 100), {400}), "last snap is T");
    check({100, 2 * G + 20000, 50}, "two grid points in one record");
    std::mt19937_64 rng(20261019);
    for (int it = 0; it < 2000; ++it) {
        std::vector<uint64_t> lens((size_t)(rng() % 1500) + 1);
        const int kind = (int)(rng() % 3);
        for (auto &x : lens) x = kind == 0 ? rng() % 700 + 1 : kind == 1 ? rng() % (3 * G) + 1 : (rng() % 200 == 0 ? rng() % (5 * G) + mkz::kCutReach - 3 : rng() % 400 + 1);
        check(lens, "random mix");
    }
    printf("%s\n", failures ? "FAILED" : "ok: every shape");
    return failures ? 1 : 0;
}
