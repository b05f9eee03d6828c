// The number formatting of the BAM -> SAM kernels (merkurio_amd/csrc/bam_numbers.hpp) compiled for the host, beside the C++ library's
// std::to_string and snprintf("%g") on the same value (tests/test_bam_sam_window_cpu.py).
//   bam_numbers_harness i FILE       FILE: one signed 64-bit integer per line -> per line "<ours> <std::to_string>"
//   bam_numbers_harness f FILE       FILE: the bits of one float (hex) per line -> per line "<taken 0|1> <ours or -> <%g>"
//   bam_numbers_harness x THREADS WHAT
//        every positive float of the binades the rule can take (exponent fields 113 ... 146) and of the two next to them on each side
//        (111, 112, 147, 148), WHAT = all: every mantissa; WHAT = some: every mantissa of the two edge binades on each side of the rule
//        (111 ... 114, 145 ... 148), and per other binade every mantissa whose scaled remainder is within 2 of one half plus 2^20 random
//        ones.  A float the formatter takes must give %g's bytes; one it refuses must be one %g writes in exponent notation.  Every 64th
//        value is checked with its sign set too.  Prints "checked N taken T bad B" and the first few bad ones.
// The length pass sizes a buffer of exactly that many bytes for the writing pass, so that a byte too many is ASan's to see; the
// two passes must agree.
#include <atomic>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "bam_numbers.hpp"

static bool ours_float(uint32_t bits, std::string &out) {
    mk::BamText<false> len{nullptr, 0};
    if (!mk::bam_put_float(len, bits)) return false;
    std::vector<uint8_t> buf(len.at);
    mk::BamText<true> w{buf.data(), 0};
    if (!mk::bam_put_float(w, bits) || w.at != len.at) abort();
    out.assign(buf.begin(), buf.end());
    return true;
}

static std::string libc_float(uint32_t bits) {
    float f;
    memcpy(&f, &bits, 4);
    char b[64];
    snprintf(b, sizeof(b), "%g", (double)f);
    return b;
}

// "" if the formatter and %g agree about this float, else what is wrong
static std::string check_float(uint32_t bits) {
    std::string o;
    const bool taken = ours_float(bits, o);
    const std::string ref = libc_float(bits);
    const bool fixed = ref.find('e') == std::string::npos && ref.find('n') == std::string::npos;  // (no exponent, not inf / nan)
    char b[160];
    if (taken && o != ref) {
        snprintf(b, sizeof(b), "%08x: ours %s, %%g %s", bits, o.c_str(), ref.c_str());
        return b;
    }
    if (!taken && fixed) {
        snprintf(b, sizeof(b), "%08x: refused, %%g %s", bits, ref.c_str());
        return b;
    }
    return "";
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    if (mode == "i" || mode == "f") {
        std::ifstream in(argv[2]);
        std::string line;
        while (std::getline(in, line)) {
            if (mode == "i") {
                const long long v = strtoll(line.c_str(), nullptr, 10);
                mk::BamText<false> len{nullptr, 0};
                mk::bam_put_int(len, v);
                std::vector<uint8_t> buf(len.at);
                mk::BamText<true> w{buf.data(), 0};
                mk::bam_put_int(w, v);
                if (w.at != len.at) abort();
                printf("%s %s\n", std::string(buf.begin(), buf.end()).c_str(), std::to_string(v).c_str());
            } else {
                const uint32_t bits = (uint32_t)strtoul(line.c_str(), nullptr, 16);
                std::string o;
                const bool taken = ours_float(bits, o);
                printf("%d %s %s\n", taken ? 1 : 0, taken ? o.c_str() : "-", libc_float(bits).c_str());
            }
        }
        return 0;
    }
    if (mode != "x" || argc != 4) return 2;
    const unsigned T = (unsigned)std::max(1, atoi(argv[2]));
    const bool all = std::string(argv[3]) == "all";
    std::vector<uint32_t> binades;
    for (uint32_t ex = 111; ex <= 148; ++ex) binades.push_back(ex);
    std::atomic<uint64_t> checked{0}, taken{0}, bad{0};
    std::mutex mu;
    std::vector<std::string> first_bad;
    auto one = [&](uint32_t bits, uint64_t &c, uint64_t &tk) {
        for (uint32_t sign = 0; sign <= ((bits & 63u) == 0 ? 1u : 0u); ++sign) {
            const uint32_t b = bits | sign << 31;
            std::string why = check_float(b);
            ++c;
            if (!why.empty()) {
                ++bad;
                std::lock_guard<std::mutex> lk(mu);
                if (first_bad.size() < 10) first_bad.push_back(why);
            } else {
                mk::BamText<false> len{nullptr, 0};
                tk += mk::bam_put_float(len, b) ? 1 : 0;
            }
        }
    };
    std::vector<std::thread> th;
    for (unsigned t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            uint64_t c = 0, tk = 0;
            std::mt19937 rng(1234 + t);
            for (uint32_t ex : binades) {
                const bool edge = ex <= 114 || ex >= 145;
                const uint32_t lo = (uint32_t)((1ull << 23) * t / T), hi = (uint32_t)((1ull << 23) * (t + 1) / T);
                if (all || edge) {
                    for (uint32_t f = lo; f < hi; ++f) one(ex << 23 | f, c, tk);
                    continue;
                }
                // near a tie: with s = 150 - ex and N = m * 10^k (k = the power that gives six digits), N mod 2^s within 2 of 2^(s - 1)
                const uint32_t s = 150 - ex;
                for (uint32_t f = lo; f < hi; ++f) {
                    unsigned long long N = f | (1u << 23);
                    while ((N >> s) < 100000ull) N *= 10;
                    const unsigned long long rem = N & ((1ull << s) - 1), half = 1ull << (s - 1);
                    if ((rem > half ? rem - half : half - rem) <= 2) one(ex << 23 | f, c, tk);
                }
                for (uint32_t k = 0; k < (1u << 20) / T + 1; ++k) one(ex << 23 | (rng() & 0x7FFFFFu), c, tk);
            }
            checked += c, taken += tk;
        });
    for (auto &x : th) x.join();
    printf("checked %" PRIu64 " taken %" PRIu64 " bad %" PRIu64 "\n", checked.load(), taken.load(), bad.load());
    for (const std::string &s : first_bad) printf("%s\n", s.c_str());
    return 0;
}
