// The number parsing of the SAM -> BAM kernels (merkurio_amd/csrc/sam_numbers.hpp) compiled for the host, beside the C library's
// strtof / strtoll / strtoul on the same spelling (tests/test_sam_bam_window_cpu.py).
//   sam_numbers_harness FILE     FILE: one "<kind>\t<spelling>" per line, kind f (float), i (integer) or c (CIGAR length)
// prints per line  "<converted 0|1> <ours> <whole 0|1> <libc's>":  floats as the hex of their bits, integers in decimal; `whole` =
// the C library took the entire spelling (and it is not empty).  Our parser gets the spelling in a buffer of exactly its length, so
// that a read past the end is ASan's to see.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "sam_numbers.hpp"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    std::string line;
    while (std::getline(in, line)) {
        if (line.size() < 2 || line[1] != '\t') return 3;
        const char kind = line[0];
        const std::string sp = line.substr(2);
        std::vector<uint8_t> exact(sp.begin(), sp.end());  // (data() of an empty vector is never read)
        const uint8_t *p = exact.data();
        const uint32_t n = (uint32_t)exact.size();
        char *end = nullptr;
        if (kind == 'f') {
            float ours = 0;
            const bool ok = mk::sam_float(p, n, &ours);
            const float ref = strtof(sp.c_str(), &end);
            uint32_t a, b;
            memcpy(&a, &ours, 4), memcpy(&b, &ref, 4);
            printf("%d %08x %d %08x\n", ok ? 1 : 0, ok ? a : 0u, (!sp.empty() && *end == 0) ? 1 : 0, b);
        } else if (kind == 'i') {
            long long ours = 0;
            const bool ok = mk::sam_int(p, n, &ours);
            const long long ref = strtoll(sp.c_str(), &end, 10);
            printf("%d %lld %d %lld\n", ok ? 1 : 0, ok ? ours : 0ll, (!sp.empty() && *end == 0) ? 1 : 0, ref);
        } else if (kind == 'c') {
            uint32_t ours = 0;
            const bool ok = mk::sam_cigar_len(p, n, &ours);
            const unsigned long ref = strtoul(sp.c_str(), &end, 10);
            printf("%d %u %d %lu\n", ok ? 1 : 0, ok ? ours : 0u, (!sp.empty() && *end == 0) ? 1 : 0, ref);
        } else {
            return 3;
        }
    }
    return 0;
}
