// test harness: what the CLI's readers make of a gzip file's members (merkurio_amd/csrc/cli/bgzf_in.cpp through WindowSource::open), WITHOUT
// a device or the library: the verdict (BGZF all the way through, or a gzip file for the serial reader), the member table, the text the
// members inflate to (WindowSource::more_into), and for every query m0:m_end:want the run bgzf_run_end() cuts and that run's table
// re-based to its first member (bgzf_rebased).
// usage: harness <file> [<m0>:<m_end>:<want> ...]
// prints "kind bgzf|gzip|plain", "members <n>", "m <data_off> <out_off> <data_len> <isize> <crc>" per member, "text <bytes> <fnv-1a 64>",
// then per query "run <m0> <m_end> <want> <m1>" followed by "r <data_off> <out_off> <data_len> <isize> <crc>" per member of the run
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "io.hpp"
using namespace cli;

static void print_member(const char *what, const mk_bgzf_member &b) {
    printf("%s %" PRIu64 " %" PRIu64 " %u %u %u\n", what, b.data_off, b.out_off, b.data_len, b.isize, b.crc);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    try {
        WindowSource ws;
        ws.open(argv[1]);
        printf("kind %s\n", ws.is_bgzf() ? "bgzf" : ws.is_gzip() ? "gzip" : "plain");
        const std::vector<mk_bgzf_member> &mem = ws.bgzf_members();
        printf("members %zu\n", mem.size());
        for (const mk_bgzf_member &b : mem) print_member("m", b);
        if (ws.is_bgzf()) {
            std::vector<char> text;
            uint64_t n = 0, h = 1469598103934665603ull;
            while (ws.more_into(text, n, 1u << 16)) {
            }
            for (uint64_t i = 0; i < n; ++i) h = (h ^ (uint8_t)text[i]) * 1099511628211ull;
            printf("text %" PRIu64 " %" PRIx64 "\n", n, h);
        }
        for (int a = 2; a < argc; ++a) {
            char *q = argv[a];
            const size_t m0 = (size_t)strtoull(q, &q, 10), m_end = (size_t)strtoull(q + 1, &q, 10);
            const uint64_t want = strtoull(q + 1, &q, 10);
            const size_t m1 = bgzf_run_end(mem, m0, m_end, want);
            printf("run %zu %zu %" PRIu64 " %zu\n", m0, m_end, want, m1);
            if (m1 > m0)
                for (const mk_bgzf_member &b : bgzf_rebased(mem.data() + m0, m1 - m0, mem[m0].data_off, mem[m0].out_off)) print_member("r", b);
        }
    } catch (const Error &e) {
        printf("#error %s\n", e.what());
    }
    return 0;
}
