// xz_windows_harness.cpp -- xz_chain.hpp on the host, a stand-alone program for tests/test_unxz_windows_cpu.py (built with
// -fsanitize=address,undefined and run directly) and for the GPU tests' window, block and stream counts (built without).
//   xz_windows_harness stream FILE OUT WINDOW_BYTES TEXT_CAP SPREAD
//        the file as mk_xz_stream_begin / _next take it: the plan of xz_chain.hpp, then every window decoded from a COPY OF ONLY THAT
//        WINDOW'S BYTES with the rebased table, by the same lzma2_decode_block, in the launch order; the text of the windows delivered
//        to OUT; one line of key=value: taken, state, status, windows, planned, blocks, streams, consumed, text, largest, and per window
//        its blocks (window-blocks) and its lc + lp (window-lclp).  TEXT_CAP 0: no cap
//   xz_windows_harness plan FILE OUT
//        xz_plan's block table: a line status= streams= lclp= text= largest= blocks=, then a row per block: in_off in_bytes text_off
//        text_bytes check_off check_kind dict_size head_off
#define main xz_harness_main  // (the one-shot harness is included for its folded<>() and slurp(); its main is not this program's)
#include "xz_harness.cpp"
#undef main

#include <string>

#include "codec/xz_chain.hpp"

namespace {

// the device's stand-in (xz_chain.hpp: Dev)
struct HostDev {
    const mkz::XzStream &S;
    std::vector<uint8_t> text, pending;
    std::string window_blocks, window_lclp;
    int decode(const mkz::XzWork &K) {
        // (a copy of exactly the window's bytes, and of exactly each block's: a read or a store past either is the sanitizer's)
        const std::vector<uint8_t> up(S.xz + K.from, S.xz + K.from + K.bytes);
        pending.assign(K.text, 0);
        std::vector<uint16_t> probs(mkz::lzma_probs(K.lclp));
        std::vector<int> status(K.blocks.size(), 0);
        for (uint32_t idx : K.order) {
            const mkz::XzBlock &B = K.blocks[idx];
            if (B.in_off + B.in_bytes > up.size() || B.check_off + mkz::xz_check_bytes(B.check_kind) > up.size() || B.text_off + B.text_bytes > pending.size()) return mkz::kXzSizes;
            std::vector<uint8_t> in(up.begin() + B.in_off, up.begin() + B.in_off + B.in_bytes), out(B.text_bytes);
            mkz::LzSerialIn src{in.data()};
            mkz::LzSerialProbs pr{probs.data()};
            mkz::LzSerialOut dst{out.data()};
            Census cs;
            uint64_t made = 0;
            int st = mkz::lzma2_decode_block(src, B.in_bytes, pr, dst, B.text_bytes, B.dict_size, K.lclp, cs, &made);
            const uint8_t *stored = up.data() + B.check_off;
            if (!st && B.check_kind == mkz::kXzCheckCrc32 && folded<uint32_t>(out.data(), out.size(), 64) != mkz::xz_le32(stored)) st = mkz::kLzCheck;
            if (!st && B.check_kind == mkz::kXzCheckCrc64 && folded<uint64_t>(out.data(), out.size(), 64) != ((uint64_t)mkz::xz_le32(stored + 4) << 32 | mkz::xz_le32(stored)))
                st = mkz::kLzCheck;
            status[idx] = st;
            if (!st && !out.empty()) memcpy(pending.data() + B.text_off, out.data(), out.size());
        }
        for (int st : status)  // the first block in file order that failed
            if (st) return st;
        window_blocks += (window_blocks.empty() ? "" : ",") + std::to_string(K.blocks.size());
        window_lclp += (window_lclp.empty() ? "" : ",") + std::to_string(K.lclp);
        return 0;
    }
    void commit(uint64_t n) { text.insert(text.end(), pending.begin(), pending.begin() + n); }
};

void write_out(const char *path, const std::vector<uint8_t> &v) {
    FILE *f = fopen(path, "wb");
    if (!f) {
        perror(path);
        exit(2);
    }
    if (!v.empty()) fwrite(v.data(), 1, v.size(), f);
    fclose(f);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "plan")) {
        const std::vector<uint8_t> xz = slurp(argv[2]);
        mkz::XzPlan P;
        const int st = mkz::xz_plan(xz.data(), xz.size(), P);
        write_out(argv[3], {});
        printf("status=%d streams=%u lclp=%u text=%llu largest=%llu blocks=%zu\n", st, P.streams, P.lclp_max, (unsigned long long)P.text_total,
               (unsigned long long)P.largest_block_text, st ? (size_t)0 : P.blocks.size());
        for (size_t k = 0; !st && k < P.blocks.size(); ++k) {
            const mkz::XzBlock &B = P.blocks[k];
            printf("%llu %llu %llu %llu %llu %u %u %llu\n", (unsigned long long)B.in_off, (unsigned long long)B.in_bytes, (unsigned long long)B.text_off,
                   (unsigned long long)B.text_bytes, (unsigned long long)B.check_off, B.check_kind, B.dict_size, (unsigned long long)P.head_off[k]);
        }
        return 0;
    }
    if (argc != 7 || strcmp(argv[1], "stream")) {
        fprintf(stderr, "usage: xz_windows_harness stream FILE OUT WINDOW_BYTES TEXT_CAP SPREAD | plan FILE OUT\n");
        return 2;
    }
    const std::vector<uint8_t> xz = slurp(argv[2]);
    const uint64_t window = strtoull(argv[4], nullptr, 10), cap = strtoull(argv[5], nullptr, 10);
    const uint32_t spread = (uint32_t)strtoul(argv[6], nullptr, 10);
    mkz::XzStream S;
    const int begun = mkz::xz_stream_open(S, xz.data(), xz.size(), window, cap ? cap : 1ull << 62, spread);
    HostDev dev{S, {}, {}, {}, {}};
    uint32_t state = 2;
    if (!begun) {
        for (uint64_t n = 0;;) {
            mkz::xz_stream_next(S, dev, &n, &state);
            if (state != 0) break;
        }
    }
    write_out(argv[3], dev.text);
    const mk_xz_stream_stats &st = S.stats;
    printf("taken=%d state=%u status=%d windows=%llu planned=%llu blocks=%llu streams=%llu consumed=%llu text=%llu largest=%llu window-blocks=%s window-lclp=%s\n", begun == 0, state,
           (int)st.status, (unsigned long long)st.windows, (unsigned long long)st.planned_windows, (unsigned long long)st.blocks, (unsigned long long)st.streams,
           (unsigned long long)st.consumed_bytes, (unsigned long long)st.text_bytes, (unsigned long long)st.largest_block_text,
           dev.window_blocks.empty() ? "-" : dev.window_blocks.c_str(), dev.window_lclp.empty() ? "-" : dev.window_lclp.c_str());
    return 0;
}
