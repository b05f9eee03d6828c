// xz_harness.cpp -- xz_plan.hpp + lzma_serial.hpp + crc64.hpp on the host, a stand-alone program for tests/test_unxz_cpu.py (built with
// and without -fsanitize=address,undefined) and the GPU tests' block and stream counts.
//   xz_harness FILE OUT [SPREAD]   the file walked and decoded block by block as mk_xz_inflate_device does it; the text to OUT (nothing
//                                  when not taken); one line of key=value: taken, status, bytes, blocks, streams, largest, lclp, and the census
//   xz_harness --fold FILE PIECES  CRC-64 and CRC-32 of FILE bytewise, and folded from PIECES pieces as mk_xz_check_kernel folds them
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "codec/crc64.hpp"
#include "codec/lzma_serial.hpp"
#include "codec/xz_plan.hpp"

namespace {

const char *kCensusNames[mkz::kLzcKeys] = {"packet.lit",       "packet.matched-lit", "packet.match",      "packet.rep0",    "packet.rep1",  "packet.rep2",
                                           "packet.rep3",      "packet.shortrep",    "len.low",           "len.mid",        "len.high",     "slot.direct",
                                           "slot.tree",        "slot.align",         "chunk.stored-reset", "chunk.stored",   "chunk.lzma",   "chunk.state",
                                           "chunk.props",      "chunk.all",          "dist.lt-len",       "dist.at-start",  "dist.at-dict"};
struct Census {
    uint64_t n[mkz::kLzcKeys] = {};
    void hit(int k) { ++n[k]; }
};

std::vector<uint8_t> slurp(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) {
        perror(path);
        exit(2);
    }
    uint8_t buf[1 << 16];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

// the check kernel's scheme: `pieces` pieces of ceil(len / pieces) bytes, the first register started from all ones, folded
template <typename T>
T folded(const uint8_t *p, uint64_t len, uint64_t pieces) {
    T table[256];
    for (uint32_t i = 0; i < 256; ++i) table[i] = mkz::xz_crc_table_entry<T>(i);
    const uint64_t piece = (len + pieces - 1) / pieces;
    T r = 0;
    for (uint64_t j = 0; j < pieces; ++j) {
        const uint64_t a = std::min(piece * j, len), e = std::min(piece * (j + 1), len);
        T c = j == 0 ? ~(T)0 : (T)0;
        for (uint64_t i = a; i < e; ++i) c = mkz::xz_crc_byte<T>(c, p[i], table);
        r = j == 0 ? c : e == a ? r : mkz::xz_crc_fold<T>(r, c, e - a);
    }
    return ~r;
}

int decode(const std::vector<uint8_t> &xz, std::vector<uint8_t> &text, mkz::XzPlan &P, Census &cs, uint32_t spread) {
    const int planned = mkz::xz_plan(xz.data(), xz.size(), P);
    if (planned) return planned;
    if (!mkz::xz_spread_ok(P, spread)) return mkz::kXzSpread;
    text.assign(P.text_total, 0);
    std::vector<uint16_t> probs(mkz::lzma_probs(P.lclp_max));
    for (const mkz::XzBlock &B : P.blocks) {
        // (copies of exactly the block's bytes: a read or a store past either is the sanitizer's)
        std::vector<uint8_t> in(xz.begin() + B.in_off, xz.begin() + B.in_off + B.in_bytes), out(B.text_bytes);
        mkz::LzSerialIn src{in.data()};
        mkz::LzSerialProbs pr{probs.data()};
        mkz::LzSerialOut dst{out.data()};
        uint64_t made = 0;
        const int st = mkz::lzma2_decode_block(src, B.in_bytes, pr, dst, B.text_bytes, B.dict_size, P.lclp_max, cs, &made);
        if (st) return st;
        const uint8_t *stored = xz.data() + B.check_off;
        if (B.check_kind == mkz::kXzCheckCrc32 && folded<uint32_t>(out.data(), out.size(), 64) != mkz::xz_le32(stored)) return mkz::kLzCheck;
        if (B.check_kind == mkz::kXzCheckCrc64 && folded<uint64_t>(out.data(), out.size(), 64) != ((uint64_t)mkz::xz_le32(stored + 4) << 32 | mkz::xz_le32(stored)))
            return mkz::kLzCheck;
        if (!out.empty()) memcpy(text.data() + B.text_off, out.data(), out.size());
    }
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "--fold")) {
        const std::vector<uint8_t> d = slurp(argv[2]);
        const uint64_t pieces = strtoull(argv[3], nullptr, 10);
        printf("crc64=%016llx fold64=%016llx crc32=%08x fold32=%08x\n", (unsigned long long)~mkz::xz_crc_bytes<uint64_t>(d.data(), d.size()),
               (unsigned long long)folded<uint64_t>(d.data(), d.size(), pieces), (unsigned)mkz::xz_crc32(d.data(), d.size()), (unsigned)folded<uint32_t>(d.data(), d.size(), pieces));
        return 0;
    }
    if (argc != 3 && argc != 4) {
        fprintf(stderr, "usage: xz_harness FILE OUT [SPREAD] | --fold FILE PIECES\n");
        return 2;
    }
    const std::vector<uint8_t> xz = slurp(argv[1]);
    std::vector<uint8_t> text;
    mkz::XzPlan P;
    Census cs;
    const int st = decode(xz, text, P, cs, argc == 4 ? (uint32_t)strtoul(argv[3], nullptr, 10) : 1u);
    if (st) text.clear();
    FILE *f = fopen(argv[2], "wb");
    if (!f) {
        perror(argv[2]);
        return 2;
    }
    if (!text.empty()) fwrite(text.data(), 1, text.size(), f);
    fclose(f);
    printf("taken=%d status=%d bytes=%llu blocks=%llu streams=%u largest=%llu lclp=%u", st == 0, st, (unsigned long long)text.size(),
           (unsigned long long)(st == 0 ? P.blocks.size() : 0), P.streams, (unsigned long long)P.largest_block_text, P.lclp_max);
    for (int k = 0; k < mkz::kLzcKeys; ++k) printf(" %s=%llu", kCensusNames[k], (unsigned long long)cs.n[k]);
    printf("\n");
    return 0;
}
