// bzip2_harness.cpp -- merkurio_amd/csrc/codec/bzip2_serial.hpp and bzip2_stream.hpp compiled for the host and run the way
// mk_bzip2_inflate_device runs them: every bit offset searched for the two magics, the table walked into streams and blocks, every
// block decoded from its guessed start and proved by where it ends, inverse BWT, the run-length step, the block and stream CRCs.
// tests/test_bunzip2_cpu.py builds this with -fsanitize=address,undefined and checks it against Python's bz2.
//
//   bzip2_harness IN.bz2 OUT
// writes the text to OUT and prints one line: "taken=1 blocks=B streams=S unaligned=U runend=R bytes=N" (U: blocks whose magic is not
// byte-aligned, R: blocks whose last symbol is a run's count) or "taken=0 why=WORD status=K".  WORD: chain (the table of magics does not
// chain: status 0 = the walk over it says so, status 1 = a block decodes but does not end on the magic behind it, which is how a magic
// too many inside a block's data shows), block (K = the decoder's status), walk (K likewise), block-crc, stream-crc.
// Exit status 0 either way (a sanitizer report is what makes it non-zero).
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "codec/bzip2_serial.hpp"
#include "codec/bzip2_stream.hpp"

using namespace mkz;

static int refuse(const char *why, int status = 0) {
    printf("taken=0 why=%s status=%d\n", why, status);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> file;
    uint8_t tmp[65536];
    for (size_t k; (k = fread(tmp, 1, sizeof tmp, f)) > 0;) file.insert(file.end(), tmp, tmp + k);
    fclose(f);
    const uint64_t n = file.size();
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    // (an exact copy for the search and the walk, so that ASan sees a read behind the file; a padded one for the bit reader)
    std::vector<uint8_t> padded(file);
    padded.resize((n + kBzStreamPad + 3) & ~3ull, 0);
    std::vector<BzMarker> markers;
    bz2_find_markers(file.data(), n, markers);
    std::vector<BzPlanBlock> blocks;
    std::vector<BzPlanStream> streams;
    if (!bz2_plan(file.data(), n, markers, blocks, streams)) {
        fclose(out);
        return refuse("chain");
    }
    std::vector<uint8_t> text;
    std::vector<uint32_t> block_crc(blocks.size());
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; ++i) table[i] = bz2_crc_table_entry(i);
    uint32_t unaligned = 0, runend = 0;
    Bz2Tables *T = new Bz2Tables;
    std::vector<uint8_t> sel(kBzSelBytes);
    for (size_t k = 0; k < blocks.size(); ++k) {
        const uint32_t cap = blocks[k].level * 100000u;
        std::vector<uint8_t> ll8(cap), pre(cap);
        std::vector<uint32_t> tt(cap), is_count(cap / 32 + 1);
        BzBits<BzHostWords> bits;
        bits.w = BzHostWords{padded.data(), padded.size() / 4};
        bits.n_bits = n * 8;
        bits.seek(blocks[k].bit);
        BzSerialMtf mtf;
        BzSerialOut o{ll8.data()};
        Bz2Block h;
        if (bz2_decode_block(bits, blocks[k].level, *T, sel.data(), mtf, o, h)) {
            delete T, fclose(out);
            return refuse("block", h.status);
        }
        if (h.end_bit != blocks[k].end_bit) {
            delete T, fclose(out);
            return refuse("chain", 1);
        }
        unaligned += (blocks[k].bit & 7) != 0;
        bz2_prefix(T->hist);
        bz2_scatter_serial(ll8.data(), h.nblock, T->hist, tt.data());
        uint64_t len = 0;
        if (int st = bz2_walk(tt.data(), h.nblock, h.orig_ptr, pre.data(), is_count.data(), &len)) {
            delete T, fclose(out);
            return refuse("walk", st);
        }
        runend += is_count[(h.nblock - 1) >> 5] >> ((h.nblock - 1) & 31u) & 1u;
        const size_t at = text.size();
        text.resize(at + len);
        bz2_expand_serial(pre.data(), is_count.data(), h.nblock, text.data() + at);
        // the CRC in 7 pieces, folded: what the CRC kernel does with 64
        const uint64_t piece = (len + 6) / 7;
        uint32_t crc = 0;
        for (uint64_t p0 = 0, j = 0; j < 7; ++j, p0 += piece) {
            const uint64_t a = std::min(p0, len), b = std::min(p0 + piece, len);
            uint32_t c = j == 0 ? 0xffffffffu : 0u;
            for (uint64_t i = a; i < b; ++i) c = bz2_crc_byte(c, text[at + i], table);
            crc = j == 0 ? c : bz2_crc_mulmod(crc, bz2_crc_x_pow_bytes(b - a)) ^ c;
        }
        crc = ~crc;
        if (crc != h.crc) {
            delete T, fclose(out);
            return refuse("block-crc");
        }
        block_crc[k] = crc;
    }
    delete T;
    for (const BzPlanStream &s : streams) {
        uint32_t c = 0;
        for (uint32_t k = 0; k < s.n_blocks; ++k) c = bz2_stream_crc_fold(c, block_crc[s.first_block + k]);
        if (c != s.crc) {
            fclose(out);
            return refuse("stream-crc");
        }
    }
    if (!text.empty()) fwrite(text.data(), 1, text.size(), out);
    fclose(out);
    printf("taken=1 blocks=%zu streams=%zu unaligned=%u runend=%u bytes=%zu\n", blocks.size(), streams.size(), unaligned, runend, text.size());
    return 0;
}
