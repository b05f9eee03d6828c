// zstd_harness.cpp -- merkurio_amd/csrc/codec/zstd_serial.hpp, zstd_plan.hpp and xxh64.hpp on the host, the phases of
// mk_zstd_inflate_device one after the other on one thread: the walk, every block's entropy decoding, the two scans, every block's
// execution, the rounds of pointer doubling (two source arrays, as on the device), the content checksums.
//     zstd_harness <in.zst> <out.bin>
// prints taken=0|1 bytes= blocks= frames= rounds= why= status= and the census of what the file exercised, one key=value each; writes
// the text (nothing where the file is not taken).  Built with the sanitizers by tests/test_unzstd_cpu.py.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "codec/xxh64.hpp"
#include "codec/zstd_plan.hpp"

using namespace mkz;

static std::vector<uint8_t> read_file(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
    fclose(f);
    return v;
}

static void census(const ZsPlan &P, const std::vector<ZsReport> &rep, const std::vector<ZsStart> &start, const std::vector<uint32_t> &ll,
                   const std::vector<uint32_t> &of) {
    const ZsCensus &c = P.census;
    const char *bt[3] = {"raw", "rle", "compressed"}, *lt[4] = {"raw", "rle", "huffman", "treeless"}, *tab[3] = {"ll", "of", "ml"},
               *md[4] = {"predefined", "rle", "fse", "repeat"};
    for (int i = 0; i < 3; ++i) printf(" block.%s=%llu", bt[i], (unsigned long long)c.block_type[i]);
    for (int i = 0; i < 4; ++i) printf(" lit.%s=%llu", lt[i], (unsigned long long)c.lit_type[i]);
    // size formats: raw / RLE have three header widths (formats 0 and 2 are the same one), Huffman / treeless four formats
    for (int i = 0; i < 2; ++i) {
        printf(" litfmt.%s.1=%llu litfmt.%s.2=%llu litfmt.%s.3=%llu", lt[i], (unsigned long long)(c.lit_format[i][0] + c.lit_format[i][2]), lt[i],
               (unsigned long long)c.lit_format[i][1], lt[i], (unsigned long long)c.lit_format[i][3]);
    }
    for (int f = 0; f < 4; ++f) printf(" litfmt.huffman.%d=%llu", f, (unsigned long long)(c.lit_format[2][f] + c.lit_format[3][f]));
    printf(" streams.1=%llu streams.4=%llu huf.direct=%llu huf.fse=%llu", (unsigned long long)c.streams[0], (unsigned long long)c.streams[1],
           (unsigned long long)c.huf_direct, (unsigned long long)c.huf_fse);
    for (int t = 0; t < 3; ++t)
        for (int m = 0; m < 4; ++m) printf(" mode.%s.%s=%llu", tab[t], md[m], (unsigned long long)c.mode[t][m]);
    for (int t = 0; t < 3; ++t)
        for (int m = 0; m < 3; ++m) printf(" repeat.%s.of-%s=%llu", tab[t], md[m], (unsigned long long)c.repeat_of[t][m]);
    for (int f = 0; f < 4; ++f) printf(" seqcount.%d=%llu", f, (unsigned long long)c.seq_form[f]);
    for (int f = 0; f < 5; ++f) printf(" fcs.%d=%llu", f == 4 ? 8 : f == 3 ? 4 : f, (unsigned long long)c.fcs_bytes[f]);
    printf(" single-segment=%llu skippable=%llu empty-frames=%llu checksums=%llu", (unsigned long long)c.single_segment, (unsigned long long)c.skippable,
           (unsigned long long)c.empty_frames, (unsigned long long)c.checksums);
    // repeat offsets: value 1 / 2 / 3 with and without a zero literals length, anywhere and as a block's first sequence after another
    // block of its frame (where the carried history decides); the longest length codes; the most sequences in a block
    unsigned long long repcase[3][2] = {}, first[3][2] = {}, max_seq = 0, far = 0;
    for (size_t k = 0; k < P.blocks.size(); ++k) {
        const ZsBlock &B = P.blocks[k];
        if (B.n_seq > max_seq) max_seq = B.n_seq;
        for (uint32_t i = 0; i < B.n_seq; ++i) {
            const uint32_t v = of[B.seq_off + i], z = ll[B.seq_off + i] == 0;
            if (v >= 1 && v <= 3) {
                repcase[v - 1][z]++;
                if (i == 0 && k > P.frames[B.frame].first_block) first[v - 1][z]++;
            } else if (v - 3 == start[k].window) {
                far++;
            }
        }
    }
    for (int v = 0; v < 3; ++v)
        for (int z = 0; z < 2; ++z)
            printf(" rep.%d.%s=%llu rep-at-block-start.%d.%s=%llu", v + 1, z ? "ll0" : "ll", repcase[v][z], v + 1, z ? "ll0" : "ll", first[v][z]);
    printf(" max-seq=%llu offset-at-window=%llu", max_seq, far);
    (void)rep;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    std::vector<uint8_t> file = read_file(argv[1]);
    const uint64_t n = file.size();
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    ZsPlan P;
    const char *why = "-";
    int status = 0;
    uint32_t rounds = 0;
    uint64_t total = 0, max_ml = 0, max_ll = 0;
    std::vector<uint8_t> text;
    std::vector<ZsReport> rep;
    std::vector<ZsStart> start;
    std::vector<uint32_t> ll, ml, of;
    bool ok = zs_plan(file.data(), n, P);
    if (!ok) why = "walk", status = P.status;
    if (ok) {
        const size_t B = P.blocks.size();
        std::vector<uint8_t> lit(P.lit_bytes + 1);
        ll.resize(P.n_seq + 1), ml.resize(P.n_seq + 1), of.resize(P.n_seq + 1);
        rep.resize(B);
        ZsTables *T = new ZsTables;
        for (size_t k = 0; k < B && ok; ++k) {
            ZsIn<ZsHostWords> in;
            in.w = ZsHostWords{file.data(), n};
            ZsSerialOut o{file.data(), lit.data(), ll.data(), ml.data(), of.data(), nullptr, nullptr};
            if (zs_decode_block(in, n, P.blocks[k], *T, o, rep[k]) != 0) ok = false, why = "block", status = rep[k].status;
        }
        delete T;
        for (uint64_t i = 0; i < P.n_seq; ++i) max_ml = ml[i] > max_ml ? ml[i] : max_ml, max_ll = ll[i] > max_ll ? ll[i] : max_ll;
        if (ok && !zs_scan(P, rep, start, &total)) ok = false, why = "scan", status = P.status;
        std::vector<uint32_t> src[2];
        if (ok) {
            text.resize(total + 1), src[0].resize(total + 1), src[1].resize(total + 1);
            uint64_t open = 0;
            for (size_t k = 0; k < B && ok; ++k) {
                ZsSerialOut o{file.data(), lit.data(), ll.data(), ml.data(), of.data(), text.data(), src[0].data()};
                uint32_t left = 0;
                const int st = zs_execute(P.blocks[k], start[k], rep[k].regen, ll.data(), ml.data(), of.data(), o, &left);
                if (st) ok = false, why = "execute", status = st;
                open += left;
            }
            const uint32_t cap = zs_round_cap(B);
            int cur = 0;
            while (ok && open) {
                if (rounds == cap) {
                    ok = false, why = "rounds", status = kZsRounds;
                    break;
                }
                open = 0;
                for (uint64_t i = 0; i < total; ++i) open += zs_resolve_byte(i, src[cur].data(), src[cur ^ 1].data(), text.data());
                cur ^= 1, ++rounds;
            }
        }
        for (const ZsFrame &F : P.frames) {
            if (!ok || !F.has_checksum) continue;
            Xxh64 h;
            h.update(text.data() + F.text_off, F.text_len);
            if ((uint32_t)h.digest() != F.checksum) ok = false, why = "checksum", status = kZsChecksum;
        }
    }
    if (ok && total) fwrite(text.data(), 1, total, out);
    fclose(out);
    printf("taken=%d bytes=%llu blocks=%zu frames=%zu rounds=%u why=%s status=%d max-ml=%llu max-ll=%llu", ok ? 1 : 0, (unsigned long long)(ok ? total : 0),
           ok ? P.blocks.size() : (size_t)0, ok ? P.frames.size() : (size_t)0, rounds, why, status, (unsigned long long)max_ml, (unsigned long long)max_ll);
    if (ok) census(P, rep, start, ll, of);
    printf("\n");
    return 0;
}
