// zstd_enc_harness.cpp -- merkurio_amd/csrc/codec/zstd_enc_serial.hpp on the host: the serial pieces of the zstd frame writer of
// zstd_deflate.hip (weights and codes of the literals, FSE normalisation, table description and encoding table, codes of the lengths and
// offsets, the section headers, the forward bit writer) behind a naive greedy parser, one thread.
//     zstd_enc_harness <text> <out.zst>
// cuts the text at the grid of the frame rule (no record table: bgzf_cuts.hpp with the zstd constants), writes one frame per cut, decodes
// every frame again with zstd_serial.hpp / zstd_plan.hpp / xxh64.hpp and prints one line per frame:
//     frame=K n= bytes= block=raw|rle|compressed lit=none|raw|rle|huffman streams= nlit= nseq= ll= of= ml= (predefined|rle|fse|-) self=0|1
// The caller (tests/test_zstd_deflate_cpu.py) decodes the frames with libzstd.  Built with -fsanitize=address,undefined.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "codec/bgzf_cuts.hpp"
#include "codec/xxh64.hpp"
#include "codec/zstd_enc_serial.hpp"
#include "codec/zstd_plan.hpp"

using namespace mkz;

struct Seq {
    uint32_t ll, ml, of;
};
struct Info {
    const char *block = "raw", *lit = "none", *mode[3] = {"-", "-", "-"};
    uint32_t streams = 0, n_lit = 0, n_seq = 0;
};

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

// greedy: the most recent position with the same three bytes, or the byte in front (a run); a match runs to the block's end
static void parse(const uint8_t *t, uint32_t n, std::vector<uint8_t> &lits, std::vector<Seq> &seqs) {
    std::vector<int32_t> head(1 << 16, -1);
    auto hash = [&](uint32_t i) { return ((t[i] | (uint32_t)t[i + 1] << 8 | (uint32_t)t[i + 2] << 16) * 0x9E3779B1u) >> 16; };
    auto common = [&](uint32_t a, uint32_t b) {
        uint32_t l = 0;
        while (a + l < n && t[a + l] == t[b + l]) ++l;
        return l;
    };
    uint32_t i = 0, run = 0;
    while (i < n) {
        uint32_t len = 0, dist = 0;
        if (i + 3 <= n) {
            const uint32_t h = hash(i);
            if (head[h] >= 0) {
                const uint32_t l = common(i, (uint32_t)head[h]);
                if (l >= 3) len = l, dist = i - (uint32_t)head[h];
            }
            if (i > 0) {
                const uint32_t l = common(i, i - 1);
                if (l >= 3 && l >= len) len = l, dist = 1;
            }
            head[h] = (int32_t)i;
        }
        if (len) {
            seqs.push_back(Seq{run, len, dist});
            for (uint32_t k = 1; k < len && i + k + 3 <= n; ++k) head[hash(i + k)] = (int32_t)(i + k);
            i += len, run = 0;
        } else {
            lits.push_back(t[i]), ++i, ++run;
        }
    }
}

static void literals_section(const std::vector<uint8_t> &lits, std::vector<uint8_t> &out, Info &I) {
    const uint32_t n = (uint32_t)lits.size();
    uint8_t hdr[8];
    uint32_t freq[256] = {}, distinct = 0, top = 0;
    for (uint8_t b : lits) freq[b]++;
    for (uint32_t s = 0; s < 256; ++s)
        if (freq[s]) ++distinct, top = s;
    auto raw = [&] {
        out.insert(out.end(), hdr, hdr + ze_lit_header_plain(0, n, hdr));
        out.insert(out.end(), lits.begin(), lits.end());
        I.lit = n ? "raw" : "none";
    };
    if (n == 0) return raw();
    // (one distinct literal: the text is one repeated byte, an RLE block -- encode_frame never comes here with it)
    if (distinct < 2) return raw();
    if (top > kZeHufMaxSym) return raw();
    uint32_t key[256], m = 0;
    for (uint32_t s = 0; s <= top; ++s)
        if (freq[s]) key[m++] = freq[s] << 9 | s;
    std::sort(key, key + m);
    uint8_t lens[256] = {}, weights[256] = {};
    uint16_t code[256];
    uint32_t rank[16];
    HuffScratch *hs = new HuffScratch;
    code_lengths_from_sorted(key, (int)m, (int)kZsHufLog, lens, *hs);
    delete hs;
    const uint32_t mb = ze_huf_weights(lens, top + 1, weights);
    ze_huf_codes(weights, top + 1, mb, code, rank);
    uint8_t tree[80];
    const uint32_t tree_bytes = ze_huf_header(weights, top, tree);
    const uint32_t streams = ze_lit_streams(n), q = streams == 4 ? (n + 3) / 4 : n;
    std::vector<uint8_t> body[4];
    for (uint32_t k = 0; k < streams; ++k) {
        const uint32_t a = k * q, b = k + 1 < streams ? a + q : n;
        body[k].assign((size_t)(b - a) * 11 / 8 + 8, 0);
        ZeBits w{body[k].data()};
        for (uint32_t j = b; j-- > a;) w.put(code[lits[j]], lens[lits[j]]);  // the first literal is written last
        body[k].resize(w.close());
    }
    uint32_t comp = tree_bytes + (streams == 4 ? 6 : 0);
    for (uint32_t k = 0; k < streams; ++k) comp += (uint32_t)body[k].size();
    if (ze_lit_header_huf_bytes(n, comp) + comp >= ze_lit_header_plain_bytes(n) + n) return raw();
    out.insert(out.end(), hdr, hdr + ze_lit_header_huf(n, comp, hdr));
    out.insert(out.end(), tree, tree + tree_bytes);
    if (streams == 4)
        for (uint32_t k = 0; k < 3; ++k) out.push_back((uint8_t)body[k].size()), out.push_back((uint8_t)(body[k].size() >> 8));
    for (uint32_t k = 0; k < streams; ++k) out.insert(out.end(), body[k].begin(), body[k].end());
    I.lit = "huffman", I.streams = streams;
}

static void sequences_section(const std::vector<Seq> &seqs, std::vector<uint8_t> &out, Info &I) {
    const uint32_t n = (uint32_t)seqs.size();
    uint8_t hdr[4];
    out.insert(out.end(), hdr, hdr + ze_seq_count(n, hdr));
    if (!n) return;
    static const char *names[3] = {"predefined", "rle", "fse"};
    std::vector<uint8_t> code[3];
    uint32_t count[3][64] = {};
    for (const Seq &s : seqs) {
        const uint32_t c[3] = {ze_ll_code(s.ll), ze_of_code(s.of), ze_ml_code(s.ml)};
        for (int t = 0; t < 3; ++t) code[t].push_back((uint8_t)c[t]), count[t][c[t]]++;
    }
    int16_t norm[3][64];
    uint32_t log[3], mode[3];
    std::vector<uint16_t> state[3];
    ZeSym tt[3][64];
    uint8_t desc[3][kZeDescMax];
    uint32_t desc_bytes[3];
    for (uint32_t t = 0; t < 3; ++t) {
        memset(desc[t], 0, sizeof desc[t]);
        mode[t] = ze_choose_table(t, count[t], n, norm[t], &log[t], desc[t], &desc_bytes[t]);
        I.mode[t] = names[mode[t]];
        uint8_t slot_sym[512];
        uint16_t cumul[65];
        state[t].assign(1u << log[t], 0);
        ze_fse_spread(norm[t], 64, log[t], slot_sym);
        ze_fse_fill(norm[t], 64, log[t], slot_sym, state[t].data(), tt[t], cumul);
    }
    out.push_back((uint8_t)(mode[0] << 6 | mode[1] << 4 | mode[2] << 2));
    for (uint32_t t = 0; t < 3; ++t) out.insert(out.end(), desc[t], desc[t] + desc_bytes[t]);
    std::vector<uint8_t> bits((size_t)n * 10 + 16, 0);
    ZeBits w{bits.data()};
    auto extra = [&](uint32_t i) {
        const Seq &s = seqs[i];
        w.put(s.ll - zs_ll_base(code[0][i]), zs_ll_bits(code[0][i]));
        w.put(s.ml - zs_ml_base(code[2][i]), zs_ml_bits(code[2][i]));
        w.put(s.of + 3 - (1u << code[1][i]), code[1][i]);
    };
    uint32_t st[3];
    for (uint32_t t = 0; t < 3; ++t) st[t] = ze_fse_first(state[t].data(), tt[t], code[t][n - 1]);
    extra(n - 1);
    for (uint32_t i = n - 1; i-- > 0;) {
        for (uint32_t t : {1u, 2u, 0u}) {  // offset, match length, literal length: the decoder updates them in the opposite order
            uint32_t nb = 0;
            const uint32_t next = ze_fse_step(state[t].data(), tt[t], st[t], code[t][i], &nb);
            w.put(st[t], nb);
            st[t] = next;
        }
        extra(i);
    }
    w.put(st[2], log[2]), w.put(st[1], log[1]), w.put(st[0], log[0]);
    bits.resize(w.close());
    out.insert(out.end(), bits.begin(), bits.end());
}

static std::vector<uint8_t> encode_frame(const uint8_t *t, uint32_t n, Info &I) {
    std::vector<uint8_t> f(12), block;
    bool same = n > 0;
    for (uint32_t i = 1; i < n && same; ++i) same = t[i] == t[0];
    uint32_t type = 0;
    if (same) {
        type = 1, block.push_back(t[0]), I.block = "rle";
    } else if (n) {
        std::vector<uint8_t> lits;
        std::vector<Seq> seqs;
        parse(t, n, lits, seqs);
        I.n_lit = (uint32_t)lits.size(), I.n_seq = (uint32_t)seqs.size();
        literals_section(lits, block, I);
        sequences_section(seqs, block, I);
        if (block.size() >= n) {
            block.assign(t, t + n);
            I = Info();
        } else {
            type = 2, I.block = "compressed";
        }
    }
    ze_frame_head(n, type, type == 1 ? n : (uint32_t)block.size(), f.data());
    f.insert(f.end(), block.begin(), block.end());
    Xxh64 h;
    h.update(t, n);
    const uint32_t sum = (uint32_t)h.digest();
    for (int k = 0; k < 4; ++k) f.push_back((uint8_t)(sum >> (8 * k)));
    return f;
}

// one frame decoded by the decoder the device runs (zstd_harness.cpp's phases); true where it gives `want`
static bool decodes_to(const std::vector<uint8_t> &file, const uint8_t *want, uint32_t n) {
    ZsPlan P;
    if (!zs_plan(file.data(), file.size(), P) || P.frames.size() != 1) return false;
    const size_t B = P.blocks.size();
    std::vector<uint8_t> lit(P.lit_bytes + 1);
    std::vector<uint32_t> ll(P.n_seq + 1), ml(P.n_seq + 1), of(P.n_seq + 1);
    std::vector<ZsReport> rep(B);
    std::vector<ZsStart> start;
    ZsTables *T = new ZsTables;
    bool ok = true;
    for (size_t k = 0; k < B && ok; ++k) {
        ZsIn<ZsHostWords> in;
        in.w = ZsHostWords{file.data(), file.size()};
        ZsSerialOut o{file.data(), lit.data(), ll.data(), ml.data(), of.data(), nullptr, nullptr};
        ok = zs_decode_block(in, file.size(), P.blocks[k], *T, o, rep[k]) == 0;
    }
    delete T;
    uint64_t total = 0;
    if (!ok || !zs_scan(P, rep, start, &total) || total != n) return false;
    std::vector<uint8_t> text(total + 1);
    std::vector<uint32_t> src(total + 1);
    for (size_t k = 0; k < B; ++k) {
        ZsSerialOut o{file.data(), lit.data(), ll.data(), ml.data(), of.data(), text.data(), src.data()};
        uint32_t left = 0;
        if (zs_execute(P.blocks[k], start[k], rep[k].regen, ll.data(), ml.data(), of.data(), o, &left) || left) return false;
    }
    if (n && memcmp(text.data(), want, n)) return false;
    Xxh64 h;
    h.update(text.data(), n);
    return P.frames[0].has_checksum && (uint32_t)h.digest() == P.frames[0].checksum;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const std::vector<uint8_t> text = read_file(argv[1]);
    FILE *out = fopen(argv[2], "wb");
    if (!out) return 2;
    const uint64_t end = text.size();
    std::vector<uint64_t> cut(end / kZsCutGrid + 3);
    const uint64_t n_cuts = zstd_record_cuts(&end, end ? 1 : 0, cut.data(), cut.size());
    for (uint64_t k = 0; k + 1 < n_cuts || (k == 0 && n_cuts == 1); ++k) {
        const uint64_t a = cut[k], b = n_cuts > 1 ? cut[k + 1] : a;
        Info I;
        const std::vector<uint8_t> f = encode_frame(text.data() + a, (uint32_t)(b - a), I);
        fwrite(f.data(), 1, f.size(), out);
        printf("frame=%llu n=%llu bytes=%zu block=%s lit=%s streams=%u nlit=%u nseq=%u ll=%s of=%s ml=%s self=%d\n", (unsigned long long)k,
               (unsigned long long)(b - a), f.size(), I.block, I.lit, I.streams, I.n_lit, I.n_seq, I.mode[0], I.mode[1], I.mode[2],
               decodes_to(f, text.data() + a, (uint32_t)(b - a)) ? 1 : 0);
    }
    fclose(out);
    return 0;
}
