// zstd_windows_harness.cpp -- merkurio_amd/csrc/codec/zstd_chain.hpp on the host: a .zst file decoded window by window as
// mk_zstd_stream_* decodes it, with the serial decoder of zstd_serial.hpp where the library has its kernels.
//     zstd_windows_harness stream <in.zst> <out.bin> <window_bytes> <text_cap>
//         the stream to its end; the text of the windows that stood, one after the other, to out.bin.  Prints state= and the
//         stats of mk_zstd_stream_stats, windows-blocks= (the blocks of every window, comma-separated), the census of what the seams
//         cut (ZsSeams and what only decoding shows: matches into the history, repeat-offset codes in a window's first sequence)
//         and the walk's census summed over the windows
//     zstd_windows_harness sweep <in.zst> <out.bin>
//         the file once in one window (to out.bin), then once per block k with the first seam behind block k and the rest in one
//         window: every text must be the first one (same=0|1).  The census is summed over all of these streams
//     zstd_windows_harness plan <in.zst>
//         zs_plan's ZsBlock table as blocks= and an FNV-1a hash of its bytes, and resumed=0|1: the same table out of the walk
//         stopped and resumed behind every block
// Built with the sanitizers by tests/test_unzstd_windows_cpu.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "codec/zstd_chain.hpp"

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

struct Extra {
    uint64_t match_below = 0, match_at = 0;  // windows with a match into a history below / equal to the frame's window
    uint64_t rep_first[3] = {0, 0, 0};       // windows inside a frame whose first sequence has offset value 1 / 2 / 3
    uint64_t settled_bytes = 0;
};

// the device's stand-in (zstd_chain.hpp: Dev)
struct SerialDev {
    std::vector<uint8_t> *sink;
    Extra *x;
    std::vector<uint8_t> in, lit, text[2];
    std::vector<uint32_t> ll, ml, of;
    int cur = 0;
    uint64_t text_total = 0;
    std::vector<ZsReport> reps;
    uint64_t text_room() { return kZsTextCapMax; }
    bool decode(const ZsWindow &W, std::vector<ZsReport> &rep) {
        const uint64_t n_in = W.n_in();
        in.assign(W.prelude, W.prelude + kZsPrelude);
        in.insert(in.end(), file + W.from, file + W.to);
        lit.assign(W.P.lit_bytes + 1, 0), ll.assign(W.P.n_seq + 1, 0), ml.assign(W.P.n_seq + 1, 0), of.assign(W.P.n_seq + 1, 0);
        rep.resize(W.P.blocks.size());
        ZsTables *T = new ZsTables;
        for (size_t k = 0; k < W.P.blocks.size(); ++k) {
            ZsIn<ZsHostWords> r;
            r.w = ZsHostWords{in.data(), n_in};
            ZsSerialOut o{in.data(), lit.data(), ll.data(), ml.data(), of.data(), nullptr, nullptr};
            zs_decode_block(r, n_in, W.P.blocks[k], *T, o, rep[k]);
        }
        delete T;
        reps = rep;
        return true;
    }
    bool execute(const ZsWindow &W, const std::vector<ZsStart> &start, uint64_t H, uint64_t total, uint32_t *rounds) {
        const int buf = cur ^ 1;
        if (H > text_total) return false;
        text[buf].assign(total + 1, 0);
        if (H) memcpy(text[buf].data(), text[cur].data() + (text_total - H), H);
        std::vector<uint32_t> src[2];
        src[0].assign(total + 1, kZsResolved), src[1].assign(total + 1, kZsResolved);
        const size_t B = W.P.blocks.size();
        uint64_t open = 0, hits = 0;
        for (size_t k = 0; k < B; ++k) {
            ZsSerialOut o{in.data(), lit.data(), ll.data(), ml.data(), of.data(), text[buf].data(), src[0].data()};
            o.settled = H;
            uint32_t left = 0;
            if (zs_execute(W.P.blocks[k], start[k], reps[k].regen, ll.data(), ml.data(), of.data(), o, &left) != 0) return false;
            open += left, hits += o.settled_hits;
        }
        if (B && !W.P.frames.empty() && W.P.frames[0].continued) {
            const ZsFrame &F = W.P.frames[0];
            if (hits) (H < F.window ? x->match_below : x->match_at)++;
            if (F.n_blocks && W.P.blocks[0].type == 2 && W.P.blocks[0].n_seq) {
                const uint32_t v = of[W.P.blocks[0].seq_off];
                if (v >= 1 && v <= 3) x->rep_first[v - 1]++;
            }
        }
        x->settled_bytes += hits;
        const uint32_t cap = zs_round_cap(B);
        int c = 0;
        *rounds = 0;
        while (open) {
            if (*rounds == cap) return false;
            open = 0;
            for (uint64_t i = H; i < total; ++i) open += zs_resolve_byte(i, src[c].data(), src[c ^ 1].data(), text[buf].data());
            c ^= 1, ++*rounds;
        }
        return true;
    }
    bool hash(uint64_t off, uint64_t len, Xxh64 &h) {
        h.update(text[cur ^ 1].data() + off, len);
        return true;
    }
    void commit(uint64_t H, uint64_t total) {
        cur ^= 1, text_total = total;
        if (text[cur].size() < total + 1) text[cur].assign(total + 1, 0);
        sink->insert(sink->end(), text[cur].data() + H, text[cur].data() + total);
    }
    const uint8_t *file = nullptr;
};

struct Run {
    uint32_t state = 2;
    mk_zstd_stream_stats stats{};
    std::string window_blocks;
};

// one stream over the file; caps[w] = the text cap of window w (the last one stands for the rest); census summed into *all
static Run run_stream(const std::vector<uint8_t> &file, uint64_t window, const std::vector<uint64_t> &caps, std::vector<uint8_t> &text, ZsSeams &seams, ZsCensus &census,
                      Extra &x) {
    Run R;
    ZsStream *S = new ZsStream;
    if (!zs_stream_open(*S, file.data(), file.size(), window)) {
        delete S;
        return R;
    }
    SerialDev dev;
    dev.sink = &text, dev.x = &x, dev.file = file.data();
    for (size_t w = 0;; ++w) {
        S->text_cap = caps[w < caps.size() ? w : caps.size() - 1];
        uint64_t n = 0, before = S->stats.blocks;
        zs_stream_next(*S, dev, &n, &R.state);
        if (R.state != 0) break;
        R.window_blocks += (R.window_blocks.empty() ? "" : ",") + std::to_string(S->stats.blocks - before);
    }
    R.stats = S->stats;
    for (size_t k = 0; k < sizeof(ZsSeams) / 8; ++k) ((uint64_t *)&seams)[k] += ((const uint64_t *)&S->seams)[k];
    for (size_t k = 0; k < sizeof(ZsCensus) / 8; ++k) ((uint64_t *)&census)[k] += ((const uint64_t *)&S->census)[k];
    delete S;
    return R;
}

static void print_census(const ZsSeams &s, const Extra &x, const ZsCensus &c) {
    const char *tab[3] = {"ll", "of", "ml"}, *md[3] = {"predefined", "rle", "fse"};
    printf(" seam.treeless=%llu", (unsigned long long)s.treeless_carried);
    for (int t = 0; t < 3; ++t)
        for (int m = 0; m < 3; ++m) printf(" seam.repeat.%s.of-%s=%llu", tab[t], md[m], (unsigned long long)s.repeat_carried[t][m]);
    printf(" seam.frame-end=%llu seam.skippable=%llu seam.two-frames=%llu seam.checksum-3-windows=%llu seam.history-below-window=%llu seam.history-at-window=%llu",
           (unsigned long long)s.frame_end_at_seam, (unsigned long long)s.skippable_at_seam, (unsigned long long)s.two_frames, (unsigned long long)s.checksum_3_windows,
           (unsigned long long)s.history_below_window, (unsigned long long)s.history_at_window);
    printf(" seam.match-below-window=%llu seam.match-at-window=%llu seam.rep-first.1=%llu seam.rep-first.2=%llu seam.rep-first.3=%llu settled-bytes=%llu",
           (unsigned long long)x.match_below, (unsigned long long)x.match_at, (unsigned long long)x.rep_first[0], (unsigned long long)x.rep_first[1],
           (unsigned long long)x.rep_first[2], (unsigned long long)x.settled_bytes);
    printf(" walk.blocks=%llu walk.frames=%llu walk.skippable=%llu walk.checksums=%llu", (unsigned long long)(c.block_type[0] + c.block_type[1] + c.block_type[2]),
           (unsigned long long)c.frames, (unsigned long long)c.skippable, (unsigned long long)c.checksums);
}

static void write_file(const char *path, const std::vector<uint8_t> &v) {
    FILE *f = fopen(path, "wb");
    if (!f) exit(2);
    if (!v.empty()) fwrite(v.data(), 1, v.size(), f);
    fclose(f);
}

static uint64_t fnv(const void *p, size_t n, uint64_t h = 0xcbf29ce484222325ull) {
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const uint8_t *)p)[i]) * 0x100000001b3ull;
    return h;
}

static int plan_mode(const std::vector<uint8_t> &file) {
    ZsPlan P;
    const bool ok = zs_plan(file.data(), file.size(), P);
    printf("walked=%d status=%d blocks=%zu frames=%zu lit=%llu seq=%llu hash=%016llx", ok ? 1 : 0, P.status, P.blocks.size(), P.frames.size(),
           (unsigned long long)P.lit_bytes, (unsigned long long)P.n_seq, (unsigned long long)fnv(P.blocks.data(), P.blocks.size() * sizeof(ZsBlock)));
    // the walk stopped and resumed behind every block: its tables count from the resumption, everything else is the file's
    bool same = ok;
    if (ok && file.size() >= 4) {
        ZsWalk W;
        std::vector<ZsBlock> all;
        uint64_t lit = 0, seq = 0, frames = 0;
        int guard = 0;
        while ((W.open || W.at < file.size()) && same && ++guard < (1 << 24)) {
            ZsPlan Q;
            if (!zs_walk(file.data(), file.size(), W, ZsLimit{0, 1}, Q)) same = false;
            for (ZsBlock B : Q.blocks) {
                for (uint32_t &d : B.def_block)
                    if (d != ~0u) d += (uint32_t)all.size();  // (one block per walk: a table of its own names block 0)
                if (B.type == 2) B.lit_off += lit, B.seq_off += seq;
                B.frame += (uint32_t)frames;
                all.push_back(B);
            }
            lit += Q.lit_bytes, seq += Q.n_seq;
            for (const ZsFrame &F : Q.frames) frames += F.closed;
        }
        // (def_block of a table defined by an earlier walk is that walk's block 0: not comparable, so it is left out of the comparison)
        same = same && all.size() == P.blocks.size();
        for (size_t k = 0; same && k < all.size(); ++k) {
            ZsBlock a = all[k], b = P.blocks[k];
            for (int i = 0; i < 4; ++i) a.def_block[i] = b.def_block[i] = 0;
            same = memcmp(&a, &b, sizeof a) == 0;
        }
    }
    printf(" resumed=%d\n", same ? 1 : 0);
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    const std::string mode = argv[1];
    const std::vector<uint8_t> file = read_file(argv[2]);
    if (mode == "plan") return plan_mode(file);
    if (argc < 4) return 2;
    ZsSeams seams;
    ZsCensus census;
    Extra x;
    std::vector<uint8_t> text;
    if (mode == "stream" && argc == 6) {
        const uint64_t window = strtoull(argv[4], nullptr, 10), cap = strtoull(argv[5], nullptr, 10);
        const Run R = run_stream(file, window, {cap ? cap : kZsTextCapMax}, text, seams, census, x);
        write_file(argv[3], text);
        printf("state=%u bytes=%zu windows=%llu frames=%llu blocks=%llu consumed=%llu text=%llu rounds=%llu max-history=%llu windows-blocks=%s", R.state, text.size(),
               (unsigned long long)R.stats.windows, (unsigned long long)R.stats.frames, (unsigned long long)R.stats.blocks, (unsigned long long)R.stats.consumed_bytes,
               (unsigned long long)R.stats.text_bytes, (unsigned long long)R.stats.rounds, (unsigned long long)R.stats.max_history,
               R.window_blocks.empty() ? "-" : R.window_blocks.c_str());
        print_census(seams, x, census);
        printf("\n");
        return 0;
    }
    if (mode == "sweep" && argc == 4) {
        const Run R = run_stream(file, 1ull << 40, {kZsTextCapMax}, text, seams, census, x);
        write_file(argv[3], text);
        bool same = true;
        uint64_t runs = 0;
        for (uint64_t k = 1; R.state == 1 && k < R.stats.blocks; ++k, ++runs) {
            std::vector<uint8_t> t2;
            const Run R2 = run_stream(file, 1ull << 40, {k * kZsBlockMax, kZsTextCapMax}, t2, seams, census, x);
            if (R2.state != 1 || t2 != text || R2.stats.blocks != R.stats.blocks || R2.stats.frames != R.stats.frames) same = false;
        }
        printf("state=%u bytes=%zu blocks=%llu frames=%llu seams=%llu same=%d", R.state, text.size(), (unsigned long long)R.stats.blocks, (unsigned long long)R.stats.frames,
               (unsigned long long)runs, same ? 1 : 0);
        print_census(seams, x, census);
        printf("\n");
        return 0;
    }
    return 2;
}
