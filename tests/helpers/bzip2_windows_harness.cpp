// bzip2_windows_harness.cpp -- merkurio_amd/csrc/codec/bzip2_chain.hpp, the window logic of mk_bzip2_stream_*, compiled for the host and
// run the way bzip2_host.cpp runs it: mkz::bz2_stream_next over a stand-in for the device made of bz2_find_markers and the serial block
// decoder of bzip2_serial.hpp.  tests/test_bunzip2_windows_cpu.py builds it (MERKURIO_TEST_SANITIZE=1: with ASan + UBSan) and checks it
// against Python's bz2.
//
//   bzip2_windows_harness run IN.bz2 OUT WINDOW [TEXT_CAP [MAX_BLOCKS]]
// streams IN at WINDOW compressed bytes per window, appends every text window to OUT and prints one line:
//   "state=S windows=W streams=N blocks=B consumed=C text=T grown=G uploads=U sizes=a,b,..."   (S: the last state; sizes: per text window)
// TEXT_CAP: bytes a text window may hold (0 = no bound); MAX_BLOCKS: blocks the stand-in decodes per window (0 = all: "no room for more").
//   bzip2_windows_harness sweep IN.bz2 TEXT FROM TO STEP
// streams IN at every window size FROM, FROM + STEP, ... <= TO and prints "sweep runs=R bad=K first_bad=WINDOW": a run is bad unless
// its text is TEXT's bytes and its last state is 1.
// Exit status 0 (a sanitizer report is what makes it non-zero).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "codec/bzip2_chain.hpp"

using namespace mkz;

namespace {

std::vector<uint8_t> read_file(const char *path) {
    std::vector<uint8_t> v;
    FILE *f = fopen(path, "rb");
    if (!f) exit(2);
    uint8_t tmp[65536];
    for (size_t k; (k = fread(tmp, 1, sizeof tmp, f)) > 0;) v.insert(v.end(), tmp, tmp + k);
    fclose(f);
    return v;
}

struct HostDev {
    uint64_t text_cap = 0, max_blocks = 0, uploads = 0;
    std::vector<uint8_t> exact, padded;  // the upload as it is (the search: ASan sees a read behind it), and with the reader's pad
    struct Pre {
        std::vector<uint8_t> pre;
        std::vector<uint32_t> is_count;
    };
    std::vector<Pre> kept;  // per decoded block: the bytes in front of the run-length step
    std::vector<uint8_t> ll8;  // a block's last column and its vector: room for the largest level met so far
    std::vector<uint32_t> tt;
    std::vector<uint8_t> text[2];
    int cur = 0;
    uint64_t n_up = 0;
    Bz2Tables *T = new Bz2Tables;
    uint32_t crc_table[256];
    HostDev() {
        for (uint32_t i = 0; i < 256; ++i) crc_table[i] = bz2_crc_table_entry(i);
    }
    ~HostDev() { delete T; }

    bool upload(const uint8_t *up, uint64_t n, std::vector<BzMarker> &markers) {
        ++uploads, n_up = n;
        exact.assign(up, up + n);
        padded = exact;
        padded.resize((n + kBzStreamPad + 3) & ~3ull, 0);
        markers.clear();
        bz2_find_markers(exact.data(), n, markers);
        return markers.size() <= bz2_marker_cap(n);
    }
    uint32_t decode(const std::vector<BzWinBlock> &blocks, std::vector<Bz2Block> &rep, std::vector<unsigned long long> &text_len) {
        const size_t B = max_blocks ? std::min<size_t>(max_blocks, blocks.size()) : blocks.size();
        rep.clear(), text_len.clear(), kept.clear();
        std::vector<uint8_t> sel(kBzSelBytes);
        for (size_t k = 0; k < B; ++k) {
            const uint32_t cap = blocks[k].level * 100000u;
            if (ll8.size() < cap) ll8.resize(cap), tt.resize(cap);
            Pre p;
            BzBits<BzHostWords> bits;
            bits.w = BzHostWords{padded.data(), padded.size() / 4};
            bits.n_bits = n_up * 8;
            bits.seek(blocks[k].bit);
            BzSerialMtf mtf;
            BzSerialOut o{ll8.data()};
            Bz2Block h;
            unsigned long long len = 0;
            if (bz2_decode_block(bits, blocks[k].level, *T, sel.data(), mtf, o, h) == 0) {
                p.pre.resize(h.nblock), p.is_count.resize(h.nblock / 32 + 1);
                bz2_prefix(T->hist);
                bz2_scatter_serial(ll8.data(), h.nblock, T->hist, tt.data());
                uint64_t l = 0;
                if (int st = bz2_walk(tt.data(), h.nblock, h.orig_ptr, p.pre.data(), p.is_count.data(), &l)) h.status = st;
                len = l;
            }
            rep.push_back(h), text_len.push_back(len), kept.push_back(std::move(p));
            if (h.status != 0 || h.end_bit != blocks[k].end_bit) break;  // (the blocks behind it need not be run)
        }
        return (uint32_t)rep.size();
    }
    uint64_t text_room() const { return text_cap ? text_cap : ~0ull; }
    bool expand(uint32_t b0, uint32_t b1, const unsigned long long *text_off, uint64_t total, uint32_t *crc, const std::vector<Bz2Block> &rep) {
        cur ^= 1;
        std::vector<uint8_t> &t = text[cur];
        t.assign(total, 0xee);
        for (uint32_t k = b0; k < b1; ++k) {
            uint8_t *at = t.data() + text_off[k - b0];
            bz2_expand_serial(kept[k].pre.data(), kept[k].is_count.data(), rep[k].nblock, at);
            const uint64_t len = (k + 1 < b1 ? text_off[k + 1 - b0] : total) - text_off[k - b0];
            uint32_t c = 0xffffffffu;
            for (uint64_t i = 0; i < len; ++i) c = bz2_crc_byte(c, at[i], crc_table);
            crc[k - b0] = ~c;
        }
        return true;
    }
};
// (the serial expansion needs a block's symbol count, which is the stream's: the adapter hands it over)
struct Adapter {
    HostDev &d;
    BzStream &S;
    bool upload(const uint8_t *up, uint64_t n, std::vector<BzMarker> &m) { return d.upload(up, n, m); }
    uint32_t decode(const std::vector<BzWinBlock> &b, std::vector<Bz2Block> &rep, std::vector<unsigned long long> &len) { return d.decode(b, rep, len); }
    uint64_t text_room() { return d.text_room(); }
    bool expand(uint32_t b0, uint32_t b1, const unsigned long long *off, uint64_t total, uint32_t *crc) { return d.expand(b0, b1, off, total, crc, S.rep); }
};

struct Run {
    uint32_t state = 2;
    std::vector<uint8_t> text;
    std::vector<uint64_t> sizes;
    mk_bzip2_stream_stats stats{};
    uint64_t uploads = 0;
};

Run stream_file(const std::vector<uint8_t> &file, uint64_t window, uint64_t text_cap, uint64_t max_blocks) {
    Run r;
    BzStream S;
    if (!bz2_stream_open(S, file.data(), file.size(), window)) return r;
    HostDev dev;
    dev.text_cap = text_cap, dev.max_blocks = max_blocks;
    Adapter a{dev, S};
    for (;;) {
        uint64_t n = 0;
        bz2_stream_next(S, a, &n, &r.state);
        if (r.state != 0) break;
        if (n > dev.text[dev.cur].size()) exit(3);
        r.text.insert(r.text.end(), dev.text[dev.cur].begin(), dev.text[dev.cur].begin() + n);
        r.sizes.push_back(n);
    }
    r.stats = S.stats, r.uploads = dev.uploads;
    return r;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const std::string mode = argv[1];
    const std::vector<uint8_t> file = read_file(argv[2]);
    if (mode == "run") {
        const Run r = stream_file(file, strtoull(argv[4], nullptr, 10), argc > 5 ? strtoull(argv[5], nullptr, 10) : 0, argc > 6 ? strtoull(argv[6], nullptr, 10) : 0);
        FILE *out = fopen(argv[3], "wb");
        if (!out) return 2;
        if (!r.text.empty()) fwrite(r.text.data(), 1, r.text.size(), out);
        fclose(out);
        printf("state=%u windows=%llu streams=%llu blocks=%llu consumed=%llu text=%llu grown=%llu uploads=%llu sizes=", r.state, (unsigned long long)r.stats.windows,
               (unsigned long long)r.stats.streams, (unsigned long long)r.stats.blocks, (unsigned long long)r.stats.consumed_bytes, (unsigned long long)r.stats.text_bytes,
               (unsigned long long)r.stats.windows_grown, (unsigned long long)r.uploads);
        for (size_t k = 0; k < r.sizes.size(); ++k) printf("%s%llu", k ? "," : "", (unsigned long long)r.sizes[k]);
        printf("\n");
        return 0;
    }
    if (mode == "sweep" && argc == 7) {
        const std::vector<uint8_t> want = read_file(argv[3]);
        const uint64_t from = strtoull(argv[4], nullptr, 10), to = strtoull(argv[5], nullptr, 10), step = strtoull(argv[6], nullptr, 10);
        uint64_t runs = 0, bad = 0, first_bad = 0;
        for (uint64_t w = from; w <= to && step; w += step, ++runs) {
            const Run r = stream_file(file, w, 0, 0);
            if (r.state != 1 || r.text != want || r.stats.text_bytes != want.size() || r.stats.consumed_bytes != file.size()) {
                if (!bad++) first_bad = w;
            }
        }
        printf("sweep runs=%llu bad=%llu first_bad=%llu\n", (unsigned long long)runs, (unsigned long long)bad, (unsigned long long)first_bad);
        return 0;
    }
    return 2;
}
