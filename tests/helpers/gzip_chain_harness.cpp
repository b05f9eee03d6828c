// gzip_chain_harness.cpp -- merkurio_amd/csrc/codec/gzip_chain.hpp (the host's part of the gzip proof: candidates, piece table,
// verdict walk, window ends, ISIZE, CRC fold) compiled for the host and run with the serial decoder of gzip_segments.hpp in the
// device's place, the way gzip_host.cpp runs it between the kernels of gzip_inflate.hip; tests/test_gunzip_chain_cpu.py compares
// the outcome with zlib's.  What plays the device:
//   block starts  per nominal chunk the first bit inside the chunk that passes seg_header_plausible and seg_confirm_block_start (the
//                 whole-block confirm; the search kernel decodes 2 048 symbols dry instead, so it may confirm other starts);
//   pieces        inflate_segment, the status from seg_end_status, as mk_gzip_segments_kernel has it;
//   resolution    piece by piece on the host; a carry stands in front of a continued member, contexts restart at each member,
//                 seg_before_stream refuses;
//   CRC-32        per block, by a table.
// usage: gzip_chain_harness <file> <window bytes, 0 = one shot over all members> <chunk bytes> <out>
//        -> "taken=0|1 state=S members=M windows=W grown=G repeated=R pieces=P", the delivered text in <out>.  state: 1 = the file's
//        end was reached, 2 = handed back (one shot: 1 or 2 as taken says)
//        gzip_chain_harness --isize <text bytes> <bytes before the window> <isize> <whole 0|1>  -> "agrees=0|1"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "codec/gzip_chain.hpp"

using namespace mkz;
typedef unsigned long long ull;

static uint32_t crc_table[256];
static uint32_t crc32_of(const uint8_t *p, uint64_t n) {
    uint32_t c = 0xffffffffu;
    for (uint64_t i = 0; i < n; ++i) c = crc_table[(c ^ p[i]) & 0xff] ^ (c >> 8);
    return ~c;
}

struct Stream {  // what mk_gzip_stream holds
    GzStreamPos at;
    uint64_t window = 0;
    uint32_t grow = 0;
    std::vector<uint8_t> carry = std::vector<uint8_t>(kSegPrefix, 0);
    uint64_t windows = 0, grown = 0, members = 0, repeated = 0, pieces = 0;
};

struct Run {  // the named options of gzip_host.cpp's driver that reach the proof
    const uint8_t *up;
    uint64_t n_up, first_ratio;
    bool count_chunks, whole;
    Stream *S;
    uint64_t n_file;
};

// gzip_host.cpp's gzip_run with the device played here: -> 0 (text appended to out), 2, 3
static int run(const Run &o, std::vector<GzCandidate> mem, uint64_t set_chunk, std::vector<uint8_t> &out, uint64_t *n_members, Stream &counts) {
    Stream *S = o.S;
    const uint64_t n_in = o.n_up;
    const uint64_t chunk = gzip_chunk_bytes(n_in, set_chunk, 256);
    const uint32_t n_chunks = (uint32_t)std::max<uint64_t>(1, n_in / chunk);
    if (mem.size() + (o.count_chunks ? n_chunks : 0) > kGzMaxPieces) return 2;
    std::vector<uint8_t> in(o.up, o.up + n_in);  // the upload: zeros behind it
    in.resize(n_in + kStreamPad + 16, 0);
    std::vector<uint16_t> t(kLaneTableU16);
    // ---- block starts (mk_gzip_find_kernel's bounds)
    std::vector<ull> starts(n_chunks, ~0ull);
    for (uint32_t c = 1; c < n_chunks; ++c) {
        const uint64_t bit0 = c * chunk * 8, bit1 = c + 1 == n_chunks ? n_in * 8 : std::min<uint64_t>(bit0 + chunk * 8, n_in * 8);
        for (uint64_t bit = bit0; bit < bit1 && bit + 64 <= n_in * 8; ++bit) {
            uint32_t v = 0;
            for (int k = 0; k < 13; ++k) v |= (uint32_t)((in[(bit + k) >> 3] >> ((bit + k) & 7)) & 1u) << k;
            if (seg_header_bits_plausible(v) && seg_header_plausible(in.data(), n_in, bit) && seg_confirm_block_start(in.data(), n_in, bit, t.data())) {
                starts[c] = bit;
                break;
            }
        }
    }
    std::vector<ull> found = gzip_found_starts(starts);
    // ---- rounds
    GzRounds R;
    R.ratio = o.first_ratio;
    GzPieces P;
    std::vector<ull> n_out;
    std::vector<uint16_t> sym;
    const bool proved = gzip_prove(mem, found, n_in, R, P, n_out, [&](const GzPieces &p, ull *p_out, int32_t *p_status) {
        sym.assign(p.elems + 32, 0);
        for (uint32_t j = 0; j < p.J; ++j) {
            uint16_t *base = sym.data() + p.off()[j];
            for (uint32_t k = 0; k < kSegPrefix; ++k) base[k] = (uint16_t)(kSegUnknown | k);
            const uint64_t end = p.end()[j], lim = p.lim()[j];
            uint64_t produced = 0, stop = 0;
            bool fin = false;
            int rc = inflate_segment(in.data(), lim, p.bits()[j], end, 0, base + kSegPrefix, p.cap()[j], t.data(), &produced, &stop, &fin);
            if (rc == 0) rc = seg_end_status(end, lim, stop, fin);
            p_out[j] = rc == kSegDesync || rc == kSegEndsEarly ? stop : produced;
            p_status[j] = rc;
        }
        counts.pieces = p.J;
        return true;
    });
    counts.repeated += R.repeated;
    if (!proved) return 2;
    const uint32_t J = P.J;
    const size_t M = mem.size();
    uint64_t next_bit = 0;
    bool next_in_member = false;
    if (S) {
        const int e = gzip_window_end(mem, P.cut_bit, S->at.pos_bit, S->at.in_member, o.n_file, (S->at.pos_bit >> 3) + n_in == o.n_file, &next_bit, &next_in_member);
        if (e) return e;
    }
    const bool continues = S && S->at.in_member;
    GzText T;
    if (!gzip_text_offsets(mem, P, n_out, o.up, o.whole, continues ? S->at.open_len : 0, T)) return 2;
    // ---- resolution: the contexts restart at every member; a carry stands in front of a continued one
    std::vector<uint8_t> text(T.total), ctx(kSegPrefix);
    for (uint32_t j = 0; j < J; ++j) {
        const bool carried = continues && P.seg_first[j] == 0;
        if (P.seg_first[j] == j) {
            if (carried) ctx = S->carry;
            else ctx.assign(kSegPrefix, 0);
        }
        const uint64_t in_front = T.off[j] - T.off[P.seg_first[j]] + (carried ? S->at.carry_len : 0);
        const uint32_t before = seg_context_before_stream(in_front);
        const uint16_t *sy = sym.data() + P.off()[j] + kSegPrefix;
        uint8_t *dst = text.data() + T.off[j];
        for (uint64_t i = 0; i < n_out[j]; ++i) {
            const uint16_t v = sy[i];
            if ((v >= 256 && !(v & kSegUnknown)) || seg_before_stream(v, before)) return 2;
            dst[i] = v & kSegUnknown ? ctx[v & 0x7fff] : (uint8_t)v;
        }
        const uint64_t n = n_out[j];
        if (n >= kSegPrefix) memcpy(ctx.data(), dst + n - kSegPrefix, kSegPrefix);
        else if (n) memmove(ctx.data(), ctx.data() + n, kSegPrefix - n), memcpy(ctx.data() + kSegPrefix - n, dst, n);
    }
    // ---- CRC-32
    std::vector<ull> blk_off;
    std::vector<uint32_t> blk_len, mem_crc;
    gzip_crc_blocks(P, T, 0xff00, blk_off, blk_len);
    std::vector<uint32_t> crcs(blk_off.size());
    for (size_t b = 0; b < blk_off.size(); ++b) crcs[b] = crc32_of(text.data() + blk_off[b], blk_len[b]);
    if (!gzip_crc_fold(mem, T, blk_len, crcs.data(), 0xff00, o.up, continues ? S->at.open_crc : 0, mem_crc)) return 2;
    // ---- the text stands
    if (S) {
        if (next_in_member) {  // launch_gzip_carry: the last 32 KiB of (prev ++ the open member's text), prev = zeros where it began here
            std::vector<uint8_t> all = gzip_window_continues(S->at, M, next_in_member) ? S->carry : std::vector<uint8_t>(kSegPrefix, 0);
            const uint8_t *open = text.data() + T.last_member_off(P);
            all.insert(all.end(), open, open + T.mem_text[M - 1]);
            S->carry.assign(all.end() - kSegPrefix, all.end());
        }
        gzip_window_stands(S->at, M, T.mem_text[M - 1], mem_crc[M - 1], next_bit, next_in_member);
        for (size_t m = 0; m < M; ++m) S->members += mem[m].closed;
        S->windows += 1;
    }
    out.insert(out.end(), text.begin(), text.end());
    if (n_members) *n_members = M;
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 6 && !strcmp(argv[1], "--isize")) {
        printf("agrees=%d\n", (int)gzip_isize_agrees(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10), (uint32_t)strtoull(argv[4], nullptr, 10), atoi(argv[5]) != 0));
        return 0;
    }
    if (argc != 5) return 2;
    for (uint32_t i = 0; i < 256; ++i) {
        uint32_t c = i;
        for (int k = 0; k < 8; ++k) c = c & 1 ? 0xedb88320u ^ (c >> 1) : c >> 1;
        crc_table[i] = c;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> gz;
    uint8_t buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) gz.insert(gz.end(), buf, buf + got);
    fclose(f);
    const uint64_t n = gz.size(), window = strtoull(argv[2], nullptr, 10), chunk = strtoull(argv[3], nullptr, 10);
    std::vector<mk_gzip_guess> guesses(gzip_member_guesses(gz.data(), n, nullptr, 0));
    gzip_member_guesses(gz.data(), n, guesses.data(), guesses.size());
    std::vector<uint8_t> out;
    Stream S;
    int state = 2, taken = 0;
    uint64_t members = 0;
    if (!guesses.empty() && window == 0) {  // mk_gzip_members_inflate_device
        std::vector<GzCandidate> mem = gzip_file_candidates(guesses, n);
        const uint64_t ratio = gzip_first_ratio(gz.data(), n, mem);
        taken = run(Run{gz.data(), n, ratio, false, true, nullptr, n}, mem, chunk, out, &members, S) == 0;
        state = taken ? 1 : 2;
    } else if (!guesses.empty()) {  // mk_gzip_stream_next until the end or a hand-back
        S.window = window;
        for (;;) {
            if (!S.at.in_member && (S.at.pos_bit >> 3) == n) {
                state = 1;
                break;
            }
            S.grow = 0;
            int st;
            for (;;) {
                const uint64_t base = S.at.pos_bit >> 3, n_up = std::min<uint64_t>(n - base, gzip_window_nominal(S.window, S.grow));
                std::vector<GzCandidate> mem;
                st = gzip_window_candidates(gz.data(), n, guesses, S.at.pos_bit, S.at.in_member, n_up, base + n_up == n, mem);
                if (!st) st = run(Run{gz.data() + base, n_up, 12, true, false, &S, n}, mem, chunk, out, nullptr, S);
                if (st != 3 || !gzip_window_may_grow(S.at.pos_bit, S.window, S.grow, n)) break;
                ++S.grow, ++S.grown;
            }
            if (st != 0) break;  // (3 that cannot grow: handed back)
        }
        taken = state == 1, members = S.members;
    }
    printf("taken=%d state=%d members=%llu windows=%llu grown=%llu repeated=%llu pieces=%llu\n", taken, state, (ull)members, (ull)S.windows, (ull)S.grown, (ull)S.repeated,
           (ull)S.pieces);
    f = fopen(argv[4], "wb");
    if (!f) return 2;
    if (!out.empty()) fwrite(out.data(), 1, out.size(), f);
    fclose(f);
    return 0;
}
