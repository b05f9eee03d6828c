// zstd_chain.hpp -- a .zst file of any size decoded window by window (mk_zstd_stream_*, include/merkurio_hip.h): everything the host
// decides about a window.  No HIP in it: zstd_host.cpp runs it with the kernels of zstd_inflate.hip behind `Dev`,
// tests/helpers/zstd_windows_harness.cpp with the serial decoder of zstd_serial.hpp.  Host code only.
//
// Every block header states its block's compressed size, so a window ends at whichever block boundary the walk (zs_walk of
// zstd_plan.hpp) stops at before anything is decoded: behind the first block at which the compressed bytes taken reach the window, or
// at which another block of 128 KiB beside the carried history would not fit the text cap, or the file ends; one block at the least.
// No start is guessed, no window grows.  What a block needs of the blocks in front of it (zstd_serial.hpp) crosses a seam in a small,
// bounded form (ZsCarry):
//   * the tables it repeats: a copy of the bytes that describe the tree and each of the three sequence tables in force behind the
//     window (their exact lengths are the walk's), laid as a PRELUDE of kZsPrelude bytes in front of the window's compressed bytes
//     in the device's input buffer.  A block that repeats one points into the prelude and its wave builds the table as it builds
//     any other: no table crosses a window in decoded form, and the decode kernel is the one-shot call's.  Bound of a description:
//     a tree's is 1 + hb bytes below hb = 128 and 1 + ceil((hb - 127) / 2) from there, 128 at the most; a table's has 4 bits of
//     accuracy log, then per symbol a value of at most log + 1 bits and behind a zero a 2-bit run flag, and a flag of 3 stands for
//     three symbols: below (max symbol + 2) * (max log + 3) + 4 bits = 82 bytes for ML, the largest.  kZsDescMax = 128 holds all
//     four; a longer one is refused, never cut;
//   * the three repeat offsets behind the window's last block, which zs_scan composes;
//   * the text its matches reach into: H = min(frame window, frame text so far) bytes, copied on the device to the front of the next
//     window's text buffer, whose blocks then start at text position H with frame_off = 0 (zs_scan says why that is exact).
// And of the open frame: its window, content size, checksum flag, text so far in 64 bits, and the running XXH64 state -- the content
// checksum stays on the host, because XXH64 does not compose across pieces: a window's new text is hashed as it comes down, and a
// frame's digest is compared when its last block has been decoded.
//
// Whatever does not add up -- anything the walk, a block, a scan or a checksum refuses, no room, a device error -- hands the file
// back (state 2) with nothing of that window delivered.  The windows in front of it passed every check but a checksum that was not
// due yet: they are what libzstd writes for those bytes before it refuses.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../../include/merkurio_hip.h"
#include "xxh64.hpp"
#include "zstd_plan.hpp"

namespace mkz {

constexpr uint64_t kZsStreamWindow = 256ull << 20;  // the default window (an unmeasured choice: README, profiles/e2e_unzstd_windows.txt)
constexpr uint32_t kZsDescMax = 128;                // bytes of one carried description (derived above)
constexpr uint32_t kZsPrelude = 4 * kZsDescMax;     // tree | LL | OF | ML, a slot each
constexpr uint32_t kZsDefCarried = 0xfffffffeu;     // ZsBlock::def_block of a table that was defined in an earlier window (the kernels do not read it)
// a window's text, history included, stays below 4 GiB (a source is a 32-bit position): the largest text cap
constexpr uint64_t kZsTextCapMax = (1ull << 32) - (1ull << 28);

// what is carried from window to window, and nothing else (the totals are the stats)
struct ZsCarry {
    bool open = false;  // a frame is open behind the window
    uint64_t window = 0, content_size = ~0ull, text = 0;  // of the open frame; text: all of it so far
    bool has_checksum = false;
    Xxh64 xxh;                      // over the open frame's text so far
    uint32_t rep[3] = {1, 4, 8};    // the repeat offsets behind the last block
    struct Tab {
        bool have = false;  // the frame has one in force
        uint8_t mode = 0;   // (tree: unused) 0 predefined -- no bytes --, 1 one symbol, 2 described
        uint32_t len = 0;
        uint8_t bytes[kZsDescMax];
    } tab[4];  // tree, LL, OF, ML
    uint32_t windows = 0;  // windows the open frame has blocks in so far
    uint64_t history() const { return open ? std::min(window, text) : 0; }
};

// what the seams of a stream cut (the tests' census; the device path does not read it)
struct ZsSeams {
    uint64_t treeless_carried = 0;    // treeless blocks whose tree was defined in an earlier window
    uint64_t repeat_carried[3][3] = {};  // LL / OF / ML repeated from an earlier window's predefined / one-symbol / described table
    uint64_t frame_end_at_seam = 0;   // windows that end with a frame's last block while the file goes on
    uint64_t skippable_at_seam = 0;   // windows behind the first that start at a skippable frame
    uint64_t two_frames = 0;          // windows with blocks of two frames or more
    uint64_t checksum_3_windows = 0;  // frames with a checksum that closed after blocks in three windows or more
    uint64_t history_below_window = 0, history_at_window = 0;  // windows that start inside a frame with H below / equal to its window
};

struct ZsWindow {
    uint64_t from = 0, to = 0;  // the window's compressed bytes in the file
    uint8_t prelude[kZsPrelude];
    ZsPlan P;                   // its blocks, positions counted in the device's input: prelude | zs[from, to)
    uint64_t n_in() const { return kZsPrelude + (to - from); }
};

struct ZsStream {
    const uint8_t *zs = nullptr;  // the whole file, the caller's
    uint64_t n = 0, window = 0, text_cap = 0;  // text_cap 0: what the device says
    ZsWalk at;
    ZsCarry carry;
    bool dead = false;
    ZsWindow W;
    mk_zstd_stream_stats stats{};
    ZsSeams seams;
    ZsCensus census;  // summed over the windows
};

inline bool zs_stream_open(ZsStream &S, const uint8_t *zs, uint64_t n, uint64_t window) {
    if (n < 4) return false;
    const uint32_t magic = (uint32_t)zs_le(zs, 4);
    if (magic != kZsMagic && (magic & 0xfffffff0u) != kZsSkipMagic) return false;
    S = ZsStream();
    S.zs = zs, S.n = n, S.window = window ? window : kZsStreamWindow;
    return true;
}

// the blocks a window may take beside `history` bytes under a text cap: another block of 128 KiB has to fit; one at the least
inline uint64_t zs_window_blocks(uint64_t text_cap, uint64_t history) {
    text_cap = std::min(text_cap, kZsTextCapMax);
    return text_cap > history ? std::max<uint64_t>(1, (text_cap - history) / kZsBlockMax) : 1;
}

// the walk's references to what is in force become references into the prelude, which is filled from the carry
inline void zs_carry_to_walk(const ZsCarry &C, ZsWalk &at, uint8_t *prelude) {
    memset(prelude, 0, kZsPrelude);
    if (!C.open) return;
    for (uint32_t k = 0; k < 4; ++k) {
        const ZsCarry::Tab &T = C.tab[k];
        ZsTabRef &R = k == 0 ? at.huf : at.tab[k - 1];
        if (!T.have) continue;
        memcpy(prelude + k * kZsDescMax, T.bytes, T.len);
        R.src = k * kZsDescMax, R.lim = R.src + T.len, R.len = T.len, R.mode = T.mode;
        R.def = k && T.mode == 0 ? ~0u : kZsDefCarried;  // (Repeat of a predefined table names no block, as within a window)
    }
}
// ... and behind the window the carry copies what is in force then: out of the file, or what it held already.  false: a description
// above the bound
inline bool zs_walk_to_carry(const ZsWalk &at, const uint8_t *zs, ZsCarry &C) {
    for (uint32_t k = 0; k < 4; ++k) {
        ZsCarry::Tab &T = C.tab[k];
        const ZsTabRef &R = k == 0 ? at.huf : at.tab[k - 1];
        const bool have = k == 0 ? at.have_huf : at.have_tabs;
        if (!have) {
            T.have = false;
            continue;
        }
        if (R.def == kZsDefCarried) continue;  // (still the carried one)
        if (k && R.mode == 0) {  // predefined: no bytes
            T.have = true, T.mode = 0, T.len = 0;
            continue;
        }
        if (R.len > kZsDescMax) return false;
        T.have = true, T.mode = R.mode, T.len = R.len;
        if (R.len) memcpy(T.bytes, zs + R.src, R.len);
    }
    return true;
}

// positions of the file -> positions of the device's input (prelude | zs[from, to)); a carried reference stands as it is
inline void zs_window_rebase(ZsWindow &W, ZsSeams &seams) {
    const uint64_t d = W.from - kZsPrelude;  // (modulo 2^64 where the window starts in front of byte kZsPrelude)
    for (ZsBlock &B : W.P.blocks) {
        B.src -= d;
        if (B.type != 2) continue;
        B.bits_src -= d;
        const bool carried_tree = B.lit_type == 3 && B.def_block[0] == kZsDefCarried;
        if (B.lit_type < 2) B.huf_src = B.huf_lim = 0;
        else if (!carried_tree) B.huf_src -= d, B.huf_lim -= d;
        seams.treeless_carried += carried_tree;
        for (uint32_t t = 0; t < 3; ++t) {
            if (!B.n_seq) continue;
            const bool carried = B.def_block[1 + t] == kZsDefCarried;
            if (carried) seams.repeat_carried[t][B.mode[t]]++;
            if (B.mode[t] == 0) B.tab_src[t] = B.tab_lim[t] = 0;  // (predefined, carried or not: reads no bytes)
            else if (!carried) B.tab_src[t] -= d, B.tab_lim[t] -= d;
        }
    }
}

// One call of mk_zstd_stream_next.  Dev is the device (or the harness's stand-in):
//   uint64_t text_room()
//        the default text cap: bytes of text, history included, a window may hold
//   bool decode(const ZsWindow &W, std::vector<ZsReport> &rep)
//        prelude and compressed bytes go up, every block's tables are built and its literals and sequences decoded -> rep
//   bool execute(const ZsWindow &W, const std::vector<ZsStart> &start, uint64_t history, uint64_t total, uint32_t *rounds)
//        the last `history` bytes of the latest window's text are copied to the front of the text buffer it does not lie in; the
//        blocks are executed behind them, text below `history` settled; rounds of resolution over [history, total) -> how many.
//        false: a block's status, more rounds than zs_round_cap(blocks), no room, any error
//   bool hash(uint64_t off, uint64_t len, Xxh64 &h)
//        text [off, off + len) of that buffer comes down through h
//   void commit(uint64_t history, uint64_t total)
//        the window stands: that buffer is the latest window's, its new text [history, total)
// *state as the header says: 0 = *text_bytes of new text stand in that buffer, 1 = end of file, 2 = handed back.
template <class Dev>
void zs_stream_next(ZsStream &S, Dev &dev, uint64_t *text_bytes, uint32_t *state) {
    *text_bytes = 0, *state = 2;
    if (S.dead) return;
    if (!S.at.open && S.at.at == S.n) {
        *state = 1;
        return;
    }
    S.dead = true;  // (until the window stands)
    ZsWindow &W = S.W;
    ZsCarry &C = S.carry;
    const uint64_t H = C.history();
    const bool first_window = S.stats.windows == 0;
    W.P = ZsPlan{};
    W.from = S.at.at;
    zs_carry_to_walk(C, S.at, W.prelude);
    if (!first_window && !S.at.open && S.n - S.at.at >= 4 && ((uint32_t)zs_le(S.zs + S.at.at, 4) & 0xfffffff0u) == kZsSkipMagic) S.seams.skippable_at_seam++;
    const uint64_t cap = S.text_cap ? S.text_cap : dev.text_room();
    if (!zs_walk(S.zs, S.n, S.at, ZsLimit{S.window, zs_window_blocks(cap, H)}, W.P)) return;
    W.to = S.at.at;
    zs_window_rebase(W, S.seams);
    const size_t B = W.P.blocks.size();
    if (B >= (1u << 30)) return;
    // ---- tables + entropy decode, the scans, execution and rounds
    std::vector<ZsReport> rep;
    if (B) {
        if (!dev.decode(W, rep) || rep.size() != B) return;
        for (const ZsReport &r : rep)
            if (r.status != 0) return;
    }
    ZsScanFrom from;
    from.history = H, from.frame_text = C.text;
    for (int k = 0; k < 3; ++k) from.rep[k] = C.rep[k];
    std::vector<ZsStart> start;
    uint64_t total = 0;
    uint32_t rep_out[3] = {1, 4, 8}, rounds = 0;
    if (!zs_scan(W.P, rep, start, &total, &from, rep_out)) return;
    if ((B || H) && !dev.execute(W, start, H, total, &rounds)) return;
    // ---- content checksums: every frame's new text through its hash, the digest where the frame closes
    uint64_t closed = 0, with_blocks = 0;
    for (const ZsFrame &F : W.P.frames) {
        with_blocks += F.n_blocks != 0;
        const uint32_t windows = (F.continued ? C.windows : 0) + (F.n_blocks != 0);
        if (F.has_checksum) {
            Xxh64 h = F.continued ? C.xxh : Xxh64();
            if (F.text_len && !dev.hash(F.text_off, F.text_len, h)) return;
            if (F.closed && (uint32_t)h.digest() != F.checksum) return;
            if (!F.closed) C.xxh = h;
            if (F.closed && windows >= 3) S.seams.checksum_3_windows++;
        }
        closed += F.closed;
    }
    // ---- the window stands: what the next one starts from
    if (H) (H < C.window ? S.seams.history_below_window : S.seams.history_at_window)++;
    if (S.at.open) {
        const ZsFrame &F = W.P.frames.back();
        C.text = (F.continued ? C.text : 0) + F.text_len;
        C.windows = (F.continued ? C.windows : 0) + (F.n_blocks != 0);
        C.open = true, C.window = F.window, C.content_size = F.content_size, C.has_checksum = F.has_checksum;
        if (!F.continued && !F.has_checksum) C.xxh = Xxh64();
        for (int k = 0; k < 3; ++k) C.rep[k] = rep_out[k];
        if (!F.continued)
            for (ZsCarry::Tab &T : C.tab) T.have = false;
        if (!zs_walk_to_carry(S.at, S.zs, C)) return;
    } else {
        C = ZsCarry();
        if (S.at.at < S.n && closed) S.seams.frame_end_at_seam++;
    }
    S.seams.two_frames += with_blocks >= 2;
    for (size_t k = 0; k < sizeof(ZsCensus) / 8; ++k) ((uint64_t *)&S.census)[k] += ((const uint64_t *)&W.P.census)[k];
    dev.commit(H, total);
    S.stats.windows += 1, S.stats.frames += closed, S.stats.blocks += B, S.stats.consumed_bytes = S.at.at, S.stats.text_bytes += total - H;
    S.stats.rounds += rounds, S.stats.max_history = std::max<uint64_t>(S.stats.max_history, H);
    S.dead = false;
    *text_bytes = total - H, *state = 0;
}

}  // namespace mkz
