// bzip2_chain.hpp -- a .bz2 file of any size decoded window by window (mk_bzip2_stream_*, include/merkurio_hip.h): everything the
// host decides about a window.  No HIP in it: bzip2_host.cpp runs it with the kernels of bzip2_inflate.hip behind `Dev`,
// tests/helpers/bzip2_windows_harness.cpp with bz2_find_markers and the serial decoder of bzip2_serial.hpp.  Host code only.
//
// A window is the compressed bytes from the byte that holds the previous cut's bit up to `window` bytes further on.  Its magics
// (every bit offset tested) are walked as bz2_plan walks a file's, from a magic that is KNOWN -- the cut of the window before, or
// the file's first: a block magic opens a block that must end exactly on the next magic of the table, and is decoded only when
// that magic lies inside the upload.  The cut is the last magic of the window; the bytes behind it go up again with the next one.
// An end-of-stream magic is consumed only when what decides the bytes behind it lies inside the upload too -- its 32 CRC bits, the
// padding to the byte, and either the file's end or "BZh" + level + the next stream's first magic --; otherwise the cut is that end
// magic.  bzip2 blocks need nothing of each other, so what is carried from window to window is small (BzStreamPos): the next bit,
// whether a stream is open, its level, and the CRC of its blocks so far, folded with bz2_stream_crc_fold.
//
// A window without a block and without a consumed stream end (a block longer than a tiny window, an incompressible block of 1.1 MB)
// is doubled and tried again.  Text is not bounded by compressed bytes (900 000 symbols expand to 46 MB behind the run-length
// step), so a window's blocks are delivered as one or several TEXT windows, each a prefix of whole blocks (at least one) that fits
// the text room; the bytes in front of the run-length step stay where the decode left them until the last one is delivered.
//
// What does not add up -- a table that does not chain, a block that does not end on its magic, a status of the decoder, a wrong block
// or stream CRC, bytes behind the last stream, data that ends early -- hands the file back (state 2).  The whole blocks in front of
// it are still delivered, then the next call says 2: what was delivered is a prefix of what libbz2 gives before it refuses, which
// writes a block's text before it looks at what follows the block.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../../include/merkurio_hip.h"
#include "bzip2_stream.hpp"

namespace mkz {

constexpr uint64_t kBzStreamWindow = 256ull << 20;  // the default window (an unmeasured choice: README, profiles/e2e_bunzip2_windows.txt)
constexpr uint32_t kBzWinMaxMarkers = 1u << 20;     // magics of one upload; more: handed back

// what is carried from window to window, and nothing else (the totals are the stats)
struct BzStreamPos {
    uint64_t pos_bit = 0;  // the next window's first bit: a magic of the open stream (a cut is a magic: proved, not guessed)
    bool open = false;     // false: every stream is closed and the file has ended behind the last one
    uint32_t level = 0;    // of the open stream
    uint32_t crc = 0;      // of the open stream's blocks so far, folded
};

struct BzWinBlock {
    uint64_t bit, end_bit;  // its magic, and the magic it must end on: bits of the upload
    uint32_t level;
};
struct BzWinEnd {
    uint32_t after_blocks;  // a stream ends behind this many blocks of the window (0: its last block lay in an earlier window)
    uint32_t crc;           // as the file has it
};
struct BzWindow {
    uint64_t base_bit = 0;  // of the upload's first byte in the file
    std::vector<BzWinBlock> blocks;
    std::vector<BzWinEnd> ends;
    uint64_t next_bit = 0;  // where the next window starts when all of this one stands (a bit of the file)
    bool next_open = false;
    uint32_t next_level = 0;
    bool fault = false;  // behind these blocks and ends the file does not add up
};

inline uint64_t bz2_window_bytes(uint64_t window, uint32_t grow) { return window << grow; }
inline uint32_t bz2_marker_cap(uint64_t n_up) { return (uint32_t)std::min<uint64_t>(n_up / 6 + 2, kBzWinMaxMarkers); }
// may the window that starts at pos_bit be doubled once more?  (Not when it reaches the file's end already)
inline bool bz2_window_may_grow(uint64_t pos_bit, uint64_t window, uint32_t grow, uint64_t n_file) {
    return grow < 48 && bz2_window_bytes(window, grow) < n_file - (pos_bit >> 3);
}

// The window that starts at bit at.pos_bit of the file (a magic of the open stream) and whose upload up[0, n_up) starts at the byte
// that holds that bit; is_last: the upload reaches the file's end.  markers: every magic that lies whole inside the upload, sorted,
// bits of the upload.  -> W.  No block, no end and no fault: the window has to grow.
inline void bz2_window_plan(const uint8_t *up, uint64_t n_up, bool is_last, const BzStreamPos &at, const std::vector<BzMarker> &markers, BzWindow &W) {
    W = BzWindow{};
    W.base_bit = (at.pos_bit >> 3) * 8;
    uint64_t pos = at.pos_bit - W.base_bit;
    uint32_t level = at.level;
    bool open = true;
    size_t m = 0;
    const size_t M = markers.size();
    while (m < M && markers[m].bit < pos) ++m;  // (bits of the first byte in front of the cut: the block before, which has been proved)
    for (;;) {
        if (m >= M || markers[m].bit != pos) {  // no magic where one must stand -- or not yet: the data ends inside it
            W.fault = m < M || is_last;
            break;
        }
        if (markers[m].kind == 0) {
            if (m + 1 >= M) {  // its closing magic is not inside the upload: the cut
                W.fault = is_last;
                break;
            }
            W.blocks.push_back(BzWinBlock{pos, markers[m + 1].bit, level});
            pos = markers[++m].bit;
            continue;
        }
        const uint64_t crc_bit = pos + 48, after = (crc_bit + 32 + 7) >> 3;  // after: the first byte behind the stream
        if (after > n_up) {
            W.fault = is_last;
            break;
        }
        uint32_t crc = 0;
        for (uint32_t k = 0; k < 32; ++k) crc = crc << 1 | (up[(crc_bit + k) >> 3] >> (7 - ((crc_bit + k) & 7)) & 1u);
        const BzWinEnd end{(uint32_t)W.blocks.size(), crc};
        if (after == n_up && is_last) {  // the file ends behind the stream
            W.ends.push_back(end);
            open = false, pos = after * 8;
            break;
        }
        if (after + 10 > n_up) {  // "BZh" + level + a magic do not fit: the next window's to see -- or, at the file's end, trailing bytes
            if (is_last) W.ends.push_back(end), W.fault = true;
            break;
        }
        size_t q = m + 1;
        while (q < M && markers[q].bit < (after + 4) * 8) ++q;
        if (up[after] != 'B' || up[after + 1] != 'Z' || up[after + 2] != 'h' || up[after + 3] < '1' || up[after + 3] > '9' || q >= M || markers[q].bit != (after + 4) * 8) {
            W.ends.push_back(end), W.fault = true;  // bytes behind the stream that are no stream
            break;
        }
        W.ends.push_back(end);
        level = (uint32_t)(up[after + 3] - '0'), pos = (after + 4) * 8, m = q;
    }
    W.next_bit = W.base_bit + pos, W.next_open = open, W.next_level = level;
}

// only blocks [0, B) of the window stay (B < blocks.size()): the next window starts at block B's magic.  What the plan found wrong
// behind it is the next window's to find again
inline void bz2_window_cut(BzWindow &W, uint32_t B) {
    W.next_bit = W.base_bit + W.blocks[B].bit, W.next_open = true, W.next_level = W.blocks[B].level;
    W.blocks.resize(B);
    while (!W.ends.empty() && W.ends.back().after_blocks > B) W.ends.pop_back();
    W.fault = false;
}

// the proof of a guess: a block decodes (status 0, the walk's included) and ends exactly on the magic behind it.  The first block
// that does not: the window is cut in front of it and faulted
inline void bz2_window_prove(BzWindow &W, const std::vector<Bz2Block> &rep) {
    for (size_t k = 0; k < W.blocks.size(); ++k)
        if (rep[k].status != 0 || rep[k].end_bit != W.blocks[k].end_bit) {
            bz2_window_cut(W, (uint32_t)k);
            W.fault = true;
            return;
        }
}

// Blocks [b0, b1) of the window have been expanded; crc[k - b0] = bzip2's CRC of block k's text.  Every block's CRC must be the
// one its header says; folded into run_crc (the open stream's), which must be what the file says wherever a stream ends behind one
// of these blocks (b0 = 0: in front of the first one too).  -> how many of the blocks stand: b1 - b0, or fewer with *bad set -- a
// block's own CRC is wrong (it does not stand), or a stream's (its last block still does: libbz2 has written it by then)
inline uint32_t bz2_window_fold(const BzWindow &W, const std::vector<Bz2Block> &rep, uint32_t b0, uint32_t b1, const uint32_t *crc, uint32_t &run_crc, size_t &next_end,
                                uint64_t &streams, bool *bad) {
    *bad = true;
    auto ends_behind = [&](uint32_t blocks) {
        for (; next_end < W.ends.size() && W.ends[next_end].after_blocks == blocks; ++next_end, ++streams) {
            if (run_crc != W.ends[next_end].crc) return false;
            run_crc = 0;
        }
        return true;
    };
    if (b0 == 0 && !ends_behind(0)) return 0;
    for (uint32_t k = b0; k < b1; ++k) {
        if (crc[k - b0] != rep[k].crc) return k - b0;
        run_crc = bz2_stream_crc_fold(run_crc, crc[k - b0]);
        if (!ends_behind(k + 1)) return k + 1 - b0;
    }
    *bad = false;
    return b1 - b0;
}

// ---- the stream
struct BzStream {
    const uint8_t *bz = nullptr;  // the whole file, the caller's
    uint64_t n = 0, window = 0;
    BzStreamPos at;
    uint32_t grow = 0;
    bool dead = false;   // handed back (state 2): nothing more is produced
    bool fault = false;  // what stood in front of a fault has been delivered: the next call hands back
    // the window whose blocks are decoded and not all delivered yet
    bool pending = false;
    BzWindow W;
    std::vector<Bz2Block> rep;
    std::vector<unsigned long long> text_len;
    uint32_t b_next = 0;  // its first block that has not been delivered
    size_t next_end = 0;  // its first stream end that has not been checked
    mk_bzip2_stream_stats stats{};
};

// "BZh1-9" at byte 0: the stream is open in front of the first magic
inline bool bz2_stream_open(BzStream &S, const uint8_t *bz, uint64_t n, uint64_t window) {
    if (n < 4 || bz[0] != 'B' || bz[1] != 'Z' || bz[2] != 'h' || bz[3] < '1' || bz[3] > '9') return false;
    S = BzStream{};
    S.bz = bz, S.n = n, S.window = window ? window : kBzStreamWindow;
    S.at.pos_bit = 32, S.at.open = true, S.at.level = (uint32_t)(bz[3] - '0');
    return true;
}

// One call of mk_bzip2_stream_next.  Dev is the device (or the harness's stand-in):
//   bool upload(const uint8_t *up, uint64_t n_up, std::vector<BzMarker> &markers)
//        the bytes go up, the magics that lie whole inside them come back sorted (bits of the upload); false: no room, too many
//        magics, any error
//   uint32_t decode(const std::vector<BzWinBlock> &blocks, std::vector<Bz2Block> &rep, std::vector<unsigned long long> &text_len)
//        blocks decoded from their magics and walked, in order -> how many: all of them, fewer where there is no room for more or
//        where one did not prove (the blocks behind it need not be run), 0: none
//   uint64_t text_room()
//        bytes of text the next text window may hold (a single block that is longer is tried all the same)
//   bool expand(uint32_t b0, uint32_t b1, const unsigned long long *text_off, uint64_t total, uint32_t *crc)
//        blocks [b0, b1) of the decoded window -> `total` bytes of text in the text buffer that the latest text window does not lie in,
//        block k at text_off[k - b0], and the CRC of each
// *state as the header says: 0 = *text_bytes of text stand in that buffer, 1 = end of file, 2 = handed back.
template <class Dev>
void bz2_stream_next(BzStream &S, Dev &dev, uint64_t *text_bytes, uint32_t *state) {
    *text_bytes = 0, *state = 2;
    if (S.dead) return;
    if (!S.pending) {
        if (S.fault) {
            S.dead = true;
            return;
        }
        if (!S.at.open) {
            *state = 1;
            return;
        }
        for (S.grow = 0;; ++S.grow, ++S.stats.windows_grown) {
            const uint64_t base = S.at.pos_bit >> 3;
            const uint64_t n_up = std::min<uint64_t>(S.n - base, bz2_window_bytes(S.window, S.grow));
            std::vector<BzMarker> markers;
            if (!dev.upload(S.bz + base, n_up, markers)) {
                S.dead = true;
                return;
            }
            bz2_window_plan(S.bz + base, n_up, base + n_up == S.n, S.at, markers, S.W);
            if (!S.W.blocks.empty() || !S.W.ends.empty()) break;
            if (S.W.fault || !bz2_window_may_grow(S.at.pos_bit, S.window, S.grow, S.n)) {
                S.dead = true;
                return;
            }
        }
        if (!S.W.blocks.empty()) {
            const uint32_t done = dev.decode(S.W.blocks, S.rep, S.text_len);
            if (done == 0) {
                S.dead = true;
                return;
            }
            if (done < S.W.blocks.size()) bz2_window_cut(S.W, done);  // (no room for more: the rest is the next window's)
            bz2_window_prove(S.W, S.rep);
        }
        S.b_next = 0, S.next_end = 0, S.pending = true;
    }
    // ---- the next text window of the decoded one: a prefix of its whole blocks, at least one
    const uint32_t B = (uint32_t)S.W.blocks.size(), b0 = S.b_next;
    uint32_t b1 = b0;
    uint64_t total = 0;
    std::vector<unsigned long long> text_off;
    const uint64_t room = B ? dev.text_room() : 0;
    while (b1 < B && (b1 == b0 || total + S.text_len[b1] <= room)) text_off.push_back(total), total += S.text_len[b1++];
    std::vector<uint32_t> crc(b1 - b0);
    if (b1 > b0 && !dev.expand(b0, b1, text_off.data(), total, crc.data())) {
        S.dead = true;
        return;
    }
    bool bad = false;
    uint64_t streams = 0;
    const uint32_t good = bz2_window_fold(S.W, S.rep, b0, b1, crc.data(), S.at.crc, S.next_end, streams, &bad);
    if (bad || (B == 0 && S.W.fault)) {
        if (good == 0) {  // nothing stands in front of it
            S.dead = true;
            return;
        }
        if (good < b1 - b0) total = text_off[good];
        S.fault = true, S.pending = false;
    } else {
        S.b_next = b1;
        if (b1 == B) {  // the window stands: what the next one starts from
            S.pending = false;
            S.at.pos_bit = S.W.next_bit, S.at.open = S.W.next_open, S.at.level = S.W.next_level;
            S.fault = S.W.fault;
            S.stats.consumed_bytes = S.at.pos_bit >> 3;
        }
    }
    S.stats.windows += 1, S.stats.streams += streams, S.stats.blocks += good, S.stats.text_bytes += total;
    *text_bytes = total, *state = 0;
}

}  // namespace mkz
