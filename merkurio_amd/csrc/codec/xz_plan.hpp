// xz_plan.hpp -- the host's walk over an .xz file (xz file format specification 1.0.4), no HIP in it: from the file's end, stream by
// stream -- footer, Index, header -- then every Block Header of every stream.  The Index states each block's stored size and text
// size, so the walk ends with a table that says where every block's LZMA2 bytes lie and where its text goes, before a bit is decoded.
// What does not add up is refused with a name (liblzma then words the error); what is valid but not this path's -- SHA-256, filters
// other than one LZMA2, a file of one huge block -- is refused with a name of its own.  Used by xz_host.cpp, xz_chain.hpp and the tests' harnesses.
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "crc64.hpp"

namespace mkz {

constexpr int kXzTruncated = -1, kXzMagic = -2, kXzHeaderCrc = -3, kXzFooter = -4, kXzBackward = -5, kXzIndex = -6, kXzIndexCrc = -7, kXzSizes = -8,
              kXzBlockHeader = -9, kXzBlockHeaderCrc = -10, kXzPadding = -11, kXzCheckKind = -12, kXzFilter = -13, kXzDict = -14, kXzTooManyBlocks = -15,
              kXzTooLarge = -16, kXzSpread = -17, kXzVli = -18, kXzDevice = -19;
constexpr uint32_t kXzMaxBlocks = 1u << 20, kXzStreamPad = 128;  // (the pad: zeros the device reads behind the file, = kStreamPad of inflate_serial.hpp)
constexpr uint32_t kXzDictMax = 3u << 29;                       // 1.5 GiB
constexpr uint32_t kXzSpreadDefault = 107;                      // ceil(2 x r_lzma / r_wave) = ceil(2 x 142.71 / 2.68): profiles/e2e_unxz.txt
constexpr uint32_t kXzCheckNone = 0, kXzCheckCrc32 = 1, kXzCheckCrc64 = 4, kXzCheckSha256 = 10;

// a block as the device reads it (xz_inflate.hip)
struct XzBlock {
    uint64_t in_off, in_bytes;      // its LZMA2 bytes in the file (behind the Block Header; the block padding and the check follow)
    uint64_t text_off, text_bytes;  // its text in the text of the whole file
    uint64_t check_off;             // the stored check in the file
    uint32_t check_kind, dict_size;
};
struct XzPlan {
    std::vector<XzBlock> blocks;
    uint32_t streams = 0, lclp_max = 0;  // lclp_max: xz_plan's; xz_walk leaves it 0
    uint64_t text_total = 0, largest_block_text = 0;
    // beside the table, for a stream's windows (xz_chain.hpp): where each block's Block Header stands in the file, and per stream in
    // file order the blocks in front of its end (a stream without blocks repeats the figure before it)
    std::vector<uint64_t> head_off;
    std::vector<uint32_t> stream_end;
};

inline uint32_t xz_check_bytes(uint32_t kind) { return kind == 0 ? 0u : kind < 4 ? 4u : kind < 7 ? 8u : kind < 10 ? 16u : kind < 13 ? 32u : 64u; }
inline uint32_t xz_le32(const uint8_t *p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

// a multi-byte integer at p[*at ...) inside p[0, end): at most 9 bytes, 63 bits, and no zero byte at its end unless it is its only one
inline bool xz_vli(const uint8_t *p, uint64_t end, uint64_t *at, uint64_t *v) {
    *v = 0;
    for (uint32_t k = 0; k < 9; ++k) {
        if (*at >= end) return false;
        const uint8_t b = p[(*at)++];
        *v |= (uint64_t)(b & 0x7f) << (7 * k);
        if (!(b & 0x80)) return b != 0 || k == 0;
    }
    return false;
}

// the chunk headers of one block's LZMA2 bytes, without decoding: the largest lc + lp any of them sets (the device sizes its
// probabilities by it).  A chunk that does not fit ends the walk: the decoder names what is wrong
inline uint32_t xz_block_lclp(const uint8_t *p, uint64_t n) {
    uint32_t most = 0;
    for (uint64_t at = 0; at < n;) {
        const uint8_t c = p[at];
        if (c == 0 || (c > 2 && c < 0x80)) break;
        if (c < 0x80) {
            if (at + 3 > n) break;
            at += 3 + ((p[at + 1] << 8 | p[at + 2]) + 1u);
            continue;
        }
        if (at + 5 + (c >= 0xC0) > n) break;
        if (c >= 0xC0 && p[at + 5] <= 224) {
            const uint32_t r = p[at + 5] % 45;
            most = std::max(most, std::min<uint32_t>(r / 9 + r % 9, 4));
        }
        at += 5 + (c >= 0xC0) + ((p[at + 3] << 8 | p[at + 4]) + 1u);
    }
    return most;
}

// one Block Header at xz[at ...), of a block whose Index record says (unpadded, text) and whose stream's check is `kind`
inline int xz_block_header(const uint8_t *xz, uint64_t at, uint64_t unpadded, uint64_t text, uint32_t kind, XzBlock &B) {
    const uint32_t hs = ((uint32_t)xz[at] + 1) * 4, cb = xz_check_bytes(kind);  // (xz[at] != 0: an Index stands where the records say a block does)
    if (xz[at] == 0) return kXzSizes;
    if ((uint64_t)hs + cb > unpadded) return kXzSizes;
    const uint8_t *h = xz + at;
    if (xz_crc32(h, hs - 4) != xz_le32(h + hs - 4)) return kXzBlockHeaderCrc;
    const uint8_t flags = h[1];
    if (flags & 0x3c) return kXzBlockHeader;
    uint64_t p = 2, v = 0;
    const uint64_t end = hs - 4, stored = unpadded - hs - cb;
    if (flags & 0x40) {
        if (!xz_vli(h, end, &p, &v)) return kXzVli;
        if (v != stored) return kXzSizes;
    }
    if (flags & 0x80) {
        if (!xz_vli(h, end, &p, &v)) return kXzVli;
        if (v != text) return kXzSizes;
    }
    uint32_t dict = 0;
    int refused = 0;
    for (uint32_t f = 0; f <= (flags & 3u); ++f) {
        uint64_t id = 0, size = 0;
        if (!xz_vli(h, end, &p, &id) || !xz_vli(h, end, &p, &size)) return kXzVli;
        if (size > end - p) return kXzBlockHeader;
        if (id == 0x21 && (flags & 3u) == 0) {
            if (size != 1 || h[p] > 40) return kXzBlockHeader;
            const uint32_t b = h[p];
            dict = b == 40 ? 0xffffffffu : (2u | (b & 1u)) << (b / 2 + 11);
            if (dict > kXzDictMax) refused = kXzDict;
        } else {
            refused = kXzFilter;  // (a chain, or one filter that is not LZMA2: valid perhaps, liblzma's either way)
        }
        p += size;
    }
    for (; p < end; ++p)
        if (h[p]) return kXzPadding;
    if (refused) return refused;
    B.in_off = at + hs, B.in_bytes = stored, B.text_bytes = text, B.check_kind = kind, B.dict_size = dict;
    const uint64_t padded = (unpadded + 3) & ~3ull;
    B.check_off = at + hs + stored + (padded - unpadded);
    for (uint64_t q = at + hs + stored; q < B.check_off; ++q)
        if (xz[q]) return kXzPadding;
    return 0;
}

// the largest lc + lp among the chunks of blocks[0, count), whose in_off counts from xz
inline uint32_t xz_blocks_lclp(const uint8_t *xz, const XzBlock *blocks, size_t count) {
    uint32_t most = 0;
    for (size_t k = 0; k < count; ++k) most = std::max(most, xz_block_lclp(xz + blocks[k].in_off, blocks[k].in_bytes));
    return most;
}

// The container walk: xz[0, n) -> P without lclp_max, or the refusal.  It reads footers, Indexes, stream headers, Block Headers and
// block padding, never a block's LZMA2 bytes: a stream (xz_chain.hpp) runs it once over the mapped file and walks the chunk headers
// window by window.  A file of no bytes is no xz file (kXzTruncated)
inline int xz_walk(const uint8_t *xz, uint64_t n, XzPlan &P) {
    static const uint8_t kMagic[6] = {0xFD, '7', 'z', 'X', 'Z', 0x00};
    P = XzPlan{};
    if (n < 32) return kXzTruncated;
    if (memcmp(xz, kMagic, 6)) return kXzMagic;  // (a file may end in Stream Padding; it may not start with it)
    struct Rec {
        uint64_t unpadded, text;
    };
    std::vector<std::vector<XzBlock>> per_stream;  // last stream first
    std::vector<std::vector<uint64_t>> per_stream_head;
    uint64_t end = n, n_blocks = 0;
    while (end > 0) {
        // ---- Stream Padding: zero bytes in multiples of four
        uint64_t e = end;
        while (e >= 4 && xz_le32(xz + e - 4) == 0) e -= 4;
        if (e == 0) return kXzMagic;
        if (e < 32) return (e & 3) || xz[e - 1] == 0 ? kXzPadding : kXzTruncated;
        // ---- Stream Footer
        const uint8_t *ft = xz + e - 12;
        if (ft[10] != 'Y' || ft[11] != 'Z') return ft[11] == 0 ? kXzPadding : kXzFooter;
        if (xz_crc32(ft + 4, 6) != xz_le32(ft)) return kXzFooter;
        if (ft[8] != 0 || (ft[9] & 0xf0)) return kXzFooter;
        const uint32_t kind = ft[9];
        const uint64_t index_bytes = ((uint64_t)xz_le32(ft + 4) + 1) * 4;
        if (index_bytes + 24 > e) return kXzBackward;
        // ---- Index
        const uint64_t ix = e - 12 - index_bytes;
        const uint8_t *I = xz + ix;
        if (I[0] != 0) return kXzBackward;
        if (xz_crc32(I, index_bytes - 4) != xz_le32(I + index_bytes - 4)) return kXzIndexCrc;
        uint64_t p = 1, count = 0;
        const uint64_t iend = index_bytes - 4;
        if (!xz_vli(I, iend, &p, &count)) return kXzVli;
        if (count > kXzMaxBlocks || (n_blocks += count) > kXzMaxBlocks) return kXzTooManyBlocks;
        std::vector<Rec> recs((size_t)count);
        uint64_t blocks_bytes = 0;
        for (Rec &r : recs) {
            if (!xz_vli(I, iend, &p, &r.unpadded) || !xz_vli(I, iend, &p, &r.text)) return kXzVli;
            if (r.unpadded < 5 || r.unpadded > (1ull << 62)) return kXzIndex;
            blocks_bytes += (r.unpadded + 3) & ~3ull;
            if (blocks_bytes > n) return kXzSizes;
        }
        if (iend - p > 3) return kXzIndex;
        for (; p < iend; ++p)
            if (I[p]) return kXzPadding;
        // ---- Stream Header, where the Index says the blocks start
        if (blocks_bytes + 12 > ix) return kXzSizes;
        const uint64_t s0 = ix - blocks_bytes - 12;
        const uint8_t *hd = xz + s0;
        if (memcmp(hd, kMagic, 6)) return kXzSizes;
        if (xz_crc32(hd + 6, 2) != xz_le32(hd + 8)) return kXzHeaderCrc;
        if (hd[6] != ft[8] || hd[7] != ft[9]) return kXzFooter;
        if (kind != kXzCheckNone && kind != kXzCheckCrc32 && kind != kXzCheckCrc64) return kXzCheckKind;
        // ---- the Block Headers
        std::vector<XzBlock> blocks((size_t)count);
        std::vector<uint64_t> heads((size_t)count);
        uint64_t at = s0 + 12;
        for (size_t k = 0; k < recs.size(); ++k) {
            heads[k] = at;
            const int st = xz_block_header(xz, at, recs[k].unpadded, recs[k].text, kind, blocks[k]);
            if (st) return st;
            at += (recs[k].unpadded + 3) & ~3ull;
        }
        per_stream.push_back(std::move(blocks));
        per_stream_head.push_back(std::move(heads));
        ++P.streams;
        end = s0;
    }
    for (size_t s = per_stream.size(); s-- > 0;) {
        for (XzBlock &B : per_stream[s]) {
            B.text_off = P.text_total;
            if (B.text_bytes > (1ull << 62) || (P.text_total += B.text_bytes) > (1ull << 62)) return kXzTooLarge;
            P.largest_block_text = std::max(P.largest_block_text, B.text_bytes);
            P.blocks.push_back(B);
        }
        P.head_off.insert(P.head_off.end(), per_stream_head[s].begin(), per_stream_head[s].end());
        P.stream_end.push_back((uint32_t)P.blocks.size());
    }
    return 0;
}

// xz[0, n) -> P with lclp_max (the one-shot call sizes its launch by it), or the refusal
inline int xz_plan(const uint8_t *xz, uint64_t n, XzPlan &P) {
    const int st = xz_walk(xz, n, P);
    if (st) return st;
    P.lclp_max = xz_blocks_lclp(xz, P.blocks.data(), P.blocks.size());
    return 0;
}

// a file of one huge block is one wave's serial decode: taken only when the largest block's text x spread <= the whole text
inline bool xz_spread_ok(const XzPlan &P, uint32_t spread) { return P.largest_block_text <= P.text_total / std::max(1u, spread); }

}  // namespace mkz
