// zstd_plan.hpp -- the host's walk over a .zst file before anything is decoded (RFC 8878 3.1): frame headers, skippable frames, frames
// back to back, every 3-byte block header, and of a compressed block the literals-section header and the sequences-section header with
// its table descriptions, which can be read without entropy decoding.  It yields, per block, what zstd_serial.hpp's ZsBlock says -- byte
// range, type, literal and sequence counts, the three modes, and for every table the block repeats the bytes that describe it and the
// block they stand in -- and with them the exact size of the literal buffer and of the sequence arrays.  "Repeat" means the table of
// the previous compressed block with sequences, which may itself have been predefined or one symbol; "treeless" the tree of the last
// block that described one.  No HIP in it: the CPU harness runs it as the library does.
//
// Refused here (status of zstd_serial.hpp): a magic that starts no frame -- legacy ones included -- or bytes behind the last frame, a
// reserved bit in the frame header descriptor, a dictionary id other than 0, a window above 2^27 bytes, a block above min(window,
// 128 KiB), a compressed block under 3 bytes or of 128 KiB (libzstd's bounds), the Reserved block type, Repeat or treeless with nothing to repeat, reserved bits in the modes byte, a section that does not
// fit its block, data that ends early.
#pragma once
#include <vector>

#include "zstd_serial.hpp"

namespace mkz {

struct ZsFrame {
    uint64_t window, content_size;  // content_size: ~0 = the header has none
    uint64_t text_off, text_len;    // (filled in once the blocks' sizes are known)
    uint32_t first_block, n_blocks, checksum;
    bool has_checksum;
    bool continued, closed;  // of a walk that starts or stops inside the frame: it began in front of the walk / it ended inside it
};
// what a file exercised (the tests' census)
struct ZsCensus {
    uint64_t block_type[3] = {0, 0, 0}, lit_type[4] = {0, 0, 0, 0}, lit_format[4][4] = {}, streams[2] = {0, 0};
    uint64_t mode[3][4] = {}, repeat_of[3][3] = {}, seq_form[4] = {0, 0, 0, 0}, huf_direct = 0, huf_fse = 0;
    uint64_t fcs_bytes[5] = {0, 0, 0, 0, 0}, single_segment = 0, skippable = 0, frames = 0, empty_frames = 0, checksums = 0;
};
struct ZsPlan {
    std::vector<ZsBlock> blocks;
    std::vector<ZsFrame> frames;
    uint64_t lit_bytes = 0, n_seq = 0;
    ZsCensus census;
    int status = 0;
};

struct ZsNoOut {
    int16_t norm[64];
    bool leader() const { return true; }
    uint32_t first() const { return 0; }
    uint32_t step() const { return 1; }
    void sync() const {}
};

inline uint64_t zs_le(const uint8_t *p, uint32_t k) {
    uint64_t v = 0;
    for (uint32_t i = 0; i < k; ++i) v |= (uint64_t)p[i] << (8 * i);
    return v;
}

// ---- the walk, resumable.  Where it stands (ZsWalk): a byte that is a frame start, a skippable frame or the file's end -- or, `open`,
// a block header of frame F, with what a later block of F may repeat: the tree, and per sequence table its mode, the bytes that
// describe it, their exact length and the block that defined it.  A stream (zstd_chain.hpp) keeps one from window to window
struct ZsTabRef {
    uint64_t src = 0, lim = 0;
    uint32_t def = ~0u, len = 0;  // len: bytes of the description (tree: 1 + hb below 128, 1 + ceil((hb - 127) / 2) from there; table: what zs_read_fse returns, 1 for one symbol)
    uint8_t mode = 0;
};
struct ZsWalk {
    uint64_t at = 0;
    bool open = false;
    ZsFrame F{};
    bool have_huf = false, have_tabs = false;
    ZsTabRef huf, tab[3];
};
// where a walk stops: behind the first block at which the bytes taken reach `bytes` or the blocks taken `blocks` (0: no such limit),
// at the file's end at the latest.  At least one block is taken
struct ZsLimit {
    uint64_t bytes = 0, blocks = 0;
};

// the walk from W over zs[0, n), appended to P (B.frame and def_block count in P's tables) -> W, where the next one starts.  A
// frame that is open at either end stands in P.frames all the same (continued / closed).  false: refused, P.status says why
inline bool zs_walk(const uint8_t *zs, uint64_t n, ZsWalk &W, const ZsLimit &lim, ZsPlan &P) {
    auto fail = [&](int st) {
        P.status = st;
        return false;
    };
    ZsIn<ZsHostWords> in;
    in.w = ZsHostWords{zs, n};
    ZsNoOut no;
    uint64_t &at = W.at;
    const uint64_t from = at;
    uint64_t taken = 0;
    bool full = false;
    if (W.open) W.F.first_block = (uint32_t)P.blocks.size(), W.F.continued = true;
    while (!full && (W.open || at < n)) {
        if (!W.open) {
            if (n - at < 4) return fail(kZsTrailing);
            const uint32_t magic = (uint32_t)zs_le(zs + at, 4);
            if ((magic & 0xfffffff0u) == kZsSkipMagic) {
                if (n - at < 8) return fail(kZsTruncated);
                const uint64_t len = zs_le(zs + at + 4, 4);
                if (len > n - at - 8) return fail(kZsTruncated);
                at += 8 + len, P.census.skippable++;
                continue;
            }
            if (magic != kZsMagic) return fail(at ? kZsTrailing : kZsMagicBad);
            at += 4;
            // ---- frame header
            if (at >= n) return fail(kZsTruncated);
            const uint32_t fhd = zs[at++];
            const uint32_t fcs_flag = fhd >> 6, single = fhd >> 5 & 1u, did_flag = fhd & 3u;
            if (fhd & 8u) return fail(kZsReservedBit);
            ZsFrame F{};
            F.has_checksum = fhd >> 2 & 1u;
            F.content_size = ~0ull;
            if (!single) {
                if (at >= n) return fail(kZsTruncated);
                const uint32_t wd = zs[at++];
                const uint64_t base = 1ull << (10 + (wd >> 3));
                F.window = base + (base >> 3) * (wd & 7u);
            }
            const uint32_t did_bytes = did_flag == 3 ? 4u : did_flag, fcs_bytes = fcs_flag == 0 ? single : 1u << fcs_flag;
            if (n - at < did_bytes + fcs_bytes) return fail(kZsTruncated);
            if (zs_le(zs + at, did_bytes) != 0) return fail(kZsDictionary);
            at += did_bytes;
            if (fcs_bytes) F.content_size = zs_le(zs + at, fcs_bytes) + (fcs_bytes == 2 ? 256u : 0u);
            at += fcs_bytes;
            if (single) F.window = F.content_size;
            if (F.window > kZsWindowMax) return fail(kZsWindow);
            P.census.fcs_bytes[fcs_bytes == 8 ? 4 : fcs_bytes == 4 ? 3 : fcs_bytes]++, P.census.single_segment += single, P.census.frames++,
                P.census.checksums += F.has_checksum;
            F.first_block = (uint32_t)P.blocks.size();
            // what a later block of the frame may repeat: nothing yet
            W.F = F, W.open = true, W.have_huf = W.have_tabs = false, W.huf = ZsTabRef{};
            for (ZsTabRef &t : W.tab) t = ZsTabRef{};
        }
        // ---- a block of the open frame
        ZsFrame &F = W.F;
        const uint64_t block_max = F.window < kZsBlockMax ? F.window : kZsBlockMax;
        {
            if (n - at < 3) return fail(kZsTruncated);
            const uint32_t bh = (uint32_t)zs_le(zs + at, 3);
            at += 3;
            const uint32_t last = bh & 1u, type = bh >> 1 & 3u, size = bh >> 3;
            if (type == 3) return fail(kZsBlockType);
            if (size > block_max) return fail(kZsBlockSize);
            const uint64_t content = type == 1 ? 1u : size;
            if (content > n - at) return fail(kZsTruncated);
            ZsBlock B{};
            B.src = at, B.size = size, B.type = (uint8_t)type, B.frame = (uint32_t)P.frames.size();
            for (uint32_t &d : B.def_block) d = ~0u;
            const uint32_t self = (uint32_t)P.blocks.size();
            if (type == 2) {
                const uint64_t end = at + size;
                // (libzstd takes a compressed block of 3 bytes at the least and of less than 128 KiB: a larger one would have been stored raw)
                if (size < 3 || size >= kZsBlockMax) return fail(kZsBlockSize);
                // ---- literals-section header
                const uint32_t b0 = zs[at], lt = b0 & 3u, sf = b0 >> 2 & 3u;
                uint32_t hdr, regen, comp = 0, streams = 1;
                if (lt < 2) {
                    hdr = sf == 1 ? 2 : sf == 3 ? 3 : 1;
                    if (hdr > size) return fail(kZsSection);
                    regen = (uint32_t)(zs_le(zs + at, hdr) >> (hdr == 1 ? 3 : 4));
                    comp = lt == 0 ? regen : 1;
                } else {
                    hdr = sf < 2 ? 3 : sf == 2 ? 4 : 5;
                    if (hdr > size) return fail(kZsSection);
                    const uint32_t w = sf < 2 ? 10 : sf == 2 ? 14 : 18;
                    const uint64_t v = zs_le(zs + at, hdr) >> 4;
                    regen = (uint32_t)(v & ((1u << w) - 1)), comp = (uint32_t)(v >> w & ((1u << w) - 1));
                    streams = sf == 0 ? 1 : 4;
                }
                if (regen > kZsBlockMax || (uint64_t)hdr + comp > size) return fail(kZsSection);
                B.lit_type = (uint8_t)lt, B.lit_hdr = hdr, B.lit_regen = regen, B.lit_comp = comp, B.streams = (uint8_t)streams;
                P.census.lit_type[lt]++, P.census.lit_format[lt][sf]++;
                if (lt >= 2) P.census.streams[streams == 4]++;
                if (lt == 2) {
                    W.huf.src = at + hdr, W.huf.lim = at + hdr + comp, W.huf.def = self, W.have_huf = true;
                    if (comp == 0) return fail(kZsSection);
                    const uint32_t hb = zs[W.huf.src];
                    W.huf.len = hb < 128 ? 1 + hb : 1 + (hb - 127 + 1) / 2;
                    (hb >= 128 ? P.census.huf_direct : P.census.huf_fse)++;
                } else if (lt == 3) {
                    if (!W.have_huf) return fail(kZsNoRepeat);
                    B.def_block[0] = W.huf.def;
                }
                B.huf_src = W.huf.src, B.huf_lim = W.huf.lim;
                B.lit_off = P.lit_bytes, P.lit_bytes += regen;
                // ---- sequences-section header
                uint64_t s = at + hdr + comp;
                if (s >= end) return fail(kZsSection);
                const uint32_t c0 = zs[s];
                uint32_t n_seq, form;
                if (c0 == 0) n_seq = 0, s += 1, form = 0;
                else if (c0 < 128) n_seq = c0, s += 1, form = 1;
                else if (c0 < 255) {
                    if (end - s < 2) return fail(kZsSection);
                    n_seq = ((c0 - 128) << 8) + zs[s + 1], s += 2, form = 2;
                } else {
                    if (end - s < 3) return fail(kZsSection);
                    n_seq = (uint32_t)zs_le(zs + s + 1, 2) + 0x7F00, s += 3, form = 3;
                }
                P.census.seq_form[form]++;
                B.n_seq = n_seq, B.seq_off = P.n_seq, P.n_seq += n_seq;
                if (n_seq) {
                    if (s >= end) return fail(kZsSection);
                    const uint32_t modes = zs[s++];
                    if (modes & 3u) return fail(kZsSeqHeader);
                    for (uint32_t t = 0; t < 3; ++t) {
                        const uint32_t m = modes >> (6 - 2 * t) & 3u;
                        P.census.mode[t][m]++;
                        ZsTabRef &R = W.tab[t];
                        if (m == 3) {
                            if (!W.have_tabs) return fail(kZsNoRepeat);
                            B.def_block[1 + t] = R.def;
                            P.census.repeat_of[t][R.mode]++;
                            continue;
                        }
                        R.mode = (uint8_t)(m == 0 ? 0 : m == 1 ? 1 : 2), R.def = m == 0 ? ~0u : self, R.src = s, R.lim = end, R.len = 0;
                        if (m == 1) {
                            if (s >= end) return fail(kZsSection);
                            s += 1, R.len = 1;
                        } else if (m == 2) {
                            uint32_t log = 0;
                            const int used = zs_read_fse(in, s, end, zs_max_symbol(t), zs_max_log(t), no.norm, no, &log);
                            if (used < 0) return fail(used);
                            s += (uint32_t)used, R.len = (uint32_t)used;
                            if (s > end) return fail(kZsSection);
                        }
                    }
                    W.have_tabs = true;
                    for (uint32_t t = 0; t < 3; ++t) B.mode[t] = W.tab[t].mode, B.tab_src[t] = W.tab[t].src, B.tab_lim[t] = W.tab[t].lim;
                }
                B.bits_src = s;
            }
            P.census.block_type[type]++;
            if (size || type == 2) P.blocks.push_back(B);  // (an empty raw or RLE block makes nothing)
            at += content;
            ++taken;
            if (last) {
                F.n_blocks = (uint32_t)P.blocks.size() - F.first_block;
                if (F.n_blocks == 0 && !F.continued) P.census.empty_frames++;
                if (F.has_checksum) {  // (the 4 checksum bytes are consumed with the frame's last block)
                    if (n - at < 4) return fail(kZsTruncated);
                    F.checksum = (uint32_t)zs_le(zs + at, 4);
                    at += 4;
                }
                F.closed = true;
                P.frames.push_back(F);
                W.open = false;
            }
            full = (lim.bytes && at - from >= lim.bytes) || (lim.blocks && taken >= lim.blocks);
        }
    }
    if (W.open) {  // the frame goes on behind this walk: its blocks so far
        W.F.n_blocks = (uint32_t)P.blocks.size() - W.F.first_block, W.F.closed = false;
        P.frames.push_back(W.F);
    }
    return true;
}

// zs[0, n) -> P: the walk run once over the whole file with no limit; false: refused, P.status says why
inline bool zs_plan(const uint8_t *zs, uint64_t n, ZsPlan &P) {
    if (n < 4) return P.status = n ? kZsMagicBad : kZsTruncated, false;
    ZsWalk W;
    return zs_walk(zs, n, W, ZsLimit{}, P);
}

// the two scans over the blocks of every frame, once decoding has said what every block makes and does to the repeat offsets: where
// its text starts (the frames' texts lie back to back) and the three offsets in front of it, from the frame's (1, 4, 8).  A walk that
// starts inside a frame (ZsScanFrom: a window of a stream) has that frame's history in text[0, history), its blocks start behind it
// with frame_off = 0 -- exact for both checks of zs_execute: a frame shorter than its window has its first byte at position 0,
// otherwise history = window and `off <= window` binds -- and with the offsets the window before left; the frame's size so far is
// 64 bits and compared when the frame closes.  rep_out: the three offsets behind the last block.  false: a frame whose size
// disagrees with its header, or 4 GiB of text and more in this walk (P.status)
struct ZsScanFrom {
    uint64_t history = 0, frame_text = 0;  // bytes of the open frame in front of this walk: kept on the device / all of them
    uint32_t rep[3] = {1, 4, 8};
};
inline bool zs_scan(ZsPlan &P, const std::vector<ZsReport> &rep, std::vector<ZsStart> &start, uint64_t *total, const ZsScanFrom *from = nullptr,
                    uint32_t *rep_out = nullptr) {
    start.assign(P.blocks.size(), ZsStart{});
    uint64_t text = from ? from->history : 0;
    uint32_t a0 = 1, a1 = 4, a2 = 8;
    for (ZsFrame &F : P.frames) {
        const bool cont = from && F.continued;
        F.text_off = text;
        a0 = cont ? from->rep[0] : 1, a1 = cont ? from->rep[1] : 4, a2 = cont ? from->rep[2] : 8;
        for (uint32_t k = F.first_block; k < F.first_block + F.n_blocks; ++k) {
            start[k] = ZsStart{text, cont ? 0 : F.text_off, F.window, a0, a1, a2, 0};
            text += rep[k].regen;
            zs_rep_apply(rep[k].rep, a0, a1, a2);
        }
        F.text_len = text - F.text_off;
        if (F.closed && F.content_size != ~0ull && F.content_size != F.text_len + (cont ? from->frame_text : 0)) return P.status = kZsContentSize, false;
    }
    if (text >= (1ull << 32) - 1) return P.status = kZsTooLarge, false;
    if (rep_out) rep_out[0] = a0, rep_out[1] = a1, rep_out[2] = a2;
    *total = text;
    return true;
}

}  // namespace mkz
