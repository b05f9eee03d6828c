// zstd_serial.hpp -- one Zstandard block decoded and executed, written once for the host and the device: compiled with g++ it is what
// the host test harness runs (tests/helpers/zstd_harness.cpp, checked against libzstd), compiled with hipcc it is the body of the
// kernels of zstd_inflate.hip, and so the meaning they keep.
//
// Replaces, for .zst input of `extract`, the zstd reader the reference gets from needletail's `compression` feature
// (src/cmd_extract.rs:281).  The format is RFC 8878: a frame is a header and a chain of blocks of at most 128 KiB; a block is raw, one
// repeated byte, or compressed.  A compressed block is a literals section (raw, one byte, or Huffman-coded in one or four backward
// bitstreams under a tree that is described by 4-bit weights or by FSE-coded weights, or that is the previous block's) and a sequences
// section: a count, three table modes (predefined, one symbol, described, repeated), and one backward bitstream in which three FSE
// states -- literals length, offset, match length -- take turns.  Executing a sequence copies `literals length` literals, then `match
// length` bytes from `offset` back; offset values 1 to 3 name the three most recent offsets.
//
// What a block needs from the rest of its frame is exactly three things, and the walk on the host (zstd_plan.hpp) or a scan supplies
// each of them, so that every block can be decoded by a wave of its own:
//   * the tables it repeats: the walk names the bytes that describe them (in whichever earlier block), and the wave builds them again;
//   * the three repeat offsets at its start: zs_decode_block leaves the block's effect on them in symbolic form (ZsRep: every slot is
//     an explicit offset or "incoming slot j minus d"), which composes in order from the frame's (1, 4, 8);
//   * the text its matches reach into: zs_execute writes, per text byte, either the byte or -- where the source lies in front of the
//     block -- the text position it copies from (kZsResolved / a position), and zs_resolve_byte is one step of pointer doubling.
//
// What differs between the host and a wave is kept behind two small policies, so that the text below exists once:
//   * the source of the file's little-endian dwords (ZsHostWords here; a 64-dword window held across the lanes of a wave there),
//   * the output side (every store done by the one thread here; single stores by the leader lane, copies by the whole wave there).
// On the device ALL lanes of the wave run these functions with the same values, so the cross-lane steps inside the policies are legal
// everywhere in them.  Tables that are indexed by the stream live in ZsTables (LDS there): nothing here keeps an array in registers.
//
// Refused, never guessed at (the caller then leaves the file to libzstd, which also words the error): a Huffman description whose
// weights do not sum to a power of two, that needs more than 11 bits or names more than 256 symbols; an FSE description whose accuracy
// log is out of range or whose probabilities do not add up; a symbol above the format's last code; a bitstream whose last byte is
// zero, that is read past its first bit, or that does not end exactly there; more literals asked for than the block has; an offset of
// zero, one that reaches in front of the frame's first byte or beyond the window; a block that regenerates more than 128 KiB; a
// section that does not fit its block.
#pragma once
#include "deflate_common.hpp"

// (everything of a block is inlined into its kernel: a reader or a report handed on by reference would otherwise live in private memory)
#define MKZS_HD MKZ_HD __attribute__((always_inline))

namespace mkz {

constexpr uint32_t kZsMagic = 0xFD2FB528u, kZsSkipMagic = 0x184D2A50u;
constexpr uint32_t kZsBlockMax = 128u << 10, kZsHufLog = 11, kZsStreamPad = 128;  // (= kStreamPad of inflate_serial.hpp)
constexpr uint64_t kZsWindowMax = 1ull << 27;
constexpr uint32_t kZsMaxLL = 35, kZsMaxOF = 31, kZsMaxML = 52, kZsLogLL = 9, kZsLogOF = 8, kZsLogML = 9, kZsLogWeights = 6;
constexpr uint32_t kZsResolved = 0xffffffffu;  // a text byte's source: none, the byte is there

// status of a file, a frame or a block (0 = decoded)
constexpr int kZsTruncated = -1, kZsMagicBad = -2, kZsReservedBit = -3, kZsDictionary = -4, kZsWindow = -5, kZsBlockSize = -6, kZsBlockType = -7,
              kZsHufWeights = -8, kZsHufBits = -9, kZsFseLog = -10, kZsFseSum = -11, kZsFseSymbol = -12, kZsNoRepeat = -13, kZsStreamStart = -14,
              kZsStreamEnd = -15, kZsLiterals = -16, kZsOffset = -17, kZsRegenerated = -18, kZsContentSize = -19, kZsChecksum = -20,
              kZsTrailing = -21, kZsSection = -22, kZsRounds = -23, kZsTooLarge = -24, kZsSeqHeader = -25;

struct ZsFse {
    uint8_t sym, nbits;
    uint16_t base;
};
// a block's decoder memory (LDS on the device: 9.8 KB per wave)
struct ZsTables {
    uint16_t huf[1u << kZsHufLog];  // symbol | bits << 8, indexed by the next max_bits bits
    ZsFse ll[1u << kZsLogLL], of[1u << kZsLogOF], ml[1u << kZsLogML], wt[1u << kZsLogWeights];
    int16_t norm[64];   // the probabilities of the table being built
    uint16_t next[64];  // ... and every symbol's next state
    uint8_t weights[256];
    uint32_t rank[16];
};

// the block's effect on the three repeat offsets: slot i = v[i] (s[i] == 3) or incoming slot s[i] minus v[i]
struct ZsRep {
    uint32_t v0, v1, v2, s0, s1, s2;
};
// what the walk yields per block (zstd_plan.hpp fills it; the kernels read it)
struct ZsBlock {
    uint64_t src;                      // first byte of the block's content
    uint64_t huf_src, huf_lim;         // the tree description to build: this block's, or the one of the block it repeats
    uint64_t tab_src[3], tab_lim[3];   // LL / OF / ML: the table description or the one symbol, likewise
    uint64_t bits_src;                 // first byte of the sequences' bitstream
    uint64_t lit_off, seq_off;         // the block's slices of the literal buffer and of the sequence arrays
    uint32_t size;                     // Block_Size: bytes of content; of an RLE block, bytes of text
    uint32_t lit_regen, lit_comp, lit_hdr, n_seq, frame;
    uint32_t def_block[4];             // the block that defined Huffman / LL / OF / ML (~0: none, predefined or its own)
    uint8_t type, lit_type, streams, mode[3];  // mode: 0 predefined, 1 one symbol, 2 described (Repeat is resolved by the walk)
    uint8_t pad_[2];
};
// what decoding leaves per block, and what a frame's scans add for the execution
struct ZsReport {
    int32_t status;
    uint32_t regen;  // bytes of text
    ZsRep rep;
};
struct ZsStart {
    uint64_t text_off, frame_off, window;
    uint32_t r0, r1, r2, pad_;
};

struct ZsHostWords {
    const uint8_t *in;
    uint64_t n;  // bytes; zeros stand for what lies behind them (the device's copy carries kZsStreamPad of them)
    MKZS_HD uint32_t word(uint64_t i) const {
        uint32_t v = 0;
        for (uint32_t k = 0; k < 4; ++k)
            if (4 * i + k < n) v |= (uint32_t)in[4 * i + k] << (8 * k);
        return v;
    }
};

// bits of the file, bit 0 of a byte first
template <class Words>
struct ZsIn {
    Words w;
    uint64_t at = ~0ull, buf = 0;  // dwords at, at + 1
    MKZS_HD uint32_t bits(uint64_t bit, uint32_t k) {  // k <= 32
        const uint64_t i = bit >> 5;
        if (i != at) {
            buf = i + 1 == at ? buf << 32 | w.word(i) : (uint64_t)w.word(i) | (uint64_t)w.word(i + 1) << 32;
            at = i;
        }
        return (uint32_t)((buf >> (bit & 31u)) & ((1ull << k) - 1));
    }
    MKZS_HD uint32_t byte(uint64_t i) { return bits(i * 8, 8); }
};

// a bitstream read from its last byte down: the highest set bit of that byte is the end mark.  Bits asked for below the first one are zeros
struct ZsBack {
    uint64_t first_bit;
    int64_t left;  // bits not yet read (below 0: read past the start)
    template <class In>
    MKZS_HD bool open(In &in, uint64_t byte0, uint64_t n_bytes) {
        first_bit = byte0 * 8, left = 0;
        if (n_bytes == 0) return false;
        const uint32_t last = in.byte(byte0 + n_bytes - 1);
        if (last == 0) return false;
        left = (int64_t)(n_bytes - 1) * 8 + (31 - __builtin_clz(last));
        return true;
    }
    template <class In>
    MKZS_HD uint32_t peek(In &in, uint32_t k) const {
        if (left >= (int64_t)k) return in.bits(first_bit + (uint64_t)left - k, k);
        return left <= 0 ? 0u : in.bits(first_bit, (uint32_t)left) << (k - (uint32_t)left);
    }
    template <class In>
    MKZS_HD uint32_t read(In &in, uint32_t k) {
        const uint32_t v = peek(in, k);
        left -= k;
        return v;
    }
};

// ---- host policy -------------------------------------------------------------------------------------------------------------------
struct ZsSerialOut {
    const uint8_t *in;   // the file
    uint8_t *lit;        // the literal buffer
    uint32_t *ll, *ml, *of;
    uint8_t *text;
    uint32_t *src;
    uint64_t settled = 0;       // text below this position is final (a stream's carried history): a match reads it as bytes
    uint64_t settled_hits = 0;  // (the tests' census: bytes copied out of it)
    MKZS_HD bool leader() const { return true; }
    MKZS_HD uint32_t first() const { return 0; }
    MKZS_HD uint32_t step() const { return 1; }
    MKZS_HD void sync() const {}
    MKZS_HD uint32_t in_byte(uint64_t i) const { return in[i]; }
    MKZS_HD void lit_put(uint64_t i, uint32_t b) const { lit[i] = (uint8_t)b; }
    MKZS_HD void lit_copy(uint64_t i, uint64_t from, uint32_t n) const {
        for (uint32_t k = 0; k < n; ++k) lit[i + k] = in[from + k];
    }
    MKZS_HD void lit_fill(uint64_t i, uint32_t n, uint32_t b) const {
        for (uint32_t k = 0; k < n; ++k) lit[i + k] = (uint8_t)b;
    }
    MKZS_HD void seq_put(uint64_t i, uint32_t l, uint32_t m, uint32_t o) const { ll[i] = l, ml[i] = m, of[i] = o; }
    // execution
    MKZS_HD void text_lits(uint64_t to, uint64_t from, uint32_t n) {
        for (uint32_t k = 0; k < n; ++k) text[to + k] = lit[from + k], src[to + k] = kZsResolved;
    }
    MKZS_HD void text_in(uint64_t to, uint64_t from, uint32_t n) {
        for (uint32_t k = 0; k < n; ++k) text[to + k] = in[from + k], src[to + k] = kZsResolved;
    }
    MKZS_HD void text_fill(uint64_t to, uint32_t n, uint32_t b) {
        for (uint32_t k = 0; k < n; ++k) text[to + k] = (uint8_t)b, src[to + k] = kZsResolved;
    }
    // byte k of the match = byte k mod off of the off bytes in front of it.  A source in front of the block is left as a position --
    // unless it lies below `settled`, where the text is final: that byte is copied --; a source inside the block that is itself a
    // position hands that position on.  -> bytes left as positions
    MKZS_HD uint32_t text_match(uint64_t to, uint64_t off, uint32_t len, uint64_t block_pos) {
        uint32_t open = 0;
        for (uint32_t k = 0; k < len; ++k) {
            const uint64_t from = to - off + (off >= len ? k : k % off);
            if (from < settled) text[to + k] = text[from], src[to + k] = kZsResolved, ++settled_hits;
            else if (from < block_pos) src[to + k] = (uint32_t)from, ++open;
            else if (src[from] == kZsResolved) text[to + k] = text[from], src[to + k] = kZsResolved;
            else src[to + k] = src[from], ++open;
        }
        return open;
    }
};

// ---- the code tables of the sequences (RFC 8878 3.1.1.3.2.1.1) -------------------------------------------------------------------------
MKZS_HD uint32_t zs_ll_bits(uint32_t c) {
    static const uint8_t t[36] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    return t[c];
}
MKZS_HD uint32_t zs_ll_base(uint32_t c) {
    static const uint32_t t[36] = {0,  1,  2,  3,  4,  5,  6,  7,  8,  9,   10,  11,  12,   13,   14,   15,   16,    18,
                                   20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536};
    return t[c];
}
MKZS_HD uint32_t zs_ml_bits(uint32_t c) {
    static const uint8_t t[53] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0,
                                  0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16};
    return t[c];
}
MKZS_HD uint32_t zs_ml_base(uint32_t c) {
    static const uint32_t t[53] = {3,  4,  5,  6,  7,  8,  9,  10, 11, 12, 13, 14, 15, 16, 17, 18,  19,  20,  21,   22,   23,   24,   25,    26,    27,   28, 29,
                                   30, 31, 32, 33, 34, 35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195, 16387, 32771, 65539};
    return t[c];
}
// the predefined distributions (3.1.1.3.2.2), accuracy logs 6, 5, 6
MKZS_HD int zs_default_norm(uint32_t which, uint32_t s) {
    static const int8_t ll[36] = {4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1, -1, -1, -1, -1};
    static const int8_t of[29] = {1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1};
    static const int8_t ml[53] = {1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
                                  1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1};
    return which == 0 ? ll[s] : which == 1 ? of[s] : ml[s];
}
MKZS_HD uint32_t zs_max_symbol(uint32_t which) { return which == 0 ? kZsMaxLL : which == 1 ? kZsMaxOF : kZsMaxML; }
MKZS_HD uint32_t zs_max_log(uint32_t which) { return which == 0 ? kZsLogLL : which == 1 ? kZsLogOF : kZsLogML; }
MKZS_HD uint32_t zs_default_log(uint32_t which) { return which == 1 ? 5u : 6u; }
MKZS_HD uint32_t zs_default_symbols(uint32_t which) { return which == 0 ? 36u : which == 1 ? 29u : 53u; }

// ---- FSE (4.1) --------------------------------------------------------------------------------------------------------------------
// the table description at bytes [at, lim) -> norm[0 .. max_sym] (the leader's stores), *log; returns its bytes or a status
template <class In, class Out>
MKZS_HD int zs_read_fse(In &in, uint64_t at, uint64_t lim, uint32_t max_sym, uint32_t max_log, int16_t *norm, Out &out, uint32_t *log) {
    for (uint32_t i = out.first(); i <= max_sym; i += out.step()) norm[i] = 0;
    out.sync();
    uint64_t bit = at * 8;
    const uint64_t lim_bit = lim * 8;
    const uint32_t al = in.bits(bit, 4) + 5;
    bit += 4;
    *log = al;
    if (at >= lim) return kZsTruncated;
    if (al > max_log) return kZsFseLog;
    int32_t remaining = 1 << al;
    uint32_t sym = 0;
    while (remaining > 0 && sym <= max_sym) {
        const uint32_t max = (uint32_t)remaining + 1, nb = 32 - __builtin_clz(max), lower = (1u << nb) - 1 - max;
        const uint32_t v = in.bits(bit, nb), lo = v & ((1u << (nb - 1)) - 1);
        uint32_t val;
        if (lo < lower) val = lo, bit += nb - 1;
        else val = v >= (1u << (nb - 1)) ? v - lower : v, bit += nb;
        const int32_t prob = (int32_t)val - 1;
        remaining -= prob < 0 ? 1 : prob;
        if (out.leader()) norm[sym] = (int16_t)prob;
        ++sym;
        if (prob == 0) {
            for (;;) {
                const uint32_t r = in.bits(bit, 2);
                bit += 2;
                sym += r;  // (these stay 0)
                if (r != 3 || sym > max_sym + 1 || bit > lim_bit) break;
            }
        }
        if (bit > lim_bit) return kZsTruncated;
        if (sym > max_sym + 1) return kZsFseSymbol;
    }
    out.sync();
    if (remaining != 0) return kZsFseSum;
    return (int)((bit - at * 8 + 7) / 8);
}
// norm[0, n_sym) of accuracy log al -> the decoding table (the leader's work: the spread is a chain)
template <class Out>
MKZS_HD void zs_build_fse(ZsFse *tab, const int16_t *norm, uint16_t *next, uint32_t n_sym, uint32_t al, Out &out) {
    if (out.leader()) {
        const uint32_t size = 1u << al, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
        uint32_t high = size - 1;
        for (uint32_t s = 0; s < n_sym; ++s) {
            if (norm[s] == -1) tab[high--].sym = (uint8_t)s, next[s] = 1;
            else next[s] = (uint16_t)norm[s];
        }
        uint32_t pos = 0;
        for (uint32_t s = 0; s < n_sym; ++s)
            for (int32_t i = 0; i < norm[s]; ++i) {
                tab[pos].sym = (uint8_t)s;
                do pos = (pos + step) & mask;
                while (pos > high);
            }
        for (uint32_t u = 0; u < size; ++u) {
            const uint32_t x = next[tab[u].sym]++;
            const uint32_t nb = al - (31 - __builtin_clz(x));
            tab[u].nbits = (uint8_t)nb, tab[u].base = (uint16_t)((x << nb) - size);
        }
    }
    out.sync();
}
// table `which` (0 LL, 1 OF, 2 ML) of a block by its resolved mode -> *log; 0 or a status
template <class In, class Out>
MKZS_HD int zs_sequence_table(In &in, ZsTables &T, ZsFse *tab, uint32_t which, uint32_t mode, uint64_t at, uint64_t lim, Out &out, uint32_t *log) {
    if (mode == 1) {
        const uint32_t s = in.byte(at);
        if (at >= lim) return kZsTruncated;
        if (s > zs_max_symbol(which)) return kZsFseSymbol;
        if (out.leader()) tab[0] = ZsFse{(uint8_t)s, 0, 0};
        out.sync();
        *log = 0;
        return 0;
    }
    uint32_t n_sym = zs_max_symbol(which) + 1;
    if (mode == 0) {
        n_sym = zs_default_symbols(which);
        for (uint32_t i = out.first(); i < n_sym; i += out.step()) T.norm[i] = (int16_t)zs_default_norm(which, i);
        out.sync();
        *log = zs_default_log(which);
    } else {
        const int r = zs_read_fse(in, at, lim, zs_max_symbol(which), zs_max_log(which), T.norm, out, log);
        if (r < 0) return r;
    }
    zs_build_fse(tab, T.norm, T.next, n_sym, *log, out);
    return 0;
}

// ---- Huffman (4.2) -------------------------------------------------------------------------------------------------------------------
// the tree description at [at, lim) -> T.huf, *max_bits; returns its bytes or a status
template <class In, class Out>
MKZS_HD int zs_read_huffman(In &in, ZsTables &T, uint64_t at, uint64_t lim, Out &out, uint32_t *max_bits) {
    if (at >= lim) return kZsTruncated;
    const uint32_t hb = in.byte(at);
    uint32_t n = 0, bytes;
    if (hb >= 128) {  // 4-bit weights, the first in the high half of its byte
        n = hb - 127, bytes = 1 + (n + 1) / 2;
        if (at + bytes > lim) return kZsTruncated;
        for (uint32_t i = 0; i < n; ++i) {  // (the reader is the wave's: every lane asks it for the same byte)
            const uint32_t w = (in.byte(at + 1 + i / 2) >> (i & 1u ? 0 : 4)) & 15u;
            if (out.leader()) T.weights[i] = (uint8_t)w;
        }
        out.sync();
    } else {  // FSE-coded weights: two states take turns until the bitstream is read past its start
        bytes = 1 + hb;
        if (hb == 0 || at + bytes > lim) return kZsTruncated;
        uint32_t al = 0;
        const int used = zs_read_fse(in, at + 1, at + bytes, 11, kZsLogWeights, T.norm, out, &al);
        if (used < 0) return used;
        zs_build_fse(T.wt, T.norm, T.next, 12, al, out);
        ZsBack b;
        if (!b.open(in, at + 1 + (uint32_t)used, hb - (uint32_t)used)) return kZsStreamStart;
        uint32_t s1 = b.read(in, al), s2 = b.read(in, al), turn = 0;
        if (b.left < 0) return kZsStreamEnd;
        for (;;) {
            if (n >= 255) return kZsHufWeights;
            const ZsFse e = T.wt[turn ? s2 : s1];
            if (out.leader()) T.weights[n] = e.sym;
            ++n;
            const uint32_t nx = e.base + b.read(in, e.nbits);
            if (turn) s2 = nx;
            else s1 = nx;
            if (b.left < 0) {  // (the other state's symbol is the last one)
                if (n >= 255) return kZsHufWeights;
                if (out.leader()) T.weights[n] = T.wt[turn ? s1 : s2].sym;
                ++n;
                break;
            }
            turn ^= 1u;
        }
        out.sync();
    }
    // the last weight is what is missing to a power of two
    for (uint32_t i = out.first(); i < 16; i += out.step()) T.rank[i] = 0;
    out.sync();
    uint32_t sum = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t w = T.weights[i];
        if (w > kZsHufLog) return kZsHufBits;
        if (w) sum += 1u << (w - 1);
    }
    if (sum == 0) return kZsHufWeights;
    const uint32_t mb = 32 - __builtin_clz(sum), rest = (1u << mb) - sum;
    if (mb > kZsHufLog) return kZsHufBits;
    if (rest & (rest - 1)) return kZsHufWeights;
    if (out.leader()) {
        T.weights[n] = (uint8_t)(32 - __builtin_clz(rest));
        for (uint32_t i = 0; i <= n; ++i) T.rank[T.weights[i]]++;
        uint32_t pos = 0;  // rank[w]: where the symbols of weight w start
        for (uint32_t w = 1; w <= mb; ++w) {
            const uint32_t c = T.rank[w];
            T.rank[w] = pos, pos += c << (w - 1);
        }
        for (uint32_t s = 0; s <= n; ++s) {
            const uint32_t w = T.weights[s];
            if (!w) continue;
            const uint32_t len = 1u << (w - 1), p0 = T.rank[w];
            for (uint32_t j = 0; j < len; ++j) T.huf[p0 + j] = (uint16_t)(s | (mb + 1 - w) << 8);
            T.rank[w] = p0 + len;
        }
    }
    out.sync();
    *max_bits = mb;
    return (int)bytes;
}

// ---- the repeat offsets (3.1.1.5) ------------------------------------------------------------------------------------------------------
// one sequence's offset value and literals length applied to the three slots (symbolic or, every s == 3, plain numbers): the offset
// it uses is slot 0 afterwards
MKZS_HD void zs_rep_step(ZsRep &r, uint32_t ofv, uint32_t ll) {
    if (ofv > 3) {
        r.v2 = r.v1, r.s2 = r.s1, r.v1 = r.v0, r.s1 = r.s0, r.v0 = ofv - 3, r.s0 = 3;
        return;
    }
    const uint32_t idx = ofv - 1 + (ll == 0 ? 1u : 0u);
    if (idx == 0) return;
    if (idx == 1) {
        const uint32_t v = r.v1, s = r.s1;
        r.v1 = r.v0, r.s1 = r.s0, r.v0 = v, r.s0 = s;
        return;
    }
    // slot 2, or slot 0 minus one byte, comes to the front
    const uint32_t v = idx == 2 ? r.v2 : (r.s0 == 3 ? r.v0 - 1 : r.v0 + 1), s = idx == 2 ? r.s2 : r.s0;
    r.v2 = r.v1, r.s2 = r.s1, r.v1 = r.v0, r.s1 = r.s0, r.v0 = v, r.s0 = s;
}
MKZS_HD uint32_t zs_rep_pick(uint32_t v, uint32_t s, uint32_t a0, uint32_t a1, uint32_t a2) { return s == 3 ? v : (s == 0 ? a0 : s == 1 ? a1 : a2) - v; }
// the offsets behind a block whose map is m, given the ones in front of it
MKZS_HD void zs_rep_apply(const ZsRep &m, uint32_t &a0, uint32_t &a1, uint32_t &a2) {
    const uint32_t n0 = zs_rep_pick(m.v0, m.s0, a0, a1, a2), n1 = zs_rep_pick(m.v1, m.s1, a0, a1, a2), n2 = zs_rep_pick(m.v2, m.s2, a0, a1, a2);
    a0 = n0, a1 = n1, a2 = n2;
}

// ---- a block's entropy decoding ----------------------------------------------------------------------------------------------------------
// Block B of a file of n bytes: literals to the block's slice of the literal buffer, sequences to its slices of the three arrays, and
// R: bytes of text, the map of the repeat offsets.  Raw and RLE blocks have neither and are the identity.
template <class In, class Out>
MKZS_HD int zs_decode_block(In &in, uint64_t n, const ZsBlock &B, ZsTables &T, Out &out, ZsReport &R) {
    R.regen = 0, R.rep = ZsRep{0, 0, 0, 0, 1, 2};
    if (B.type != 2) {
        if (B.src + (B.type == 0 ? B.size : 1u) > n || B.size > kZsBlockMax) return R.status = kZsTruncated;
        R.regen = B.size;
        return R.status = 0;
    }
    const uint64_t end = B.src + B.size;
    if (end > n || B.lit_regen > kZsBlockMax) return R.status = kZsTruncated;
    // ---- literals
    uint64_t at = B.src + B.lit_hdr;
    if (B.lit_type == 0) {
        if (at + B.lit_regen > end) return R.status = kZsSection;
        out.lit_copy(B.lit_off, at, B.lit_regen);
        at += B.lit_regen;
    } else if (B.lit_type == 1) {
        if (at + 1 > end) return R.status = kZsSection;
        out.lit_fill(B.lit_off, B.lit_regen, in.byte(at));
        at += 1;
    } else {
        if (at + B.lit_comp > end) return R.status = kZsSection;
        uint32_t mb = 0;
        const int used = zs_read_huffman(in, T, B.huf_src, B.huf_lim, out, &mb);
        if (used < 0) return R.status = used;
        uint64_t s_at = at + (B.lit_type == 2 ? (uint32_t)used : 0u);
        const uint64_t s_end = at + B.lit_comp;
        if (s_at > s_end) return R.status = kZsSection;
        uint32_t l0 = (uint32_t)(s_end - s_at), l1 = 0, l2 = 0, l3 = 0, q = B.lit_regen;  // the streams' bytes; what each but the last makes
        if (B.streams == 4) {
            if (s_at + 6 > s_end) return R.status = kZsSection;
            l0 = in.bits(s_at * 8, 16), l1 = in.bits(s_at * 8 + 16, 16), l2 = in.bits(s_at * 8 + 32, 16);
            s_at += 6;
            if ((uint64_t)l0 + l1 + l2 > s_end - s_at) return R.status = kZsSection;
            l3 = (uint32_t)(s_end - s_at) - l0 - l1 - l2;
            q = (B.lit_regen + 3) / 4;
            if (3 * q > B.lit_regen) return R.status = kZsSection;
        }
        uint64_t o = B.lit_off;
        for (uint32_t k = 0; k < B.streams; ++k) {
            const uint32_t len = k == 0 ? l0 : k == 1 ? l1 : k == 2 ? l2 : l3, cnt = k + 1 < B.streams ? q : B.lit_regen - k * q;
            ZsBack b;
            if (!b.open(in, s_at, len)) return R.status = kZsStreamStart;
            for (uint32_t j = 0; j < cnt; ++j) {
                const uint32_t e = T.huf[b.peek(in, mb)];
                b.left -= e >> 8;
                out.lit_put(o + j, e & 255u);
            }
            if (b.left != 0) return R.status = kZsStreamEnd;
            s_at += len, o += cnt;
        }
        at = s_end;
    }
    // ---- sequences
    uint32_t lits = 0, regen = B.lit_regen;
    if (B.n_seq) {
        uint32_t log_ll = 0, log_of = 0, log_ml = 0;
        int r = zs_sequence_table(in, T, T.ll, 0, B.mode[0], B.tab_src[0], B.tab_lim[0], out, &log_ll);
        if (r == 0) r = zs_sequence_table(in, T, T.of, 1, B.mode[1], B.tab_src[1], B.tab_lim[1], out, &log_of);
        if (r == 0) r = zs_sequence_table(in, T, T.ml, 2, B.mode[2], B.tab_src[2], B.tab_lim[2], out, &log_ml);
        if (r) return R.status = r;
        if (B.bits_src < at || B.bits_src > end) return R.status = kZsSection;
        ZsBack b;
        if (!b.open(in, B.bits_src, end - B.bits_src)) return R.status = kZsStreamStart;
        uint32_t sl = b.read(in, log_ll), so = b.read(in, log_of), sm = b.read(in, log_ml);
        for (uint32_t i = 0; i < B.n_seq; ++i) {
            const ZsFse el = T.ll[sl], eo = T.of[so], em = T.ml[sm];
            if (el.sym > kZsMaxLL || eo.sym > kZsMaxOF || em.sym > kZsMaxML) return R.status = kZsFseSymbol;
            const uint32_t ofv = (1u << eo.sym) + b.read(in, eo.sym);
            const uint32_t ml = zs_ml_base(em.sym) + b.read(in, zs_ml_bits(em.sym));
            const uint32_t ll = zs_ll_base(el.sym) + b.read(in, zs_ll_bits(el.sym));
            if (i + 1 < B.n_seq) {
                sl = el.base + b.read(in, el.nbits);
                sm = em.base + b.read(in, em.nbits);
                so = eo.base + b.read(in, eo.nbits);
            }
            if (b.left < 0) return R.status = kZsStreamEnd;
            if (ll > B.lit_regen - lits) return R.status = kZsLiterals;
            if (ml > kZsBlockMax - regen) return R.status = kZsRegenerated;
            lits += ll, regen += ml;
            out.seq_put(B.seq_off + i, ll, ml, ofv);
            zs_rep_step(R.rep, ofv, ll);
        }
        if (b.left != 0) return R.status = kZsStreamEnd;
    } else if (B.bits_src != end) {
        return R.status = kZsSection;
    }
    if (regen > kZsBlockMax) return R.status = kZsRegenerated;
    R.regen = regen;
    return R.status = 0;
}

// ---- a block's execution ---------------------------------------------------------------------------------------------------------------
// Block B, whose text starts at S.text_off with the repeat offsets S.r0 .. r2, written: bytes, and positions where a match reaches in
// front of the block.  *open: how many bytes are left as positions.  regen: what decoding said the block makes.
template <class Out>
MKZS_HD int zs_execute(const ZsBlock &B, const ZsStart &S, uint32_t regen, const uint32_t *seq_ll, const uint32_t *seq_ml, const uint32_t *seq_of, Out &out,
                      uint32_t *open) {
    *open = 0;
    if (B.type == 0) {
        out.text_in(S.text_off, B.src, B.size);
        return 0;
    }
    if (B.type == 1) {
        out.text_fill(S.text_off, B.size, out.in_byte(B.src));
        return 0;
    }
    ZsRep r{S.r0, S.r1, S.r2, 3, 3, 3};
    uint64_t to = S.text_off, lit = B.lit_off;
    const uint64_t text_end = S.text_off + regen, lit_end = B.lit_off + B.lit_regen;
    uint32_t left_open = 0;
    for (uint32_t i = 0; i < B.n_seq; ++i) {
        const uint32_t ll = seq_ll[B.seq_off + i], ml = seq_ml[B.seq_off + i], ofv = seq_of[B.seq_off + i];
        zs_rep_step(r, ofv, ll);
        const uint64_t off = r.v0;
        if (ll > lit_end - lit || (uint64_t)ll + ml > text_end - to) return kZsRegenerated;  // (decoding has summed them: cannot happen)
        out.text_lits(to, lit, ll);
        to += ll, lit += ll;
        if (off == 0 || off > to - S.frame_off || off > S.window) return kZsOffset;
        left_open += out.text_match(to, off, ml, S.text_off);
        to += ml;
    }
    if (lit_end - lit != text_end - to) return kZsRegenerated;
    out.text_lits(to, lit, (uint32_t)(lit_end - lit));
    *open = left_open;
    return 0;
}

// ---- cross-block resolution: one step of pointer doubling for text byte i, from the sources `a` of the round before to `b` --------------
// Every source lies in an earlier block -- of the same launch: what lies below a stream's settled history never becomes a position --,
// so a chain is at most as long as the launch has blocks.  -> 1: the byte is still a position
MKZS_HD uint32_t zs_resolve_byte(uint64_t i, const uint32_t *a, uint32_t *b, uint8_t *text) {
    const uint32_t s = a[i];
    if (s == kZsResolved) {
        b[i] = kZsResolved;
        return 0;
    }
    const uint32_t ss = a[s];
    if (ss == kZsResolved) {
        text[i] = text[s], b[i] = kZsResolved;
        return 0;
    }
    b[i] = ss;
    return 1;
}
MKZS_HD uint32_t zs_round_cap(uint64_t n_blocks) {
    uint32_t lg = 0;
    while ((1ull << lg) < n_blocks) ++lg;
    return lg + 2;
}

}  // namespace mkz
