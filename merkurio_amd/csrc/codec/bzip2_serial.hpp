// bzip2_serial.hpp -- one bzip2 block decoded from a known bit offset, written once for the host and the device: compiled with g++
// it is what the host test harness runs (tests/helpers/bzip2_harness.cpp, checked against Python's bz2), compiled with hipcc it is
// the body of the kernels of bzip2_inflate.hip, and so the meaning they keep.
//
// Replaces, for .bz2 input of `extract`, the bzip2 reader the reference gets from needletail's `compression` feature
// (src/cmd_extract.rs:281).  The format is defined by its reference implementation (bzip2 1.0.8, decompress.c / huffman.c): a stream
// is "BZh" + level, then blocks that each start with the 48-bit magic 0x314159265359 at ANY bit offset, then the end magic
// 0x177245385090 and the stream's CRC.  A block: CRC-32 of its text, the `randomised` bit, origPtr (24 bits), the map of bytes in use
// (16 + 16 x 16 bits), nGroups (3 bits), nSelectors (15), the selectors (unary, move-to-front coded), the code lengths of every group
// (5-bit start, then +1 / -1 steps), then the symbols in groups of 50, each group under the code its selector names: RUNA / RUNB
// zero runs, move-to-front indices, end of block.  What comes out is the last column of a Burrows-Wheeler matrix; the inverse
// transform is a counting sort and a walk of nblock dependent steps; the walk's bytes are run-length coded once more (four equal
// bytes are followed by a count of further copies).
//
// What differs between the host and a wave is kept behind three small policies, so that the text below exists once:
//   * the bit reader's source of big-endian dwords (BzHostWords here; a 64-dword window held across the lanes of a wave there),
//   * the move-to-front list (an array here; 256 entries across the lanes there),
//   * the output side (every store done by the one thread here; by the leader lane, runs by the whole wave there).
// On the device ALL lanes of the wave run bz2_decode_block with the same values (the reader's state is wave-uniform), so the
// cross-lane steps inside the policies are legal everywhere in it.
//
// Refused, never guessed at (the caller then leaves the file to libbz2, which also words the error): `randomised` blocks (bzip2 has
// not written one since 0.9.5), origPtr >= nblock, nGroups outside 2..6, nSelectors 0 or above 18 002, a selector >= nGroups, a code
// length outside 1..20, more symbols than level x 100 000, a run of 2 Mi or more, running off the data's end, and a code under which
// a symbol does not decode.  That last one is how libbz2 judges an over- or under-subscribed code: it never counts codewords, it
// builds limit / base / perm from whatever lengths it is given and refuses when a codeword grows past 20 bits or indexes outside
// perm.  The tables here are built by the same rule, so the verdict on every stream is libbz2's.
#pragma once
#include "deflate_common.hpp"

namespace mkz {

constexpr uint64_t kBzBlockMagic = 0x314159265359ull, kBzEndMagic = 0x177245385090ull;
constexpr uint32_t kBzMaxSelectors = 18002, kBzMaxAlpha = 258, kBzMaxCodeLen = 20, kBzGroupSize = 50, kBzMaxGroups = 6;
constexpr uint32_t kBzSelBytes = 18048;   // a block's selectors in memory (a multiple of 64)
constexpr uint32_t kBzStreamPad = 128;    // readable bytes the data needs behind its last one (= kStreamPad of inflate_serial.hpp)

// status of a block (0 = decoded)
constexpr int kBzTruncated = -1, kBzRandomised = -2, kBzOrigPtr = -3, kBzGroups = -4, kBzSelectors = -5, kBzCodeLength = -6, kBzCode = -7,
              kBzSelector = -8, kBzTooManySymbols = -9, kBzNoBytesInUse = -10, kBzRunTooLong = -11, kBzRunCut = -12, kBzNotABlock = -13;

// a block's decoder memory (LDS on the device: 7.1 KB per wave)
struct Bz2Tables {
    int32_t limit[kBzMaxGroups][24], base[kBzMaxGroups][24];  // (libbz2 indexes up to length + 2)
    uint16_t perm[kBzMaxGroups][kBzMaxAlpha];
    uint8_t len[kBzMaxGroups][kBzMaxAlpha + 2];
    uint8_t min_len[8];
    uint8_t seq_to_unseq[256];
    uint32_t hist[256];  // bytes of the block's last column; bz2_prefix turns it into where every byte's rows start
};

// what a decoded block reports
struct Bz2Block {
    uint64_t end_bit;  // the bit behind the block's end-of-block symbol: where the next magic must stand
    uint32_t crc, orig_ptr, nblock;
    int32_t status;
};

struct BzHostWords {
    const uint8_t *in;
    uint64_t n_words;  // readable dwords (data + pad); zeros stand for what lies behind them
    MKZ_HD uint32_t word(uint64_t i) const {
        if (i >= n_words) return 0;
        const uint8_t *p = in + 4 * i;
        return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3];
    }
};

// bits of the stream, first bit of a byte = its top one.  `taken` may pass n_bits by less than 64 before a caller looks (over()):
// the words then read lie inside the pad.
template <class Words>
struct BzBits {
    Words w;
    uint64_t n_bits = 0, taken = 0, next_word = 0, buf = 0;
    uint32_t cnt = 0;  // valid bits at the low end of buf
    MKZ_HD void seek(uint64_t bit) {
        next_word = bit >> 5, buf = 0, cnt = 0, taken = bit & ~31ull;
        need32();
        take((uint32_t)bit & 31u);
    }
    MKZ_HD void need32() {
        if (cnt < 32) buf = buf << 32 | w.word(next_word++), cnt += 32;
    }
    MKZ_HD uint32_t peek(uint32_t k) const { return (uint32_t)((buf >> (cnt - k)) & ((1ull << k) - 1)); }  // k <= 32 <= cnt
    MKZ_HD void take(uint32_t k) { cnt -= k, taken += k; }
    MKZ_HD uint32_t get(uint32_t k) {
        need32();
        const uint32_t v = peek(k);
        take(k);
        return v;
    }
    MKZ_HD bool over() const { return taken > n_bits; }
};

// ---- host policies ---------------------------------------------------------------------------------------------------------------
struct BzSerialMtf {
    uint8_t list[256];
    MKZ_HD void init() {
        for (int i = 0; i < 256; ++i) list[i] = (uint8_t)i;
    }
    MKZ_HD uint32_t front() const { return list[0]; }
    MKZ_HD uint32_t take(uint32_t nn) {  // the entry at nn moves to the front
        const uint8_t v = list[nn];
        for (uint32_t i = nn; i > 0; --i) list[i] = list[i - 1];
        list[0] = v;
        return v;
    }
};
struct BzSerialOut {
    uint8_t *ll8;
    MKZ_HD bool leader() const { return true; }
    MKZ_HD uint32_t first() const { return 0; }  // this thread's share of a loop over independent items: first, first + step, ...
    MKZ_HD uint32_t step() const { return 1; }
    MKZ_HD void sync() const {}
    MKZ_HD void put(uint32_t i, uint32_t uc) const { ll8[i] = (uint8_t)uc; }
    MKZ_HD void fill(uint32_t i, uint32_t n, uint32_t uc) const {
        for (uint32_t k = 0; k < n; ++k) ll8[i + k] = (uint8_t)uc;
    }
};

// limit / base / perm of group t as BZ2_hbCreateDecodeTables builds them (huffman.c), lengths 1..20 each
MKZ_HD void bz2_build_tables(Bz2Tables &T, uint32_t t, uint32_t alpha) {
    uint32_t min_len = 32, max_len = 0;
    for (uint32_t i = 0; i < alpha; ++i) {
        const uint32_t l = T.len[t][i];
        max_len = l > max_len ? l : max_len, min_len = l < min_len ? l : min_len;
    }
    uint32_t pp = 0;
    for (uint32_t l = min_len; l <= max_len; ++l)
        for (uint32_t j = 0; j < alpha; ++j)
            if (T.len[t][j] == l) T.perm[t][pp++] = (uint16_t)j;
    for (; pp < kBzMaxAlpha; ++pp) T.perm[t][pp] = 0xffff;  // (libbz2 leaves what an earlier block put there; no symbol here)
    int32_t *base = T.base[t], *limit = T.limit[t];
    for (int i = 0; i < 24; ++i) base[i] = 0, limit[i] = 0;
    for (uint32_t i = 0; i < alpha; ++i) base[T.len[t][i] + 1]++;
    for (int i = 1; i < 23; ++i) base[i] += base[i - 1];
    int32_t vec = 0;
    for (uint32_t l = min_len; l <= max_len; ++l) {
        vec += base[l + 1] - base[l];
        limit[l] = vec - 1;
        vec <<= 1;
    }
    for (uint32_t l = min_len + 1; l <= max_len; ++l) base[l] = ((limit[l - 1] + 1) << 1) - base[l];
    T.min_len[t] = (uint8_t)min_len;
}

// The block whose magic stands at the reader's position -> its last column in out (at most level x 100 000 bytes), the histogram of
// those bytes in T.hist, and h.  sel: kBzSelBytes of the block's own memory.
template <class Bits, class Mtf, class Out>
MKZ_HD int bz2_decode_block(Bits &b, uint32_t level, Bz2Tables &T, uint8_t *sel, Mtf &mtf, Out &out, Bz2Block &h) {
    h.end_bit = 0, h.crc = 0, h.orig_ptr = 0, h.nblock = 0;
    {
        const uint64_t hi = b.get(24), lo = b.get(24);
        if ((hi << 24 | lo) != kBzBlockMagic || b.over()) return h.status = b.over() ? kBzTruncated : kBzNotABlock;
    }
    h.crc = b.get(32);
    if (b.get(1)) return h.status = kBzRandomised;
    h.orig_ptr = b.get(24);
    // the bytes in use
    uint32_t n_in_use = 0;
    {
        const uint32_t in_use16 = b.get(16);
        for (uint32_t i = 0; i < 16; ++i) {
            if (!(in_use16 >> (15 - i) & 1u)) continue;
            const uint32_t m = b.get(16);
            for (uint32_t j = 0; j < 16; ++j)
                if (m >> (15 - j) & 1u) {
                    if (out.leader()) T.seq_to_unseq[n_in_use] = (uint8_t)(i * 16 + j);
                    ++n_in_use;
                }
        }
    }
    if (b.over()) return h.status = kBzTruncated;
    if (n_in_use == 0) return h.status = kBzNoBytesInUse;
    const uint32_t alpha = n_in_use + 2;
    const uint32_t n_groups = b.get(3);
    if (n_groups < 2 || n_groups > kBzMaxGroups) return h.status = kBzGroups;
    const uint32_t n_sel = b.get(15);
    if (n_sel < 1 || n_sel > kBzMaxSelectors) return h.status = kBzSelectors;
    {
        uint32_t pos = 0x543210u;  // the move-to-front list of the groups, 4 bits each
        for (uint32_t i = 0; i < n_sel; ++i) {
            uint32_t j = 0;
            while (b.get(1)) {
                if (++j >= n_groups) return h.status = kBzSelector;
            }
            if (b.over()) return h.status = kBzTruncated;
            const uint32_t v = pos >> (4 * j) & 15u, low = (1u << (4 * j)) - 1;
            pos = (pos & ~((low << 4) | 15u)) | ((pos & low) << 4) | v;
            if (out.leader()) sel[i] = (uint8_t)v;
        }
    }
    for (uint32_t t = 0; t < n_groups; ++t) {
        uint32_t curr = b.get(5);
        for (uint32_t i = 0; i < alpha; ++i) {
            for (;;) {
                if (curr < 1 || curr > kBzMaxCodeLen) return h.status = kBzCodeLength;
                if (!b.get(1)) break;
                curr += b.get(1) ? -1 : 1;
                if (b.over()) return h.status = kBzTruncated;
            }
            if (out.leader()) T.len[t][i] = (uint8_t)curr;
        }
    }
    if (b.over()) return h.status = kBzTruncated;
    out.sync();
    for (uint32_t t = out.first(); t < n_groups; t += out.step()) bz2_build_tables(T, t, alpha);
    for (uint32_t i = out.first(); i < 256; i += out.step()) T.hist[i] = 0;
    mtf.init();
    out.sync();
    // the symbols
    const uint32_t eob = n_in_use + 1, cap = level * 100000u;
    uint32_t nblock = 0, group = 0, left = 0, g = 0;
    int status = 1;
    uint32_t run = 0, run_bit = 1;  // the zero run being read: its length so far, the weight of the next RUNA (x 1) / RUNB (x 2)
    while (status == 1) {
        if (left == 0) {
            if (group >= n_sel) {
                status = kBzSelector;
                break;
            }
            g = sel[group++], left = kBzGroupSize;
        }
        --left;
        b.need32();
        const uint32_t top = b.peek(kBzMaxCodeLen);
        uint32_t zn = T.min_len[g];
        while (zn <= kBzMaxCodeLen && (int32_t)(top >> (kBzMaxCodeLen - zn)) > T.limit[g][zn]) ++zn;
        if (zn > kBzMaxCodeLen) {
            status = kBzCode;
            break;
        }
        b.take(zn);
        const int32_t at = (int32_t)(top >> (kBzMaxCodeLen - zn)) - T.base[g][zn];
        if (at < 0 || at >= (int32_t)kBzMaxAlpha) {
            status = kBzCode;
            break;
        }
        if (b.over()) {
            status = kBzTruncated;
            break;
        }
        const uint32_t sym = T.perm[g][at];
        if (sym > eob) {
            status = kBzCode;
            break;
        }
        if (sym <= 1) {  // RUNA / RUNB: the run's length in bijective base 2
            if (run_bit >= 2u * 1024 * 1024) status = kBzRunTooLong;
            run += run_bit << sym, run_bit <<= 1;
            continue;
        }
        if (run) {
            const uint32_t uc = T.seq_to_unseq[mtf.front()];
            if (run > cap - nblock) {
                status = kBzTooManySymbols;
                break;
            }
            if (out.leader()) T.hist[uc] += run;
            out.fill(nblock, run, uc);
            nblock += run, run = 0, run_bit = 1;
        }
        if (sym == eob) {
            status = 0;
            break;
        }
        if (nblock >= cap) {
            status = kBzTooManySymbols;
            break;
        }
        const uint32_t uc = T.seq_to_unseq[mtf.take(sym - 1)];
        if (out.leader()) T.hist[uc] += 1;
        out.put(nblock++, uc);
    }
    h.nblock = nblock, h.end_bit = b.taken;
    if (status == 0 && h.orig_ptr >= nblock) status = kBzOrigPtr;
    out.sync();
    return h.status = status;
}

// ---- the inverse Burrows-Wheeler transform ------------------------------------------------------------------------------------------
// Row j of the sorted matrix starts with byte F[j] and is followed, in the text, by row T[j] = the place in the last column of the j-th
// byte in stable order.  One entry per row: T[j] << 8 | F[j].  The text is F[p], p = origPtr, T[origPtr], T[T[origPtr]] ...
// (libbz2 keeps the last column's byte in the low 8 bits instead and starts one step further; the walk visits the same bytes.)

// hist (counts) -> where every byte's rows start
MKZ_HD void bz2_prefix(uint32_t *hist) {
    uint32_t at = 0;
    for (int i = 0; i < 256; ++i) {
        const uint32_t c = hist[i];
        hist[i] = at, at += c;
    }
}
MKZ_HD void bz2_scatter_serial(const uint8_t *ll8, uint32_t nblock, uint32_t *start, uint32_t *tt) {
    for (uint32_t i = 0; i < nblock; ++i) tt[start[ll8[i]]++] = i << 8 | ll8[i];
}

// The walk: the nblock bytes in front of the last run-length step -> pre[0, nblock); bit i of is_count = byte i is a count (it
// follows four equal bytes) and stands for that many further copies of the byte in front of it; *text_len = the block's text.
// One thread: every step waits for the load of the step before it.  is_count: (nblock + 31) / 32 words.
MKZ_HD int bz2_walk(const uint32_t *tt, uint32_t nblock, uint32_t orig_ptr, uint8_t *pre, uint32_t *is_count, uint64_t *text_len) {
    uint32_t p = orig_ptr, last = 256, run = 0, bits = 0;
    uint64_t len = 0;
    for (uint32_t i = 0; i < nblock; ++i) {
        const uint32_t e = tt[p];
        const uint32_t ch = e & 0xffu;
        p = e >> 8;
        pre[i] = (uint8_t)ch;
        if (run == 4) {
            bits |= 1u << (i & 31u), len += ch, run = 0, last = 256;
        } else if (ch == last) {
            ++run, ++len;
        } else {
            last = ch, run = 1, ++len;
        }
        if ((i & 31u) == 31u) is_count[i >> 5] = bits, bits = 0;
    }
    if (nblock & 31u) is_count[nblock >> 5] = bits;
    *text_len = len;
    return run == 4 ? kBzRunCut : 0;  // (four equal bytes and no count: libbz2 reads past the block and calls it a data error)
}
MKZ_HD void bz2_expand_serial(const uint8_t *pre, const uint32_t *is_count, uint32_t nblock, uint8_t *text) {
    for (uint32_t i = 0; i < nblock; ++i) {
        if (is_count[i >> 5] >> (i & 31u) & 1u) {
            for (uint32_t k = 0; k < pre[i]; ++k) *text++ = pre[i - 1];
        } else {
            *text++ = pre[i];
        }
    }
}

// ---- bzip2's CRC-32: polynomial 0x04c11db7, first bit on top, register and result inverted -------------------------------------------
// In pieces as the gzip one is (deflate_common.hpp): state(B, r) = state(B, 0) ^ r * x^(8|B|) mod P.
constexpr uint32_t kBzCrcPoly = 0x04c11db7u;
MKZ_HD uint32_t bz2_crc_table_entry(uint32_t i) {
    uint32_t c = i << 24;
    for (int k = 0; k < 8; ++k) c = (c & 0x80000000u) ? (c << 1) ^ kBzCrcPoly : c << 1;
    return c;
}
MKZ_HD uint32_t bz2_crc_byte(uint32_t c, uint32_t byte, const uint32_t *table) { return (c << 8) ^ table[(c >> 24) ^ byte]; }
// a * b mod P (x^k = bit k)
MKZ_HD uint32_t bz2_crc_mulmod(uint32_t a, uint32_t b) {
    uint32_t r = 0;
    for (int i = 31; i >= 0; --i) {
        r = (r & 0x80000000u) ? (r << 1) ^ kBzCrcPoly : r << 1;
        if (b >> i & 1u) r ^= a;
    }
    return r;
}
// x^(8 n) mod P
MKZ_HD uint32_t bz2_crc_x_pow_bytes(uint64_t n) {
    uint32_t r = 1u, sq = 0x100u;
    for (; n; n >>= 1) {
        if (n & 1) r = bz2_crc_mulmod(r, sq);
        sq = bz2_crc_mulmod(sq, sq);
    }
    return r;
}
MKZ_HD uint32_t bz2_stream_crc_fold(uint32_t stream_crc, uint32_t block_crc) { return (stream_crc << 1 | stream_crc >> 31) ^ block_crc; }

}  // namespace mkz
