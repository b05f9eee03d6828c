// zstd_enc_serial.hpp -- the pieces of a Zstandard block WRITER that have a serial definition, written once for the host and the device
// (the __HIPCC__ seam of deflate_common.hpp): compiled with g++ they are what tests/helpers/zstd_enc_harness.cpp drives behind a naive
// parser and checks with zstd_serial.hpp and libzstd; compiled with hipcc one lane of a wave runs them between the parallel phases of
// zstd_deflate.hip (histograms, code lookup, bit packing live there).
//
// The format is RFC 8878, read from the decoder's side in zstd_serial.hpp.  The fixed choices of this writer (include/merkurio_hip.h,
// mk_zstd_deflate_records): one block per frame; offsets always coded as offset + 3, never a repeat-offset code; Huffman trees described
// by direct 4-bit weights only (symbols 0 .. 128, code lengths limited to 11), so literals with a byte above 128 stay raw; per sequence
// table RLE where one code occurs, else the cheaper of Predefined and FSE_Compressed by an estimate from the histogram; the writer's own
// normalised counts never use the "less than one" probability (-1), so their symbol spread has no serial dependence.
//
// Both kinds of bit stream (Huffman literals, FSE sequences) are WRITTEN forward, lowest bit first, and closed with a single set bit:
// the decoder starts at that bit and reads downward, so what it needs first is written last.
#pragma once
#include "zstd_serial.hpp"

namespace mkz {

constexpr uint32_t kZeHufMaxSym = 128;  // direct weights: 127 + (number of weights) is the header byte, the last symbol's weight is implied
constexpr uint32_t kZeDescMax = 96;     // bytes an FSE table description takes at most here (<= 53 symbols of <= 10 bits, zero runs of 2 bits)

// ---- literal length / match length / offset -> code (the extra bits are value - base of the code, zs_*_base / zs_*_bits) --------------
MKZS_HD uint32_t ze_ll_code(uint32_t ll) {
    if (ll < 16) return ll;
    if (ll >= 64) return (uint32_t)floor_log2(ll) + 19;
    uint32_t c = 16;
    while (zs_ll_base(c + 1) <= ll) ++c;
    return c;
}
MKZS_HD uint32_t ze_ml_code(uint32_t ml) {  // ml >= 3
    if (ml < 35) return ml - 3;
    if (ml >= 131) return (uint32_t)floor_log2(ml - 3) + 36;
    uint32_t c = 32;
    while (zs_ml_base(c + 1) <= ml) ++c;
    return c;
}
MKZS_HD uint32_t ze_of_code(uint32_t offset) { return (uint32_t)floor_log2(offset + 3); }  // extra bits: offset + 3 - (1 << code), `code` of them

// ---- a bit stream written forward into zeroed bytes ---------------------------------------------------------------------------------------
struct ZeBits {
    uint8_t *p;
    uint64_t bit = 0;
    MKZS_HD void put(uint32_t v, uint32_t nb) {  // nb <= 32
        if (!nb) return;
        uint64_t x = (uint64_t)(nb < 32 ? v & ((1u << nb) - 1) : v) << (bit & 7u);
        for (uint64_t at = bit >> 3; x; x >>= 8, ++at) p[at] |= (uint8_t)x;
        bit += nb;
    }
    MKZS_HD uint32_t close() {  // the end mark -> bytes
        put(1, 1);
        return (uint32_t)((bit + 7) >> 3);
    }
    MKZS_HD uint32_t bytes() const { return (uint32_t)((bit + 7) >> 3); }
};

// ---- Huffman: code lengths (code_lengths_from_sorted, limit 11) -> weights, codes, the direct-weight header -------------------------------
// lens[0, n_sym) (0: unused) -> weights[0, n_sym); returns the longest length (= the decoder's max_bits)
MKZS_HD uint32_t ze_huf_weights(const uint8_t *lens, uint32_t n_sym, uint8_t *weights) {
    uint32_t mb = 0;
    for (uint32_t s = 0; s < n_sym; ++s) mb = lens[s] > mb ? lens[s] : mb;
    for (uint32_t s = 0; s < n_sym; ++s) weights[s] = lens[s] ? (uint8_t)(mb + 1 - lens[s]) : 0;
    return mb;
}
// the codes the decoder's table implies: the symbols of weight w, by symbol, take the next 2^(w-1) entries each -> code[s] of mb + 1 - w bits,
// its most significant bit read first.  rank: 16 words of scratch
MKZS_HD void ze_huf_codes(const uint8_t *weights, uint32_t n_sym, uint32_t mb, uint16_t *code, uint32_t *rank) {
    for (uint32_t w = 0; w < 16; ++w) rank[w] = 0;
    for (uint32_t s = 0; s < n_sym; ++s) rank[weights[s]]++;
    uint32_t pos = 0;
    for (uint32_t w = 1; w <= mb; ++w) {
        const uint32_t c = rank[w];
        rank[w] = pos, pos += c << (w - 1);
    }
    for (uint32_t s = 0; s < n_sym; ++s) {
        const uint32_t w = weights[s];
        code[s] = 0;
        if (!w) continue;
        code[s] = (uint16_t)(rank[w] >> (w - 1));
        rank[w] += 1u << (w - 1);
    }
}
MKZS_HD uint32_t ze_huf_header_bytes(uint32_t last_sym) { return 1 + (last_sym + 1) / 2; }
// weights[0, last_sym) written, the one of last_sym (the largest used symbol, 1 .. 128) implied; returns the bytes
MKZS_HD uint32_t ze_huf_header(const uint8_t *weights, uint32_t last_sym, uint8_t *out) {
    out[0] = (uint8_t)(127 + last_sym);
    for (uint32_t i = 0; i < last_sym; i += 2) out[1 + i / 2] = (uint8_t)(weights[i] << 4 | (i + 1 < last_sym ? weights[i + 1] : 0));
    return ze_huf_header_bytes(last_sym);
}

// ---- FSE: normalised counts, the table description, the cost estimate -----------------------------------------------------------------------
// -log2(p / 2^log) in 1/256 bit, the fraction interpolated linearly (p >= 1)
MKZS_HD uint32_t ze_cost256(uint32_t p, uint32_t log) {
    const uint32_t hb = (uint32_t)floor_log2(p);
    const uint32_t frac = ((p << 8) >> hb) - 256;  // 0 .. 255
    return ((log - hb) << 8) - frac;
}
// the accuracy log of a described table: enough slots for the distinct codes, no more than the sequences can fill, within the format's maximum
MKZS_HD uint32_t ze_fse_log(uint32_t which, uint32_t total) {
    const uint32_t hb = (uint32_t)floor_log2(total);
    uint32_t log = hb > 2 ? hb - 2 : 0;
    if (log < 6) log = 6;  // (64 slots: every alphabet here has at most 53 codes)
    return log > zs_max_log(which) ? zs_max_log(which) : log;
}
// count[0, n_sym) of `total` (>= 2 distinct codes) -> norm[0, n_sym): 0 for an unused code, >= 1 for a used one, summing to 1 << log
MKZS_HD void ze_fse_normalize(const uint32_t *count, uint32_t n_sym, uint32_t total, uint32_t log, int16_t *norm) {
    int32_t left = 1 << log;
    uint32_t big = 0;
    for (uint32_t s = 0; s < n_sym; ++s) {
        uint32_t p = 0;
        if (count[s]) {
            p = (uint32_t)(((uint64_t)count[s] << log) / total);
            if (!p) p = 1;
        }
        norm[s] = (int16_t)p, left -= (int32_t)p;
        if (norm[s] > norm[big]) big = s;
    }
    if (left >= 0) {
        norm[big] = (int16_t)(norm[big] + left);
        return;
    }
    while (left < 0) {  // the small codes were rounded up to one slot each: the largest ones give them
        big = 0;
        for (uint32_t s = 1; s < n_sym; ++s)
            if (norm[s] > norm[big]) big = s;
        norm[big]--, left++;
    }
}
// the description of norm (4.1.1; the inverse of zs_read_fse) into zeroed bytes -> its bytes.  norm sums to 1 << log and holds no -1
MKZS_HD uint32_t ze_fse_describe(const int16_t *norm, uint32_t n_sym, uint32_t log, uint8_t *out) {
    ZeBits b{out};
    b.put(log - 5, 4);
    int32_t remaining = 1 << log;
    uint32_t s = 0;
    while (remaining > 0 && s < n_sym) {
        const uint32_t max = (uint32_t)remaining + 1, nb = 32 - (uint32_t)__builtin_clz(max), lower = (1u << nb) - 1 - max;
        const uint32_t val = (uint32_t)(norm[s] + 1);
        if (val < lower) b.put(val, nb - 1);
        else b.put(val < (1u << (nb - 1)) ? val : val + lower, nb);
        remaining -= norm[s];
        ++s;
        if (val == 1) {  // how many more unused codes follow, in steps of three
            uint32_t z = 0;
            while (s + z < n_sym && !norm[s + z]) ++z;
            s += z;
            for (; z >= 3; z -= 3) b.put(3, 2);
            b.put(z, 2);
        }
    }
    return b.bytes();
}
// bits the payload takes under a distribution, estimated from the histogram (1/256 bit).  norm: the table's, or nullptr for the predefined one
MKZS_HD uint64_t ze_table_cost(const uint32_t *count, uint32_t n_sym, const int16_t *norm, uint32_t which, uint32_t log) {
    uint64_t c = 0;
    for (uint32_t s = 0; s < n_sym; ++s) {
        if (!count[s]) continue;
        const int p = norm ? norm[s] : zs_default_norm(which, s);
        c += (uint64_t)count[s] * ze_cost256(p < 1 ? 1u : (uint32_t)p, log);
    }
    return c;
}
// the mode of table `which` (0 LL, 1 OF, 2 ML) from its histogram: 1 = RLE where one code occurs, else 0 = Predefined or 2 = FSE_Compressed,
// whichever costs less (description + payload).  norm[0, 64), *log: the distribution the encoder builds its table from; desc (zeroed,
// kZeDescMax bytes), *desc_bytes: what goes into the sequences section for it
MKZS_HD uint32_t ze_choose_table(uint32_t which, const uint32_t *count, uint32_t total, int16_t *norm, uint32_t *log, uint8_t *desc, uint32_t *desc_bytes) {
    const uint32_t n_def = zs_default_symbols(which);
    uint32_t n_sym = 0, distinct = 0, only = 0;
    for (uint32_t s = 0; s <= zs_max_symbol(which); ++s)
        if (count[s]) n_sym = s + 1, ++distinct, only = s;
    if (distinct == 1) {
        for (uint32_t s = 0; s < 64; ++s) norm[s] = 0;
        norm[only] = 1, *log = 0, desc[0] = (uint8_t)only, *desc_bytes = 1;
        return 1;
    }
    const uint32_t flog = ze_fse_log(which, total);
    for (uint32_t s = 0; s < 64; ++s) norm[s] = 0;
    ze_fse_normalize(count, n_sym, total, flog, norm);
    const uint32_t bytes = ze_fse_describe(norm, n_sym, flog, desc);
    const bool pre_ok = n_sym <= n_def;
    const uint64_t cost_fse = (uint64_t)bytes * 8 * 256 + ze_table_cost(count, n_sym, norm, which, flog);
    if (pre_ok && ze_table_cost(count, n_sym, nullptr, which, zs_default_log(which)) <= cost_fse) {
        for (uint32_t s = 0; s < 64; ++s) norm[s] = s < n_def ? (int16_t)zs_default_norm(which, s) : 0;
        for (uint32_t k = 0; k < bytes; ++k) desc[k] = 0;
        *log = zs_default_log(which), *desc_bytes = 0;
        return 0;
    }
    *log = flog, *desc_bytes = bytes;
    return 2;
}

// ---- FSE: the encoding table ------------------------------------------------------------------------------------------------------------
struct ZeSym {
    int32_t dnb, dfs;  // deltaNbBits, deltaFindState of FSE's encoder: bits out = (state + dnb) >> 16, next = table[(state >> bits) + dfs]
};
// the spread of 4.1.1 (what zs_build_fse does for the decoder): slot -> symbol.  Serial form; zstd_deflate.hip spreads across the wave
MKZS_HD void ze_fse_spread(const int16_t *norm, uint32_t n_sym, uint32_t log, uint8_t *slot_sym) {
    const uint32_t size = 1u << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    uint32_t high = size - 1;
    for (uint32_t s = 0; s < n_sym; ++s)
        if (norm[s] == -1) slot_sym[high--] = (uint8_t)s;
    uint32_t pos = 0;
    for (uint32_t s = 0; s < n_sym; ++s)
        for (int32_t i = 0; i < norm[s]; ++i) {
            slot_sym[pos] = (uint8_t)s;
            do pos = (pos + step) & mask;
            while (pos > high);
        }
}
// slot_sym -> state[0, size) and tt[0, n_sym).  cumul: n_sym + 1 halfwords of scratch
MKZS_HD void ze_fse_fill(const int16_t *norm, uint32_t n_sym, uint32_t log, const uint8_t *slot_sym, uint16_t *state, ZeSym *tt, uint16_t *cumul) {
    const uint32_t size = 1u << log;
    cumul[0] = 0;
    for (uint32_t s = 0; s < n_sym; ++s) cumul[s + 1] = (uint16_t)(cumul[s] + (norm[s] == -1 ? 1 : norm[s]));
    for (uint32_t u = 0; u < size; ++u) state[cumul[slot_sym[u]]++] = (uint16_t)(size + u);
    int32_t total = 0;
    for (uint32_t s = 0; s < n_sym; ++s) {
        const int32_t p = norm[s] == -1 ? 1 : norm[s];
        if (p == 0) {
            tt[s] = ZeSym{(int32_t)((log + 1) << 16) - (int32_t)size, 0};
        } else if (p == 1) {
            tt[s] = ZeSym{(int32_t)(log << 16) - (int32_t)size, total - 1};
            total += 1;
        } else {
            const uint32_t out = log - (uint32_t)floor_log2((uint32_t)p - 1);
            tt[s] = ZeSym{(int32_t)(out << 16) - (int32_t)((uint32_t)p << out), total - p};
            total += p;
        }
    }
}
// the state a chain starts in when the LAST symbol it codes is sym (no bits are written for it)
MKZS_HD uint32_t ze_fse_first(const uint16_t *state, const ZeSym *tt, uint32_t sym) {
    const ZeSym t = tt[sym];
    const uint32_t nb = (uint32_t)(t.dnb + (1 << 15)) >> 16;
    const uint32_t v = (nb << 16) - (uint32_t)t.dnb;
    return state[(int32_t)(v >> nb) + t.dfs];
}
// one step: the low *nb bits of st go out, -> the next state
MKZS_HD uint32_t ze_fse_step(const uint16_t *state, const ZeSym *tt, uint32_t st, uint32_t sym, uint32_t *nb) {
    const ZeSym t = tt[sym];
    *nb = (uint32_t)((int32_t)st + t.dnb) >> 16;
    return state[(int32_t)(st >> *nb) + t.dfs];
}

// ---- section headers ------------------------------------------------------------------------------------------------------------------------
// Raw (type 0) / RLE (type 1) literals of `regen` bytes -> header bytes
MKZS_HD uint32_t ze_lit_header_plain(uint32_t type, uint32_t regen, uint8_t *out) {
    if (regen < 32) {
        out[0] = (uint8_t)(type | regen << 3);
        return 1;
    }
    if (regen < 4096) {
        out[0] = (uint8_t)(type | 1u << 2 | (regen & 15u) << 4), out[1] = (uint8_t)(regen >> 4);
        return 2;
    }
    out[0] = (uint8_t)(type | 3u << 2 | (regen & 15u) << 4), out[1] = (uint8_t)(regen >> 4), out[2] = (uint8_t)(regen >> 12);
    return 3;
}
MKZS_HD uint32_t ze_lit_header_plain_bytes(uint32_t regen) { return regen < 32 ? 1 : regen < 4096 ? 2 : 3; }
// Huffman-coded literals: one stream below 1024 literals (10-bit sizes), four from there on (14-bit sizes below 16384, 18-bit beyond)
MKZS_HD uint32_t ze_lit_streams(uint32_t regen) { return regen < 1024 ? 1 : 4; }
MKZS_HD uint32_t ze_lit_header_huf_bytes(uint32_t regen, uint32_t comp) { return regen < 1024 ? 3 : (regen < 16384 && comp < 16384) ? 4 : 5; }
MKZS_HD uint32_t ze_lit_header_huf(uint32_t regen, uint32_t comp, uint8_t *out) {
    const uint32_t bytes = ze_lit_header_huf_bytes(regen, comp), fmt = bytes == 3 ? 0 : bytes == 4 ? 2 : 3, w = bytes == 3 ? 10 : bytes == 4 ? 14 : 18;
    const uint64_t v = 2u | fmt << 2 | (uint64_t)regen << 4 | (uint64_t)comp << (4 + w);
    for (uint32_t k = 0; k < bytes; ++k) out[k] = (uint8_t)(v >> (8 * k));
    return bytes;
}
// the sequence count (3.1.1.3.2.1) -> bytes
MKZS_HD uint32_t ze_seq_count(uint32_t n_seq, uint8_t *out) {
    if (n_seq < 128) {
        out[0] = (uint8_t)n_seq;
        return 1;
    }
    if (n_seq < 0x7F00) {
        out[0] = (uint8_t)((n_seq >> 8) + 128), out[1] = (uint8_t)n_seq;
        return 2;
    }
    out[0] = 255, out[1] = (uint8_t)(n_seq - 0x7F00), out[2] = (uint8_t)((n_seq - 0x7F00) >> 8);
    return 3;
}
// the frame around one block of `size` content bytes (type 0 raw, 1 RLE, 2 compressed) of n bytes of text: 9 bytes of frame header and the
// block header (descriptor 0xA4: Single_Segment, Content_Checksum, 4-byte Frame_Content_Size; Last_Block set)
MKZS_HD void ze_frame_head(uint32_t n, uint32_t type, uint32_t size, uint8_t *out) {
    out[0] = 0x28, out[1] = 0xB5, out[2] = 0x2F, out[3] = 0xFD, out[4] = 0xA4;
    for (uint32_t k = 0; k < 4; ++k) out[5 + k] = (uint8_t)(n >> (8 * k));
    const uint32_t bh = 1u | type << 1 | size << 3;
    out[9] = (uint8_t)bh, out[10] = (uint8_t)(bh >> 8), out[11] = (uint8_t)(bh >> 16);
}

}  // namespace mkz
