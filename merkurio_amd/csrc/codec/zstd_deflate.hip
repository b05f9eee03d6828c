// zstd_deflate.hip -- Zstandard frames written on the device: LZ77 parse, Huffman literals, FSE sequences, bit packing, XXH64.
//
// Behind mk_zstd_deflate_records (include/merkurio_hip.h): the kept records of `extract` leave as .zst the way they leave as BGZF under
// -z (bgzf_deflate.hip), so that a job that reads reads.fastq.zst can hand back hits.fastq.zst without the host's libzstd threads.  One
// frame per cut of the record-end rule (bgzf_cuts.hpp with kZsCutGrid / kZsCutReach: at most 128 KiB of text), one block per frame, no
// match reaches in front of its block: every frame decodes alone.  The serial pieces (weights, table descriptions, FSE tables, headers)
// are zstd_enc_serial.hpp's, which the host harness checks against libzstd; the fixed choices are listed there.
//
// One WAVE per frame, one wave per workgroup, a resident grid (8 waves per CU) whose waves take the next frame from a counter:
//   1. parse, 64 positions at a time, as bgzf_deflate.hip does: 3-byte hash -> most recent earlier position (1 Ki entries in LDS), match
//      length by 8-byte compares up to the block's end (no 258 cap), a distance-1 candidate for runs, the wave-uniform walk with one-step
//      lazy evaluation.  Literals are compacted into the wave's literal scratch and counted in LDS; a match writes (literals so far,
//      length, offset) to the wave's sequence scratch.
//   2. literals (raw or Huffman; never RLE, see there): keys rank-sorted by the wave, one lane runs the length-limited builder (11 bits) and derives weights and codes; the
//      bits of each of the one or four streams are summed by the wave, so the section's size is known before a bit is written.
//   3. sequences: codes and histograms by the wave (a sequence per lane); lanes 0-2 choose a table's mode each; the symbol spread runs
//      across the wave, lanes 0-2 fill a table each; then the only serial chain: the three FSE states walk the sequences from the last
//      to the first, a state per lane (offset, match length, literal length), and leave every sequence's state bits in the scratch.
//   4. the block's size is exact now: not smaller than the text -> a Raw block.  Otherwise the sections are written: lanes look their
//      codes up, a wave scan places them, they are OR-ed into an LDS staging area and whole bytes go out.  Both kinds of stream are
//      written forward from what the decoder needs LAST and closed with one set bit.
//   5. XXH64 of the text with the four accumulators on four lanes.
// Bound: as bgzf_deflate.hip, latency of dependent LDS / L2 accesses; plus the state chain (two dependent LDS reads per sequence).
#include <hip/hip_runtime.h>

#include "codec_kernels.h"
#include "xxh64.hpp"
#include "zstd_enc_serial.hpp"

namespace mkz {
namespace {

constexpr int kZdHashBits = 10;
constexpr uint32_t kZdMinLen = 3;

__device__ __forceinline__ uint32_t ld32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint64_t ld64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0)); }
__device__ __forceinline__ uint32_t below(uint64_t mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
}
__device__ __forceinline__ uint64_t bits_range(uint32_t a, uint32_t b) {  // bits a .. b-1, a <= b <= 64
    const uint64_t hi = b >= 64 ? ~0ull : (1ull << b) - 1, lo = a >= 64 ? ~0ull : (1ull << a) - 1;
    return hi & ~lo;
}
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, uint32_t lane) {
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t u = __shfl_up(v, o);
        if (lane >= (uint32_t)o) v += u;
    }
    return v;
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    return (uint64_t)(uint32_t)__shfl((int)(uint32_t)v, src) | (uint64_t)(uint32_t)__shfl((int)(uint32_t)(v >> 32), src) << 32;
}
// bytes a[0..) and b[0..) have in common, at most maxlen (reads up to 7 bytes past a + maxlen)
__device__ __forceinline__ uint32_t match_len(const uint8_t *a, const uint8_t *b, uint32_t maxlen) {
    uint32_t l = 0;
    while (l < maxlen) {
        const uint64_t x = ld64(a + l) ^ ld64(b + l);
        if (x) {
            l += (uint32_t)__builtin_ctzll(x) >> 3;
            break;
        }
        l += 8;
    }
    return l < maxlen ? l : maxlen;
}

struct ZdLds {
    union {  // the hash table is dead when the parse is over, before the encoding tables come to life
        uint32_t head[1 << kZdHashBits];
        struct {
            uint16_t state[1280];  // LL (512 states) at 0, OF (256) at 512, ML (512) at 768
            ZeSym tt[3][64];
        } fse;
    };
    uint32_t lit_freq[256];
    uint32_t key[132], skey[132];  // (count << 9 | symbol) of the used literals 0 .. 128, unsorted and ascending
    HuffScratch hs;
    uint8_t lens[132], weights[132];
    uint16_t hcode[132];
    uint32_t rank[16];
    uint32_t seq_freq[3][64];
    int16_t norm[3][64];
    uint8_t slot_sym[3][512];
    uint16_t cumul[3][66];
    uint8_t desc[3][kZeDescMax];
    uint8_t tree[72];
    uint32_t meta[16];   // per table t: [t] mode, [3 + t] accuracy log, [6 + t] description bytes, [9 + t] last slot of the spread
    uint32_t words[192];  // the staging area of the bit packer
};
static_assert(sizeof(ZdLds) <= 20480, "8 waves per CU (160 KiB of LDS)");
static_assert(sizeof(((ZdLds *)0)->fse) <= sizeof(((ZdLds *)0)->head), "the encoding tables fit the hash table's place");

// ---- the bit packer: every lane adds up to two fields (a below b), a wave scan places them, whole bytes go out -------------------------
__device__ __forceinline__ void or_bits(uint32_t *words, uint32_t off, uint64_t v, uint32_t n) {
    if (!n) return;
    if (n < 64) v &= (1ull << n) - 1;
    const uint32_t wi = off >> 5, sh = off & 31u;
    const uint64_t lo = v << sh;
    if ((uint32_t)lo) atomicOr(&words[wi], (uint32_t)lo);
    if ((uint32_t)(lo >> 32)) atomicOr(&words[wi + 1], (uint32_t)(lo >> 32));
    const uint32_t top = sh ? (uint32_t)(v >> (64 - sh)) : 0;
    if (top) atomicOr(&words[wi + 2], top);
}
struct Packer {
    uint32_t *words;  // zero but for the bits held
    uint8_t *dst;     // where the next whole byte goes
    uint8_t *lim;     // the slot's end: nothing is written from here on
    uint32_t fill;    // bits held (below 8 between two adds)
    __device__ __forceinline__ void begin(uint8_t *d, uint32_t lane) {
        dst = d, fill = 0;
        __syncthreads();
        for (uint32_t k = lane; k < 192; k += 64) words[k] = 0;
        __syncthreads();
    }
    // na + nb <= 75 bits per lane: 64 lanes and the held bits stay below 152 words
    __device__ __forceinline__ void add(uint32_t lane, uint64_t a, uint32_t na, uint64_t b, uint32_t nb) {
        const uint32_t n = na + nb, incl = wave_incl_scan(n, lane);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t off = fill + incl - n;
        or_bits(words, off, a, na);
        or_bits(words, off + na, b, nb);
        __syncthreads();
        fill += total;
        const uint32_t bytes = fill >> 3;
        for (uint32_t k = lane; k < bytes; k += 64)
            if (dst + k < lim) dst[k] = (uint8_t)(words[k >> 2] >> (8 * (k & 3u)));
        const uint32_t carry = (words[bytes >> 2] >> (8 * (bytes & 3u))) & 255u;
        __syncthreads();
        for (uint32_t k = lane; k < 192; k += 64) words[k] = 0;
        __syncthreads();
        if (lane == 0) words[0] = carry;
        __syncthreads();
        dst += bytes, fill &= 7u;
    }
    // the end mark, then the last, partial byte
    __device__ __forceinline__ void close(uint32_t lane, uint64_t last, uint32_t n_last) {
        add(lane, lane == 0 ? last : 0, lane == 0 ? n_last : 0, lane == 0 ? 1 : 0, lane == 0 ? 1 : 0);
        if (fill) {
            if (lane == 0 && dst < lim) *dst = (uint8_t)words[0];
            ++dst;
        }
        __syncthreads();
    }
};

// ---- XXH64 of d[0, n), seed 0: the four accumulators on lanes 0-3 (the other lanes repeat them), then the tail on every lane ----------
__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return x << r | x >> (64 - r); }
__device__ __forceinline__ uint64_t xxh_round(uint64_t acc, uint64_t in) { return rotl64(acc + in * Xxh64::P2, 31) * Xxh64::P1; }
__device__ __forceinline__ uint64_t xxh_merge(uint64_t h, uint64_t v) { return (h ^ xxh_round(0, v)) * Xxh64::P1 + Xxh64::P4; }
__device__ uint32_t wave_xxh64(const uint8_t *d, uint32_t n, uint32_t lane) {
    const uint32_t l4 = lane & 3u;
    uint64_t h;
    if (n >= 32) {
        uint64_t v = l4 == 0 ? Xxh64::P1 + Xxh64::P2 : l4 == 1 ? Xxh64::P2 : l4 == 2 ? 0ull : 0ull - Xxh64::P1;
        const uint32_t stripes = n >> 5;
        const uint8_t *p = d + 8 * l4;
        for (uint32_t s = 0; s < stripes; ++s, p += 32) v = xxh_round(v, ld64(p));
        const uint64_t v1 = shfl64(v, 0), v2 = shfl64(v, 1), v3 = shfl64(v, 2), v4 = shfl64(v, 3);
        h = rotl64(v1, 1) + rotl64(v2, 7) + rotl64(v3, 12) + rotl64(v4, 18);
        h = xxh_merge(xxh_merge(xxh_merge(xxh_merge(h, v1), v2), v3), v4);
    } else {
        h = Xxh64::P5;
    }
    h += n;
    const uint8_t *p = d + (n & ~31u);
    uint32_t r = n & 31u;
    for (; r >= 8; p += 8, r -= 8) h = rotl64(h ^ xxh_round(0, ld64(p)), 27) * Xxh64::P1 + Xxh64::P4;
    if (r >= 4) h = rotl64(h ^ (uint64_t)ld32(p) * Xxh64::P1, 23) * Xxh64::P2 + Xxh64::P3, p += 4, r -= 4;
    for (; r; ++p, --r) h = rotl64(h ^ *p * Xxh64::P5, 11) * Xxh64::P1;
    h ^= h >> 33, h *= Xxh64::P2, h ^= h >> 29, h *= Xxh64::P3, h ^= h >> 32;
    return (uint32_t)h;
}

// keys are distinct (the symbol is part of them): the rank of a key is the number of smaller keys
__device__ void wave_rank_sort(const uint32_t *key, uint32_t m, uint32_t *sorted, uint32_t lane) {
    for (uint32_t k = lane; k < m; k += 64) {
        const uint32_t mine = key[k];
        uint32_t r = 0;
        for (uint32_t j = 0; j < m; ++j) r += key[j] < mine;
        sorted[r] = mine;
    }
    __syncthreads();
}

// the symbol spread of table t across the wave: step k of the walk over the slots is slot (k * step) & mask; the steps that land at or
// below `high` (the slots above it hold the "less than one" symbols of a predefined table) take the symbols' occurrences in order
__device__ void wave_fse_spread(ZdLds &L, uint32_t t, uint32_t lane) {
    const uint32_t log = L.meta[3 + t], size = 1u << log, mask = size - 1, step = (size >> 1) + (size >> 3) + 3;
    const int16_t *norm = L.norm[t];
    uint16_t *cumul = L.cumul[t];
    if (lane == 0) {
        uint32_t high = size - 1;
        for (uint32_t s = 0; s < 64; ++s)
            if (norm[s] == -1) L.slot_sym[t][high--] = (uint8_t)s;
        L.meta[9 + t] = high;
        cumul[0] = 0;
    }
    const uint32_t mine = norm[lane] > 0 ? (uint32_t)norm[lane] : 0;
    cumul[lane + 1] = (uint16_t)wave_incl_scan(mine, lane);
    __syncthreads();
    const uint32_t high = L.meta[9 + t];
    uint32_t run = 0;
    for (uint32_t k0 = 0; k0 < size; k0 += 64) {
        const uint32_t k = k0 + lane, pos = (k * step) & mask;
        const bool valid = k < size && pos <= high;
        const uint64_t vm = __ballot(valid);
        if (valid) {
            const uint32_t j = run + below(vm);  // occurrence j: the symbol s with cumul[s] <= j < cumul[s + 1]
            uint32_t lo = 0, hi = 64;
            while (hi - lo > 1) {
                const uint32_t mid = (lo + hi) >> 1;
                if (cumul[mid] <= j) lo = mid;
                else hi = mid;
            }
            L.slot_sym[t][pos] = (uint8_t)lo;
        }
        run += (uint32_t)__popcll(vm);
    }
    __syncthreads();
}

// the wave's scratch in device memory
struct ZdScratch {
    uint8_t *lit;                                 // kZsDeflateLitBytes
    uint32_t *seq_lit, *seq_ml, *seq_of;          // per sequence: literals in front of its match (running count), match length, offset
    uint32_t *code, *sbits;                       // ... its three codes (LL | OF << 8 | ML << 16); its state bits (count << 26 | bits)
    __device__ __forceinline__ explicit ZdScratch(uint8_t *base) {
        lit = base;
        seq_lit = reinterpret_cast<uint32_t *>(base + kZsDeflateLitBytes);
        seq_ml = seq_lit + kZsDeflateSeqCap, seq_of = seq_ml + kZsDeflateSeqCap, code = seq_of + kZsDeflateSeqCap, sbits = code + kZsDeflateSeqCap;
    }
};
static_assert(kZsDeflateLitBytes + 5ull * 4 * kZsDeflateSeqCap == kZsDeflateWaveScratch && kZsDeflateLitBytes % 4 == 0, "the scratch of a wave");
static_assert(kZsDeflateSeqCap * kZdMinLen >= kZsBlockMax && kZsDeflateLitBytes >= kZsBlockMax, "a block's sequences and literals fit the scratch");
static_assert(kZsDeflateSlotBytes >= kZsBlockMax + 16 && kZsDeflateSlotBytes % 4 == 0, "a frame of a Raw block fits its slot");

}  // namespace

// frame b = the text in[off[b], off[b] + len[b]) (len[b] <= 128 KiB; a longer entry is cut short) -> slots[b * kZsDeflateSlotBytes ...],
// its bytes in slot_len[b]; kinds[0 .. 2] += Raw / RLE / Compressed blocks
__global__ __launch_bounds__(64) void mk_zstd_deflate_kernel(const uint8_t *__restrict__ in, const unsigned long long *__restrict__ off,
                                                             const uint32_t *__restrict__ len, uint32_t n_frames, uint8_t *__restrict__ scratch,
                                                             uint8_t *__restrict__ slots, uint32_t *__restrict__ slot_len,
                                                             uint32_t *__restrict__ next_frame, uint32_t *__restrict__ kinds) {
    __shared__ ZdLds L;
    const uint32_t lane = lane_id();
    const ZdScratch S(scratch + (uint64_t)blockIdx.x * kZsDeflateWaveScratch);

    for (;;) {
        uint32_t b = 0;
        if (lane == 0) b = atomicAdd(next_frame, 1u);
        b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
        if (b >= n_frames) break;
        const uint8_t *const src = in + off[b];
        const uint32_t n = len[b] < kZsBlockMax ? len[b] : kZsBlockMax;
        uint8_t *const slot = slots + (uint64_t)b * kZsDeflateSlotBytes;
        uint8_t *const body = slot + 12;
        uint8_t *const slot_end = slot + kZsDeflateSlotBytes;

        // ---- 0. one repeated byte?  (the scan ends at the first 64 bytes that hold another one)
        bool same = n > 0;
        for (uint32_t base = 0; base < n && same; base += 64) same = !__ballot(base + lane < n && src[base + lane] != src[0]);

        uint32_t type = 0, size = n;  // the block: raw unless something smaller is found
        uint32_t n_lit = 0, n_seq = 0;
        uint32_t lit_mode = 0, lit_comp = 0, lit_section = 0, seq_section = 0, streams = 0, q = 0, top = 0;
        uint32_t sb0 = 0, sb1 = 0, sb2 = 0, sb3 = 0;  // bits of the four literal streams
        uint64_t last_bits = 0;
        uint32_t n_last = 0;
        if (same) {
            type = 1;
        } else if (n) {
            for (uint32_t k = lane; k < (1u << kZdHashBits); k += 64) L.head[k] = 0xffffffffu;
            for (uint32_t k = lane; k < 256; k += 64) L.lit_freq[k] = 0;
            __syncthreads();

            // ---- 1. parse ---------------------------------------------------------------------------------------------------
            uint32_t p = 0;  // the next position the parse takes
            for (uint32_t base = 0; base < n; base += 64) {
                if (p >= base + 64) continue;  // inside a match
                const uint32_t i = base + lane;
                const bool can = i + kZdMinLen <= n;
                const uint32_t w = i < n ? ld32(src + i) : 0;  // (bytes behind n: the next frame or the padding, never part of a match)
                uint32_t cand = 0xffffffffu, h = 0;
                if (can) {
                    h = ((w & 0xffffffu) * 0x9E3779B1u) >> (32 - kZdHashBits);
                    cand = L.head[h];
                }
                if (can) L.head[h] = i;  // lanes with one hash: one of them stays, all are earlier positions for what follows
                uint32_t mlen = 0, dist = 0;
                if (can && i >= p) {
                    const uint32_t maxlen = n - i;
                    if (cand != 0xffffffffu) {
                        const uint32_t l = match_len(src + i, src + cand, maxlen);
                        if (l >= kZdMinLen) mlen = l, dist = i - cand;
                    }
                    if (i > 0 && mlen < maxlen && ((ld32(src + i - 1) ^ w) & 0xffffffu) == 0) {  // a run: the nearest candidate the table cannot hold yet
                        const uint32_t l = match_len(src + i, src + i - 1, maxlen);
                        if (l >= mlen) mlen = l, dist = 1;
                    }
                }
                // the walk: wave-uniform, one step per match
                const uint32_t lim = n - base < 64 ? n - base : 64;
                const uint64_t has = __ballot(mlen >= kZdMinLen);
                uint64_t starts = 0, mstarts = 0;
                uint32_t qq = p - base;
                while (qq < lim) {
                    const uint64_t rest = has & bits_range(qq, 64);
                    if (!rest) {
                        starts |= bits_range(qq, lim);
                        qq = lim;
                        break;
                    }
                    const uint32_t m = (uint32_t)__builtin_ctzll(rest);
                    starts |= bits_range(qq, m + 1);
                    const uint32_t l0 = (uint32_t)__builtin_amdgcn_readlane((int)mlen, (int)m);
                    if (m + 1 < lim && ((has >> (m + 1)) & 1) && (uint32_t)__builtin_amdgcn_readlane((int)mlen, (int)(m + 1)) > l0) {
                        qq = m + 1;  // the next position starts a longer match: this one goes out as a literal
                        continue;
                    }
                    mstarts |= 1ull << m;
                    qq = m + l0;
                }
                p = base + qq;
                const uint64_t lits = starts & ~mstarts;
                const uint32_t lit_at = n_lit + below(lits);
                if ((lits >> lane) & 1) {
                    S.lit[lit_at] = (uint8_t)w;
                    atomicAdd(&L.lit_freq[w & 255u], 1u);
                }
                if ((mstarts >> lane) & 1) {
                    const uint32_t idx = n_seq + below(mstarts);
                    S.seq_lit[idx] = lit_at, S.seq_ml[idx] = mlen, S.seq_of[idx] = dist;
                }
                n_lit += (uint32_t)__popcll(lits), n_seq += (uint32_t)__popcll(mstarts);
            }
            __threadfence_block();
            __syncthreads();

            // ---- 2. literals: raw (0) or Huffman (2) ------------------------------------------------------------------------------
            uint32_t m_keys = 0, distinct = 0;
            for (uint32_t s0 = 0; s0 < 256; s0 += 64) {
                const uint32_t s = s0 + lane, f = L.lit_freq[s];
                const uint64_t used = __ballot(f != 0), keyed = __ballot(f != 0 && s <= kZeHufMaxSym);
                if (f && s <= kZeHufMaxSym) L.key[m_keys + below(keyed)] = f << 9 | s;  // (at most 129 of them)
                if (used) top = s0 + 63 - (uint32_t)__builtin_clzll(used);
                m_keys += (uint32_t)__popcll(keyed), distinct += (uint32_t)__popcll(used);
            }
            for (uint32_t k = lane; k < 132; k += 64) L.lens[k] = 0;
            __syncthreads();
            lit_section = ze_lit_header_plain_bytes(n_lit) + n_lit;
            // (RLE literals cannot occur: with no history in front of the block the first occurrence of every byte value is a literal, so one
            // distinct literal means one distinct byte, which is the RLE block above)
            if (distinct >= 2 && top <= kZeHufMaxSym) {
                wave_rank_sort(L.key, m_keys, L.skey, lane);
                if (lane == 0) {
                    code_lengths_from_sorted(L.skey, (int)m_keys, (int)kZsHufLog, L.lens, L.hs);
                    L.meta[15] = ze_huf_weights(L.lens, top + 1, L.weights);
                    ze_huf_codes(L.weights, top + 1, L.meta[15], L.hcode, L.rank);
                    ze_huf_header(L.weights, top, L.tree);
                }
                __syncthreads();
                streams = ze_lit_streams(n_lit), q = streams == 4 ? (n_lit + 3) / 4 : n_lit;
                for (uint32_t j = lane; j < n_lit; j += 64) {
                    const uint32_t l = L.lens[S.lit[j]], k = j / q;
                    sb0 += k == 0 ? l : 0, sb1 += k == 1 ? l : 0, sb2 += k == 2 ? l : 0, sb3 += k >= 3 ? l : 0;
                }
                sb0 = wave_sum(sb0), sb1 = wave_sum(sb1), sb2 = wave_sum(sb2), sb3 = wave_sum(sb3);
                lit_comp = ze_huf_header_bytes(top) + (sb0 >> 3) + 1;
                if (streams == 4) lit_comp += 6 + (sb1 >> 3) + 1 + (sb2 >> 3) + 1 + (sb3 >> 3) + 1;
                const uint32_t huf = ze_lit_header_huf_bytes(n_lit, lit_comp) + lit_comp;
                if (huf < lit_section) lit_mode = 2, lit_section = huf;
            }

            // ---- 3. sequences ---------------------------------------------------------------------------------------------------
            seq_section = 1;
            if (n_seq) {
                for (uint32_t k = lane; k < 192; k += 64) (&L.seq_freq[0][0])[k] = 0;
                __syncthreads();
                uint32_t extra = 0;
                for (uint32_t i = lane; i < n_seq; i += 64) {
                    const uint32_t ll = S.seq_lit[i] - (i ? S.seq_lit[i - 1] : 0);
                    const uint32_t cl = ze_ll_code(ll), co = ze_of_code(S.seq_of[i]), cm = ze_ml_code(S.seq_ml[i]);
                    S.code[i] = cl | co << 8 | cm << 16;
                    atomicAdd(&L.seq_freq[0][cl], 1u), atomicAdd(&L.seq_freq[1][co], 1u), atomicAdd(&L.seq_freq[2][cm], 1u);
                    extra += zs_ll_bits(cl) + co + zs_ml_bits(cm);
                }
                extra = wave_sum(extra);
                for (uint32_t k = lane; k < 3 * kZeDescMax; k += 64) (&L.desc[0][0])[k] = 0;
                __threadfence_block();
                __syncthreads();
                if (lane < 3) L.meta[lane] = ze_choose_table(lane, L.seq_freq[lane], n_seq, L.norm[lane], &L.meta[3 + lane], L.desc[lane], &L.meta[6 + lane]);
                __syncthreads();
                for (uint32_t t = 0; t < 3; ++t) wave_fse_spread(L, t, lane);
                if (lane < 3) ze_fse_fill(L.norm[lane], 64, L.meta[3 + lane], L.slot_sym[lane], L.fse.state + (lane == 0 ? 0u : lane == 1 ? 512u : 768u), L.fse.tt[lane], L.cumul[lane]);
                __syncthreads();
                // the state chain: lane 0 offsets, lane 1 match lengths, the others literal lengths; sequence n_seq - 1 first
                const uint32_t t = lane == 0 ? 1u : lane == 1 ? 2u : 0u, shift = t == 0 ? 0u : t == 1 ? 8u : 16u;
                const uint16_t *const state = L.fse.state + (t == 0 ? 0u : t == 1 ? 512u : 768u);
                const ZeSym *const tt = L.fse.tt[t];
                uint32_t st = 0, state_bits = 0;
                for (uint32_t r0 = 0; r0 < n_seq; r0 += 64) {
                    const uint32_t cnt = n_seq - r0 < 64 ? n_seq - r0 : 64;
                    const uint32_t mine = lane < cnt ? S.code[n_seq - 1 - (r0 + lane)] : 0;
                    for (uint32_t j = 0; j < cnt; ++j) {
                        const uint32_t sym = ((uint32_t)__builtin_amdgcn_readlane((int)mine, (int)j) >> shift) & 255u;
                        uint32_t nb = 0, v = 0;
                        if (r0 + j == 0) {
                            st = ze_fse_first(state, tt, sym);
                        } else {
                            const uint32_t next = ze_fse_step(state, tt, st, sym, &nb);
                            v = st & ((1u << nb) - 1), st = next;
                        }
                        const uint32_t v1 = (uint32_t)__shfl((int)v, 1), n1 = (uint32_t)__shfl((int)nb, 1), v2 = (uint32_t)__shfl((int)v, 2), n2 = (uint32_t)__shfl((int)nb, 2);
                        if (lane == 0) L.words[j] = (nb + n1 + n2) << 26 | v | v1 << nb | v2 << (nb + n1);
                        state_bits += nb + n1 + n2;
                    }
                    __syncthreads();
                    if (lane < cnt) S.sbits[n_seq - 1 - (r0 + lane)] = L.words[lane];
                    __syncthreads();
                }
                state_bits = (uint32_t)__builtin_amdgcn_readfirstlane((int)state_bits);
                // what closes the stream: the states of match length, offset, literal length (the decoder reads them in the opposite order)
                const uint32_t log_ll = L.meta[3], log_of = L.meta[4], log_ml = L.meta[5];
                const uint32_t s_of = (uint32_t)__shfl((int)st, 0), s_ml = (uint32_t)__shfl((int)st, 1), s_ll = (uint32_t)__shfl((int)st, 2);
                last_bits = (uint64_t)(s_ml & ((1u << log_ml) - 1)) | (uint64_t)(s_of & ((1u << log_of) - 1)) << log_ml |
                            (uint64_t)(s_ll & ((1u << log_ll) - 1)) << (log_ml + log_of);
                n_last = log_ll + log_of + log_ml;
                const uint32_t stream_bits = extra + state_bits + n_last + 1;
                seq_section = (n_seq < 128 ? 1u : n_seq < 0x7F00 ? 2u : 3u) + 1 + L.meta[6] + L.meta[7] + L.meta[8] + ((stream_bits + 7) >> 3);
            }
            if (lit_section + seq_section < n) type = 2, size = lit_section + seq_section;
        }

        // ---- 4. the frame ---------------------------------------------------------------------------------------------------------
        if (lane == 0) {
            ze_frame_head(n, type, type == 1 ? n : size, slot);
            atomicAdd(&kinds[type], 1u);
        }
        uint32_t content = size;  // bytes behind the block header
        if (type == 1) {
            content = 1;
            if (lane == 0) body[0] = src[0];
        } else if (type == 0) {
            uint32_t *const bw = reinterpret_cast<uint32_t *>(body);
            for (uint32_t k = lane; k < n >> 2; k += 64) bw[k] = ld32(src + 4 * k);
            if (lane < (n & 3u)) body[(n & ~3u) + lane] = src[(n & ~3u) + lane];
        } else {
            uint8_t *o = body;
            Packer pk{L.words, o, slot_end, 0};
            if (lit_mode == 0) {
                if (lane == 0) ze_lit_header_plain(0, n_lit, o);
                o += ze_lit_header_plain_bytes(n_lit);
                for (uint32_t k = lane; k < n_lit; k += 64) o[k] = S.lit[k];
                o += n_lit;
            } else {
                if (lane == 0) ze_lit_header_huf(n_lit, lit_comp, o);
                o += ze_lit_header_huf_bytes(n_lit, lit_comp);
                const uint32_t tree_bytes = ze_huf_header_bytes(top);
                for (uint32_t k = lane; k < tree_bytes; k += 64) o[k] = L.tree[k];
                o += tree_bytes;
                if (streams == 4) {
                    if (lane < 6) {
                        const uint32_t sz = ((lane >> 1) == 0 ? sb0 : (lane >> 1) == 1 ? sb1 : sb2) / 8 + 1;
                        o[lane] = (uint8_t)(sz >> (8 * (lane & 1u)));
                    }
                    o += 6;
                }
                for (uint32_t k = 0; k < streams; ++k) {
                    const uint32_t a = k * q, e = k + 1 < streams ? a + q : n_lit, cnt = e - a;
                    pk.begin(o, lane);
                    for (uint32_t r0 = 0; r0 < cnt; r0 += 64) {  // the stream's last literal first
                        uint32_t c = 0, l = 0;
                        if (r0 + lane < cnt) {
                            const uint32_t sym = S.lit[e - 1 - (r0 + lane)];
                            c = L.hcode[sym], l = L.lens[sym];
                        }
                        pk.add(lane, c, l, 0, 0);
                    }
                    pk.close(lane, 0, 0);
                    o = pk.dst;
                }
            }
            if (lane == 0) {
                uint8_t *s = o + ze_seq_count(n_seq, o);
                if (n_seq) {
                    *s++ = (uint8_t)(L.meta[0] << 6 | L.meta[1] << 4 | L.meta[2] << 2);
                    for (uint32_t t = 0; t < 3; ++t)
                        for (uint32_t k = 0; k < L.meta[6 + t]; ++k) *s++ = L.desc[t][k];
                }
            }
            if (n_seq) {
                o += (n_seq < 128 ? 1u : n_seq < 0x7F00 ? 2u : 3u) + 1 + L.meta[6] + L.meta[7] + L.meta[8];
                pk.begin(o, lane);
                for (uint32_t r0 = 0; r0 < n_seq; r0 += 64) {  // the last sequence first: its state bits, then its extra bits (LL, ML, OF)
                    uint64_t a = 0, x = 0;
                    uint32_t na = 0, nx = 0;
                    if (r0 + lane < n_seq) {
                        const uint32_t i = n_seq - 1 - (r0 + lane);
                        const uint32_t sbv = S.sbits[i], c = S.code[i], cl = c & 255u, co = (c >> 8) & 255u, cm = c >> 16;
                        a = sbv & 0x3ffffffu, na = sbv >> 26;
                        const uint32_t ll = S.seq_lit[i] - (i ? S.seq_lit[i - 1] : 0);
                        const uint32_t bl = zs_ll_bits(cl), bm = zs_ml_bits(cm);
                        x = (uint64_t)(ll - zs_ll_base(cl)) | (uint64_t)(S.seq_ml[i] - zs_ml_base(cm)) << bl |
                            (uint64_t)(S.seq_of[i] + 3 - (1u << co)) << (bl + bm);
                        nx = bl + bm + co;
                    }
                    pk.add(lane, a, na, x, nx);
                }
                pk.close(lane, last_bits, n_last);
            } else {
                o += 1;
            }
        }
        // ---- 5. the checksum
        const uint32_t sum = wave_xxh64(src, n, lane);
        if (lane < 4 && body + content + lane < slot_end) body[content + lane] = (uint8_t)(sum >> (8 * lane));
        if (lane == 0) slot_len[b] = 16 + content;
        __syncthreads();
    }
}

__global__ __launch_bounds__(128) void mk_zstd_cuts_kernel(const unsigned long long *__restrict__ rec_end, uint64_t n_rec, uint64_t T, uint32_t n_grid,
                                                           unsigned long long *__restrict__ off, uint32_t *__restrict__ len, uint32_t *__restrict__ n_frames) {
    cut_ranges<kZsCutGrid, kZsCutReach>(rec_end, n_rec, T, n_grid, off, len, n_frames);
}

// ---- frames back to back (the two kernels of bgzf_deflate.hip's pack step, over this file's slot size) -------------------------------
__global__ __launch_bounds__(1024) void mk_zstd_offsets_kernel(const uint32_t *__restrict__ len, uint64_t *__restrict__ off, uint64_t *__restrict__ total,
                                                               uint32_t n) {
    __shared__ uint64_t part[1024];
    const uint32_t per = (n + 1023) / 1024, b0 = threadIdx.x * per < n ? threadIdx.x * per : n, e0 = b0 + per < n ? b0 + per : n;
    uint64_t s = 0;
    for (uint32_t i = b0; i < e0; ++i) s += len[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (int k = 0; k < 1024; ++k) {
            const uint64_t v = part[k];
            part[k] = run;
            run += v;
        }
        *total = run;
    }
    __syncthreads();
    uint64_t run = part[threadIdx.x];
    for (uint32_t i = b0; i < e0; ++i) {
        off[i] = run;
        run += len[i];
    }
}
__global__ __launch_bounds__(256) void mk_zstd_pack_kernel(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ len, const uint64_t *__restrict__ off,
                                                           uint8_t *__restrict__ packed) {
    const uint32_t b = blockIdx.x, n = len[b] < kZsDeflateSlotBytes ? len[b] : kZsDeflateSlotBytes;
    const uint8_t *s = slots + (uint64_t)b * kZsDeflateSlotBytes;
    uint8_t *d = packed + off[b];
    for (uint32_t k = threadIdx.x; k < n; k += 256) d[k] = s[k];
}

// ---- launchers --------------------------------------------------------------------------------------------------------------------------
uint32_t zstd_deflate_grid(uint32_t n_frames, int num_cus) {
    const uint32_t resident = (uint32_t)num_cus * 8;
    return n_frames < resident ? n_frames : resident;
}
void launch_zstd_cuts(const unsigned long long *rec_end, uint64_t n_rec, uint64_t n_text, uint32_t n_grid, unsigned long long *off, uint32_t *len,
                      uint32_t *n_frames, hipStream_t s) {
    if (!n_grid) return;
    const uint32_t blocks = (n_grid + 127) / 128;
    hipLaunchKernelGGL(mk_zstd_cuts_kernel, dim3(blocks < kCutBlocks ? blocks : kCutBlocks), dim3(128), 0, s, rec_end, n_rec, n_text, n_grid, off, len, n_frames);
}
void launch_zstd_deflate(const uint8_t *in, const unsigned long long *off, const uint32_t *len, uint32_t n_frames, uint8_t *scratch, uint8_t *slots,
                         uint32_t *slot_len, uint32_t *next_frame, uint32_t *kinds, uint32_t grid, hipStream_t s) {
    if (!n_frames) return;
    (void)hipMemsetAsync(next_frame, 0, 4, s);
    hipLaunchKernelGGL(mk_zstd_deflate_kernel, dim3(grid), dim3(64), 0, s, in, off, len, n_frames, scratch, slots, slot_len, next_frame, kinds);
}
void launch_zstd_pack(const uint8_t *slots, const uint32_t *slot_len, uint64_t *slot_off, uint64_t *total, uint32_t n_frames, uint8_t *packed, hipStream_t s) {
    if (!n_frames) return;
    hipLaunchKernelGGL(mk_zstd_offsets_kernel, dim3(1), dim3(1024), 0, s, slot_len, slot_off, total, n_frames);
    hipLaunchKernelGGL(mk_zstd_pack_kernel, dim3(n_frames), dim3(256), 0, s, slots, slot_len, slot_off, packed);
}

}  // namespace mkz
