// bzip2_inflate.hip -- a .bz2 file decoded on the device, a wave per block (mk_bzip2_inflate_device, codec_host.cpp).
//
// bzip2 is the compressed input that suits this machine: its blocks (at most 900 000 symbols) are independent, every block starts
// with a 48-bit magic that can be searched for at every bit offset, and a block that decodes to exactly the bit where the next magic
// stands proves its guessed start.  Replaces, for `extract`, the bzip2 reader the reference gets from needletail (src/cmd_extract.rs:281).
//
//   mk_bz2_markers_kernel  every bit offset tested for the two magics; the hits leave the wave compacted (ballot / popcount, one
//                          atomic per wave and bit phase) as bit << 1 | kind.  The host sorts the few of them and walks them into
//                          streams and blocks (bzip2_stream.hpp).
//   mk_bz2_decode_kernel   one wave per block.  All 64 lanes run bz2_decode_block of bzip2_serial.hpp with the same values: the bit
//                          reader is fed from a window of 64 dwords held one per lane (one global round trip per 256 bytes of
//                          stream), the move-to-front list is 256 bytes across the lanes (4 per lane; a take is two cross-lane
//                          moves, no loop), the six code tables are built by six lanes at once, zero runs are stored by the
//                          whole wave, single bytes by lane 0.  Then the wave turns the histogram into row starts (a scan across
//                          the lanes) and scatters the inverse-BWT vector 64 symbols at a time: lanes that hold the same byte find
//                          each other with 8 ballots, their ranks inside the group keep the sort stable.
//   mk_bz2_walk_kernel     lane 0 of a wave per block walks the vector from origPtr: nblock dependent loads, latency-bound (the
//                          accepted cost here; splitting the cycle into sub-chains is the next step).  It leaves the bytes in front
//                          of the last run-length step, one bit per byte that says "this is a run's count", and the text's length.
//   mk_bz2_expand_kernel   after the host's offsets scan: a wave per block expands 64 bytes per turn to the block's place in the
//                          text (a scan of the lengths across the lanes; a count's copies are stored by the whole wave).
//   mk_bz2_crc_kernel      a wave per block: 64 pieces of the block's text, bzip2's CRC of each, folded (bz2_crc_mulmod).
//
// LDS: Bz2Tables, 7.1 KB per wave (the decode kernel; 1 KB in the CRC kernel, none elsewhere): LDS admits 22 waves per CU, the wave
// slots 32.  Selectors (18 KB) and the 4-byte vector live in device memory.  No private memory anywhere.
#include <hip/hip_runtime.h>

#include "bzip2_serial.hpp"
#include "codec_kernels.h"

namespace mkz {
namespace {

// ---- the policies of bzip2_serial.hpp for a wave ------------------------------------------------------------------------------------
struct BzWaveWords {
    const uint32_t *in32;
    uint64_t n_words, base;
    uint32_t mine, lane;
    __device__ uint32_t word(uint64_t i) {
        if ((i >> 6) != base) {
            base = i >> 6;
            const uint64_t j = base * 64 + lane;
            mine = j < n_words ? __builtin_bswap32(in32[j]) : 0u;
        }
        return (uint32_t)__shfl((int)mine, (int)(i & 63u));
    }
};
// entry p of the list = byte p & 3 of lane p >> 2
struct BzWaveMtf {
    uint32_t m, lane;
    __device__ void init() {
        const uint32_t b = lane * 4;
        m = b | (b + 1) << 8 | (b + 2) << 16 | (b + 3) << 24;
    }
    __device__ uint32_t front() const { return (uint32_t)__shfl((int)m, 0) & 0xffu; }
    __device__ uint32_t take(uint32_t nn) {
        const uint32_t L = nn >> 2, K = nn & 3u;
        const uint32_t v = ((uint32_t)__shfl((int)m, (int)L) >> (8 * K)) & 0xffu;
        const uint32_t up = (uint32_t)__shfl_up((int)m, 1);
        const uint32_t shifted = m << 8 | (lane ? up >> 24 : 0u);  // every entry one place further back
        const uint32_t mask = K == 3 ? 0xffffffffu : (1u << (8 * (K + 1))) - 1;  // lane L: the entries up to nn move, the rest stay
        m = lane < L ? shifted : lane == L ? (shifted & mask) | (m & ~mask) : m;
        if (lane == 0) m = (m & ~0xffu) | v;
        return v;
    }
};
struct BzWaveOut {
    uint8_t *ll8;
    uint32_t lane;
    __device__ bool leader() const { return lane == 0; }
    __device__ uint32_t first() const { return lane; }
    __device__ uint32_t step() const { return 64; }
    __device__ void sync() const { __syncthreads(); }
    __device__ void put(uint32_t i, uint32_t uc) const {
        if (lane == 0) ll8[i] = (uint8_t)uc;
    }
    __device__ void fill(uint32_t i, uint32_t n, uint32_t uc) const {
        for (uint32_t k = lane; k < n; k += 64) ll8[i + k] = (uint8_t)uc;
    }
};

__device__ inline uint32_t wave_inclusive_scan(uint32_t x, uint32_t lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = (uint32_t)__shfl_up((int)x, d);
        if (lane >= (uint32_t)d) x += t;
    }
    return x;
}

// in32: the file (n bytes, zeros up to n_words dwords behind it).  A thread tests the 32 bit offsets of one dword.
__global__ __launch_bounds__(256) void mk_bz2_markers_kernel(const uint32_t *in32, uint64_t n, uint64_t n_words, unsigned long long *table, uint32_t cap,
                                                            uint32_t *count) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t mask48 = (1ull << 48) - 1;
    for (uint64_t base = (uint64_t)blockIdx.x * 256; base * 4 < n; base += (uint64_t)gridDim.x * 256) {
        const uint64_t t = base + threadIdx.x;
        const bool ok = t * 4 < n;
        const uint32_t w0 = ok ? __builtin_bswap32(in32[t]) : 0u, w1 = ok && t + 1 < n_words ? __builtin_bswap32(in32[t + 1]) : 0u,
                       w2 = ok && t + 2 < n_words ? __builtin_bswap32(in32[t + 2]) : 0u;
        const uint64_t hi = (uint64_t)w0 << 32 | w1;
        uint32_t hits = 0, kinds = 0;  // bit j * 8 + k: the magic at bit k of byte j
        for (uint32_t j = 0; j < 4; ++j) {
            const uint64_t v = j ? hi << (8 * j) | w2 >> (32 - 8 * j) : hi;
            for (uint32_t k = 0; k < 8; ++k) {
                const uint64_t cand = (v >> (16 - k)) & mask48;
                const bool inside = (t * 4 + j) * 8 + k + 48 <= n * 8;
                const bool blk = cand == kBzBlockMagic, end = cand == kBzEndMagic;
                if (ok && inside && (blk || end)) hits |= 1u << (j * 8 + k), kinds |= (end ? 1u : 0u) << (j * 8 + k);
            }
        }
        if (!__any(hits != 0)) continue;
        for (uint32_t q = 0; q < 32; ++q) {
            const bool hit = hits >> q & 1u;
            const unsigned long long m = __ballot(hit);
            if (!m) continue;
            uint32_t at = 0;
            if (lane == (uint32_t)__builtin_ctzll(m)) at = atomicAdd(count, (uint32_t)__popcll(m));
            at = (uint32_t)__shfl((int)at, __builtin_ctzll(m));
            const uint32_t mine = at + (uint32_t)__popcll(m & ((1ull << lane) - 1));
            if (hit && mine < cap) table[mine] = (unsigned long long)(t * 32 + q) << 1 | (kinds >> q & 1u);
        }
    }
}

// block b = first + blockIdx.x: its magic at bit blk_bit[b], of a stream of level blk_level[b]; its last column, later the bytes in
// front of the run-length step, at pre + blk_pre[b] (cap bytes, then cap / 8 bytes of count bits; cap = the level's symbols rounded
// up to 128); selectors and vector in slot blockIdx.x of scratch (kBzSelBytes, then 4 x cap bytes)
__global__ __launch_bounds__(64) void mk_bz2_decode_kernel(const uint32_t *in32, uint64_t n, uint64_t n_words, const unsigned long long *blk_bit,
                                                          const uint32_t *blk_level, const unsigned long long *blk_pre, uint8_t *pre, uint8_t *scratch,
                                                          uint64_t slot_bytes, uint32_t first, Bz2Block *rep) {
    __shared__ Bz2Tables T;
    const uint32_t lane = threadIdx.x, b = first + blockIdx.x;
    uint8_t *sel = scratch + (uint64_t)blockIdx.x * slot_bytes;
    uint32_t *tt = reinterpret_cast<uint32_t *>(sel + kBzSelBytes);
    uint8_t *ll8 = pre + blk_pre[b];
    BzBits<BzWaveWords> bits;
    bits.w = BzWaveWords{in32, n_words, ~0ull, 0u, lane};
    bits.n_bits = n * 8;
    bits.seek(blk_bit[b]);
    BzWaveMtf mtf{0u, lane};
    BzWaveOut out{ll8, lane};
    Bz2Block h;
    const int st = bz2_decode_block(bits, blk_level[b], T, sel, mtf, out, h);
    if (lane == 0) rep[b] = h;
    if (st) return;  // (the same in every lane)
    // where every byte's rows start: bins 4 lane .. 4 lane + 3, a scan across the lanes
    {
        const uint32_t c0 = T.hist[4 * lane], c1 = T.hist[4 * lane + 1], c2 = T.hist[4 * lane + 2], c3 = T.hist[4 * lane + 3];
        const uint32_t s = c0 + c1 + c2 + c3, excl = wave_inclusive_scan(s, lane) - s;
        __syncthreads();
        T.hist[4 * lane] = excl, T.hist[4 * lane + 1] = excl + c0, T.hist[4 * lane + 2] = excl + c0 + c1, T.hist[4 * lane + 3] = excl + c0 + c1 + c2;
        __syncthreads();
    }
    // the vector: entry (row) = place in the last column << 8 | byte, the places of equal bytes in ascending order
    const uint32_t nblock = h.nblock;
    uint32_t next = lane < nblock ? ll8[lane] : 0u;
    for (uint32_t i0 = 0; i0 < nblock; i0 += 64) {
        const uint32_t i = i0 + lane, byte = next;
        const bool ok = i < nblock;
        next = i + 64 < nblock ? ll8[i + 64] : 0u;  // (on its way during this turn)
        unsigned long long same = __ballot(ok);
        for (uint32_t k = 0; k < 8; ++k) {
            const unsigned long long m = __ballot(byte >> k & 1u);
            same &= (byte >> k & 1u) ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1));
        const uint32_t start = ok ? T.hist[byte] : 0u;
        if (ok) tt[start + rank] = i << 8 | byte;
        __syncthreads();
        if (ok && rank + 1 == (uint32_t)__popcll(same)) T.hist[byte] = start + rank + 1;
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void mk_bz2_walk_kernel(const unsigned long long *blk_pre, const uint32_t *blk_level, uint8_t *pre, const uint8_t *scratch,
                                                        uint64_t slot_bytes, uint32_t first, Bz2Block *rep, unsigned long long *text_len) {
    const uint32_t b = first + blockIdx.x;
    if (threadIdx.x != 0) return;
    text_len[b] = 0;
    if (rep[b].status != 0) return;
    const uint32_t cap = (blk_level[b] * 100000u + 127u) & ~127u;
    const uint32_t *tt = reinterpret_cast<const uint32_t *>(scratch + (uint64_t)blockIdx.x * slot_bytes + kBzSelBytes);
    uint8_t *p = pre + blk_pre[b];
    uint64_t len = 0;
    const int st = bz2_walk(tt, rep[b].nblock, rep[b].orig_ptr, p, reinterpret_cast<uint32_t *>(p + cap), &len);
    text_len[b] = len;
    if (st) rep[b].status = st;
}

__global__ __launch_bounds__(64) void mk_bz2_expand_kernel(const unsigned long long *blk_pre, const uint32_t *blk_level, const uint8_t *pre, const Bz2Block *rep,
                                                          const unsigned long long *text_off, uint8_t *text) {
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    const uint32_t cap = (blk_level[b] * 100000u + 127u) & ~127u, nblock = rep[b].nblock;
    const uint8_t *p = pre + blk_pre[b];
    const uint32_t *is_count = reinterpret_cast<const uint32_t *>(p + cap);
    uint8_t *o = text + text_off[b];
    uint32_t carry = 0;  // the byte in front of this turn's first
    for (uint32_t i0 = 0; i0 < nblock; i0 += 64) {
        const uint32_t i = i0 + lane;
        const bool ok = i < nblock;
        const uint32_t sym = ok ? p[i] : 0u;
        const bool cnt = ok && (is_count[i >> 5] >> (i & 31u) & 1u);
        const uint32_t len = !ok ? 0u : cnt ? sym : 1u;
        const uint32_t incl = wave_inclusive_scan(len, lane), excl = incl - len;
        const uint32_t up = (uint32_t)__shfl_up((int)sym, 1);
        const uint32_t prev = lane ? up : carry;
        if (ok && !cnt) o[excl] = (uint8_t)sym;
        for (unsigned long long m = __ballot(cnt && sym != 0); m; m &= m - 1) {
            const int l = __builtin_ctzll(m);
            const uint32_t run = (uint32_t)__shfl((int)sym, l), at = (uint32_t)__shfl((int)excl, l), ch = (uint32_t)__shfl((int)prev, l);
            for (uint32_t k = lane; k < run; k += 64) o[at + k] = (uint8_t)ch;
        }
        carry = (uint32_t)__shfl((int)sym, 63);
        o += (uint32_t)__shfl((int)incl, 63);
    }
}

__global__ __launch_bounds__(64) void mk_bz2_crc_kernel(const uint8_t *text, const unsigned long long *text_off, const unsigned long long *text_len, uint32_t *crc) {
    __shared__ uint32_t table[256];
    const uint32_t b = blockIdx.x, lane = threadIdx.x;
    for (uint32_t i = lane; i < 256; i += 64) table[i] = bz2_crc_table_entry(i);
    __syncthreads();
    const uint64_t len = text_len[b], piece = (len + 63) / 64;
    const uint8_t *t = text + text_off[b];
    const uint64_t a = min(piece * lane, len), e = min(piece * (lane + 1), len);
    uint32_t c = lane == 0 ? 0xffffffffu : 0u;
    for (uint64_t i = a; i < e; ++i) c = bz2_crc_byte(c, t[i], table);
    // fold: every lane follows (the values are the same in all of them)
    const uint32_t full = bz2_crc_x_pow_bytes(piece);
    uint32_t r = (uint32_t)__shfl((int)c, 0);
    for (uint32_t j = 1; j < 64; ++j) {
        const uint64_t aj = min(piece * j, len), ej = min(piece * (j + 1), len);
        const uint32_t cj = (uint32_t)__shfl((int)c, (int)j);
        if (ej == aj) continue;
        r = bz2_crc_mulmod(r, ej - aj == piece ? full : bz2_crc_x_pow_bytes(ej - aj)) ^ cj;
    }
    if (lane == 0) crc[b] = ~r;
}

}  // namespace

void launch_bz2_markers(const uint8_t *in, uint64_t n, uint64_t n_words, unsigned long long *table, uint32_t cap, uint32_t *count, int num_cus, hipStream_t s) {
    const uint64_t want = (n / 4 + 255) / 256 + 1;
    const uint32_t grid = (uint32_t)(want < (uint64_t)num_cus * 16 ? want : (uint64_t)num_cus * 16);
    hipLaunchKernelGGL(mk_bz2_markers_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<const uint32_t *>(in), n, n_words, table, cap, count);
}
void launch_bz2_decode(const uint8_t *in, uint64_t n, uint64_t n_words, const unsigned long long *blk_bit, const uint32_t *blk_level, const unsigned long long *blk_pre,
                       uint8_t *pre, uint8_t *scratch, uint64_t slot_bytes, uint32_t first, uint32_t count, void *rep, hipStream_t s) {
    hipLaunchKernelGGL(mk_bz2_decode_kernel, dim3(count), dim3(64), 0, s, reinterpret_cast<const uint32_t *>(in), n, n_words, blk_bit, blk_level, blk_pre, pre, scratch,
                       slot_bytes, first, reinterpret_cast<Bz2Block *>(rep));
}
void launch_bz2_walk(const unsigned long long *blk_pre, const uint32_t *blk_level, uint8_t *pre, const uint8_t *scratch, uint64_t slot_bytes, uint32_t first,
                     uint32_t count, void *rep, unsigned long long *text_len, hipStream_t s) {
    hipLaunchKernelGGL(mk_bz2_walk_kernel, dim3(count), dim3(64), 0, s, blk_pre, blk_level, pre, scratch, slot_bytes, first, reinterpret_cast<Bz2Block *>(rep), text_len);
}
void launch_bz2_expand(const unsigned long long *blk_pre, const uint32_t *blk_level, const uint8_t *pre, const void *rep, const unsigned long long *text_off,
                       uint8_t *text, uint32_t n_blocks, hipStream_t s) {
    hipLaunchKernelGGL(mk_bz2_expand_kernel, dim3(n_blocks), dim3(64), 0, s, blk_pre, blk_level, pre, reinterpret_cast<const Bz2Block *>(rep), text_off, text);
}
void launch_bz2_crc(const uint8_t *text, const unsigned long long *text_off, const unsigned long long *text_len, uint32_t *crc, uint32_t n_blocks, hipStream_t s) {
    hipLaunchKernelGGL(mk_bz2_crc_kernel, dim3(n_blocks), dim3(64), 0, s, text, text_off, text_len, crc);
}

}  // namespace mkz
