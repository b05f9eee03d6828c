// xz_inflate.hip -- an .xz file decoded on the device, a wave per block (mk_xz_inflate_device, and window by window mk_xz_stream_*: xz_host.cpp).
//
// The Index of an .xz file says where every block's bytes lie and how long its text is (xz_plan.hpp), so nothing is searched for or
// guessed here: block b's wave decodes its LZMA2 chunks to text + text_off[b].  LZMA inside a block is serial, one adaptive bit at
// a time; the gain is blocks side by side.
//
//   mk_xz_decode_kernel  one wave per block.  All 64 lanes run lzma2_decode_block of lzma_serial.hpp with the same values: range,
//                        code, state, the four distances and the positions are made wave-uniform where they enter (readfirstlane
//                        of a probability, of an input dword), so the compiler keeps the decoder on the scalar side.  The
//                        probabilities are 16-bit entries in LDS, 1846 + (768 << (lc + lp)) of them, sized per launch by the largest
//                        lc + lp among the file's chunks.  Compressed bytes reach the wave 64 dwords at a time, one per lane.  Behind
//                        the probabilities: a ring of the latest kXzRing text bytes.
//   mk_xz_check_kernel   a wave per block: 64 pieces of the block's text, the CRC-32 or CRC-64 register of each, folded by a
//                        carry-less multiply-mod (crc64.hpp), compared with the stored check.  Check None: nothing is read.  A lane's
//                        piece is contiguous (ceil(len / 64) bytes, walked bytewise), so the lanes' reads lie a piece apart and are not
//                        coalesced: nothing beside the decode today; interleaved or wave-wide pieces are the step if decode gets faster.
//
// WHERE THE DECODER READS TEXT BACK FROM, and why those bytes are there.  It reads back the byte at rep0 (a matched literal, a short
// rep), the last byte of a match (the next literal's context), and a match's source.
//   * A literal is stored into the ring by EVERY lane, the same byte at the same address: a lane that reads it later reads a byte it
//     stored itself, which program order of one thread guarantees.  Likewise every probability.  Literals go to device memory kXzLitStage
//     at a time, or when a match or the block's end needs them there (flush: lane i reads ring byte i -- its own store).
//   * A match is stored by the whole wave in turns of 64 bytes, lane i byte 64 t + i, to device memory and to the ring; where
//     dist < len the lanes read src + i % dist, so every turn reads bytes from in front of the match only.  Behind a match stands a
//     barrier (a block is one wave: the barrier is the wait for the LDS stores): ring bytes another lane stored are read only behind it.
//   * The ring serves a distance only when dist + len <= kXzRing: source and destination then do not meet in the ring.  Any other
//     source is read from device memory, where this wave stored it earlier (all pending literals are flushed in front of a match,
//     and a far matched literal lies more than kXzRing - kXzLitStage bytes behind the flushed end).  In front of such a read stands a
//     workgroup-scope fence: it waits for the wave's own stores, and within one compute unit loads behind it see them.
//
// LDS per wave: 2 x (1846 + (768 << lclp)) + kXzRing bytes = 19.7 KB at lc + lp = 3 (xz's presets), 31.7 KB at 4: of 160 KiB that
// admits 8 and 5 waves per CU.  No private memory (scratch 0); 106 SGPRs, 38 VGPRs, and 493 SGPR spills (491 before the order table): the decoder's values are
// scalar, but the compiler keeps part of them in VGPR lanes (v_writelane / v_readlane) inside the bit loop.
#include <hip/hip_runtime.h>

#include "codec_kernels.h"
#include "crc64.hpp"
#include "lzma_serial.hpp"
#include "xz_kernel_edges.h"
#include "xz_plan.hpp"

namespace mkz {
namespace {

__device__ inline uint32_t uni(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }

// ---- the policies of lzma_serial.hpp for a wave ---------------------------------------------------------------------------------------
// the file's dwords (little-endian, zeros up to n_words behind it), 64 at a time; byte i of the block = byte base + i of the file
struct XzWaveIn {
    const uint32_t *in32;
    uint64_t n_words, base, window, cur_w;
    uint32_t mine, cur, lane;
    __device__ uint32_t byte(uint64_t i) {
        const uint64_t a = base + i, w = a >> 2;
        if (w != cur_w) {
            if ((w / kXzRefillDwords) != window) {
                window = w / kXzRefillDwords;
                const uint64_t j = window * kXzRefillDwords + lane;
                mine = j < n_words ? in32[j] : 0u;
            }
            cur_w = w, cur = uni((uint32_t)__shfl((int)mine, (int)(w % kXzRefillDwords)));
        }
        return cur >> (8 * (uint32_t)(a & 3u)) & 0xffu;
    }
};
struct XzWaveProbs {
    uint16_t *v;
    uint32_t lane;
    __device__ uint32_t get(uint32_t i) const { return uni(v[i]); }
    __device__ void set(uint32_t i, uint32_t x) { v[i] = (uint16_t)x; }
    __device__ void fill(uint32_t n) {
        __syncthreads();
        for (uint32_t i = lane; i < n; i += 64) v[i] = (uint16_t)kLzProbInit;
        __syncthreads();
    }
};
struct XzWaveOut {
    uint8_t *text;  // the block's
    uint8_t *ring;
    const uint8_t *in8;  // the file, for stored chunks
    uint64_t in_base, flushed;
    uint32_t lane;
    // text[flushed, upto) leaves the ring (at most kXzLitStage literals, each stored by every lane)
    __device__ void flush(uint64_t upto) {
        const uint32_t n = (uint32_t)(upto - flushed);
        if (lane < n) text[flushed + lane] = ring[(flushed + lane) & (kXzRing - 1)];
        flushed = upto;
    }
    __device__ void lit(uint64_t pos, uint32_t b) {
        ring[pos & (kXzRing - 1)] = (uint8_t)b;
        if (pos + 1 - flushed == kXzLitStage) flush(pos + 1);
    }
    __device__ uint32_t back(uint64_t pos, uint64_t dist) const {
        if (dist <= kXzRing) return uni(ring[(pos - dist) & (kXzRing - 1)]);
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        return uni(text[pos - dist]);
    }
    __device__ void copy(uint64_t pos, uint64_t dist, uint32_t len) {
        flush(pos);
        const bool near = dist + len <= kXzRing;
        const uint32_t d32 = dist < len ? (uint32_t)dist : len;  // (k % d32 = k where dist >= len)
        if (!near) __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        for (uint32_t k = lane; k < len; k += 64) {
            const uint64_t src = pos - dist + (k < d32 ? k : k % d32);
            const uint8_t b = near ? ring[src & (kXzRing - 1)] : text[src];
            text[pos + k] = b;
            ring[(pos + k) & (kXzRing - 1)] = b;
        }
        flushed = pos + len;
        __syncthreads();
    }
    template <class In>
    __device__ void stored(uint64_t pos, In &, uint64_t at, uint32_t n) {
        flush(pos);
        const uint8_t *src = in8 + in_base + at;
        for (uint32_t k = lane; k < n; k += 64) {
            const uint8_t b = src[k];
            text[pos + k] = b;
            ring[(pos + k) & (kXzRing - 1)] = b;
        }
        flushed = pos + n;
        __syncthreads();
    }
    __device__ void finish(uint64_t pos) { flush(pos); }
};

// blocks[b]: XzBlock; the file (a stream: the window's span of it) in in32 (n_words dwords, zeros behind its bytes: the j < n_words
// guard of XzWaveIn keeps the last block's read-ahead inside the upload); text: of the whole file (the window).  status[b] = 0 or the
// refusal.  order (may be null): workgroup i handles block order[i] -- a window passes its blocks largest text first; that workgroups
// start in index order is an assumption, nothing here depends on it.  Dynamic LDS: 2 x lzma_probs(lclp_room) rounded up to 16, then kXzRing
__global__ __launch_bounds__(64) void mk_xz_decode_kernel(const uint32_t *in32, uint64_t n_words, const XzBlock *blocks, const uint32_t *order, uint8_t *text,
                                                         uint32_t lclp_room, int32_t *status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const uint32_t lane = threadIdx.x, b = order ? order[blockIdx.x] : blockIdx.x;
    const XzBlock B = blocks[b];
    XzWaveIn in{in32, n_words, B.in_off, ~0ull, ~0ull, 0u, 0u, lane};
    XzWaveProbs pr{reinterpret_cast<uint16_t *>(lds), lane};
    XzWaveOut out{text + B.text_off, lds + ((2 * lzma_probs(lclp_room) + 15u) & ~15u), reinterpret_cast<const uint8_t *>(in32), B.in_off, 0, lane};
    LzNoCensus cs;
    uint64_t made = 0;
    const int st = lzma2_decode_block(in, B.in_bytes, pr, out, B.text_bytes, B.dict_size, lclp_room, cs, &made);
    if (lane == 0) status[b] = st;
}

// check[b] = 0: the block's check matches (or its kind is None), kLzCheck: it does not
template <typename T>
__device__ int xz_check_block(const uint8_t *t, uint64_t len, const uint8_t *stored, T *table, uint32_t lane) {
    for (uint32_t i = lane; i < 256; i += 64) table[i] = xz_crc_table_entry<T>(i);
    __syncthreads();
    const uint64_t piece = (len + 63) / 64;
    const uint64_t a = min(piece * lane, len), e = min(piece * (lane + 1), len);
    T c = lane == 0 ? ~(T)0 : (T)0;
    for (uint64_t i = a; i < e; ++i) c = xz_crc_byte<T>(c, t[i], table);
    // fold: every lane follows (the values are the same in all of them)
    const T full = xz_crc_x_pow_bytes<T>(piece);
    T r = ~(T)0;
    for (uint32_t j = 0; j < 64; ++j) {
        const uint64_t aj = min(piece * j, len), ej = min(piece * (j + 1), len);
        T cj;
        if (sizeof(T) == 8) {
            const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)c, (int)j), hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)c >> 32), (int)j);
            cj = (T)((uint64_t)hi << 32 | lo);
        } else {
            cj = (T)(uint32_t)__shfl((int)(uint32_t)c, (int)j);
        }
        if (j == 0) {
            r = cj;
            continue;
        }
        if (ej == aj) continue;
        r = xz_crc_mulmod<T>(r, ej - aj == piece ? full : xz_crc_x_pow_bytes<T>(ej - aj)) ^ cj;
    }
    r = ~r;
    T want = 0;
    for (uint32_t k = 0; k < sizeof(T); ++k) want |= (T)stored[k] << (8 * k);
    return r == want ? 0 : kLzCheck;
}

__global__ __launch_bounds__(64) void mk_xz_check_kernel(const uint8_t *in8, const XzBlock *blocks, const uint32_t *order, const uint8_t *text, const int32_t *status,
                                                        int32_t *check) {
    __shared__ uint64_t table[256];
    const uint32_t lane = threadIdx.x, b = order ? order[blockIdx.x] : blockIdx.x;
    const XzBlock B = blocks[b];
    int st = 0;
    if (status[b] != 0 || B.check_kind == kXzCheckNone) {
        st = 0;  // (a block that failed is the decode status's; None costs nothing)
    } else if (B.check_kind == kXzCheckCrc32) {
        st = xz_check_block<uint32_t>(text + B.text_off, B.text_bytes, in8 + B.check_off, reinterpret_cast<uint32_t *>(table), lane);
    } else {
        st = xz_check_block<uint64_t>(text + B.text_off, B.text_bytes, in8 + B.check_off, table, lane);
    }
    if (lane == 0) check[b] = st;
}

}  // namespace

size_t xz_decode_lds_bytes(uint32_t lclp_room) { return ((2 * lzma_probs(lclp_room) + 15u) & ~15u) + kXzRing; }

void launch_xz_decode(const uint8_t *in, uint64_t n_words, const void *blocks, const uint32_t *order, uint32_t n_blocks, uint8_t *text, uint32_t lclp_room,
                      int32_t *status, hipStream_t s) {
    hipLaunchKernelGGL(mk_xz_decode_kernel, dim3(n_blocks), dim3(64), xz_decode_lds_bytes(lclp_room), s, reinterpret_cast<const uint32_t *>(in), n_words,
                       reinterpret_cast<const XzBlock *>(blocks), order, text, lclp_room, status);
}
void launch_xz_check(const uint8_t *in, const void *blocks, const uint32_t *order, uint32_t n_blocks, const uint8_t *text, const int32_t *status, int32_t *check,
                     hipStream_t s) {
    hipLaunchKernelGGL(mk_xz_check_kernel, dim3(n_blocks), dim3(64), 0, s, in, reinterpret_cast<const XzBlock *>(blocks), order, text, status, check);
}

}  // namespace mkz
