// zstd_inflate.hip -- a .zst file decoded on the device, a wave per block (mk_zstd_inflate_device, zstd_host.cpp).
//
// A zstd frame is a chain of blocks of at most 128 KiB whose starts the host reads without decoding anything (zstd_plan.hpp), and a
// block depends on the rest of its frame through three nameable things only: the tables it repeats, the three repeat offsets at its
// start, the text its matches reach into.  Each is carried by a kernel boundary or a small scan; no wave waits for another inside a
// kernel.  Replaces, for `extract`, the zstd reader the reference gets from needletail (src/cmd_extract.rs:281).
//
//   mk_zs_decode_kernel    one wave per block, all blocks of all frames side by side.  All 64 lanes run zs_decode_block of
//                          zstd_serial.hpp with the same values: the bit readers are fed from a window of 64 dwords held one per lane,
//                          the Huffman table and the three FSE tables are built in LDS -- a table the block repeats is built again
//                          from the bytes that describe it in the defining block, which the walk has named, so no table crosses
//                          between waves -- raw and one-byte literals are copied and filled by the whole wave, the four Huffman
//                          streams and the sequences are decoded one after the other (single stores by lane 0).  It leaves the
//                          literals, the sequences as (literals length, match length, offset value), the bytes the block makes and
//                          its effect on the repeat offsets in symbolic form.
//   (the host's two scans: where every block's text starts, and the three offsets in front of it -- zs_scan)
//   mk_zs_execute_kernel   one wave per block: literals are copied by the whole wave; a match copies byte k from byte k mod offset of
//                          the offset bytes in front of it, all lanes at once whatever the overlap.  A source in front of the block's
//                          first byte is not read: the byte records the text position it copies from (one 32-bit source per byte).
//                          What the wave itself wrote is read back past the CU's L1, behind a wait for its stores.
//   mk_zs_resolve_kernel   one round of pointer doubling over the text: a byte whose source is there takes its value, any other takes
//                          its source's source.  A round reads the round before it only (two source arrays); the host launches
//                          rounds until one leaves nothing open, at most log2(blocks) + 2 of them.
//
// A stream (mk_zstd_stream_*, zstd_chain.hpp) launches the same three kernels per window: text below `settled` -- the history the
// window before left, copied to the front of the text buffer -- is final, the execute step reads a match source there as a byte,
// and the rounds start behind it.  The one-shot call passes 0 for both.
//
// LDS: ZsTables, 9.8 KB per wave in the decode kernel (58 VGPRs; LDS admits 16 waves per CU), none elsewhere (14 and 14 VGPRs).  No
// private memory anywhere (profiles/isa_resources.txt).
#include <hip/hip_runtime.h>

#include "codec_kernels.h"
#include "zstd_serial.hpp"

namespace mkz {
namespace {

// ---- the policies of zstd_serial.hpp for a wave.  Inlined by force: a policy whose `this` is handed to a call lives in private memory
struct ZsWaveWords {
    const uint32_t *in32;
    uint64_t n_words, base;
    uint32_t mine, lane;
    __device__ __forceinline__ uint32_t word(uint64_t i) {
        if ((i >> 6) != base) {
            base = i >> 6;
            const uint64_t j = base * 64 + lane;
            mine = j < n_words ? in32[j] : 0u;
        }
        return (uint32_t)__shfl((int)mine, (int)(i & 63u));
    }
};
struct ZsWaveOut {
    const uint8_t *in;
    uint8_t *lit;
    uint32_t *ll, *ml, *of;
    uint8_t *text;
    uint32_t *src;
    uint32_t lane;
    uint64_t synced;   // every store of this wave to text below this position has been waited for
    uint64_t settled;  // text below this position is final: a stream's history, copied there by an earlier operation of the launch's
                       // HIP stream (the one-shot call: 0)
    __device__ __forceinline__ bool leader() const { return lane == 0; }
    __device__ __forceinline__ uint32_t first() const { return lane; }
    __device__ __forceinline__ uint32_t step() const { return 64; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
    __device__ __forceinline__ uint32_t in_byte(uint64_t i) const { return in[i]; }
    __device__ __forceinline__ void lit_put(uint64_t i, uint32_t b) const {
        if (lane == 0) lit[i] = (uint8_t)b;
    }
    __device__ __forceinline__ void lit_copy(uint64_t i, uint64_t from, uint32_t n) const {
        for (uint32_t k = lane; k < n; k += 64) lit[i + k] = in[from + k];
    }
    __device__ __forceinline__ void lit_fill(uint64_t i, uint32_t n, uint32_t b) const {
        for (uint32_t k = lane; k < n; k += 64) lit[i + k] = (uint8_t)b;
    }
    __device__ __forceinline__ void seq_put(uint64_t i, uint32_t l, uint32_t m, uint32_t o) const {
        if (lane == 0) ll[i] = l, ml[i] = m, of[i] = o;
    }
    __device__ __forceinline__ void text_lits(uint64_t to, uint64_t from, uint32_t n) {
        for (uint32_t k = lane; k < n; k += 64) text[to + k] = lit[from + k], src[to + k] = kZsResolved;
    }
    __device__ __forceinline__ void text_in(uint64_t to, uint64_t from, uint32_t n) {
        for (uint32_t k = lane; k < n; k += 64) text[to + k] = in[from + k], src[to + k] = kZsResolved;
    }
    __device__ __forceinline__ void text_fill(uint64_t to, uint32_t n, uint32_t b) {
        for (uint32_t k = lane; k < n; k += 64) text[to + k] = (uint8_t)b, src[to + k] = kZsResolved;
    }
    __device__ __forceinline__ uint32_t text_match(uint64_t to, uint64_t off, uint32_t len, uint64_t block_pos) {
        const uint64_t src_end = to - off + (off < len ? off : len);
        if (src_end > block_pos && src_end > synced) {  // the wave reads what it wrote: behind a wait for those stores
            __threadfence();
            __syncthreads();
            synced = to;
        }
        uint32_t open = 0;
        for (uint32_t k0 = 0; k0 < len; k0 += 64) {
            const uint32_t k = k0 + lane;
            bool is_open = false;
            if (k < len) {
                const uint64_t from = to - off + (off >= len ? k : k % off);
                if (from < settled) {
                    // (a per-lane choice, no cross-lane step inside it.  A plain load: this launch does not write below `settled`)
                    text[to + k] = text[from], src[to + k] = kZsResolved;
                } else if (from < block_pos) {
                    src[to + k] = (uint32_t)from, is_open = true;
                } else {
                    // (past the CU's L1: a line may have been cached before its last bytes were stored)
                    const uint32_t s = __hip_atomic_load(src + from, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (s == kZsResolved) text[to + k] = __hip_atomic_load(text + from, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), src[to + k] = kZsResolved;
                    else src[to + k] = s, is_open = true;
                }
            }
            open += (uint32_t)__popcll(__ballot(is_open));
        }
        return open;
    }
};

__global__ __launch_bounds__(64) void mk_zs_decode_kernel(const uint8_t *in, uint64_t n, uint64_t n_words, const ZsBlock *blocks, uint8_t *lit, uint32_t *ll,
                                                         uint32_t *ml, uint32_t *of, ZsReport *rep) {
    __shared__ ZsTables T;
    const uint32_t lane = threadIdx.x, b = blockIdx.x;
    ZsIn<ZsWaveWords> bits;
    bits.w = ZsWaveWords{reinterpret_cast<const uint32_t *>(in), n_words, ~0ull, 0u, lane};
    ZsWaveOut out{in, lit, ll, ml, of, nullptr, nullptr, lane, 0, 0};
    ZsReport r;
    zs_decode_block(bits, n, blocks[b], T, out, r);
    if (lane == 0) rep[b] = r;
}

__global__ __launch_bounds__(64) void mk_zs_execute_kernel(const uint8_t *in, const ZsBlock *blocks, const ZsStart *start, const ZsReport *rep, uint8_t *lit,
                                                          uint32_t *ll, uint32_t *ml, uint32_t *of, uint8_t *text, uint32_t *src, uint64_t settled,
                                                          int32_t *status, unsigned long long *open_total) {
    const uint32_t lane = threadIdx.x, b = blockIdx.x;
    ZsWaveOut out{in, lit, ll, ml, of, text, src, lane, 0, settled};
    uint32_t open = 0;
    const int st = zs_execute(blocks[b], start[b], rep[b].regen, ll, ml, of, out, &open);
    if (lane == 0) {
        status[b] = st;
        if (open) atomicAdd(open_total, (unsigned long long)open);
    }
}

// positions [first, total): what lies below `first` (a stream's settled history) is final and is never a source's source -- every
// source of a visited byte is either settled, and was then copied by the execute step, or lies in an earlier block of the same
// window --, so zs_round_cap(blocks of the window) bounds the rounds as it bounds them for a whole file
__global__ __launch_bounds__(256) void mk_zs_resolve_kernel(const uint32_t *a, uint32_t *b, uint8_t *text, uint64_t first, uint64_t total,
                                                            unsigned long long *open_total) {
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t base = first + (uint64_t)blockIdx.x * 256; base < total; base += (uint64_t)gridDim.x * 256) {
        const uint64_t i = base + threadIdx.x;
        const uint32_t open = i < total ? zs_resolve_byte(i, a, b, text) : 0u;
        const unsigned long long m = __ballot(open != 0);
        if (m && lane == (uint32_t)__builtin_ctzll(m)) atomicAdd(open_total, (unsigned long long)__popcll(m));
    }
}

}  // namespace

void launch_zs_decode(const uint8_t *in, uint64_t n, uint64_t n_words, const void *blocks, uint32_t n_blocks, uint8_t *lit, uint32_t *ll, uint32_t *ml, uint32_t *of,
                      void *rep, hipStream_t s) {
    hipLaunchKernelGGL(mk_zs_decode_kernel, dim3(n_blocks), dim3(64), 0, s, in, n, n_words, reinterpret_cast<const ZsBlock *>(blocks), lit, ll, ml, of,
                       reinterpret_cast<ZsReport *>(rep));
}
void launch_zs_execute(const uint8_t *in, const void *blocks, const void *start, const void *rep, uint32_t n_blocks, uint8_t *lit, uint32_t *ll, uint32_t *ml,
                       uint32_t *of, uint8_t *text, uint32_t *src, uint64_t settled, int32_t *status, unsigned long long *open_total, hipStream_t s) {
    hipLaunchKernelGGL(mk_zs_execute_kernel, dim3(n_blocks), dim3(64), 0, s, in, reinterpret_cast<const ZsBlock *>(blocks), reinterpret_cast<const ZsStart *>(start),
                       reinterpret_cast<const ZsReport *>(rep), lit, ll, ml, of, text, src, settled, status, open_total);
}
void launch_zs_resolve(const uint32_t *a, uint32_t *b, uint8_t *text, uint64_t first, uint64_t total, unsigned long long *open_total, int num_cus, hipStream_t s) {
    const uint64_t want = (total - first + 255) / 256;
    const uint32_t grid = (uint32_t)(want < (uint64_t)num_cus * 16 ? want : (uint64_t)num_cus * 16);
    hipLaunchKernelGGL(mk_zs_resolve_kernel, dim3(grid ? grid : 1), dim3(256), 0, s, a, b, text, first, total, open_total);
}

}  // namespace mkz
