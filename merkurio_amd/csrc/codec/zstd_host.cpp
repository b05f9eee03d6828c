// zstd_host.cpp -- host side of mk_zstd_inflate_device (include/merkurio_hip.h): a .zst file decoded on the device, a wave per block,
// the whole file in one call.  The walk over the frames and block headers is mkz::zs_plan, the two scans mkz::zs_scan (zstd_plan.hpp,
// no HIP in it: the CPU harness of the tests runs both); kernels: zstd_inflate.hip.  Here: upload, tables + entropy decode, scans,
// execution, the rounds of cross-block resolution, and the content checksum, which the host computes per frame over the text as it
// comes down through the staging buffers (XXH64 is four serial chains: nothing for a wave to fold).  The buffers are the gzip path's
// (codec_internal.h).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../host_common.h"
#include "codec_internal.h"
#include "codec_kernels.h"
#include "xxh64.hpp"
#include "zstd_plan.hpp"

using mkz::elapsed;
using mkz::now_ms;

namespace {

// a device error on this path hands the file back (*taken stays 0), it is not the caller's error.  NOTE: the macro RETURNS false from
// the function that uses it, behind a wait for the stream: a copy may still be on its way into a vector of that function
#define MKZS_HIP(call)                              \
    do {                                            \
        if ((call) != hipSuccess) {                 \
            (void)hipGetLastError();                \
            (void)hipStreamSynchronize(c->stream);  \
            (void)hipGetLastError();                \
            return false;                           \
        }                                           \
    } while (0)

bool zs_room(uint64_t need, uint64_t held) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
    return need <= held || need - held <= free_b / 2;
}
bool zs_ensure(void **p, size_t *cap, size_t need) {
    if (mk::ensure_device(p, cap, need) == MK_OK) return true;
    (void)hipGetLastError();
    return false;
}
uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

// the whole file in one call; false: not taken
bool zstd_inflate(mk_codec *c, const uint8_t *zs, uint64_t n, uint64_t *text_bytes, uint64_t *n_blocks) {
    mkz::ZsPlan P;
    if (!mkz::zs_plan(zs, n, P)) return false;
    const size_t B = P.blocks.size();
    uint64_t total = 0;
    uint32_t rounds = 0;
    if (B) {
        if (B >= (1u << 30)) return false;
        MKZS_HIP(hipSetDevice(c->device));
        // ---- upload: the file (zeros behind it up to the reader's pad) and the walk's table
        double t0 = now_ms();
        const uint64_t n_words = (n + mkz::kZsStreamPad + 3) / 4;
        const uint64_t lit_bytes = up16(P.lit_bytes + 16), seq_bytes = up16((P.n_seq + 4) * 4);
        // tables: blocks | reports | starts | status | two counters
        const uint64_t o_rep = up16(B * sizeof(mkz::ZsBlock)), o_start = o_rep + up16(B * sizeof(mkz::ZsReport)), o_status = o_start + up16(B * sizeof(mkz::ZsStart)),
                       o_count = o_status + up16(B * 4), tab_bytes = o_count + 64;
        if (!zs_room(n_words * 4 + lit_bytes + 3 * seq_bytes + tab_bytes, c->gz_in_cap + c->gz_sym_cap + c->gz_tab_cap) ||
            !zs_ensure(&c->d_gz_in, &c->gz_in_cap, n_words * 4) || !zs_ensure(&c->d_gz_sym, &c->gz_sym_cap, lit_bytes + 3 * seq_bytes) ||
            !zs_ensure(&c->d_gz_tab, &c->gz_tab_cap, tab_bytes))
            return false;
        if (mkz::upload(c, c->d_gz_in, zs, n)) return false;
        MKZS_HIP(hipMemsetAsync((uint8_t *)c->d_gz_in + n, 0, n_words * 4 - n, c->stream));
        uint8_t *tab = (uint8_t *)c->d_gz_tab;
        MKZS_HIP(hipMemcpyAsync(tab, P.blocks.data(), B * sizeof(mkz::ZsBlock), hipMemcpyHostToDevice, c->stream));
        MKZS_HIP(hipStreamSynchronize(c->stream));
        c->zs_ms[0] = (float)(now_ms() - t0);
        uint8_t *lit = (uint8_t *)c->d_gz_sym;
        uint32_t *ll = (uint32_t *)(lit + lit_bytes), *ml = (uint32_t *)(lit + lit_bytes + seq_bytes), *of = (uint32_t *)(lit + lit_bytes + 2 * seq_bytes);
        unsigned long long *d_open = (unsigned long long *)(tab + o_count);
        // ---- tables + entropy decode
        MKZS_HIP(hipEventRecord(c->ev[0], c->stream));
        mkz::launch_zs_decode((const uint8_t *)c->d_gz_in, n, n_words, tab, (uint32_t)B, lit, ll, ml, of, tab + o_rep, c->stream);
        MKZS_HIP(hipGetLastError());
        MKZS_HIP(hipEventRecord(c->ev[1], c->stream));
        std::vector<mkz::ZsReport> rep(B);
        MKZS_HIP(hipMemcpyAsync(rep.data(), tab + o_rep, B * sizeof(mkz::ZsReport), hipMemcpyDeviceToHost, c->stream));
        MKZS_HIP(hipStreamSynchronize(c->stream));
        c->zs_ms[1] = elapsed(c->ev[0], c->ev[1]);
        for (const mkz::ZsReport &r : rep)
            if (r.status != 0) return false;
        // ---- the two scans: where every block's text starts, the repeat offsets in front of it
        t0 = now_ms();
        std::vector<mkz::ZsStart> start;
        if (!mkz::zs_scan(P, rep, start, &total)) return false;
        c->zs_ms[2] = (float)(now_ms() - t0);
        // ---- execution: the text, and one source per byte in two arrays (a round reads one and writes the other)
        const uint64_t src_bytes = up16(total * 4 + 16);
        if (!zs_room(total + 128 + 2 * src_bytes, c->gz_text_cap + c->gz_ctx_cap) || !zs_ensure(&c->d_gz_text, &c->gz_text_cap, total + 128) ||
            !zs_ensure(&c->d_gz_ctx, &c->gz_ctx_cap, 2 * src_bytes))
            return false;
        uint32_t *src[2] = {(uint32_t *)c->d_gz_ctx, (uint32_t *)((uint8_t *)c->d_gz_ctx + src_bytes)};
        MKZS_HIP(hipMemcpyAsync(tab + o_start, start.data(), B * sizeof(mkz::ZsStart), hipMemcpyHostToDevice, c->stream));
        MKZS_HIP(hipMemsetAsync(d_open, 0, 8, c->stream));
        MKZS_HIP(hipEventRecord(c->ev[0], c->stream));
        mkz::launch_zs_execute((const uint8_t *)c->d_gz_in, tab, tab + o_start, tab + o_rep, (uint32_t)B, lit, ll, ml, of, (uint8_t *)c->d_gz_text, src[0],
                               (int32_t *)(tab + o_status), d_open, c->stream);
        MKZS_HIP(hipGetLastError());
        MKZS_HIP(hipEventRecord(c->ev[1], c->stream));
        std::vector<int32_t> status(B);
        unsigned long long open = 0;
        MKZS_HIP(hipMemcpyAsync(status.data(), tab + o_status, B * 4, hipMemcpyDeviceToHost, c->stream));
        MKZS_HIP(hipMemcpyAsync(&open, d_open, 8, hipMemcpyDeviceToHost, c->stream));
        MKZS_HIP(hipStreamSynchronize(c->stream));
        c->zs_ms[3] = elapsed(c->ev[0], c->ev[1]);
        for (int32_t st : status)
            if (st != 0) return false;
        // ---- cross-block resolution: rounds of pointer doubling until one leaves nothing open
        t0 = now_ms();
        const uint32_t cap = mkz::zs_round_cap(B);
        int cur = 0;
        while (open) {
            if (rounds == cap) return false;
            MKZS_HIP(hipMemsetAsync(d_open, 0, 8, c->stream));
            mkz::launch_zs_resolve(src[cur], src[cur ^ 1], (uint8_t *)c->d_gz_text, total, d_open, c->num_cus, c->stream);
            MKZS_HIP(hipGetLastError());
            MKZS_HIP(hipMemcpyAsync(&open, d_open, 8, hipMemcpyDeviceToHost, c->stream));
            MKZS_HIP(hipStreamSynchronize(c->stream));
            cur ^= 1, ++rounds;
        }
        c->zs_ms[4] = (float)(now_ms() - t0);
        // ---- content checksums: the low 32 bits of XXH64 of every frame's text that carries one
        t0 = now_ms();
        for (const mkz::ZsFrame &F : P.frames) {
            if (!F.has_checksum) continue;
            mkz::Xxh64 h;
            if (F.text_len && mkz::download_each(c, (const uint8_t *)c->d_gz_text + F.text_off, F.text_len, [&](const uint8_t *p, uint64_t m) { h.update(p, m); })) {
                (void)hipGetLastError();
                return false;
            }
            if ((uint32_t)h.digest() != F.checksum) return false;
        }
        c->zs_ms[5] = (float)(now_ms() - t0);
    } else {
        for (const mkz::ZsFrame &F : P.frames) {  // frames without text: their sizes and checksums are checked all the same
            if (F.content_size != ~0ull && F.content_size != 0) return false;
            if (F.has_checksum && (uint32_t)mkz::Xxh64().digest() != F.checksum) return false;
        }
    }
    c->gz_text_bytes = total, c->zs_blocks = (uint32_t)B, c->zs_frames = (uint32_t)P.frames.size(), c->zs_rounds = rounds;
    *text_bytes = total, *n_blocks = B;
    return true;
}

}  // namespace

extern "C" {

int mk_zstd_inflate_device(mk_codec *c, const uint8_t *zs, uint64_t n, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_blocks) {
    MK_ABI_BEGIN
    if (!c || !text_bytes || !taken || !n_blocks || (n && !zs)) return mk::fail(MK_E_INVALID_ARG, "mk_zstd_inflate_device: NULL argument");
    *text_bytes = 0, *taken = 0, *n_blocks = 0;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->stream_open()) return mk::fail(MK_E_INVALID_ARG, "mk_zstd_inflate_device: the handle has an open stream (mk_gzip_stream_end, mk_bzip2_stream_end)");
    c->gz_text_bytes = 0, c->zs_blocks = c->zs_frames = c->zs_rounds = 0;
    for (float &x : c->zs_ms) x = 0;
    // (whatever keeps the file from being taken -- anything the walk, a block or a checksum refuses, no room, a device error -- is MK_OK
    // with *taken = 0: the file is libzstd's)
    uint64_t text = 0, blocks = 0;
    if (zstd_inflate(c, zs, n, &text, &blocks)) *text_bytes = text, *n_blocks = blocks, *taken = 1;
    else c->gz_text_bytes = 0;
    // what is left to keep is the text: the file, the literals, the sequences and the source arrays go back to the device now
    mkz::gz_keep_text(c);
    return MK_OK;
    MK_ABI_END
}

int mk_zstd_info(const mk_codec *c, uint32_t *blocks, uint32_t *frames, uint32_t *rounds, float ms[6]) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_zstd_info: NULL handle");
    if (blocks) *blocks = c->zs_blocks;
    if (frames) *frames = c->zs_frames;
    if (rounds) *rounds = c->zs_rounds;
    if (ms)
        for (int k = 0; k < 6; ++k) ms[k] = c->zs_ms[k];
    return MK_OK;
}

}  // extern "C"
