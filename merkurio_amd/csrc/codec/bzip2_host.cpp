// bzip2_host.cpp -- host side of mk_bzip2_inflate_device (include/merkurio_hip.h): a .bz2 file decoded on the device, a wave per
// block.  The walk over the table of magics is mkz::bz2_plan (bzip2_stream.hpp); kernels: bzip2_inflate.hip.  The buffers are the gzip
// path's (codec_internal.h).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../host_common.h"
#include "bzip2_stream.hpp"
#include "codec_internal.h"
#include "codec_kernels.h"

using mkz::elapsed;
using mkz::now_ms;
using mkz::upload;

namespace {

constexpr uint32_t kBzMaxMarkers = 1u << 20;  // candidates of one file; more = not taken (900 kB blocks: 1 Mi of them are ~1 TB of text)
constexpr uint64_t kBzMaxPassBlocks = 4096;

// a device error on this path hands the file back (*taken stays 0), it is not the caller's error.  NOTE: the macro RETURNS from
// the function that uses it.  Kernels of the pass may still be in flight then; nothing is waited for here, because the wrapper
// (mk_bzip2_inflate_device) frees the buffers they use right after, and hipFree waits for the device first
#define MKB_HIP(call)                      \
    do {                                   \
        if ((call) != hipSuccess) {        \
            (void)hipGetLastError();       \
            return MK_OK;                  \
        }                                  \
    } while (0)

// `need` bytes in buffers of which the handle holds `held` already: what has to be added fits into half of the free memory
bool bz_room(uint64_t need, uint64_t held) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return false;
    return need <= held || need - held <= free_b / 2;
}
bool bz_ensure(void **p, size_t *cap, size_t need) {
    if (mk::ensure_device(p, cap, need) == MK_OK) return true;
    (void)hipGetLastError();
    return false;
}

int bzip2_inflate(mk_codec *c, const uint8_t *bz, uint64_t n, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_blocks) {
    if (n < 14 || bz[0] != 'B' || bz[1] != 'Z' || bz[2] != 'h' || bz[3] < '1' || bz[3] > '9') return MK_OK;
    MKB_HIP(hipSetDevice(c->device));
    // ---- the file goes up whole
    double t0 = now_ms();
    const uint64_t n_words = (n + mkz::kBzStreamPad + 3) / 4;
    if (!bz_room(n_words * 4 + kBzMaxMarkers * 8ull + 64, c->gz_in_cap + c->gz_tab_cap) || !bz_ensure(&c->d_gz_in, &c->gz_in_cap, n_words * 4) ||
        !bz_ensure(&c->d_gz_tab, &c->gz_tab_cap, kBzMaxMarkers * 8ull + 64))
        return MK_OK;
    if (upload(c, c->d_gz_in, bz, n)) return MK_OK;
    MKB_HIP(hipMemsetAsync((uint8_t *)c->d_gz_in + n, 0, n_words * 4 - n, c->stream));
    MKB_HIP(hipStreamSynchronize(c->stream));
    c->bz_ms[0] = (float)(now_ms() - t0);
    // ---- every bit offset tested for the two magics
    t0 = now_ms();
    unsigned long long *d_markers = (unsigned long long *)c->d_gz_tab;
    uint32_t *d_count = (uint32_t *)(d_markers + kBzMaxMarkers);
    MKB_HIP(hipMemsetAsync(d_count, 0, 4, c->stream));
    mkz::launch_bz2_markers((const uint8_t *)c->d_gz_in, n, n_words, d_markers, kBzMaxMarkers, d_count, c->num_cus, c->stream);
    MKB_HIP(hipGetLastError());
    uint32_t count = 0;
    MKB_HIP(hipMemcpyAsync(&count, d_count, 4, hipMemcpyDeviceToHost, c->stream));
    MKB_HIP(hipStreamSynchronize(c->stream));
    if (count > kBzMaxMarkers) return MK_OK;
    std::vector<unsigned long long> raw(count);
    if (count) MKB_HIP(hipMemcpyAsync(raw.data(), d_markers, count * 8ull, hipMemcpyDeviceToHost, c->stream));
    MKB_HIP(hipStreamSynchronize(c->stream));
    std::sort(raw.begin(), raw.end());
    std::vector<mkz::BzMarker> markers(count);
    for (uint32_t k = 0; k < count; ++k) markers[k] = mkz::BzMarker{raw[k] >> 1, (uint32_t)(raw[k] & 1u)};
    c->bz_ms[1] = (float)(now_ms() - t0);
    // ---- the table walked into streams and blocks (guesses: every block has yet to end on the magic behind it)
    std::vector<mkz::BzPlanBlock> blocks;
    std::vector<mkz::BzPlanStream> streams;
    if (!mkz::bz2_plan(bz, n, markers, blocks, streams)) return MK_OK;
    const size_t B = blocks.size();
    std::vector<uint32_t> crcs(B);
    uint64_t total = 0;
    if (B) {
        // per block: its symbols as bytes (later: the bytes in front of the run-length step) and a bit per byte, kept for all
        // blocks; selectors and the 4-byte vector per block of a pass
        std::vector<unsigned long long> bit(B), pre_off(B), text_off(B), text_len(B);
        std::vector<uint32_t> level(B);
        uint64_t pre_total = 0, slot_bytes = 0;
        for (size_t k = 0; k < B; ++k) {
            const uint64_t cap = (blocks[k].level * 100000ull + 127) & ~127ull;
            bit[k] = blocks[k].bit, level[k] = blocks[k].level, pre_off[k] = pre_total;
            pre_total += cap + cap / 8;
            slot_bytes = std::max<uint64_t>(slot_bytes, mkz::kBzSelBytes + 4 * cap);
        }
        size_t free_b = 0, total_b = 0;
        MKB_HIP(hipMemGetInfo(&free_b, &total_b));
        const uint64_t budget = free_b / 2 + c->gz_sym_cap + c->gz_ctx_cap;  // (what the handle holds of them already is not asked for again)
        if (pre_total + slot_bytes > budget) return MK_OK;
        uint64_t pass = c->bz_pass_blocks ? c->bz_pass_blocks : std::max<uint64_t>(1, (budget - pre_total) / 2 / slot_bytes);
        pass = std::min<uint64_t>(std::min<uint64_t>(pass, B), kBzMaxPassBlocks);
        // tables behind each other: bit | pre_off | text_off | text_len (u64) | level | crc (u32) | reports
        const size_t tab_bytes = B * (8 * 4 + 4 * 2 + sizeof(mkz::Bz2Block)) + 64;
        if (!bz_ensure(&c->d_gz_tab, &c->gz_tab_cap, tab_bytes) || !bz_ensure(&c->d_gz_sym, &c->gz_sym_cap, pre_total + 64) ||
            !bz_ensure(&c->d_gz_ctx, &c->gz_ctx_cap, pass * slot_bytes))
            return MK_OK;
        unsigned long long *d_bit = (unsigned long long *)c->d_gz_tab, *d_pre = d_bit + B, *d_toff = d_pre + B, *d_tlen = d_toff + B;
        mkz::Bz2Block *d_rep = (mkz::Bz2Block *)(d_tlen + B);
        uint32_t *d_level = (uint32_t *)(d_rep + B), *d_crc = d_level + B;
        MKB_HIP(hipMemcpyAsync(d_bit, bit.data(), B * 8, hipMemcpyHostToDevice, c->stream));
        MKB_HIP(hipMemcpyAsync(d_pre, pre_off.data(), B * 8, hipMemcpyHostToDevice, c->stream));
        MKB_HIP(hipMemcpyAsync(d_level, level.data(), B * 4, hipMemcpyHostToDevice, c->stream));
        std::vector<mkz::Bz2Block> rep(B);
        for (size_t b0 = 0; b0 < B; b0 += pass) {
            const uint32_t cnt = (uint32_t)std::min<uint64_t>(pass, B - b0);
            MKB_HIP(hipEventRecord(c->ev[0], c->stream));
            mkz::launch_bz2_decode((const uint8_t *)c->d_gz_in, n, n_words, d_bit, d_level, d_pre, (uint8_t *)c->d_gz_sym, (uint8_t *)c->d_gz_ctx, slot_bytes, (uint32_t)b0,
                                   cnt, d_rep, c->stream);
            MKB_HIP(hipGetLastError());
            MKB_HIP(hipEventRecord(c->ev[1], c->stream));
            mkz::launch_bz2_walk(d_pre, d_level, (uint8_t *)c->d_gz_sym, (const uint8_t *)c->d_gz_ctx, slot_bytes, (uint32_t)b0, cnt, d_rep, d_tlen, c->stream);
            MKB_HIP(hipGetLastError());
            MKB_HIP(hipEventRecord(c->ev[2], c->stream));
            MKB_HIP(hipMemcpyAsync(rep.data() + b0, d_rep + b0, cnt * sizeof(mkz::Bz2Block), hipMemcpyDeviceToHost, c->stream));
            MKB_HIP(hipMemcpyAsync(text_len.data() + b0, d_tlen + b0, cnt * 8ull, hipMemcpyDeviceToHost, c->stream));
            MKB_HIP(hipStreamSynchronize(c->stream));
            c->bz_ms[2] += elapsed(c->ev[0], c->ev[1]), c->bz_ms[3] += elapsed(c->ev[1], c->ev[2]);
            // the proof of a guess: the block ends exactly on the magic behind it.  (Every return inside this loop, MKB_HIP's included,
            // leaves *taken at 0: the file is libbz2's.  The stream has been waited for above, so nothing of this pass is in flight here)
            for (size_t k = b0; k < b0 + cnt; ++k)
                if (rep[k].status != 0 || rep[k].end_bit != blocks[k].end_bit) return MK_OK;
        }
        for (size_t k = 0; k < B; ++k) text_off[k] = total, total += text_len[k];
        // ---- the text at every block's offset, and its CRC.  Both phases are the kernels' own time between events, like the decode and
        // the walk: the allocation of the text and the small copies around them belong to no phase
        MKB_HIP(hipMemGetInfo(&free_b, &total_b));
        if (total + 128 > c->gz_text_cap && total + 128 - c->gz_text_cap > free_b / 2) return MK_OK;
        if (!bz_ensure(&c->d_gz_text, &c->gz_text_cap, total + 128)) return MK_OK;
        MKB_HIP(hipMemcpyAsync(d_toff, text_off.data(), B * 8, hipMemcpyHostToDevice, c->stream));
        MKB_HIP(hipEventRecord(c->ev[0], c->stream));
        mkz::launch_bz2_expand(d_pre, d_level, (const uint8_t *)c->d_gz_sym, d_rep, d_toff, (uint8_t *)c->d_gz_text, (uint32_t)B, c->stream);
        MKB_HIP(hipGetLastError());
        MKB_HIP(hipEventRecord(c->ev[1], c->stream));
        mkz::launch_bz2_crc((const uint8_t *)c->d_gz_text, d_toff, d_tlen, d_crc, (uint32_t)B, c->stream);
        MKB_HIP(hipGetLastError());
        MKB_HIP(hipEventRecord(c->ev[2], c->stream));
        MKB_HIP(hipMemcpyAsync(crcs.data(), d_crc, B * 4, hipMemcpyDeviceToHost, c->stream));
        MKB_HIP(hipStreamSynchronize(c->stream));
        c->bz_ms[3] += elapsed(c->ev[0], c->ev[1]), c->bz_ms[4] = elapsed(c->ev[1], c->ev[2]);
        for (size_t k = 0; k < B; ++k)
            if (crcs[k] != rep[k].crc) return MK_OK;
    }
    for (const mkz::BzPlanStream &s : streams) {
        uint32_t crc = 0;
        for (uint32_t k = 0; k < s.n_blocks; ++k) crc = mkz::bz2_stream_crc_fold(crc, crcs[s.first_block + k]);
        if (crc != s.crc) return MK_OK;
    }
    c->gz_text_bytes = total, c->bz_blocks = (uint32_t)B;
    *text_bytes = total, *taken = 1, *n_blocks = B;
    return MK_OK;
}

}  // namespace

extern "C" {

int mk_bzip2_inflate_device(mk_codec *c, const uint8_t *bz, uint64_t n, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_blocks) {
    MK_ABI_BEGIN
    if (!c || !text_bytes || !taken || !n_blocks || (n && !bz)) return mk::fail(MK_E_INVALID_ARG, "mk_bzip2_inflate_device: NULL argument");
    *text_bytes = 0, *taken = 0, *n_blocks = 0;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->gzs.active) return mk::fail(MK_E_INVALID_ARG, "mk_bzip2_inflate_device: the handle has an open stream (mk_gzip_stream_end)");
    c->gz_text_bytes = 0, c->bz_blocks = 0;
    for (float &x : c->bz_ms) x = 0;
    const int rc = bzip2_inflate(c, bz, n, text_bytes, taken, n_blocks);
    // what is left to keep is the text: the file, the bytes in front of the run-length step and the vectors go back to the device now
    mkz::gz_keep_text(c);
    return rc;
    MK_ABI_END
}

int mk_bzip2_info(const mk_codec *c, uint32_t *blocks, float ms[5]) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_bzip2_info: NULL handle");
    if (blocks) *blocks = c->bz_blocks;
    if (ms)
        for (int k = 0; k < 5; ++k) ms[k] = c->bz_ms[k];
    return MK_OK;
}

}  // extern "C"
