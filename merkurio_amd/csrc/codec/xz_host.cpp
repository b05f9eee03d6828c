// xz_host.cpp -- host side of mk_xz_inflate_device and mk_xz_stream_* (include/merkurio_hip.h): an .xz file decoded on the device, a
// wave per block -- the whole file in one call, or a file of any size window by window.  The walk over streams, Index records and
// Block Headers is mkz::xz_walk / xz_plan (xz_plan.hpp), everything that is decided about a window xz_chain.hpp's; neither has HIP in
// it and the CPU harnesses of the tests run them; kernels: xz_inflate.hip.  Here: the one body both entry points share -- the upload of
// the compressed bytes and of the block table, the decode launch, the check launch, and the per-block statuses: the first block that
// failed names why the file (the window) is handed back -- and the calls around it.  The buffers are the gzip path's (codec_internal.h).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../host_common.h"
#include "codec_kernels.h"
#include "codec_stream.hpp"
#include "lzma_serial.hpp"
#include "xz_chain.hpp"
#include "xz_plan.hpp"

using mkz::elapsed;
using mkz::now_ms;

namespace {

uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

// ---- the one body: src[0, n) goes up (zeros behind it up to the reader's pad; n_words is THIS upload's, and the kernel's j < n_words
// guard keeps the last block's read-ahead inside it), then the table of B blocks whose in_off / check_off count from src and whose
// text_off from d_text; behind the table: status, check, and the launch order (order == nullptr: block b is workgroup b's).  Decode, a
// wave per block, LDS sized by lclp; then the checks.  0, or the status of the first block in table order that failed, kXzTooLarge
// (no room for the upload and the tables), kXzDevice.  ms[0..2] += upload, decode, check
int xz_run(mk_codec *c, const uint8_t *src, uint64_t n, const mkz::XzBlock *blocks, size_t B, const uint32_t *order, uint32_t lclp, uint8_t *d_text, float *ms) {
    double t0 = now_ms();
    const uint64_t n_words = (n + mkz::kXzStreamPad + 3) / 4;
    const uint64_t o_status = up16(B * sizeof(mkz::XzBlock)), o_check = o_status + up16(B * 4), o_order = o_check + up16(B * 4);
    const uint64_t tab_bytes = o_order + (order ? up16(B * 4) : 0);
    if (!mkz::ensure_quiet(&c->d_gz_in, &c->gz_in_cap, n_words * 4) || !mkz::ensure_quiet(&c->d_gz_tab, &c->gz_tab_cap, tab_bytes)) return mkz::kXzTooLarge;
    if (mkz::upload(c, c->d_gz_in, src, n)) {
        (void)hipGetLastError();
        return mkz::kXzDevice;
    }
    MKZ_HIP(hipMemsetAsync((uint8_t *)c->d_gz_in + n, 0, n_words * 4 - n, c->stream), mkz::kXzDevice);
    uint8_t *tab = (uint8_t *)c->d_gz_tab;
    MKZ_HIP(hipMemcpyAsync(tab, blocks, B * sizeof(mkz::XzBlock), hipMemcpyHostToDevice, c->stream), mkz::kXzDevice);
    if (order) MKZ_HIP(hipMemcpyAsync(tab + o_order, order, B * 4, hipMemcpyHostToDevice, c->stream), mkz::kXzDevice);
    MKZ_HIP(hipStreamSynchronize(c->stream), mkz::kXzDevice);
    ms[0] += (float)(now_ms() - t0);
    int32_t *d_status = (int32_t *)(tab + o_status), *d_check = (int32_t *)(tab + o_check);
    const uint32_t *d_order = order ? (const uint32_t *)(tab + o_order) : nullptr;
    MKZ_HIP(hipEventRecord(c->ev[0], c->stream), mkz::kXzDevice);
    mkz::launch_xz_decode((const uint8_t *)c->d_gz_in, n_words, tab, d_order, (uint32_t)B, d_text, lclp, d_status, c->stream);
    MKZ_HIP(hipGetLastError(), mkz::kXzDevice);
    MKZ_HIP(hipEventRecord(c->ev[1], c->stream), mkz::kXzDevice);
    mkz::launch_xz_check((const uint8_t *)c->d_gz_in, tab, d_order, (uint32_t)B, d_text, d_status, d_check, c->stream);
    MKZ_HIP(hipGetLastError(), mkz::kXzDevice);
    MKZ_HIP(hipEventRecord(c->ev[2], c->stream), mkz::kXzDevice);
    std::vector<int32_t> status(2 * B);
    MKZ_HIP(hipMemcpyAsync(status.data(), d_status, B * 4, hipMemcpyDeviceToHost, c->stream), mkz::kXzDevice);
    MKZ_HIP(hipMemcpyAsync(status.data() + B, d_check, B * 4, hipMemcpyDeviceToHost, c->stream), mkz::kXzDevice);
    MKZ_HIP(hipStreamSynchronize(c->stream), mkz::kXzDevice);
    ms[1] += elapsed(c->ev[0], c->ev[1]), ms[2] += elapsed(c->ev[1], c->ev[2]);
    for (size_t k = 0; k < B; ++k) {  // the first block that failed
        if (status[k] != 0) return status[k];
        if (status[B + k] != 0) return status[B + k];
    }
    return 0;
}
uint64_t xz_run_bytes(uint64_t n, size_t B, bool order) { return (n + mkz::kXzStreamPad + 3) / 4 * 4 + up16(B * sizeof(mkz::XzBlock)) + (order ? 3 : 2) * up16(B * 4); }

// the whole file in one call; 0: taken, else the refusal (xz_plan.hpp, lzma_serial.hpp)
int xz_inflate(mk_codec *c, const uint8_t *xz, uint64_t n, uint64_t *text_bytes, uint64_t *n_blocks) {
    double t_all = now_ms();
    mkz::XzPlan P;
    const int planned = mkz::xz_plan(xz, n, P);
    if (planned) return planned;
    c->xz_streams = P.streams, c->xz_largest = P.largest_block_text;
    const size_t B = P.blocks.size();
    if (!mkz::xz_spread_ok(P, c->xz_spread ? c->xz_spread : mkz::kXzSpreadDefault)) return mkz::kXzSpread;
    if (B) {
        MKZ_HIP(hipSetDevice(c->device), mkz::kXzDevice);
        size_t free_b = 0, total_b = 0;
        MKZ_HIP(hipMemGetInfo(&free_b, &total_b), mkz::kXzDevice);
        if (P.text_total > free_b / 2) return mkz::kXzTooLarge;  // (the text alone, whatever is held: not mkz::room, which credits what is held)
        if (!mkz::room(xz_run_bytes(n, B, false) + P.text_total + 128, c->gz_in_cap + c->gz_tab_cap + c->gz_text_cap, free_b)) return mkz::kXzTooLarge;
        if (!mkz::ensure_quiet(&c->d_gz_text, &c->gz_text_cap, P.text_total + 128)) return mkz::kXzTooLarge;
        const int st = xz_run(c, xz, n, P.blocks.data(), B, nullptr, P.lclp_max, (uint8_t *)c->d_gz_text, c->xz_ms);
        if (st) return st;
    }
    c->gz_text_bytes = P.text_total, c->xz_blocks = (uint32_t)B;
    c->xz_ms[3] = (float)(now_ms() - t_all);
    *text_bytes = P.text_total, *n_blocks = B;
    return 0;
}

// ---- the device behind a stream (xz_chain.hpp: Dev)
struct XzStreamDev {
    mk_codec *c;
    mk_xz_stream &D;
    int decode(const mkz::XzWork &K) {
        const size_t B = K.blocks.size();
        size_t free_b = 0, total_b = 0;
        MKZ_HIP(hipMemGetInfo(&free_b, &total_b), mkz::kXzDevice);
        if (!mkz::room(xz_run_bytes(K.bytes, B, true) + K.text + 128, c->gz_in_cap + c->gz_tab_cap + D.text.cap[D.text.other()], free_b)) return mkz::kXzTooLarge;
        if (!D.text.ensure_other(K.text + 128)) return mkz::kXzTooLarge;
        return xz_run(c, D.s.xz + K.from, K.bytes, K.blocks.data(), B, K.order.data(), K.lclp, D.text.other_text(), D.s.stats.ms);
    }
    void commit(uint64_t) { D.text.flip(c); }
};

// Two text buffers of T beside the largest window's upload and tables in half of what is free: T = a sixth of the free memory (xz
// text is seldom smaller than its compressed bytes, so the upload takes at most about a third of that half; the plan is checked
// against the half itself at _begin).  An unmeasured choice (profiles/e2e_unxz_windows.txt)
uint64_t xz_default_text_cap(uint64_t free_b) { return std::max<uint64_t>(free_b / 6, 1u << 20); }

}  // namespace

extern "C" {

int mk_xz_inflate_device(mk_codec *c, const uint8_t *xz, uint64_t n, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_blocks) {
    MK_ABI_BEGIN
    if (!c || !text_bytes || !taken || !n_blocks || (n && !xz)) return mk::fail(MK_E_INVALID_ARG, "mk_xz_inflate_device: NULL argument");
    *text_bytes = 0, *taken = 0, *n_blocks = 0;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->stream_open()) return mkz::refuse_open_stream("mk_xz_inflate_device");
    c->gz_text_bytes = 0, c->xz_blocks = c->xz_streams = 0, c->xz_status = 0, c->xz_largest = 0;
    for (float &x : c->xz_ms) x = 0;
    // (whatever keeps the file from being taken -- anything the walk, a block or a check refuses, the spread rule, no room, a device
    // error -- is MK_OK with *taken = 0 and a named status: the file is liblzma's)
    uint64_t text = 0, blocks = 0;
    c->xz_status = xz_inflate(c, xz, n, &text, &blocks);
    if (c->xz_status == 0) *text_bytes = text, *n_blocks = blocks, *taken = 1;
    else c->gz_text_bytes = 0;
    // what is left to keep is the text: the file and the tables go back to the device now
    mkz::gz_keep_text(c);
    return MK_OK;
    MK_ABI_END
}

int mk_xz_info(const mk_codec *c, uint32_t *blocks, uint32_t *streams, uint32_t *status, uint64_t *largest_block_text, float ms[4]) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_xz_info: NULL handle");
    if (blocks) *blocks = c->xz_blocks;
    if (streams) *streams = c->xz_streams;
    if (status) *status = (uint32_t)c->xz_status;
    if (largest_block_text) *largest_block_text = c->xz_largest;
    if (ms)
        for (int k = 0; k < 4; ++k) ms[k] = c->xz_ms[k];
    return MK_OK;
}

// ---- an .xz file of any size, window by window

int mk_xz_stream_begin(mk_codec *c, const uint8_t *xz, uint64_t n, uint64_t window_bytes, uint32_t *taken) {
    MK_ABI_BEGIN
    if (!c || !taken || (n && !xz)) return mk::fail(MK_E_INVALID_ARG, "mk_xz_stream_begin: NULL argument");
    *taken = 0;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->stream_open()) return mkz::refuse_open_stream("mk_xz_stream_begin");
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    // (whatever keeps the stream from opening is MK_OK with *taken = 0 and a named status in mk_xz_stream_info: the file is liblzma's)
    c->xzs = mk_xz_stream();
    mkz::XzStream &S = c->xzs.s;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
        (void)hipGetLastError();
        S.stats.status = mkz::kXzDevice;
        return MK_OK;
    }
    const uint64_t held = c->gz_in_cap + c->gz_tab_cap + c->gz_text_cap + c->gz_sym_cap + c->gz_ctx_cap;  // (released below, when the stream opens)
    const uint64_t T = c->xz_text_cap ? c->xz_text_cap : xz_default_text_cap(free_b + held);
    if (mkz::xz_stream_open(S, xz, n, window_bytes, T, c->xz_spread ? c->xz_spread : mkz::kXzSpreadDefault)) return MK_OK;
    uint64_t text = 0, upload = 0, blocks = 0;
    mkz::xz_stream_needs(S, &text, &upload, &blocks);
    if (2 * (text + 128) + xz_run_bytes(upload, blocks, true) > (free_b + held) / 2) {  // (what is held goes back first: it counts as free, not as had)
        S.stats.status = mkz::kXzTooLarge;
        return MK_OK;
    }
    mkz::gz_release(c);  // the one-shot text of an earlier call goes: d_gz_text is the stream's from here on
    c->xz_blocks = c->xz_streams = 0, c->xz_status = 0, c->xz_largest = 0;
    c->xzs.active = true;
    *taken = 1;
    return MK_OK;
    MK_ABI_END
}

int mk_xz_stream_next(mk_codec *c, uint64_t *text_bytes, uint32_t *state) {
    return mkz::chain_stream_next(
        c, &mk_codec::xzs, text_bytes, state,
        [&](mk_xz_stream &D) {
            XzStreamDev dev{c, D};
            const double t0 = now_ms();
            mkz::xz_stream_next(D.s, dev, text_bytes, state);
            D.s.stats.ms[3] += (float)(now_ms() - t0);
        },
        [](mk_xz_stream &D) { D.s.stats.status = mkz::kXzDevice; });
}

int mk_xz_stream_info(const mk_codec *c, mk_xz_stream_stats *out) { return mkz::stream_info(c, &mk_codec::xzs, out); }

int mk_xz_stream_end(mk_codec *c) { return mkz::stream_end(c, &mk_codec::xzs); }

int mk_codec_set_xz_spread(mk_codec *c, uint32_t spread) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_codec_set_xz_spread: NULL handle");
    std::lock_guard<std::mutex> lock(c->mu);
    c->xz_spread = spread;
    return MK_OK;
}

}  // extern "C"
