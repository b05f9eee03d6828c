// xz_host.cpp -- host side of mk_xz_inflate_device (include/merkurio_hip.h): an .xz file decoded on the device, a wave per block, the
// whole file in one call.  The walk over streams, Index records and Block Headers is mkz::xz_plan (xz_plan.hpp, no HIP in it: the CPU
// harness of the tests runs it); kernels: xz_inflate.hip.  Here: the spread rule, the upload of the file and of the block table, the
// decode launch, the check launch, and the per-block statuses: the first block that failed names why the file is handed back.  The
// buffers are the gzip path's (codec_internal.h).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../host_common.h"
#include "codec_internal.h"
#include "codec_kernels.h"
#include "lzma_serial.hpp"
#include "xz_plan.hpp"

using mkz::elapsed;
using mkz::now_ms;

namespace {

// a device error on this path hands the file back (*taken stays 0), it is not the caller's error.  NOTE: the macro RETURNS from the
// function that uses it, behind a wait for the stream: a copy may still be on its way into a vector of that function
#define MKXZ_HIP(call)                              \
    do {                                            \
        if ((call) != hipSuccess) {                 \
            (void)hipGetLastError();                \
            (void)hipStreamSynchronize(c->stream);  \
            (void)hipGetLastError();                \
            return mkz::kXzDevice;                  \
        }                                           \
    } while (0)

bool xz_ensure(void **p, size_t *cap, size_t need) {
    if (mk::ensure_device(p, cap, need) == MK_OK) return true;
    (void)hipGetLastError();
    return false;
}
uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

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
        MKXZ_HIP(hipSetDevice(c->device));
        size_t free_b = 0, total_b = 0;
        MKXZ_HIP(hipMemGetInfo(&free_b, &total_b));
        if (P.text_total > free_b / 2) return mkz::kXzTooLarge;
        // ---- upload: the file (zeros behind it up to the reader's pad) and the block table; behind the table: status, check
        double t0 = now_ms();
        const uint64_t n_words = (n + mkz::kXzStreamPad + 3) / 4;
        const uint64_t o_status = up16(B * sizeof(mkz::XzBlock)), o_check = o_status + up16(B * 4), tab_bytes = o_check + up16(B * 4);
        const uint64_t need = n_words * 4 + tab_bytes + P.text_total + 128, held = c->gz_in_cap + c->gz_tab_cap + c->gz_text_cap;
        if (need > held && need - held > free_b / 2) return mkz::kXzTooLarge;
        if (!xz_ensure(&c->d_gz_in, &c->gz_in_cap, n_words * 4) || !xz_ensure(&c->d_gz_tab, &c->gz_tab_cap, tab_bytes) ||
            !xz_ensure(&c->d_gz_text, &c->gz_text_cap, P.text_total + 128))
            return mkz::kXzTooLarge;
        if (mkz::upload(c, c->d_gz_in, xz, n)) {
            (void)hipGetLastError();
            return mkz::kXzDevice;
        }
        MKXZ_HIP(hipMemsetAsync((uint8_t *)c->d_gz_in + n, 0, n_words * 4 - n, c->stream));
        uint8_t *tab = (uint8_t *)c->d_gz_tab;
        MKXZ_HIP(hipMemcpyAsync(tab, P.blocks.data(), B * sizeof(mkz::XzBlock), hipMemcpyHostToDevice, c->stream));
        MKXZ_HIP(hipStreamSynchronize(c->stream));
        c->xz_ms[0] = (float)(now_ms() - t0);
        // ---- decode, a wave per block; then the checks
        int32_t *d_status = (int32_t *)(tab + o_status), *d_check = (int32_t *)(tab + o_check);
        MKXZ_HIP(hipEventRecord(c->ev[0], c->stream));
        mkz::launch_xz_decode((const uint8_t *)c->d_gz_in, n_words, tab, (uint32_t)B, (uint8_t *)c->d_gz_text, P.lclp_max, d_status, c->stream);
        MKXZ_HIP(hipGetLastError());
        MKXZ_HIP(hipEventRecord(c->ev[1], c->stream));
        mkz::launch_xz_check((const uint8_t *)c->d_gz_in, tab, (uint32_t)B, (const uint8_t *)c->d_gz_text, d_status, d_check, c->stream);
        MKXZ_HIP(hipGetLastError());
        MKXZ_HIP(hipEventRecord(c->ev[2], c->stream));
        std::vector<int32_t> status(2 * B);
        MKXZ_HIP(hipMemcpyAsync(status.data(), d_status, B * 4, hipMemcpyDeviceToHost, c->stream));
        MKXZ_HIP(hipMemcpyAsync(status.data() + B, d_check, B * 4, hipMemcpyDeviceToHost, c->stream));
        MKXZ_HIP(hipStreamSynchronize(c->stream));
        c->xz_ms[1] = elapsed(c->ev[0], c->ev[1]), c->xz_ms[2] = elapsed(c->ev[1], c->ev[2]);
        for (size_t k = 0; k < B; ++k) {  // the first block that failed
            if (status[k] != 0) return status[k];
            if (status[B + k] != 0) return status[B + k];
        }
    }
    c->gz_text_bytes = P.text_total, c->xz_blocks = (uint32_t)B;
    c->xz_ms[3] = (float)(now_ms() - t_all);
    *text_bytes = P.text_total, *n_blocks = B;
    return 0;
}

}  // namespace

extern "C" {

int mk_xz_inflate_device(mk_codec *c, const uint8_t *xz, uint64_t n, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_blocks) {
    MK_ABI_BEGIN
    if (!c || !text_bytes || !taken || !n_blocks || (n && !xz)) return mk::fail(MK_E_INVALID_ARG, "mk_xz_inflate_device: NULL argument");
    *text_bytes = 0, *taken = 0, *n_blocks = 0;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->stream_open()) return mk::fail(MK_E_INVALID_ARG, "mk_xz_inflate_device: the handle has an open stream (mk_gzip_stream_end, mk_bzip2_stream_end, mk_zstd_stream_end)");
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

int mk_codec_set_xz_spread(mk_codec *c, uint32_t spread) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_codec_set_xz_spread: NULL handle");
    std::lock_guard<std::mutex> lock(c->mu);
    c->xz_spread = spread;
    return MK_OK;
}

}  // extern "C"
