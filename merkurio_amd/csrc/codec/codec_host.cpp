// codec_host.cpp -- the mk_codec handle of the C ABI's device codec (include/merkurio_hip.h): create / destroy, the setters, the
// times, and the staging copies that move the callers' host buffers.  A format per file beside it: bgzf_host.cpp, gzip_host.cpp,
// bzip2_host.cpp (codec_internal.h says what they share).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <mutex>
#include <thread>
#include <vector>

#include "../host_common.h"
#include "codec_stream.hpp"

namespace {

// ---- host buffers <-> device through the handle's two page-locked staging buffers (r05) -------------------------------------
// A caller's plain (pageable) buffer cannot be a DMA source or target: the runtime stages it through a bounce buffer on ONE thread,
// and a freshly allocated output buffer additionally takes a page fault per 4 KiB inside that copy -- mk_bgzf_inflate of 1 GB spent
// 335 of its 376 ms there (kernels 41 ms; tools/codec_real.py before this change).  Here the host threads copy piece k + 1 into /
// out of one staging buffer (first touch of the caller's pages included, on all of them) while the DMA engine moves piece k through
// the other.  Buffers that are page-locked already (mk_host_alloc) and small ones go the direct way.
constexpr uint64_t kStageBytes = 32ull << 20, kStageFrom = 4ull << 20;

unsigned copy_threads() {
    const unsigned hc = std::thread::hardware_concurrency();
    return std::max(1u, std::min(16u, hc ? hc : 4u));
}

bool is_page_locked(const void *p) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // (an ordinary malloc'ed pointer is "invalid value" to this query: not an error of ours)
        return false;
    }
    return a.type == hipMemoryTypeHost;
}
int stage_buffers(mk_codec *c) {
    for (int k = 0; k < 2; ++k) {
        if (!c->h_stage[k]) MKC_HIP(hipHostMalloc(&c->h_stage[k], kStageBytes, hipHostMallocDefault), "hipHostMalloc of a staging buffer");
        if (!c->ev_stage[k]) MKC_HIP(hipEventCreateWithFlags(&c->ev_stage[k], hipEventDisableTiming), "hipEventCreate");
    }
    return MK_OK;
}

}  // namespace

namespace mkz {

void parallel_copy(uint8_t *dst, const uint8_t *src, uint64_t n) {
    const unsigned T = (unsigned)std::min<uint64_t>(copy_threads(), n / (1u << 20) + 1);
    if (T <= 1) {
        memcpy(dst, src, n);
        return;
    }
    std::vector<std::thread> th;
    for (unsigned t = 1; t < T; ++t) th.emplace_back([=] { memcpy(dst + n * t / T, src + n * t / T, (size_t)(n * (t + 1) / T - n * t / T)); });
    memcpy(dst, src, (size_t)(n / T));
    for (auto &x : th) x.join();
}
// src[0, n) -> d_dst, enqueued on the handle's stream; the host side of it is done when this returns
int upload(mk_codec *c, void *d_dst, const uint8_t *src, uint64_t n) {
    if (n < kStageFrom || is_page_locked(src)) {
        MKC_HIP(hipMemcpyAsync(d_dst, src, n, hipMemcpyHostToDevice, c->stream), "upload");
        return MK_OK;
    }
    int rc = stage_buffers(c);
    if (rc) return rc;
    int k = 0;
    for (uint64_t at = 0; at < n; at += kStageBytes, k ^= 1) {
        const uint64_t m = std::min<uint64_t>(kStageBytes, n - at);
        if (at >= 2 * kStageBytes) MKC_HIP(hipEventSynchronize(c->ev_stage[k]), "hipEventSynchronize");  // its previous piece has left
        parallel_copy((uint8_t *)c->h_stage[k], src + at, m);
        MKC_HIP(hipMemcpyAsync((uint8_t *)d_dst + at, c->h_stage[k], m, hipMemcpyHostToDevice, c->stream), "upload");
        MKC_HIP(hipEventRecord(c->ev_stage[k], c->stream), "hipEventRecord");
    }
    // the staging buffers are reused by the next transfer of the call: wait until both have been read
    MKC_HIP(hipEventSynchronize(c->ev_stage[0]), "hipEventSynchronize");
    MKC_HIP(hipEventSynchronize(c->ev_stage[1]), "hipEventSynchronize");
    return MK_OK;
}
// d_src[0, n) -> dst; waits for the stream (everything enqueued before it included)
int download(mk_codec *c, uint8_t *dst, const void *d_src, uint64_t n) {
    if (n < kStageFrom || is_page_locked(dst)) {
        if (n) MKC_HIP(hipMemcpyAsync(dst, d_src, n, hipMemcpyDeviceToHost, c->stream), "download");
        MKC_HIP(hipStreamSynchronize(c->stream), "download");
        return MK_OK;
    }
    int rc = stage_buffers(c);
    if (rc) return rc;
    // piece j travels into buffer j & 1 while the host threads copy piece j - 1 out of the other
    const uint64_t pieces = (n + kStageBytes - 1) / kStageBytes;
    for (uint64_t j = 0; j <= pieces; ++j) {
        if (j < pieces) {
            const uint64_t at = j * kStageBytes, m = std::min<uint64_t>(kStageBytes, n - at);
            MKC_HIP(hipMemcpyAsync(c->h_stage[j & 1], (const uint8_t *)d_src + at, m, hipMemcpyDeviceToHost, c->stream), "download");
            MKC_HIP(hipEventRecord(c->ev_stage[j & 1], c->stream), "hipEventRecord");
        }
        if (j > 0) {
            const uint64_t at = (j - 1) * kStageBytes, m = std::min<uint64_t>(kStageBytes, n - at);
            MKC_HIP(hipEventSynchronize(c->ev_stage[(j - 1) & 1]), "hipEventSynchronize");
            parallel_copy(dst + at, (const uint8_t *)c->h_stage[(j - 1) & 1], m);
        }
    }
    return MK_OK;
}
int download_each(mk_codec *c, const void *d_src, uint64_t n, const std::function<void(const uint8_t *, uint64_t)> &each) {
    int rc = stage_buffers(c);
    if (rc) return rc;
    const uint64_t pieces = (n + kStageBytes - 1) / kStageBytes;
    for (uint64_t j = 0; j <= pieces; ++j) {
        if (j < pieces) {
            const uint64_t at = j * kStageBytes, m = std::min<uint64_t>(kStageBytes, n - at);
            MKC_HIP(hipMemcpyAsync(c->h_stage[j & 1], (const uint8_t *)d_src + at, m, hipMemcpyDeviceToHost, c->stream), "download");
            MKC_HIP(hipEventRecord(c->ev_stage[j & 1], c->stream), "hipEventRecord");
        }
        if (j > 0) {
            MKC_HIP(hipEventSynchronize(c->ev_stage[(j - 1) & 1]), "hipEventSynchronize");
            each((const uint8_t *)c->h_stage[(j - 1) & 1], std::min<uint64_t>(kStageBytes, n - (j - 1) * kStageBytes));
        }
    }
    return MK_OK;
}
double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
// (the one place that names the streams a handle may hold, beside mk_codec::stream_open)
void streams_close(mk_codec *c) {
    stream_close(c, c->gzs);
    stream_close(c, c->bzs);
    stream_close(c, c->zss);
    stream_close(c, c->xzs);
}

}  // namespace mkz

extern "C" {

int mk_codec_cut_times(const mk_codec *c, uint64_t *n_members, float ms[3]) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_codec_cut_times: NULL handle");
    if (n_members) *n_members = c->cut_members;
    if (ms)
        for (int k = 0; k < 3; ++k) ms[k] = c->cut_ms[k];
    return MK_OK;
}

int mk_codec_create(int device, mk_codec **out) {
    MK_ABI_BEGIN
    if (!out) return mk::fail(MK_E_INVALID_ARG, "mk_codec_create: out is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return mk::fail(MK_E_HIP, "no HIP device (the BGZF codec has no CPU path)");
    if (device < 0 || device >= n) return mk::fail(MK_E_INVALID_ARG, "mk_codec_create: device %d of %d", device, n);
    MKC_HIP(hipSetDevice(device), "hipSetDevice");
    mk_codec *c = new mk_codec;
    c->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) c->num_cus = prop.multiProcessorCount;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    for (int k = 0; k < 4 && e == hipSuccess; ++k) e = hipEventCreate(&c->ev[k]);
    if (e != hipSuccess) {
        mk_codec_destroy(c);
        return mk::hip_fail(e, "mk_codec_create");
    }
    *out = c;
    return MK_OK;
    MK_ABI_END
}

void mk_codec_destroy(mk_codec *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    mkz::streams_close(c);  // (an open stream's text buffers are what d_gz_text points at)
    for (void *p : {c->d_in, c->d_crc, c->d_tokens, c->d_slots, c->d_len, c->d_off, c->d_out, c->d_aux, c->d_ends, c->d_cut, c->d_gz_in, c->d_gz_sym, c->d_gz_tab, c->d_gz_ctx, c->d_gz_text})
        if (p) (void)hipFree(p);
    for (hipEvent_t e : c->ev)
        if (e) (void)hipEventDestroy(e);
    for (int k = 0; k < 2; ++k) {
        if (c->h_stage[k]) (void)hipHostFree(c->h_stage[k]);
        if (c->ev_stage[k]) (void)hipEventDestroy(c->ev_stage[k]);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int mk_codec_set_pass_limits(mk_codec *c, uint64_t deflate_members, uint64_t inflate_text_bytes) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_codec_set_pass_limits: NULL handle");
    std::lock_guard<std::mutex> lock(c->mu);
    c->deflate_pass_blocks = deflate_members;
    c->inflate_pass_text = inflate_text_bytes;
    return MK_OK;
}

int mk_codec_set_gzip_chunk(mk_codec *c, uint64_t chunk_bytes) {
    if (!c || (chunk_bytes && (chunk_bytes < 4096 || chunk_bytes > (1u << 20) || (chunk_bytes & (chunk_bytes - 1)))))
        return mk::fail(MK_E_INVALID_ARG, "mk_codec_set_gzip_chunk: handle / a power of two of 4 KiB ... 1 MiB");
    std::lock_guard<std::mutex> lock(c->mu);
    c->gzip_chunk = chunk_bytes;
    return MK_OK;
}
int mk_codec_set_inflate_kernel(mk_codec *c, int which) {
    if (!c || which < 0 || which > 6) return mk::fail(MK_E_INVALID_ARG, "mk_codec_set_inflate_kernel: handle / selector");
    std::lock_guard<std::mutex> lock(c->mu);
    c->inflate_kernel = which;
    return MK_OK;
}

int mk_codec_times(const mk_codec *c, float ms[3]) {
    if (!c || !ms) return mk::fail(MK_E_INVALID_ARG, "mk_codec_times: NULL argument");
    for (int k = 0; k < 3; ++k) ms[k] = c->ms[k];
    return MK_OK;
}

int mk_codec_set_bzip2_pass_blocks(mk_codec *c, uint64_t blocks) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_codec_set_bzip2_pass_blocks: NULL handle");
    std::lock_guard<std::mutex> lock(c->mu);
    c->bz_pass_blocks = blocks;
    return MK_OK;
}

int mk_codec_set_bzip2_text_cap(mk_codec *c, uint64_t text_bytes) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_codec_set_bzip2_text_cap: NULL handle");
    std::lock_guard<std::mutex> lock(c->mu);
    c->bz_text_cap = text_bytes;
    return MK_OK;
}

int mk_codec_set_zstd_text_cap(mk_codec *c, uint64_t text_bytes) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_codec_set_zstd_text_cap: NULL handle");
    std::lock_guard<std::mutex> lock(c->mu);
    c->zs_text_cap = text_bytes;
    return MK_OK;
}

int mk_codec_set_xz_text_cap(mk_codec *c, uint64_t text_bytes) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_codec_set_xz_text_cap: NULL handle");
    std::lock_guard<std::mutex> lock(c->mu);
    c->xz_text_cap = text_bytes;
    return MK_OK;
}

}  // extern "C"
