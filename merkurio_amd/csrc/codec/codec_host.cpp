// codec_host.cpp -- host side of the C ABI's BGZF codec (include/merkurio_hip.h, v5): the mk_codec handle, its device
// buffers, chunking of a call into device-sized pieces, the BSIZE walk.  Kernels: bgzf_deflate.hip, bgzf_inflate.hip.
// Reference interface replaced: the BGZF reader / writer of `bam 0.1.4` as `merkurio tag` drives it
// (src/cmd_tag.rs:254-271 `BamWriter::build().write_header(..).from_path`, :503-506 `BamReader::from_path(.., threads)`)
// and needletail's gzip reader on bgzip'ed inputs (src/cmd_extract.rs:281).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <iterator>
#include <mutex>
#include <thread>
#include <vector>

#include "../host_common.h"
#include "bgzf_cuts.hpp"
#include "bzip2_stream.hpp"
#include "codec_internal.h"
#include "codec_kernels.h"
#include "gzip_segments.hpp"

namespace mk {
int hip_fail(hipError_t e, const char *what);
int ensure_device(void **p, size_t *cap, size_t need);
}  // namespace mk

namespace {

// Members per device pass (mk_codec_set_pass_limits overrides).  Deflate deals its members from a counter to a resident
// grid of 16 waves per CU, so a pass only has to be large: 49 152 members = 3.2 GB of text (its 64 KiB slot per member is
// what bounds it).  Inflate is bound by the latency of its slowest lane, 25-60 ms per launch whatever it holds
// (profiles/r04_codec_kernels.txt): a pass takes as many members as the part holds streams, 3 GiB of text.
constexpr uint64_t kDeflateChunkBlocks = 49152;
constexpr uint64_t kInflateChunkText = 3ull << 30;

#define MKC_HIP(call, what)                                   \
    do {                                                      \
        const hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return mk::hip_fail(e_, what);  \
    } while (0)

float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
}

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
double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void gzip_stream_close(mk_codec *c);  // (below, with the stream)

const uint8_t kEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

}  // namespace

namespace mkz {

int deflate_pass(mk_codec *c, hipStream_t st, const uint8_t *d_text, uint64_t n_text, uint32_t bb, const unsigned long long *off, const uint32_t *len,
                 uint32_t blocks, void *d_packed, size_t packed_cap, void **d_members, uint64_t *total) {
    int rc;
    const uint32_t grid = deflate_grid(blocks, c->num_cus);
    if ((rc = mk::ensure_device(&c->d_crc, &c->crc_cap, blocks * 4ull)) || (rc = mk::ensure_device(&c->d_tokens, &c->tokens_cap, (uint64_t)grid * kTokensPerWave * 4)) ||
        (rc = mk::ensure_device(&c->d_slots, &c->slots_cap, (uint64_t)blocks * kSlotBytes)) || (rc = mk::ensure_device(&c->d_len, &c->len_cap, (blocks + 1) * 4ull)) ||
        (rc = mk::ensure_device(&c->d_off, &c->off_cap, (blocks + 2) * 8ull)))
        return rc;
    // (a stored member: its text + 31 bytes)
    const uint64_t bound = off ? std::min<uint64_t>((uint64_t)blocks * kMaxBlockBytes, n_text) + blocks * 31ull : mk_bgzf_deflate_bound(n_text, bb);
    if (packed_cap < bound) {
        if ((rc = mk::ensure_device(&c->d_out, &c->out_cap, bound))) return rc;
        d_packed = c->d_out;
    }
    uint64_t *d_total = (uint64_t *)c->d_off + blocks;
    if (off) {
        launch_crc_ranges(d_text, off, len, blocks, (uint32_t *)c->d_crc, st);
        launch_deflate_ranges(d_text, off, len, blocks, (const uint32_t *)c->d_crc, (uint32_t *)c->d_tokens, (uint8_t *)c->d_slots, (uint32_t *)c->d_len,
                              (uint32_t *)(d_total + 1), grid, st);
    } else {
        launch_crc(d_text, n_text, bb, blocks, (uint32_t *)c->d_crc, st);
        launch_deflate(d_text, n_text, bb, blocks, (const uint32_t *)c->d_crc, (uint32_t *)c->d_tokens, (uint8_t *)c->d_slots, (uint32_t *)c->d_len,
                       (uint32_t *)(d_total + 1), grid, st);
    }
    launch_pack((const uint8_t *)c->d_slots, (const uint32_t *)c->d_len, (uint64_t *)c->d_off, d_total, blocks, (uint8_t *)d_packed, st);
    *total = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(total, d_total, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return mk::fail(MK_E_HIP, "BGZF deflate on the device failed");
    *d_members = d_packed;
    return MK_OK;
}

// d_text[0, n_text) (kPad readable bytes behind it) whose records end at d_ends[0, n_ends) (device memory, non-decreasing, the last
// one = n_text) -> BGZF members that end at record ends (the cut rule of include/merkurio_hip.h), in passes of members
// (mk_codec_set_pass_limits).  *need = the bytes of all members, *n_members how many.  A pass's members are downloaded to out as long
// as everything so far has fitted out_cap: *need > out_cap means out holds only the passes in front of the one that did not fit (the
// caller reports MK_E_CAPACITY).  c->cut_ms: cut, deflate, download.  d_packed / packed_cap: as deflate_pass.  (Shared with
// mk_extract_window_members, extract_window.cpp: the ends are then the offsets scan of a window's written lengths.)
int deflate_ranges(mk_codec *c, hipStream_t st, const uint8_t *d_text, uint64_t n_text, const unsigned long long *d_ends, uint64_t n_ends, void *d_packed,
                   size_t packed_cap, uint8_t *out, uint64_t out_cap, uint64_t *need, uint64_t *n_members) {
    *need = 0, *n_members = 0;
    c->cut_ms[0] = c->cut_ms[1] = c->cut_ms[2] = 0, c->cut_members = 0;
    if (!n_text) return MK_OK;
    const uint64_t grid64 = (n_text + kCutGrid - 1) / kCutGrid;
    if (grid64 >= 0xFFFFFFFFull) return mk::fail(MK_E_UNSUPPORTED, "%llu output members", (unsigned long long)grid64);
    const uint32_t n_grid = (uint32_t)grid64;
    int rc;
    // the range table: count | off[n_grid] | len[n_grid]
    if ((rc = mk::ensure_device(&c->d_cut, &c->cut_cap, 16 + n_grid * 12ull))) return rc;
    uint32_t *d_count = (uint32_t *)c->d_cut;
    unsigned long long *d_off = (unsigned long long *)((uint8_t *)c->d_cut + 16);
    uint32_t *d_len = (uint32_t *)(d_off + n_grid);
    double t0 = now_ms();
    launch_cuts(d_ends, n_ends, n_text, n_grid, d_off, d_len, d_count, st);
    uint32_t members = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&members, d_count, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return mk::fail(MK_E_HIP, "the cut kernel failed");
    if (members > n_grid || members + 1 < n_grid) return mk::fail(MK_E_HIP, "the cut kernel reports %u members of %u grid points", members, n_grid);
    c->cut_ms[0] = (float)(now_ms() - t0);
    // passes of members; a pass's members are downloaded as long as everything so far has fitted
    const uint64_t pass = std::min<uint64_t>(c->deflate_pass_blocks ? c->deflate_pass_blocks : kDeflateChunkBlocks, 0x7FFFFFFFu);
    uint64_t written = 0;
    bool fits = true;
    for (uint64_t m0 = 0; m0 < members; m0 += pass) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(pass, members - m0);
        void *d_members = nullptr;
        uint64_t total = 0;
        t0 = now_ms();
        if ((rc = deflate_pass(c, st, d_text, n_text, 0, d_off + m0, d_len + m0, cnt, d_packed, packed_cap, &d_members, &total))) return rc;
        c->cut_ms[1] += (float)(now_ms() - t0);
        fits = fits && written + total <= out_cap;
        if (fits && total) {
            t0 = now_ms();
            if (hipMemcpyAsync(out + written, d_members, total, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
                return mk::fail(MK_E_HIP, "download of the members failed");
            c->cut_ms[2] += (float)(now_ms() - t0);
        }
        written += total;
    }
    *need = written, *n_members = members, c->cut_members = members;
    return MK_OK;
}

}  // namespace mkz

extern "C" {

int mk_bgzf_record_cuts(const uint64_t *rec_end, uint64_t n_rec, uint64_t *cut, uint64_t cap, uint64_t *n_cuts) {
    if (!n_cuts || (n_rec && !rec_end) || (cap && !cut)) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_record_cuts: NULL argument");
    *n_cuts = 0;
    for (uint64_t r = 1; r < n_rec; ++r)
        if (rec_end[r] < rec_end[r - 1]) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_record_cuts: record end %llu lies in front of the one before it", (unsigned long long)r);
    const uint64_t k = mkz::record_cuts(rec_end, n_rec, cut, cap);
    *n_cuts = k;
    if (k > cap) return mk::fail(MK_E_CAPACITY, "mk_bgzf_record_cuts: %llu cuts, room for %llu", (unsigned long long)k, (unsigned long long)cap);
    return MK_OK;
}

int mk_bgzf_deflate_records(mk_codec *c, const uint8_t *text, uint64_t n, const uint64_t *rec_end, uint64_t n_rec, uint8_t *out, uint64_t out_cap,
                            uint64_t *out_len, uint64_t *n_members) {
    MK_ABI_BEGIN
    if (!c || !out_len || !n_members || (n && (!text || !rec_end)) || (out_cap && !out)) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate_records: NULL argument");
    *out_len = 0, *n_members = 0;
    if ((n_rec ? rec_end[n_rec - 1] : 0) != n) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate_records: the last record does not end where the text does");
    for (uint64_t r = 1; r < n_rec; ++r)
        if (rec_end[r] < rec_end[r - 1]) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate_records: record end %llu lies in front of the one before it", (unsigned long long)r);
    std::lock_guard<std::mutex> lock(c->mu);
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    c->ms[0] = c->ms[1] = c->ms[2] = 0;
    if (!n) return MK_OK;
    int rc;
    if ((rc = mk::ensure_device(&c->d_in, &c->in_cap, n + mkz::kPad)) || (rc = mk::ensure_device(&c->d_ends, &c->ends_cap, n_rec * 8ull))) return rc;
    const double t_up = now_ms();
    if ((rc = upload(c, c->d_in, text, n)) || (rc = upload(c, c->d_ends, (const uint8_t *)rec_end, n_rec * 8ull))) return rc;
    MKC_HIP(hipMemsetAsync((uint8_t *)c->d_in + n, 0, mkz::kPad, c->stream), "hipMemsetAsync");
    MKC_HIP(hipStreamSynchronize(c->stream), "upload of the text");
    c->ms[0] = (float)(now_ms() - t_up);
    uint64_t need = 0;
    if ((rc = mkz::deflate_ranges(c, c->stream, (const uint8_t *)c->d_in, n, (const unsigned long long *)c->d_ends, n_rec, nullptr, 0, out, out_cap, &need, n_members)))
        return rc;
    c->ms[1] = c->cut_ms[0] + c->cut_ms[1], c->ms[2] = c->cut_ms[2];
    *out_len = need;
    if (need > out_cap) return mk::fail(MK_E_CAPACITY, "mk_bgzf_deflate_records: the members take %llu bytes, room for %llu", (unsigned long long)need, (unsigned long long)out_cap);
    return MK_OK;
    MK_ABI_END
}

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
    gzip_stream_close(c);  // (its text buffers are what d_gz_text points at)
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

uint64_t mk_bgzf_deflate_bound(uint64_t n, uint32_t block_bytes) {
    const uint64_t bb = block_bytes ? block_bytes : mkz::kMaxBlockBytes;
    const uint64_t blocks = (n + bb - 1) / bb;
    return n + blocks * 31;  // a stored member: 18 + 5 + text + 8
}

const uint8_t *mk_bgzf_eof(void) { return kEof; }

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

int mk_bgzf_deflate_pieces(mk_codec *c, const uint8_t *const *pieces, const uint64_t *sizes, uint64_t n_pieces, uint32_t block_bytes,
                           uint8_t *out, uint64_t out_cap, uint64_t *out_len) {
    MK_ABI_BEGIN
    if (!c || !out_len || (n_pieces && (!pieces || !sizes))) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate: NULL argument");
    uint64_t n = 0;
    for (uint64_t k = 0; k < n_pieces; ++k) {
        if (sizes[k] && !pieces[k]) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate: piece %llu is NULL", (unsigned long long)k);
        n += sizes[k];
    }
    if (n && !out) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate: NULL argument");
    const uint32_t bb = block_bytes ? block_bytes : mkz::kMaxBlockBytes;
    if (bb > mkz::kMaxBlockBytes) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate: block_bytes %u > %u", bb, mkz::kMaxBlockBytes);
    const uint64_t bound = mk_bgzf_deflate_bound(n, bb);
    *out_len = 0;
    if (out_cap < bound) {
        *out_len = bound;
        return mk::fail(MK_E_CAPACITY, "mk_bgzf_deflate: out_cap %llu < bound %llu", (unsigned long long)out_cap, (unsigned long long)bound);
    }
    std::lock_guard<std::mutex> lock(c->mu);
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    c->ms[0] = c->ms[1] = c->ms[2] = 0;
    const uint64_t chunk_bytes = (c->deflate_pass_blocks ? c->deflate_pass_blocks : kDeflateChunkBlocks) * bb;
    uint64_t written = 0;
    uint64_t piece = 0, piece_at = 0;  // where the text of the next device pass starts
    for (uint64_t at = 0; at < n; at += chunk_bytes) {
        const uint64_t cn = std::min<uint64_t>(chunk_bytes, n - at);
        const uint32_t blocks = (uint32_t)((cn + bb - 1) / bb);
        const uint32_t grid = mkz::deflate_grid(blocks, c->num_cus);
        int rc;
        if ((rc = mk::ensure_device(&c->d_in, &c->in_cap, cn + mkz::kPad)) || (rc = mk::ensure_device(&c->d_crc, &c->crc_cap, blocks * 4ull)) ||
            (rc = mk::ensure_device(&c->d_tokens, &c->tokens_cap, (uint64_t)grid * mkz::kTokensPerWave * 4)) ||
            (rc = mk::ensure_device(&c->d_slots, &c->slots_cap, (uint64_t)blocks * mkz::kSlotBytes)) ||
            (rc = mk::ensure_device(&c->d_len, &c->len_cap, blocks * 4ull)) || (rc = mk::ensure_device(&c->d_off, &c->off_cap, (blocks + 2) * 8ull)) ||
            (rc = mk::ensure_device(&c->d_out, &c->out_cap, mk_bgzf_deflate_bound(cn, bb))))
            return rc;
        uint64_t *d_total = (uint64_t *)c->d_off + blocks;
        const double t_up = now_ms();
        for (uint64_t done = 0; done < cn;) {  // the pieces land back to back: the concatenation exists on the device only
            while (piece_at == sizes[piece]) ++piece, piece_at = 0;
            const uint64_t k = std::min<uint64_t>(cn - done, sizes[piece] - piece_at);
            if ((rc = upload(c, (uint8_t *)c->d_in + done, pieces[piece] + piece_at, k))) return rc;
            done += k, piece_at += k;
        }
        MKC_HIP(hipMemsetAsync((uint8_t *)c->d_in + cn, 0, mkz::kPad, c->stream), "hipMemsetAsync");
        MKC_HIP(hipStreamSynchronize(c->stream), "upload of the text");
        c->ms[0] += (float)(now_ms() - t_up);
        MKC_HIP(hipEventRecord(c->ev[1], c->stream), "hipEventRecord");
        mkz::launch_crc((const uint8_t *)c->d_in, cn, bb, blocks, (uint32_t *)c->d_crc, c->stream);
        mkz::launch_deflate((const uint8_t *)c->d_in, cn, bb, blocks, (const uint32_t *)c->d_crc, (uint32_t *)c->d_tokens, (uint8_t *)c->d_slots,
                            (uint32_t *)c->d_len, (uint32_t *)(d_total + 1), grid, c->stream);
        mkz::launch_pack((const uint8_t *)c->d_slots, (const uint32_t *)c->d_len, (uint64_t *)c->d_off, d_total, blocks, (uint8_t *)c->d_out, c->stream);
        MKC_HIP(hipGetLastError(), "BGZF deflate kernels");
        MKC_HIP(hipEventRecord(c->ev[2], c->stream), "hipEventRecord");
        uint64_t total = 0;
        MKC_HIP(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, c->stream), "download of the size");
        MKC_HIP(hipStreamSynchronize(c->stream), "BGZF deflate");
        if (total > out_cap - written) return mk::fail(MK_E_CAPACITY, "mk_bgzf_deflate: members exceed the bound (internal error)");
        const double t_down = now_ms();
        if ((rc = download(c, out + written, c->d_out, total))) return rc;
        c->ms[1] += elapsed(c->ev[1], c->ev[2]), c->ms[2] += (float)(now_ms() - t_down);
        written += total;
    }
    *out_len = written;
    return MK_OK;
    MK_ABI_END
}

int mk_bgzf_deflate(mk_codec *c, const uint8_t *in, uint64_t n, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_len) {
    if (n && !in) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate: NULL argument");
    return mk_bgzf_deflate_pieces(c, &in, &n, n ? 1 : 0, block_bytes, out, out_cap, out_len);
}

int mk_bgzf_members(const uint8_t *in, uint64_t n, mk_bgzf_member *members, uint64_t cap, uint64_t *n_members, uint64_t *consumed,
                    uint64_t *text_bytes) {
    if (!n_members || (n && !in)) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_members: NULL argument");
    uint64_t at = 0, k = 0, text = 0;
    while (n - at >= 18) {
        const uint8_t *h = in + at;
        if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return mk::fail(MK_E_CORRUPT, "not a BGZF member at byte %llu", (unsigned long long)at);
        const uint32_t xlen = h[10] | (uint32_t)h[11] << 8;
        if (n - at < 12 + (uint64_t)xlen) break;
        uint32_t bsize = 0;
        bool found = false;
        for (uint32_t x = 0; x + 4 <= xlen;) {  // the extra field's subfields: SI1 SI2 SLEN data
            const uint8_t *f = h + 12 + x;
            const uint32_t slen = f[2] | (uint32_t)f[3] << 8;
            if (f[0] == 'B' && f[1] == 'C' && slen == 2 && x + 6 <= xlen) bsize = f[4] | (uint32_t)f[5] << 8, found = true;
            x += 4 + slen;
        }
        if (!found) return mk::fail(MK_E_CORRUPT, "gzip member without a BC subfield at byte %llu", (unsigned long long)at);
        const uint64_t size = (uint64_t)bsize + 1;
        if (size < 12 + (uint64_t)xlen + 8) return mk::fail(MK_E_CORRUPT, "BGZF member with BSIZE %u at byte %llu", bsize, (unsigned long long)at);
        if (n - at < size) break;
        uint32_t crc, isize;
        memcpy(&crc, h + size - 8, 4), memcpy(&isize, h + size - 4, 4);
        if (isize > 65536) return mk::fail(MK_E_CORRUPT, "BGZF member with ISIZE %u at byte %llu", isize, (unsigned long long)at);
        // RFC 1952's optional fields between the extra field and the DEFLATE stream (bgzip sets none of them, a gzip member
        // that carries a BC subfield may): FNAME / FCOMMENT are zero-terminated, FHCRC is two bytes; reserved bits refuse
        uint64_t skip = 12 + (uint64_t)xlen;
        if (h[3] & 0xE0) return mk::fail(MK_E_UNSUPPORTED, "gzip member with reserved FLG bits (0x%02x) at byte %llu", h[3], (unsigned long long)at);
        for (int bit = 3; bit <= 4; ++bit)
            if (h[3] & (1 << bit)) {
                const void *z = skip < size - 8 ? memchr(h + skip, 0, (size_t)(size - 8 - skip)) : nullptr;
                if (!z) return mk::fail(MK_E_CORRUPT, "gzip member with an unterminated %s at byte %llu", bit == 3 ? "FNAME" : "FCOMMENT", (unsigned long long)at);
                skip = (uint64_t)((const uint8_t *)z - h) + 1;
            }
        if (h[3] & 2) skip += 2;
        if (skip + 8 > size) return mk::fail(MK_E_CORRUPT, "BGZF member whose header fields overrun BSIZE at byte %llu", (unsigned long long)at);
        if (members && k < cap) members[k] = mk_bgzf_member{at + skip, text, (uint32_t)(size - skip - 8), isize, crc, 0};
        ++k, text += isize, at += size;
    }
    *n_members = k;
    if (consumed) *consumed = at;
    if (text_bytes) *text_bytes = text;
    return MK_OK;
}

// ---- a gzip file in parallel pieces (gzip_segments.hpp says how; kernels: gzip_inflate.hip) -------------------------------------
}  // extern "C"

namespace {

// RFC 1952: does a member's header parse at gz[b ...]?  -> the offset of the byte behind it (FEXTRA / FNAME / FCOMMENT / FHCRC
// walked), with room for a DEFLATE stream (2 bytes at least) and the 8 trailer bytes inside the file; 0 = no header here
uint64_t gzip_header_end(const uint8_t *gz, uint64_t n, uint64_t b) {
    if (n - b < 10 + 2 + 8 || gz[b] != 0x1f || gz[b + 1] != 0x8b || gz[b + 2] != 8 || (gz[b + 3] & 0xE0)) return 0;
    const uint8_t flg = gz[b + 3];
    uint64_t p = b + 10;
    if (flg & 4) {
        if (p + 2 > n) return 0;
        p += 2 + (gz[p] | (uint64_t)gz[p + 1] << 8);
    }
    for (int bit = 3; bit <= 4; ++bit)
        if (flg & (1 << bit)) {
            const void *z = p < n ? memchr(gz + p, 0, (size_t)(n - p)) : nullptr;
            if (!z) return 0;
            p = (uint64_t)((const uint8_t *)z - gz) + 1;
        }
    if (flg & 2) p += 2;
    return p <= n && n - p >= 2 + 8 ? p : 0;
}

// a candidate member of the uploaded bytes: its DEFLATE stream is [pay, end), the trailer behind it says crc / isize
struct GzMember {
    uint64_t pay, end;
    uint32_t crc, isize;
};

// up[0, n_up) goes to the device as it is; `mem` = the chain of candidate members in it, mem[0] a real one.  A candidate that does
// not end on its final block in front of its trailer was cut at a guess that is no member start: the guess is dropped (the candidate
// joined with the next one) and the pieces are decoded again, four rounds in all.  *taken = 1: every member left decoded from its
// first bit to a final block that ends in its last payload byte, and its text has the trailer's CRC-32 and ISIZE -- the chain zlib
// walks, since a DEFLATE stream decoded from a given bit has one end.  Called with the handle's mutex held.
int gzip_inflate_chain(mk_codec *c, const uint8_t *up, uint64_t n_up, std::vector<GzMember> mem, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_members) {
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    int rc;
    // nominal chunks of compressed bytes (a block of zlib's is 15-40 KiB of them).  A piece is decoded by one wave at that wave's pace
    // (~13 MB/s of text), so what counts is the largest piece and how many rounds of the device's decoder slots (17 per CU) the
    // pieces make.  Cuts every 16 KiB give every block its own piece (no piece can be smaller); up to a round and a half of them
    // that is the fastest (61 MB of stream: 27 ms against 37); above, cuts every 64 KiB (pieces of ~2 blocks, a third of the
    // search waves) are (245 MB: 63 ms against 67).  At most 32 768 chunks (the prefix kernel's grid; a stream of more than 2 GiB
    // gets larger chunks).  With the members' first bits the pieces are at most 65 535 (a grid dimension): more is not taken.
    const uint64_t n_in = n_up;
    uint64_t chunk = c->gzip_chunk ? c->gzip_chunk : (n_in / (32u << 10) <= (uint64_t)c->num_cus * 17 * 3 / 2 ? 16u << 10 : 64u << 10);
    while (n_in / chunk > 32768) chunk *= 2;
    const uint32_t n_chunks = (uint32_t)std::max<uint64_t>(1, n_in / chunk);
    constexpr uint64_t kMaxSegments = 65535;
    if (mem.size() > kMaxSegments) return MK_OK;
    if ((rc = mk::ensure_device(&c->d_gz_in, &c->gz_in_cap, n_in + mkz::kPad + 16))) return rc;
    // tables: starts[n_chunks] | per segment (J <= n_chunks + members of them), 64-bit: bits, end, lim, off, cap | n_out | text_off |
    // 32-bit: first[J + 1], status[J] | bad
    const size_t max_seg = (size_t)n_chunks + mem.size();
    const size_t tab_words = (size_t)n_chunks + max_seg * 8 + 16;
    if ((rc = mk::ensure_device(&c->d_gz_tab, &c->gz_tab_cap, tab_words * 8))) return rc;
    unsigned long long *d_starts = (unsigned long long *)c->d_gz_tab;
    double t0 = now_ms();
    if ((rc = upload(c, c->d_gz_in, up, n_in))) return rc;
    MKC_HIP(hipMemsetAsync((uint8_t *)c->d_gz_in + n_in, 0, mkz::kPad + 16, c->stream), "hipMemsetAsync");
    MKC_HIP(hipStreamSynchronize(c->stream), "upload of the stream");
    c->gz_ms[0] = (float)(now_ms() - t0);
    // ---- block starts: searched over all the bytes as they lie there, headers and trailers included
    t0 = now_ms();
    std::vector<unsigned long long> starts(n_chunks, ~0ull);
    mkz::launch_gzip_find((const uint8_t *)c->d_gz_in, n_in, chunk, n_chunks, chunk, d_starts, c->stream);  // (a start behind the next cut is the next chunk's to find)
    MKC_HIP(hipGetLastError(), "gzip block search");
    if (n_chunks > 1) MKC_HIP(hipMemcpyAsync(starts.data() + 1, d_starts + 1, (n_chunks - 1) * 8ull, hipMemcpyDeviceToHost, c->stream), "download of the block starts");
    MKC_HIP(hipStreamSynchronize(c->stream), "gzip block search");
    c->gz_ms[1] = (float)(now_ms() - t0);
    std::vector<unsigned long long> found;  // (increasing)
    for (uint32_t k = 1; k < n_chunks; ++k)
        if (starts[k] != ~0ull && (found.empty() || starts[k] > found.back())) found.push_back(starts[k]);
    // ---- segments -> symbols.  Room per segment: 12 x its compressed bytes (FASTQ / FASTA / text: 3-6 x), then 48 x once more.
    // A start the search took for one and that is none (as good as never: gzip_segments.hpp) shows here: the piece in front of it
    // runs over it (kSegDesync, and says at which block boundary it stands).  Such starts are dropped and the pieces decoded
    // again, a few times at most -- as are the member starts that are none.
    std::vector<unsigned long long> tab, n_out, text_off;  // tab: bits | end | lim | off | cap, J of each
    std::vector<uint32_t> seg_first, mem_first;            // segment -> first segment of its member; member -> its first segment (M + 1)
    std::vector<int32_t> status;
    unsigned long long *d_bits = nullptr, *d_end = nullptr, *d_lim = nullptr, *d_off = nullptr, *d_cap = nullptr, *d_nout = nullptr, *d_toff = nullptr;
    uint32_t *d_first = nullptr, *d_bad = nullptr;
    int32_t *d_status = nullptr;
    uint32_t J = 0;
    bool done = false;
    t0 = now_ms();
    // (ISIZE says how much text there is in all -- below 4 GiB of it: the first guess per piece is half as much again as the stream's
    // own ratio, which spares a 1.27 GB FASTQ two thirds of a 6 GB allocation; a stream of 4 GiB of text or more starts at 12)
    uint64_t said_text = 0;
    for (const GzMember &m : mem) said_text += m.isize;
    const uint64_t whole_ratio = n_in ? said_text / n_in + 1 : 1;
    uint64_t ratio = (n_in < (1ull << 29) && said_text > n_in) ? std::min<uint64_t>(12, whole_ratio + whole_ratio / 2 + 1) : 12;
    for (int dropped_rounds = 0, member_rounds = 0; !done;) {
        // the table: every member's first bit is a start that is KNOWN; of the searched ones those inside its payload are kept (one in
        // a header or a trailer is none)
        const size_t M = mem.size();
        std::vector<unsigned long long> bits, end, lim;
        mem_first.assign(M + 1, 0), seg_first.clear();
        size_t f = 0;
        for (size_t m = 0; m < M; ++m) {
            mem_first[m] = (uint32_t)bits.size();
            const unsigned long long b0 = mem[m].pay * 8, b1 = mem[m].end * 8;
            bits.push_back(b0);
            while (f < found.size() && found[f] <= b0) ++f;
            for (; f < found.size() && found[f] < b1; ++f) bits.push_back(found[f]);
            for (size_t j = mem_first[m]; j < bits.size(); ++j) {
                end.push_back(j + 1 < bits.size() ? bits[j + 1] : ~0ull);
                lim.push_back(std::max(mem[m].end, mem[m].pay));  // (a guess inside the header in front of it leaves no room: such a member reads nothing and fails)
                seg_first.push_back(mem_first[m]);
            }
        }
        if (bits.size() > kMaxSegments) return MK_OK;
        J = (uint32_t)bits.size();
        mem_first[M] = J;
        seg_first.push_back(J);  // (what the kernels compare the last segment's with)
        tab.assign((size_t)J * 5, 0);
        unsigned long long *seg_off = tab.data() + (size_t)J * 3, *seg_cap = seg_off + J;
        std::copy(bits.begin(), bits.end(), tab.begin()), std::copy(end.begin(), end.end(), tab.begin() + J), std::copy(lim.begin(), lim.end(), tab.begin() + 2 * (size_t)J);
        uint64_t elems = 0;
        for (uint32_t j = 0; j < J; ++j) {
            const uint64_t b0 = bits[j] >> 3, b1 = end[j] != ~0ull ? end[j] >> 3 : lim[j];
            seg_cap[j] = 65536 + ratio * (b1 - b0 + 1);
            seg_off[j] = elems;
            elems += mkz::kSegPrefix + seg_cap[j] + mkz::kSegSlack;
            elems = (elems + 7) & ~7ull;  // (16-byte aligned buffers)
        }
        d_bits = d_starts + n_chunks, d_end = d_bits + J, d_lim = d_end + J, d_off = d_lim + J, d_cap = d_off + J, d_nout = d_cap + J, d_toff = d_nout + J;
        d_first = (uint32_t *)(d_toff + J), d_status = (int32_t *)(d_first + J + 1), d_bad = (uint32_t *)(d_status + J);
        n_out.assign(J, 0), status.assign(J, 0);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && elems * 2 > c->gz_sym_cap && elems * 2 - c->gz_sym_cap > free_b / 2) return MK_OK;  // not taken: too large for this device
        if ((rc = mk::ensure_device(&c->d_gz_sym, &c->gz_sym_cap, elems * 2 + 64))) return rc;
        MKC_HIP(hipMemcpyAsync(d_bits, tab.data(), tab.size() * 8ull, hipMemcpyHostToDevice, c->stream), "upload of the segment table");
        mkz::launch_gzip_segments((const uint8_t *)c->d_gz_in, d_bits, d_end, d_lim, d_off, d_cap, J, (uint16_t *)c->d_gz_sym, d_nout, d_status, c->num_cus, c->stream,
                                  c->inflate_kernel == 1);
        MKC_HIP(hipGetLastError(), "gzip segment decode");
        MKC_HIP(hipMemcpyAsync(n_out.data(), d_nout, J * 8ull, hipMemcpyDeviceToHost, c->stream), "download");
        MKC_HIP(hipMemcpyAsync(status.data(), d_status, J * 4ull, hipMemcpyDeviceToHost, c->stream), "download");
        MKC_HIP(hipStreamSynchronize(c->stream), "gzip segment decode");
        c->gz_segments = J;
        // Member by member from the file's first: a piece that ends on the next start proves that start; the first piece that runs
        // over its end disproves every start in front of the block boundary it stands at (what lies behind is looked at next time).
        // A member whose pieces do not add up otherwise ends somewhere else than at the guess behind it: that guess goes.  What
        // follows a dropped guess says nothing until a member decodes whole again (a real one: the walk goes on from there, so that
        // false guesses in several members cost one round, not one each).
        bool overflow = false, starts_dropped = false, anchored = true;
        std::vector<char> join(M, 0);  // member m ends at no member start: it is joined with member m + 1
        std::vector<unsigned long long> gone;
        for (size_t m = 0; m < M; ++m) {
            if (m && join[m - 1]) continue;  // (it starts at the guess that has just gone)
            int32_t st = 0;
            uint32_t at = mem_first[m];
            bool over = false;
            for (; at < mem_first[m + 1] && st == 0; ++at) {
                if (status[at] == mkz::kSegOverflow) over = true;
                else st = status[at];
            }
            if (st == 0 && !over) {
                anchored = true;
                continue;
            }
            if (!anchored) continue;
            if (st == 0) {
                overflow = true;
            } else if (st == mkz::kSegDesync && at < mem_first[m + 1]) {  // (at: behind the piece that ran over a start, not the member's last)
                const unsigned long long stands_at = n_out[at - 1];
                const size_t before = gone.size();
                for (uint32_t j = at; j < mem_first[m + 1] && bits[j] < stands_at; ++j) gone.push_back(bits[j]);
                if (gone.size() == before) return MK_OK;  // (nothing to drop: not what this is for)
                starts_dropped = true;
            } else {
                if (m + 1 == M) return MK_OK;  // (no guess to drop: a stream that does not decode, or ends elsewhere -- zlib will say what this file is)
                join[m] = 1, anchored = false;
            }
        }
        if (starts_dropped) {
            if (++dropped_rounds > 3) return MK_OK;
            std::vector<unsigned long long> kept;
            std::set_difference(found.begin(), found.end(), gone.begin(), gone.end(), std::back_inserter(kept));
            found.swap(kept);
        }
        if (std::find(join.begin(), join.end(), 1) != join.end()) {
            if (++member_rounds > 3) return MK_OK;
            std::vector<GzMember> left;
            for (size_t m = 0; m < M; ++m) {
                if (m && join[m - 1]) left.back().end = mem[m].end, left.back().crc = mem[m].crc, left.back().isize = mem[m].isize;
                else left.push_back(mem[m]);
            }
            mem.swap(left);
            continue;
        }
        if (starts_dropped) continue;
        if (!overflow) done = true;
        else if (ratio == 48) break;
        else ratio = 48;
    }
    c->gz_ms[2] = (float)(now_ms() - t0);
    if (!done) return MK_OK;
    // every member's text: below 4 GiB, and as long as its trailer says
    const size_t M = mem.size();
    text_off.assign(J, 0);
    std::vector<uint64_t> mem_text(M, 0);
    uint64_t total = 0;
    uint32_t max_member_segs = 1;
    for (size_t m = 0; m < M; ++m) {
        for (uint32_t j = mem_first[m]; j < mem_first[m + 1]; ++j) text_off[j] = total, total += n_out[j], mem_text[m] += n_out[j];
        if (mem_text[m] >> 32 || (uint32_t)mem_text[m] != mem[m].isize) return MK_OK;
        max_member_segs = std::max(max_member_segs, mem_first[m + 1] - mem_first[m]);
    }
    // ---- contexts, text, CRC-32
    t0 = now_ms();
    // (the contexts, and behind them two sets of J - 1 maps of 32 768 16-bit elements: launch_gzip_resolve)
    if ((rc = mk::ensure_device(&c->d_gz_ctx, &c->gz_ctx_cap, (size_t)J * mkz::kSegPrefix * 5 + 16))) return rc;
    if ((rc = mk::ensure_device(&c->d_gz_text, &c->gz_text_cap, total + 64))) return rc;
    MKC_HIP(hipMemcpyAsync(d_toff, text_off.data(), J * 8ull, hipMemcpyHostToDevice, c->stream), "upload of the text offsets");
    MKC_HIP(hipMemcpyAsync(d_first, seg_first.data(), (J + 1) * 4ull, hipMemcpyHostToDevice, c->stream), "upload of the member table");
    MKC_HIP(hipMemsetAsync(d_bad, 0, 4, c->stream), "hipMemsetAsync");
    mkz::launch_gzip_resolve((const uint16_t *)c->d_gz_sym, d_off, d_nout, d_toff, d_first, J, max_member_segs, (uint8_t *)c->d_gz_ctx, (uint8_t *)c->d_gz_text, d_bad,
                             c->stream);
    MKC_HIP(hipGetLastError(), "gzip resolution");
    uint32_t bad = 0;
    MKC_HIP(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, c->stream), "download");
    MKC_HIP(hipStreamSynchronize(c->stream), "gzip resolution");
    c->gz_ms[3] = (float)(now_ms() - t0);
    if (bad) return MK_OK;
    t0 = now_ms();
    {
        // CRC-32 of every member's text: per block of at most 65 280 bytes on the device (the BGZF writer's wave), the grid cut member
        // by member, folded here: crc(A ++ B) = crc(A) * x^(8 |B|) mod P  ^  crc(B)
        const uint32_t bb = mkz::kMaxBlockBytes;
        std::vector<unsigned long long> blk_off;
        std::vector<uint32_t> blk_len;
        for (size_t m = 0; m < M; ++m)
            for (uint64_t at = 0; at < mem_text[m]; at += bb) blk_off.push_back(text_off[mem_first[m]] + at), blk_len.push_back((uint32_t)std::min<uint64_t>(bb, mem_text[m] - at));
        const size_t blocks = blk_off.size();
        if (blocks >> 32) return MK_OK;
        if ((rc = mk::ensure_device(&c->d_crc, &c->crc_cap, blocks * 4ull + 16)) || (rc = mk::ensure_device(&c->d_off, &c->off_cap, blocks * 8ull + 16)) ||
            (rc = mk::ensure_device(&c->d_len, &c->len_cap, blocks * 4ull + 16)))
            return rc;
        std::vector<uint32_t> crcs(blocks);
        if (blocks) {
            MKC_HIP(hipMemcpyAsync(c->d_off, blk_off.data(), blocks * 8ull, hipMemcpyHostToDevice, c->stream), "upload of the CRC blocks");
            MKC_HIP(hipMemcpyAsync(c->d_len, blk_len.data(), blocks * 4ull, hipMemcpyHostToDevice, c->stream), "upload of the CRC blocks");
            mkz::launch_crc_ranges((const uint8_t *)c->d_gz_text, (const unsigned long long *)c->d_off, (const uint32_t *)c->d_len, (uint32_t)blocks, (uint32_t *)c->d_crc,
                                   c->stream);
            MKC_HIP(hipGetLastError(), "CRC kernel");
            MKC_HIP(hipMemcpyAsync(crcs.data(), c->d_crc, blocks * 4ull, hipMemcpyDeviceToHost, c->stream), "download of the CRCs");
        }
        MKC_HIP(hipStreamSynchronize(c->stream), "CRC kernel");
        const uint32_t shift_full = mkz::crc_x_pow_bytes(bb);
        size_t b = 0;
        for (size_t m = 0; m < M; ++m) {
            uint32_t crc = 0;
            for (uint64_t at = 0; at < mem_text[m]; at += bb, ++b) crc = mkz::crc_mulmod(crc, blk_len[b] == bb ? shift_full : mkz::crc_x_pow_bytes(blk_len[b])) ^ crcs[b];
            if (crc != mem[m].crc) return MK_OK;
        }
    }
    c->gz_ms[4] = (float)(now_ms() - t0);
    c->gz_text_bytes = total;
    *text_bytes = total, *taken = 1;
    if (n_members) *n_members = M;
    // what is left to keep is the text: the symbols (24 x the compressed bytes) and the contexts go back to the device now
    for (void **q : {&c->d_gz_sym, &c->d_gz_ctx, &c->d_gz_in}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    c->gz_sym_cap = c->gz_ctx_cap = c->gz_in_cap = 0;
    return MK_OK;
}

}  // namespace

extern "C" {

int mk_gzip_member_guesses(const uint8_t *gz, uint64_t n, mk_gzip_guess *table, uint64_t cap, uint64_t *n_guesses) {
    if (!n_guesses || (n && !gz)) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_member_guesses: NULL argument");
    *n_guesses = 0;
    if (n < 20 || !gzip_header_end(gz, n, 0)) return MK_OK;  // (not a gzip file: no guesses)
    uint64_t k = 0;
    auto trailer = [&](uint64_t member, uint64_t end) {  // the 8 bytes in front of `end` are what the member in front of it ends with
        if (table && member < cap) memcpy(&table[member].crc, gz + end - 8, 4), memcpy(&table[member].isize, gz + end - 4, 4);
    };
    for (uint64_t b = 0; n - b >= 20;) {
        const uint64_t p = gzip_header_end(gz, n, b);
        if (p && (b == 0 || b >= 8)) {  // (behind the first one: with the room of a trailer in front of it)
            if (k) trailer(k - 1, b);
            if (table && k < cap) table[k] = mk_gzip_guess{b, p, 0, 0};
            ++k;
        }
        const void *next = memchr(gz + b + 1, 0x1f, (size_t)(n - b - 1));  // (ID1: one byte in 256)
        if (!next) break;
        b = (uint64_t)((const uint8_t *)next - gz);
    }
    trailer(k - 1, n);
    *n_guesses = k;
    return MK_OK;
}

int mk_gzip_inflate_device(mk_codec *c, const uint8_t *gz, uint64_t n, uint64_t *text_bytes, uint32_t *taken) {
    MK_ABI_BEGIN
    if (!c || !text_bytes || !taken || (n && !gz)) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_inflate_device: NULL argument");
    *text_bytes = 0, *taken = 0;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->gzs.active) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_inflate_device: the handle has an open stream (mk_gzip_stream_end)");
    c->gz_text_bytes = 0, c->gz_segments = 0;
    for (float &x : c->gz_ms) x = 0;
    // RFC 1952: the member's header, then the DEFLATE stream up to the 8 trailer bytes.  One member is what is taken here: the stream
    // has to end where the file does, on the final block its last piece meets in front of the trailer (a file of several members
    // does not: mk_gzip_members_inflate_device).  Not gzip / reserved flags / no room for a stream: not taken.
    const uint64_t p = n ? gzip_header_end(gz, n, 0) : 0;
    if (!p) return MK_OK;
    GzMember one{0, n - 8 - p, 0, 0};
    memcpy(&one.crc, gz + n - 8, 4), memcpy(&one.isize, gz + n - 4, 4);
    return gzip_inflate_chain(c, gz + p, one.end, {one}, text_bytes, taken, nullptr);
    MK_ABI_END
}

int mk_gzip_members_inflate_device(mk_codec *c, const uint8_t *gz, uint64_t n, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_members) {
    MK_ABI_BEGIN
    if (!c || !text_bytes || !taken || !n_members || (n && !gz)) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_members_inflate_device: NULL argument");
    *text_bytes = 0, *taken = 0, *n_members = 0;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->gzs.active) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_members_inflate_device: the handle has an open stream (mk_gzip_stream_end)");
    c->gz_text_bytes = 0, c->gz_segments = 0;
    for (float &x : c->gz_ms) x = 0;
    // the member starts as the host can guess them: every place where a header parses.  The file goes up whole; which guesses are
    // member starts is what the decode proves (gzip_inflate_chain).  Bytes behind the last member cannot be proved away: not taken.
    uint64_t n_guesses = 0;
    int rc = mk_gzip_member_guesses(gz, n, nullptr, 0, &n_guesses);
    if (rc || !n_guesses) return rc;
    std::vector<mk_gzip_guess> guesses(n_guesses);
    if ((rc = mk_gzip_member_guesses(gz, n, guesses.data(), n_guesses, &n_guesses))) return rc;
    std::vector<GzMember> mem(n_guesses);
    for (uint64_t k = 0; k < n_guesses; ++k) mem[k] = GzMember{guesses[k].data_off, (k + 1 < n_guesses ? guesses[k + 1].header_off : n) - 8, guesses[k].crc, guesses[k].isize};
    return gzip_inflate_chain(c, gz, n, std::move(mem), text_bytes, taken, n_members);
    MK_ABI_END
}

int mk_gzip_text_read(mk_codec *c, uint64_t offset, uint8_t *out, uint64_t len) {
    MK_ABI_BEGIN
    if (!c || (len && !out)) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_text_read: NULL argument");
    std::lock_guard<std::mutex> lock(c->mu);
    if (offset > c->gz_text_bytes || len > c->gz_text_bytes - offset) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_text_read: [%llu, +%llu) is outside the text", (unsigned long long)offset, (unsigned long long)len);
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    return download(c, out, (const uint8_t *)c->d_gz_text + offset, len);
    MK_ABI_END
}

const void *mk_gzip_text_device(const mk_codec *c, uint64_t *text_bytes) {
    if (text_bytes) *text_bytes = c ? c->gz_text_bytes : 0;
    return c && c->gz_text_bytes ? c->d_gz_text : nullptr;
}

int mk_gzip_text_release(mk_codec *c) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_text_release: NULL handle");
    std::lock_guard<std::mutex> lock(c->mu);
    (void)hipSetDevice(c->device);
    gzip_stream_close(c);  // (an open stream's text is the text: the stream ends with it)
    for (void **p : {&c->d_gz_in, &c->d_gz_sym, &c->d_gz_tab, &c->d_gz_ctx, &c->d_gz_text}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    c->gz_in_cap = c->gz_sym_cap = c->gz_tab_cap = c->gz_ctx_cap = c->gz_text_cap = 0;
    c->gz_text_bytes = 0;
    return MK_OK;
}

int mk_gzip_info(const mk_codec *c, uint32_t *segments, float ms[5]) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_info: NULL handle");
    if (segments) *segments = c->gz_segments;
    if (ms)
        for (int k = 0; k < 5; ++k) ms[k] = c->gz_ms[k];
    return MK_OK;
}

}  // extern "C"

// ---- a gzip file of any size, window by window (mk_gzip_stream_*) ------------------------------------------------------------------
namespace {

constexpr uint64_t kStreamWindow = 256ull << 20;  // the default window (an unmeasured choice: README)
constexpr uint64_t kStreamMargin = 64;            // bytes uploaded behind the window: a trailer and the fixed part of the next header

uint64_t stream_held(const mk_codec *c) {
    return c->gz_in_cap + c->gz_sym_cap + c->gz_tab_cap + c->gz_ctx_cap + c->gzs.text_cap[0] + c->gzs.text_cap[1] + (c->gzs.d_carry[0] ? 2ull * mkz::kSegPrefix : 0);
}

// a candidate member of a window: its DEFLATE stream starts at bit `pay_bit` of the upload; closed: its trailer lies at byte `end`
// of the upload (crc / isize read there); open: the trailer lies behind the upload, the member goes on in the next window
struct WinMember {
    uint64_t header, pay_bit, end;  // header: byte of the upload where its header parses (the continued member: 0, unused)
    bool closed;
};

// One window: *state = 0 (c->gz_text_bytes of text in the current text buffer) or 2.  3 = grow the window and call again.  A return
// other than MK_OK is a device error (the caller makes it state 2).  Called with the handle's mutex held.
int gzip_stream_window(mk_codec *c, uint32_t *state) {
    mk_gzip_stream &S = c->gzs;
    *state = 2;
    int rc;
    const uint64_t base = S.pos_bit >> 3;
    const uint64_t nominal = (S.window << S.grow) + kStreamMargin;
    const uint64_t n_up = std::min<uint64_t>(S.n - base, nominal);
    const bool is_last = base + n_up == S.n;
    const uint8_t *up = S.gz + base;
    // ---- the candidate members: the one the window continues or the header it starts at, then every guess inside the upload
    std::vector<WinMember> mem;
    if (S.in_member) {
        mem.push_back(WinMember{0, S.pos_bit - base * 8, 0, false});
    } else {
        const uint64_t p = gzip_header_end(S.gz, S.n, base);
        if (!p) return MK_OK;  // bytes behind the last member that are no member
        if (p + 2 > base + n_up) {
            *state = 3;
            return MK_OK;
        }
        mem.push_back(WinMember{0, (p - base) * 8, 0, false});
    }
    {
        const uint64_t from = base + (mem[0].pay_bit >> 3);
        auto g = std::upper_bound(S.guesses.begin(), S.guesses.end(), from, [](uint64_t v, const mk_gzip_guess &x) { return v < x.header_off; });
        for (; g != S.guesses.end() && g->data_off + 2 <= base + n_up; ++g) {
            if (g->header_off < base + 8) continue;  // (no room for a trailer in front of it inside this upload)
            mem.back().end = g->header_off - base - 8, mem.back().closed = true;
            mem.push_back(WinMember{g->header_off - base, (g->data_off - base) * 8, 0, false});
        }
        if (is_last) mem.back().end = n_up - 8, mem.back().closed = true;
    }
    const uint64_t n_in = n_up;
    uint64_t chunk = c->gzip_chunk ? c->gzip_chunk : (n_in / (32u << 10) <= (uint64_t)c->num_cus * 17 * 3 / 2 ? 16u << 10 : 64u << 10);
    while (n_in / chunk > 32768) chunk *= 2;
    const uint32_t n_chunks = (uint32_t)std::max<uint64_t>(1, n_in / chunk);
    constexpr uint64_t kMaxSegments = 65535;
    if (mem.size() + n_chunks > kMaxSegments) return MK_OK;
    // buffers by the window's nominal size, so that every window of a file finds them there: nothing is sized by the file
    const size_t seg_room = (size_t)std::max<uint64_t>(1, nominal / chunk) + 16;
    if ((rc = mk::ensure_device(&c->d_gz_in, &c->gz_in_cap, nominal + mkz::kPad + 16))) return rc;
    const size_t max_seg = std::max<size_t>(seg_room, (size_t)n_chunks + mem.size());
    if ((rc = mk::ensure_device(&c->d_gz_tab, &c->gz_tab_cap, ((size_t)n_chunks + max_seg * 8 + 16) * 8))) return rc;
    unsigned long long *d_starts = (unsigned long long *)c->d_gz_tab;
    double t0 = now_ms();
    if ((rc = upload(c, c->d_gz_in, up, n_in))) return rc;
    MKC_HIP(hipMemsetAsync((uint8_t *)c->d_gz_in + n_in, 0, mkz::kPad + 16, c->stream), "hipMemsetAsync");
    MKC_HIP(hipStreamSynchronize(c->stream), "upload of the window");
    S.stats.ms[0] += (float)(now_ms() - t0);
    t0 = now_ms();
    std::vector<unsigned long long> starts(n_chunks, ~0ull), found;
    mkz::launch_gzip_find((const uint8_t *)c->d_gz_in, n_in, chunk, n_chunks, chunk, d_starts, c->stream);
    MKC_HIP(hipGetLastError(), "gzip block search");
    if (n_chunks > 1) MKC_HIP(hipMemcpyAsync(starts.data() + 1, d_starts + 1, (n_chunks - 1) * 8ull, hipMemcpyDeviceToHost, c->stream), "download of the block starts");
    MKC_HIP(hipStreamSynchronize(c->stream), "gzip block search");
    S.stats.ms[1] += (float)(now_ms() - t0);
    for (uint32_t k = 1; k < n_chunks; ++k)
        if (starts[k] != ~0ull && (found.empty() || starts[k] > found.back())) found.push_back(starts[k]);
    // ---- pieces -> symbols, in rounds as gzip_inflate_chain runs them.  The last candidate of a window that is not the file's last
    // is OPEN: its pieces end at found starts only, and the last of those is the cut -- no piece is decoded behind it.
    std::vector<unsigned long long> tab, n_out, bits, end, lim;
    std::vector<uint32_t> seg_first, mem_first;
    std::vector<int32_t> status;
    unsigned long long *d_bits = nullptr, *d_end = nullptr, *d_lim = nullptr, *d_off = nullptr, *d_cap = nullptr, *d_nout = nullptr, *d_toff = nullptr;
    uint32_t *d_first = nullptr, *d_bad = nullptr;
    int32_t *d_status = nullptr;
    uint32_t J = 0;
    uint64_t ratio = 12, cut_bit = ~0ull;  // cut_bit: the open member's last start (~0: it has none)
    bool done = false;
    t0 = now_ms();
    for (int dropped_rounds = 0, member_rounds = 0, round = 0; !done; ++round) {
        if (round) ++S.stats.rounds_repeated;
        const size_t M = mem.size();
        bits.clear(), end.clear(), lim.clear(), seg_first.clear();
        mem_first.assign(M + 1, 0);
        cut_bit = ~0ull;
        size_t f = 0;
        for (size_t m = 0; m < M; ++m) {
            mem_first[m] = (uint32_t)bits.size();
            const unsigned long long b0 = mem[m].pay_bit, b1 = mem[m].closed ? mem[m].end * 8 : n_in * 8;
            std::vector<unsigned long long> at{b0};
            while (f < found.size() && found[f] <= b0) ++f;
            for (; f < found.size() && found[f] < b1; ++f) at.push_back(found[f]);
            if (!mem[m].closed) {  // (the last start is where the window ends)
                if (at.size() > 1) cut_bit = at.back();
                at.pop_back();
            }
            for (size_t j = 0; j < at.size(); ++j) {
                bits.push_back(at[j]);
                end.push_back(j + 1 < at.size() ? at[j + 1] : mem[m].closed ? ~0ull : cut_bit);
                lim.push_back(mem[m].closed ? std::max(mem[m].end, mem[m].pay_bit >> 3) : n_in);
                seg_first.push_back(mem_first[m]);
            }
        }
        if (bits.size() > kMaxSegments) return MK_OK;
        J = (uint32_t)bits.size();
        mem_first[M] = J;
        seg_first.push_back(J);
        if (!J) break;  // (one open member without a start: the window grows)
        tab.assign((size_t)J * 5, 0);
        unsigned long long *seg_off = tab.data() + (size_t)J * 3, *seg_cap = seg_off + J;
        std::copy(bits.begin(), bits.end(), tab.begin()), std::copy(end.begin(), end.end(), tab.begin() + J), std::copy(lim.begin(), lim.end(), tab.begin() + 2 * (size_t)J);
        uint64_t elems = 0;
        for (uint32_t j = 0; j < J; ++j) {
            const uint64_t b0 = bits[j] >> 3, b1 = end[j] != ~0ull ? end[j] >> 3 : lim[j];
            seg_cap[j] = 65536 + ratio * (b1 - b0 + 1);
            seg_off[j] = elems;
            elems += mkz::kSegPrefix + seg_cap[j] + mkz::kSegSlack;
            elems = (elems + 7) & ~7ull;
        }
        if (J > max_seg) return mk::fail(MK_E_HIP, "mk_gzip_stream_next: %u pieces, a table for %llu (internal error)", J, (unsigned long long)max_seg);
        d_bits = d_starts + n_chunks, d_end = d_bits + J, d_lim = d_end + J, d_off = d_lim + J, d_cap = d_off + J, d_nout = d_cap + J, d_toff = d_nout + J;
        d_first = (uint32_t *)(d_toff + J), d_status = (int32_t *)(d_first + J + 1), d_bad = (uint32_t *)(d_status + J);
        n_out.assign(J, 0), status.assign(J, 0);
        const uint64_t sym_need = std::max<uint64_t>(elems, seg_room * (uint64_t)(mkz::kSegPrefix + 65536 + mkz::kSegSlack + 8 + ratio) + ratio * nominal) * 2 + 64;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && sym_need > c->gz_sym_cap && sym_need - c->gz_sym_cap > free_b / 2) return MK_OK;  // no room on this device
        if ((rc = mk::ensure_device(&c->d_gz_sym, &c->gz_sym_cap, sym_need))) return rc;
        MKC_HIP(hipMemcpyAsync(d_bits, tab.data(), tab.size() * 8ull, hipMemcpyHostToDevice, c->stream), "upload of the segment table");
        mkz::launch_gzip_segments((const uint8_t *)c->d_gz_in, d_bits, d_end, d_lim, d_off, d_cap, J, (uint16_t *)c->d_gz_sym, d_nout, d_status, c->num_cus, c->stream,
                                  c->inflate_kernel == 1);
        MKC_HIP(hipGetLastError(), "gzip segment decode");
        MKC_HIP(hipMemcpyAsync(n_out.data(), d_nout, J * 8ull, hipMemcpyDeviceToHost, c->stream), "download");
        MKC_HIP(hipMemcpyAsync(status.data(), d_status, J * 4ull, hipMemcpyDeviceToHost, c->stream), "download");
        MKC_HIP(hipStreamSynchronize(c->stream), "gzip segment decode");
        c->gz_segments = J;
        // the walk of gzip_inflate_chain; an open member has no last piece to judge, and every one of its pieces ends at a found start
        bool overflow = false, starts_dropped = false, anchored = true;
        std::vector<char> join(M, 0);
        std::vector<unsigned long long> gone;
        for (size_t m = 0; m < M; ++m) {
            if (m && join[m - 1]) continue;
            int32_t st = 0;
            uint32_t at = mem_first[m];
            bool over = false;
            for (; at < mem_first[m + 1] && st == 0; ++at) {
                if (status[at] == mkz::kSegOverflow) over = true;
                else st = status[at];
            }
            if (st == 0 && !over) {
                anchored = true;
                continue;
            }
            if (!anchored) continue;
            if (st == 0) {
                overflow = true;
            } else if (st == mkz::kSegDesync && (at < mem_first[m + 1] || !mem[m].closed)) {
                const unsigned long long from = bits[at - 1], stands_at = n_out[at - 1], b1 = mem[m].closed ? mem[m].end * 8 : n_in * 8;
                const size_t before = gone.size();
                for (unsigned long long x : found)
                    if (x > from && x < stands_at && x < b1) gone.push_back(x);
                if (gone.size() == before) return MK_OK;
                starts_dropped = true;
            } else {
                if (m + 1 == M) return MK_OK;  // (no guess to drop: a stream that does not decode, or ends elsewhere)
                join[m] = 1, anchored = false;
            }
        }
        if (starts_dropped) {
            if (++dropped_rounds > 3) return MK_OK;
            std::sort(gone.begin(), gone.end());
            std::vector<unsigned long long> kept;
            std::set_difference(found.begin(), found.end(), gone.begin(), gone.end(), std::back_inserter(kept));
            found.swap(kept);
        }
        if (std::find(join.begin(), join.end(), 1) != join.end()) {
            if (++member_rounds > 3) return MK_OK;
            std::vector<WinMember> left;
            for (size_t m = 0; m < M; ++m) {
                if (m && join[m - 1]) left.back().end = mem[m].end, left.back().closed = mem[m].closed;
                else left.push_back(mem[m]);
            }
            mem.swap(left);
            continue;
        }
        if (starts_dropped) continue;
        if (!overflow) done = true;
        else if (ratio == 48) return MK_OK;
        else ratio = 48;
    }
    S.stats.ms[2] += (float)(now_ms() - t0);
    // ---- where the window ends
    const size_t M = mem.size();
    const WinMember &last = mem[M - 1];
    uint64_t next_bit;
    bool next_in_member;
    if (last.closed) next_bit = S.n * 8, next_in_member = false;
    else if (cut_bit != ~0ull) next_bit = base * 8 + cut_bit, next_in_member = true;
    else if (M > 1) next_bit = (base + last.header) * 8, next_in_member = false;  // (the open member begins the next window, header first)
    else next_bit = S.pos_bit, next_in_member = S.in_member;
    if (next_bit <= S.pos_bit && !last.closed) {  // no proved start to stop at
        *state = is_last ? 2 : 3;
        return MK_OK;
    }
    // ---- every closed member's text is as long as its trailer says (modulo 2^32, of all its windows)
    std::vector<unsigned long long> text_off(std::max<uint32_t>(J, 1), 0);
    std::vector<uint64_t> mem_text(M, 0);
    uint64_t total = 0;
    uint32_t max_member_segs = 1;
    for (size_t m = 0; m < M; ++m) {
        for (uint32_t j = mem_first[m]; j < mem_first[m + 1]; ++j) text_off[j] = total, total += n_out[j], mem_text[m] += n_out[j];
        if (mem[m].closed) {
            uint32_t isize;
            memcpy(&isize, up + mem[m].end + 4, 4);
            const uint64_t len = mem_text[m] + (m == 0 && S.in_member ? S.open_len : 0);
            if ((uint32_t)len != isize) return MK_OK;
        }
        max_member_segs = std::max(max_member_segs, mem_first[m + 1] - mem_first[m]);
    }
    t0 = now_ms();
    void **d_text = &S.d_text[S.text_cur ^ 1];
    size_t *text_cap = &S.text_cap[S.text_cur ^ 1];
    if ((rc = mk::ensure_device(&c->d_gz_ctx, &c->gz_ctx_cap, std::max<size_t>(J, seg_room) * mkz::kSegPrefix * 5 + 16))) return rc;
    if ((rc = mk::ensure_device(d_text, text_cap, std::max<uint64_t>(total, ratio * nominal) + 64))) return rc;
    uint32_t bad = 0;
    if (J) {
        MKC_HIP(hipMemcpyAsync(d_toff, text_off.data(), J * 8ull, hipMemcpyHostToDevice, c->stream), "upload of the text offsets");
        MKC_HIP(hipMemcpyAsync(d_first, seg_first.data(), (J + 1) * 4ull, hipMemcpyHostToDevice, c->stream), "upload of the member table");
        MKC_HIP(hipMemsetAsync(d_bad, 0, 4, c->stream), "hipMemsetAsync");
        mkz::launch_gzip_resolve((const uint16_t *)c->d_gz_sym, d_off, d_nout, d_toff, d_first, J, max_member_segs, (uint8_t *)c->d_gz_ctx, (uint8_t *)*d_text, d_bad,
                                 c->stream, S.in_member ? (const uint8_t *)S.d_carry[S.carry_cur] : nullptr, S.carry_len);
        MKC_HIP(hipGetLastError(), "gzip resolution");
        MKC_HIP(hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, c->stream), "download");
        MKC_HIP(hipStreamSynchronize(c->stream), "gzip resolution");
    }
    S.stats.ms[3] += (float)(now_ms() - t0);
    if (bad) return MK_OK;
    // ---- CRC-32 per member of its text in this window, folded into what the member had before the window
    t0 = now_ms();
    std::vector<uint32_t> mem_crc(M, 0);
    {
        const uint32_t bb = mkz::kMaxBlockBytes;
        std::vector<unsigned long long> blk_off;
        std::vector<uint32_t> blk_len;
        for (size_t m = 0; m < M; ++m)
            for (uint64_t at = 0; at < mem_text[m]; at += bb) blk_off.push_back(text_off[mem_first[m]] + at), blk_len.push_back((uint32_t)std::min<uint64_t>(bb, mem_text[m] - at));
        const size_t blocks = blk_off.size();
        if (blocks >> 32) return MK_OK;
        if ((rc = mk::ensure_device(&c->d_crc, &c->crc_cap, blocks * 4ull + 16)) || (rc = mk::ensure_device(&c->d_off, &c->off_cap, blocks * 8ull + 16)) ||
            (rc = mk::ensure_device(&c->d_len, &c->len_cap, blocks * 4ull + 16)))
            return rc;
        std::vector<uint32_t> crcs(blocks);
        if (blocks) {
            MKC_HIP(hipMemcpyAsync(c->d_off, blk_off.data(), blocks * 8ull, hipMemcpyHostToDevice, c->stream), "upload of the CRC blocks");
            MKC_HIP(hipMemcpyAsync(c->d_len, blk_len.data(), blocks * 4ull, hipMemcpyHostToDevice, c->stream), "upload of the CRC blocks");
            mkz::launch_crc_ranges((const uint8_t *)*d_text, (const unsigned long long *)c->d_off, (const uint32_t *)c->d_len, (uint32_t)blocks, (uint32_t *)c->d_crc, c->stream);
            MKC_HIP(hipGetLastError(), "CRC kernel");
            MKC_HIP(hipMemcpyAsync(crcs.data(), c->d_crc, blocks * 4ull, hipMemcpyDeviceToHost, c->stream), "download of the CRCs");
        }
        MKC_HIP(hipStreamSynchronize(c->stream), "CRC kernel");
        const uint32_t shift_full = mkz::crc_x_pow_bytes(bb);
        size_t b = 0;
        for (size_t m = 0; m < M; ++m) {
            uint32_t crc = m == 0 && S.in_member ? S.open_crc : 0;
            for (uint64_t at = 0; at < mem_text[m]; at += bb, ++b) crc = mkz::crc_mulmod(crc, blk_len[b] == bb ? shift_full : mkz::crc_x_pow_bytes(blk_len[b])) ^ crcs[b];
            mem_crc[m] = crc;
            if (mem[m].closed) {
                uint32_t said;
                memcpy(&said, up + mem[m].end, 4);
                if (crc != said) return MK_OK;
            }
        }
    }
    S.stats.ms[4] += (float)(now_ms() - t0);
    // ---- the window stands: what the next one starts from
    if (next_in_member) {
        const bool continued = M == 1 && S.in_member;  // the open member is the one this window continued
        const uint8_t *prev = continued ? (const uint8_t *)S.d_carry[S.carry_cur] : nullptr;
        const uint64_t t_open = mem_text[M - 1];
        mkz::launch_gzip_carry((const uint8_t *)*d_text + (J && mem_first[M - 1] < J ? text_off[mem_first[M - 1]] : total), t_open, prev, (uint8_t *)S.d_carry[S.carry_cur ^ 1], c->stream);
        MKC_HIP(hipGetLastError(), "gzip carry");
        MKC_HIP(hipStreamSynchronize(c->stream), "gzip carry");
        S.carry_len = (uint32_t)std::min<uint64_t>(mkz::kSegPrefix, (continued ? S.carry_len : 0) + t_open);
        S.carry_cur ^= 1;
        S.open_crc = mem_crc[M - 1];
        S.open_len = (continued ? S.open_len : 0) + t_open;
    } else {
        S.carry_len = 0, S.open_crc = 0, S.open_len = 0;
    }
    for (size_t m = 0; m < M; ++m) S.stats.members += mem[m].closed;
    S.pos_bit = next_bit, S.in_member = next_in_member;
    S.text_cur ^= 1;
    c->d_gz_text = *d_text, c->gz_text_cap = *text_cap, c->gz_text_bytes = total;
    S.stats.windows += 1, S.stats.text_bytes += total, S.stats.consumed_bytes = S.pos_bit >> 3;
    S.stats.peak_device_bytes = std::max<uint64_t>(S.stats.peak_device_bytes, stream_held(c));
    *state = 0;
    return MK_OK;
}

void gzip_stream_close(mk_codec *c) {
    mk_gzip_stream &S = c->gzs;
    if (!S.active) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (void **q : {&S.d_carry[0], &S.d_carry[1], &S.d_text[0], &S.d_text[1], &c->d_gz_sym, &c->d_gz_ctx, &c->d_gz_in, &c->d_gz_tab}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    c->gz_sym_cap = c->gz_ctx_cap = c->gz_in_cap = c->gz_tab_cap = 0;
    c->d_gz_text = nullptr, c->gz_text_cap = 0, c->gz_text_bytes = 0;
    S = mk_gzip_stream{};
}

}  // namespace

extern "C" {

uint32_t mk_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return mkz::crc_mulmod(crc_a, mkz::crc_x_pow_bytes(len_b)) ^ crc_b; }

int mk_gzip_stream_begin(mk_codec *c, const uint8_t *gz, uint64_t n, uint64_t window_bytes, uint32_t *taken) {
    MK_ABI_BEGIN
    if (!c || !taken || (n && !gz)) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_stream_begin: NULL argument");
    *taken = 0;
    if (window_bytes && (window_bytes < 4096 || window_bytes > (1ull << 40))) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_stream_begin: a window of 4 KiB at least");
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->gzs.active) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_stream_begin: the handle has an open stream (mk_gzip_stream_end)");
    uint64_t n_guesses = 0;
    int rc = mk_gzip_member_guesses(gz, n, nullptr, 0, &n_guesses);
    if (rc || !n_guesses) return rc;  // (not a gzip file)
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    // the one-shot text of an earlier call goes: d_gz_text is the stream's from here on
    for (void **q : {&c->d_gz_in, &c->d_gz_sym, &c->d_gz_tab, &c->d_gz_ctx, &c->d_gz_text}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    c->gz_in_cap = c->gz_sym_cap = c->gz_tab_cap = c->gz_ctx_cap = c->gz_text_cap = 0;
    c->gz_text_bytes = 0, c->gz_segments = 0;
    mk_gzip_stream &S = c->gzs;
    S = mk_gzip_stream{};
    S.guesses.resize(n_guesses);
    if ((rc = mk_gzip_member_guesses(gz, n, S.guesses.data(), n_guesses, &n_guesses))) return rc;
    for (int k = 0; k < 2; ++k) {
        if (hipMalloc(&S.d_carry[k], mkz::kSegPrefix) != hipSuccess || hipMemsetAsync(S.d_carry[k], 0, mkz::kSegPrefix, c->stream) != hipSuccess) {
            (void)hipGetLastError();
            S.active = true;
            gzip_stream_close(c);
            return MK_OK;  // (the codec rule: the device's trouble is "not taken")
        }
    }
    S.active = true, S.gz = gz, S.n = n, S.window = window_bytes ? window_bytes : kStreamWindow;
    *taken = 1;
    return MK_OK;
    MK_ABI_END
}

int mk_gzip_stream_next(mk_codec *c, uint64_t *text_bytes, uint32_t *state) {
    MK_ABI_BEGIN
    if (!c || !text_bytes || !state) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_stream_next: NULL argument");
    *text_bytes = 0, *state = 2;
    std::lock_guard<std::mutex> lock(c->mu);
    mk_gzip_stream &S = c->gzs;
    if (!S.active) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_stream_next: no open stream (mk_gzip_stream_begin)");
    if (S.dead) return MK_OK;
    if (!S.in_member && (S.pos_bit >> 3) == S.n) {
        *state = 1;
        return MK_OK;
    }
    if (hipSetDevice(c->device) != hipSuccess) {
        S.dead = true;
        return MK_OK;
    }
    S.grow = 0;
    for (;;) {
        uint32_t st = 2;
        const int rc = gzip_stream_window(c, &st);
        if (rc != MK_OK) st = 2, (void)hipGetLastError();
        if (st == 3) {  // no proved start inside the window: twice the window, as long as the file and the device have the room
            const uint64_t base = S.pos_bit >> 3;
            if (base + (S.window << S.grow) + kStreamMargin >= S.n || S.grow >= 24) st = 2;
            else {
                ++S.grow, ++S.stats.windows_grown;
                continue;
            }
        }
        if (st == 0) *text_bytes = c->gz_text_bytes;
        else S.dead = true, c->gz_text_bytes = 0;
        *state = st;
        return MK_OK;
    }
    MK_ABI_END
}

int mk_gzip_stream_info(const mk_codec *c, mk_gzip_stream_stats *out) {
    if (!c || !out) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_stream_info: NULL argument");
    std::lock_guard<std::mutex> lock(const_cast<mk_codec *>(c)->mu);  // (mk_gzip_stream_next writes them under it: a call beside it waits for the window)
    *out = c->gzs.stats;  // (no stream open: what the last one left, zeros if there was none)
    return MK_OK;
}

int mk_gzip_stream_end(mk_codec *c) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_stream_end: NULL handle");
    std::lock_guard<std::mutex> lock(c->mu);
    gzip_stream_close(c);
    return MK_OK;
}

}  // extern "C"

extern "C" {

int mk_bgzf_inflate(mk_codec *c, const uint8_t *in, uint64_t n_in, const mk_bgzf_member *members, uint64_t n_members, uint8_t *out,
                    uint64_t out_cap, uint64_t *bad_member) {
    MK_ABI_BEGIN
    if (!c || (n_members && (!in || !members)) || (out_cap && !out)) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_inflate: NULL argument");
    static_assert(sizeof(mk_bgzf_member) == sizeof(mkz::Member), "member layouts");
    if (bad_member) *bad_member = 0;
    for (uint64_t i = 0; i < n_members; ++i) {
        const mk_bgzf_member &m = members[i];
        if (m.data_off > n_in || m.data_len > n_in - m.data_off || m.isize > 65536 || m.out_off > out_cap || m.isize > out_cap - m.out_off) {
            if (bad_member) *bad_member = i;
            return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_inflate: member %llu lies outside its buffers", (unsigned long long)i);
        }
    }
    std::lock_guard<std::mutex> lock(c->mu);
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    c->ms[0] = c->ms[1] = c->ms[2] = 0;
    std::vector<mkz::Member> part;
    std::vector<int32_t> status;
    for (uint64_t m0 = 0; m0 < n_members;) {
        // a run of members whose compressed bytes and text are both contiguous enough to move in one piece each
        uint64_t m1 = m0, text = 0, in_lo = members[m0].data_off, in_hi = in_lo, out_lo = members[m0].out_off, out_hi = out_lo;
        const uint64_t pass_text = c->inflate_pass_text ? c->inflate_pass_text : kInflateChunkText;
        while (m1 < n_members && (m1 == m0 || text + members[m1].isize <= pass_text)) {
            const mk_bgzf_member &m = members[m1];
            in_lo = std::min(in_lo, m.data_off), in_hi = std::max(in_hi, m.data_off + m.data_len);
            out_lo = std::min(out_lo, m.out_off), out_hi = std::max(out_hi, m.out_off + m.isize);
            text += m.isize, ++m1;
        }
        if (out_hi - out_lo > 2 * kInflateChunkText || in_hi - in_lo > 2 * kInflateChunkText)
            return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_inflate: members %llu.. are scattered over more than a device pass holds",
                            (unsigned long long)m0);
        const uint32_t cnt = (uint32_t)(m1 - m0);
        part.resize(cnt);
        for (uint32_t k = 0; k < cnt; ++k) {
            const mk_bgzf_member &m = members[m0 + k];
            part[k] = mkz::Member{m.data_off - in_lo, m.out_off - out_lo, m.data_len, m.isize, m.crc, 0};
        }
        const uint64_t cn = in_hi - in_lo, tn = out_hi - out_lo;
        int rc;
        if ((rc = mk::ensure_device(&c->d_in, &c->in_cap, cn + mkz::kPad)) || (rc = mk::ensure_device(&c->d_aux, &c->aux_cap, cnt * sizeof(mkz::Member))) ||
            (rc = mk::ensure_device(&c->d_out, &c->out_cap, tn + 16)) || (rc = mk::ensure_device(&c->d_len, &c->len_cap, cnt * 4ull)))
            return rc;
        const double t_up = now_ms();
        if ((rc = upload(c, c->d_in, in + in_lo, cn))) return rc;
        MKC_HIP(hipMemsetAsync((uint8_t *)c->d_in + cn, 0, mkz::kPad, c->stream), "hipMemsetAsync");
        MKC_HIP(hipMemcpyAsync(c->d_aux, part.data(), cnt * sizeof(mkz::Member), hipMemcpyHostToDevice, c->stream), "upload of the member table");
        MKC_HIP(hipStreamSynchronize(c->stream), "upload of the members");
        c->ms[0] += (float)(now_ms() - t_up);
        MKC_HIP(hipEventRecord(c->ev[1], c->stream), "hipEventRecord");
        mkz::launch_inflate((const uint8_t *)c->d_in, cn, (const mkz::Member *)c->d_aux, cnt, (uint8_t *)c->d_out, (int32_t *)c->d_len, c->num_cus, c->stream,
                            c->inflate_kernel);
        mkz::launch_crc_check((const uint8_t *)c->d_out, (const mkz::Member *)c->d_aux, cnt, (int32_t *)c->d_len, c->stream);
        MKC_HIP(hipGetLastError(), "BGZF inflate kernels");
        MKC_HIP(hipEventRecord(c->ev[2], c->stream), "hipEventRecord");
        status.resize(cnt);
        MKC_HIP(hipMemcpyAsync(status.data(), c->d_len, cnt * 4ull, hipMemcpyDeviceToHost, c->stream), "download of the status words");
        MKC_HIP(hipStreamSynchronize(c->stream), "BGZF inflate");
        // (a damaged member's text is not handed out: the status words first)
        bool all_ok = true;
        for (uint32_t k = 0; k < cnt && all_ok; ++k) all_ok = status[k] == 0;
        const double t_down = now_ms();
        if (all_ok && tn && (rc = download(c, out + out_lo, c->d_out, tn))) return rc;
        c->ms[1] += elapsed(c->ev[1], c->ev[2]), c->ms[2] += (float)(now_ms() - t_down);
        for (uint32_t k = 0; k < cnt; ++k)
            if (status[k]) {
                if (bad_member) *bad_member = m0 + k;
                if (status[k] > 0)  // the decoder was content (0), the checksum kernel raised its bit
                    return mk::fail(MK_E_CORRUPT, "BGZF member %llu: CRC-32 of the inflated text differs from the trailer's", (unsigned long long)(m0 + k));
                return mk::fail(MK_E_CORRUPT, "BGZF member %llu does not inflate to its ISIZE (decoder status %d)", (unsigned long long)(m0 + k), status[k]);
            }
        m0 = m1;
    }
    return MK_OK;
    MK_ABI_END
}

}  // extern "C"

// ---- a .bz2 file decoded on the device, a wave per block (mk_bzip2_inflate_device; bzip2_inflate.hip) -----------------------------------

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
    for (void **q : {&c->d_gz_sym, &c->d_gz_ctx, &c->d_gz_in}) {
        if (*q) (void)hipFree(*q);
        *q = nullptr;
    }
    c->gz_sym_cap = c->gz_ctx_cap = c->gz_in_cap = 0;
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

int mk_codec_set_bzip2_pass_blocks(mk_codec *c, uint64_t blocks) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_codec_set_bzip2_pass_blocks: NULL handle");
    std::lock_guard<std::mutex> lock(c->mu);
    c->bz_pass_blocks = blocks;
    return MK_OK;
}

}  // extern "C"
