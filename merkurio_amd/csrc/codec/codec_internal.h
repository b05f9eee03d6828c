// codec_internal.h -- the opaque mk_codec handle and what the codec's host files share: codec_host.cpp (the handle, the staging
// copies), bgzf_host.cpp, gzip_host.cpp, bzip2_host.cpp, zstd_host.cpp, xz_host.cpp (a format each); codec_stream.hpp has the frame of the
// four streams' entry points.  window_ingest.cpp borrows the handle's device buffers for mk_extract_fastq_bgzf, which inflates a
// window of members straight into the matcher's text buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <functional>
#include <mutex>
#include <vector>

#include "../host_common.h"
#include "bzip2_chain.hpp"
#include "gzip_chain.hpp"
#include "xz_chain.hpp"
#include "zstd_chain.hpp"

namespace mk {
int hip_fail(hipError_t e, const char *what);
int ensure_device(void **p, size_t *cap, size_t need);
}  // namespace mk

#define MKC_HIP(call, what)                                   \
    do {                                                      \
        const hipError_t e_ = (call);                         \
        if (e_ != hipSuccess) return mk::hip_fail(e_, what);  \
    } while (0)

// A device error on a decode path hands the file back (*taken stays 0, a stream's state 2), it is not the caller's error.  NOTE: the
// macro RETURNS `ret` from the function that uses it (whose handle is `c`), behind a wait for the stream: a copy may still be on its
// way into a vector of that function or of its caller
#define MKZ_HIP(call, ret)                          \
    do {                                            \
        if ((call) != hipSuccess) {                 \
            (void)hipGetLastError();                \
            (void)hipStreamSynchronize(c->stream);  \
            (void)hipGetLastError();                \
            return ret;                             \
        }                                           \
    } while (0)

struct mk_codec;

namespace mkz {
// `need` bytes in buffers of which the handle holds `held` already: what has to be added fits into half of the free memory
inline bool room(uint64_t need, uint64_t held, uint64_t free_b) { return need <= held || need - held <= free_b / 2; }
inline bool room(uint64_t need, uint64_t held) {
    size_t free_b = 0, total_b = 0;
    return hipMemGetInfo(&free_b, &total_b) == hipSuccess && room(need, held, free_b);
}
// mk::ensure_device on a path where no room is "not taken": the error is swallowed
inline bool ensure_quiet(void **p, size_t *cap, size_t need) {
    if (mk::ensure_device(p, cap, need) == MK_OK) return true;
    (void)hipGetLastError();
    return false;
}

// The two text buffers every stream owns.  The latest window's text lies in d[cur], and the handle's d_gz_text / gz_text_cap point at
// it; the next window is made in the other one, so window w's text stays valid until the call that produces window w + 2.
struct TextWindows {
    void *d[2] = {nullptr, nullptr};
    size_t cap[2] = {0, 0};
    int cur = 0;
    int other() const { return cur ^ 1; }  // the buffer the latest window does not lie in
    uint8_t *other_text() const { return (uint8_t *)d[cur ^ 1]; }
    bool ensure_other(size_t need) { return ensure_quiet(&d[cur ^ 1], &cap[cur ^ 1], need); }
    // the other buffer holds the latest window now: the handle's text is what lies `history` bytes into it (zstd: the new text behind
    // the window's history)
    inline void flip(mk_codec *c, uint64_t history = 0);
    uint64_t held() const { return cap[0] + cap[1]; }
    void free_all() {
        for (int k = 0; k < 2; ++k) {
            if (d[k]) (void)hipFree(d[k]);
            d[k] = nullptr, cap[k] = 0;
        }
    }
};
}  // namespace mkz

// The four streams (codec_stream.hpp has what their entry points share): `format` words their messages, info() is what mk_*_stream_info
// reports and what outlives the stream, text the two windows.  Symbols, tables, contexts and compressed bytes are the handle's d_gz_*.

// mk_gzip_stream_*: a gzip file in windows of its compressed bytes (gzip_host.cpp).  Beside the text, two carry buffers of 32 KiB
struct mk_gzip_stream {
    static constexpr const char *format = "gzip";
    bool active = false, dead = false;  // dead: handed back (state 2), nothing more is produced
    const uint8_t *gz = nullptr;
    uint64_t n = 0, window = 0;
    std::vector<mk_gzip_guess> guesses;  // of the whole file, once
    mkz::GzStreamPos at;                 // where the next window starts, and what the open member has so far (gzip_chain.hpp)
    uint32_t grow = 0;
    int carry_cur = 0;
    void *d_carry[2] = {nullptr, nullptr};
    mkz::TextWindows text;
    mk_gzip_stream_stats stats{};
    mk_gzip_stream_stats &info() { return stats; }
};

// mk_bzip2_stream_*: a .bz2 file in windows of its compressed bytes (bzip2_host.cpp).  What is decided about a window is mkz::BzStream's
// (bzip2_chain.hpp)
struct mk_bzip2_stream {
    static constexpr const char *format = "bzip2";
    bool active = false;
    mkz::BzStream s;
    mkz::TextWindows text;
    uint64_t n_up = 0;  // bytes of the latest upload
    size_t n_tab = 0;   // blocks the device tables of the decoded window are laid out for
    mk_bzip2_stream_stats &info() { return s.stats; }
};

// mk_zstd_stream_*: a .zst file in windows of its compressed bytes (zstd_host.cpp).  What is decided about a window is mkz::ZsStream's
// (zstd_chain.hpp).  A text buffer holds a window's history and its new text behind it
struct mk_zstd_stream {
    static constexpr const char *format = "zstd";
    bool active = false;
    mkz::ZsStream s;
    mkz::TextWindows text;
    uint64_t text_total = 0;  // history + new text of the latest window, in text.d[text.cur]
    mk_zstd_stream_stats &info() { return s.stats; }
};

// mk_xz_stream_*: an .xz file in windows of whole blocks (xz_host.cpp).  What is decided about a window is mkz::XzStream's (xz_chain.hpp:
// all windows are planned at _begin)
struct mk_xz_stream {
    static constexpr const char *format = "xz";
    bool active = false;
    mkz::XzStream s;
    mkz::TextWindows text;
    mk_xz_stream_stats &info() { return s.stats; }
};

struct mk_codec {
    int device = 0, num_cus = 256;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::mutex mu;
    // deflate: input chunk, per-block CRCs / sizes / offsets, token scratch, member slots, packed members
    // inflate: compressed chunk (d_in), member table (d_aux), text (d_out), status words (d_len)
    void *d_in = nullptr, *d_crc = nullptr, *d_tokens = nullptr, *d_slots = nullptr, *d_len = nullptr, *d_off = nullptr, *d_out = nullptr,
         *d_aux = nullptr;
    size_t in_cap = 0, crc_cap = 0, tokens_cap = 0, slots_cap = 0, len_cap = 0, off_cap = 0, out_cap = 0, aux_cap = 0;
    // members that end at record ends: the record ends (u64), and the range table the cut kernel makes of them (bgzf_host.cpp: deflate_ranges)
    void *d_ends = nullptr, *d_cut = nullptr;
    size_t ends_cap = 0, cut_cap = 0;
    float cut_ms[3] = {0, 0, 0};  // of the last such call: cut kernel, CRC-32 + deflate + pack, download
    uint64_t cut_members = 0;
    // host buffers travel through two page-locked staging buffers, filled / emptied by the host threads beside the DMA (codec_host.cpp)
    void *h_stage[2] = {nullptr, nullptr};
    hipEvent_t ev_stage[2] = {nullptr, nullptr};
    // mk_gzip_inflate_device: the compressed stream, the segments' symbols, segment tables, contexts, and the text, which stays
    // here until the next such call or mk_gzip_text_release
    void *d_gz_in = nullptr, *d_gz_sym = nullptr, *d_gz_tab = nullptr, *d_gz_ctx = nullptr, *d_gz_text = nullptr;
    size_t gz_in_cap = 0, gz_sym_cap = 0, gz_tab_cap = 0, gz_ctx_cap = 0, gz_text_cap = 0;
    uint64_t gz_text_bytes = 0;
    uint32_t gz_segments = 0;  // of the last call (diagnostic)
    float gz_ms[5] = {0, 0, 0, 0, 0};  // upload, block search, segments, resolve + translate, CRC
    // mk_bzip2_inflate_device (its text is gz_text too; compressed file, bytes in front of the run-length step, tables and pass
    // scratch borrow d_gz_in / d_gz_sym / d_gz_tab / d_gz_ctx)
    uint32_t bz_blocks = 0;
    float bz_ms[5] = {0, 0, 0, 0, 0};  // upload, marker search, block decode, text, CRC
    uint64_t bz_pass_blocks = 0;       // mk_codec_set_bzip2_pass_blocks; 0 = by the free memory
    uint64_t bz_text_cap = 0;          // mk_codec_set_bzip2_text_cap: bytes per text window of a bzip2 stream; 0 = by the free memory
    // mk_zstd_inflate_device (its text is gz_text too; compressed file, literals + sequences, tables and the two source arrays borrow
    // d_gz_in / d_gz_sym / d_gz_tab / d_gz_ctx)
    uint32_t zs_blocks = 0, zs_frames = 0, zs_rounds = 0;
    float zs_ms[6] = {0, 0, 0, 0, 0, 0};  // upload, tables + entropy decode, scans, execution, cross-block rounds, checksum
    uint64_t zs_text_cap = 0;             // mk_codec_set_zstd_text_cap: bytes of text per window of a zstd stream; 0 = by the free memory
    // mk_xz_inflate_device (xz_host.cpp; its text is gz_text too; the file and the block table borrow d_gz_in / d_gz_tab)
    uint32_t xz_blocks = 0, xz_streams = 0;
    int xz_status = 0;        // 0 = taken, else why the last call handed the file back (xz_plan.hpp, lzma_serial.hpp)
    uint64_t xz_largest = 0;  // text bytes of the file's largest block
    float xz_ms[4] = {0, 0, 0, 0};  // upload, decode, check, the whole call
    uint32_t xz_spread = 0;         // mk_codec_set_xz_spread; 0 = kXzSpreadDefault
    uint64_t xz_text_cap = 0;       // mk_codec_set_xz_text_cap: bytes of text per window of an xz stream; 0 = by the free memory
    // mk_zstd_deflate_records (zstd_host.cpp; text, record ends, range table, slots and packed frames are the deflate side's buffers above,
    // the waves' literal / sequence scratch is d_tokens)
    uint64_t zd_frames = 0;
    uint32_t zd_kinds[3] = {0, 0, 0};  // Raw, RLE, Compressed blocks of the last call
    float zd_ms[3] = {0, 0, 0};        // upload, cut + deflate + pack, download
    int inflate_kernel = 0;  // mk_codec_set_inflate_kernel: 0 = chosen per call, 1 = a lane per member, 2 = a wave per member
    float ms[3] = {0, 0, 0};
    uint64_t gzip_chunk = 0;  // mk_codec_set_gzip_chunk; 0 = by the stream's size
    uint64_t deflate_pass_blocks = 0, inflate_pass_text = 0;  // mk_codec_set_pass_limits; 0 = the defaults below
    mk_gzip_stream gzs;
    mk_bzip2_stream bzs;
    mk_zstd_stream zss;
    mk_xz_stream xzs;
    bool stream_open() const { return gzs.active || bzs.active || zss.active || xzs.active; }  // one stream per handle, and no one-shot call beside it
};

inline void mkz::TextWindows::flip(mk_codec *c, uint64_t history) {
    cur ^= 1;
    c->d_gz_text = d[cur] ? (uint8_t *)d[cur] + history : nullptr;
    c->gz_text_cap = d[cur] ? cap[cur] - history : 0;
}

namespace mkz {
// What every call that may not run beside a stream says (the one-shot calls, the four _begin, the frame writers)
constexpr const char *kOpenStream = "the handle has an open stream (mk_gzip_stream_end, mk_bzip2_stream_end, mk_zstd_stream_end, mk_xz_stream_end)";
inline int refuse_open_stream(const char *entry) { return mk::fail(MK_E_INVALID_ARG, "%s: %s", entry, kOpenStream); }
// whichever stream is open ends, with its text buffers (which are what d_gz_text points at) and the handle's scratch (codec_host.cpp)
void streams_close(mk_codec *c);
// ---- codec_host.cpp: host buffers <-> device through the handle's two page-locked staging buffers
void parallel_copy(uint8_t *dst, const uint8_t *src, uint64_t n);
// src[0, n) -> d_dst, enqueued on the handle's stream; the host side of it is done when this returns
int upload(mk_codec *c, void *d_dst, const uint8_t *src, uint64_t n);
// d_src[0, n) -> dst; waits for the stream (everything enqueued before it included)
int download(mk_codec *c, uint8_t *dst, const void *d_src, uint64_t n);
// d_src[0, n) handed to `each` piece by piece, in order, out of the staging buffers: piece k + 1 travels while `each` works on piece k
int download_each(mk_codec *c, const void *d_src, uint64_t n, const std::function<void(const uint8_t *, uint64_t)> &each);
double now_ms();
inline float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
}
// ---- gzip_host.cpp: the buffers of the gzip / bzip2 paths.  gz_release: all five and their caps (the text included: gz_text_bytes = 0).
// gz_keep_text: what is left to keep is the text -- the compressed bytes, the symbols and the contexts go back to the device.
void gz_release(mk_codec *c);
void gz_keep_text(mk_codec *c);
// ---- zstd_host.cpp
// zd_frames, zd_kinds and zd_ms back to 0: what mk_zstd_deflate_info reports starts again
void zstd_deflate_reset(mk_codec *c);
// d_text[0, n_text) (kPad ZERO bytes behind it) whose records end at d_ends[0, n_ends) (device memory, non-decreasing, the last one =
// n_text) -> the zstd frames of the cut rule (include/merkurio_hip.h), cut, compressed and packed on stream st in passes, downloaded to
// out as long as they fit out_cap: *need = the bytes of all of them (> out_cap: the caller reports MK_E_CAPACITY), *frames how many.
// ADDS to zd_frames, zd_kinds, zd_ms[1] and zd_ms[2].  The caller holds c->mu, with c->device current
int zstd_deflate_ranges(mk_codec *c, hipStream_t st, const uint8_t *d_text, uint64_t n_text, const unsigned long long *d_ends, uint64_t n_ends, uint8_t *out,
                        uint64_t out_cap, uint64_t *need, uint64_t *frames);
// ---- bgzf_host.cpp
// One device pass of the deflate side, shared by everything that writes members from text that lies on the device (the tag windows'
// output side, mk_bgzf_deflate_records): CRC-32, deflate and pack of `blocks` members of d_text on
// stream st, with the codec's buffers (the caller holds c->mu).  Member b = d_text[b * bb ...] (off == nullptr; the last one ends at
// n_text) or d_text[off[b], off[b] + len[b]) (device tables).  The members land back to back in d_packed when packed_cap holds
// their bound, in c->d_out otherwise: *d_members says where, *total how many bytes (the stream has been waited for).
int deflate_pass(mk_codec *c, hipStream_t st, const uint8_t *d_text, uint64_t n_text, uint32_t bb, const unsigned long long *off, const uint32_t *len,
                 uint32_t blocks, void *d_packed, size_t packed_cap, void **d_members, uint64_t *total);
// d_text[0, n_text) (kPad readable bytes behind it) whose records end at d_ends[0, n_ends) (device memory, non-decreasing, the last one
// = n_text) -> the members of the cut rule (include/merkurio_hip.h), cut and deflated in passes, downloaded to out as long as they
// fit out_cap: *need = the bytes of all of them (> out_cap: the caller reports MK_E_CAPACITY), *n_members how many.  Sets c->cut_ms.
int deflate_ranges(mk_codec *c, hipStream_t st, const uint8_t *d_text, uint64_t n_text, const unsigned long long *d_ends, uint64_t n_ends, void *d_packed,
                   size_t packed_cap, uint8_t *out, uint64_t out_cap, uint64_t *need, uint64_t *n_members);
}  // namespace mkz
