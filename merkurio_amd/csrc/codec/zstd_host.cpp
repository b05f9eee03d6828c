// zstd_host.cpp -- host side of mk_zstd_inflate_device and mk_zstd_stream_* (include/merkurio_hip.h): a .zst file decoded on the
// device, a wave per block -- the whole file in one call, or a file of any size window by window.  The walk over the frames and block
// headers is mkz::zs_walk, the two scans mkz::zs_scan (zstd_plan.hpp), everything that is decided about a window zstd_chain.hpp's;
// none of them has HIP in it and the CPU harnesses of the tests run them; kernels: zstd_inflate.hip.  Here: the three device steps
// both entry points share -- upload + tables + entropy decode; execution + the rounds of cross-block resolution; the content checksum,
// which the host computes over the text as it comes down through the staging buffers (XXH64 is four serial chains: nothing for a
// wave to fold) -- and the calls around them.  The buffers are the gzip path's (codec_internal.h).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../host_common.h"
#include "codec_kernels.h"
#include "codec_stream.hpp"
#include "xxh64.hpp"
#include "zstd_plan.hpp"

using mkz::elapsed;
using mkz::now_ms;

namespace {

uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

// the device tables of B blocks behind each other: blocks | reports | starts | status | two counters
struct ZsTab {
    uint64_t o_rep, o_start, o_status, o_count, bytes;
    explicit ZsTab(size_t B) {
        o_rep = up16(B * sizeof(mkz::ZsBlock)), o_start = o_rep + up16(B * sizeof(mkz::ZsReport)), o_status = o_start + up16(B * sizeof(mkz::ZsStart));
        o_count = o_status + up16(B * 4), bytes = o_count + 64;
    }
};
// literals | LL | ML | OF of a plan inside d_gz_sym
struct ZsSym {
    uint64_t lit_bytes, seq_bytes;
    explicit ZsSym(const mkz::ZsPlan &P) : lit_bytes(up16(P.lit_bytes + 16)), seq_bytes(up16((P.n_seq + 4) * 4)) {}
    uint64_t bytes() const { return lit_bytes + 3 * seq_bytes; }
};

// ---- step 1: the device's input is pre[0, n_pre) | zs[0, n) (zeros behind it up to the reader's pad), which the positions of P's
// blocks count in; tables + entropy decode of all of them -> rep.  false: no room, a device error.  ms[0], ms[1]
bool zs_decode(mk_codec *c, const uint8_t *pre, uint64_t n_pre, const uint8_t *zs, uint64_t n, const mkz::ZsPlan &P, std::vector<mkz::ZsReport> &rep, float *ms) {
    const size_t B = P.blocks.size();
    double t0 = now_ms();
    const uint64_t n_in = n_pre + n, n_words = (n_in + mkz::kZsStreamPad + 3) / 4;
    const ZsSym sym(P);
    const ZsTab t(B);
    if (!mkz::room(n_words * 4 + sym.bytes() + t.bytes, c->gz_in_cap + c->gz_sym_cap + c->gz_tab_cap) || !mkz::ensure_quiet(&c->d_gz_in, &c->gz_in_cap, n_words * 4) ||
        !mkz::ensure_quiet(&c->d_gz_sym, &c->gz_sym_cap, sym.bytes()) || !mkz::ensure_quiet(&c->d_gz_tab, &c->gz_tab_cap, t.bytes))
        return false;
    if (n_pre) MKZ_HIP(hipMemcpyAsync(c->d_gz_in, pre, n_pre, hipMemcpyHostToDevice, c->stream), false);
    if (mkz::upload(c, (uint8_t *)c->d_gz_in + n_pre, zs, n)) return false;
    MKZ_HIP(hipMemsetAsync((uint8_t *)c->d_gz_in + n_in, 0, n_words * 4 - n_in, c->stream), false);
    uint8_t *tab = (uint8_t *)c->d_gz_tab;
    MKZ_HIP(hipMemcpyAsync(tab, P.blocks.data(), B * sizeof(mkz::ZsBlock), hipMemcpyHostToDevice, c->stream), false);
    MKZ_HIP(hipStreamSynchronize(c->stream), false);
    ms[0] += (float)(now_ms() - t0);
    uint8_t *lit = (uint8_t *)c->d_gz_sym;
    uint32_t *ll = (uint32_t *)(lit + sym.lit_bytes), *ml = (uint32_t *)(lit + sym.lit_bytes + sym.seq_bytes), *of = (uint32_t *)(lit + sym.lit_bytes + 2 * sym.seq_bytes);
    MKZ_HIP(hipEventRecord(c->ev[0], c->stream), false);
    mkz::launch_zs_decode((const uint8_t *)c->d_gz_in, n_in, n_words, tab, (uint32_t)B, lit, ll, ml, of, tab + t.o_rep, c->stream);
    MKZ_HIP(hipGetLastError(), false);
    MKZ_HIP(hipEventRecord(c->ev[1], c->stream), false);
    rep.resize(B);
    MKZ_HIP(hipMemcpyAsync(rep.data(), tab + t.o_rep, B * sizeof(mkz::ZsReport), hipMemcpyDeviceToHost, c->stream), false);
    MKZ_HIP(hipStreamSynchronize(c->stream), false);
    ms[1] += elapsed(c->ev[0], c->ev[1]);
    return true;
}

// ---- step 2: the decoded blocks executed from start[] into d_text[0, total) (128 bytes of room behind it), and one source per byte
// in two arrays (a round reads one and writes the other); d_text[0, settled) is final: d_hist[0, settled) copied there first (a
// stream's history; the one-shot call: none), and the rounds of pointer doubling visit [settled, total) until one leaves nothing
// open -> *rounds.  false: a block's status, more rounds than the cap, no room, a device error.  ms[3], ms[4]
bool zs_text(mk_codec *c, const mkz::ZsPlan &P, const std::vector<mkz::ZsStart> &start, uint8_t *d_text, const uint8_t *d_hist, uint64_t settled, uint64_t total,
             uint32_t *rounds, float *ms) {
    const size_t B = P.blocks.size();
    *rounds = 0;
    if (settled) MKZ_HIP(hipMemcpyAsync(d_text, d_hist, settled, hipMemcpyDeviceToDevice, c->stream), false);
    if (!B) {
        MKZ_HIP(hipStreamSynchronize(c->stream), false);
        return true;
    }
    const ZsSym sym(P);
    const ZsTab t(B);
    const uint64_t src_bytes = up16(total * 4 + 16);
    if (!mkz::room(2 * src_bytes, c->gz_ctx_cap) || !mkz::ensure_quiet(&c->d_gz_ctx, &c->gz_ctx_cap, 2 * src_bytes)) return false;
    uint8_t *tab = (uint8_t *)c->d_gz_tab, *lit = (uint8_t *)c->d_gz_sym;
    uint32_t *ll = (uint32_t *)(lit + sym.lit_bytes), *ml = (uint32_t *)(lit + sym.lit_bytes + sym.seq_bytes), *of = (uint32_t *)(lit + sym.lit_bytes + 2 * sym.seq_bytes);
    uint32_t *src[2] = {(uint32_t *)c->d_gz_ctx, (uint32_t *)((uint8_t *)c->d_gz_ctx + src_bytes)};
    unsigned long long *d_open = (unsigned long long *)(tab + t.o_count);
    MKZ_HIP(hipMemcpyAsync(tab + t.o_start, start.data(), B * sizeof(mkz::ZsStart), hipMemcpyHostToDevice, c->stream), false);
    MKZ_HIP(hipMemsetAsync(d_open, 0, 8, c->stream), false);
    MKZ_HIP(hipEventRecord(c->ev[0], c->stream), false);
    if (settled) {  // (kZsResolved is all ones)
        MKZ_HIP(hipMemsetAsync(src[0], 0xff, settled * 4, c->stream), false);
        MKZ_HIP(hipMemsetAsync(src[1], 0xff, settled * 4, c->stream), false);
    }
    mkz::launch_zs_execute((const uint8_t *)c->d_gz_in, tab, tab + t.o_start, tab + t.o_rep, (uint32_t)B, lit, ll, ml, of, d_text, src[0], settled,
                           (int32_t *)(tab + t.o_status), d_open, c->stream);
    MKZ_HIP(hipGetLastError(), false);
    MKZ_HIP(hipEventRecord(c->ev[1], c->stream), false);
    std::vector<int32_t> status(B);
    unsigned long long open = 0;
    MKZ_HIP(hipMemcpyAsync(status.data(), tab + t.o_status, B * 4, hipMemcpyDeviceToHost, c->stream), false);
    MKZ_HIP(hipMemcpyAsync(&open, d_open, 8, hipMemcpyDeviceToHost, c->stream), false);
    MKZ_HIP(hipStreamSynchronize(c->stream), false);
    ms[3] += elapsed(c->ev[0], c->ev[1]);
    for (int32_t st : status)
        if (st != 0) return false;
    // ---- cross-block resolution: rounds of pointer doubling until one leaves nothing open
    const double t0 = now_ms();
    const uint32_t cap = mkz::zs_round_cap(B);
    int cur = 0;
    while (open) {
        if (*rounds == cap) return false;
        MKZ_HIP(hipMemsetAsync(d_open, 0, 8, c->stream), false);
        mkz::launch_zs_resolve(src[cur], src[cur ^ 1], d_text, settled, total, d_open, c->num_cus, c->stream);
        MKZ_HIP(hipGetLastError(), false);
        MKZ_HIP(hipMemcpyAsync(&open, d_open, 8, hipMemcpyDeviceToHost, c->stream), false);
        MKZ_HIP(hipStreamSynchronize(c->stream), false);
        cur ^= 1, ++*rounds;
    }
    ms[4] += (float)(now_ms() - t0);
    return true;
}

// ---- step 3: d_text[0, len) comes down through h.  ms[5]
bool zs_hash(mk_codec *c, const uint8_t *d_text, uint64_t len, mkz::Xxh64 &h, float *ms) {
    const double t0 = now_ms();
    if (len && mkz::download_each(c, d_text, len, [&](const uint8_t *p, uint64_t m) { h.update(p, m); })) {
        (void)hipGetLastError();
        return false;
    }
    ms[5] += (float)(now_ms() - t0);
    return true;
}

// the whole file in one call; false: not taken
bool zstd_inflate(mk_codec *c, const uint8_t *zs, uint64_t n, uint64_t *text_bytes, uint64_t *n_blocks) {
    mkz::ZsPlan P;
    if (!mkz::zs_plan(zs, n, P)) return false;
    const size_t B = P.blocks.size();
    uint64_t total = 0;
    uint32_t rounds = 0;
    if (B) {
        if (B >= (1u << 30)) return false;
        MKZ_HIP(hipSetDevice(c->device), false);
        std::vector<mkz::ZsReport> rep;
        if (!zs_decode(c, nullptr, 0, zs, n, P, rep, c->zs_ms)) return false;
        for (const mkz::ZsReport &r : rep)
            if (r.status != 0) return false;
        // ---- the two scans: where every block's text starts, the repeat offsets in front of it
        const double t0 = now_ms();
        std::vector<mkz::ZsStart> start;
        if (!mkz::zs_scan(P, rep, start, &total)) return false;
        c->zs_ms[2] = (float)(now_ms() - t0);
        // ---- execution and rounds: the text, 8 bytes of sources per byte beside it
        if (!mkz::room(total + 128 + 2 * up16(total * 4 + 16), c->gz_text_cap + c->gz_ctx_cap) || !mkz::ensure_quiet(&c->d_gz_text, &c->gz_text_cap, total + 128)) return false;
        if (!zs_text(c, P, start, (uint8_t *)c->d_gz_text, nullptr, 0, total, &rounds, c->zs_ms)) return false;
        // ---- content checksums: the low 32 bits of XXH64 of every frame's text that carries one
        for (const mkz::ZsFrame &F : P.frames) {
            if (!F.has_checksum) continue;
            mkz::Xxh64 h;
            if (!zs_hash(c, (const uint8_t *)c->d_gz_text + F.text_off, F.text_len, h, c->zs_ms)) return false;
            if ((uint32_t)h.digest() != F.checksum) return false;
        }
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

// ---- the device behind a stream (zstd_chain.hpp: Dev)
struct ZsStreamDev {
    mk_codec *c;
    mk_zstd_stream &D;
    uint64_t text_room() { return default_text_cap(c); }
    // per text byte of a window: the byte in each of the two text buffers and two 4-byte sources -- a tenth of half of the free
    // memory, an unmeasured choice (profiles/e2e_unzstd_windows.txt)
    static uint64_t default_text_cap(const mk_codec *c) {
        if (c->zs_text_cap) return c->zs_text_cap;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return mkz::kZsBlockMax;
        return std::min<uint64_t>(free_b / 2 / 10, mkz::kZsTextCapMax);
    }
    bool decode(const mkz::ZsWindow &W, std::vector<mkz::ZsReport> &rep) {
        return zs_decode(c, W.prelude, mkz::kZsPrelude, D.s.zs + W.from, W.to - W.from, W.P, rep, D.s.stats.ms);
    }
    bool execute(const mkz::ZsWindow &W, const std::vector<mkz::ZsStart> &start, uint64_t history, uint64_t total, uint32_t *rounds) {
        if (history > D.text_total) return false;
        if (!mkz::room(total + 128 + 2 * up16(total * 4 + 16), D.text.cap[D.text.other()] + c->gz_ctx_cap) || !D.text.ensure_other(total + 128)) return false;
        const uint8_t *hist = history ? (const uint8_t *)D.text.d[D.text.cur] + (D.text_total - history) : nullptr;
        return zs_text(c, W.P, start, D.text.other_text(), hist, history, total, rounds, D.s.stats.ms);
    }
    bool hash(uint64_t off, uint64_t len, mkz::Xxh64 &h) { return zs_hash(c, D.text.other_text() + off, len, h, D.s.stats.ms); }
    void commit(uint64_t history, uint64_t total) { D.text.flip(c, history), D.text_total = total; }
};

}  // namespace

namespace mkz {

void zstd_deflate_reset(mk_codec *c) {
    c->zd_frames = 0;
    for (int k = 0; k < 3; ++k) c->zd_kinds[k] = 0, c->zd_ms[k] = 0;
}

// d_text[0, n_text) (kPad ZERO bytes behind it: the deflate kernel reads 16 at a time) whose records end at d_ends[0, n_ends) (device
// memory, non-decreasing, the last one = n_text) -> the frames of the cut rule (include/merkurio_hip.h, mk_zstd_record_cuts), cut,
// compressed and packed on stream st in passes of frames.  *need = the bytes of all frames, *frames how many.  A pass's frames are
// downloaded to out as long as everything so far has fitted out_cap: *need > out_cap means out holds only the passes in front of the
// one that did not fit (the caller reports MK_E_CAPACITY).  ADDS to c->zd_frames, c->zd_kinds and c->zd_ms[1], [2] (cut + deflate +
// pack, download): a caller with several texts per call (the two sources of a paired window) resets them once (zstd_deflate_reset).
// The caller holds c->mu and has made c->device current.  (Shared with mk_extract_window_frames, extract_window.cpp: the ends are then
// the offsets scan of a window's written lengths, where a record that is not kept repeats the end in front of it.)
int zstd_deflate_ranges(mk_codec *c, hipStream_t st, const uint8_t *d_text, uint64_t n_text, const unsigned long long *d_ends, uint64_t n_ends, uint8_t *out,
                        uint64_t out_cap, uint64_t *need, uint64_t *frames_out) {
    *need = 0, *frames_out = 0;
    if (!n_text) return MK_OK;
    const uint64_t grid64 = (n_text + kZsCutGrid - 1) / kZsCutGrid;
    if (grid64 >= 0x7FFFFFFFull) return mk::fail(MK_E_UNSUPPORTED, "%llu output frames", (unsigned long long)grid64);
    const uint32_t n_grid = (uint32_t)grid64;
    int rc;
    // the range table: count | kinds[3] | off[n_grid] | len[n_grid]
    if ((rc = mk::ensure_device(&c->d_cut, &c->cut_cap, 16 + n_grid * 12ull))) return rc;
    uint32_t *d_count = (uint32_t *)c->d_cut, *d_kinds = d_count + 1;
    unsigned long long *d_off = (unsigned long long *)((uint8_t *)c->d_cut + 16);
    uint32_t *d_len = (uint32_t *)(d_off + n_grid);
    double t0 = now_ms();
    MKC_HIP(hipMemsetAsync(c->d_cut, 0, 16, st), "hipMemsetAsync");
    launch_zstd_cuts(d_ends, n_ends, n_text, n_grid, d_off, d_len, d_count, st);
    uint32_t frames = 0;
    MKC_HIP(hipGetLastError(), "the cut kernel");
    MKC_HIP(hipMemcpyAsync(&frames, d_count, 4, hipMemcpyDeviceToHost, st), "download of the frame count");
    MKC_HIP(hipStreamSynchronize(st), "the cut kernel");
    if (frames > n_grid || frames + 1 < n_grid) return mk::fail(MK_E_HIP, "the cut kernel reports %u frames of %u grid points", frames, n_grid);
    c->zd_ms[1] += (float)(now_ms() - t0);
    // passes of frames; a pass is downloaded as long as everything so far has fitted.  4 096 frames by default: 0.54 GB of slots (131 328 B
    // each) beside the resident waves' scratch (8 per CU x 1 005 376 B: 2.06 GB on 256 CUs once a pass has that many frames)
    const uint64_t pass = std::min<uint64_t>(c->deflate_pass_blocks ? c->deflate_pass_blocks : 4096, 0x7FFFFFFFu);
    uint64_t written = 0;
    bool fits = true;
    for (uint64_t f0 = 0; f0 < frames; f0 += pass) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(pass, frames - f0);
        const uint32_t grid = zstd_deflate_grid(cnt, c->num_cus);
        const uint64_t bound = std::min<uint64_t>((uint64_t)cnt * kZsBlockMax, n_text) + cnt * 16ull;
        if ((rc = mk::ensure_device(&c->d_tokens, &c->tokens_cap, (uint64_t)grid * kZsDeflateWaveScratch)) ||
            (rc = mk::ensure_device(&c->d_slots, &c->slots_cap, (uint64_t)cnt * kZsDeflateSlotBytes)) ||
            (rc = mk::ensure_device(&c->d_len, &c->len_cap, (cnt + 1) * 4ull)) || (rc = mk::ensure_device(&c->d_off, &c->off_cap, (cnt + 2) * 8ull)) ||
            (rc = mk::ensure_device(&c->d_out, &c->out_cap, bound)))
            return rc;
        uint64_t *d_total = (uint64_t *)c->d_off + cnt;
        t0 = now_ms();
        launch_zstd_deflate(d_text, d_off + f0, d_len + f0, cnt, (uint8_t *)c->d_tokens, (uint8_t *)c->d_slots, (uint32_t *)c->d_len, (uint32_t *)(d_total + 1),
                            d_kinds, grid, st);
        launch_zstd_pack((const uint8_t *)c->d_slots, (const uint32_t *)c->d_len, (uint64_t *)c->d_off, d_total, cnt, (uint8_t *)c->d_out, st);
        uint64_t total = 0;
        MKC_HIP(hipGetLastError(), "zstd deflate kernels");
        MKC_HIP(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st), "download of the size");
        MKC_HIP(hipStreamSynchronize(st), "zstd deflate on the device");
        c->zd_ms[1] += (float)(now_ms() - t0);
        if (total > bound) return mk::fail(MK_E_HIP, "zstd frames exceed their bound (internal error)");
        fits = fits && written + total <= out_cap;
        if (fits && total) {  // (st has been waited for: the packed frames are final, whichever stream carries them down)
            t0 = now_ms();
            if ((rc = download(c, out + written, c->d_out, total))) return rc;
            c->zd_ms[2] += (float)(now_ms() - t0);
        }
        written += total;
    }
    uint32_t kinds[3] = {0, 0, 0};
    MKC_HIP(hipMemcpyAsync(kinds, d_kinds, 12, hipMemcpyDeviceToHost, st), "download of the block kinds");
    MKC_HIP(hipStreamSynchronize(st), "download of the block kinds");
    for (int k = 0; k < 3; ++k) c->zd_kinds[k] += kinds[k];
    c->zd_frames += frames;
    *need = written, *frames_out = frames;
    return MK_OK;
}

}  // namespace mkz

extern "C" {

int mk_zstd_inflate_device(mk_codec *c, const uint8_t *zs, uint64_t n, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_blocks) {
    MK_ABI_BEGIN
    if (!c || !text_bytes || !taken || !n_blocks || (n && !zs)) return mk::fail(MK_E_INVALID_ARG, "mk_zstd_inflate_device: NULL argument");
    *text_bytes = 0, *taken = 0, *n_blocks = 0;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->stream_open()) return mkz::refuse_open_stream("mk_zstd_inflate_device");
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

// ---- a .zst file of any size, window by window

int mk_zstd_stream_begin(mk_codec *c, const uint8_t *zs, uint64_t n, uint64_t window_bytes, uint32_t *taken) {
    MK_ABI_BEGIN
    if (!c || !taken || (n && !zs)) return mk::fail(MK_E_INVALID_ARG, "mk_zstd_stream_begin: NULL argument");
    *taken = 0;
    if (window_bytes > (1ull << 40)) return mk::fail(MK_E_INVALID_ARG, "mk_zstd_stream_begin: a window of 1 TiB at most");
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->stream_open()) return mkz::refuse_open_stream("mk_zstd_stream_begin");
    mkz::ZsStream s;
    if (!mkz::zs_stream_open(s, zs, n, window_bytes)) return MK_OK;  // (not a zstd file)
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    mkz::gz_release(c);  // the one-shot text of an earlier call goes: d_gz_text is the stream's from here on
    c->zs_blocks = c->zs_frames = c->zs_rounds = 0;
    c->zss = mk_zstd_stream();
    c->zss.s = s, c->zss.active = true;
    c->zss.s.text_cap = ZsStreamDev::default_text_cap(c);  // (once: a stream's windows do not move with the free memory)
    *taken = 1;
    return MK_OK;
    MK_ABI_END
}

int mk_zstd_stream_next(mk_codec *c, uint64_t *text_bytes, uint32_t *state) {
    return mkz::chain_stream_next(c, &mk_codec::zss, text_bytes, state, [&](mk_zstd_stream &D) {
        ZsStreamDev dev{c, D};
        const float *ms = D.s.stats.ms;
        const double t0 = now_ms();
        const float in_steps = ms[0] + ms[1] + ms[3] + ms[4] + ms[5];
        mkz::zs_stream_next(D.s, dev, text_bytes, state);
        // (scans: what the window's call spent on the host outside the device steps -- the walk and the two scans)
        D.s.stats.ms[2] += std::max(0.f, (float)(now_ms() - t0) - (ms[0] + ms[1] + ms[3] + ms[4] + ms[5] - in_steps));
    });
}

int mk_zstd_stream_info(const mk_codec *c, mk_zstd_stream_stats *out) { return mkz::stream_info(c, &mk_codec::zss, out); }

int mk_zstd_stream_end(mk_codec *c) { return mkz::stream_end(c, &mk_codec::zss); }

// ---- zstd frames written on the device (zstd_deflate.hip): the kept records of `extract` as a .zst file, one frame per cut

int mk_zstd_record_cuts(const uint64_t *rec_end, uint64_t n_rec, uint64_t *cut, uint64_t cap, uint64_t *n_cuts) {
    if (!n_cuts || (n_rec && !rec_end) || (cap && !cut)) return mk::fail(MK_E_INVALID_ARG, "mk_zstd_record_cuts: NULL argument");
    *n_cuts = 0;
    for (uint64_t r = 1; r < n_rec; ++r)
        if (rec_end[r] < rec_end[r - 1]) return mk::fail(MK_E_INVALID_ARG, "mk_zstd_record_cuts: record end %llu lies in front of the one before it", (unsigned long long)r);
    const uint64_t k = mkz::zstd_record_cuts(rec_end, n_rec, cut, cap);
    *n_cuts = k;
    if (k > cap) return mk::fail(MK_E_CAPACITY, "mk_zstd_record_cuts: %llu cuts, room for %llu", (unsigned long long)k, (unsigned long long)cap);
    return MK_OK;
}

uint64_t mk_zstd_deflate_bound(uint64_t n) { return n + 16 * (n / mkz::kZsCutGrid + 2); }  // a frame of a Raw block: 16 bytes + its text

int mk_zstd_deflate_records(mk_codec *c, const uint8_t *text, uint64_t n, const uint64_t *rec_end, uint64_t n_rec, uint8_t *out, uint64_t out_cap,
                            uint64_t *out_len, uint64_t *n_frames) {
    MK_ABI_BEGIN
    if (!c || !out_len || !n_frames || (n && (!text || !rec_end)) || (out_cap && !out)) return mk::fail(MK_E_INVALID_ARG, "mk_zstd_deflate_records: NULL argument");
    *out_len = 0, *n_frames = 0;
    if ((n_rec ? rec_end[n_rec - 1] : 0) != n) return mk::fail(MK_E_INVALID_ARG, "mk_zstd_deflate_records: the last record does not end where the text does");
    for (uint64_t r = 1; r < n_rec; ++r)
        if (rec_end[r] < rec_end[r - 1]) return mk::fail(MK_E_INVALID_ARG, "mk_zstd_deflate_records: record end %llu lies in front of the one before it", (unsigned long long)r);
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->stream_open()) return mkz::refuse_open_stream("mk_zstd_deflate_records");
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    mkz::zstd_deflate_reset(c);
    if (!n) return MK_OK;
    int rc;
    if ((rc = mk::ensure_device(&c->d_in, &c->in_cap, n + mkz::kPad)) || (rc = mk::ensure_device(&c->d_ends, &c->ends_cap, n_rec * 8ull))) return rc;
    const double t0 = mkz::now_ms();
    if ((rc = mkz::upload(c, c->d_in, text, n)) || (rc = mkz::upload(c, c->d_ends, (const uint8_t *)rec_end, n_rec * 8ull))) return rc;
    MKC_HIP(hipMemsetAsync((uint8_t *)c->d_in + n, 0, mkz::kPad, c->stream), "hipMemsetAsync");
    MKC_HIP(hipStreamSynchronize(c->stream), "upload of the text");
    c->zd_ms[0] = (float)(mkz::now_ms() - t0);
    uint64_t need = 0;
    if ((rc = mkz::zstd_deflate_ranges(c, c->stream, (const uint8_t *)c->d_in, n, (const unsigned long long *)c->d_ends, n_rec, out, out_cap, &need, n_frames))) return rc;
    *out_len = need;
    if (need > out_cap) return mk::fail(MK_E_CAPACITY, "mk_zstd_deflate_records: the frames take %llu bytes, room for %llu", (unsigned long long)need, (unsigned long long)out_cap);
    return MK_OK;
    MK_ABI_END
}

int mk_zstd_deflate_info(const mk_codec *c, uint64_t *n_frames, uint32_t kinds[3], float ms[3]) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_zstd_deflate_info: NULL handle");
    if (n_frames) *n_frames = c->zd_frames;
    for (int k = 0; k < 3; ++k) {
        if (kinds) kinds[k] = c->zd_kinds[k];
        if (ms) ms[k] = c->zd_ms[k];
    }
    return MK_OK;
}

}  // extern "C"
