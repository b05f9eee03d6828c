// bzip2_host.cpp -- host side of mk_bzip2_inflate_device and mk_bzip2_stream_* (include/merkurio_hip.h): a .bz2 file decoded on the
// device, a wave per block -- the whole file in one call, or a file of any size window by window.  The walk over a file's table of
// magics is mkz::bz2_plan (bzip2_stream.hpp), everything that is decided about a window is bzip2_chain.hpp's, which has no HIP in it
// and runs on the CPU in the tests; kernels: bzip2_inflate.hip.  Here: the three device steps both entry points share -- upload +
// marker search, decode + walk in passes, expansion + CRC of a range of blocks -- and the calls around them.  The buffers are the gzip
// path's (codec_internal.h).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../host_common.h"
#include "bzip2_chain.hpp"
#include "codec_kernels.h"
#include "codec_stream.hpp"

using mkz::elapsed;
using mkz::now_ms;
using mkz::upload;

namespace {

constexpr uint32_t kBzMaxMarkers = 1u << 20;  // candidates of one file; more = not taken (900 kB blocks: 1 Mi of them are ~1 TB of text)
constexpr uint64_t kBzMaxPassBlocks = 4096;

// the device tables of B blocks behind each other: bit | pre_off | text_off | text_len (u64) | reports | level | crc (u32)
struct BzTab {
    unsigned long long *bit, *pre, *toff, *tlen;
    mkz::Bz2Block *rep;
    uint32_t *level, *crc;
    static size_t bytes(size_t B) { return B * (8 * 4 + 4 * 2 + sizeof(mkz::Bz2Block)) + 64; }
    BzTab(void *d, size_t B) {
        bit = (unsigned long long *)d, pre = bit + B, toff = pre + B, tlen = toff + B;
        rep = (mkz::Bz2Block *)(tlen + B);
        level = (uint32_t *)(rep + B), crc = level + B;
    }
};
// a block's room in front of the run-length step: its symbols as bytes (later: the bytes the walk leaves) and a bit per byte
uint64_t bz_pre_bytes(uint32_t level) {
    const uint64_t cap = (level * 100000ull + 127) & ~127ull;
    return cap + cap / 8;
}
uint64_t bz_slot_bytes(uint32_t level) { return mkz::kBzSelBytes + 4 * ((level * 100000ull + 127) & ~127ull); }

// ---- step 1: up[0, n) goes up (zeros behind it up to the reader's pad), every bit offset is tested for the two magics -> the hits
// that lie whole inside it, sorted, bits of the upload.  false: no room, more than `cap` of them, a device error.  ms[0], ms[1]
bool bz_upload_and_search(mk_codec *c, const uint8_t *up, uint64_t n, uint32_t cap, std::vector<mkz::BzMarker> &markers, float *ms) {
    double t0 = now_ms();
    const uint64_t n_words = (n + mkz::kBzStreamPad + 3) / 4;
    if (!mkz::room(n_words * 4 + cap * 8ull + 64, c->gz_in_cap + c->gz_tab_cap) || !mkz::ensure_quiet(&c->d_gz_in, &c->gz_in_cap, n_words * 4) ||
        !mkz::ensure_quiet(&c->d_gz_tab, &c->gz_tab_cap, cap * 8ull + 64))
        return false;
    if (upload(c, c->d_gz_in, up, n)) return false;
    MKZ_HIP(hipMemsetAsync((uint8_t *)c->d_gz_in + n, 0, n_words * 4 - n, c->stream), false);
    MKZ_HIP(hipStreamSynchronize(c->stream), false);
    ms[0] += (float)(now_ms() - t0);
    t0 = now_ms();
    unsigned long long *d_markers = (unsigned long long *)c->d_gz_tab;
    uint32_t *d_count = (uint32_t *)(d_markers + cap);
    MKZ_HIP(hipMemsetAsync(d_count, 0, 4, c->stream), false);
    mkz::launch_bz2_markers((const uint8_t *)c->d_gz_in, n, n_words, d_markers, cap, d_count, c->num_cus, c->stream);
    MKZ_HIP(hipGetLastError(), false);
    uint32_t count = 0;
    MKZ_HIP(hipMemcpyAsync(&count, d_count, 4, hipMemcpyDeviceToHost, c->stream), false);
    MKZ_HIP(hipStreamSynchronize(c->stream), false);
    if (count > cap) return false;
    std::vector<unsigned long long> raw(count);
    if (count) MKZ_HIP(hipMemcpyAsync(raw.data(), d_markers, count * 8ull, hipMemcpyDeviceToHost, c->stream), false);
    MKZ_HIP(hipStreamSynchronize(c->stream), false);
    std::sort(raw.begin(), raw.end());
    markers.resize(count);
    for (uint32_t k = 0; k < count; ++k) markers[k] = mkz::BzMarker{raw[k] >> 1, (uint32_t)(raw[k] & 1u)};
    ms[1] += (float)(now_ms() - t0);
    return true;
}

// ---- step 2: blocks [0, B) of the upload of n bytes, block k's magic at bit[k] of a stream of level[k], decoded and walked in
// passes -> rep, text_len of blocks [0, *done).  Per block: its bytes in front of the run-length step, kept for all blocks until the
// text is written; selectors and the 4-byte vector per block of a pass.  prefix: where the device has no room for all B, the
// largest prefix of them that fits is decoded (else: false).  The proof of a guess -- the block ends exactly on end_bit[k], the
// magic behind it -- is checked pass by pass: the passes behind the first block that fails it are not run (*done = the end of its
// pass).  *n_tab: how many blocks the device tables are laid out for (BzTab).  false: no room, a device error.  ms[2], ms[3]
bool bz_decode(mk_codec *c, uint64_t n, size_t B, const unsigned long long *bit, const uint32_t *level, const unsigned long long *end_bit, bool prefix,
               std::vector<mkz::Bz2Block> &rep, std::vector<unsigned long long> &text_len, float *ms, size_t *n_tab, size_t *done) {
    *done = 0, *n_tab = 0;
    const uint64_t n_words = (n + mkz::kBzStreamPad + 3) / 4;
    size_t free_b = 0, total_b = 0;
    MKZ_HIP(hipMemGetInfo(&free_b, &total_b), false);
    const uint64_t budget = free_b / 2 + c->gz_sym_cap + c->gz_ctx_cap;  // (what the handle holds of them already is not asked for again)
    std::vector<unsigned long long> pre_off(B);
    uint64_t pre_total = 0, slot_bytes = 0;
    size_t fit = 0;
    for (; fit < B; ++fit) {
        const uint64_t slot = std::max<uint64_t>(slot_bytes, bz_slot_bytes(level[fit]));
        if (pre_total + bz_pre_bytes(level[fit]) + slot > budget) break;
        pre_off[fit] = pre_total, pre_total += bz_pre_bytes(level[fit]), slot_bytes = slot;
    }
    if (fit == 0 || (fit < B && !prefix)) return false;
    B = fit, *n_tab = fit;
    uint64_t pass = c->bz_pass_blocks ? c->bz_pass_blocks : std::max<uint64_t>(1, (budget - pre_total) / 2 / slot_bytes);
    pass = std::min<uint64_t>(std::min<uint64_t>(pass, B), kBzMaxPassBlocks);
    if (!mkz::ensure_quiet(&c->d_gz_tab, &c->gz_tab_cap, BzTab::bytes(B)) || !mkz::ensure_quiet(&c->d_gz_sym, &c->gz_sym_cap, pre_total + 64) ||
        !mkz::ensure_quiet(&c->d_gz_ctx, &c->gz_ctx_cap, pass * slot_bytes))
        return false;
    const BzTab t(c->d_gz_tab, B);
    MKZ_HIP(hipMemcpyAsync(t.bit, bit, B * 8, hipMemcpyHostToDevice, c->stream), false);
    MKZ_HIP(hipMemcpyAsync(t.pre, pre_off.data(), B * 8, hipMemcpyHostToDevice, c->stream), false);
    MKZ_HIP(hipMemcpyAsync(t.level, level, B * 4, hipMemcpyHostToDevice, c->stream), false);
    rep.assign(B, mkz::Bz2Block{}), text_len.assign(B, 0);
    for (size_t b0 = 0; b0 < B; b0 += pass) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(pass, B - b0);
        MKZ_HIP(hipEventRecord(c->ev[0], c->stream), false);
        mkz::launch_bz2_decode((const uint8_t *)c->d_gz_in, n, n_words, t.bit, t.level, t.pre, (uint8_t *)c->d_gz_sym, (uint8_t *)c->d_gz_ctx, slot_bytes, (uint32_t)b0, cnt,
                               t.rep, c->stream);
        MKZ_HIP(hipGetLastError(), false);
        MKZ_HIP(hipEventRecord(c->ev[1], c->stream), false);
        mkz::launch_bz2_walk(t.pre, t.level, (uint8_t *)c->d_gz_sym, (const uint8_t *)c->d_gz_ctx, slot_bytes, (uint32_t)b0, cnt, t.rep, t.tlen, c->stream);
        MKZ_HIP(hipGetLastError(), false);
        MKZ_HIP(hipEventRecord(c->ev[2], c->stream), false);
        MKZ_HIP(hipMemcpyAsync(rep.data() + b0, t.rep + b0, cnt * sizeof(mkz::Bz2Block), hipMemcpyDeviceToHost, c->stream), false);
        MKZ_HIP(hipMemcpyAsync(text_len.data() + b0, t.tlen + b0, cnt * 8ull, hipMemcpyDeviceToHost, c->stream), false);
        MKZ_HIP(hipStreamSynchronize(c->stream), false);
        ms[2] += elapsed(c->ev[0], c->ev[1]), ms[3] += elapsed(c->ev[1], c->ev[2]);
        *done = b0 + cnt;
        // (the stream has been waited for above, so nothing of this pass is in flight here)
        for (size_t k = b0; k < b0 + cnt; ++k)
            if (rep[k].status != 0 || rep[k].end_bit != end_bit[k]) return true;
    }
    return true;
}

// ---- step 3: blocks [b0, b1) of the B decoded ones -> d_text, block k at text_off[k - b0] (offsets inside d_text), and the CRC of
// each block's text.  Both phases are the kernels' own time between events, like the decode and the walk: the allocation of the text
// and the small copies around them belong to no phase.  ms[3], ms[4]
bool bz_text(mk_codec *c, size_t B, size_t b0, size_t b1, const unsigned long long *text_off, uint8_t *d_text, uint32_t *crc, float *ms) {
    const BzTab t(c->d_gz_tab, B);
    const uint32_t cnt = (uint32_t)(b1 - b0);
    MKZ_HIP(hipMemcpyAsync(t.toff + b0, text_off, cnt * 8ull, hipMemcpyHostToDevice, c->stream), false);
    MKZ_HIP(hipEventRecord(c->ev[0], c->stream), false);
    mkz::launch_bz2_expand(t.pre + b0, t.level + b0, (const uint8_t *)c->d_gz_sym, t.rep + b0, t.toff + b0, d_text, cnt, c->stream);
    MKZ_HIP(hipGetLastError(), false);
    MKZ_HIP(hipEventRecord(c->ev[1], c->stream), false);
    mkz::launch_bz2_crc(d_text, t.toff + b0, t.tlen + b0, t.crc + b0, cnt, c->stream);
    MKZ_HIP(hipGetLastError(), false);
    MKZ_HIP(hipEventRecord(c->ev[2], c->stream), false);
    MKZ_HIP(hipMemcpyAsync(crc, t.crc + b0, cnt * 4ull, hipMemcpyDeviceToHost, c->stream), false);
    MKZ_HIP(hipStreamSynchronize(c->stream), false);
    ms[3] += elapsed(c->ev[0], c->ev[1]), ms[4] += elapsed(c->ev[1], c->ev[2]);
    return true;
}

// the whole file in one call; false: not taken
bool bzip2_inflate(mk_codec *c, const uint8_t *bz, uint64_t n, uint64_t *text_bytes, uint64_t *n_blocks) {
    if (n < 14 || bz[0] != 'B' || bz[1] != 'Z' || bz[2] != 'h' || bz[3] < '1' || bz[3] > '9') return false;
    MKZ_HIP(hipSetDevice(c->device), false);
    std::vector<mkz::BzMarker> markers;
    if (!bz_upload_and_search(c, bz, n, kBzMaxMarkers, markers, c->bz_ms)) return false;
    // ---- the table walked into streams and blocks (guesses: every block has yet to end on the magic behind it)
    std::vector<mkz::BzPlanBlock> blocks;
    std::vector<mkz::BzPlanStream> streams;
    if (!mkz::bz2_plan(bz, n, markers, blocks, streams)) return false;
    const size_t B = blocks.size();
    std::vector<uint32_t> crcs(B);
    uint64_t total = 0;
    if (B) {
        std::vector<unsigned long long> bit(B), end_bit(B), text_off(B), text_len;
        std::vector<uint32_t> level(B);
        for (size_t k = 0; k < B; ++k) bit[k] = blocks[k].bit, end_bit[k] = blocks[k].end_bit, level[k] = blocks[k].level;
        std::vector<mkz::Bz2Block> rep;
        size_t done = 0, n_tab = 0;
        if (!bz_decode(c, n, B, bit.data(), level.data(), end_bit.data(), false, rep, text_len, c->bz_ms, &n_tab, &done) || done < B) return false;
        for (size_t k = 0; k < B; ++k)
            if (rep[k].status != 0 || rep[k].end_bit != end_bit[k]) return false;
        for (size_t k = 0; k < B; ++k) text_off[k] = total, total += text_len[k];
        // ---- the text at every block's offset, and its CRC
        if (!mkz::room(total + 128, c->gz_text_cap) || !mkz::ensure_quiet(&c->d_gz_text, &c->gz_text_cap, total + 128)) return false;
        if (!bz_text(c, B, 0, B, text_off.data(), (uint8_t *)c->d_gz_text, crcs.data(), c->bz_ms)) return false;
        for (size_t k = 0; k < B; ++k)
            if (crcs[k] != rep[k].crc) return false;
    }
    for (const mkz::BzPlanStream &s : streams) {
        uint32_t crc = 0;
        for (uint32_t k = 0; k < s.n_blocks; ++k) crc = mkz::bz2_stream_crc_fold(crc, crcs[s.first_block + k]);
        if (crc != s.crc) return false;
    }
    c->gz_text_bytes = total, c->bz_blocks = (uint32_t)B;
    *text_bytes = total, *n_blocks = B;
    return true;
}

// ---- the device behind a stream (bzip2_chain.hpp: Dev)
struct BzStreamDev {
    mk_codec *c;
    mk_bzip2_stream &D;
    bool upload(const uint8_t *up, uint64_t n_up, std::vector<mkz::BzMarker> &markers) {
        D.n_up = n_up;
        return bz_upload_and_search(c, up, n_up, mkz::bz2_marker_cap(n_up), markers, D.s.stats.ms);
    }
    uint32_t decode(const std::vector<mkz::BzWinBlock> &blocks, std::vector<mkz::Bz2Block> &rep, std::vector<unsigned long long> &text_len) {
        const size_t B = blocks.size();
        std::vector<unsigned long long> bit(B), end_bit(B);
        std::vector<uint32_t> level(B);
        for (size_t k = 0; k < B; ++k) bit[k] = blocks[k].bit, end_bit[k] = blocks[k].end_bit, level[k] = blocks[k].level;
        size_t done = 0;
        if (!bz_decode(c, D.n_up, B, bit.data(), level.data(), end_bit.data(), true, rep, text_len, D.s.stats.ms, &D.n_tab, &done)) return 0;
        rep.resize(done), text_len.resize(done);
        return (uint32_t)done;
    }
    uint64_t text_room() {
        if (c->bz_text_cap) return c->bz_text_cap;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 0;
        const uint64_t room = free_b / 2 + D.text.cap[D.text.other()];
        return room > 128 ? room - 128 : 0;  // (expand asks for the text and 128 bytes behind it within the same bound)
    }
    bool expand(uint32_t b0, uint32_t b1, const unsigned long long *text_off, uint64_t total, uint32_t *crc) {
        if (!mkz::room(total + 128, D.text.cap[D.text.other()]) || !D.text.ensure_other(total + 128)) return false;
        if (!bz_text(c, D.n_tab, b0, b1, text_off, D.text.other_text(), crc, D.s.stats.ms)) return false;
        D.text.flip(c);
        return true;
    }
};

}  // namespace

extern "C" {

int mk_bzip2_inflate_device(mk_codec *c, const uint8_t *bz, uint64_t n, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_blocks) {
    MK_ABI_BEGIN
    if (!c || !text_bytes || !taken || !n_blocks || (n && !bz)) return mk::fail(MK_E_INVALID_ARG, "mk_bzip2_inflate_device: NULL argument");
    *text_bytes = 0, *taken = 0, *n_blocks = 0;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->stream_open()) return mkz::refuse_open_stream("mk_bzip2_inflate_device");
    c->gz_text_bytes = 0, c->bz_blocks = 0;
    for (float &x : c->bz_ms) x = 0;
    // (whatever keeps the file from being taken -- anything the walk or the proof refuses, no room, a device error -- is MK_OK with
    // *taken = 0: the file is libbz2's)
    uint64_t text = 0, blocks = 0;
    if (bzip2_inflate(c, bz, n, &text, &blocks)) *text_bytes = text, *n_blocks = blocks, *taken = 1;
    // what is left to keep is the text: the file, the bytes in front of the run-length step and the vectors go back to the device now
    mkz::gz_keep_text(c);
    return MK_OK;
    MK_ABI_END
}

int mk_bzip2_info(const mk_codec *c, uint32_t *blocks, float ms[5]) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_bzip2_info: NULL handle");
    if (blocks) *blocks = c->bz_blocks;
    if (ms)
        for (int k = 0; k < 5; ++k) ms[k] = c->bz_ms[k];
    return MK_OK;
}

// ---- a .bz2 file of any size, window by window

int mk_bzip2_stream_begin(mk_codec *c, const uint8_t *bz, uint64_t n, uint64_t window_bytes, uint32_t *taken) {
    MK_ABI_BEGIN
    if (!c || !taken || (n && !bz)) return mk::fail(MK_E_INVALID_ARG, "mk_bzip2_stream_begin: NULL argument");
    *taken = 0;
    if (window_bytes > (1ull << 40)) return mk::fail(MK_E_INVALID_ARG, "mk_bzip2_stream_begin: a window of 1 TiB at most");
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->stream_open()) return mkz::refuse_open_stream("mk_bzip2_stream_begin");
    mkz::BzStream s;
    if (!mkz::bz2_stream_open(s, bz, n, window_bytes)) return MK_OK;  // (not a bzip2 file)
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    mkz::gz_release(c);  // the one-shot text of an earlier call goes: d_gz_text is the stream's from here on
    c->bz_blocks = 0;
    c->bzs = mk_bzip2_stream{};
    c->bzs.s = s, c->bzs.active = true;
    *taken = 1;
    return MK_OK;
    MK_ABI_END
}

int mk_bzip2_stream_next(mk_codec *c, uint64_t *text_bytes, uint32_t *state) {
    return mkz::chain_stream_next(c, &mk_codec::bzs, text_bytes, state, [&](mk_bzip2_stream &D) {
        BzStreamDev dev{c, D};
        mkz::bz2_stream_next(D.s, dev, text_bytes, state);
    });
}

int mk_bzip2_stream_info(const mk_codec *c, mk_bzip2_stream_stats *out) { return mkz::stream_info(c, &mk_codec::bzs, out); }

int mk_bzip2_stream_end(mk_codec *c) { return mkz::stream_end(c, &mk_codec::bzs); }

}  // extern "C"
