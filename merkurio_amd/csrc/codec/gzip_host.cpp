// gzip_host.cpp -- host side of the C ABI's gzip reader (include/merkurio_hip.h, mk_gzip_*): a gzip file inflated on the device in
// parallel pieces -- one member, a file of several members, or a file of any size window by window.  gzip_segments.hpp says how the
// pieces are decoded (kernels: gzip_inflate.hip); which guessed member start is real, which found block start is dropped and when a
// file is handed back to zlib is decided in gzip_chain.hpp, which has no HIP in it and runs on the CPU in the tests.  Here: ONE driver
// (gzip_run) around it -- upload, block search, rounds of piece decodes, resolution, CRC-32 -- and the entry points that call it.
// The handle and the staging copies: codec_host.cpp.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../host_common.h"
#include "codec_kernels.h"
#include "codec_stream.hpp"
#include "gzip_chain.hpp"

namespace {

using mkz::now_ms;

constexpr uint64_t kStreamWindow = 256ull << 20;  // the default window (an unmeasured choice: README)

void free_all(std::initializer_list<void **> ps) {
    for (void **p : ps) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

uint64_t stream_held(const mk_codec *c) { return mkz::stream_held(c, c->gzs.text) + (c->gzs.d_carry[0] ? 2ull * mkz::kSegPrefix : 0); }

// What the callers of the driver do differently.  Each of these is meant.
struct GzRun {
    // What is uploaded: up[0, n_up) goes to the device as it is -- the payload of the one member without header and trailer
    // (mk_gzip_inflate_device), the whole file (mk_gzip_members_inflate_device), the bytes [base, base + n_up) of a window.  The
    // candidates' offsets and the cuts the block search starts from are relative to it; trailers are read on the host at up + end,
    // inside the upload or right behind it.
    const uint8_t *up;
    uint64_t n_up;
    // First ratio of a piece's room to its compressed bytes.  One-shot: ISIZE says how much text there is in all (gzip_first_ratio).
    // A window has no such sum: 12.
    uint64_t first_ratio;
    // Segment limit, checked before anything is allocated.  One-shot: the members alone.  A window: members + chunks, since its
    // tables are sized before the search says how many pieces there are.
    bool count_chunks;
    // Buffer sizes.  0 (one-shot): by the input.  A window: by the nominal window -- compressed bytes, table and context room per
    // nominal chunk, symbols and text of ratio x nominal -- so that every window of a file finds them there and nothing is sized by
    // the file (mk_gzip_stream_stats::peak_device_bytes).
    uint64_t nominal;
    // ISIZE.  One-shot (whole = true): a member of 4 GiB of text or more is refused, the length is compared exactly.  A window:
    // modulo 2^32, with what the member had before the window.
    bool whole;
    // Text buffer.  nullptr (one-shot): c->d_gz_text.  A stream: the one of its two text buffers that the latest window does not
    // lie in; the carry of the window before goes into the resolution, the next one is made behind it.
    mk_gzip_stream *stream;
    // Timers: upload, block search, pieces, resolution, CRC-32 are ADDED to ms[0 .. 4] -- c->gz_ms, which a one-shot call has zeroed,
    // or the stream's sums over its windows.  (A stream also counts rounds_repeated and members; both record gz_segments.)
    float *ms;
    // Freeing.  One-shot: once the text stands, the compressed bytes, the symbols (24 x the compressed bytes) and the contexts go
    // back to the device.  A stream keeps them for its next window, until it closes.
    bool keep_text_only;
    // (Error rule, at the callers: a device error is returned by a one-shot call and becomes state 2 of a stream.)
};

// the device tables behind starts[n_chunks], per piece (J of them): 64-bit bits | end | lim | off | cap | n_out | text_off, 32-bit
// first[J + 1] | status[J] | bad
struct DevTab {
    unsigned long long *bits, *end, *lim, *off, *cap, *nout, *toff;
    uint32_t *first, *bad;
    int32_t *status;
    DevTab(unsigned long long *d_starts, uint32_t n_chunks, uint32_t J) {
        bits = d_starts + n_chunks, end = bits + J, lim = end + J, off = lim + J, cap = off + J, nout = cap + J, toff = nout + J;
        first = (uint32_t *)(toff + J), status = (int32_t *)(first + J + 1), bad = (uint32_t *)(status + J);
    }
};

// one round's pieces -> symbols, n_out[], status[].  *room = false: the symbols do not fit this device (not taken)
int decode_pieces(mk_codec *c, const mkz::GzPieces &P, const DevTab &t, uint64_t sym_floor, unsigned long long *n_out, int32_t *status, bool *room) {
    const uint32_t J = P.J;
    const uint64_t sym_need = std::max<uint64_t>(P.elems, sym_floor) * 2 + 64;
    size_t free_b = 0, total_b = 0;
    *room = hipMemGetInfo(&free_b, &total_b) != hipSuccess || mkz::room(sym_need, c->gz_sym_cap, free_b);  // (no answer: the allocation decides)
    if (!*room) return MK_OK;
    int rc;
    if ((rc = mk::ensure_device(&c->d_gz_sym, &c->gz_sym_cap, sym_need))) return rc;
    MKC_HIP(hipMemcpyAsync(t.bits, P.tab.data(), P.tab.size() * 8ull, hipMemcpyHostToDevice, c->stream), "upload of the segment table");
    mkz::launch_gzip_segments((const uint8_t *)c->d_gz_in, t.bits, t.end, t.lim, t.off, t.cap, J, (uint16_t *)c->d_gz_sym, t.nout, t.status, c->num_cus, c->stream,
                              c->inflate_kernel == 1);
    MKC_HIP(hipGetLastError(), "gzip segment decode");
    MKC_HIP(hipMemcpyAsync(n_out, t.nout, J * 8ull, hipMemcpyDeviceToHost, c->stream), "download");
    MKC_HIP(hipMemcpyAsync(status, t.status, J * 4ull, hipMemcpyDeviceToHost, c->stream), "download");
    MKC_HIP(hipStreamSynchronize(c->stream), "gzip segment decode");
    c->gz_segments = J;
    return MK_OK;
}

// The driver.  `mem` = the chain of candidate members in the upload, mem[0] a real one (or the member a window continues).
// *state = 0: the text stands (c->gz_text_bytes of it, in c->d_gz_text): every member left decoded from its first bit to a final block
// that ends in its last payload byte -- an open one to a proved block start --, with its trailer's CRC-32 and ISIZE.  2: not taken.
// 3 (a window only): no proved start to stop at, the window grows.  Another return than MK_OK is a device error.  Called with the
// handle's mutex held and its device set.
int gzip_run(mk_codec *c, const GzRun &o, std::vector<mkz::GzCandidate> mem, uint32_t *state, uint64_t *n_members) {
    using namespace mkz;
    *state = 2;
    mk_gzip_stream *S = o.stream;
    int rc;
    const uint64_t n_in = o.n_up;
    const uint64_t chunk = gzip_chunk_bytes(n_in, c->gzip_chunk, c->num_cus);
    const uint32_t n_chunks = (uint32_t)std::max<uint64_t>(1, n_in / chunk);
    if (mem.size() + (o.count_chunks ? n_chunks : 0) > kGzMaxPieces) return MK_OK;
    const size_t seg_room = o.nominal ? (size_t)std::max<uint64_t>(1, o.nominal / chunk) + 16 : 0;
    if ((rc = mk::ensure_device(&c->d_gz_in, &c->gz_in_cap, std::max(o.nominal, n_in) + kPad + 16))) return rc;
    // tables: starts[n_chunks] | DevTab (J <= n_chunks + members pieces) | 16 words to spare
    const size_t max_seg = std::max<size_t>(seg_room, (size_t)n_chunks + mem.size());
    if ((rc = mk::ensure_device(&c->d_gz_tab, &c->gz_tab_cap, ((size_t)n_chunks + max_seg * 8 + 16) * 8))) return rc;
    unsigned long long *d_starts = (unsigned long long *)c->d_gz_tab;
    double t0 = now_ms();
    if ((rc = upload(c, c->d_gz_in, o.up, n_in))) return rc;
    MKC_HIP(hipMemsetAsync((uint8_t *)c->d_gz_in + n_in, 0, kPad + 16, c->stream), "hipMemsetAsync");
    MKC_HIP(hipStreamSynchronize(c->stream), "upload of the stream");
    o.ms[0] += (float)(now_ms() - t0);
    // ---- block starts: searched over all the bytes as they lie there, headers and trailers included
    t0 = now_ms();
    std::vector<unsigned long long> starts(n_chunks, ~0ull);
    launch_gzip_find((const uint8_t *)c->d_gz_in, n_in, chunk, n_chunks, chunk, d_starts, c->stream);  // (a start behind the next cut is the next chunk's to find)
    MKC_HIP(hipGetLastError(), "gzip block search");
    if (n_chunks > 1) MKC_HIP(hipMemcpyAsync(starts.data() + 1, d_starts + 1, (n_chunks - 1) * 8ull, hipMemcpyDeviceToHost, c->stream), "download of the block starts");
    MKC_HIP(hipStreamSynchronize(c->stream), "gzip block search");
    o.ms[1] += (float)(now_ms() - t0);
    std::vector<unsigned long long> found = gzip_found_starts(starts);
    // ---- pieces -> symbols, in rounds (gzip_prove): 12 x a piece's compressed bytes of room, then 48 x once more
    t0 = now_ms();
    GzRounds R;
    R.ratio = o.first_ratio;
    GzPieces P;
    std::vector<unsigned long long> n_out;
    const bool proved = gzip_prove(mem, found, n_in, R, P, n_out, [&](const GzPieces &p, unsigned long long *p_out, int32_t *p_status) {
        if (p.J > max_seg) {
            rc = mk::fail(MK_E_HIP, "gzip pieces: %u of them, a table for %llu (internal error)", p.J, (unsigned long long)max_seg);
            return false;
        }
        bool room = true;
        rc = decode_pieces(c, p, DevTab(d_starts, n_chunks, p.J), seg_room * (uint64_t)(kSegPrefix + 65536 + kSegSlack + 8 + R.ratio) + R.ratio * o.nominal, p_out, p_status, &room);
        return rc == MK_OK && room;
    });
    o.ms[2] += (float)(now_ms() - t0);
    if (S) S->stats.rounds_repeated += R.repeated;
    if (rc || !proved) return rc;
    const uint32_t J = P.J;
    const size_t M = mem.size();
    const DevTab t(d_starts, n_chunks, J);
    // ---- where a window ends
    uint64_t next_bit = 0;
    bool next_in_member = false;
    if (S) {
        const int e = gzip_window_end(mem, P.cut_bit, S->at.pos_bit, S->at.in_member, S->n, (S->at.pos_bit >> 3) + n_in == S->n, &next_bit, &next_in_member);
        if (e) {
            *state = (uint32_t)e;
            return MK_OK;
        }
    }
    // ---- every closed member's text is as long as its trailer says
    const bool continues = S && S->at.in_member;  // mem[0] began in an earlier window
    GzText T;
    if (!gzip_text_offsets(mem, P, n_out, o.up, o.whole, continues ? S->at.open_len : 0, T)) return MK_OK;
    // ---- contexts, text
    t0 = now_ms();
    // (the contexts, and behind them two sets of J - 1 maps of 32 768 16-bit elements: codec_kernels.h)
    if ((rc = mk::ensure_device(&c->d_gz_ctx, &c->gz_ctx_cap, std::max<size_t>(J, seg_room) * kSegPrefix * 5 + 16))) return rc;
    // (a stream: the buffer its latest window does not lie in; no room for it is "not taken", rc being MK_OK here)
    const size_t text_need = std::max<uint64_t>(T.total, R.ratio * o.nominal) + 64;
    if (S ? !S->text.ensure_other(text_need) : (rc = mk::ensure_device(&c->d_gz_text, &c->gz_text_cap, text_need)) != MK_OK) return rc;
    const uint8_t *const d_text = S ? S->text.other_text() : (const uint8_t *)c->d_gz_text;
    uint32_t bad = 0;
    if (J) {
        MKC_HIP(hipMemcpyAsync(t.toff, T.off.data(), J * 8ull, hipMemcpyHostToDevice, c->stream), "upload of the text offsets");
        MKC_HIP(hipMemcpyAsync(t.first, P.seg_first.data(), (J + 1) * 4ull, hipMemcpyHostToDevice, c->stream), "upload of the member table");
        MKC_HIP(hipMemsetAsync(t.bad, 0, 4, c->stream), "hipMemsetAsync");
        launch_gzip_resolve((const uint16_t *)c->d_gz_sym, t.off, t.nout, t.toff, t.first, J, T.max_member_segs, (uint8_t *)c->d_gz_ctx, (uint8_t *)d_text, t.bad, c->stream,
                            continues ? (const uint8_t *)S->d_carry[S->carry_cur] : nullptr, continues ? S->at.carry_len : 0);
        MKC_HIP(hipGetLastError(), "gzip resolution");
        MKC_HIP(hipMemcpyAsync(&bad, t.bad, 4, hipMemcpyDeviceToHost, c->stream), "download");
        MKC_HIP(hipStreamSynchronize(c->stream), "gzip resolution");
    }
    o.ms[3] += (float)(now_ms() - t0);
    if (bad) return MK_OK;
    // ---- CRC-32 per member of its text, folded into what the member had before the window (gzip_chain.hpp)
    t0 = now_ms();
    std::vector<unsigned long long> blk_off;
    std::vector<uint32_t> blk_len, mem_crc;
    gzip_crc_blocks(P, T, kMaxBlockBytes, blk_off, blk_len);
    const size_t blocks = blk_off.size();
    if (blocks >> 32) return MK_OK;
    if ((rc = mk::ensure_device(&c->d_crc, &c->crc_cap, blocks * 4ull + 16)) || (rc = mk::ensure_device(&c->d_off, &c->off_cap, blocks * 8ull + 16)) ||
        (rc = mk::ensure_device(&c->d_len, &c->len_cap, blocks * 4ull + 16)))
        return rc;
    std::vector<uint32_t> crcs(blocks);
    if (blocks) {
        MKC_HIP(hipMemcpyAsync(c->d_off, blk_off.data(), blocks * 8ull, hipMemcpyHostToDevice, c->stream), "upload of the CRC blocks");
        MKC_HIP(hipMemcpyAsync(c->d_len, blk_len.data(), blocks * 4ull, hipMemcpyHostToDevice, c->stream), "upload of the CRC blocks");
        launch_crc_ranges(d_text, (const unsigned long long *)c->d_off, (const uint32_t *)c->d_len, (uint32_t)blocks, (uint32_t *)c->d_crc, c->stream);
        MKC_HIP(hipGetLastError(), "CRC kernel");
        MKC_HIP(hipMemcpyAsync(crcs.data(), c->d_crc, blocks * 4ull, hipMemcpyDeviceToHost, c->stream), "download of the CRCs");
    }
    MKC_HIP(hipStreamSynchronize(c->stream), "CRC kernel");
    if (!gzip_crc_fold(mem, T, blk_len, crcs.data(), kMaxBlockBytes, o.up, continues ? S->at.open_crc : 0, mem_crc)) return MK_OK;
    o.ms[4] += (float)(now_ms() - t0);
    // ---- the text stands
    if (S) {
        if (next_in_member) {  // the last 32 KiB of the open member's text so far: what the next window's first pieces reach back into
            const uint8_t *prev = gzip_window_continues(S->at, M, next_in_member) ? (const uint8_t *)S->d_carry[S->carry_cur] : nullptr;
            launch_gzip_carry(d_text + T.last_member_off(P), T.mem_text[M - 1], prev, (uint8_t *)S->d_carry[S->carry_cur ^ 1], c->stream);
            MKC_HIP(hipGetLastError(), "gzip carry");
            MKC_HIP(hipStreamSynchronize(c->stream), "gzip carry");
            S->carry_cur ^= 1;
        }
        gzip_window_stands(S->at, M, T.mem_text[M - 1], mem_crc[M - 1], next_bit, next_in_member);
        for (size_t m = 0; m < M; ++m) S->stats.members += mem[m].closed;
        S->text.flip(c);
        S->stats.windows += 1, S->stats.text_bytes += T.total, S->stats.consumed_bytes = S->at.pos_bit >> 3;
    }
    c->gz_text_bytes = T.total;
    if (n_members) *n_members = M;
    if (o.keep_text_only) gz_keep_text(c);
    if (S) S->stats.peak_device_bytes = std::max<uint64_t>(S->stats.peak_device_bytes, stream_held(c));
    *state = 0;
    return MK_OK;
}

// The one-shot calls: every candidate lies whole in the upload
int gzip_one_shot(mk_codec *c, const uint8_t *up, uint64_t n_up, std::vector<mkz::GzCandidate> mem, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_members) {
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    uint32_t state = 2;
    const int rc = gzip_run(c, GzRun{up, n_up, mkz::gzip_first_ratio(up, n_up, mem), false, 0, true, nullptr, c->gz_ms, true}, std::move(mem), &state, n_members);
    if (rc) return rc;
    if (state == 0) *text_bytes = c->gz_text_bytes, *taken = 1;
    return MK_OK;
}

// One window of a stream: *state = 0 (c->gz_text_bytes of text in the current text buffer), 2, or 3 = grow the window and call again
int gzip_stream_window(mk_codec *c, uint32_t *state) {
    mk_gzip_stream &S = c->gzs;
    const uint64_t base = S.at.pos_bit >> 3;
    const uint64_t nominal = mkz::gzip_window_nominal(S.window, S.grow);
    const uint64_t n_up = std::min<uint64_t>(S.n - base, nominal);
    std::vector<mkz::GzCandidate> mem;
    if ((*state = (uint32_t)mkz::gzip_window_candidates(S.gz, S.n, S.guesses, S.at.pos_bit, S.at.in_member, n_up, base + n_up == S.n, mem))) return MK_OK;
    return gzip_run(c, GzRun{S.gz + base, n_up, 12, true, nominal, false, &S, S.stats.ms, false}, std::move(mem), state, nullptr);
}

}  // namespace

namespace mkz {

void gz_release(mk_codec *c) {
    free_all({&c->d_gz_in, &c->d_gz_sym, &c->d_gz_tab, &c->d_gz_ctx, &c->d_gz_text});
    c->gz_in_cap = c->gz_sym_cap = c->gz_tab_cap = c->gz_ctx_cap = c->gz_text_cap = 0;
    c->gz_text_bytes = 0;
}

void gz_keep_text(mk_codec *c) {
    free_all({&c->d_gz_sym, &c->d_gz_ctx, &c->d_gz_in});
    c->gz_sym_cap = c->gz_ctx_cap = c->gz_in_cap = 0;
}

}  // namespace mkz

extern "C" {

int mk_gzip_member_guesses(const uint8_t *gz, uint64_t n, mk_gzip_guess *table, uint64_t cap, uint64_t *n_guesses) {
    if (!n_guesses || (n && !gz)) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_member_guesses: NULL argument");
    *n_guesses = mkz::gzip_member_guesses(gz, n, table, cap);
    return MK_OK;
}

uint32_t mk_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b) { return mkz::crc_mulmod(crc_a, mkz::crc_x_pow_bytes(len_b)) ^ crc_b; }

int mk_gzip_inflate_device(mk_codec *c, const uint8_t *gz, uint64_t n, uint64_t *text_bytes, uint32_t *taken) {
    MK_ABI_BEGIN
    if (!c || !text_bytes || !taken || (n && !gz)) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_inflate_device: NULL argument");
    *text_bytes = 0, *taken = 0;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->stream_open()) return mkz::refuse_open_stream("mk_gzip_inflate_device");
    c->gz_text_bytes = 0, c->gz_segments = 0;
    for (float &x : c->gz_ms) x = 0;
    // RFC 1952: the member's header, then the DEFLATE stream up to the 8 trailer bytes.  One member is what is taken here: the stream
    // has to end where the file does, on the final block its last piece meets in front of the trailer (a file of several members
    // does not: mk_gzip_members_inflate_device).  Not gzip / reserved flags / no room for a stream: not taken.
    const uint64_t p = n ? mkz::gzip_header_end(gz, n, 0) : 0;
    if (!p) return MK_OK;
    return gzip_one_shot(c, gz + p, n - 8 - p, {mkz::GzCandidate{0, 0, n - 8 - p, true}}, text_bytes, taken, nullptr);
    MK_ABI_END
}

int mk_gzip_members_inflate_device(mk_codec *c, const uint8_t *gz, uint64_t n, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_members) {
    MK_ABI_BEGIN
    if (!c || !text_bytes || !taken || !n_members || (n && !gz)) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_members_inflate_device: NULL argument");
    *text_bytes = 0, *taken = 0, *n_members = 0;
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->stream_open()) return mkz::refuse_open_stream("mk_gzip_members_inflate_device");
    c->gz_text_bytes = 0, c->gz_segments = 0;
    for (float &x : c->gz_ms) x = 0;
    // the member starts as the host can guess them: every place where a header parses.  The file goes up whole; which guesses are
    // member starts is what the decode proves.  Bytes behind the last member cannot be proved away: not taken.
    const uint64_t n_guesses = mkz::gzip_member_guesses(gz, n, nullptr, 0);
    if (!n_guesses) return MK_OK;
    std::vector<mk_gzip_guess> guesses(n_guesses);
    mkz::gzip_member_guesses(gz, n, guesses.data(), n_guesses);
    uint64_t members = 0;
    const int rc = gzip_one_shot(c, gz, n, mkz::gzip_file_candidates(guesses, n), text_bytes, taken, &members);
    if (*taken) *n_members = members;
    return rc;
    MK_ABI_END
}

int mk_gzip_text_read(mk_codec *c, uint64_t offset, uint8_t *out, uint64_t len) {
    MK_ABI_BEGIN
    if (!c || (len && !out)) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_text_read: NULL argument");
    std::lock_guard<std::mutex> lock(c->mu);
    if (offset > c->gz_text_bytes || len > c->gz_text_bytes - offset) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_text_read: [%llu, +%llu) is outside the text", (unsigned long long)offset, (unsigned long long)len);
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    return mkz::download(c, out, (const uint8_t *)c->d_gz_text + offset, len);
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
    mkz::streams_close(c);  // (an open stream's text is the text: the stream ends with it)
    mkz::gz_release(c);
    return MK_OK;
}

int mk_gzip_info(const mk_codec *c, uint32_t *segments, float ms[5]) {
    if (!c) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_info: NULL handle");
    if (segments) *segments = c->gz_segments;
    if (ms)
        for (int k = 0; k < 5; ++k) ms[k] = c->gz_ms[k];
    return MK_OK;
}

// ---- a gzip file of any size, window by window

int mk_gzip_stream_begin(mk_codec *c, const uint8_t *gz, uint64_t n, uint64_t window_bytes, uint32_t *taken) {
    MK_ABI_BEGIN
    if (!c || !taken || (n && !gz)) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_stream_begin: NULL argument");
    *taken = 0;
    if (window_bytes && (window_bytes < 4096 || window_bytes > (1ull << 40))) return mk::fail(MK_E_INVALID_ARG, "mk_gzip_stream_begin: a window of 4 KiB at least");
    std::lock_guard<std::mutex> lock(c->mu);
    if (c->stream_open()) return mkz::refuse_open_stream("mk_gzip_stream_begin");
    const uint64_t n_guesses = mkz::gzip_member_guesses(gz, n, nullptr, 0);
    if (!n_guesses) return MK_OK;  // (not a gzip file)
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    mkz::gz_release(c);  // the one-shot text of an earlier call goes: d_gz_text is the stream's from here on
    c->gz_segments = 0;
    mk_gzip_stream &S = c->gzs;
    S = mk_gzip_stream{};
    S.guesses.resize(n_guesses);
    mkz::gzip_member_guesses(gz, n, S.guesses.data(), n_guesses);
    for (int k = 0; k < 2; ++k) {
        if (hipMalloc(&S.d_carry[k], mkz::kSegPrefix) != hipSuccess || hipMemsetAsync(S.d_carry[k], 0, mkz::kSegPrefix, c->stream) != hipSuccess) {
            (void)hipGetLastError();
            S.active = true;
            mkz::stream_close(c, S);
            return MK_OK;  // (the codec rule: the device's trouble is "not taken")
        }
    }
    S.active = true, S.gz = gz, S.n = n, S.window = window_bytes ? window_bytes : kStreamWindow;
    *taken = 1;
    return MK_OK;
    MK_ABI_END
}

int mk_gzip_stream_next(mk_codec *c, uint64_t *text_bytes, uint32_t *state) {
    return mkz::stream_next(c, &mk_codec::gzs, text_bytes, state, [&](mk_gzip_stream &S) {
        if (S.dead) return;
        if (!S.at.in_member && (S.at.pos_bit >> 3) == S.n) {
            *state = 1;
            return;
        }
        if (hipSetDevice(c->device) != hipSuccess) {
            S.dead = true;
            return;
        }
        S.grow = 0;
        for (;;) {
            uint32_t st = 2;
            const int rc = gzip_stream_window(c, &st);
            if (rc != MK_OK) st = 2, (void)hipGetLastError();  // (a device error hands the stream back)
            if (st == 3) {  // no proved start inside the window: twice the window, as long as the file and the device have the room
                if (!mkz::gzip_window_may_grow(S.at.pos_bit, S.window, S.grow, S.n)) st = 2;
                else {
                    ++S.grow, ++S.stats.windows_grown;
                    continue;
                }
            }
            if (st == 0) *text_bytes = c->gz_text_bytes;
            else S.dead = true, c->gz_text_bytes = 0;
            *state = st;
            return;
        }
    });
}

int mk_gzip_stream_info(const mk_codec *c, mk_gzip_stream_stats *out) { return mkz::stream_info(c, &mk_codec::gzs, out); }

int mk_gzip_stream_end(mk_codec *c) { return mkz::stream_end(c, &mk_codec::gzs); }

}  // extern "C"
