// extract_window.cpp -- `extract` on text windows that stay on the device: the window steps of window_ingest.cpp, then the extract loop
// as in mk_extract_single / mk_extract_paired, then the kept records' way back -- their stored text (window_kept) or BGZF members of
// their written form, or zstd frames of it (window_members)
#include <mutex>

#include "device_loop.hpp"
#include "codec/codec_internal.h"
#include "codec/codec_kernels.h"

using namespace mk;

namespace {

// what the written text of a window's kept records leaves the device as
enum class Packed { kMembers, kFrames };  // BGZF members (mk_extract_window_members), zstd frames (mk_extract_window_frames)
const char *entry_name(Packed kind) { return kind == Packed::kFrames ? "mk_extract_window_frames" : "mk_extract_window_members"; }

// scratch of a kept-records step in m->d_aux: `arrays` u32 arrays of n + 2 entries from *d_len on | a spare word | the tile sums of
// the offsets scan; room for the offsets themselves in m->d_off
int kept_scratch(mk_matcher *m, uint64_t n, uint32_t arrays, uint32_t **d_len, unsigned long long **d_tile) {
    const size_t n_tiles = n / ingest_scan_tile() + 2;
    if (int rc = ensure_device(&m->d_aux, &m->d_aux_cap, arrays * (n + 2) * 4 + 16 + n_tiles * 8 + 64)) return rc;
    *d_len = (uint32_t *)m->d_aux;
    *d_tile = (unsigned long long *)(((uintptr_t)(*d_len + arrays * (n + 2) + 1) + 15) & ~(uintptr_t)15);
    return ensure_device((void **)&m->d_off, &m->d_off_cap, (n + 1) * sizeof(uint64_t));
}

bool keeps_big_record(const uint8_t *keep_host, const std::vector<uint32_t> &rs, uint64_t n) {
    for (uint64_t r = 0; r < n; ++r)
        if (keep_host[r] && rs[r + 1] - rs[r] >= kBigRecord) return true;
    return false;
}

// chromosome-sized records: every kept record of kBigRecord stored bytes or more goes to m->d_seq + at[r] by a device copy of its own,
// but for its last `left` bytes (the gather kernel's)
int copy_big_records(mk_matcher *m, const WindowSide &W, uint64_t n, const uint8_t *keep_host, const std::vector<uint32_t> &rs, const unsigned long long *at,
                     uint32_t left, hipStream_t st) {
    for (uint64_t r = 0; r < n; ++r) {
        const uint64_t len = rs[r + 1] - rs[r];
        if (keep_host[r] && len >= kBigRecord &&
            hipMemcpyAsync(m->d_seq + at[r], (const uint8_t *)W.T->d_text + rs[r], len - left, hipMemcpyDeviceToDevice, st) != hipSuccess)
            return fail(MK_E_HIP, "copy of a kept record failed");
    }
    return MK_OK;
}

// text of the kept records of side W (keep flags in d_keep, already final: invert applied by the caller as 0; rs[n] = W.n_used),
// packed -> host
int window_kept(mk_matcher *m, WindowSide &W, uint64_t n, const uint8_t *d_keep, const std::vector<uint32_t> &rs, const uint8_t *keep_host, mk_window_source &S,
                DeviceLoop &dl) {
    hipStream_t st = dl.st;
    S.n_kept_bytes = 0;
    if (!n) return MK_OK;
    int rc;
    // lengths by the flags, then the pack step: offsets scan, gather, download
    uint32_t *d_len = nullptr;
    unsigned long long *d_tile = nullptr, total = 0;
    if ((rc = kept_scratch(m, n, 1, &d_len, &d_tile))) return rc;
    launch_ingest_select(d_keep, 0u, W.d_rec_start, n, (uint32_t)W.n_used, d_len, st);
    if ((rc = scan_offsets(d_len, n, d_tile, (unsigned long long *)m->d_off, st, &total, "selection of the kept records failed"))) return rc;
    S.n_kept_bytes = total;
    if (total > S.kept_cap) return fail(MK_E_CAPACITY, "the kept records take %llu bytes", total);
    if (!total) return MK_OK;
    if ((rc = pack_gather(m, W, W.d_rec_start, d_len, n, total, 0, kBigRecord, st, "copy of the kept records failed"))) return rc;
    if (keeps_big_record(keep_host, rs, n)) {  // (where each kept record goes: the sum of the stored lengths in front of it)
        std::vector<unsigned long long> at(n);
        unsigned long long sum = 0;
        for (uint64_t r = 0; r < n; ++r) at[r] = sum, sum += keep_host[r] ? rs[r + 1] - rs[r] : 0;
        if ((rc = copy_big_records(m, W, n, keep_host, rs, at.data(), 0, st))) return rc;
    }
    return pack_download(m, S.kept, total, st, "copy of the kept records failed");
}

// the kept records of side W in their written form (include/merkurio_hip.h), packed on the device, then cut and compressed there --
// BGZF members or zstd frames by `kind`, the one place the two differ: only they come down -- or, below S.text_below bytes, the text.
// With logging the ids of the kept records follow, packed by the sequences' gather kernel.  *status = 2: a FASTA record the device does not write (nothing has been written to S's buffers).
// The time of the codec's steps is ADDED to cut_ms / *cut_members (a paired window has two sides); frames: to the handle's zd_* fields.
int window_members(mk_matcher *m, mk_codec *codec, Packed kind, uint32_t format, WindowSide &W, uint64_t n, const uint8_t *d_keep, const std::vector<uint32_t> &rs,
                   const uint8_t *keep_host, int logging, mk_window_members &S, DeviceLoop &dl, float cut_ms[3], uint64_t *cut_members, uint32_t *status) {
    hipStream_t st = dl.st;
    if (!n) return MK_OK;
    int rc;
    const bool fasta = format == MK_TEXT_FASTA;
    const uint8_t *d_text = (const uint8_t *)W.T->d_text;
    // scratch: written lengths | id starts | id lengths | refusal word | tile sums
    uint32_t *d_len = nullptr;
    unsigned long long *d_tile = nullptr;
    if ((rc = kept_scratch(m, n, 3, &d_len, &d_tile))) return rc;
    uint32_t *d_id_start = d_len + n + 2, *d_id_len = d_id_start + n + 2, *d_refused = d_id_len + n + 2;
    unsigned long long *d_off = (unsigned long long *)m->d_off;
    // the two written-form kernels are timed by stream events (S.written_ms), read once the stream has been waited for anyway
    struct Events {
        hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
        ~Events() {
            for (hipEvent_t x : e)
                if (x) (void)hipEventDestroy(x);
        }
    } ev;
    for (hipEvent_t &x : ev.e)
        if (hipEventCreate(&x) != hipSuccess) return fail(MK_E_HIP, "hipEventCreate failed");
    bool gathered = false;
    auto kernel_ms = [&] {  // (the stream is idle)
        float a = 0, b = 0;
        (void)hipEventElapsedTime(&a, ev.e[0], ev.e[1]);
        if (gathered) (void)hipEventElapsedTime(&b, ev.e[2], ev.e[3]);
        S.written_ms = a + b;
    };
    uint32_t refused = 0;
    unsigned long long total = 0;
    if (hipMemsetAsync(d_refused, 0, 4, st) != hipSuccess || hipEventRecord(ev.e[0], st) != hipSuccess) return fail(MK_E_HIP, "hipMemsetAsync failed");
    launch_ingest_written_select(d_text, d_keep, 0u, fasta, W.d_line, W.d_seq_len, W.d_rec_start, n, (uint32_t)W.n_used, d_len, logging ? d_id_start : nullptr,
                                 logging ? d_id_len : nullptr, d_refused, st);
    // (the refusal word comes down with the scan's total: one wait)
    if (hipGetLastError() != hipSuccess || hipEventRecord(ev.e[1], st) != hipSuccess ||
        hipMemcpyAsync(&refused, d_refused, 4, hipMemcpyDeviceToHost, st) != hipSuccess)
        return fail(MK_E_HIP, "selection of the written records failed");
    if ((rc = scan_offsets(d_len, n, d_tile, d_off, st, &total, "selection of the written records failed"))) return rc;
    if (refused) {
        *status = 2;
        return MK_OK;
    }
    for (uint64_t r = 0; r < n; ++r) S.n_kept += keep_host[r] != 0;
    S.n_written = total;
    int cap_rc = MK_OK;
    if (total) {
        if ((rc = pack_room(m, total, mkz::kPad))) return rc;
        // chromosome-sized FASTA records go to their written offset, but for the last 16 stored bytes (the kernel's)
        if (fasta && keeps_big_record(keep_host, rs, n)) {
            std::vector<unsigned long long> off(n + 1);
            if (hipMemcpyAsync(off.data(), d_off, (n + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
                return fail(MK_E_HIP, "copy of the written offsets failed");
            if ((rc = copy_big_records(m, W, n, keep_host, rs, off.data(), 16, st))) return rc;
        }
        if (hipEventRecord(ev.e[2], st) != hipSuccess) return fail(MK_E_HIP, "hipEventRecord failed");
        launch_ingest_written_gather(d_text, fasta, W.d_line, W.d_seq_len, W.d_rec_start, n, (uint32_t)W.n_used, d_len, d_off, m->d_seq,
                                     fasta ? kBigRecord : 0xFFFFFFFFu, st);
        // (no wait of its own: the download, or the cut kernel's count, waits for the stream)
        if (hipGetLastError() != hipSuccess || hipEventRecord(ev.e[3], st) != hipSuccess || hipMemsetAsync(m->d_seq + total, 0, mkz::kPad, st) != hipSuccess)
            return fail(MK_E_HIP, "gather of the written records failed");
        gathered = true;
        if (S.text_below && total < S.text_below) {  // a small window: its text, for the caller to gather with its neighbours'
            S.as_text = 1;
            S.n_member_bytes = total;
            if (total > S.members_cap) {
                if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "gather of the written records failed");
                cap_rc = fail(MK_E_CAPACITY, "the written records take %llu bytes", total);
            } else if ((rc = pack_download(m, S.members, total, st, "copy of the written records failed"))) {
                return rc;
            }
        } else {
            std::lock_guard<std::mutex> lock(codec->mu);
            uint64_t need = 0, members = 0;
            // (the codec times its steps by the host's clock: the gather must not run into the cut kernel's share)
            if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "gather of the written records failed");
            // the offsets scan is the record-end table: off[r + 1] = where record r's written form ends (a record that is not kept
            // repeats the end in front of it)
            if (kind == Packed::kFrames) {
                if ((rc = mkz::zstd_deflate_ranges(codec, st, m->d_seq, total, d_off + 1, n, S.members, S.members_cap, &need, &members))) return rc;
            } else {
                if ((rc = mkz::deflate_ranges(codec, st, m->d_seq, total, d_off + 1, n, nullptr, 0, S.members, S.members_cap, &need, &members))) return rc;
                for (int k = 0; k < 3; ++k) cut_ms[k] += codec->cut_ms[k];
                *cut_members += members;
            }
            S.n_member_bytes = need, S.n_members = members;
            if (need > S.members_cap)
                cap_rc = fail(MK_E_CAPACITY, "the %s of the kept records take %llu bytes", kind == Packed::kFrames ? "frames" : "members", (unsigned long long)need);
        }
    }
    kernel_ms();
    if (!logging || !S.n_kept) return cap_rc;
    // ---- the ids of the kept records, packed the way the sequences are: start and length table, offsets scan, gather
    if ((rc = scan_offsets(d_id_len, n, d_tile, d_off, st, &total, "selection of the ids failed"))) return rc;
    S.n_id_bytes = total;
    if (total > S.ids_cap) return fail(MK_E_CAPACITY, "the ids of the kept records take %llu bytes", total);
    std::vector<unsigned long long> off(n + 1);
    if ((rc = pack_gather(m, W, d_id_start, d_id_len, n, total, 0, 0xFFFFFFFFu, st, "copy of the ids failed"))) return rc;
    if (hipMemcpyAsync(off.data(), d_off, (n + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess) return fail(MK_E_HIP, "copy of the ids failed");
    if ((rc = pack_download(m, S.ids, total, st, "copy of the ids failed"))) return rc;
    uint64_t q = 0;
    for (uint64_t r = 0; r < n; ++r)
        if (keep_host[r]) S.id_end[q++] = off[r + 1];
    return cap_rc;
}

// the body of mk_extract_window (mem == nullptr) and of mk_extract_window_members / mk_extract_window_frames (one mk_window_members per
// source; kind: which of the two), and of mk_extract_window_open (front != nullptr: the one source's window may begin anywhere -- the index
// step finds its first record start, the text in front of it goes back through *front)
int extract_window_body(mk_matcher *m, mk_codec *codec, uint32_t format, uint32_t n_sources, mk_window_source *src, mk_window_members *mem, mk_window_front *front, Packed kind, int logging,
                        int invert, uint64_t rec_cap, uint64_t *n_rec_out, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *c,
                        uint32_t *counts, uint32_t *status) {
    if (!m || !src || !n_rec_out || !status || !c || (logging && !counts)) return fail(MK_E_INVALID_ARG, "null argument");
    if (n_sources < 1 || n_sources > 2) return fail(MK_E_INVALID_ARG, "mk_extract_window: one source (single file) or two (paired files)");
    if (format > MK_TEXT_FASTA) return fail(MK_E_INVALID_ARG, "mk_extract_window: unknown text format %u", format);
    *n_rec_out = 0;
    *status = 0;
    if (n_rows) *n_rows = 0;
    for (uint32_t k = 0; k < n_sources; ++k) {
        mk_window_source &S = src[k];
        S.n_window = S.n_used = S.n_tail = S.n_kept_bytes = S.n_rec_seen = 0;
        if ((S.n_head && !S.head) || (S.n_text && !S.text) || (S.n_members && (!S.bgzf || !S.members)) || (S.n_device_text && !S.device_text) ||
            (S.kept_cap && !S.kept) ||
            (S.all_cap && !S.all) || (S.tail_cap && !S.tail))
            return fail(MK_E_INVALID_ARG, "mk_extract_window: a size without its buffer in source %u", k);
        if (!mem) continue;
        mk_window_members &M = mem[k];
        M.n_member_bytes = M.n_members = M.n_written = M.n_kept = M.n_id_bytes = 0, M.as_text = 0, M.written_ms = 0;
        if ((M.members_cap && !M.members) || (M.ids_cap && !M.ids) || (logging && !M.id_end))
            return fail(MK_E_INVALID_ARG, "%s: a size without its buffer in source %u", entry_name(kind), k);
        if (S.kept || S.kept_cap)
            return fail(MK_E_INVALID_ARG, "%s: the kept records leave as members or frames, not as source %u's kept text", entry_name(kind), k);
    }
    if (mem) {
        if (!codec) return fail(MK_E_INVALID_ARG, "%s: the members or frames need a codec handle", entry_name(kind));
        if (logging && invert) return fail(MK_E_INVALID_ARG, "%s: with logging and invert the rows name records that are not kept", entry_name(kind));
        if (codec->device != m->device) return fail(MK_E_INVALID_ARG, "%s: the codec and the matcher are on different devices", entry_name(kind));
        if (kind == Packed::kFrames) {  // (the frame writer's rule, as mk_zstd_deflate_records has it; what it reports starts again)
            std::lock_guard<std::mutex> lock(codec->mu);
            if (codec->stream_open()) return mkz::refuse_open_stream("mk_extract_window_frames");
            mkz::zstd_deflate_reset(codec);
        }
    }
    MK_ABI_BEGIN
    if (hipSetDevice(m->device) != hipSuccess) return fail(MK_E_HIP, "hipSetDevice failed");
    DeviceLoop dl(m);
    hipStream_t st = dl.st;
    int rc;
    const bool paired = n_sources == 2;
    const bool ac = m->algo == MK_ALGO_AC;
    WindowSide W[2];
    // ---- the text of every source on the device, then what the index kernels make of it
    uint64_t most = 0;
    for (uint32_t k = 0; k < n_sources; ++k) {
        W[k].T = &m->txt[k];
        if ((rc = window_assemble(m, codec, src[k], W[k], dl))) return rc;
        most = std::max(most, W[k].n_window);
    }
    if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "upload of the window failed");
    dl.mark(1);
    if ((rc = ensure_device((void **)&m->d_seq, &m->d_seq_cap, most + 64))) return rc;
    uint64_t n = ~0ull;
    for (uint32_t k = 0; k < n_sources; ++k) {
        if (W[k].n_window == 0) {  // nothing of this input in the window
            W[k].n_avail = 0;
            if (front) {  // (no text, no start)
                *status = 2;
                return MK_OK;
            }
        } else {
            uint8_t *fa_seq = nullptr;
            if (format == MK_TEXT_FASTA) {  // the index step compacts the sequences already: every input has a buffer of its own for them
                if ((rc = ensure_device(&W[k].T->d_fa_seq, &W[k].T->d_fa_seq_cap, W[k].n_window + 64))) return rc;
                fa_seq = (uint8_t *)W[k].T->d_fa_seq;
            }
            uint64_t from = 0;
            if ((rc = window_index(m, format, src[k].ends_at_record != 0, W[k], fa_seq, st, status, front ? &from : nullptr))) return rc;
            if (front) front->n_front = *status == 2 ? W[k].n_window : from;
            if (*status) return MK_OK;
        }
        src[k].n_rec_seen = W[k].n_avail;
        n = std::min(n, W[k].n_avail);
    }
    *n_rec_out = n;
    if (n > rec_cap || !keep) return fail(MK_E_CAPACITY, "%llu records in the window, room for %llu", (unsigned long long)n, (unsigned long long)rec_cap);
    // ---- record tables -> host; bytes of the n records per source; the tails
    std::vector<uint32_t> rs[2];
    for (uint32_t k = 0; k < n_sources; ++k) {
        rs[k].assign(n + 1, 0);
        if (W[k].n_window && hipMemcpyAsync(rs[k].data(), W[k].d_rec_start, (n + 1) * 4, hipMemcpyDeviceToHost, st) != hipSuccess)
            return fail(MK_E_HIP, "copy of the record table failed");
    }
    if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "copy of the record table failed");
    for (uint32_t k = 0; k < n_sources; ++k) {
        mk_window_source &S = src[k];
        // all of a window that ends at a record end belongs to its records (a last line without '\n' included)
        W[k].n_used = (n == W[k].n_avail && S.ends_at_record) ? W[k].n_window : (W[k].n_window ? rs[k][n] : 0);
        rs[k][n] = (uint32_t)W[k].n_used;
        S.n_used = W[k].n_used;
        S.n_tail = W[k].n_window - W[k].n_used;
        if (S.rec_start)
            for (uint64_t r = 0; r <= n; ++r) S.rec_start[r] = rs[k][r];
        if (front) {  // the text in front of the found start
            if (front->n_front > front->front_cap)
                return fail(MK_E_CAPACITY, "mk_extract_window_open: the text in front of the window's first record takes %llu bytes", (unsigned long long)front->n_front);
            if (front->n_front && hipMemcpyAsync(front->front, W[k].T->d_text, front->n_front, hipMemcpyDeviceToHost, st) != hipSuccess)
                return fail(MK_E_HIP, "download of the front failed");
        }
        if (S.tail || S.tail_cap) {
            if (S.n_tail > S.tail_cap) return fail(MK_E_CAPACITY, "mk_extract_window: the text behind the window's records takes %llu bytes", (unsigned long long)S.n_tail);
            if (S.n_tail && hipMemcpyAsync(S.tail, (const uint8_t *)W[k].T->d_text + W[k].n_used, S.n_tail, hipMemcpyDeviceToHost, st) != hipSuccess)
                return fail(MK_E_HIP, "download of the tail failed");
        }
        if (S.all) {
            if (W[k].n_window > S.all_cap) return fail(MK_E_CAPACITY, "mk_extract_window: the window's text takes %llu bytes", (unsigned long long)W[k].n_window);
            if (W[k].n_window && hipMemcpyAsync(S.all, W[k].T->d_text, W[k].n_window, hipMemcpyDeviceToHost, st) != hipSuccess)
                return fail(MK_E_HIP, "download of the text failed");
        }
    }
    if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "download of the text failed");
    dl.mark(1);
    if (n == 0) return MK_OK;
    // ---- the loop bodies (src/cmd_extract.rs:321-406 single, :463-612 paired) on the first n records of every source
    const uint32_t mode = logging ? MK_MODE_HITS : MK_MODE_ANY;
    std::vector<uint8_t> f[2];
    uint64_t flagged[2] = {0, 0}, n_seq[2] = {0, 0};
    unsigned long long found[2] = {0, 0};
    for (uint32_t k = 0; k < n_sources; ++k) {
        f[k].resize(n);
        if ((rc = scan_sequences(m, W[k], n, kSeqPlain, dl, mode, f[k].data(), &flagged[k], &n_seq[k]))) return rc;
        found[k] = dl.found;
        if (paired && k == 0 && logging && (rc = dl.stash_mate1())) return rc;
    }
    uint64_t total_rows = 0;
    if (logging && !paired) {
        if ((rc = dl.log_single(c, n, n_seq[0], flagged[0], rows, rows_cap))) return rc;
        if ((rc = dl.pattern_counts(ac, n, counts))) return rc;
        total_rows = found[0];
    } else if (logging) {
        total_rows = found[0] + found[1];
        if (!ac && std::max(n_seq[0], n_seq[1]) >= (1ull << 31))  // (BNDMq's pair order keeps the mate in bit 31 of the position)
            return fail(MK_E_UNSUPPORTED, "mk_extract_window: paired windows of 2 GiB of sequence or more under BNDMq");
        if ((rc = dl.log_pair(c, n, n_seq[0] + n_seq[1], found[0], flagged[0], flagged[1], rows, rows_cap, counts))) return rc;
    }
    // ---- keep (single :400-405, paired :600-606), on the host for the caller and on the device for the kept records' text
    dl.host_begin();
    extract_keep(f[0].data(), paired ? f[1].data() : nullptr, n, invert, keep, c);
    dl.mark(1);
    // ---- the kept records leave: their stored text per source that asks for it, or (mem) every source's members
    bool want_kept = mem != nullptr;
    for (uint32_t k = 0; k < n_sources; ++k) want_kept = want_kept || src[k].kept != nullptr || src[k].kept_cap != 0;
    if (want_kept) {
        if ((rc = ensure_device((void **)&m->d_flags2, &m->d_flags2_cap, n + 8))) return rc;
        if (hipMemcpyAsync(m->d_flags2, keep, n, hipMemcpyHostToDevice, st) != hipSuccess) return fail(MK_E_HIP, "upload of the keep flags failed");
        int cap_rc = MK_OK;
        float cut_ms[3] = {0, 0, 0};
        uint64_t cut_members = 0;
        for (uint32_t k = 0; k < n_sources && !*status; ++k) {
            if (mem) rc = window_members(m, codec, kind, format, W[k], n, m->d_flags2, rs[k], keep, logging, mem[k], dl, cut_ms, &cut_members, status);
            else if (src[k].kept || src[k].kept_cap) rc = window_kept(m, W[k], n, m->d_flags2, rs[k], keep, src[k], dl);
            else continue;
            if (rc == MK_E_CAPACITY) cap_rc = rc;  // (every source reports its needs before the call returns)
            else if (rc) return rc;
        }
        if (mem && kind == Packed::kMembers) {
            std::lock_guard<std::mutex> lock(codec->mu);
            for (int k = 0; k < 3; ++k) codec->cut_ms[k] = cut_ms[k];
            codec->cut_members = cut_members;
        }
        if (mem && *status) {  // a record the device does not write: nothing of this window has left as members
            for (uint32_t k = 0; k < n_sources; ++k)
                mem[k].n_member_bytes = mem[k].n_members = mem[k].n_written = mem[k].n_kept = mem[k].n_id_bytes = 0, mem[k].as_text = 0;
            return MK_OK;
        }
        if (cap_rc) return cap_rc;
    }
    dl.finish();
    if (n_rows) *n_rows = total_rows;
    return check_rows_cap(logging, rows, rows_cap, total_rows);
    MK_ABI_END
}
}  // namespace

extern "C" {

int mk_extract_window(mk_matcher *m, mk_codec *codec, uint32_t format, uint32_t n_sources, mk_window_source *src, int logging, int invert,
                      uint64_t rec_cap, uint64_t *n_rec_out, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *c,
                      uint32_t *counts, uint32_t *status) {
    return extract_window_body(m, codec, format, n_sources, src, nullptr, nullptr, Packed::kMembers, logging, invert, rec_cap, n_rec_out, keep, rows, rows_cap, n_rows, c, counts, status);
}

int mk_extract_window_members(mk_matcher *m, mk_codec *codec, uint32_t format, uint32_t n_sources, mk_window_source *src, mk_window_members *mem,
                              int logging, int invert, uint64_t rec_cap, uint64_t *n_rec_out, uint8_t *keep, mk_row *rows, uint64_t rows_cap,
                              uint64_t *n_rows, mk_counters *c, uint32_t *counts, uint32_t *status) {
    if (!mem) return fail(MK_E_INVALID_ARG, "null argument");
    return extract_window_body(m, codec, format, n_sources, src, mem, nullptr, Packed::kMembers, logging, invert, rec_cap, n_rec_out, keep, rows, rows_cap, n_rows, c, counts, status);
}

int mk_extract_window_frames(mk_matcher *m, mk_codec *codec, uint32_t format, uint32_t n_sources, mk_window_source *src, mk_window_members *mem,
                             int logging, int invert, uint64_t rec_cap, uint64_t *n_rec_out, uint8_t *keep, mk_row *rows, uint64_t rows_cap,
                             uint64_t *n_rows, mk_counters *c, uint32_t *counts, uint32_t *status) {
    if (!mem) return fail(MK_E_INVALID_ARG, "null argument");
    return extract_window_body(m, codec, format, n_sources, src, mem, nullptr, Packed::kFrames, logging, invert, rec_cap, n_rec_out, keep, rows, rows_cap, n_rows, c, counts, status);
}

int mk_extract_window_open(mk_matcher *m, mk_codec *codec, uint32_t format, uint32_t n_sources, mk_window_source *src, int logging, int invert,
                           uint64_t rec_cap, uint64_t *n_rec_out, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *c,
                           uint32_t *counts, uint32_t *status, mk_window_front *fronts) {
    // (what only this entry refuses comes first, in front of any use of the handle or the device)
    if (!src || !fronts) return fail(MK_E_INVALID_ARG, "null argument");
    if (n_sources != 1) return fail(MK_E_INVALID_ARG, "mk_extract_window_open: one source -- the two files of a pair cannot be opened independently");
    if (src[0].n_head != 0) return fail(MK_E_INVALID_ARG, "mk_extract_window_open: an open window has no head");
    if (fronts->front_cap && !fronts->front) return fail(MK_E_INVALID_ARG, "mk_extract_window_open: a size without its buffer (front)");
    fronts->n_front = 0;
    return extract_window_body(m, codec, format, n_sources, src, nullptr, fronts, Packed::kMembers, logging, invert, rec_cap, n_rec_out, keep, rows, rows_cap, n_rows, c, counts, status);
}

// (v4 / v5 entry points, kept: one FASTQ source whose window ends at a record end / one bgzip'ed FASTQ source with a head)
int mk_extract_fastq_text(mk_matcher *m, const uint8_t *text, uint64_t n_text, int logging, int invert, uint64_t rec_cap, uint64_t *n_rec_out,
                          uint64_t *rec_start, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *c, uint32_t *counts,
                          uint32_t *status) {
    if (!m || !n_rec_out || !status || !c || (logging && !counts) || (n_text && !text)) return fail(MK_E_INVALID_ARG, "null argument");
    *n_rec_out = 0;
    *status = 0;
    if (n_rows) *n_rows = 0;
    if (n_text == 0) return MK_OK;
    mk_window_source S;
    memset(&S, 0, sizeof(S));
    S.text = text, S.n_text = n_text, S.ends_at_record = 1, S.rec_start = rec_start;
    if (!rec_start) rec_cap = 0;
    return mk_extract_window(m, nullptr, MK_TEXT_FASTQ, 1, &S, logging, invert, rec_cap, n_rec_out, keep, rows, rows_cap, n_rows, c, counts, status);
}

int mk_extract_fastq_bgzf(mk_matcher *m, mk_codec *codec, const uint8_t *head, uint64_t n_head, const uint8_t *bgzf, uint64_t n_bgzf,
                          const mk_bgzf_member *members, uint64_t n_members, int last, mk_window_text *io, int logging, int invert, uint64_t rec_cap, uint64_t *n_rec_out, uint64_t *rec_start, uint8_t *keep,
                          mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *c, uint32_t *counts, uint32_t *status) {
    if (!m || !codec || !io || !n_rec_out || !status || !c || (logging && !counts) || (n_head && !head) ||
        (n_members && (!bgzf || !members)))
        return fail(MK_E_INVALID_ARG, "null argument");
    io->n_text = io->n_used = io->n_tail = io->n_kept_bytes = 0;
    if (!io->text && (!io->tail || (io->kept_cap && !io->kept))) return fail(MK_E_INVALID_ARG, "mk_extract_fastq_bgzf: neither a text buffer nor tail / kept buffers");
    mk_window_source S;
    memset(&S, 0, sizeof(S));
    S.head = head, S.n_head = n_head, S.bgzf = bgzf, S.n_bgzf = n_bgzf, S.members = members, S.n_members = n_members;
    S.ends_at_record = last ? 1 : 0;
    S.rec_start = rec_start;
    if (!rec_start) rec_cap = 0;
    std::vector<uint8_t> dummy(1);
    if (io->text) {
        S.all = io->text, S.all_cap = io->text_cap;
    } else {
        S.tail = io->tail, S.tail_cap = io->tail_cap;
        S.kept = io->kept ? io->kept : dummy.data(), S.kept_cap = io->kept_cap;
    }
    const int rc = mk_extract_window(m, codec, MK_TEXT_FASTQ, 1, &S, logging, invert, rec_cap, n_rec_out, keep, rows, rows_cap, n_rows, c, counts, status);
    io->n_text = S.n_window, io->n_used = S.n_used, io->n_tail = io->text ? 0 : S.n_tail, io->n_kept_bytes = S.n_kept_bytes;
    // (v5 contract: a window without one whole record is the caller's reader's business -- unless nothing follows it)
    if (rc == MK_OK && !*status && S.n_window && S.n_used == 0) *status = last ? 0u : 1u;
    return rc;
}

}  // extern "C"
