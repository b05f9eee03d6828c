// tag_windows.cpp -- `tag` on a window that stays on the device (r05, ABI v7 and its additions; kernels: bam.hip, sam.hip): the four
// mk_tag_*_window, each one of two input sides, the shared scan and keep steps, and one of two output sides
#include <functional>
#include <mutex>

#include "device_loop.hpp"
#include "sam_numbers.hpp"
#include "codec/codec_internal.h"
#include "codec/codec_kernels.h"

using namespace mk;

namespace {

constexpr int kBamProofRounds = 8;  // walks of the record chain before a window is left to the host reader

// the record chain of text[0, n) -> W's tables (d_rec_start = record offsets, d_seq_start, d_seq_len; rec_len behind them):
// *n_rec records covering *n_used bytes; W.fixed > 0: every sequence has this length.  *status |= 1: not for the device.
int bam_index(mk_matcher *m, WindowSide &W, hipStream_t st, uint64_t *n_rec, uint64_t *n_used, uint32_t **d_rec_len, uint32_t *status) {
    mk_matcher::TextSlot &T = *W.T;
    const uint64_t n = W.n_window;
    const uint8_t *d_text = (const uint8_t *)T.d_text;
    const uint32_t piece = m->bam_piece ? m->bam_piece : 65536u;
    const uint32_t n_pieces = (uint32_t)((n + piece - 1) / piece);
    int rc;
    // d_ing_a: start | land | count | base (u32 per piece each) | st[4]
    if ((rc = ensure_device(&T.d_ing_a, &T.d_ing_a_cap, ((size_t)n_pieces * 4 + 8) * 4))) return rc;
    uint32_t *d_start = (uint32_t *)T.d_ing_a, *d_land = d_start + n_pieces, *d_count = d_land + n_pieces, *d_base = d_count + n_pieces,
             *d_st = d_base + n_pieces;
    launch_bam_find(d_text, n, piece, n_pieces, d_start, st);
    std::vector<uint32_t> start(n_pieces), land(n_pieces), count(n_pieces);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(start.data(), d_start, (size_t)n_pieces * 4, hipMemcpyDeviceToHost, st) != hipSuccess)
        return fail(MK_E_HIP, "BAM record search failed");
    bool proved = false;
    std::vector<uint8_t> valid(n_pieces);
    for (int round = 0; round < kBamProofRounds && !proved; ++round) {
        launch_bam_walk_count(d_text, n, piece, n_pieces, d_start, d_land, d_count, st);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(land.data(), d_land, (size_t)n_pieces * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipMemcpyAsync(count.data(), d_count, (size_t)n_pieces * 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail(MK_E_HIP, "BAM record walk failed");
        // Piece 0 starts at a record start (the caller's contract); a walk that lands on the next piece's start makes that one too.
        // One pass from the left: a start that is not met is replaced by the landing -- which is right, because everything to its
        // left is -- and its own landing is then unknown (valid = 0) until the next walk, unless the new start lies behind the
        // piece altogether (a record longer than a piece: nothing starts in it, the walk is the identity).
        std::fill(valid.begin(), valid.end(), 1);
        proved = true;
        for (uint32_t p = 0; p < n_pieces; ++p) {
            if (!valid[p]) {
                const uint64_t stop = p + 1 < n_pieces ? (uint64_t)(p + 1) * piece : n;
                if (start[p] != 0xFFFFFFFFu && start[p] >= stop) {
                    land[p] = start[p], count[p] = 0, valid[p] = 1;
                } else {
                    proved = false;
                    continue;
                }
            }
            if (count[p] & 0x80000000u) {  // the text ends inside the record at land[p]: nothing whole follows it
                for (uint32_t q = p + 1; q < n_pieces; ++q) start[q] = land[q] = land[p], count[q] = 0;
                break;
            }
            if (p + 1 < n_pieces && land[p] != 0xFFFFFFFFu && start[p + 1] != land[p]) {
                start[p + 1] = land[p];
                valid[p + 1] = 0;
            }
        }
        if (hipMemcpyAsync(d_start, start.data(), (size_t)n_pieces * 4, hipMemcpyHostToDevice, st) != hipSuccess) return fail(MK_E_HIP, "copy failed");
    }
    for (uint32_t p = 0; p < n_pieces; ++p) proved = proved && start[p] != 0xFFFFFFFFu;
    if (!proved) {
        *status |= 1;
        return MK_OK;
    }
    std::vector<uint32_t> base(n_pieces);
    uint64_t total = 0;
    for (uint32_t p = 0; p < n_pieces; ++p) {
        base[p] = (uint32_t)total;
        total += count[p] & 0x7FFFFFFFu;
    }
    *n_rec = total;
    *n_used = n_pieces ? land[n_pieces - 1] : 0;
    if (total >= 0xFFFFFFF0ull) return fail(MK_E_UNSUPPORTED, "%llu records in one BAM window", (unsigned long long)total);
    // tables: record offsets | sequence starts | sequence lengths | record lengths | out lengths | existing-tag offsets | (BAM -> SAM: where SEQ starts in
    // the line) (u32, n + 2 each) | out offsets (u64) | tiles (u64)
    const size_t n_tiles = total / ingest_scan_tile() + 2;
    if ((rc = ensure_device(&T.d_ing_b, &T.d_ing_b_cap, 7 * (total + 2) * 4 + 16 + (total + 2) * 8 + n_tiles * 8 + 64))) return rc;
    W.d_rec_start = (uint32_t *)T.d_ing_b;
    W.d_seq_start = W.d_rec_start + total + 2;
    W.d_seq_len = W.d_seq_start + total + 2;
    *d_rec_len = W.d_seq_len + total + 2;
    const uint32_t st_init[4] = {0u, 0xFFFFFFFFu, 0u, 0u};
    if (hipMemcpyAsync(d_base, base.data(), (size_t)n_pieces * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemcpyAsync(d_st, st_init, sizeof(st_init), hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(MK_E_HIP, "copy failed");
    launch_bam_walk_emit(d_text, n, piece, n_pieces, d_start, d_base, W.d_rec_start, *d_rec_len, W.d_seq_start, W.d_seq_len, d_st, st);
    uint32_t st_host[4] = {0, 0, 0, 0};
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(st_host, d_st, sizeof(st_host), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "BAM record indexing failed");
    if (st_host[0]) *status |= 1;  // a record the serial parser refuses ("truncated file"): the host reader words it
    W.fixed = (total && st_host[1] == st_host[2] && st_host[1] > 0) ? st_host[1] : 0;
    W.d_st = d_st;
    return MK_OK;
}

// names[0, total) = the NUL-terminated names of the flagged records among n, in record order; rows in emission order (record-major
// in both orders) -> row_name[k] = where the name of row k's record starts: a walk along both
void name_rows(const mk_row *rows, uint64_t n_rows, const uint8_t *flags, uint64_t n, const uint8_t *names, uint64_t total, uint64_t *row_name) {
    uint64_t r = 0, at = 0;  // r = the flagged record whose name starts at `at`
    while (r < n && !flags[r]) ++r;
    for (uint64_t k = 0; k < n_rows; ++k) {
        const uint64_t rec = rows[k].rec;
        while (r < rec && at < total) {
            at += strlen((const char *)names + at) + 1;
            ++r;
            while (r < n && !flags[r]) ++r;
        }
        row_name[k] = at;
    }
}

double ms_since(std::chrono::steady_clock::time_point &t) {
    const auto now = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(now - t).count();
    t = now;
    return ms;
}

// ---- `tag` on a window that stays on the device: what the four mk_tag_*_window share.  An entry point is one of two input sides, which
// make the record table (bam_front: BGZF members behind a head, the record chain / sam_index: SAM text, the line table and
// mk_sam_fields_kernel), then tag_scan and tag_keep, then one of two output sides, which send the kept records off (members_back: BGZF
// members / text_back: text), then tag_commit.
// ms[7] of such a call: the time spent growing device buffers inside it (part of the phases, reported on its own)
struct AllocMs {
    float *out;
    explicit AllocMs(float *out_) : out(out_) { g_alloc_ms = 0, g_free_ms = 0; }
    ~AllocMs() { *out = (float)g_alloc_ms; }
};

// One such window between the steps: the fields of mk_bam_window / mk_sam_window that the steps use, the record table's per-record
// arrays, and what a step leaves for the next one
struct TagWindow {
    const char *who;  // the entry point, for its messages
    mk_row *rows;
    uint64_t rows_cap, *row_name;
    uint8_t *names;
    uint64_t names_cap, *n_kept, *n_rows, *n_names_bytes;
    uint64_t n;  // records
    uint32_t *d_out_len, *d_ex_off;
    unsigned long long *d_out_off;
    const uint32_t *d_qname_len;  // SAM: the QNAMEs' lengths (BAM's names are found from the records)
    // tag_scan ->
    std::vector<uint8_t> flags;  // records with a hit; after tag_keep: the kept records
    mk_counters lc{};            // counters of this window: added to the caller's only when the window is done (tag_commit) -- a refused
    std::vector<uint32_t> lcounts;  // or repeated window counts nothing
    unsigned long long *d_found_off = nullptr;
    uint32_t *d_found_pat = nullptr;
    unsigned long long out_text = 0;  // tag_keep -> bytes of the kept records with their tags
};
template <class Win>
TagWindow tag_window(Win *w, const char *who, uint64_t n, uint32_t *d_out_len, uint32_t *d_ex_off, unsigned long long *d_out_off, const uint32_t *d_qname_len) {
    return TagWindow{who, w->rows, w->rows_cap, w->row_name, w->names, w->names_cap, &w->n_kept, &w->n_rows, &w->n_names_bytes, n, d_out_len, d_ex_off, d_out_off,
                     d_qname_len};
}

// sequences -> the scan buffer, scan, log rows with the names of their records, emission order, pattern sets
int tag_scan(mk_matcher *m, DeviceLoop &dl, const WindowSide &W, TagWindow &X, SeqForm form, int logging) {
    hipStream_t st = dl.st;
    const uint64_t n = X.n;
    const uint8_t *d_text = (const uint8_t *)W.T->d_text;
    int rc;
    uint64_t flagged = 0, n_seq = 0;
    X.flags.resize(n);
    if ((rc = scan_sequences(m, W, n, form, dl, MK_MODE_HITS, X.flags.data(), &flagged, &n_seq))) return rc;
    const bool ac = m->algo == MK_ALGO_AC;
    bool set_order = false;
    uint64_t n_rows = 0;
    X.lcounts.assign(logging ? m->n_pat : 0, 0);
    if (logging) {  // src/cmd_tag.rs:400-416, :443-451
        n_rows = dl.found;
        if ((rc = dl.log_single(&X.lc, n, n_seq, flagged, X.rows, X.rows_cap))) return rc;
        set_order = !ac;
        if (ac && (rc = dl.pattern_counts(true, n, X.lcounts.data()))) return rc;
        // the names of the records with a hit, NUL-terminated, in record order; a row finds its record's by a walk along both.
        // BAM: read_name with its NUL.  SAM: QNAME gathered with the tab behind it, which then becomes the NUL.
        if (flagged) {
            const bool sam = form == kSeqSam;
            uint32_t *d_name_len = sam ? X.d_out_len : (uint32_t *)X.d_out_off;       // (both free until the tag step)
            const uint32_t *d_name_start = sam ? W.d_rec_start : X.d_out_len;
            unsigned long long *d_name_off = (unsigned long long *)m->d_off;          // (the scan is done with the sequence offsets)
            unsigned long long total = 0;
            if (sam) launch_sam_names(X.d_qname_len, m->d_flags, n, d_name_len, st);
            else launch_bam_names(d_text, W.d_rec_start, m->d_flags, n, X.d_out_len, d_name_len, st);
            if ((rc = scan_offsets(d_name_len, n, W.d_tile, d_name_off, st, &total, "selection of the names failed"))) return rc;
            *X.n_names_bytes = total;
            if (total <= X.names_cap && n_rows <= X.rows_cap) {
                // (the sequences have been scanned: their buffer holds the names now)
                if ((rc = pack_gather(m, W, d_name_start, d_name_len, n, total, 0, 0xFFFFFFFFu, st, "download of the names failed"))) return rc;
                if (sam) launch_sam_name_ends(d_name_len, d_name_off, n, m->d_seq, st);
                if ((rc = pack_download(m, X.names, total, st, "download of the names failed"))) return rc;
                name_rows(X.rows, n_rows, X.flags.data(), n, X.names, total, X.row_name);
            }
        }
    }
    *X.n_rows = n_rows;
    if (!set_order && (rc = dl.order(false, n))) return rc;
    uint32_t *d_cnt = nullptr;
    uint64_t n_found = 0;
    if ((rc = dl.pattern_sets_device(n, logging && !ac, &X.d_found_off, &X.d_found_pat, &d_cnt, &n_found))) return rc;
    if (logging && !ac && n_found) {  // BNDMq: one count per record and pattern (:431-433)
        if (hipMemcpy(X.lcounts.data(), d_cnt, (size_t)m->n_pat * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(MK_E_HIP, "copy of the counts failed");
    }
    return MK_OK;
}

// keep or drop and the size every kept record leaves with (`taglen`: the format's kernel, which fills m->d_flags2, d_out_len,
// d_ex_off and W.d_st), where each goes (d_out_off), and whether the rows and names fit.  *status != 0: optional fields the device does
// not decide about (the kernel's bits & status_mask) -- this window is the host path's, nothing further is set.
int tag_keep(mk_matcher *m, DeviceLoop &dl, const WindowSide &W, TagWindow &X, int logging, uint32_t status_mask, const std::function<void()> &taglen,
             uint32_t *status) {
    hipStream_t st = dl.st;
    const uint64_t n = X.n;
    int rc;
    if ((rc = ensure_device((void **)&m->d_flags2, &m->d_flags2_cap, n + 8))) return rc;
    if (hipMemsetAsync(W.d_st, 0, 4, st) != hipSuccess) return fail(MK_E_HIP, "hipMemsetAsync failed");
    taglen();
    launch_ingest_offsets(X.d_out_len, n, W.d_tile, X.d_out_off, st);
    unsigned long long out_text = 0;
    uint32_t st_tag = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&out_text, X.d_out_off + n, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&st_tag, W.d_st, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipMemcpyAsync(X.flags.data(), m->d_flags2, n, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "tag kernels failed");
    if (st_tag) {
        *status = st_tag & status_mask;
        return MK_OK;
    }
    uint64_t kept = 0;
    for (uint64_t r = 0; r < n; ++r) kept += X.flags[r];
    *X.n_kept = kept;
    X.lc.nb_records_extracted = kept;
    X.out_text = out_text;
    if (logging && (*X.n_rows > X.rows_cap || *X.n_names_bytes > X.names_cap))
        return fail(MK_E_CAPACITY, "%s: %llu rows and %llu bytes of names", X.who, (unsigned long long)*X.n_rows, (unsigned long long)*X.n_names_bytes);
    return MK_OK;
}

// the window is done: its counters join the caller's
void tag_commit(DeviceLoop &dl, const TagWindow &X, mk_counters *c, uint32_t *counts) {
    c->nb_records_tot += X.lc.nb_records_tot, c->nb_bases += X.lc.nb_bases, c->nb_hits_tot[0] += X.lc.nb_hits_tot[0];
    c->nb_records_hit[0] += X.lc.nb_records_hit[0], c->nb_records_extracted += X.lc.nb_records_extracted;
    for (size_t i = 0; i < X.lcounts.size(); ++i) counts[i] += X.lcounts[i];
    dl.finish();
}

// What every mk_tag_*_window starts with.  tag_args: the checks all four make (handles = the handles the entry point takes are there);
// the entry point's own checks follow it.  TAG_WINDOW_BEGIN, behind those: nothing reported yet, the device, and the call's dl, st, rc,
// t (the phase clock) and ms[7].
template <class Win>
int tag_args(const char *who, bool handles, const Win *w, const mk_counters *c, const uint32_t *counts, const uint32_t *status, int logging) {
    if (!handles || !w || !c || !status || (logging && !counts)) return fail(MK_E_INVALID_ARG, "null argument");
    if ((w->n_head && !w->head) || (w->tail_cap && !w->tail) || (w->out_cap && !w->out) || (logging && w->rows_cap && (!w->rows || !w->row_name)) ||
        (w->names_cap && !w->names))
        return fail(MK_E_INVALID_ARG, "%s: a size without its buffer", who);
    return MK_OK;
}
#define TAG_WINDOW_BEGIN                                                                                        \
    w->n_window = w->n_used = w->n_tail = w->n_rec = w->n_kept = w->out_len = w->n_rows = w->n_names_bytes = 0; \
    for (float &x : w->ms) x = 0;                                                                               \
    *status = 0;                                                                                                \
    if (hipSetDevice(m->device) != hipSuccess) return fail(MK_E_HIP, "hipSetDevice failed");                    \
    DeviceLoop dl(m);                                                                                           \
    hipStream_t st = dl.st;                                                                                     \
    int rc;                                                                                                     \
    auto t = std::chrono::steady_clock::now();                                                                  \
    AllocMs alloc_ms(&w->ms[7]);

// ---- the two output sides
// the window's tagged records, back to back in text slot 1 (out_text bytes, kPad zero bytes behind them), deflated into BGZF members of
// bb bytes of text and downloaded: the last step of mk_tag_bam_window and mk_tag_sam_bam_window (the codec's buffers; its kernels on
// this stream).  *out_len = the members' bytes (more than out_cap: MK_E_CAPACITY); ms_deflate / ms_download: the two phases.
int window_deflate(mk_matcher *m, mk_codec *codec, const WindowSide &W, DeviceLoop &dl, const char *who, unsigned long long out_text, uint32_t bb, uint8_t *out,
                   uint64_t out_cap, uint64_t *out_len, float *ms_deflate, float *ms_download, std::chrono::steady_clock::time_point &t) {
    hipStream_t st = dl.st;
    int rc;
    mk_matcher::TextSlot &O = m->txt[1];
    std::lock_guard<std::mutex> lock(codec->mu);
    const uint64_t blocks64 = (out_text + bb - 1) / bb;
    if (blocks64 >= 0xFFFFFFFFull) return fail(MK_E_UNSUPPORTED, "%s: %llu output members", who, (unsigned long long)blocks64);
    const uint32_t blocks = (uint32_t)blocks64;
    // the packed members go where the window's text was: it has been read for the last time by the record output kernel (a buffer
    // of the output's size less to grow -- growing device buffers is what a job's first windows spend most of their time on)
    void *d_packed = nullptr;
    uint64_t total = 0;
    if ((rc = mkz::deflate_pass(codec, st, (const uint8_t *)O.d_text, out_text, bb, nullptr, nullptr, blocks, W.T->d_text, W.T->d_text_cap, &d_packed, &total))) return rc;
    *ms_deflate = (float)ms_since(t);
    *out_len = total;
    if (total > out_cap) return fail(MK_E_CAPACITY, "%s: the members take %llu bytes", who, (unsigned long long)total);
    if (hipMemcpyAsync(out, d_packed, total, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "download of the members failed");
    *ms_download = (float)ms_since(t);
    return MK_OK;
}

// The members output: what mk_tag_bam_window and mk_tag_sam_bam_window end with.  rc = tag_keep's; `emit` writes the kept records back to
// back to where it is told (the format's kernels, as `taglen`; `emit_failed` words their failure).  ms[0..2]: emit, deflate, download;
// a window that writes nothing (no output buffer: the checks have run / nothing is kept) stamps ms[0] where stamp_idle says so.
template <class Win>
int members_back(mk_matcher *m, mk_codec *codec, Win *w, const WindowSide &W, const TagWindow &X, DeviceLoop &dl, int rc, const uint32_t *status, uint32_t bb,
                 float *ms, bool stamp_idle, const char *emit_failed, const std::function<int(uint8_t *)> &emit, std::chrono::steady_clock::time_point &t) {
    hipStream_t st = dl.st;
    const unsigned long long out_text = X.out_text;
    w->out_text_bytes = out_text;
    if (rc || *status) return rc;
    if ((!w->out && !w->out_cap) || out_text == 0) {
        if (stamp_idle) ms[0] = (float)ms_since(t);
        return MK_OK;
    }
    mk_matcher::TextSlot &O = m->txt[1];
    if ((rc = ensure_device(&O.d_text, &O.d_text_cap, out_text + mkz::kPad + 64)) || (rc = emit((uint8_t *)O.d_text))) return rc;
    if (hipGetLastError() != hipSuccess || hipMemsetAsync((uint8_t *)O.d_text + out_text, 0, mkz::kPad, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "%s", emit_failed);
    ms[0] = (float)ms_since(t);
    return window_deflate(m, codec, W, dl, X.who, out_text, bb, w->out, w->out_cap, &w->out_len, &ms[1], &ms[2], t);
}

// The text output: what mk_tag_sam_window and mk_tag_bam_sam_window end with.  rc = tag_keep's; out_len is reported whatever became of the
// window; `emit` writes the kept lines back to back to where it is told.  ms[0..1]: emit, download.
template <class Win>
int text_back(mk_matcher *m, Win *w, const TagWindow &X, DeviceLoop &dl, int rc, const uint32_t *status, float *ms, const char *emit_failed,
              const std::function<void(uint8_t *)> &emit, std::chrono::steady_clock::time_point &t) {
    hipStream_t st = dl.st;
    const unsigned long long out_text = X.out_text;
    const bool write = w->out || w->out_cap;
    if (write) w->out_len = out_text;
    if (rc || *status) return rc;
    if (write && out_text > w->out_cap) return fail(MK_E_CAPACITY, "%s: the kept lines take %llu bytes", X.who, out_text);
    if (write && out_text) {
        mk_matcher::TextSlot &O = m->txt[1];
        if ((rc = ensure_device(&O.d_text, &O.d_text_cap, out_text + 64))) return rc;
        emit((uint8_t *)O.d_text);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "%s", emit_failed);
        ms[0] = (float)ms_since(t);
        if (hipMemcpyAsync(w->out, O.d_text, out_text, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail(MK_E_HIP, "download of the kept lines failed");
        ms[1] = (float)ms_since(t);
    } else {
        ms[0] = (float)ms_since(t);
    }
    return MK_OK;
}

// ---- the two input sides
// a window of SAM text -> its record tables: what mk_tag_sam_window and mk_tag_sam_bam_window start with
struct SamIndex {
    uint64_t n = 0;  // records
    SamTables R{};
    uint32_t *d_out_len = nullptr, *d_ex_off = nullptr, *d_extra = nullptr;  // one entry per line each (d_extra: `extra` of them)
    unsigned long long *d_out_off = nullptr;
};
// upload (ms[0]), line table and fields (ms[1]), n_window / n_rec / n_used / the tail; *status = 1: a record line with fewer than 10 fields
template <class Win>
int sam_index(mk_matcher *m, Win *w, const char *who, uint32_t extra, DeviceLoop &dl, WindowSide &W, SamIndex &I, uint32_t *status,
              std::chrono::steady_clock::time_point &t) {
    hipStream_t st = dl.st;
    int rc;
    // ---- the text: head, then the body behind it
    W.T = &m->txt[0];
    mk_matcher::TextSlot &T = *W.T;
    mk_window_source S;
    memset(&S, 0, sizeof(S));
    S.head = w->head, S.n_head = w->n_head, S.text = w->text, S.n_text = w->n_text;
    if ((rc = window_assemble(m, nullptr, S, W, dl))) return rc;
    if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "upload of the window failed");
    w->ms[0] = (float)ms_since(t);
    w->n_window = W.n_window;
    const uint64_t n_text = W.n_window;
    if (n_text == 0) return MK_OK;  // (I.n == 0)
    const uint8_t *d_text = (const uint8_t *)T.d_text;
    // ---- line table (ingest.hip), then what every line is (sam.hip)
    if ((rc = line_table(W, st, 0, nullptr))) return rc;
    // a last line without '\n' is a line when nothing follows the window, else the next window's head
    const bool open_end = W.last_byte != '\n';
    const uint64_t n_lines = (uint64_t)W.total_nl + (w->last && open_end ? 1 : 0);
    const size_t per = n_lines + 2, n_tiles = n_lines / ingest_scan_tile() + 2;
    // line starts | record-or-not | six entries per line | out lengths | existing-value offsets | `extra` more arrays (u32) | offsets (u64) | tiles (u64)
    if ((rc = ensure_device(&T.d_ing_b, &T.d_ing_b_cap, ((size_t)W.total_nl + 4 + (9 + extra) * per) * 4 + 16 + per * 8 + n_tiles * 8 + 64))) return rc;
    W.d_line = (uint32_t *)T.d_ing_b;
    uint32_t *d_is_rec = W.d_line + W.total_nl + 4;
    SamTables L{d_is_rec + per, d_is_rec + 2 * per, d_is_rec + 3 * per, d_is_rec + 4 * per, d_is_rec + 5 * per, d_is_rec + 6 * per};
    uint32_t *d_out_len = d_is_rec + 7 * per, *d_ex_off = d_is_rec + 8 * per;
    I.d_extra = d_is_rec + 9 * per;
    unsigned long long *d_out_off = (unsigned long long *)(((uintptr_t)(d_is_rec + (9 + extra) * per) + 15) & ~(uintptr_t)15);
    W.d_tile = d_out_off + per;
    launch_ingest_lines(d_text, n_text, W.d_block, W.d_total, W.d_line, st);
    const uint32_t st_init[3] = {0u, 0xFFFFFFFFu, 0u};
    if (hipMemcpyAsync(W.d_st, st_init, sizeof(st_init), hipMemcpyHostToDevice, st) != hipSuccess) return fail(MK_E_HIP, "copy failed");
    launch_sam_fields(d_text, W.d_line, n_lines, d_is_rec, L, W.d_st, st);
    unsigned long long n_rec_dev = 0;
    if (n_lines && (rc = scan_offsets(d_is_rec, n_lines, W.d_tile, d_out_off, st, &n_rec_dev, "SAM line indexing failed"))) return rc;
    uint32_t st_host[3] = {0, 0, 0};
    if (hipMemcpyAsync(st_host, W.d_st, sizeof(st_host), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "SAM line indexing failed");
    if (st_host[0]) {  // a record line with fewer than 10 fields: the host reader words it
        *status = 1;
        return MK_OK;
    }
    const uint64_t n = n_rec_dev;
    SamTables R = L;
    if (n != n_lines) {  // header or empty lines among the records: the records' entries move to tables of their own
        if ((rc = ensure_device(&T.d_fa_seq, &T.d_fa_seq_cap, 6 * (size_t)(n + 2) * 4))) return rc;
        uint32_t *r0 = (uint32_t *)T.d_fa_seq;
        R = SamTables{r0, r0 + (n + 2), r0 + 2 * (n + 2), r0 + 3 * (n + 2), r0 + 4 * (n + 2), r0 + 5 * (n + 2)};
        launch_sam_compact(d_is_rec, d_out_off, n_lines, L, R, st);
        if (hipGetLastError() != hipSuccess) return fail(MK_E_HIP, "SAM line indexing failed");
    }
    W.d_rec_start = R.rec_start, W.d_seq_start = R.seq_start, W.d_seq_len = R.seq_len;
    W.fixed = (n && st_host[1] == st_host[2] && st_host[1] > 0) ? st_host[1] : 0;
    uint64_t used = n_text;
    if (!w->last && open_end) {  // the bytes behind the last '\n' are the tail
        uint32_t last_start = 0;
        if (hipMemcpyAsync(&last_start, W.d_line + W.total_nl, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail(MK_E_HIP, "SAM line indexing failed");
        used = last_start;
    }
    w->n_rec = n, w->n_used = used, w->n_tail = n_text - used;
    if (w->n_tail > w->tail_cap) return fail(MK_E_CAPACITY, "%s: the text behind the window's last line end takes %llu bytes", who, (unsigned long long)w->n_tail);
    if (w->n_tail && (hipMemcpyAsync(w->tail, d_text + used, w->n_tail, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess))
        return fail(MK_E_HIP, "download of the tail failed");
    w->ms[1] = (float)ms_since(t);
    I.n = n, I.R = R, I.d_out_len = d_out_len, I.d_ex_off = d_ex_off, I.d_out_off = d_out_off;
    return MK_OK;
}

// a window of BGZF members -> its record table: what mk_tag_bam_window and mk_tag_bam_sam_window start with
struct BamIndex {
    uint64_t n = 0;  // records
    uint32_t *d_rec_len = nullptr, *d_out_len = nullptr, *d_ex_off = nullptr, *d_extra = nullptr;  // one entry per record each (d_extra: `extra` of them)
    unsigned long long *d_out_off = nullptr;
};
// head, then the members inflated behind it (window_assemble: upload, inflate, CRC-32 / ISIZE of every member; ms[0], ms[1]), the record
// chain, n_window / n_rec / n_used, the tail and on_tail (ms[2]); *status = 1: bam_index's, 8: the file ends inside a record
template <class Win>
int bam_front(mk_matcher *m, mk_codec *codec, Win *w, const char *who, uint32_t extra, DeviceLoop &dl, WindowSide &W, BamIndex &I, uint32_t *status,
              std::chrono::steady_clock::time_point &t) {
    hipStream_t st = dl.st;
    int rc;
    W.T = &m->txt[0];
    mk_window_source S;
    memset(&S, 0, sizeof(S));
    S.head = w->head, S.n_head = w->n_head, S.bgzf = w->bgzf, S.n_bgzf = w->n_bgzf, S.members = w->members, S.n_members = w->n_members;
    if ((rc = window_assemble(m, codec, S, W, dl))) return rc;
    if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "upload of the window failed");
    w->ms[1] = (float)ms_since(t);  // (upload + inflate: batch_ms splits them)
    w->ms[0] = m->batch_ms[0];
    w->ms[1] -= w->ms[0];
    w->n_window = W.n_window;
    const uint64_t n_text = W.n_window;
    if (n_text == 0) return MK_OK;  // (I.n == 0)
    uint64_t n = 0, n_used = 0;
    if ((rc = bam_index(m, W, st, &n, &n_used, &I.d_rec_len, status)) || *status) return rc;
    if (w->last && n_used != n_text) {  // the file ends inside a record
        *status = 8;
        return MK_OK;
    }
    w->n_rec = n, w->n_used = n_used, w->n_tail = n_text - n_used;
    if (w->n_tail > w->tail_cap) return fail(MK_E_CAPACITY, "%s: the text behind the window's records takes %llu bytes", who, (unsigned long long)w->n_tail);
    if (w->n_tail && hipMemcpyAsync(w->tail, (const uint8_t *)W.T->d_text + n_used, w->n_tail, hipMemcpyDeviceToHost, st) != hipSuccess)
        return fail(MK_E_HIP, "download of the tail failed");
    if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "download of the tail failed");
    if (w->on_tail) w->on_tail(w->on_tail_ctx, w->tail, w->n_tail);
    w->ms[2] = (float)ms_since(t);
    // behind the record lengths (bam_index has made the room): out lengths | existing-tag offsets | `extra` more arrays (u32) | offsets (u64) | tiles (u64)
    I.n = n, I.d_out_len = I.d_rec_len + n + 2, I.d_ex_off = I.d_out_len + n + 2, I.d_extra = I.d_ex_off + n + 2;
    I.d_out_off = (unsigned long long *)(((uintptr_t)(I.d_ex_off + (1 + extra) * (n + 2)) + 15) & ~(uintptr_t)15);
    W.d_tile = I.d_out_off + n + 2;
    return MK_OK;
}

// The reference names of a SAM -> BAM window on the device: offsets (u32) | table | bytes.  The host builds an open-addressing table of
// them -- a few thousand names in most files, 10^5 in some assemblies -- with the first of equal names in it (BamWriter::encode_record's
// ref_id takes the first), so the kernel never walks the list.  A job's windows all bring the same names: the handle keeps a copy of
// what it made the device's from, and a window whose names equal it (one memcmp) uploads nothing.
struct SamRefsDevice {
    const uint8_t *bytes = nullptr;
    const uint32_t *off = nullptr, *table = nullptr;
    uint32_t mask = 0;
};
// (with_table = false: mk_tag_bam_sam_window, which finds a name by its index -- names a table was made for serve it as they are)
int upload_refs(mk_matcher *m, const char *who, bool with_table, const uint8_t *names, const uint64_t *off, uint64_t n_refs, hipStream_t st, SamRefsDevice &D) {
    if (!n_refs) return MK_OK;
    for (uint64_t i = 1; i <= n_refs; ++i)
        if (off[i] < off[i - 1]) return fail(MK_E_INVALID_ARG, "%s: reference name offsets must ascend", who);
    const uint64_t n_bytes = off[n_refs] - off[0];
    if (n_refs >= (1u << 30) || n_bytes >= 0xFFFFFFF0ull) return fail(MK_E_UNSUPPORTED, "%s: %llu reference names", who, (unsigned long long)n_refs);
    const uint8_t *base = names + off[0];
    bool same = m->refs_valid && (m->refs_slots || !with_table) && m->refs_off.size() == n_refs + 1 && m->refs_names.size() == n_bytes &&
                memcmp(m->refs_names.data(), base, n_bytes) == 0;
    for (uint64_t i = 0; same && i <= n_refs; ++i) same = m->refs_off[i] == off[i] - off[0];
    if (!same) {
        m->refs_valid = false, m->refs_slots = 0;  // (until the new ones are up)
        uint32_t slots = with_table ? 16 : 0;
        while (with_table && slots < 2 * n_refs) slots <<= 1;
        std::vector<uint32_t> h(n_refs + 1 + slots, 0);
        uint32_t *table = h.data() + n_refs + 1;
        for (uint64_t i = 0; i <= n_refs; ++i) h[i] = (uint32_t)(off[i] - off[0]);
        for (uint64_t i = 0; with_table && i < n_refs; ++i) {
            const uint32_t a = h[i], n = h[i + 1] - h[i];
            for (uint32_t slot = sam_name_hash(base + a, n) & (slots - 1);; slot = (slot + 1) & (slots - 1)) {
                if (!table[slot]) {
                    table[slot] = (uint32_t)i + 1;
                    break;
                }
                const uint32_t j = table[slot] - 1;
                if (h[j + 1] - h[j] == n && memcmp(base + h[j], base + a, n) == 0) break;  // (an earlier reference of that name)
            }
        }
        int rc;
        if ((rc = ensure_device(&m->d_refs, &m->d_refs_cap, h.size() * 4 + n_bytes + 64))) return rc;
        uint8_t *d = (uint8_t *)m->d_refs;
        if (hipMemcpyAsync(d, h.data(), h.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess ||
            (n_bytes && hipMemcpyAsync(d + h.size() * 4, base, n_bytes, hipMemcpyHostToDevice, st) != hipSuccess) || hipStreamSynchronize(st) != hipSuccess)
            return fail(MK_E_HIP, "upload of the reference names failed");
        m->refs_names.assign(base, base + n_bytes);
        m->refs_off.resize(n_refs + 1);
        for (uint64_t i = 0; i <= n_refs; ++i) m->refs_off[i] = off[i] - off[0];
        m->refs_slots = slots;
        m->refs_valid = true;
    }
    const uint8_t *d = (const uint8_t *)m->d_refs;
    D.off = (const uint32_t *)d, D.table = D.off + n_refs + 1, D.bytes = d + ((size_t)n_refs + 1 + m->refs_slots) * 4, D.mask = m->refs_slots - 1;
    return MK_OK;
}
}  // namespace

extern "C" {

int mk_matcher_set_bam_piece(mk_matcher *m, uint32_t piece_bytes) {
    if (!m || (piece_bytes && piece_bytes < 64)) return fail(MK_E_INVALID_ARG, "mk_matcher_set_bam_piece: handle / a piece of at least 64 bytes");
    m->bam_piece = piece_bytes;
    return MK_OK;
}

int mk_tag_bam_window(mk_matcher *m, mk_codec *codec, mk_bam_window *w, int logging, mk_counters *c, uint32_t *counts, uint32_t *status) {
    static const char who[] = "mk_tag_bam_window";
    if (int bad = tag_args(who, m && codec, w, c, counts, status, logging)) return bad;
    if (w->n_members && (!w->bgzf || !w->members)) return fail(MK_E_INVALID_ARG, "mk_tag_bam_window: a size without its buffer");
    const uint32_t bb = w->block_bytes ? w->block_bytes : mkz::kMaxBlockBytes;
    if (bb > mkz::kMaxBlockBytes) return fail(MK_E_INVALID_ARG, "mk_tag_bam_window: block_bytes %u > %u", bb, mkz::kMaxBlockBytes);
    w->out_text_bytes = 0;
    MK_ABI_BEGIN
    TAG_WINDOW_BEGIN
    WindowSide W;
    BamIndex I;
    if ((rc = bam_front(m, codec, w, who, 0, dl, W, I, status, t)) || *status || I.n == 0) return rc;
    const uint64_t n = I.n;
    const uint8_t *d_text = (const uint8_t *)W.T->d_text;
    TagWindow X = tag_window(w, who, n, I.d_out_len, I.d_ex_off, I.d_out_off, nullptr);
    // ---- sequences -> the scan buffer, scan, emission order, pattern sets
    if ((rc = tag_scan(m, dl, W, X, kSeqBam, logging))) return rc;
    w->ms[3] = (float)ms_since(t);
    // ---- keep, tag, pack
    rc = tag_keep(m, dl, W, X, logging, 6u, [&] {
        launch_bam_taglen(d_text, W.d_rec_start, I.d_rec_len, W.d_seq_start, W.d_seq_len, X.d_found_off, X.d_found_pat, m->d_pat_off, m->d_pat_bytes, n,
                          w->filter_matching != 0, w->invert != 0, w->tag[0], w->tag[1], m->d_flags2, I.d_out_len, I.d_ex_off, W.d_st, st);
    }, status);
    // ---- the records with their tags, then their BGZF members (tag -s, or nothing kept: neither)
    rc = members_back(m, codec, w, W, X, dl, rc, status, bb, &w->ms[4], false, "record output kernel failed", [&](uint8_t *d_out) {
        launch_bam_emit(d_text, W.d_rec_start, I.d_rec_len, I.d_out_len, I.d_out_off, X.d_found_off, X.d_found_pat, m->d_pat_bytes, m->d_pat_off, I.d_ex_off, n,
                        w->tag[0], w->tag[1], d_out, st);
        return MK_OK;
    }, t);
    if (rc || *status) return rc;
    tag_commit(dl, X, c, counts);
    return MK_OK;
    MK_ABI_END
}

// ---- `tag` on a window of SAM text that stays on the device (an addition to ABI v7; kernels: sam.hip).  Lines can be cut by the host
// without reading them, so a caller's windows need no tail chain: the tail exists for callers that cut anywhere.
int mk_tag_sam_window(mk_matcher *m, mk_sam_window *w, int logging, mk_counters *c, uint32_t *counts, uint32_t *status) {
    static const char who[] = "mk_tag_sam_window";
    if (int bad = tag_args(who, m != nullptr, w, c, counts, status, logging)) return bad;
    if (w->n_text && !w->text) return fail(MK_E_INVALID_ARG, "mk_tag_sam_window: a size without its buffer");
    if (w->tag[0] == '\t' || w->tag[1] == '\t' || w->tag[0] == '\n' || w->tag[1] == '\n')
        return fail(MK_E_INVALID_ARG, "mk_tag_sam_window: a tag name holds a tab or a line end");
    MK_ABI_BEGIN
    TAG_WINDOW_BEGIN
    WindowSide W;
    SamIndex I;
    if ((rc = sam_index(m, w, who, 0, dl, W, I, status, t)) || *status || I.n == 0) return rc;
    const uint64_t n = I.n;
    const SamTables &R = I.R;
    const uint8_t *d_text = (const uint8_t *)W.T->d_text;
    TagWindow X = tag_window(w, who, n, I.d_out_len, I.d_ex_off, I.d_out_off, R.name_len);
    // ---- SEQ fields -> the scan buffer, scan, emission order, pattern sets
    if ((rc = tag_scan(m, dl, W, X, kSeqSam, logging))) return rc;
    w->ms[2] = (float)ms_since(t);
    // ---- keep, tag, emit
    rc = tag_keep(m, dl, W, X, logging, 4u, [&] {
        launch_sam_taglen(d_text, R, X.d_found_off, X.d_found_pat, m->d_pat_off, m->d_pat_bytes, n, w->filter_matching != 0, w->invert != 0, w->tag[0], w->tag[1],
                          m->d_flags2, I.d_out_len, I.d_ex_off, W.d_st, st);
    }, status);
    rc = text_back(m, w, X, dl, rc, status, &w->ms[3], "line output kernel failed", [&](uint8_t *d_out) {
        launch_sam_emit(d_text, R, I.d_out_len, I.d_out_off, X.d_found_off, X.d_found_pat, m->d_pat_bytes, m->d_pat_off, I.d_ex_off, n, w->tag[0], w->tag[1], d_out, st);
    }, t);
    if (rc || *status) return rc;
    tag_commit(dl, X, c, counts);
    return MK_OK;
    MK_ABI_END
}

// ---- `tag` SAM text -> BAM with the records encoded on the device (an addition to ABI v7; kernels: the second half of sam.hip): the
// line input and the members output; between them a kept line becomes a BAM record.
int mk_tag_sam_bam_window(mk_matcher *m, mk_codec *codec, mk_sam_bam_window *w, int logging, mk_counters *c, uint32_t *counts, uint32_t *status) {
    static const char who[] = "mk_tag_sam_bam_window";
    if (int bad = tag_args(who, m && codec, w, c, counts, status, logging)) return bad;
    if ((w->n_text && !w->text) || (w->n_refs && (!w->ref_names || !w->ref_off)))
        return fail(MK_E_INVALID_ARG, "mk_tag_sam_bam_window: a size without its buffer");
    if (w->tag[0] == '\t' || w->tag[1] == '\t' || w->tag[0] == '\n' || w->tag[1] == '\n')
        return fail(MK_E_INVALID_ARG, "mk_tag_sam_bam_window: a tag name holds a tab or a line end");
    const uint32_t bb = w->block_bytes ? w->block_bytes : mkz::kMaxBlockBytes;
    if (bb > mkz::kMaxBlockBytes) return fail(MK_E_INVALID_ARG, "mk_tag_sam_bam_window: block_bytes %u > %u", bb, mkz::kMaxBlockBytes);
    if (codec->device != m->device) return fail(MK_E_INVALID_ARG, "mk_tag_sam_bam_window: the codec and the matcher are on different devices");
    w->out_text_bytes = 0;
    MK_ABI_BEGIN
    TAG_WINDOW_BEGIN
    WindowSide W;
    SamIndex I;
    if ((rc = sam_index(m, w, who, 1, dl, W, I, status, t)) || *status || I.n == 0) return rc;
    const uint64_t n = I.n;
    const SamTables &R = I.R;
    const uint8_t *d_text = (const uint8_t *)W.T->d_text;
    uint32_t *d_n_cig = I.d_extra;
    TagWindow X = tag_window(w, who, n, I.d_out_len, I.d_ex_off, I.d_out_off, R.name_len);
    // ---- SEQ fields -> the scan buffer, scan, emission order, pattern sets
    if ((rc = tag_scan(m, dl, W, X, kSeqSam, logging))) return rc;
    w->ms[2] = (float)ms_since(t);
    // ---- keep, the tag's value, the size of every kept line as a BAM record
    rc = tag_keep(m, dl, W, X, logging, 7u, [&] {
        launch_sam_taglen(d_text, R, X.d_found_off, X.d_found_pat, m->d_pat_off, m->d_pat_bytes, n, w->filter_matching != 0, w->invert != 0, w->tag[0], w->tag[1],
                          m->d_flags2, I.d_out_len, I.d_ex_off, W.d_st, st);
        launch_sam_bam_len(d_text, R, m->d_flags2, n, I.d_out_len, d_n_cig, W.d_st, st);
    }, status);
    // ---- the records (the reference names go up with the first window that writes any), then their BGZF members
    rc = members_back(m, codec, w, W, X, dl, rc, status, bb, &w->ms[3], true, "record output kernels failed", [&](uint8_t *d_out) {
        SamRefsDevice F;
        if (int rc_refs = upload_refs(m, who, true, w->ref_names, w->ref_off, w->n_refs, st, F)) return rc_refs;
        launch_sam_bam_encode(d_text, R, m->d_flags2, I.d_out_len, I.d_out_off, d_n_cig, X.d_found_off, X.d_found_pat, m->d_pat_bytes, m->d_pat_off, I.d_ex_off, F.bytes,
                              F.off, F.table, F.mask, n, w->tag[0], w->tag[1], d_out, st);
        return MK_OK;
    }, t);
    if (rc || *status) return rc;
    tag_commit(dl, X, c, counts);
    return MK_OK;
    MK_ABI_END
}

// ---- `tag` BAM -> SAM text with the lines formatted on the device (an addition to ABI v7; kernels: the BAM -> SAM part of bam.hip): the
// member input and the text output; between them a kept record becomes its SAM line.
int mk_tag_bam_sam_window(mk_matcher *m, mk_codec *codec, mk_bam_sam_window *w, int logging, mk_counters *c, uint32_t *counts, uint32_t *status) {
    static const char who[] = "mk_tag_bam_sam_window";
    if (int bad = tag_args(who, m && codec, w, c, counts, status, logging)) return bad;
    if ((w->n_members && (!w->bgzf || !w->members)) || (w->n_refs && (!w->ref_names || !w->ref_off)))
        return fail(MK_E_INVALID_ARG, "mk_tag_bam_sam_window: a size without its buffer");
    MK_ABI_BEGIN
    TAG_WINDOW_BEGIN
    WindowSide W;
    BamIndex I;
    if ((rc = bam_front(m, codec, w, who, 1, dl, W, I, status, t)) || *status || I.n == 0) return rc;
    const uint64_t n = I.n;
    const uint8_t *d_text = (const uint8_t *)W.T->d_text;
    uint32_t *d_seq_at = I.d_extra;  // where SEQ starts in a kept record's line
    TagWindow X = tag_window(w, who, n, I.d_out_len, I.d_ex_off, I.d_out_off, nullptr);
    // ---- sequences -> the scan buffer, scan, emission order, pattern sets
    if ((rc = tag_scan(m, dl, W, X, kSeqBam, logging))) return rc;
    w->ms[3] = (float)ms_since(t);
    // ---- keep, the tag's value, the length of every kept record's line
    SamRefsDevice F;
    if ((rc = upload_refs(m, who, false, w->ref_names, w->ref_off, w->n_refs, st, F))) return rc;
    rc = tag_keep(m, dl, W, X, logging, 6u, [&] {
        launch_bam_taglen(d_text, W.d_rec_start, I.d_rec_len, W.d_seq_start, W.d_seq_len, X.d_found_off, X.d_found_pat, m->d_pat_off, m->d_pat_bytes, n,
                          w->filter_matching != 0, w->invert != 0, w->tag[0], w->tag[1], m->d_flags2, I.d_out_len, I.d_ex_off, W.d_st, st);
        launch_bam_sam_len(d_text, W.d_rec_start, I.d_rec_len, m->d_flags2, n, F.bytes, F.off, (uint32_t)w->n_refs, I.d_out_len, d_seq_at, W.d_st, st);
    }, status);
    rc = text_back(m, w, X, dl, rc, status, &w->ms[4], "line output kernels failed", [&](uint8_t *d_out) {
        launch_bam_sam_emit(d_text, W.d_rec_start, I.d_rec_len, W.d_seq_start, W.d_seq_len, I.d_out_len, I.d_out_off, d_seq_at, X.d_found_off, X.d_found_pat,
                            m->d_pat_bytes, m->d_pat_off, I.d_ex_off, F.bytes, F.off, (uint32_t)w->n_refs, n, w->tag[0], w->tag[1], d_out, st);
    }, t);
    if (rc || *status) return rc;
    tag_commit(dl, X, c, counts);
    return MK_OK;
    MK_ABI_END
}

}  // extern "C"
