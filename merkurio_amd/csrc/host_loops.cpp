// host_loops.cpp -- what the reference's record loops do with the matcher's answers, restated
// for batches so that keep/drop decisions, log rows and counters are bit-identical:
//   extract single   src/cmd_extract.rs:321-406
//   extract paired   src/cmd_extract.rs:463-612
//   tag              src/cmd_tag.rs:387-490
// The matching itself is the gfx950 scan kernel; nothing here searches text.  extract (single) and tag work on the
// device from end to end: scan -> tuples ordered on the device (order_hits.hip) -> log rows, per-pattern counts and
// the per-record pattern sets by the kernels of sets.hip -> results copied back.  The host threads only turn flags
// into keep decisions.  The paired loop orders both mates' tuples as one list, the mate inside a key field.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "matcher_internal.h"
#include "sam_numbers.hpp"
#include "codec/codec_internal.h"
#include "codec/codec_kernels.h"

using namespace mk;

namespace {

// scan one batch, growing the hit buffer on MK_E_CAPACITY
int scan_all(mk_matcher *m, const uint8_t *seq, const uint64_t *off, uint64_t n_rec, uint32_t mode,
             std::vector<uint8_t> &flags, std::vector<mk_hit> &hits) {
    flags.assign(n_rec ? n_rec : 1, 0);
    uint64_t n = 0;
    if (mode == MK_MODE_ANY) return mk_scan_batch(m, seq, off, n_rec, mode, flags.data(), nullptr, 0, &n);
    hits.resize(std::max<uint64_t>(4096, n_rec / 8));
    int rc = mk_scan_batch(m, seq, off, n_rec, mode, flags.data(), hits.data(), hits.size(), &n);
    if (rc == MK_E_CAPACITY) {
        hits.resize(n);
        rc = mk_scan_batch(m, seq, off, n_rec, mode, flags.data(), hits.data(), hits.size(), &n);
    }
    if (rc) return rc;
    hits.resize(n);
    return MK_OK;
}

struct RowSink {
    mk_row *rows;
    uint64_t cap;
    uint64_t n = 0;
    void push(uint32_t file, const mk_hit &h) {
        if (rows && n < cap) {
            rows[n].rec = h.rec;
            rows[n].pat = h.pat;
            rows[n].pos = h.pos;
            rows[n].file = file;
            rows[n]._pad = 0;
        }
        ++n;
    }
};

// pattern_hit_counts for one file's ordered hits.
// AC: += 1 per hit (src/cmd_extract.rs:353).  BNDMq: += 1 per (record, pattern) that has at
// least one hit (src/cmd_extract.rs:380-383): hits are pattern-major inside a record, so a
// new (rec, pat) run starts whenever either changes.
void count_patterns(uint32_t algo, const std::vector<mk_hit> &hits, uint32_t *counts) {
    if (algo == MK_ALGO_AC) {
        for (auto &h : hits) counts[h.pat] += 1;
    } else {
        for (size_t i = 0; i < hits.size(); ++i)
            if (i == 0 || hits[i].rec != hits[i - 1].rec || hits[i].pat != hits[i - 1].pat) counts[hits[i].pat] += 1;
    }
}

uint64_t popcount_flags(const std::vector<uint8_t> &f, uint64_t n) {
    uint64_t c = 0;
    for (uint64_t i = 0; i < n; ++i) c += f[i] != 0;
    return c;
}

// One driver-loop call on the device: upload, scan, then whatever the loop derives from the tuples, each step
// enqueued on the handle's stream; the time of the call is split into upload / device / download / host.
struct DeviceLoop {
    mk_matcher *m;
    hipStream_t st;
    unsigned long long found = 0;  // tuples of the scan (all of them are on the device)
    uint64_t n_bytes = 0;
    using clk = std::chrono::steady_clock;
    clk::time_point t_last;
    int phase = 0;
    explicit DeviceLoop(mk_matcher *m_) : m(m_), st(m_->stream), t_last(clk::now()) {
        for (float &x : m->batch_ms) x = 0;
    }
    void mark(int next) {  // the stream is idle at every call: time since the last mark goes to the current phase
        const auto t = clk::now();
        m->batch_ms[phase] += std::chrono::duration<float, std::milli>(t - t_last).count();
        t_last = t;
        phase = next;
    }
    void host_begin() { mark(3); }
    void finish() { mark(3); }

    int scan(const uint8_t *seq, const uint64_t *off, uint64_t n_rec, uint32_t mode, uint8_t *flags, uint64_t *flagged) {
        int rc = batch_check(seq, off, n_rec, &n_bytes);
        if (rc) return rc;
        uint32_t batch_len = 0;
        phase = 0;
        if ((rc = batch_upload(m, seq, off, n_rec, n_bytes, &batch_len))) return rc;
        if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "upload failed");
        mark(1);
        return scan_flags(n_rec, mode, batch_len, flags, flagged);
    }
    // the batch is already in m->d_seq / m->d_off (ingest.hip put it there; batch_len > 0: every record has that length): scan + flags
    int scan_resident(uint64_t n_seq_bytes, uint64_t n_rec, uint32_t mode, uint32_t batch_len, uint8_t *flags, uint64_t *flagged) {
        n_bytes = n_seq_bytes;
        m->ragged = !batch_len;
        *flagged = 0;
        if (n_bytes == 0) {  // every sequence is empty: nothing can match
            std::fill(flags, flags + n_rec, 0);
            found = 0;
            if (n_rec && hipMemsetAsync(m->d_flags, 0, n_rec, st) != hipSuccess) return fail(MK_E_HIP, "hipMemsetAsync failed");
            return MK_OK;
        }
        return scan_flags(n_rec, mode, batch_len, flags, flagged);
    }
    // the scan of the batch on the device and its flags -> host.  All tuples stay on the device: no caller-side limit.  The scan starts
    // with the room the handle already has (hit-dense batches -- tag / extract -l on already extracted reads -- overflowed n_rec / 8 on
    // EVERY batch and ran their scan twice; after the first such batch one scan suffices)
    int scan_flags(uint64_t n_rec, uint32_t mode, uint32_t batch_len, uint8_t *flags, uint64_t *flagged) {
        const uint64_t cap0 = std::max<uint64_t>(std::max<uint64_t>(4096, n_rec / 8), m->d_hits_cap / sizeof(mk_hit));
        int rc = batch_scan(m, n_bytes, n_rec, mode, batch_len, cap0, ~0ull, &found);
        if (rc) return rc;
        mark(2);
        if ((rc = batch_flags(m, n_rec, flags, flagged))) return rc;
        mark(1);
        return MK_OK;
    }
    // rec_bound: the records the tuples come from (the bins of the ordering)
    int order(bool ac_order, uint64_t rec_bound) { return order_hits_on_device(m, m->d_hits, found, ac_order, rec_bound, st); }

    // mk_row per tuple (in their current order) -> rows[0, min(found, cap)); pair: the marked pair list (sets.hip), rows with their mate
    int rows_to_host(mk_row *rows, uint64_t cap, bool pair = false) {
        const uint64_t n = std::min<uint64_t>(found, rows ? cap : 0);
        if (!n) return MK_OK;
        int rc = ensure_device(&m->d_aux, &m->d_aux_cap, n * sizeof(mk_row));
        if (rc) return rc;
        if (pair) launch_rows_pair(m->d_hits, n, m->algo == MK_ALGO_AC, (mk_row *)m->d_aux, st);
        else launch_rows(m->d_hits, n, 0, (mk_row *)m->d_aux, st);
        if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "row kernel failed");
        mark(2);
        if (hipMemcpy(rows, m->d_aux, n * sizeof(mk_row), hipMemcpyDeviceToHost) != hipSuccess) return fail(MK_E_HIP, "copy of the log rows failed");
        mark(1);
        return MK_OK;
    }

    // counts[i] += the n_pat counts at d_counts (u32; wide: u64, of which the low words count); the copy is charged to the download,
    // the sums to the host.  d_counts == nullptr: nothing to add.
    int add_counts(const void *d_counts, bool wide, uint32_t *counts) {
        const uint32_t n_pat = m->n_pat, stride = wide ? 2 : 1;
        std::vector<uint32_t> v(d_counts ? (size_t)n_pat * stride : 0);
        if (!v.empty() && hipMemcpy(v.data(), d_counts, v.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(MK_E_HIP, "copy of the counts failed");
        mark(3);
        for (size_t i = 0; i < v.size(); i += stride) counts[i / stride] += v[i];
        mark(1);
        return MK_OK;
    }

    // counters of one file's scan of n_rec records (single :326-387, tag :443-451), its tuples in emission order (AC / BNDMq)
    // and their log rows
    int log_single(mk_counters *c, uint64_t n_rec, uint64_t n_bases, uint64_t flagged, mk_row *rows, uint64_t rows_cap) {
        c->nb_records_tot += n_rec;
        c->nb_bases += n_bases;
        c->nb_hits_tot[0] += found;
        c->nb_records_hit[0] += flagged;
        int rc = order(m->algo == MK_ALGO_AC, n_rec);
        if (rc) return rc;
        return rows_to_host(rows, rows_cap);
    }

    // paired extract, after mate 1's scan: its tuples wait in their own buffer while mate 2 is scanned
    int stash_mate1() {
        if (!found) return MK_OK;
        int rc = ensure_device(&m->d_pair, &m->d_pair_cap, found * sizeof(mk_hit));
        if (rc) return rc;
        if (hipMemcpyAsync(m->d_pair, m->d_hits, found * sizeof(mk_hit), hipMemcpyDeviceToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail(MK_E_HIP, "copy of the first mate's tuples failed");
        return MK_OK;
    }

    // paired extract, after mate 2's scan of n_rec records (stash_mate1 kept mate 1's n1 tuples): one list -- mate 2's tuples (already
    // in the scan buffer), then mate 1's, the mate marked inside a key field -- in pair order, its log rows and pattern_hit_counts:
    // AC one per hit of either mate (:492,:520); BNDMq one per pair, pattern and mate with a hit (:575-584)
    int join_mates(unsigned long long n1, uint64_t n_rec, mk_row *rows, uint64_t rows_cap, uint32_t *counts) {
        const bool ac = m->algo == MK_ALGO_AC;
        const unsigned long long n2 = found;
        if (n1 + n2 == 0) return MK_OK;
        int rc;
        if ((n1 + n2) * sizeof(mk_hit) > m->d_hits_cap) {  // grow the scan buffer, keeping mate 2's tuples
            void *bigger = nullptr;
            size_t cap = 0;
            if ((rc = ensure_device(&bigger, &cap, (n1 + n2) * sizeof(mk_hit)))) return rc;
            if (n2 && hipMemcpy(bigger, m->d_hits, n2 * sizeof(mk_hit), hipMemcpyDeviceToDevice) != hipSuccess) {
                (void)hipFree(bigger);
                return fail(MK_E_HIP, "copy of the second mate's tuples failed");
            }
            if (m->d_hits) (void)hipFree(m->d_hits);
            m->d_hits = (mk_hit *)bigger;
            m->d_hits_cap = cap;
        }
        if (n1 && hipMemcpyAsync(m->d_hits + n2, m->d_pair, n1 * sizeof(mk_hit), hipMemcpyDeviceToDevice, st) != hipSuccess)
            return fail(MK_E_HIP, "copy of the first mate's tuples failed");
        launch_pair_mark(m->d_hits, n2, 1, ac, st);
        launch_pair_mark(m->d_hits + n2, n1, 0, ac, st);
        found = n1 + n2;
        if ((rc = order(ac, ac ? 2 * n_rec : n_rec))) return rc;  // (AC: record' = 2 * record + mate)
        if ((rc = rows_to_host(rows, rows_cap, true))) return rc;
        if (ac) {
            unsigned long long n = found;  // the histogram kernel reads the tuple count from the device
            if (hipMemcpyAsync(m->d_nhits, &n, sizeof(n), hipMemcpyHostToDevice, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
                return fail(MK_E_HIP, "copy failed");
            return pattern_counts(true, 0, counts);
        }
        if ((rc = ensure_device(&m->d_aux, &m->d_aux_cap, (size_t)m->n_pat * 4))) return rc;
        if (hipMemsetAsync(m->d_aux, 0, (size_t)m->n_pat * 4, st) != hipSuccess) return fail(MK_E_HIP, "memset failed");
        launch_count_pair_heads(m->d_hits, found, (uint32_t *)m->d_aux, m->n_pat, st);
        if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "count kernel failed");
        mark(2);
        return add_counts(m->d_aux, false, counts);
    }

    // pattern_hit_counts += this batch's: per hit (AC, src/cmd_extract.rs:353) or per (record, pattern) with a hit
    // (BNDMq, :380-383; the tuples must be in BNDMq order = set order)
    int pattern_counts(bool per_hit, uint64_t n_rec, uint32_t *counts) {
        if (!found) return MK_OK;
        const uint32_t n_pat = m->n_pat;
        if (per_hit) {
            int rc = ensure_device(&m->d_aux, &m->d_aux_cap, ((size_t)n_pat + MK_NUM_SUMMARY) * 8);
            if (rc) return rc;
            if (hipMemsetAsync(m->d_aux, 0, ((size_t)n_pat + MK_NUM_SUMMARY) * 8, st) != hipSuccess) return fail(MK_E_HIP, "memset failed");
            ScanParams p;
            memset(&p, 0, sizeof(p));
            p.hits = m->d_hits;
            p.n_hits = m->d_nhits;  // still holds `found`
            p.hits_cap = found;
            p.counters = (unsigned long long *)m->d_aux;
            p.n_pat = n_pat;
            launch_hist_hits(p, m->num_cus, st);
            if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "histogram kernel failed");
            mark(2);
            return add_counts(m->d_aux, true, counts);
        }
        // BNDMq: the heads of the (record, pattern) runs = the entries of the pattern sets
        uint64_t n_found = 0;
        return pattern_sets(n_rec, nullptr, nullptr, 0, &n_found, counts);
    }

    // the distinct patterns of every record (tuples in set order) as a CSR in the handle's scratch (m->d_aux): *d_off_out[n_rec + 1],
    // *d_pat_out[*n_found]; want_counts: *d_cnt_out[n_pat] = entries per pattern (BNDMq's pattern_hit_counts).  The stream is idle on return.
    int pattern_sets_device(uint64_t n_rec, bool want_counts, unsigned long long **d_off_out, uint32_t **d_pat_out, uint32_t **d_cnt_out, uint64_t *n_found) {
        const uint32_t n_pat = m->n_pat;
        // (the set kernels rank run heads and sum tiles in 32 bits, sets.hip)
        if (found >= (1ull << 32)) return fail(MK_E_UNSUPPORTED, "%llu occurrences in one batch: the per-record pattern sets take at most 2^32 - 1", found);
        const size_t off_bytes = (n_rec + 1) * 8, pat_bytes = ((size_t)found * 4 + 15) & ~(size_t)15;
        const size_t tiles = std::max<size_t>((found + 4095) / 4096, (n_rec + 1 + 4095) / 4096) + 1;
        const size_t cnt_bytes = ((size_t)n_pat * 4 + 15) & ~(size_t)15;
        int rc = ensure_device(&m->d_aux, &m->d_aux_cap, off_bytes + pat_bytes + tiles * 8 + 16 + cnt_bytes);
        if (rc) return rc;
        char *base = (char *)m->d_aux;
        unsigned long long *d_off = (unsigned long long *)base;
        uint32_t *d_pat = (uint32_t *)(base + off_bytes);
        void *d_tile = base + off_bytes + pat_bytes;
        unsigned long long *d_total = (unsigned long long *)(base + off_bytes + pat_bytes + tiles * 8);
        uint32_t *d_cnt = (uint32_t *)(base + off_bytes + pat_bytes + tiles * 8 + 16);
        launch_pattern_sets(m->d_hits, found, n_rec, d_pat, d_off, d_total, d_tile, st);
        unsigned long long total = 0;
        if (hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, st) != hipSuccess) return fail(MK_E_HIP, "copy failed");
        if (want_counts) {
            if (hipMemsetAsync(d_cnt, 0, cnt_bytes, st) != hipSuccess) return fail(MK_E_HIP, "memset failed");
        }
        if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "pattern-set kernels failed");
        *n_found = total;
        if (want_counts && total) {
            launch_count_u32(d_pat, total, d_cnt, n_pat, st);
            if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "count kernel failed");
        }
        *d_off_out = d_off, *d_pat_out = d_pat, *d_cnt_out = d_cnt;
        return MK_OK;
    }

    // the same, copied to the host.  found_off == nullptr: only the counts.
    int pattern_sets(uint64_t n_rec, uint64_t *found_off, uint32_t *found_pat, uint64_t found_cap, uint64_t *n_found, uint32_t *counts) {
        const size_t off_bytes = (n_rec + 1) * 8;
        unsigned long long *d_off = nullptr;
        uint32_t *d_pat = nullptr, *d_cnt = nullptr;
        int rc = pattern_sets_device(n_rec, counts != nullptr, &d_off, &d_pat, &d_cnt, n_found);
        if (rc) return rc;
        const uint64_t total = *n_found;
        mark(2);
        if (found_off && hipMemcpy(found_off, d_off, off_bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(MK_E_HIP, "copy of the set offsets failed");
        const uint64_t n_copy = std::min<uint64_t>(total, found_pat ? found_cap : 0);
        if (n_copy && hipMemcpy(found_pat, d_pat, n_copy * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(MK_E_HIP, "copy of the sets failed");
        return add_counts(counts && total ? d_cnt : nullptr, false, counts);
    }
};

// keep flags of the extract loop (single :400-405, paired :600-606; f2 == nullptr: single): a record -- a pair -- is kept when it has
// a hit, or under -v when it has none, and counts once per record, twice per pair
void extract_keep(const uint8_t *f1, const uint8_t *f2, uint64_t n, int invert, uint8_t *keep, mk_counters *c) {
    for (uint64_t r = 0; r < n; ++r) {
        const bool hit = f1[r] || (f2 && f2[r]);
        keep[r] = (uint8_t)(hit != (invert != 0));
        c->nb_records_extracted += (f2 ? 2u : 1u) * keep[r];
    }
}

int check_rows_cap(int logging, const mk_row *rows, uint64_t rows_cap, uint64_t need) {
    if (logging && rows && need > rows_cap) return fail(MK_E_CAPACITY, "rows buffer too small: need %llu", (unsigned long long)need);
    return MK_OK;
}

}  // namespace

extern "C" {

int mk_extract_single(mk_matcher *m, const uint8_t *seq, const uint64_t *off, uint64_t n_rec, int logging,
                      int invert, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows,
                      mk_counters *c, uint32_t *counts) {
    if (!m || !keep || !c || (logging && !counts)) return fail(MK_E_INVALID_ARG, "null argument");
    if (n_rows) *n_rows = 0;
    if (n_rec == 0) return MK_OK;
    MK_ABI_BEGIN
    DeviceLoop dl(m);
    std::vector<uint8_t> flags(n_rec);
    uint64_t flagged = 0;
    int rc = dl.scan(seq, off, n_rec, logging ? MK_MODE_HITS : MK_MODE_ANY, flags.data(), &flagged);
    if (rc) return rc;
    if (logging) {
        // rows in emission order (:338-351 / :369-377) and pattern_hit_counts: AC one per hit (:353), BNDMq one per
        // record and pattern (:380-383) -- BNDMq's emission order is the set order, so its heads are counted in place
        if ((rc = dl.log_single(c, n_rec, off[n_rec] - off[0], flagged, rows, rows_cap))) return rc;
        if ((rc = dl.pattern_counts(m->algo == MK_ALGO_AC, n_rec, counts))) return rc;
    }
    dl.host_begin();
    extract_keep(flags.data(), nullptr, n_rec, invert, keep, c);
    dl.finish();
    if (n_rows) *n_rows = dl.found;
    return check_rows_cap(logging, rows, rows_cap, dl.found);
    MK_ABI_END
}

// ---- text windows in, records out (r05: FASTA, paired inputs, heads): the raw bytes of a window of every
// input file go to the device as they are (plain text is uploaded, BGZF members are inflated there), are indexed and gathered on
// the device (ingest.hip), then the extract loop runs as in mk_extract_single / mk_extract_paired
}  // extern "C"

namespace {

// One input of a window on the device: its text in slot T (m->txt[k]) and what the index kernels made of it
struct WindowSide {
    mk_matcher::TextSlot *T = nullptr;
    uint64_t n_window = 0;  // bytes of text (head + body)
    uint8_t last_byte = '\n';
    uint32_t total_nl = 0;
    uint64_t n_avail = 0;   // whole records found
    uint64_t n_used = 0;    // bytes of the first n records (n = what the call processes)
    uint32_t fixed = 0;     // > 0: every sequence has this length (FASTQ)
    uint64_t seq_total = 0; // FASTA: sequence bytes of all records
    uint32_t *d_block = nullptr, *d_total = nullptr, *d_st = nullptr, *d_line = nullptr, *d_rec_start = nullptr, *d_seq_start = nullptr,
             *d_seq_len = nullptr;
    unsigned long long *d_tile = nullptr, *d_block64 = nullptr, *d_fa_off = nullptr;  // d_fa_off: FASTA's sequence offsets
};

constexpr uint32_t kBigRecord = 1u << 20;  // records from here on are copied one by one when the kept records are packed

// text of a source -> T->d_text[0, n_window): head, then the body (uploaded, taken from an upload-ahead slot, or inflated from
// BGZF members).  Enqueued on st; the caller synchronises.  *corrupt_member: index of a damaged member (MK_E_CORRUPT).
int window_assemble(mk_matcher *m, mk_codec *codec, mk_window_source &S, WindowSide &W, DeviceLoop &dl) {
    hipStream_t st = dl.st;
    int rc;
    uint64_t body = S.n_text;
    for (uint64_t i = 0; i < S.n_members; ++i) {
        const mk_bgzf_member &b = S.members[i];
        if (b.data_off > S.n_bgzf || b.data_len > S.n_bgzf - b.data_off || b.isize > 65536 || b.out_off != body - S.n_text)
            return fail(MK_E_INVALID_ARG, "mk_extract_window: member %llu lies outside its buffer or its text is not in sequence", (unsigned long long)i);
        body += b.isize;
    }
    if ((S.n_text != 0) + (S.n_members != 0) + (S.n_device_text != 0) > 1)
        return fail(MK_E_INVALID_ARG, "mk_extract_window: a source's body is plain text, BGZF members or device text -- one of them");
    body += S.n_device_text;
    W.n_window = S.n_head + body;
    S.n_window = W.n_window;
    if (W.n_window == 0) return MK_OK;
    if (W.n_window >= 0xFFFFFFF0ull) return fail(MK_E_UNSUPPORTED, "a text window must be shorter than 4 GiB (%llu bytes)", (unsigned long long)W.n_window);
    mk_matcher::TextSlot &T = *W.T;
    // a body that mk_upload_text_ahead has already sent (same pointer, same size): without a head its buffer BECOMES the text
    // buffer, with one it is copied behind the head on the device
    bool ahead = false;
    if (S.n_text) {
        std::lock_guard<std::mutex> lk(m->ahead_mu);
        for (auto &a : m->ahead) {
            if (!a.text || a.text != S.text || ahead) continue;
            if (a.n != S.n_text) {  // (another window out of the same buffer: stale)
                if (hipEventSynchronize(a.ev) != hipSuccess) return fail(MK_E_HIP, "hipEventSynchronize failed");
                a.text = nullptr;
                continue;
            }
            if (hipStreamWaitEvent(st, a.ev, 0) != hipSuccess) return fail(MK_E_HIP, "hipStreamWaitEvent failed");
            if (S.n_head == 0) {
                std::swap(T.d_text, a.d);
                std::swap(T.d_text_cap, a.cap);
            } else {
                if ((rc = ensure_device(&T.d_text, &T.d_text_cap, W.n_window + 64))) return rc;
                if (hipMemcpyAsync((uint8_t *)T.d_text + S.n_head, a.d, S.n_text, hipMemcpyDeviceToDevice, st) != hipSuccess)
                    return fail(MK_E_HIP, "copy of the uploaded window failed");
                // (the slot may be refilled by the uploader as soon as it is marked free: let the copy out of it finish first)
                if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "copy of the uploaded window failed");
            }
            a.text = nullptr;
            ahead = true;
        }
    }
    if (!ahead && (rc = ensure_device(&T.d_text, &T.d_text_cap, W.n_window + 64))) return rc;
    if (S.n_head && hipMemcpyAsync(T.d_text, S.head, S.n_head, hipMemcpyHostToDevice, st) != hipSuccess) return fail(MK_E_HIP, "upload of the head failed");
    if (S.n_text && !ahead && hipMemcpyAsync((uint8_t *)T.d_text + S.n_head, S.text, S.n_text, hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(MK_E_HIP, "upload of the text failed");
    if (S.n_device_text && hipMemcpyAsync((uint8_t *)T.d_text + S.n_head, S.device_text, S.n_device_text, hipMemcpyDefault, st) != hipSuccess)
        return fail(MK_E_HIP, "copy of the device text failed");
    if (S.n_members) {
        if (!codec) return fail(MK_E_INVALID_ARG, "mk_extract_window: BGZF members need a codec handle");
        if (codec->device != m->device) return fail(MK_E_INVALID_ARG, "mk_extract_window: the codec and the matcher are on different devices");
        // the members' bytes and their table go up (a fifth of the text), the text is inflated behind the head in place
        std::lock_guard<std::mutex> lock(codec->mu);
        uint64_t in_lo = S.members[0].data_off, in_hi = in_lo;
        std::vector<mkz::Member> part(S.n_members);
        for (uint64_t i = 0; i < S.n_members; ++i) {
            in_lo = std::min<uint64_t>(in_lo, S.members[i].data_off);
            in_hi = std::max<uint64_t>(in_hi, S.members[i].data_off + S.members[i].data_len);
        }
        for (uint64_t i = 0; i < S.n_members; ++i)
            part[i] = mkz::Member{S.members[i].data_off - in_lo, S.n_head + S.members[i].out_off, S.members[i].data_len, S.members[i].isize, S.members[i].crc, 0};
        const uint64_t cn = in_hi - in_lo;
        if ((rc = ensure_device(&codec->d_in, &codec->in_cap, cn + mkz::kPad)) ||
            (rc = ensure_device(&codec->d_aux, &codec->aux_cap, (S.n_members + 1) * sizeof(mkz::Member))) ||
            (rc = ensure_device(&codec->d_len, &codec->len_cap, (S.n_members + 1) * 4ull)))
            return rc;
        if (hipMemcpyAsync(codec->d_in, S.bgzf + in_lo, cn, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemsetAsync((uint8_t *)codec->d_in + cn, 0, mkz::kPad, st) != hipSuccess ||
            hipMemcpyAsync(codec->d_aux, part.data(), S.n_members * sizeof(mkz::Member), hipMemcpyHostToDevice, st) != hipSuccess)
            return fail(MK_E_HIP, "upload of the members failed");
        if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "upload of the members failed");
        dl.mark(1);
        mkz::launch_inflate((const uint8_t *)codec->d_in, cn, (const mkz::Member *)codec->d_aux, (uint32_t)S.n_members, (uint8_t *)T.d_text,
                            (int32_t *)codec->d_len, codec->num_cus, st, codec->inflate_kernel);
        mkz::launch_crc_check((const uint8_t *)T.d_text, (const mkz::Member *)codec->d_aux, (uint32_t)S.n_members, (int32_t *)codec->d_len, st);
        std::vector<int32_t> st_words(S.n_members);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(st_words.data(), codec->d_len, S.n_members * 4ull, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail(MK_E_HIP, "BGZF inflate failed");
        dl.mark(2);
        for (uint64_t i = 0; i < S.n_members; ++i)
            if (st_words[i])
                return fail(MK_E_CORRUPT, st_words[i] > 0 ? "BGZF member %llu: CRC-32 of the inflated text differs from the trailer's (status %d)"
                                                           : "BGZF member %llu does not inflate to its ISIZE (decoder status %d)",
                            (unsigned long long)i, st_words[i]);
    }
    return MK_OK;
}

// line table, whole records and their tables for the text in W.T (enqueued work waited for): W.n_avail, d_rec_start[n_avail + 1],
// FASTQ: d_seq_start / d_seq_len / W.fixed; FASTA: the sequences already lie in d_seq_out with offsets d_fa_off[n_avail + 1].
// *status = 1: this text is not what the device takes (the caller's reader decides what it is).
int window_index(mk_matcher *m, uint32_t format, bool ends_at_record, WindowSide &W, uint8_t *d_seq_out, hipStream_t st, uint32_t *status) {
    mk_matcher::TextSlot &T = *W.T;
    int rc;
    const uint64_t n_text = W.n_window;
    const uint8_t *d_text = (const uint8_t *)T.d_text;
    const uint32_t n_blocks = (uint32_t)((n_text + ingest_block_bytes() - 1) / ingest_block_bytes());
    // d_ing_a: newline count per block | total | status, min, max | (FASTA) u64 per block + 1
    const size_t a_words = (size_t)n_blocks + 8;
    if ((rc = ensure_device(&T.d_ing_a, &T.d_ing_a_cap, a_words * 4 + 16 + ((size_t)n_blocks + 2) * 8))) return rc;
    W.d_block = (uint32_t *)T.d_ing_a;
    W.d_total = W.d_block + n_blocks;
    W.d_st = W.d_total + 1;
    W.d_block64 = (unsigned long long *)(((uintptr_t)(W.d_block + a_words) + 15) & ~(uintptr_t)15);
    launch_ingest_count(d_text, n_text, W.d_block, W.d_total, st);
    uint8_t first_last[2] = {0, 0};
    if (hipMemcpyAsync(&W.total_nl, W.d_total, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&first_last[0], d_text, 1, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&first_last[1], d_text + n_text - 1, 1, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "newline count failed");
    W.last_byte = first_last[1];
    const uint32_t total_nl = W.total_nl;
    if (format == MK_TEXT_FASTA) {
        if (first_last[0] != '>') {  // blank lines or anything else in front of the first header: the host reader's business
            *status = 1;
            return MK_OK;
        }
        // line table | record starts | (u64) sequence offsets
        const size_t max_rec = (size_t)total_nl + 2;  // (a header per line at most)
        const size_t ws = ((size_t)total_nl + 4) * 4 + (max_rec + 2) * 4 + 16 + (max_rec + 2) * 8;
        if ((rc = ensure_device(&T.d_ing_b, &T.d_ing_b_cap, ws))) return rc;
        W.d_line = (uint32_t *)T.d_ing_b;
        W.d_rec_start = W.d_line + total_nl + 4;
        W.d_fa_off = (unsigned long long *)(((uintptr_t)(W.d_rec_start + max_rec + 2) + 15) & ~(uintptr_t)15);
        launch_ingest_lines(d_text, n_text, W.d_block, W.d_total, W.d_line, st);
        if (hipMemsetAsync(W.d_block64 + n_blocks, 0, 8, st) != hipSuccess) return fail(MK_E_HIP, "hipMemsetAsync failed");
        launch_ingest_fasta_count(d_text, n_text, W.d_block, W.d_line, W.d_block64, st);
        unsigned long long totals = 0;
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&totals, W.d_block64 + n_blocks, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail(MK_E_HIP, "FASTA indexing failed");
        const uint64_t heads = totals >> 32;
        W.seq_total = totals & 0xFFFFFFFFull;
        launch_ingest_fasta_emit(d_text, n_text, W.d_block, W.d_line, W.d_block64, d_seq_out, W.d_rec_start, W.d_fa_off, st);
        if (hipGetLastError() != hipSuccess) return fail(MK_E_HIP, "FASTA gather failed to launch");
        // a record is whole once the next header (or the end of the input) has been seen
        W.n_avail = ends_at_record ? heads : (heads ? heads - 1 : 0);
        W.fixed = 0;
        return MK_OK;
    }
    uint64_t n_lines = total_nl;
    if (ends_at_record) {
        n_lines += W.last_byte != '\n' ? 1 : 0;
        if (n_lines % 4 != 0) {  // not whole 4-line records: the caller's reader decides what this text is
            *status = 1;
            return MK_OK;
        }
    }
    const uint64_t n_rec = n_lines / 4;
    W.n_avail = n_rec;
    // workspace: line starts | record starts (+1) | sequence starts | sequence lengths | tile sums
    const size_t n_tiles = n_rec / ingest_scan_tile() + 2;
    const size_t ws = ((size_t)total_nl + 4 + 3 * (n_rec + 2) + 8) * 4 + n_tiles * 8 + 64;
    if ((rc = ensure_device(&T.d_ing_b, &T.d_ing_b_cap, ws))) return rc;
    W.d_line = (uint32_t *)T.d_ing_b;
    W.d_rec_start = W.d_line + total_nl + 4;
    W.d_seq_start = W.d_rec_start + n_rec + 2;
    W.d_seq_len = W.d_seq_start + n_rec + 2;
    W.d_tile = (unsigned long long *)(((uintptr_t)(W.d_seq_len + n_rec + 2) + 15) & ~(uintptr_t)15);
    const uint32_t st_init[3] = {0u, 0xFFFFFFFFu, 0u};
    if (hipMemcpyAsync(W.d_st, st_init, sizeof(st_init), hipMemcpyHostToDevice, st) != hipSuccess) return fail(MK_E_HIP, "copy failed");
    launch_ingest_records(d_text, n_text, W.d_block, W.d_total, W.d_line, n_rec, W.d_rec_start, W.d_seq_start, W.d_seq_len, W.d_st, st);
    uint32_t st_host[3] = {0, 0, 0};
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(st_host, W.d_st, sizeof(st_host), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "record indexing failed");
    if (st_host[0]) {  // some record is not '@' / sequence / '+' / quality of equal length
        *status = 1;
        return MK_OK;
    }
    W.fixed = (n_rec && st_host[1] == st_host[2] && st_host[1] > 0) ? st_host[1] : 0;
    return MK_OK;
}

// exclusive scan of d_len[0, n) -> d_off[0, n], its total d_off[n] -> *total (enqueued work waited for; `what`: the message of a failure)
int scan_offsets(const uint32_t *d_len, uint64_t n, unsigned long long *d_tile, unsigned long long *d_off, hipStream_t st, unsigned long long *total,
                 const char *what) {
    launch_ingest_offsets(d_len, n, d_tile, d_off, st);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(total, d_off + n, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "%s", what);
    return MK_OK;
}

// how a window's text holds its sequences: as they are (FASTQ), as BAM's 4-bit codes, as SAM's SEQ field (a-z upper-cased for the matcher)
enum SeqForm { kSeqPlain, kSeqBam, kSeqSam };

// the sequences of W's first n records -> the scan buffer, scanned: flags (host + m->d_flags), tuples in m->d_hits (dl.found), *n_seq
// sequence bytes.  FASTQ / BAM / SAM are gathered by W.d_seq_start / W.d_seq_len (W.fixed > 0: all of that length) in the way their
// form asks for; FASTA's were compacted by the index step.
int scan_sequences(mk_matcher *m, const WindowSide &W, uint64_t n, SeqForm form, DeviceLoop &dl, uint32_t mode, uint8_t *flags, uint64_t *flagged,
                   uint64_t *n_seq) {
    hipStream_t st = dl.st;
    const uint32_t fixed = W.fixed;
    unsigned long long total = (unsigned long long)n * fixed;
    int rc;
    if ((rc = ensure_device((void **)&m->d_flags, &m->d_flags_cap, n + 8)) || (rc = ensure_device((void **)&m->d_off, &m->d_off_cap, (n + 1) * sizeof(uint64_t))))
        return rc;
    if (W.d_fa_off) {  // FASTA: the offsets of the compacted sequences become the batch's
        if (hipMemcpyAsync(m->d_off, W.d_fa_off, (n + 1) * 8, hipMemcpyDeviceToDevice, st) != hipSuccess ||
            hipMemcpyAsync(&total, W.d_fa_off + n, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail(MK_E_HIP, "copy of the sequence offsets failed");
        *n_seq = total;
        // (one record of 4 GiB or more cannot be addressed by mk_hit.pos, as mk_scan_batch refuses it.)  The sequences lie in the
        // slot's own buffer: it stands in for the scan buffer for this scan.
        mk_matcher::TextSlot &T = *W.T;
        void *seq = m->d_seq;
        size_t cap = m->d_seq_cap;
        m->d_seq = (uint8_t *)T.d_fa_seq, m->d_seq_cap = T.d_fa_seq_cap;
        rc = dl.scan_resident(total, n, mode, 0, flags, flagged);
        T.d_fa_seq = m->d_seq, T.d_fa_seq_cap = m->d_seq_cap;
        m->d_seq = (uint8_t *)seq, m->d_seq_cap = cap;
        return rc;
    }
    if (!fixed && (rc = scan_offsets(W.d_seq_len, n, W.d_tile, (unsigned long long *)m->d_off, st, &total, "offset scan failed"))) return rc;
    *n_seq = total;
    if ((rc = ensure_device((void **)&m->d_seq, &m->d_seq_cap, total + 64))) return rc;
    if (form == kSeqBam) launch_bam_unpack((const uint8_t *)W.T->d_text, W.d_seq_start, W.d_seq_len, (const unsigned long long *)m->d_off, fixed, n, m->d_seq, st);
    else if (form == kSeqSam) launch_sam_gather((const uint8_t *)W.T->d_text, W.d_seq_start, W.d_seq_len, (const unsigned long long *)m->d_off, fixed, n, m->d_seq, st);
    else launch_ingest_gather((const uint8_t *)W.T->d_text, W.d_seq_start, W.d_seq_len, (const unsigned long long *)m->d_off, fixed, n, m->d_seq, st);
    if (hipGetLastError() != hipSuccess) return fail(MK_E_HIP, form == kSeqPlain ? "ingest kernels failed to launch" : "sequence unpacking failed to launch");
    return dl.scan_resident(total, n, mode, fixed, flags, flagged);
}

// text of the kept records of side W (keep flags in d_keep, already final: invert applied by the caller as 0), packed -> host
int window_kept(mk_matcher *m, uint32_t format, WindowSide &W, uint64_t n, const uint8_t *d_keep, const std::vector<uint32_t> &rs, const uint8_t *keep_host,
                mk_window_source &S, DeviceLoop &dl) {
    hipStream_t st = dl.st;
    S.n_kept_bytes = 0;
    if (!n) return MK_OK;
    int rc;
    // lengths by the flags, the offsets scan and the gather kernel of the sequences once more -- into the scan buffer, which has
    // done its work.  (FASTA has no per-record length table of its own: one is carved behind the record starts' u64 table.)
    uint32_t *d_len = W.d_seq_len;
    unsigned long long *d_tile = W.d_tile;
    if (format == MK_TEXT_FASTA) {
        const size_t n_tiles = n / ingest_scan_tile() + 2;
        if ((rc = ensure_device(&m->d_aux, &m->d_aux_cap, (n + 2) * 4 + n_tiles * 8 + 64))) return rc;
        d_len = (uint32_t *)m->d_aux;
        d_tile = (unsigned long long *)(((uintptr_t)(d_len + n + 2) + 15) & ~(uintptr_t)15);
    }
    unsigned long long total = 0;
    launch_ingest_select(d_keep, 0u, W.d_rec_start, n, (uint32_t)W.n_used, d_len, st);
    if ((rc = ensure_device((void **)&m->d_off, &m->d_off_cap, (n + 1) * sizeof(uint64_t)))) return rc;
    if ((rc = scan_offsets(d_len, n, d_tile, (unsigned long long *)m->d_off, st, &total, "selection of the kept records failed"))) return rc;
    S.n_kept_bytes = total;
    if (total > S.kept_cap) return fail(MK_E_CAPACITY, "the kept records take %llu bytes", total);
    if (!total) return MK_OK;
    if ((rc = ensure_device((void **)&m->d_seq, &m->d_seq_cap, total + 64))) return rc;
    launch_ingest_gather((const uint8_t *)W.T->d_text, W.d_rec_start, d_len, (const unsigned long long *)m->d_off, 0, n, m->d_seq, st, kBigRecord);
    // chromosome-sized records: one device copy each
    uint64_t at = 0;
    for (uint64_t r = 0; r < n; ++r) {
        if (!keep_host[r]) continue;
        const uint64_t len = (r + 1 < n ? rs[r + 1] : W.n_used) - rs[r];
        if (len >= kBigRecord && hipMemcpyAsync(m->d_seq + at, (const uint8_t *)W.T->d_text + rs[r], len, hipMemcpyDeviceToDevice, st) != hipSuccess)
            return fail(MK_E_HIP, "copy of a kept record failed");
        at += len;
    }
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(S.kept, m->d_seq, total, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "copy of the kept records failed");
    return MK_OK;
}


// the kept records of side W in their written form (include/merkurio_hip.h), packed on the device, then cut and deflated there:
// only the members come down -- or, below S.text_below bytes, the text.  With logging the ids of the kept records follow, packed by
// the sequences' gather kernel.  *status = 2: a FASTA record the device does not write (nothing has been written to S's buffers).
// The time of the codec's steps is ADDED to cut_ms / *cut_members (a paired window has two sides).
int window_members(mk_matcher *m, mk_codec *codec, uint32_t format, WindowSide &W, uint64_t n, const uint8_t *d_keep, const std::vector<uint32_t> &rs,
                   const uint8_t *keep_host, int logging, mk_window_members &S, DeviceLoop &dl, float cut_ms[3], uint64_t *cut_members, uint32_t *status) {
    hipStream_t st = dl.st;
    if (!n) return MK_OK;
    int rc;
    const bool fasta = format == MK_TEXT_FASTA;
    const uint8_t *d_text = (const uint8_t *)W.T->d_text;
    // scratch: written lengths | id starts | id lengths | refusal word | tile sums
    const size_t n_tiles = n / ingest_scan_tile() + 2;
    if ((rc = ensure_device(&m->d_aux, &m->d_aux_cap, 3 * (n + 2) * 4 + 16 + n_tiles * 8 + 64))) return rc;
    uint32_t *d_len = (uint32_t *)m->d_aux, *d_id_start = d_len + n + 2, *d_id_len = d_id_start + n + 2, *d_refused = d_id_len + n + 2;
    unsigned long long *d_tile = (unsigned long long *)(((uintptr_t)(d_refused + 1) + 15) & ~(uintptr_t)15);
    if ((rc = ensure_device((void **)&m->d_off, &m->d_off_cap, (n + 1) * sizeof(uint64_t)))) return rc;
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
        if ((rc = ensure_device((void **)&m->d_seq, &m->d_seq_cap, total + 64 + mkz::kPad))) return rc;
        // chromosome-sized FASTA records: one device copy each at their written offset, but for the last 16 stored bytes (the kernel's)
        bool big = false;
        for (uint64_t r = 0; fasta && r < n && !big; ++r) big = keep_host[r] && rs[r + 1] - rs[r] >= kBigRecord;
        if (big) {
            std::vector<unsigned long long> off(n + 1);
            if (hipMemcpyAsync(off.data(), d_off, (n + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
                return fail(MK_E_HIP, "copy of the written offsets failed");
            for (uint64_t r = 0; r < n; ++r) {
                const uint64_t len = rs[r + 1] - rs[r];
                if (keep_host[r] && len >= kBigRecord &&
                    hipMemcpyAsync(m->d_seq + off[r], d_text + rs[r], len - 16, hipMemcpyDeviceToDevice, st) != hipSuccess)
                    return fail(MK_E_HIP, "copy of a kept record failed");
            }
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
            } else if (hipMemcpyAsync(S.members, m->d_seq, total, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
                return fail(MK_E_HIP, "copy of the written records failed");
            }
        } else {
            std::lock_guard<std::mutex> lock(codec->mu);
            uint64_t need = 0, members = 0;
            // (the codec times its steps by the host's clock: the gather must not run into the cut kernel's share)
            if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "gather of the written records failed");
            // the offsets scan is the record-end table: off[r + 1] = where record r's written form ends (a record that is not kept
            // repeats the end in front of it)
            if ((rc = mkz::deflate_ranges(codec, st, m->d_seq, total, d_off + 1, n, nullptr, 0, S.members, S.members_cap, &need, &members))) return rc;
            for (int k = 0; k < 3; ++k) cut_ms[k] += codec->cut_ms[k];
            *cut_members += members;
            S.n_member_bytes = need, S.n_members = members;
            if (need > S.members_cap) cap_rc = fail(MK_E_CAPACITY, "the members of the kept records take %llu bytes", (unsigned long long)need);
        }
    }
    kernel_ms();
    if (!logging || !S.n_kept) return cap_rc;
    // ---- the ids of the kept records, packed the way the sequences are: start and length table, offsets scan, gather
    if ((rc = scan_offsets(d_id_len, n, d_tile, d_off, st, &total, "selection of the ids failed"))) return rc;
    S.n_id_bytes = total;
    if (total > S.ids_cap) return fail(MK_E_CAPACITY, "the ids of the kept records take %llu bytes", total);
    std::vector<unsigned long long> off(n + 1);
    if ((rc = ensure_device((void **)&m->d_seq, &m->d_seq_cap, total + 64))) return rc;
    launch_ingest_gather(d_text, d_id_start, d_id_len, d_off, 0, n, m->d_seq, st);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(off.data(), d_off, (n + 1) * 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (total && hipMemcpyAsync(S.ids, m->d_seq, total, hipMemcpyDeviceToHost, st) != hipSuccess) || hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "copy of the ids failed");
    uint64_t q = 0;
    for (uint64_t r = 0; r < n; ++r)
        if (keep_host[r]) S.id_end[q++] = off[r + 1];
    return cap_rc;
}
}  // namespace

extern "C" {

int mk_host_alloc(size_t bytes, void **out) {
    if (!out) return fail(MK_E_INVALID_ARG, "null argument");
    *out = nullptr;
    hipError_t e = hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault);
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc");
    return MK_OK;
}

void mk_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

int mk_upload_text_ahead(mk_matcher *m, const uint8_t *text, uint64_t n_text) {
    if (!m || (n_text && !text)) return fail(MK_E_INVALID_ARG, "null argument");
    if (n_text == 0 || n_text >= 0xFFFFFFF0ull) return MK_OK;  // (nothing to do / the call itself will refuse it)
    MK_ABI_BEGIN
    if (hipSetDevice(m->device) != hipSuccess) return fail(MK_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(m->ahead_mu);
    if (!m->stream_ahead && hipStreamCreateWithFlags(&m->stream_ahead, hipStreamNonBlocking) != hipSuccess)
        return fail(MK_E_HIP, "hipStreamCreate failed");
    mk_matcher::AheadSlot *slot = nullptr;
    // a slot that still holds an earlier window from this very buffer is stale (the host did not come back for it and is now
    // refilling the buffer): its copy must have finished reading before the new bytes are trusted -- the caller has of course
    // already overwritten them, so all that is left to do is to wait and take the slot over
    for (auto &a : m->ahead)
        if (a.text == text) {
            if (hipEventSynchronize(a.ev) != hipSuccess) return fail(MK_E_HIP, "hipEventSynchronize failed");
            a.text = nullptr;
            slot = &a;
        }
    for (auto &a : m->ahead)
        if (!a.text && !slot) slot = &a;
    if (!slot) return MK_OK;  // every slot waits already: this window will upload itself
    if (!slot->ev && hipEventCreateWithFlags(&slot->ev, hipEventDisableTiming) != hipSuccess) return fail(MK_E_HIP, "hipEventCreate failed");
    int rc = ensure_device(&slot->d, &slot->cap, n_text + 64);
    if (rc) return rc;
    if (hipMemcpyAsync(slot->d, text, n_text, hipMemcpyHostToDevice, m->stream_ahead) != hipSuccess ||
        hipEventRecord(slot->ev, m->stream_ahead) != hipSuccess)
        return fail(MK_E_HIP, "upload of the next text window failed");
    slot->text = text;
    slot->n = n_text;
    return MK_OK;
    MK_ABI_END
}

}  // extern "C"

namespace {

// the body of mk_extract_window (mem == nullptr) and mk_extract_window_members (one mk_window_members per source)
int extract_window_body(mk_matcher *m, mk_codec *codec, uint32_t format, uint32_t n_sources, mk_window_source *src, mk_window_members *mem, int logging,
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
            return fail(MK_E_INVALID_ARG, "mk_extract_window_members: a size without its buffer in source %u", k);
        if (S.kept || S.kept_cap) return fail(MK_E_INVALID_ARG, "mk_extract_window_members: the kept records leave as members, not as source %u's kept text", k);
    }
    if (mem) {
        if (!codec) return fail(MK_E_INVALID_ARG, "mk_extract_window_members: the members need a codec handle");
        if (codec->device != m->device) return fail(MK_E_INVALID_ARG, "mk_extract_window_members: the codec and the matcher are on different devices");
        if (logging && invert) return fail(MK_E_INVALID_ARG, "mk_extract_window_members: with logging and invert the rows name records that are not kept");
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
        } else {
            uint8_t *fa_seq = nullptr;
            if (format == MK_TEXT_FASTA) {  // the index step compacts the sequences already: every input has a buffer of its own for them
                if ((rc = ensure_device(&W[k].T->d_fa_seq, &W[k].T->d_fa_seq_cap, W[k].n_window + 64))) return rc;
                fa_seq = (uint8_t *)W[k].T->d_fa_seq;
            }
            if ((rc = window_index(m, format, src[k].ends_at_record != 0, W[k], fa_seq, st, status))) return rc;
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
        c->nb_records_tot += 2 * n;  // :472
        c->nb_bases += n_seq[0] + n_seq[1];
        c->nb_hits_tot[0] += found[0];
        c->nb_hits_tot[1] += found[1];
        c->nb_records_hit[0] += flagged[0];
        c->nb_records_hit[1] += flagged[1];
        total_rows = found[0] + found[1];
        if (!ac && std::max(n_seq[0], n_seq[1]) >= (1ull << 31))  // (BNDMq's pair order keeps the mate in bit 31 of the position)
            return fail(MK_E_UNSUPPORTED, "mk_extract_window: paired windows of 2 GiB of sequence or more under BNDMq");
        if ((rc = dl.join_mates(found[0], n, rows, rows_cap, counts))) return rc;
    }
    // ---- keep (single :400-405, paired :600-606), on the host for the caller and on the device for the kept records' text
    dl.host_begin();
    extract_keep(f[0].data(), paired ? f[1].data() : nullptr, n, invert, keep, c);
    dl.mark(1);
    bool want_kept = false;
    for (uint32_t k = 0; k < n_sources; ++k) want_kept = want_kept || src[k].kept != nullptr || src[k].kept_cap != 0;
    if (want_kept) {
        if ((rc = ensure_device((void **)&m->d_flags2, &m->d_flags2_cap, n + 8))) return rc;
        if (hipMemcpyAsync(m->d_flags2, keep, n, hipMemcpyHostToDevice, st) != hipSuccess) return fail(MK_E_HIP, "upload of the keep flags failed");
        int cap_rc = MK_OK;
        for (uint32_t k = 0; k < n_sources; ++k) {
            if (!src[k].kept && !src[k].kept_cap) continue;
            rc = window_kept(m, format, W[k], n, m->d_flags2, rs[k], keep, src[k], dl);
            if (rc == MK_E_CAPACITY) cap_rc = rc;  // (every source reports its need before the call returns)
            else if (rc) return rc;
        }
        if (cap_rc) return cap_rc;
    }
    if (mem) {
        if ((rc = ensure_device((void **)&m->d_flags2, &m->d_flags2_cap, n + 8))) return rc;
        if (hipMemcpyAsync(m->d_flags2, keep, n, hipMemcpyHostToDevice, st) != hipSuccess) return fail(MK_E_HIP, "upload of the keep flags failed");
        int cap_rc = MK_OK;
        float cut_ms[3] = {0, 0, 0};
        uint64_t cut_members = 0;
        for (uint32_t k = 0; k < n_sources && !*status; ++k) {
            rc = window_members(m, codec, format, W[k], n, m->d_flags2, rs[k], keep, logging, mem[k], dl, cut_ms, &cut_members, status);
            if (rc == MK_E_CAPACITY) cap_rc = rc;  // (every source reports its needs before the call returns)
            else if (rc) return rc;
        }
        {
            std::lock_guard<std::mutex> lock(codec->mu);
            for (int k = 0; k < 3; ++k) codec->cut_ms[k] = cut_ms[k];
            codec->cut_members = cut_members;
        }
        if (*status) {  // a record the device does not write: nothing of this window has left as members
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
    return extract_window_body(m, codec, format, n_sources, src, nullptr, logging, invert, rec_cap, n_rec_out, keep, rows, rows_cap, n_rows, c, counts, status);
}

int mk_extract_window_members(mk_matcher *m, mk_codec *codec, uint32_t format, uint32_t n_sources, mk_window_source *src, mk_window_members *mem,
                              int logging, int invert, uint64_t rec_cap, uint64_t *n_rec_out, uint8_t *keep, mk_row *rows, uint64_t rows_cap,
                              uint64_t *n_rows, mk_counters *c, uint32_t *counts, uint32_t *status) {
    if (!mem) return fail(MK_E_INVALID_ARG, "null argument");
    return extract_window_body(m, codec, format, n_sources, src, mem, logging, invert, rec_cap, n_rec_out, keep, rows, rows_cap, n_rows, c, counts, status);
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

// ---- `tag` on a window of BAM text that stays on the device (r05, ABI v7; kernels: bam.hip) ---------------------------------------
}  // extern "C"

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
                if ((rc = ensure_device((void **)&m->d_seq, &m->d_seq_cap, total + 64))) return rc;
                launch_ingest_gather(d_text, d_name_start, d_name_len, d_name_off, 0, n, m->d_seq, st);
                if (sam) launch_sam_name_ends(d_name_len, d_name_off, n, m->d_seq, st);
                if (hipGetLastError() != hipSuccess || hipMemcpyAsync(X.names, m->d_seq, total, hipMemcpyDeviceToHost, st) != hipSuccess ||
                    hipStreamSynchronize(st) != hipSuccess)
                    return fail(MK_E_HIP, "download of the names failed");
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
    const uint32_t n_blocks = (uint32_t)((n_text + ingest_block_bytes() - 1) / ingest_block_bytes());
    if ((rc = ensure_device(&T.d_ing_a, &T.d_ing_a_cap, ((size_t)n_blocks + 8) * 4))) return rc;  // newline count per block | total | status, min, max
    W.d_block = (uint32_t *)T.d_ing_a;
    W.d_total = W.d_block + n_blocks;
    W.d_st = W.d_total + 1;
    launch_ingest_count(d_text, n_text, W.d_block, W.d_total, st);
    if (hipMemcpyAsync(&W.total_nl, W.d_total, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&W.last_byte, d_text + n_text - 1, 1, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "newline count failed");
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

// the pair loop with the rows merged on the host (mates of 2 GiB or more under BNDMq: the device pair order keeps
// the mate in bit 31 of the position)
static int extract_paired_host_merge(mk_matcher *m, const uint8_t *seq1, const uint64_t *off1, const uint8_t *seq2,
                                     const uint64_t *off2, uint64_t n_rec, int invert, uint8_t *keep, mk_row *rows,
                                     uint64_t rows_cap, uint64_t *n_rows, mk_counters *c, uint32_t *counts) {
    std::vector<uint8_t> f1, f2;
    std::vector<mk_hit> h1, h2;
    int rc = scan_all(m, seq1, off1, n_rec, MK_MODE_HITS, f1, h1);
    if (rc) return rc;
    rc = scan_all(m, seq2, off2, n_rec, MK_MODE_HITS, f2, h2);
    if (rc) return rc;
    RowSink sink{rows, rows_cap};
    c->nb_records_tot += 2 * n_rec;  // :472
    c->nb_bases += (off1[n_rec] - off1[0]) + (off2[n_rec] - off2[0]);
    c->nb_hits_tot[0] += h1.size();
    c->nb_hits_tot[1] += h2.size();
    c->nb_records_hit[0] += popcount_flags(f1, n_rec);
    c->nb_records_hit[1] += popcount_flags(f2, n_rec);
    count_patterns(m->algo, h1, counts);  // BNDMq: once per mate that hit (:575-584)
    count_patterns(m->algo, h2, counts);
    size_t i1 = 0, i2 = 0;  // merge the two ordered hit lists pair by pair
    while (i1 < h1.size() || i2 < h2.size()) {
        const uint64_t r1 = i1 < h1.size() ? h1[i1].rec : ~0ull, r2 = i2 < h2.size() ? h2[i2].rec : ~0ull;
        const uint64_t r = std::min(r1, r2);
        size_t e1 = i1, e2 = i2;
        while (e1 < h1.size() && h1[e1].rec == r) ++e1;
        while (e2 < h2.size() && h2[e2].rec == r) ++e2;
        if (m->algo == MK_ALGO_AC) {  // all of mate 1, then all of mate 2 (:480-533)
            for (size_t k = i1; k < e1; ++k) sink.push(0, h1[k]);
            for (size_t k = i2; k < e2; ++k) sink.push(1, h2[k]);
        } else {  // per pattern: mate-1 hits then mate-2 hits (:543-585)
            size_t a = i1, b = i2;
            while (a < e1 || b < e2) {
                const uint32_t pa = a < e1 ? h1[a].pat : 0xFFFFFFFFu, pb = b < e2 ? h2[b].pat : 0xFFFFFFFFu;
                const uint32_t p = std::min(pa, pb);
                while (a < e1 && h1[a].pat == p) sink.push(0, h1[a++]);
                while (b < e2 && h2[b].pat == p) sink.push(1, h2[b++]);
            }
        }
        i1 = e1;
        i2 = e2;
    }
    for (uint64_t r = 0; r < n_rec; ++r) {  // :600-606
        const bool found = f1[r] || f2[r];
        keep[r] = (uint8_t)(found != (invert != 0));
        c->nb_records_extracted += 2 * keep[r];
    }
    if (n_rows) *n_rows = sink.n;
    if (rows && sink.n > rows_cap) return fail(MK_E_CAPACITY, "rows buffer too small: need %llu", (unsigned long long)sink.n);
    return MK_OK;
}

int mk_extract_paired(mk_matcher *m, const uint8_t *seq1, const uint64_t *off1, uint64_t n_rec1,
                      const uint8_t *seq2, const uint64_t *off2, uint64_t n_rec2, int logging, int invert,
                      uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *c,
                      uint32_t *counts) {
    if (!m || !keep || !c || (logging && !counts)) return fail(MK_E_INVALID_ARG, "null argument");
    if (n_rows) *n_rows = 0;
    if (n_rec1 != n_rec2)  // src/cmd_extract.rs:465-468, :608-612
        return fail(MK_E_PAIR_MISMATCH,
                    "The two input files have a different number of records. Please provide valid paired-end read files.");
    const uint64_t n_rec = n_rec1;
    if (n_rec == 0) return MK_OK;
    if (!off1 || !off2) return fail(MK_E_INVALID_ARG, "null buffer");
    MK_ABI_BEGIN
    const bool ac = m->algo == MK_ALGO_AC;
    if (logging && !ac) {  // the device pair order of BNDMq keeps the mate in bit 31 of the position
        bool small = true;
        if ((off1[n_rec] - off1[0]) >= (1ull << 31) || (off2[n_rec] - off2[0]) >= (1ull << 31))
            for (uint64_t i = 0; i < n_rec && small; ++i)
                small = off1[i + 1] - off1[i] < (1ull << 31) && off2[i + 1] - off2[i] < (1ull << 31);
        if (!small) return extract_paired_host_merge(m, seq1, off1, seq2, off2, n_rec, invert, keep, rows, rows_cap, n_rows, c, counts);
    }
    DeviceLoop dl(m);
    std::vector<uint8_t> f1(n_rec), f2(n_rec);
    uint64_t flagged1 = 0, flagged2 = 0;
    const uint32_t mode = logging ? MK_MODE_HITS : MK_MODE_ANY;
    int rc = dl.scan(seq1, off1, n_rec, mode, f1.data(), &flagged1);
    if (rc) return rc;
    const unsigned long long n1 = dl.found;
    if (logging && (rc = dl.stash_mate1())) return rc;
    if ((rc = dl.scan(seq2, off2, n_rec, mode, f2.data(), &flagged2))) return rc;
    const unsigned long long n2 = dl.found;
    if (logging) {
        c->nb_records_tot += 2 * n_rec;  // :472
        c->nb_bases += (off1[n_rec] - off1[0]) + (off2[n_rec] - off2[0]);
        c->nb_hits_tot[0] += n1;
        c->nb_hits_tot[1] += n2;
        c->nb_records_hit[0] += flagged1;
        c->nb_records_hit[1] += flagged2;
        if ((rc = dl.join_mates(n1, n_rec, rows, rows_cap, counts))) return rc;
    }
    dl.host_begin();
    extract_keep(f1.data(), f2.data(), n_rec, invert, keep, c);
    dl.finish();
    const uint64_t total_rows = logging ? n1 + n2 : 0;
    if (n_rows) *n_rows = total_rows;
    return check_rows_cap(logging, rows, rows_cap, total_rows);
    MK_ABI_END
}

int mk_tag_records(mk_matcher *m, const uint8_t *seq, const uint64_t *off, uint64_t n_rec, int logging,
                   int filter_matching, int invert, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows,
                   mk_counters *c, uint32_t *counts, uint64_t *found_off, uint32_t *found_pat, uint64_t found_cap) {
    if (!m || !keep || !c || !found_off || (logging && !counts)) return fail(MK_E_INVALID_ARG, "null argument");
    if (n_rows) *n_rows = 0;
    found_off[0] = 0;
    if (n_rec == 0) return MK_OK;
    MK_ABI_BEGIN
    DeviceLoop dl(m);
    std::vector<uint8_t> flags(n_rec);
    uint64_t flagged = 0;
    // the tag loop always needs the matched-pattern SET (src/cmd_tag.rs:392-442)
    int rc = dl.scan(seq, off, n_rec, MK_MODE_HITS, flags.data(), &flagged);
    if (rc) return rc;
    const bool ac = m->algo == MK_ALGO_AC;
    bool set_order = false;  // are the tuples in (record, pattern, position) order?
    if (logging) {  // (records counted before filtering, :446-450)
        if ((rc = dl.log_single(c, n_rec, off[n_rec] - off[0], flagged, rows, rows_cap))) return rc;
        set_order = !ac;
        if (ac && (rc = dl.pattern_counts(true, n_rec, counts))) return rc;  // one per hit (:412); BNDMq: below, from the sets
    }
    // distinct matched patterns per record, ascending: kmers_found after sort_unstable + dedup (:484-485)
    if (!set_order && (rc = dl.order(false, n_rec))) return rc;
    uint64_t n_found = 0;
    if ((rc = dl.pattern_sets(n_rec, found_off, found_pat, found_cap, &n_found, (logging && !ac) ? counts : nullptr))) return rc;
    dl.host_begin();
    for (uint64_t r = 0; r < n_rec; ++r) {  // :457-467
        const bool has = flags[r] != 0;
        keep[r] = (uint8_t)(filter_matching ? has : (invert ? !has : true));
        c->nb_records_extracted += keep[r];
    }
    dl.finish();
    if (n_rows) *n_rows = logging ? dl.found : 0;
    if (n_found > found_cap) return fail(MK_E_CAPACITY, "found_pat too small: need %llu", (unsigned long long)n_found);
    return check_rows_cap(logging, rows, rows_cap, dl.found);
    MK_ABI_END
}

int mk_matcher_batch_times(const mk_matcher *m, float ms[4]) {
    if (!m || !ms) return fail(MK_E_INVALID_ARG, "null argument");
    for (int i = 0; i < 4; ++i) ms[i] = m->batch_ms[i];
    return MK_OK;
}

int mk_tag_value(const mk_matcher *m, const uint32_t *found_pat, uint64_t n_found, const char *existing, char *out,
                 size_t cap, size_t *out_len) {
    if (!m || (!found_pat && n_found)) return fail(MK_E_INVALID_ARG, "null argument");
    MK_ABI_BEGIN
    std::vector<std::string> items;
    for (uint64_t i = 0; i < n_found; ++i) {
        const uint32_t p = found_pat[i];
        if (p >= m->n_pat) return fail(MK_E_INVALID_ARG, "pattern index %u out of range", p);
        items.emplace_back((const char *)m->pat_bytes.data() + m->pat_off[p], m->pat_off[p + 1] - m->pat_off[p]);
    }
    if (existing && existing[0]) {  // src/cmd_tag.rs:470-481: non-empty Z value split on ','
        const char *s = existing;
        for (;;) {
            const char *e = strchr(s, ',');
            items.emplace_back(s, e ? (size_t)(e - s) : strlen(s));
            if (!e) break;
            s = e + 1;
        }
    }
    std::sort(items.begin(), items.end());  // :484-485
    items.erase(std::unique(items.begin(), items.end()), items.end());
    std::string joined;
    for (size_t i = 0; i < items.size(); ++i) {
        if (i) joined += ',';
        joined += items[i];
    }
    if (out_len) *out_len = joined.size();
    if (!out || cap < joined.size() + 1) return fail(MK_E_CAPACITY, "tag buffer too small: need %zu", joined.size() + 1);
    memcpy(out, joined.c_str(), joined.size() + 1);
    return MK_OK;
    MK_ABI_END
}

}  // extern "C"
