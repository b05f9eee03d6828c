// device_loop.hpp -- what the driver loops share: a call's steps on the device (DeviceLoop), the keep rule of extract, and the steps
// of a text window (window_ingest.cpp) that extract_window.cpp and tag_windows.cpp are made of.  The loops restate what the reference's
// record loops do with the matcher's answers, for batches, so that keep/drop decisions, log rows and counters are bit-identical:
//   extract single   src/cmd_extract.rs:321-406
//   extract paired   src/cmd_extract.rs:463-612
//   tag              src/cmd_tag.rs:387-490
// The matching itself is the gfx950 scan kernel; nothing here searches text.  extract (single) and tag work on the
// device from end to end: scan -> tuples ordered on the device (order_hits.hip) -> log rows, per-pattern counts and
// the per-record pattern sets by the kernels of sets.hip -> results copied back.  The host threads only turn flags
// into keep decisions.  The paired loop orders both mates' tuples as one list, the mate inside a key field.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "matcher_internal.h"

struct mk_codec;

#pragma GCC visibility push(hidden)  // (nothing of this is the library's interface)
namespace mk {

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

    // counters of a pair's two scans of n_rec records each (paired :472-533; mate 2's tuples are the scan's, mate 1's n1 were
    // stashed), then join_mates
    int log_pair(mk_counters *c, uint64_t n_rec, uint64_t n_bases, unsigned long long n1, uint64_t flagged1, uint64_t flagged2, mk_row *rows,
                 uint64_t rows_cap, uint32_t *counts) {
        c->nb_records_tot += 2 * n_rec;  // :472
        c->nb_bases += n_bases;
        c->nb_hits_tot[0] += n1;
        c->nb_hits_tot[1] += found;
        c->nb_records_hit[0] += flagged1;
        c->nb_records_hit[1] += flagged2;
        return join_mates(n1, n_rec, rows, rows_cap, counts);
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
inline void extract_keep(const uint8_t *f1, const uint8_t *f2, uint64_t n, int invert, uint8_t *keep, mk_counters *c) {
    for (uint64_t r = 0; r < n; ++r) {
        const bool hit = f1[r] || (f2 && f2[r]);
        keep[r] = (uint8_t)(hit != (invert != 0));
        c->nb_records_extracted += (f2 ? 2u : 1u) * keep[r];
    }
}

inline int check_rows_cap(int logging, const mk_row *rows, uint64_t rows_cap, uint64_t need) {
    if (logging && rows && need > rows_cap) return fail(MK_E_CAPACITY, "rows buffer too small: need %llu", (unsigned long long)need);
    return MK_OK;
}

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

// exclusive scan of d_len[0, n) -> d_off[0, n], its total d_off[n] -> *total (enqueued work waited for; `what`: the message of a failure)
inline int scan_offsets(const uint32_t *d_len, uint64_t n, unsigned long long *d_tile, unsigned long long *d_off, hipStream_t st, unsigned long long *total,
                 const char *what) {
    launch_ingest_offsets(d_len, n, d_tile, d_off, st);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(total, d_off + n, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "%s", what);
    return MK_OK;
}

// how a window's text holds its sequences: as they are (FASTQ), as BAM's 4-bit codes, as SAM's SEQ field (a-z upper-cased for the matcher)
enum SeqForm { kSeqPlain, kSeqBam, kSeqSam };

// ---- the steps of a text window (window_ingest.cpp; each is described where it is defined)
int window_assemble(mk_matcher *m, mk_codec *codec, mk_window_source &S, WindowSide &W, DeviceLoop &dl);
int line_table(WindowSide &W, hipStream_t st, size_t extra_bytes, uint8_t *first_byte);
int window_index(mk_matcher *m, uint32_t format, bool ends_at_record, WindowSide &W, uint8_t *d_seq_out, hipStream_t st, uint32_t *status,
                 uint64_t *open_from = nullptr);
int scan_sequences(mk_matcher *m, const WindowSide &W, uint64_t n, SeqForm form, DeviceLoop &dl, uint32_t mode, uint8_t *flags, uint64_t *flagged,
                   uint64_t *n_seq);
// pieces of the window's text, back to back in m->d_seq: scan_offsets into m->d_off says where each goes and what they take, then
int pack_room(mk_matcher *m, unsigned long long total, size_t pad);
int pack_gather(mk_matcher *m, const WindowSide &W, const uint32_t *d_start, const uint32_t *d_len, uint64_t n, unsigned long long total, size_t pad,
                uint32_t big_from, hipStream_t st, const char *what);
int pack_download(mk_matcher *m, void *dst, unsigned long long total, hipStream_t st, const char *what);

}  // namespace mk
#pragma GCC visibility pop
