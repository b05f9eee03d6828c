// record_loops.cpp -- the driver loops on batches of records that the caller has parsed: mk_extract_single, mk_extract_paired (and its
// host merge for mates the device's pair order cannot hold), mk_tag_records, mk_tag_value; the page-locked buffers of their callers
#include <string>

#include "device_loop.hpp"

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
    extract_keep(f1.data(), f2.data(), n_rec, invert, keep, c);  // :600-606
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
    if (logging && (rc = dl.log_pair(c, n_rec, (off1[n_rec] - off1[0]) + (off2[n_rec] - off2[0]), n1, flagged1, flagged2, rows, rows_cap, counts))) return rc;
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

}  // extern "C"
