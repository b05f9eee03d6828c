#include "sam_in.hpp"

#include "bam_text.hpp"
#include "host_mem.hpp"

namespace cli {

// SAM text: header lines ('@') may appear anywhere a line starts; records keep their file order.
// The text is cut at line starts into one piece per host thread; a record is five offsets.
// The records of the lines of d[from, stop) (both at line starts) are appended to recs; '@' lines are skipped (open() took the header)
static void parse_sam_text(const char *d, uint64_t n, uint64_t from, uint64_t stop, std::vector<SamFile::Rec> &recs) {
    const uint64_t span = stop - from;
    const size_t T = std::max<size_t>(1, std::min<size_t>(io_threads(), span / (8u << 20) + 1));
    std::vector<uint64_t> cut(T + 1, stop);
    cut[0] = from;
    for (size_t t = 1; t < T; ++t) {
        uint64_t p = std::max<uint64_t>(cut[t - 1], from + span * t / T);
        if (p > 0 && p < stop) p = line_end(d, n, p - 1) + 1;  // first line start at or after p
        cut[t] = std::min(p, stop);
    }
    std::vector<std::vector<SamFile::Rec>> parts(T);
    run_threads(T, [&](size_t t) {
        uint64_t p = cut[t];
        const uint64_t stop = cut[t + 1];
        parts[t].reserve((stop - p) / 300 + 16);
        while (p < stop) {
            const uint64_t e = line_end(d, n, p);
            const uint64_t le = strip_cr(d, p, e);
            if (le > p && d[p] != '@') {
                SamFile::Rec r;
                r.off = p;
                r.len = (uint32_t)(le - p);
                const char *q = (const char *)memchr(d + p, '\t', le - p);
                if (!q) bail("Error during SAM record parsing: too few fields");
                r.name_len = (uint32_t)(q - (d + p));
                for (int f = 1; f < 9; ++f) {  // q: the tab in front of field f + 1
                    q = (const char *)memchr(q + 1, '\t', d + le - (q + 1));
                    if (!q) bail("Error during SAM record parsing: too few fields");
                }
                const char *sb = q + 1;
                const char *se = (const char *)memchr(sb, '\t', d + le - sb);
                if (!se) se = d + le;
                r.seq_off = (uint64_t)(sb - d);
                r.l_seq = (se - sb == 1 && *sb == '*') ? 0 : (uint32_t)(se - sb);
                parts[t].push_back(r);
            }
            p = e + 1;
        }
    });
    size_t total = recs.size();
    for (auto &v : parts) total += v.size();
    recs.reserve(total);
    for (auto &v : parts) recs.insert(recs.end(), v.begin(), v.end());
}

// where a window of SAM text that starts at d[from] (a line start) and takes ~window_bytes ends: the first line start at or after
// the target; more_follows (d[0, n) is not the end of the text, its last line may go on): complete lines only
static uint64_t sam_window_stop(const char *d, uint64_t n, uint64_t from, uint64_t window_bytes, bool more_follows) {
    uint64_t stop = std::min(n, from + window_bytes);
    if (stop < n) stop = std::min(line_end(d, n, stop > 0 ? stop - 1 : 0) + 1, n);
    if (stop >= n && more_follows) {
        stop = n;
        while (stop > from && d[stop - 1] != '\n') --stop;
    }
    return stop;
}

// BAM header + reference dictionary at d[0,n).  false: the bytes end inside it (take more input).
static bool parse_bam_header(const char *d, uint64_t n, SamFile &out, uint64_t *end) {
    const uint8_t *p = (const uint8_t *)d, *e = p + n;
    auto need = [&](size_t k) { return (size_t)(e - p) >= k; };
    if (!need(8)) return false;
    if (memcmp(p, "BAM\1", 4) != 0) bail("Error reading BAM file: bad magic");
    int32_t l_text;
    memcpy(&l_text, p + 4, 4);
    if (l_text < 0) bail("Error during BAM record parsing: truncated file");
    p += 8;
    if (!need((size_t)l_text + 4)) return false;
    size_t tl = (size_t)l_text;
    while (tl && p[tl - 1] == 0) --tl;
    out.header.assign((const char *)p, tl);
    if (!out.header.empty() && out.header.back() != '\n') out.header += '\n';
    p += l_text;
    int32_t n_ref;
    memcpy(&n_ref, p, 4);
    p += 4;
    out.ref_names.clear();
    out.ref_lens.clear();
    for (int32_t i = 0; i < n_ref; ++i) {
        if (!need(4)) return false;
        int32_t l_name;
        memcpy(&l_name, p, 4);
        if (l_name < 0) bail("Error during BAM record parsing: truncated file");
        if (!need(4 + (size_t)l_name + 4)) return false;
        out.ref_names.emplace_back((const char *)p + 4, l_name > 0 ? (size_t)l_name - 1 : 0);
        uint32_t l_ref;
        memcpy(&l_ref, p + 4 + l_name, 4);
        out.ref_lens.push_back(l_ref);
        p += 4 + (size_t)l_name + 4;
    }
    *end = (uint64_t)((const char *)p - d);
    return true;
}

// Records from d + from on: a chain of block_size fields; the fixed part of each record is validated here
// so that later (parallel) accesses stay inside the record.  Stops after the record that crosses `soft_stop`
// (window size) or in front of a record that does not end inside d[0,n) -- an error unless partial_ok.
// Returns the offset behind the last record taken.
static uint64_t parse_bam_records_serial(const char *d, uint64_t n, uint64_t from, uint64_t soft_stop, bool partial_ok, std::vector<SamFile::Rec> &recs) {
    uint64_t p = from;
    while (p < n && p < soft_stop) {
        if (n - p < 4) {
            if (partial_ok) break;
            bail("Error during BAM record parsing: truncated file");
        }
        int32_t block;
        memcpy(&block, d + p, 4);
        if (block < 32) bail("Error during BAM record parsing: truncated file");
        if (n - p - 4 < (uint64_t)block) {
            if (partial_ok) break;
            bail("Error during BAM record parsing: truncated file");
        }
        const uint8_t *r = (const uint8_t *)d + p + 4;
        const uint8_t l_name = r[8];
        uint16_t n_cig;
        int32_t l_seq;
        memcpy(&n_cig, r + 12, 2);
        memcpy(&l_seq, r + 16, 4);
        const uint64_t fixed = 32ull + l_name + 4ull * n_cig;
        if (l_seq < 0 || fixed + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq > (uint64_t)block)
            bail("Error during BAM record parsing: truncated file");
        SamFile::Rec rec;
        rec.off = p;
        rec.len = (uint32_t)block + 4;
        rec.name_len = l_name ? l_name - 1u : 0u;
        rec.seq_off = rec.off + 4 + fixed;
        rec.l_seq = (uint32_t)l_seq;
        recs.push_back(rec);
        p += 4 + (uint64_t)block;
    }
    return p;
}

// ---- the BAM record chain on all host threads -------------------------------------------------------------------
// A record's place is only known from the one before it (block_size hops): 8 M hops are 0.1 s per GiB on one thread.
// The chain is walked in pieces instead: every thread but the first FINDS a record start behind its piece's first byte --
// a position where four records in a row have consistent fixed fields (sizes that add up, a printable NUL-terminated name,
// reference ids and positions >= -1) -- and walks from there; the pieces are accepted only if every walk ends EXACTLY on
// the next piece's start, which no false start survives.  Anything else falls back to the serial walk above.
static int64_t bam_record_size_if_plausible(const uint8_t *d, uint64_t n, uint64_t p) {  // 4 + block_size, 0 = not a record, -1 = runs out of d
    if (n - p < 36) return -1;
    int32_t block, ref, pos, l_seq, nref, npos;
    memcpy(&block, d + p, 4), memcpy(&ref, d + p + 4, 4), memcpy(&pos, d + p + 8, 4), memcpy(&l_seq, d + p + 20, 4);
    memcpy(&nref, d + p + 24, 4), memcpy(&npos, d + p + 28, 4);
    if (block < 32 || block > (1 << 28) || ref < -1 || ref > (1 << 24) || pos < -1 || l_seq < 0 || nref < -1 || nref > (1 << 24) || npos < -1) return 0;
    const uint8_t l_name = d[p + 12];
    uint16_t n_cig;
    memcpy(&n_cig, d + p + 16, 2);
    const uint64_t fixed = 32ull + l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq;
    if (l_name == 0 || fixed > (uint64_t)block) return 0;
    if (n - p - 4 < (uint64_t)block) return -1;
    const uint8_t *name = d + p + 36;
    if (name[l_name - 1] != 0) return 0;
    for (uint32_t k = 0; k + 1 < l_name; ++k)
        if (name[k] < 33 || name[k] > 126) return 0;
    return 4 + (int64_t)block;
}
// the first position at or behind `from` (and before `stop`) where four plausible records follow each other; ~0 = none
static uint64_t bam_find_record_start(const uint8_t *d, uint64_t n, uint64_t from, uint64_t stop) {
    for (uint64_t p = from; p < stop; ++p) {
        uint64_t q = p;
        int k = 0;
        for (; k < 4; ++k) {
            const int64_t sz = bam_record_size_if_plausible(d, n, q);
            if (sz <= 0) break;
            q += (uint64_t)sz;
        }
        if (k == 4) return p;
    }
    return ~0ull;
}

static uint64_t parse_bam_records(const char *d, uint64_t n, uint64_t from, uint64_t soft_stop, bool partial_ok, std::vector<SamFile::Rec> &recs) {
    const uint64_t span = soft_stop > from ? soft_stop - from : 0;
    const size_t T = std::min<size_t>(io_threads(), (size_t)(span >> 24));  // pieces of >= 16 MB
    if (T < 2) return parse_bam_records_serial(d, n, from, soft_stop, partial_ok, recs);
    std::vector<uint64_t> start(T + 1, ~0ull);
    start[0] = from;
    start[T] = soft_stop;
    run_threads(T - 1, [&](size_t t) {
        const uint64_t c = from + span * (t + 1) / T;
        start[t + 1] = bam_find_record_start((const uint8_t *)d, n, c, std::min<uint64_t>(soft_stop, c + (1u << 20)));
    });
    for (size_t t = 1; t < T; ++t)
        if (start[t] == ~0ull || start[t] <= start[t - 1]) return parse_bam_records_serial(d, n, from, soft_stop, partial_ok, recs);
    std::vector<std::vector<SamFile::Rec>> part(T);
    std::vector<uint64_t> end(T, 0);
    std::vector<std::string> err(T);
    run_threads(T, [&](size_t t) {
        try {
            // a piece ends where the next one starts; only the last one has the window's own end (and its partial_ok)
            end[t] = parse_bam_records_serial(d, t + 1 < T ? start[t + 1] : n, start[t], start[t + 1], t + 1 < T ? false : partial_ok, part[t]);
        } catch (const Error &e) {
            err[t] = e.what();
        }
    });
    bool ok = true;
    for (size_t t = 0; t < T; ++t) ok = ok && err[t].empty() && (t + 1 == T || end[t] == start[t + 1]);
    if (!ok) return parse_bam_records_serial(d, n, from, soft_stop, partial_ok, recs);  // (also words the errors in file order)
    size_t total = recs.size();
    for (auto &x : part) total += x.size();
    recs.reserve(total);
    for (auto &x : part) recs.insert(recs.end(), x.begin(), x.end());
    return end[T - 1];
}

void SamFile::open(const std::string &path) {
    const std::string ext = extension(path);
    if (ext.empty()) bail("Could not detect the file extension: \"" + path + "\"");
    if (ext != "sam" && ext != "bam") bail("Input file must be a BAM or SAM file.");
    header.clear();
    recs.clear();
    ref_names.clear();
    ref_lens.clear();
    is_bam = ext == "bam";
    src.open(path);
    cursor = 0;
    if (is_bam) {
        uint64_t end = 0;
        while (!parse_bam_header(bytes(), n_bytes(), *this, &end)) {
            if (src.exhausted()) bail("Error during BAM record parsing: truncated file");
            src.more_into(buf, buf_len, 1u << 16);
        }
        cursor = end;
    } else {
        // header = the '@' lines in front of the first record (SAM spec 1.3); a compressed text needs them
        // complete in the buffer first
        for (;;) {
            const char *d = bytes();
            const uint64_t n = n_bytes();
            uint64_t p = 0;
            bool complete = false;
            header.clear();
            while (p < n) {
                const uint64_t e = line_end(d, n, p);
                if (e >= n && !src.exhausted()) break;  // the line may go on
                const uint64_t le = strip_cr(d, p, e);
                if (le > p && d[p] != '@') {
                    complete = true;
                    break;
                }
                if (le > p) {
                    header.append(d + p, le - p);
                    header += '\n';
                }
                p = std::min(e + 1, n);
            }
            if (complete || p >= n) {
                if (complete || src.exhausted()) {
                    cursor = p;
                    break;
                }
            }
            if (!src.more_into(buf, buf_len, 1u << 16)) {
                cursor = p;
                break;
            }
        }
    }
    data = bytes();
}

void SamFile::seek_bam(size_t member, const char *head, uint64_t n_head, size_t end_member) {
    std::vector<char> b(head, head + n_head);  // (head may point into buf)
    buf.swap(b);
    buf_len = n_head;
    cursor = 0;
    recs.clear();
    have_next = false;
    bam_bounded = end_member < src.n_bgzf_members();
    src.seek_member(member, end_member);
    data = buf.data();
}

void SamFile::drop_front(uint64_t k) {
    if (src.mapped() || k == 0) return;
    if (k > buf_len) k = buf_len;
    memmove(buf.data(), buf.data() + k, buf_len - k);
    buf_len -= k;
}

// The next records of a compressed input: b[0, bl) holds the text not yet turned into records (it starts at a record /
// line start), more is inflated behind it until ~window_bytes are there, the records are parsed into rs; cur = the
// bytes of b they cover.  false: no record is left.
bool SamFile::next_window(std::vector<char> &b, uint64_t &bl, uint64_t &cur, std::vector<Rec> &rs, uint64_t window_bytes) {
    rs.clear();
    cur = 0;
    for (;;) {
        if (bl < window_bytes) src.more_into(b, bl, window_bytes - bl);
        const char *d = b.data();
        const uint64_t n = bl;
        if (cur >= n && src.exhausted()) return false;
        if (is_bam) {
            cur = parse_bam_records(d, n, cur, std::min<uint64_t>(n, cur + window_bytes), !src.exhausted() || bam_bounded, rs);
        } else {
            const uint64_t stop = sam_window_stop(d, n, cur, window_bytes, !src.exhausted());
            if (stop > cur) parse_sam_text(d, n, cur, stop, rs);
            cur = stop;
        }
        if (!rs.empty()) return true;
        if (src.exhausted() && cur >= n) return false;
        if (src.exhausted()) {  // bytes are left that are no record
            if (is_bam && !bam_bounded) bail("Error during BAM record parsing: truncated file");
            return false;  // (BAM with an end: the record that crosses it stays behind `cur`)
        }
        src.more_into(b, bl, std::max<uint64_t>(window_bytes, bl));  // one record larger than the window
    }
}

// (compressed input) the window after the current one, prepared beside it: the unconsumed tail of the current window
// opens a second buffer, the inflate (device codec or host threads) and the record index run on the calling thread while
// the current window's `data` / `recs` stay as they are; the next fill() swaps the result in
void SamFile::prefetch(uint64_t window_bytes) {
    if (src.mapped() || have_next) return;
    if (window_bytes < (1u << 16)) window_bytes = 1u << 16;
    carry_tail(buf, buf_len, cursor, nbuf, nbuf_len);
    next_more = next_window(nbuf, nbuf_len, ncursor, nrecs, window_bytes);
    have_next = true;
}

bool SamFile::fill(uint64_t window_bytes) {
    if (window_bytes < (1u << 16)) window_bytes = 1u << 16;
    if (!src.mapped()) {  // compressed: drop what became records, take more
        if (have_next) {  // prefetch() has done that already
            have_next = false;
            buf.swap(nbuf);
            buf_len = nbuf_len;
            cursor = ncursor;
            recs.swap(nrecs);
            nrecs.clear();
            data = buf.data();
            return next_more;
        }
        drop_front(cursor);
        const bool more = next_window(buf, buf_len, cursor, recs, window_bytes);
        data = buf.data();
        return more;
    }
    recs.clear();
    for (;;) {
        const char *d = src.text();
        const uint64_t n = std::min<uint64_t>(src.text_size(), text_end);
        data = d;
        if (cursor >= n) return false;
        if (is_bam) {
            cursor = parse_bam_records(d, n, cursor, std::min<uint64_t>(n, cursor + window_bytes), false, recs);
        } else {
            const uint64_t stop = sam_window_stop(d, n, cursor, window_bytes, false);
            if (stop > cursor) parse_sam_text(d, n, cursor, stop, recs);
            cursor = stop;
        }
        if (!recs.empty()) return true;
        // a window without records (blank lines): next one
    }
}

void SamFile::gather(size_t b0, size_t b1, std::vector<uint8_t> &seq, std::vector<uint64_t> &off) const {
    const size_t n = b1 - b0;
    off.resize(n + 1);
    off[0] = 0;
    for (size_t i = 0; i < n; ++i) off[i + 1] = off[i] + recs[b0 + i].l_seq;
    seq.resize(off[n] + 1);
    const size_t T = std::max<size_t>(1, std::min<size_t>(io_threads(), n / 65536 + 1));
    run_threads(T, [&](size_t t) {
        for (size_t i = n * t / T; i < n * (t + 1) / T; ++i) {
            uint8_t *o = seq.data() + off[i];
            const uint32_t l = recs[b0 + i].l_seq;
            const uint8_t *src = (const uint8_t *)data + recs[b0 + i].seq_off;
            if (is_bam) {
                for (uint32_t k = 0; k < l; ++k) o[k] = (uint8_t)kBamSeq[(src[k >> 1] >> ((~k & 1) << 2)) & 15];
            } else {  // the matcher sees upper-case text (bam crate: sequences are stored packed, case is lost)
                for (uint32_t k = 0; k < l; ++k) o[k] = (src[k] >= 'a' && src[k] <= 'z') ? (uint8_t)(src[k] & ~0x20) : src[k];
            }
        }
    });
    seq[off[n]] = 0;
}

void SamFile::append_line(size_t i, std::string &out) const {
    if (is_bam)
        bam_record_to_sam((const uint8_t *)data + recs[i].off, ref_names, out);
    else
        out.append(data + recs[i].off, recs[i].len);
}

int SamFile::find_tag(size_t i, const std::string &tag, std::string *val) const {
    if (!is_bam) {
        const char *b = data + recs[i].off, *e = b + recs[i].len;
        for (int f = 0; f < 11; ++f) {
            b = (const char *)memchr(b, '\t', e - b);
            if (!b) return 0;
            ++b;
        }
        while (b < e) {
            const char *t = (const char *)memchr(b, '\t', e - b);
            if (!t) t = e;
            if (t - b >= 5 && b[0] == tag[0] && b[1] == tag[1] && b[2] == ':') {
                if (b[3] != 'Z' || b[4] != ':') return 2;
                val->assign(b + 5, t - (b + 5));
                return 1;
            }
            b = t + 1;
        }
        return 0;
    }
    // BAM: walk the optional fields behind name, CIGAR, SEQ and QUAL
    const uint8_t *r = raw(i);
    Cur c{r + (recs[i].seq_off - recs[i].off - 4) + ((size_t)recs[i].l_seq + 1) / 2 + recs[i].l_seq, r + raw_len(i)};
    while (c.p < c.e) {
        const uint8_t *tg = c.take(2);
        const char type = (char)c.get<uint8_t>();
        const bool mine = tg[0] == (uint8_t)tag[0] && tg[1] == (uint8_t)tag[1];
        if (mine && type != 'Z') return 2;
        switch (type) {
        case 'A': case 'c': case 'C': c.take(1); break;
        case 's': case 'S': c.take(2); break;
        case 'i': case 'I': case 'f': c.take(4); break;
        case 'Z': case 'H': {
            const uint8_t *s0 = c.p;
            while (c.p < c.e && *c.p) ++c.p;
            if (mine) {
                val->assign((const char *)s0, c.p - s0);
                return 1;
            }
            if (c.p < c.e) ++c.p;
            break;
        }
        case 'B': {
            const char sub = (char)c.get<uint8_t>();
            const int32_t cnt = c.get<int32_t>();
            const size_t w = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            if (cnt < 0) bail("Error during BAM record parsing: truncated file");
            c.take(w * (size_t)cnt);
            break;
        }
        default: bail("Error during BAM record parsing: unknown tag type");
        }
    }
    return 0;
}

}  // namespace cli
