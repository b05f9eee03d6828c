#include "fastx.hpp"

#include <sys/mman.h>

#include <thread>

#include "host_mem.hpp"

namespace cli {

// records of d[p, stop): p is at a record start (or blank lines before one); a record that starts
// before `stop` is parsed completely even if it runs past it
// partial_ok (windowed reading: more text follows d[0,n)): a record that cannot be shown to end inside
// d[0,n) is not an error, parsing stops in front of it.  Returns the offset where parsing stopped.
static uint64_t parse_fastx_range(const char *d, uint64_t n, uint64_t p, uint64_t stop, bool fastq,
                                  std::vector<FastxFile::Rec> &recs, bool partial_ok = false) {
    while (p < stop) {
        if (d[p] == '\n' || d[p] == '\r') {  // blank line between records
            ++p;
            continue;
        }
        FastxFile::Rec r{};
        if (!fastq) {
            if (d[p] != '>') bail("Error during FASTQ/A record parsing.");
            uint64_t e = line_end(d, n, p);
            r.id_b = p + 1;
            r.id_e = strip_cr(d, p + 1, e);
            uint64_t s = std::min(e + 1, n);
            r.raw_b = s;
            uint64_t q = s;  // the sequence runs to the line end before the next line that starts with '>'
            for (;;) {
                if (q >= n || d[q] == '>') break;
                q = std::min(line_end(d, n, q) + 1, n);
            }
            if (partial_ok && q >= n) return p;  // no following header in sight: the record may go on
            uint64_t re = q;
            while (re > s && (d[re - 1] == '\n' || d[re - 1] == '\r')) --re;  // drop the final line end
            r.raw_e = re;
            r.qual_b = r.qual_e = 0;
            p = q;
        } else {
            if (d[p] != '@') bail("Error during FASTQ/A record parsing.");
            uint64_t e1 = line_end(d, n, p);
            if (partial_ok) {  // all four lines, line ends included, must be inside the window
                uint64_t e = e1;
                for (int k = 0; k < 3 && e < n; ++k) e = line_end(d, n, e + 1);
                if (e >= n) return p;
            }
            if (e1 >= n) bail("Error during FASTQ/A record parsing.");
            r.id_b = p + 1;
            r.id_e = strip_cr(d, p + 1, e1);
            uint64_t e2 = line_end(d, n, e1 + 1);
            r.raw_b = e1 + 1;
            r.raw_e = strip_cr(d, e1 + 1, e2);
            if (e2 + 1 >= n || d[e2 + 1] != '+') bail("Error during FASTQ/A record parsing.");
            uint64_t e3 = line_end(d, n, e2 + 1);
            if (e3 >= n) bail("Error during FASTQ/A record parsing.");
            uint64_t e4 = line_end(d, n, e3 + 1);
            r.qual_b = e3 + 1;
            r.qual_e = strip_cr(d, e3 + 1, e4);
            if (r.qual_e - r.qual_b != r.raw_e - r.raw_b) bail("Error during FASTQ/A record parsing.");
            p = std::min(e4 + 1, n);
        }
        recs.push_back(r);
    }
    return p;
}

// first record start at or after `from` (line-aligned).  FASTQ: a line starting with '@' whose
// second-next line starts with '+' (a quality line may start with '@', but then the line two
// below it is a sequence line, which never starts with '+').
static uint64_t next_record_start(const char *d, uint64_t n, uint64_t from, bool fastq) {
    uint64_t p = from == 0 ? 0 : std::min(line_end(d, n, from - 1) + 1, n);
    while (p < n) {
        if (!fastq) {
            if (d[p] == '>') return p;
        } else if (d[p] == '@') {
            uint64_t e1 = line_end(d, n, p);
            uint64_t e2 = e1 < n ? line_end(d, n, e1 + 1) : n;
            if (e2 + 1 < n && d[e2 + 1] == '+') return p;
        }
        p = std::min(line_end(d, n, p) + 1, n);
    }
    return n;
}

uint64_t FastxFile::append_seq(size_t i, std::vector<uint8_t> &out) const {
    const Rec &r = recs[i];
    const size_t before = out.size();
    if (fastq) {
        out.insert(out.end(), data + r.raw_b, data + r.raw_e);
    } else {
        for (uint64_t k = r.raw_b; k < r.raw_e; ++k)
            if (data[k] != '\n' && data[k] != '\r') out.push_back((uint8_t)data[k]);
    }
    return out.size() - before;
}

void FastxFile::gather(size_t b0, size_t b1, std::vector<uint8_t> &seq, std::vector<uint64_t> &off) const {
    const size_t nb = b1 - b0;
    off.resize(nb + 1);
    off[0] = 0;
    if (!fastq) {  // FASTA: line breaks have to be squeezed out; few, long records
        seq.clear();
        for (size_t i = b0; i < b1; ++i) {
            append_seq(i, seq);
            off[i - b0 + 1] = seq.size();
        }
        seq.push_back(0);
        return;
    }
    for (size_t i = 0; i < nb; ++i) off[i + 1] = off[i] + raw_len(b0 + i);
    seq.resize(off[nb] + 1);
    const size_t T = std::max<size_t>(1, std::min<size_t>((size_t)io_threads(), nb / 65536 + 1));
    std::vector<std::thread> th;
    for (size_t t = 0; t < T; ++t)
        th.emplace_back([&, t] {
            for (size_t i = nb * t / T; i < nb * (t + 1) / T; ++i)
                memcpy(seq.data() + off[i], data + recs[b0 + i].raw_b, off[i + 1] - off[i]);
        });
    for (auto &x : th) x.join();
    seq[off[nb]] = 0;
}

void FastxFile::write(size_t i, Sink &w) const {
    // needletail's SequenceRecord::write(writer, None) ends every line with the record's own line
    // ending, detected on its header line: CRLF input stays CRLF (the wrapped lines inside a FASTA
    // raw_seq keep theirs anyway)
    const Rec &r = recs[i];
    const bool crlf = r.id_e < data_n && data[r.id_e] == '\r';
    const char *nl = crlf ? "\r\n" : "\n";
    const size_t nl_len = crlf ? 2 : 1;
    w.write(fastq ? "@" : ">", 1);
    w.write(data + r.id_b, r.id_e - r.id_b);
    w.write(nl, nl_len);
    w.write(data + r.raw_b, r.raw_e - r.raw_b);
    w.write(nl, nl_len);
    if (fastq) {
        w.write("+", 1);
        w.write(nl, nl_len);
        w.write(data + r.qual_b, r.qual_e - r.qual_b);
        w.write(nl, nl_len);
    }
}

void FastxFile::parse_span(uint64_t b, uint64_t e) { parse_fastx_range(data, data_n, b, e, fastq, recs); }
uint64_t FastxFile::parse_span_partial(uint64_t b, uint64_t e, bool partial_ok) { return parse_fastx_range(data, data_n, b, e, fastq, recs, partial_ok); }

// ---- FastxStream: FASTA / FASTQ records, one window at a time -----------------------------------------
// parses d[from, stop) into spare_recs (spare_data / spare_n / spare_end)
void FastxStream::parse_window(const char *d, uint64_t n, uint64_t from, uint64_t stop, bool partial_ok) {
    spare_data = d;
    spare_n = n;
    spare_recs.clear();
    uint64_t p = from;
    while (p < n && (d[p] == '\n' || d[p] == '\r')) ++p;
    spare_end = p;
    if (p >= n) return;
    if (!started && !starts_record(d[p])) bail("Error during FASTQ/A record parsing.");
    if (stop <= p) stop = std::min(n, p + 1);
    // split at record starts and parse the pieces on host threads
    uint64_t T = std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)io_threads(), (stop - p) / (16u << 20) + 1));
    std::vector<uint64_t> cut(T + 1);
    cut[0] = p;
    cut[T] = stop;
    for (uint64_t t = 1; t < T; ++t) cut[t] = std::min(stop, std::max(cut[t - 1], next_record_start(d, n, p + (stop - p) * t / T, fastq)));
    // A record longer than a piece (a chromosome in a FASTA) leaves no record start between the last split
    // targets and `stop`: those cuts were clamped to `stop`, i.e. to the middle of that record.  Drop the empty
    // trailing pieces, so that the piece that owns the record is the LAST one: it reports where the window really
    // ends, and it is the one that may find its record cut off by the end of a compressed buffer.
    while (T > 1 && cut[T - 1] >= stop) --T;  // cut[T] == stop still holds
    std::vector<std::vector<FastxFile::Rec>> parts(T);
    std::vector<uint64_t> ends(T, 0);
    run_threads((size_t)T, [&](size_t t) {
        parts[t].reserve((cut[t + 1] - cut[t]) / 200 + 16);
        // only the last piece can run into the end of the window
        ends[t] = parse_fastx_range(d, n, cut[t], cut[t + 1], fastq, parts[t], partial_ok && t + 1 == T);
    });
    size_t total = 0;
    for (auto &v : parts) total += v.size();
    spare_recs.reserve(total);
    for (auto &v : parts) spare_recs.insert(spare_recs.end(), v.begin(), v.end());
    spare_end = ends[T - 1];
}

void FastxStream::prefetch(uint64_t window_bytes) {
    if (have_spare) return;
    src.settle();
    if (window_bytes < (1u << 16)) window_bytes = 1u << 16;
    if (src.mapped()) {
        const uint64_t n = src.text_size();
        // a record that starts inside the window is parsed completely (the text behind it is mapped too)
        if (cursor < n) {
            const uint64_t a0 = cursor & ~(uint64_t)4095;  // page-aligned hint: this window's pages, now
            (void)madvise(const_cast<char *>(src.text()) + a0, (size_t)(std::min(n, cursor + window_bytes + (1u << 20)) - a0), MADV_WILLNEED);
            parse_window(src.text(), n, cursor, std::min(n, cursor + window_bytes), false);
        }
        else
            parse_window(src.text(), n, n, n, false);
        have_spare = true;
        return;
    }
    // compressed: the unconsumed tail of the current buffer opens the other one, then inflate until a
    // complete record is in it
    std::vector<char> &nb = bufs[cur ^ 1];
    uint64_t &nl = lens[cur ^ 1];
    carry_tail(bufs[cur], lens[cur], cursor, nb, nl);
    uint64_t want = window_bytes > nl ? window_bytes - nl : 0;
    for (;;) {
        if (want) src.more_into(nb, nl, want);
        parse_window(nb.data(), nl, 0, nl, !src.exhausted());
        if (!spare_recs.empty() || src.exhausted()) break;
        want = std::max<uint64_t>(window_bytes, nl);  // one record larger than the window: take more
    }
    have_spare = true;
}

bool FastxStream::fill(uint64_t window_bytes) {
    prefetch(window_bytes);
    have_spare = false;
    view.recs.swap(spare_recs);
    spare_recs.clear();
    view.data = spare_data;
    view.data_n = spare_n;
    view.fastq = fastq;
    cur_end = spare_end;
    if (!src.mapped()) cur ^= 1;
    cursor = cur_end;  // until consume() says otherwise: the whole window
    return !view.recs.empty();
}

void FastxStream::consume(size_t n) { cursor = n < view.recs.size() ? view.recs[n].id_b - 1 : cur_end; }

// ---- raw windows (device ingest) ------------------------------------------------------------------------------
// the last record start of d[0, n) at or behind `from` (n if there is none)
static uint64_t last_record_start(const char *d, uint64_t n, uint64_t from, bool fastq) {
    uint64_t last = n;
    for (uint64_t r = next_record_start(d, n, from, fastq); r < n; r = next_record_start(d, n, r + 1, fastq)) last = r;
    if (last == n && !fastq && from > 0) {
        // FASTA records can be far longer than the stretch that was searched (a chromosome): walk back to the last '>' at a line start
        for (uint64_t p = from; p > 0;) {
            const void *g = memrchr(d, '>', (size_t)p);
            if (!g) break;
            p = (uint64_t)((const char *)g - d);
            if (p == 0 || d[p - 1] == '\n') return p;
        }
    }
    return last;
}

bool FastxStream::raw_fill(uint64_t window_bytes, const char **text, uint64_t *n_out, uint64_t *resume) {
    *resume = 0;
    if (window_bytes < (1u << 16)) window_bytes = 1u << 16;
    src.settle();
    if (src.mapped()) {
        const char *d = src.text();
        const uint64_t n = src.text_size();
        uint64_t p = cursor;
        while (p < n && (d[p] == '\n' || d[p] == '\r')) ++p;
        if (p >= n || !starts_record(d[p])) return false;
        uint64_t end = std::min(n, p + window_bytes);
        if (end < n) {
            const uint64_t a0 = p & ~(uint64_t)4095;
            (void)madvise(const_cast<char *>(d) + a0, (size_t)(std::min(n, end + (1u << 20)) - a0), MADV_WILLNEED);
            end = next_record_start(d, n, end, fastq);  // the first record start at or behind the target
        }
        cursor = p;
        raw_next = end;
        *resume = end;
        *text = d + p;
        *n_out = end - p;
        return end > p;
    }
    // compressed: the unconsumed tail of the current buffer opens the other one, then inflate
    std::vector<char> &nb = bufs[cur ^ 1];
    uint64_t &nl = lens[cur ^ 1];
    carry_tail(bufs[cur], lens[cur], cursor, nb, nl);
    uint64_t want = window_bytes > nl ? window_bytes - nl : 0;
    uint64_t cut = 0;
    for (;;) {
        if (want) src.more_into(nb, nl, want);
        uint64_t p = 0;
        while (p < nl && (nb[p] == '\n' || nb[p] == '\r')) ++p;
        if (p >= nl && src.exhausted()) {
            cur ^= 1;
            cursor = nl;
            return false;
        }
        if (p < nl && !starts_record(nb[p])) {  // neither FASTQ nor FASTA: leave everything to fill()
            cur ^= 1;
            cursor = 0;
            return false;
        }
        if (src.exhausted()) {
            cut = nl;
            break;
        }
        // more text follows: hand out whole records only -- everything in front of the last record start
        cut = last_record_start(nb.data(), nl, nl > (1u << 20) ? nl - (1u << 20) : 0, fastq);
        if (cut < nl && cut > p) break;
        want = std::max<uint64_t>(window_bytes, nl);  // one record larger than the window: take more
    }
    cur ^= 1;
    cursor = 0;  // (until raw_consume: a refused window is parsed again by fill())
    raw_next = cut;
    *text = nb.data();
    *n_out = cut;
    return cut > 0;
}

void FastxStream::raw_consume() { cursor = raw_next; }

bool FastxStream::raw_skip(uint64_t n) {
    src.settle();
    if (src.mapped()) {
        cursor = std::min<uint64_t>(src.text_size(), n);
        return cursor == n;
    }
    // (everything inflated so far is in front of the cursor or in bufs[cur] behind it: nothing has been consumed)
    for (;;) {
        const uint64_t have = lens[cur] > cursor ? lens[cur] - cursor : 0;
        if (n <= have) {
            cursor += n;
            return true;
        }
        n -= have;
        lens[cur] = 0, cursor = 0;
        if (src.exhausted()) return false;
        src.more_into(bufs[cur], lens[cur], std::min<uint64_t>(n, 64u << 20));
    }
}

bool FastxStream::raw_rest(const char **text, uint64_t *n_out) {
    src.settle();
    if (src.mapped()) {
        const uint64_t n = src.text_size();
        if (cursor >= n) return false;
        *text = src.text() + cursor;
        *n_out = n - cursor;
        cursor = n;
        return true;
    }
    std::vector<char> &nb = bufs[cur ^ 1];
    uint64_t &nl = lens[cur ^ 1];
    carry_tail(bufs[cur], lens[cur], cursor, nb, nl);
    while (!src.exhausted()) src.more_into(nb, nl, 64u << 20);
    cur ^= 1;
    cursor = nl;
    *text = nb.data();
    *n_out = nl;
    return nl > 0;
}

}  // namespace cli
