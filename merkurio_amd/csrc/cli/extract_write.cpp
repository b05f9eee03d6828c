// extract_write.cpp -- the writer of the extract window driver: a finished window's log rows (reference emission order) and its kept
// records, from whichever text came back for it -- the host parser's records, packed kept records, the whole window, or (-z) BGZF
// members / written text with the ids beside them.  Owns the kept-record formatter.
#include "extract_windows.hpp"

namespace cli {

using Side = xw::Side;
using Win = xw::Win;
using Layout = xw::Side::Result::Layout;

namespace {

struct Span {  // where a record of a device-indexed side lies: (text piece, its size, begin, end)
    const char *p;
    uint64_t n, b, e;
};

// A kept record in the form the reference writes: record.write(_, None) re-emits the lines (FASTQ: with a bare '+') -- a record that is
// stored that way already (and ends in its line end) is written as one piece
void append_written(std::string &o, const Span &sp, bool fastq, FastxFile &one) {
    one.data = sp.p;
    one.data_n = sp.n;
    one.recs.clear();
    one.parse_span(sp.b, sp.e);
    if (one.recs.size() != 1) bail("Error during matching: the device's record table and the host parser disagree");
    const FastxFile::Rec &rec = one.recs[0];
    const bool crlf = rec.id_e < sp.n && sp.p[rec.id_e] == '\r';
    const uint64_t nl = crlf ? 2 : 1;
    const bool verbatim = sp.p[sp.e - 1] == '\n' && (fastq ? (rec.qual_b == rec.raw_e + 2 * nl + 1 && rec.qual_e + nl == sp.e)
                                                           : (rec.raw_e + nl == sp.e && rec.raw_b == rec.id_e + nl));
    if (verbatim) {
        o.append(sp.p + sp.b, (size_t)(sp.e - sp.b));
        return;
    }
    const char *eol = crlf ? "\r\n" : "\n";  // (FastxFile::write, into the buffer)
    o.append(fastq ? "@" : ">", 1).append(sp.p + rec.id_b, (size_t)(rec.id_e - rec.id_b)).append(eol, nl);
    o.append(sp.p + rec.raw_b, (size_t)(rec.raw_e - rec.raw_b)).append(eol, nl);
    if (fastq) o.append("+", 1).append(eol, nl).append(sp.p + rec.qual_b, (size_t)(rec.qual_e - rec.qual_b)).append(eol, nl);
}

}  // namespace

void WindowExtract::Impl::write_window(Win &W, Sink &w1, Sink &w2, const std::string &name1, const std::string &name2, PhaseTimer &tm) {
    Sink *w[2] = {&w1, &w2};
    const std::string *names[2] = {&name1, &name2};
    auto file_of = [&](const mk_row &r) -> const std::string & { return *names[r.file]; };
    if (W.by_host) {
        emit_log_rows(
            *lg, *pats, W.rows.data(), lg->active ? W.n_rows : 0,
            [&](const mk_row &r) {
                const FastxFile &ff = W.side[r.file].out.parsed;
                const auto &rec = ff.recs[r.rec];
                return std::pair<const char *, size_t>(ff.data + rec.id_b, rec.id_e - rec.id_b);
            },
            file_of);
        if (!a.suppress_output)
            for (uint64_t r : W.kept)
                for (int i = 0; i < n_in; ++i) W.side[i].out.parsed.write(r, *w[i]), w[i]->end_record();
        return;
    }
    if (W.side[0].out.layout == Layout::MEMBERS || W.side[0].out.layout == Layout::WRITTEN) return write_members_window(W, w, names, tm);
    // record r of side i in the text the writer holds: its own table for packed kept records
    std::vector<uint64_t> packed_start[2];
    for (int i = 0; i < n_in; ++i) {
        const Side::Result &R = W.side[i].out;
        if (R.layout != Layout::PACKED_KEPT) continue;
        uint64_t at = 0;
        for (uint64_t r : W.kept) {
            packed_start[i].push_back(at);
            at += R.rec_start[r + 1] - R.rec_start[r];
        }
        packed_start[i].push_back(at);
        if (at != R.text.size()) bail("Error during matching: the kept records' text does not have the size of its record table");
    }
    auto record_span = [&](int i, uint64_t r) -> Span {
        const Side::Result &R = W.side[i].out;
        if (R.layout == Layout::HEAD_BODY) bail("Error during matching: a window reached the writer without its text");
        if (R.layout == Layout::PACKED_KEPT) {
            const size_t q = (size_t)(std::lower_bound(W.kept.begin(), W.kept.end(), r) - W.kept.begin());
            if (q >= W.kept.size() || W.kept[q] != r) bail("Error during matching: a log row names a record whose text did not come back");
            return Span{R.text.data(), R.text.size(), packed_start[i][q], packed_start[i][q + 1]};
        }
        return Span{R.text.data(), R.text.size(), R.rec_start[r], R.rec_start[r + 1]};
    };
    // id of a record: its header line without the marker and the line end
    auto id_of = [&](const mk_row &row) {
        const Span sp = record_span((int)row.file, row.rec);
        const uint64_t b = sp.b + 1;
        const char *nl = (const char *)memchr(sp.p + b, '\n', (size_t)(sp.e - b));
        uint64_t e = nl ? (uint64_t)(nl - sp.p) : sp.e;
        if (e > b && sp.p[e - 1] == '\r') --e;
        return std::pair<const char *, size_t>(sp.p + b, (size_t)(e - b));
    };
    emit_log_rows(*lg, *pats, W.rows.data(), lg->active ? W.n_rows : 0, id_of, file_of);
    tm.mark("window: log rows");
    if (!a.suppress_output) {
        // kept records are written by the host reader's own code from the record's lines -- formatted by the host threads into
        // one buffer per thread and input, written in order (a window of 2 x 128 MB holds ~8 000 kept records at the usual 1 %,
        // a window of extracted reads 800 000)
        const std::vector<uint64_t> &kept = W.kept;
        const size_t T = std::max<size_t>(1, std::min<size_t>(io_threads(), kept.size() / 1024));
        std::vector<std::string> out[2];
        std::vector<std::vector<uint64_t>> out_ends[2];  // (-z: where every record ends in its buffer)
        const bool mark_ends = w[0]->z_ends != nullptr;
        for (int i = 0; i < 2; ++i) out[i].resize(T), out_ends[i].resize(T);
        run_threads(T, [&](size_t t) {
            FastxFile one;
            one.fastq = fastq;
            for (size_t q = kept.size() * t / T; q < kept.size() * (t + 1) / T; ++q)
                for (int i = 0; i < n_in; ++i) {
                    append_written(out[i][t], record_span(i, kept[q]), fastq, one);
                    if (mark_ends) out_ends[i][t].push_back(out[i][t].size());
                }
        });
        for (size_t t = 0; t < T; ++t)
            for (int i = 0; i < n_in; ++i) w[i]->write_records(out[i][t], out_ends[i][t]);
    }
    tm.mark("window: records out");
}

// a window of the -z member path (--zstd-output: frames): log rows from the packed ids, then per output the members as they are, or -- a window below
// --z-members-from -- the written text, which gathers with its neighbours' as the host writer's would (its record ends are found
// again: every fourth line end of FASTQ, every header line of FASTA)
void WindowExtract::Impl::write_members_window(Win &W, Sink **w, const std::string **names, PhaseTimer &tm) {
    auto id_of = [&](const mk_row &row) {
        const Side::Result &R = W.side[row.file].out;
        const size_t q = (size_t)(std::lower_bound(W.kept.begin(), W.kept.end(), row.rec) - W.kept.begin());
        if (q >= R.id_end.size() || W.kept[q] != row.rec) bail("Error during matching: a log row names a record whose id did not come back");
        const uint64_t b = q ? R.id_end[q - 1] : 0;
        return std::pair<const char *, size_t>(R.ids.data() + b, (size_t)(R.id_end[q] - b));
    };
    emit_log_rows(*lg, *pats, W.rows.data(), lg->active ? W.n_rows : 0, id_of, [&](const mk_row &r) -> const std::string & { return *names[r.file]; });
    tm.mark("window: log rows");
    bool any_members = false;
    for (int i = 0; i < n_in; ++i) {
        Side::Result &R = W.side[i].out;
        if (R.layout == Layout::MEMBERS) {
            any_members = true;
            if (!R.text.empty()) w[i]->put_members((const uint8_t *)R.text.data(), R.text.size(), R.n_members);
            continue;
        }
        std::vector<uint64_t> ends;
        const char *p = R.text.data();
        const uint64_t n = R.text.size();
        uint64_t lines = 0;
        for (const char *q = p; q < p + n && (q = (const char *)memchr(q, '\n', (size_t)(p + n - q))); ++q) {
            const uint64_t at = (uint64_t)(q - p) + 1;
            if (fastq ? (++lines % 4 == 0) : (at == n || p[at] == '>')) ends.push_back(at);
        }
        if (n) w[i]->write_records(std::string(p, (size_t)n), ends);
    }
    (any_members ? z_member_windows : z_text_windows) += 1;
    for (int k = 0; k < 4; ++k) z_ms[k] += W.z_ms[k];
    tm.mark("window: records out");
}

}  // namespace cli
