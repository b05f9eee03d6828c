// test harness: the window pipeline of `merkurio extract` (merkurio_amd/csrc/cli/extract_windows.cpp: WindowExtract::prepare + run, with
// extract_sources.cpp, extract_window_call.cpp and extract_write.cpp) WITHOUT a device and without the library, --window-mb 1.  Built
// by g++ alone from those files and the readers; extract_device_text.cpp is left out and replaced by stubs:
//   take_on_device          answers "nothing": every input is host text (device_free_bytes: unknown)
//   mk_extract_window       joins head ++ text per source and indexes it with FastxFile::parse_span_partial; fills rec_start, n_window,
//                           n_used, n_tail, n_rec_seen and *n_rec (the smallest count over the sources) as the header's contract says,
//                           honours rec_cap and rows_cap with MK_E_CAPACITY and the stated need, and sets *status = 1 for a window in
//                           which a source holds a blank line (or anything the parser refuses).  Device-side outputs (tail, kept, all)
//                           and bodies (members, device text) are MK_E_INVALID_ARG: host text needs none of them
//   THE KEEP RULE           a record "hits" when the byte sum of its id (header line without marker and line end) is divisible by 3;
//                           a record (a pair: either mate) with a hit is kept, `invert` flips that -- nothing depends on where the
//                           windows are cut.  With logging: one row per kept record and source (pat 0, pos 0), in record order
//   mk_extract_single / _paired   (windows that reach host_window) see sequences only: a record hits when its first base is 'A'.  The
//                           test's inputs give exactly the records whose id hits a sequence that starts with 'A'
//   mk_host_alloc           malloc (the pool of staging buffers is used as it is); the rest are no-ops, the -z call is never reached
// usage: harness <out prefix> <handles> <flags: v = invert, l = text log, c = host_codec, - = none> <in1> [<in2>]
// writes <prefix>_1.out (_2.out) and <prefix>.log; prints "#window <n> heads <bytes> <bytes> by_host <0|1>" per window the stub answered
// (in call order), "#records <n>", and "#error <message>" with exit status 1 when the job raised one.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "extract_sources.hpp"
using namespace cli;

namespace cli {
namespace xw {
uint64_t device_free_bytes(int) { return 0; }
std::unique_ptr<Source> take_on_device(InputFile &, int, int, uint64_t, Gate &) { return nullptr; }
}  // namespace xw
}  // namespace cli

static std::mutex g_mu;
static unsigned long long g_windows = 0;

static bool id_hits(const char *p, size_t n) {
    unsigned s = 0;
    for (size_t k = 0; k < n; ++k) s += (unsigned char)p[k];
    return s % 3 == 0;
}

// keep[r] from hit(r, source), rows for the kept records; MK_E_CAPACITY with the need when the rows do not fit
template <class Hit>
static int keep_and_rows(uint64_t n, uint32_t n_sources, Hit hit, int logging, int invert, uint8_t *keep, mk_row *rows, uint64_t rows_cap,
                         uint64_t *n_rows, mk_counters *c, uint32_t *counts) {
    uint64_t kept = 0;
    for (uint64_t r = 0; r < n; ++r) {
        bool any = false;
        for (uint32_t i = 0; i < n_sources; ++i) any = any || hit(r, i);
        keep[r] = any != (invert != 0);
        kept += keep[r];
    }
    *n_rows = logging ? kept * n_sources : 0;
    if (*n_rows > rows_cap) return MK_E_CAPACITY;
    uint64_t q = 0;
    for (uint64_t r = 0; r < n && logging; ++r)
        for (uint32_t i = 0; i < n_sources && keep[r]; ++i) rows[q++] = mk_row{r, 0, 0, i, 0};
    c->nb_records_tot += n, c->nb_records_extracted += kept;
    counts[0] += (uint32_t)kept;
    return MK_OK;
}

extern "C" {
int mk_extract_window(mk_matcher *, mk_codec *, uint32_t format, uint32_t n_sources, mk_window_source *src, int logging, int invert, uint64_t rec_cap,
                      uint64_t *n_rec, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *c, uint32_t *counts,
                      uint32_t *status) {
    std::string text[2];
    FastxFile ff[2];
    uint64_t stop[2] = {0, 0}, n = ~0ull;
    bool refused = false;
    for (uint32_t i = 0; i < n_sources; ++i) {
        const mk_window_source &Q = src[i];
        if (Q.n_members || Q.n_device_text || Q.tail || Q.kept || Q.all || !Q.rec_start) return MK_E_INVALID_ARG;
        text[i].assign((const char *)Q.head, Q.n_head).append((const char *)Q.text, Q.n_text);
        const std::string &t = text[i];
        refused = refused || (!t.empty() && (t[0] == '\n' || t[0] == '\r')) || t.find("\n\n") != std::string::npos || t.find("\n\r") != std::string::npos;
        ff[i].fastq = format == MK_TEXT_FASTQ, ff[i].data = t.data(), ff[i].data_n = t.size();
        try {
            stop[i] = ff[i].parse_span_partial(0, t.size(), !Q.ends_at_record);
        } catch (const Error &) {
            refused = true;
        }
        n = std::min<uint64_t>(n, ff[i].recs.size());
    }
    *status = refused ? 1 : 0;
    if (!refused && n > rec_cap) {
        *n_rec = n;
        return MK_E_CAPACITY;
    }
    if (!refused) {
        for (uint32_t i = 0; i < n_sources; ++i) {
            mk_window_source &Q = src[i];
            for (uint64_t r = 0; r < n; ++r) Q.rec_start[r] = ff[i].recs[r].id_b - 1;
            Q.n_window = text[i].size(), Q.n_rec_seen = ff[i].recs.size();
            Q.n_used = Q.rec_start[n] = n < ff[i].recs.size() ? ff[i].recs[n].id_b - 1 : stop[i];
            Q.n_tail = Q.n_window - Q.n_used, Q.n_kept_bytes = 0;
        }
        *n_rec = n;
        auto hit = [&](uint64_t r, uint32_t i) { return id_hits(ff[i].data + ff[i].recs[r].id_b, ff[i].recs[r].id_e - ff[i].recs[r].id_b); };
        const int rc = keep_and_rows(n, n_sources, hit, logging, invert, keep, rows, rows_cap, n_rows, c, counts);
        if (rc != MK_OK) return rc;
    }
    std::lock_guard<std::mutex> lk(g_mu);
    printf("#window %llu heads %llu %llu by_host %d\n", g_windows++, (unsigned long long)src[0].n_head,
           (unsigned long long)(n_sources == 2 ? src[1].n_head : 0), refused ? 1 : 0);
    return MK_OK;
}
int mk_extract_single(mk_matcher *, const uint8_t *seq, const uint64_t *off, uint64_t n_rec, int logging, int invert, uint8_t *keep, mk_row *rows,
                      uint64_t rows_cap, uint64_t *n_rows, mk_counters *c, uint32_t *counts) {
    auto hit = [&](uint64_t r, uint32_t) { return off[r + 1] > off[r] && seq[off[r]] == 'A'; };
    return keep_and_rows(n_rec, 1, hit, logging, invert, keep, rows, rows_cap, n_rows, c, counts);
}
int mk_extract_paired(mk_matcher *, const uint8_t *seq1, const uint64_t *off1, uint64_t n_rec, const uint8_t *seq2, const uint64_t *off2, uint64_t,
                      int logging, int invert, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *c, uint32_t *counts) {
    auto hit = [&](uint64_t r, uint32_t i) { return i ? off2[r + 1] > off2[r] && seq2[off2[r]] == 'A' : off1[r + 1] > off1[r] && seq1[off1[r]] == 'A'; };
    return keep_and_rows(n_rec, 2, hit, logging, invert, keep, rows, rows_cap, n_rows, c, counts);
}
int mk_extract_window_members(mk_matcher *, mk_codec *, uint32_t, uint32_t, mk_window_source *, mk_window_members *, int, int, uint64_t, uint64_t *,
                              uint8_t *, mk_row *, uint64_t, uint64_t *, mk_counters *, uint32_t *, uint32_t *) {
    return MK_E_UNSUPPORTED;
}
int mk_upload_text_ahead(mk_matcher *, const uint8_t *, uint64_t) { return MK_OK; }
int mk_matcher_batch_times(const mk_matcher *, float ms[4]) {
    ms[0] = ms[1] = ms[2] = ms[3] = 0;
    return MK_OK;
}
int mk_codec_create(int, mk_codec **) { return MK_E_UNSUPPORTED; }
void mk_codec_destroy(mk_codec *) {}
int mk_codec_cut_times(const mk_codec *, uint64_t *, float *) { return MK_OK; }
int mk_host_alloc(size_t bytes, void **out) { return (*out = malloc(bytes)) ? MK_OK : MK_E_NOMEM; }
void mk_host_free(void *p) { free(p); }
const char *mk_last_error(void) { return "stub"; }
}

int main(int argc, char **argv) {
    if (argc != 5 && argc != 6) return 2;
    const std::string prefix = argv[1], flags = argv[3];
    const bool paired = argc == 6, log = flags.find('l') != std::string::npos;
    int rc = 0;
    Sink w1, w2;
    Loggers lg;
    try {
        ExtractArgs a;
        a.in_fastx = argv[4];
        if (paired) a.in_fastq_2 = std::string(argv[5]);
        a.window_mb = 1, a.window_mb_given = true;
        a.invert_match = flags.find('v') != std::string::npos;
        a.host_codec = flags.find('c') != std::string::npos;
        if (log) {
            a.out_log = prefix + ".log";
            lg.text.out.reset(new Sink);
            lg.text.out->open(*a.out_log);
            lg.active = true;
        }
        static char handles[8];  // (distinct dummy pointers: the stubs never look behind them)
        const size_t N = (size_t)std::max(1, std::min(8, atoi(argv[2])));
        std::vector<int> devs(N, 0);
        std::vector<mk_matcher *> ms;
        for (size_t d = 0; d < N; ++d) ms.push_back((mk_matcher *)&handles[d]);
        Patterns pats;
        pats.list = {"ACGT"};
        w1.open(prefix + "_1.out");
        if (paired) w2.open(prefix + "_2.out");
        std::vector<mk_counters> dev_c(N);
        for (auto &x : dev_c) memset(&x, 0, sizeof(x));
        std::vector<std::vector<uint32_t>> dev_counts(N, std::vector<uint32_t>(1, 0));
        PhaseTimer tm;
        tm.on = false;
        WindowExtract wx;
        if (!wx.prepare(a, devs)) {
            printf("#not for the window path\n");
            return 3;
        }
        try {
            wx.run(a, pats, lg, ms, devs, w1, w2, file_name(a.in_fastx), paired ? file_name(*a.in_fastq_2) : "", dev_c, dev_counts, tm);
        } catch (const Error &e) {
            printf("#error %s\n", e.what());
            rc = 1;
        }
        unsigned long long n = 0;
        for (auto &x : dev_c) n += x.nb_records_tot;
        printf("#records %llu\n", n);
    } catch (const Error &e) {
        printf("#error %s\n", e.what());
        rc = 1;
    }
    w1.flush(), w2.flush(), lg.text.flush();
    return rc;
}
