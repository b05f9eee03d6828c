// test harness: `merkurio extract --open-windows` (merkurio_amd/csrc/cli/extract_windows.cpp: the reader that does not wait for tails, the
// device threads, the writer's seam and re-run steps) on ONE bgzip'ed FASTQ input WITHOUT a device and without the library, --window-mb 1.
// Built by g++ alone (ASan + UBSan) from the four stage files and the readers; the library's calls are stubs:
//   mk_extract_window       head ++ body (plain text, or BGZF members inflated by zlib) indexed with FastxFile::parse_span_partial; fills
//                           rec_start, n_window, n_used, n_tail, n_rec_seen, the tail and the kept records' text under the header's
//                           capacity protocol; *status = 1 for a text the parser refuses
//   mk_extract_window_open  the same behind a start that the stub NAMES, by OPEN_GUESS -- the seam and ordering logic is under test here,
//                           not the start rule.  The inputs' header lines begin "@r", their quality lines "@F", and a quality line has
//                           the record shape (tests/open_start.py: adversarial), so a false guess parses:
//                             true   the first line >= 1 that begins "@r"        false   the first line >= 1 that begins "@F"
//                             mix    one or the other by the window's first member (the same choice whatever thread asks)
//                           no such line: *status = 2
//   THE KEEP RULE           a record is kept when the second byte of its sequence is 'A' (window calls and mk_extract_single alike)
//   OPEN_FAIL_SEAM=n        the n-th seam call (an ordinary call with a head and a plain-text body) fails with MK_E_HIP
//   OPEN_SLOW=1             open calls of even windows sleep 30 ms: windows finish out of order
// usage: harness <out prefix> <handles> <flags: o = --open-windows, l = text log, - = none> <in.fastq.gz>
// writes <prefix>_1.out and <prefix>.log; prints "#call <open|seam|plain> head <bytes> status <s>" per window call, "#records <n>", and
// "#error <message>" with exit status 1 when the job raised one.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "bgzf_in.hpp"
#include "extract_sources.hpp"
using namespace cli;

namespace cli {
namespace xw {
uint64_t device_free_bytes(int) { return 0; }
std::unique_ptr<Source> take_on_device(InputFile &, int, int, uint64_t, Gate &) { return nullptr; }
}  // namespace xw
}  // namespace cli

static std::mutex g_mu;
static int g_seams = 0;

static int answer(uint32_t format, mk_window_source &Q, mk_window_front *F, int logging, int invert, uint64_t rec_cap, uint64_t *n_rec, uint8_t *keep,
                  mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *c, uint32_t *counts, uint32_t *status) {
    std::string t((const char *)Q.head, Q.n_head);
    if (Q.n_members) {
        uint64_t body = 0;
        for (uint64_t i = 0; i < Q.n_members; ++i) body += Q.members[i].isize;
        const size_t at = t.size();
        t.resize(at + body);
        inflate_bgzf_members_host(Q.bgzf, Q.members, Q.n_members, &t[at], "stub");
    } else {
        t.append((const char *)Q.text, Q.n_text);
    }
    const bool seam = !F && Q.n_head && Q.n_text && !Q.n_members;
    auto say = [&](uint32_t st) {
        std::lock_guard<std::mutex> lk(g_mu);
        printf("#call %s head %llu status %u\n", F ? "open" : seam ? "seam" : "plain", (unsigned long long)Q.n_head, st);
    };
    if (seam) {
        std::lock_guard<std::mutex> lk(g_mu);
        const char *f = getenv("OPEN_FAIL_SEAM");
        if (f && ++g_seams == atoi(f)) return MK_E_HIP;
    }
    *n_rec = 0, *status = 0, *n_rows = 0;
    Q.n_window = t.size(), Q.n_used = Q.n_tail = Q.n_kept_bytes = Q.n_rec_seen = 0;
    uint64_t from = 0;
    if (F) {
        const char *g = getenv("OPEN_GUESS");
        const std::string mode = g ? g : "true";
        const uint64_t first = Q.n_members ? Q.members[0].data_off : 0;
        if (getenv("OPEN_SLOW") && (first >> 3) % 2 == 0) std::this_thread::sleep_for(std::chrono::milliseconds(30));
        const bool want_true = mode == "true" || (mode == "mix" && (first >> 4) % 2 == 0);
        const char *mark = want_true ? "\n@r" : "\n@F";
        const size_t p = t.find(mark);
        if (p == std::string::npos) {
            *status = 2, F->n_front = t.size();
            say(2);
            return MK_OK;
        }
        from = p + 1;
        F->n_front = from;
    }
    FastxFile ff;
    ff.fastq = format == MK_TEXT_FASTQ, ff.data = t.data(), ff.data_n = t.size();
    uint64_t stop = 0;
    try {
        stop = ff.parse_span_partial(from, t.size(), !Q.ends_at_record);
    } catch (const Error &) {
        *status = 1;
        say(1);
        return MK_OK;
    }
    const uint64_t n = ff.recs.size();
    *n_rec = n;
    if (n > rec_cap) return MK_E_CAPACITY;
    if (F && F->n_front > F->front_cap) return MK_E_CAPACITY;
    if (F) memcpy(F->front, t.data(), (size_t)from);
    for (uint64_t r = 0; r < n; ++r) Q.rec_start[r] = ff.recs[r].id_b - 1;
    Q.n_rec_seen = n;
    Q.n_used = Q.rec_start[n] = stop;  // (a window that ends at a record end: all of it, if it is whole records)
    Q.n_tail = Q.n_window - Q.n_used;
    if (Q.tail || Q.tail_cap) {
        if (Q.n_tail > Q.tail_cap) return MK_E_CAPACITY;
        memcpy(Q.tail, t.data() + Q.n_used, (size_t)Q.n_tail);
    }
    if (Q.all) {
        if (Q.n_window > Q.all_cap) return MK_E_CAPACITY;
        memcpy(Q.all, t.data(), t.size());
    }
    uint64_t kept = 0, kept_bytes = 0;
    for (uint64_t r = 0; r < n; ++r) {
        const FastxFile::Rec &R = ff.recs[r];
        const bool hit = R.raw_e - R.raw_b >= 2 && t[R.raw_b + 1] == 'A';
        keep[r] = hit != (invert != 0);
        kept += keep[r];
        if (keep[r]) kept_bytes += Q.rec_start[r + 1] - Q.rec_start[r];
    }
    if (Q.kept || Q.kept_cap) {
        Q.n_kept_bytes = kept_bytes;
        if (kept_bytes > Q.kept_cap) return MK_E_CAPACITY;
        uint64_t at = 0;
        for (uint64_t r = 0; r < n; ++r)
            if (keep[r]) memcpy(Q.kept + at, t.data() + Q.rec_start[r], (size_t)(Q.rec_start[r + 1] - Q.rec_start[r])), at += Q.rec_start[r + 1] - Q.rec_start[r];
    }
    *n_rows = logging ? kept : 0;
    if (*n_rows > rows_cap) return MK_E_CAPACITY;
    uint64_t q = 0;
    for (uint64_t r = 0; r < n && logging; ++r)
        if (keep[r]) rows[q++] = mk_row{r, 0, 0, 0, 0};
    c->nb_records_tot += n, c->nb_records_extracted += kept;
    counts[0] += (uint32_t)kept;
    say(0);
    return MK_OK;
}

extern "C" {
int mk_extract_window(mk_matcher *, mk_codec *, uint32_t format, uint32_t n_sources, mk_window_source *src, int logging, int invert, uint64_t rec_cap,
                      uint64_t *n_rec, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *c, uint32_t *counts,
                      uint32_t *status) {
    if (n_sources != 1) return MK_E_INVALID_ARG;
    return answer(format, src[0], nullptr, logging, invert, rec_cap, n_rec, keep, rows, rows_cap, n_rows, c, counts, status);
}
int mk_extract_window_open(mk_matcher *, mk_codec *, uint32_t format, uint32_t n_sources, mk_window_source *src, int logging, int invert, uint64_t rec_cap,
                           uint64_t *n_rec, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *c, uint32_t *counts,
                           uint32_t *status, mk_window_front *fronts) {
    if (n_sources != 1 || src[0].n_head || !fronts) return MK_E_INVALID_ARG;
    return answer(format, src[0], fronts, logging, invert, rec_cap, n_rec, keep, rows, rows_cap, n_rows, c, counts, status);
}
int mk_extract_single(mk_matcher *, const uint8_t *seq, const uint64_t *off, uint64_t n_rec, int logging, int invert, uint8_t *keep, mk_row *rows,
                      uint64_t rows_cap, uint64_t *n_rows, mk_counters *c, uint32_t *counts) {
    uint64_t kept = 0;
    for (uint64_t r = 0; r < n_rec; ++r) keep[r] = (off[r + 1] - off[r] >= 2 && seq[off[r] + 1] == 'A') != (invert != 0), kept += keep[r];
    *n_rows = logging ? kept : 0;
    if (*n_rows > rows_cap) return MK_E_CAPACITY;
    uint64_t q = 0;
    for (uint64_t r = 0; r < n_rec && logging; ++r)
        if (keep[r]) rows[q++] = mk_row{r, 0, 0, 0, 0};
    c->nb_records_tot += n_rec, c->nb_records_extracted += kept;
    counts[0] += (uint32_t)kept;
    return MK_OK;
}
int mk_extract_paired(mk_matcher *, const uint8_t *, const uint64_t *, uint64_t, const uint8_t *, const uint64_t *, uint64_t, int, int, uint8_t *, mk_row *,
                      uint64_t, uint64_t *, mk_counters *, uint32_t *) {
    return MK_E_UNSUPPORTED;
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
static char g_codec;
int mk_codec_create(int, mk_codec **out) {
    *out = (mk_codec *)&g_codec;  // (a dummy: the stubs never look behind it)
    return MK_OK;
}
void mk_codec_destroy(mk_codec *) {}
int mk_codec_cut_times(const mk_codec *, uint64_t *, float *) { return MK_OK; }
int mk_host_alloc(size_t bytes, void **out) { return (*out = malloc(bytes)) ? MK_OK : MK_E_NOMEM; }
void mk_host_free(void *p) { free(p); }
const char *mk_last_error(void) { return "stub"; }
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const std::string prefix = argv[1], flags = argv[3];
    const bool log = flags.find('l') != std::string::npos;
    int rc = 0;
    Sink w1, w2;
    Loggers lg;
    try {
        ExtractArgs a;
        a.in_fastx = argv[4];
        a.window_mb = 1, a.window_mb_given = true;
        a.open_windows = flags.find('o') != std::string::npos;
        if (log) {
            a.out_log = prefix + ".log";
            lg.text.out.reset(new Sink);
            lg.text.out->open(*a.out_log);
            lg.active = true;
        }
        static char handles[8];
        const size_t N = (size_t)std::max(1, std::min(8, atoi(argv[2])));
        std::vector<int> devs(N, 0);
        std::vector<mk_matcher *> ms;
        for (size_t d = 0; d < N; ++d) ms.push_back((mk_matcher *)&handles[d]);
        Patterns pats;
        pats.list = {"ACGT"};
        w1.open(prefix + "_1.out");
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
            wx.run(a, pats, lg, ms, devs, w1, w2, file_name(a.in_fastx), "", dev_c, dev_counts, tm);
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
