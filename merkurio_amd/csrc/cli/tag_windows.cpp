// tag_windows.cpp -- `merkurio tag` BAM -> BAM (or -S) with the records resident on the device (r05; SURVEY.md §8 rows a11 / f-3;
// the reader loop, process_record and the writer of src/cmd_tag.rs:503-615, :387-497, :254-271).
//
// The r04 path inflated a window of the BAM into host memory (device codec), indexed its record chain and un-nibbled the
// sequences on the host threads, sent those to the scan, appended the tags on the host threads and handed the records back to
// the device to be deflated: the text crossed the host boundary three times.  Here a window is the compressed members AS THEY ARE
// STORED: mk_tag_bam_window inflates them, indexes the records, unpacks, scans, tags and deflates on the device; what comes back
// is the window's last unfinished record (the next window's head), the log rows with their record names, and finished BGZF
// members that go to the file as they are.
//
// Two windows per device are in flight, each on a handle (and stream) of its own (--gpus N: consecutive windows on different devices): window k + 1 needs only the TAIL of window k -- known right
// after k's record index (mk_bam_window::on_tail) -- so its upload and inflate run beside k's scan, tag, deflate and download, and
// its members are copied into page-locked memory (a mapped file is not a DMA source) beside all of that.  Results are emitted in
// window order; the writer thread writes window k - 1 meanwhile.
//
// A window the device refuses -- a record that fails the parser's checks, optional fields that do not parse, a kept record whose
// field of the tag's name is not a plain string, a damaged member -- hands the input back to the host reader AT THAT WINDOW'S FIRST BYTE
// (SamFile::seek_bam): the r04 path takes the rest of the file and words the reference's errors.  (The window behind it may have
// been started already: its results are dropped.)
//
// Plain SAM text -> SAM text (or -S) goes the same way (tag_sam_windows_on_device, mk_tag_sam_window, sam.hip) without the codec and
// without the head chain: a window is a slice of the memory-mapped file cut at a line start (a '\n' can be found without reading the
// lines), so windows are INDEPENDENT; it is staged through a page-locked buffer and comes back as the kept lines with their tag field
// appended, written as they are.  A refused window (a line with fewer than 10 fields, a kept record whose field of the tag's name is
// not a plain string) hands the input back to the host loop at its first byte (SamFile::seek_text).
//
// Plain SAM text -> BAM (tag_sam_bam_windows_on_device, mk_tag_sam_bam_window) is the SAM driver's input side and the BAM driver's
// output side: the same independent windows, whose kept lines come back as BGZF members of BAM records (encoded on the device from
// the @SQ names the BamWriter's header was written from) and go to BamWriter::put_members.  On top of SAM -> SAM's refusals, a window
// with a kept line that BamWriter::encode_record would refuse, or whose numbers are not plain ones, is the host loop's.
//
// BAM -> SAM text / STDOUT (tag_bam_sam_windows_on_device, mk_tag_bam_sam_window) is the BAM driver's input side -- member windows, the
// head chain, two windows in flight per device -- and the SAM driver's output side: the kept records come back as finished SAM lines
// (formatted on the device from the reference names of the BAM header) in a page-locked buffer and go to the text writer in window
// order.  On top of BAM -> BAM's refusals, a window with a kept record that carries a float "%g" would write in exponent notation is
// the host loop's.
//
// Both formats share one driver (run_windows): the round-robin over the workers, the repeat of a call that asked for more room, the
// emit turn, refusal and error bookkeeping, counters and log rows.  BamWorker / SamWorker / SamBamWorker / BamSamWorker say how a window is staged, run and written.
#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>

#include "../../../include/merkurio_hip.h"
#include "commands.hpp"
#include "extract_common.hpp"
#include "io.hpp"

namespace cli {

namespace {

// members [m0, m1) of the file: their table re-based to the first one's DEFLATE stream, and that byte range of the file
struct WindowMembers {
    size_t m0 = 0, m1 = 0;
    uint64_t file_lo = 0, file_hi = 0, text = 0;
    std::vector<mk_bgzf_member> mem;
};

// file[lo, hi) -> dst on a few host threads (first touch of the mapping's pages included)
void copy_in(const uint8_t *file, uint64_t lo, uint64_t hi, uint8_t *dst) {
    const uint64_t n = hi - lo;
    const size_t T = std::max<size_t>(1, std::min<size_t>(std::max(1u, io_threads() / 2), (size_t)(n >> 22) + 1));
    run_threads(T, [&](size_t t) { memcpy(dst + n * t / T, file + lo + n * t / T, (size_t)(n * (t + 1) / T - n * t / T)); });
}

// what the workers share: whose turn it is to emit, and how the job ends early
struct Pipe {
    std::mutex mu;
    std::condition_variable cv;
    size_t emit_turn = 0;         // windows before this one have been emitted
    bool stop = false;            // a window was refused or failed: nothing further is emitted
    size_t refused = ~(size_t)0;  // the window the host reader takes over at
    std::string error;
    // BAM's head chain: window k + 1 starts with window k's tail, reported by the library as soon as it is known (on_tail)
    size_t heads_ready = 0;  // the head of window `heads_ready` is in `head` (windows before it have theirs already)
    std::vector<uint8_t> head;
    std::vector<uint8_t> refused_head;  // the head the refused window was given
};

// One worker per handle: window k runs on worker k mod n_workers (with the handles of several devices in a row, consecutive windows
// go to different devices).  `make(id)` gives worker id its format's state W: W.w is the library's window struct (tag and keep rule
// filled in here), W.load(k) puts window k's input where the device reads it (false: the job has been stopped), W.call(...) runs the
// window, W.grow() makes the room for tail and output that a call asked for, W.write() hands the output on, W.refused(k, rc, status)
// notes a window left to the host reader (pipe.mu held).  Results leave in window order, and after `stop` none do; a worker holds
// one finished window at most while it waits for its turn.  Ends with bail() on the first error.
template <class Make>
void run_windows(const TagArgs &a, Pipe &pipe, size_t n_win, size_t n_workers, const std::vector<TagHandle> &handles, Loggers &lg, const Patterns &pats,
                 const std::string &in_name, double (&t_dev)[8], Make make) {
    auto worker = [&](size_t id) {
        auto W = make(id);
        std::vector<uint8_t> names(1u << 16);
        std::vector<mk_row> rows(4096);
        std::vector<uint64_t> row_name(4096);
        mk_counters wc;
        std::vector<uint32_t> wcounts(lg.active ? pats.list.size() : 0, 0);
        for (size_t k = id; k < n_win; k += n_workers) {
            {
                std::lock_guard<std::mutex> lk(pipe.mu);
                if (pipe.stop) return;
            }
            auto &w = W.w;
            memset(&w, 0, sizeof(w));
            w.filter_matching = a.filter_matching, w.invert = a.invert_match;
            w.tag[0] = (uint8_t)a.tag[0], w.tag[1] = (uint8_t)a.tag[1];
            if (!W.load(k)) return;
            uint32_t status = 0;
            int rc;
            for (;;) {  // (a window that does not fit is done again with the sizes it asked for)
                memset(&wc, 0, sizeof(wc));
                std::fill(wcounts.begin(), wcounts.end(), 0);
                w.rows = rows.data(), w.rows_cap = rows.size(), w.row_name = row_name.data(), w.names = names.data(), w.names_cap = names.size();
                rc = W.call(lg.active, &wc, wcounts.data(), &status);
                if (rc != MK_E_CAPACITY) break;
                bool grew = W.grow();
                if (w.n_rows > rows.size()) rows.resize(w.n_rows), row_name.resize(w.n_rows), grew = true;
                if (w.n_names_bytes > names.size()) names.resize(w.n_names_bytes), grew = true;
                if (!grew) break;
            }
            const bool refused = (W.corrupt_is_refused && rc == MK_E_CORRUPT) || (rc == MK_OK && status != 0);
            std::string err;
            if (!refused && rc != MK_OK) err = std::string("Error during matching: ") + mk_last_error();
            // results leave in window order
            std::unique_lock<std::mutex> lk(pipe.mu);
            pipe.cv.wait(lk, [&] { return pipe.stop || pipe.emit_turn == k; });
            if (pipe.stop) return;  // (an earlier window ended the job: this one's results are dropped)
            if (refused || !err.empty()) {
                pipe.stop = true;
                if (refused) pipe.refused = k, W.refused(k, rc, status);
                else pipe.error = err;
                pipe.cv.notify_all();
                return;
            }
            lk.unlock();
            // (only the worker whose turn it is gets here: the counters of its device, the loggers and the output are its alone)
            add_counters(*handles[id].counters, wc);
            add_counts(*handles[id].pattern_counts, wcounts);
            for (int i = 0; i < 8; ++i) t_dev[i] += w.ms[i];
            std::string emit_err;
            try {
                if (lg.active)
                    emit_log_rows(
                        lg, pats, rows.data(), w.n_rows,
                        [&](const mk_row &r) {
                            const char *nm = (const char *)names.data() + row_name[&r - rows.data()];
                            return std::pair<const char *, size_t>(nm, strlen(nm));
                        },
                        [&](const mk_row &) -> const std::string & { return in_name; });
                W.write();
            } catch (const Error &e) {
                emit_err = e.what()[0] ? e.what() : "error";
            }
            lk.lock();
            if (!emit_err.empty()) pipe.stop = true, pipe.error = emit_err;
            pipe.emit_turn = k + 1;
            pipe.cv.notify_all();
            if (pipe.stop) return;
        }
    };
    // (a worker that throws must not leave the others waiting)
    run_threads(n_workers, [&](size_t id) {
        try {
            worker(id);
        } catch (const Error &e) {
            std::lock_guard<std::mutex> lk(pipe.mu);
            if (pipe.error.empty()) pipe.error = e.what()[0] ? e.what() : "error";
            pipe.stop = true;
            pipe.cv.notify_all();
        }
    });
    if (!pipe.error.empty()) bail(pipe.error);
}

// ---- BAM
struct TailCtx {
    Pipe *pipe;
    size_t k;
};

void on_tail(void *ctx, const uint8_t *tail, uint64_t n_tail) {
    TailCtx *t = (TailCtx *)ctx;
    std::lock_guard<std::mutex> lk(t->pipe->mu);
    if (t->pipe->heads_ready != t->k) return;  // (a call repeated with larger buffers reports its tail again)
    t->pipe->head.assign(tail, tail + n_tail);
    t->pipe->heads_ready = t->k + 1;
    t->pipe->cv.notify_all();
}

// (BAM-shaped text deflates to a third; a window that does not fit is done again with the size it asked for)
uint64_t out_guess(uint64_t text) { return text / 3 + (4u << 20); }

struct BamWorker {
    const std::vector<WindowMembers> &wins;
    const uint8_t *file;
    BamWriter *bw;
    Pipe &pipe;
    bool timing;
    mk_matcher *m;
    mk_codec *codec;
    HostBuffer stage, out;  // the window's members (page-locked); the members it turns into (moved to the writer)
    std::vector<uint8_t> tail = std::vector<uint8_t>(1u << 20), head;
    TailCtx tctx{};
    mk_bam_window w{};
    static constexpr bool corrupt_is_refused = true;  // (a damaged member)
    ~BamWorker() {
        if (!g_process_is_ending) mk_codec_destroy(codec);
    }
    bool load(size_t k) {
        const WindowMembers &X = wins[k];
        if (!X.mem.empty()) {
            if (!stage.grow(X.file_hi - X.file_lo, 1u << 20)) bail(std::string("Error during BAM record parsing: ") + mk_last_error());
            copy_in(file, X.file_lo, X.file_hi, stage.p);
        }
        if (bw && out.cap < out_guess(X.text + (1u << 20))) {
            out.reset();
            out = bw->take_raw_buffer(out_guess(X.text + (1u << 20)));
        }
        {
            std::unique_lock<std::mutex> lk(pipe.mu);
            pipe.cv.wait(lk, [&] { return pipe.stop || pipe.heads_ready >= k; });
            if (pipe.stop) return false;
            head = pipe.head;
        }
        tctx = TailCtx{&pipe, k};
        w.head = head.data(), w.n_head = head.size();
        w.bgzf = stage.p, w.n_bgzf = X.file_hi - X.file_lo;
        w.members = X.mem.data(), w.n_members = X.mem.size();
        w.last = k + 1 == wins.size();
        w.on_tail = on_tail, w.on_tail_ctx = &tctx;
        return true;
    }
    int call(int logging, mk_counters *wc, uint32_t *wcounts, uint32_t *status) {
        w.tail = tail.data(), w.tail_cap = tail.size();
        w.out = bw ? out.p : nullptr, w.out_cap = bw ? out.cap : 0;
        const int rc = mk_tag_bam_window(m, codec, &w, logging, wc, wcounts, status);
        if (rc == MK_OK && !*status) on_tail(&tctx, tail.data(), w.n_tail);  // (an empty window returns before the library reports it)
        return rc;
    }
    bool grow() {
        bool grew = false;
        if (w.n_tail > tail.size()) tail.resize(w.n_tail + (1u << 20)), grew = true;
        if (bw && w.out_len > out.cap) {
            out.reset();
            out = bw->take_raw_buffer(w.out_len);
            grew = true;
        }
        return grew;
    }
    void refused(size_t k, int rc, uint32_t status) {  // (the head the window was given, not the current one)
        pipe.refused_head = head;
        if (timing)
            fprintf(stderr, "[timing] window %llu left to the host reader (%s)\n", (unsigned long long)k,
                    rc == MK_E_CORRUPT ? "a damaged member"
                    : status & 1       ? "record chain"
                    : status & 2       ? "optional fields"
                    : status & 4       ? "existing tag"
                                       : "unfinished record");
    }
    void write() {
        if (bw && w.out_len) bw->put_members(std::move(out), w.out_len);
    }
};

// ---- SAM text: windows cut at line starts have no heads or tails and are independent
struct SamWorker {
    const std::vector<std::pair<uint64_t, uint64_t>> &wins;
    const uint8_t *file;
    Sink *out_sink;
    uint32_t &refused_status;
    mk_matcher *m;
    HostBuffer stage, out;  // the window's text; the kept lines (both page-locked)
    uint8_t no_tail[8];
    mk_sam_window w{};
    static constexpr bool corrupt_is_refused = false;
    bool load(size_t k) {
        const uint64_t b = wins[k].first, n = wins[k].second - wins[k].first;
        if (!stage.grow(n, 1u << 20)) bail(std::string("Error during SAM record parsing: ") + mk_last_error());
        copy_in(file, b, b + n, stage.p);
        // (a kept line grows by its tag field: a tenth of a 350-byte line per matched 31-mer; a window that does not fit is
        // done again with the size it asked for)
        if (out_sink && out.cap < n + n / 4 + (1u << 20) && !out.grow(n + n / 4 + (1u << 20), 1u << 20))
            bail(std::string("Error during SAM record parsing: ") + mk_last_error());
        w.text = stage.p, w.n_text = n;
        w.last = 1;  // (the window ends at a line end or at the end of the file: all of it is lines)
        return true;
    }
    int call(int logging, mk_counters *wc, uint32_t *wcounts, uint32_t *status) {
        w.tail = no_tail, w.tail_cap = sizeof(no_tail);
        w.out = out_sink ? out.p : nullptr, w.out_cap = out_sink ? out.cap : 0;
        return mk_tag_sam_window(m, &w, logging, wc, wcounts, status);
    }
    bool grow() {
        if (!out_sink || w.out_len <= out.cap) return false;
        if (!out.grow(w.out_len, 1u << 20)) bail(std::string("Error during SAM record parsing: ") + mk_last_error());
        return true;
    }
    void refused(size_t, int, uint32_t status) { refused_status = status; }
    void write() {
        if (out_sink && w.out_len) out_sink->write((const char *)out.p, w.out_len);
    }
};

// ---- SAM text -> BAM: SamWorker's windows, BamWorker's output
struct SamBamWorker {
    const std::vector<std::pair<uint64_t, uint64_t>> &wins;
    const uint8_t *file;
    BamWriter *bw;
    const std::vector<uint8_t> &ref_bytes;
    const std::vector<uint64_t> &ref_off;
    uint32_t &refused_status;
    mk_matcher *m;
    mk_codec *codec;
    HostBuffer stage, out;  // the window's text (page-locked); the members it turns into (moved to the writer)
    uint8_t no_tail[8];
    mk_sam_bam_window w{};
    static constexpr bool corrupt_is_refused = false;
    ~SamBamWorker() {
        if (!g_process_is_ending) mk_codec_destroy(codec);
    }
    bool load(size_t k) {
        const uint64_t b = wins[k].first, n = wins[k].second - wins[k].first;
        if (!stage.grow(n, 1u << 20)) bail(std::string("Error during SAM record parsing: ") + mk_last_error());
        copy_in(file, b, b + n, stage.p);
        // (a BAM record is shorter than its line, and BAM-shaped text deflates to a third)
        if (out.cap < out_guess(n)) {
            out.reset();
            out = bw->take_raw_buffer(out_guess(n));
        }
        w.text = stage.p, w.n_text = n;
        w.last = 1;  // (the window ends at a line end or at the end of the file: all of it is lines)
        w.ref_names = ref_bytes.data(), w.ref_off = ref_off.data(), w.n_refs = ref_off.size() - 1;
        return true;
    }
    int call(int logging, mk_counters *wc, uint32_t *wcounts, uint32_t *status) {
        w.tail = no_tail, w.tail_cap = sizeof(no_tail);
        w.out = out.p, w.out_cap = out.cap;
        return mk_tag_sam_bam_window(m, codec, &w, logging, wc, wcounts, status);
    }
    bool grow() {
        if (w.out_len <= out.cap) return false;
        out.reset();
        out = bw->take_raw_buffer(w.out_len);
        return true;
    }
    void refused(size_t, int, uint32_t status) { refused_status = status; }
    void write() {
        if (w.out_len) bw->put_members(std::move(out), w.out_len);
    }
};

// ---- BAM -> SAM text: BamWorker's windows, SamWorker's output
struct BamSamWorker {
    const std::vector<WindowMembers> &wins;
    const uint8_t *file;
    Sink *out_sink;
    const std::vector<uint8_t> &ref_bytes;
    const std::vector<uint64_t> &ref_off;
    Pipe &pipe;
    uint32_t &refused_status;
    int &refused_rc;
    bool all_kept;  // neither -m nor -v
    mk_matcher *m;
    mk_codec *codec;
    HostBuffer stage, out;  // the window's members; the kept lines (both page-locked)
    std::vector<uint8_t> tail = std::vector<uint8_t>(1u << 20), head;
    TailCtx tctx{};
    double ratio = 0;  // line bytes per byte of window text of this worker's previous window (0: none yet)
    mk_bam_sam_window w{};
    static constexpr bool corrupt_is_refused = true;  // (a damaged member)
    ~BamSamWorker() {
        if (!g_process_is_ending) mk_codec_destroy(codec);
    }
    // The first guess comes from the flags: with everything kept the lines take more than the window's text (SEQ doubles, the numbers
    // grow), with -m or -v what the k-mers select -- an eighth is a guess.  After that the previous window's ratio and a quarter: a
    // window that does not fit is done again with the size it asked for, which this keeps the exception.
    uint64_t out_room(uint64_t text) const {
        const double r = ratio > 0 ? ratio * 1.25 : all_kept ? 2.25 : 0.125;
        return (uint64_t)((double)text * r) + (1u << 20);
    }
    bool load(size_t k) {
        const WindowMembers &X = wins[k];
        if (!X.mem.empty()) {
            if (!stage.grow(X.file_hi - X.file_lo, 1u << 20)) bail(std::string("Error during BAM record parsing: ") + mk_last_error());
            copy_in(file, X.file_lo, X.file_hi, stage.p);
        }
        if (out.cap < out_room(X.text + (1u << 20)) && !out.grow(out_room(X.text + (1u << 20)), 1u << 20))
            bail(std::string("Error during BAM record parsing: ") + mk_last_error());
        {
            std::unique_lock<std::mutex> lk(pipe.mu);
            pipe.cv.wait(lk, [&] { return pipe.stop || pipe.heads_ready >= k; });
            if (pipe.stop) return false;
            head = pipe.head;
        }
        tctx = TailCtx{&pipe, k};
        w.head = head.data(), w.n_head = head.size();
        w.bgzf = stage.p, w.n_bgzf = X.file_hi - X.file_lo;
        w.members = X.mem.data(), w.n_members = X.mem.size();
        w.last = k + 1 == wins.size();
        w.ref_names = ref_bytes.data(), w.ref_off = ref_off.data(), w.n_refs = ref_off.size() - 1;
        w.on_tail = on_tail, w.on_tail_ctx = &tctx;
        return true;
    }
    int call(int logging, mk_counters *wc, uint32_t *wcounts, uint32_t *status) {
        w.tail = tail.data(), w.tail_cap = tail.size();
        w.out = out.p, w.out_cap = out.cap;
        const int rc = mk_tag_bam_sam_window(m, codec, &w, logging, wc, wcounts, status);
        if (rc == MK_OK && !*status) {
            on_tail(&tctx, tail.data(), w.n_tail);  // (an empty window returns before the library reports it)
            if (w.n_window) ratio = (double)w.out_len / (double)w.n_window;
        }
        return rc;
    }
    bool grow() {
        bool grew = false;
        if (w.n_tail > tail.size()) tail.resize(w.n_tail + (1u << 20)), grew = true;
        if (w.out_len > out.cap) {
            if (!out.grow(w.out_len, 1u << 20)) bail(std::string("Error during BAM record parsing: ") + mk_last_error());
            grew = true;
        }
        return grew;
    }
    void refused(size_t, int rc, uint32_t status) {  // (the head the window was given, not the current one)
        pipe.refused_head = head;
        refused_status = status, refused_rc = rc;
    }
    void write() {
        if (w.out_len) out_sink->write((const char *)out.p, w.out_len);
    }
};

// [b, e) per window, e = the first line start at or behind b + window_bytes
std::vector<std::pair<uint64_t, uint64_t>> cut_at_lines(const uint8_t *file, uint64_t from, uint64_t n_file, uint64_t window_bytes) {
    std::vector<std::pair<uint64_t, uint64_t>> wins;
    for (uint64_t b = from; b < n_file;) {
        uint64_t e = std::min(n_file, b + std::max<uint64_t>(window_bytes, 1));
        if (e < n_file) {
            const void *nl = memchr(file + e - 1, '\n', n_file - (e - 1));
            e = nl ? (uint64_t)((const uint8_t *)nl - file) + 1 : n_file;
        }
        wins.emplace_back(b, e);
        b = e;
    }
    return wins;
}

// the BAM windows of the rest of the file: runs of members of ~window_bytes of text (the same whatever the heads turn out to be);
// have_head: records behind the header that open() has inflated already -- a window of their own if no member follows
std::vector<WindowMembers> cut_at_members(const WindowSource &src, uint64_t window_bytes, bool have_head) {
    const size_t n_mem = src.n_bgzf_members();
    std::vector<WindowMembers> wins;
    for (size_t m0 = src.next_member(); m0 < n_mem;) {
        WindowMembers W;
        W.m0 = m0;
        size_t m1 = m0;
        while (m1 < n_mem && (W.text < window_bytes || m1 == m0)) {
            uint64_t off;
            uint32_t len, isize, crc;
            src.bgzf_member_at(m1, &off, &len, &isize, &crc);
            if (m1 == m0) W.file_lo = off;
            W.file_hi = off + len;
            W.mem.push_back(mk_bgzf_member{off - W.file_lo, W.text, len, isize, crc, 0});
            W.text += isize;
            ++m1;
        }
        W.m1 = m1;
        m0 = m1;
        wins.push_back(std::move(W));
    }
    if (wins.empty() && have_head) {
        WindowMembers W;
        W.m0 = W.m1 = n_mem;
        wins.push_back(std::move(W));
    }
    return wins;
}

}  // namespace

bool tag_bam_windows_on_device(const TagArgs &a, SamFile &sam, const std::vector<TagHandle> &handles, Loggers &lg, const Patterns &pats,
                               const std::string &in_name, BamWriter *bw, uint64_t window_bytes) {
    const WindowSource &src = sam.source();
    const uint8_t *file = src.file_bytes();
    const bool timing = getenv("MERKURIO_TIMING") != nullptr;
    uint64_t n_pending = 0;
    const char *pend = sam.bam_pending(&n_pending);
    Pipe pipe;
    pipe.head.assign(pend, pend + n_pending);
    const std::vector<WindowMembers> wins = cut_at_members(src, window_bytes, !pipe.head.empty());
    if (wins.empty()) return true;
    const size_t n_win = wins.size();
    // (window k runs on handle k mod n_workers: with the handles of several devices in a row, consecutive windows go to different devices)
    const size_t n_workers = std::max<size_t>(1, std::min<size_t>(handles.size(), n_win));
    double t_dev[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    run_windows(a, pipe, n_win, n_workers, handles, lg, pats, in_name, t_dev, [&](size_t id) {
        mk_codec *codec = nullptr;
        if (mk_codec_create(handles[id].device, &codec) != MK_OK) bail(std::string("Error during BAM record parsing: ") + mk_last_error());
        return BamWorker{wins, file, bw, pipe, timing, handles[id].m, codec};
    });
    if (timing)
        fprintf(stderr,
                "[timing] %llu of %llu windows on the device (%llu in flight): upload %.3f, inflate %.3f, record index %.3f, unpack + scan + sets %.3f, "
                "tag + pack %.3f, deflate %.3f, download %.3f s (of these, growing device buffers: %.3f s)\n",
                (unsigned long long)pipe.emit_turn, (unsigned long long)n_win, (unsigned long long)n_workers, t_dev[0] / 1e3, t_dev[1] / 1e3, t_dev[2] / 1e3,
                t_dev[3] / 1e3, t_dev[4] / 1e3, t_dev[5] / 1e3, t_dev[6] / 1e3, t_dev[7] / 1e3);
    if (pipe.refused != ~(size_t)0) {
        sam.seek_bam(wins[pipe.refused].m0, (const char *)pipe.refused_head.data(), pipe.refused_head.size());
        return false;
    }
    return true;
}

bool tag_sam_windows_on_device(const TagArgs &a, SamFile &sam, const std::vector<TagHandle> &handles, Loggers &lg, const Patterns &pats,
                               const std::string &in_name, Sink *out_sink, uint64_t window_bytes) {
    const WindowSource &src = sam.source();
    const uint8_t *file = (const uint8_t *)src.text();
    const uint64_t n_file = src.text_size();
    const bool timing = getenv("MERKURIO_TIMING") != nullptr;
    const std::vector<std::pair<uint64_t, uint64_t>> wins = cut_at_lines(file, sam.text_cursor(), n_file, window_bytes);
    if (wins.empty()) return true;
    const size_t n_win = wins.size();
    const size_t n_workers = std::max<size_t>(1, std::min<size_t>(handles.size(), n_win));
    Pipe pipe;
    uint32_t refused_status = 0;
    double t_dev[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    run_windows(a, pipe, n_win, n_workers, handles, lg, pats, in_name, t_dev,
                [&](size_t id) { return SamWorker{wins, file, out_sink, refused_status, handles[id].m}; });
    if (timing) {
        fprintf(stderr,
                "[timing] %llu of %llu SAM text windows on the device (%llu in flight): upload %.3f, line index + fields %.3f, gather + scan + sets %.3f, "
                "tag + emit %.3f, download %.3f s (of these, growing device buffers: %.3f s)\n",
                (unsigned long long)pipe.emit_turn, (unsigned long long)n_win, (unsigned long long)n_workers, t_dev[0] / 1e3, t_dev[1] / 1e3, t_dev[2] / 1e3,
                t_dev[3] / 1e3, t_dev[4] / 1e3, t_dev[7] / 1e3);
        if (pipe.refused != ~(size_t)0)
            fprintf(stderr, "[timing] window %llu left to the host reader (%s)\n", (unsigned long long)pipe.refused,
                    refused_status & 1 ? "a line with too few fields" : "existing tag");
    }
    if (pipe.refused != ~(size_t)0) {
        sam.seek_text(wins[pipe.refused].first);
        return false;
    }
    sam.seek_text(n_file);
    return true;
}

bool tag_sam_bam_windows_on_device(const TagArgs &a, SamFile &sam, const std::vector<TagHandle> &handles, Loggers &lg, const Patterns &pats,
                                   const std::string &in_name, BamWriter &bw, uint64_t window_bytes) {
    const WindowSource &src = sam.source();
    const uint8_t *file = (const uint8_t *)src.text();
    const uint64_t n_file = src.text_size();
    const bool timing = getenv("MERKURIO_TIMING") != nullptr;
    const std::vector<std::pair<uint64_t, uint64_t>> wins = cut_at_lines(file, sam.text_cursor(), n_file, window_bytes);
    if (wins.empty()) return true;
    // the reference names the writer's header holds, in its order: what encode_record looks RNAME and RNEXT up in
    std::vector<uint8_t> ref_bytes;
    std::vector<uint64_t> ref_off(1, 0);
    for (const std::string &nm : bw.ref_names) {
        ref_bytes.insert(ref_bytes.end(), nm.begin(), nm.end());
        ref_off.push_back(ref_bytes.size());
    }
    ref_bytes.push_back(0);  // (never empty: a pointer to hand over)
    const size_t n_win = wins.size();
    const size_t n_workers = std::max<size_t>(1, std::min<size_t>(handles.size(), n_win));
    Pipe pipe;
    uint32_t refused_status = 0;
    double t_dev[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    run_windows(a, pipe, n_win, n_workers, handles, lg, pats, in_name, t_dev, [&](size_t id) {
        mk_codec *codec = nullptr;
        if (mk_codec_create(handles[id].device, &codec) != MK_OK) bail(std::string("Error during SAM record parsing: ") + mk_last_error());
        return SamBamWorker{wins, file, &bw, ref_bytes, ref_off, refused_status, handles[id].m, codec};
    });
    if (timing) {
        fprintf(stderr,
                "[timing] %llu of %llu SAM text -> BAM windows on the device (%llu in flight): upload %.3f, line index + fields %.3f, gather + scan + sets "
                "%.3f, tag + encode %.3f, deflate %.3f, download %.3f s (of these, growing device buffers: %.3f s)\n",
                (unsigned long long)pipe.emit_turn, (unsigned long long)n_win, (unsigned long long)n_workers, t_dev[0] / 1e3, t_dev[1] / 1e3, t_dev[2] / 1e3,
                t_dev[3] / 1e3, t_dev[4] / 1e3, t_dev[5] / 1e3, t_dev[7] / 1e3);
        if (pipe.refused != ~(size_t)0)
            fprintf(stderr, "[timing] window %llu left to the host loop (%s)\n", (unsigned long long)pipe.refused,
                    refused_status & 1   ? "a line with too few fields"
                    : refused_status & 2 ? "a record the device does not encode"
                                         : "existing tag");
    }
    if (pipe.refused != ~(size_t)0) {
        sam.seek_text(wins[pipe.refused].first);
        return false;
    }
    sam.seek_text(n_file);
    return true;
}

bool tag_bam_sam_windows_on_device(const TagArgs &a, SamFile &sam, const std::vector<TagHandle> &handles, Loggers &lg, const Patterns &pats,
                                   const std::string &in_name, Sink &out_sink, uint64_t window_bytes) {
    const WindowSource &src = sam.source();
    const uint8_t *file = src.file_bytes();
    const bool timing = getenv("MERKURIO_TIMING") != nullptr;
    uint64_t n_pending = 0;
    const char *pend = sam.bam_pending(&n_pending);
    Pipe pipe;
    pipe.head.assign(pend, pend + n_pending);
    const std::vector<WindowMembers> wins = cut_at_members(src, window_bytes, !pipe.head.empty());
    if (wins.empty()) return true;
    // the reference names of the input's binary header, in its order: what RNAME and RNEXT are printed from
    std::vector<uint8_t> ref_bytes;
    std::vector<uint64_t> ref_off(1, 0);
    for (const std::string &nm : sam.ref_names) {
        ref_bytes.insert(ref_bytes.end(), nm.begin(), nm.end());
        ref_off.push_back(ref_bytes.size());
    }
    ref_bytes.push_back(0);  // (never empty: a pointer to hand over)
    const size_t n_win = wins.size();
    const size_t n_workers = std::max<size_t>(1, std::min<size_t>(handles.size(), n_win));
    uint32_t refused_status = 0;
    int refused_rc = MK_OK;
    double t_dev[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    run_windows(a, pipe, n_win, n_workers, handles, lg, pats, in_name, t_dev, [&](size_t id) {
        mk_codec *codec = nullptr;
        if (mk_codec_create(handles[id].device, &codec) != MK_OK) bail(std::string("Error during BAM record parsing: ") + mk_last_error());
        return BamSamWorker{wins, file, &out_sink, ref_bytes, ref_off, pipe, refused_status, refused_rc, !a.filter_matching && !a.invert_match,
                            handles[id].m, codec};
    });
    if (timing) {
        fprintf(stderr,
                "[timing] %llu of %llu BAM -> SAM text windows on the device (%llu in flight): upload %.3f, inflate %.3f, record index %.3f, unpack + scan + "
                "sets %.3f, tag + format %.3f, download %.3f s (of these, growing device buffers: %.3f s)\n",
                (unsigned long long)pipe.emit_turn, (unsigned long long)n_win, (unsigned long long)n_workers, t_dev[0] / 1e3, t_dev[1] / 1e3, t_dev[2] / 1e3,
                t_dev[3] / 1e3, t_dev[4] / 1e3, t_dev[5] / 1e3, t_dev[7] / 1e3);
        if (pipe.refused != ~(size_t)0)
            fprintf(stderr, "[timing] window %llu left to the host loop (%s)\n", (unsigned long long)pipe.refused,
                    refused_rc == MK_E_CORRUPT ? "a damaged member"
                    : refused_status & 1       ? "record chain"
                    : refused_status & 2       ? "a record the device does not format"
                    : refused_status & 4       ? "existing tag"
                                               : "unfinished record");
    }
    if (pipe.refused != ~(size_t)0) {
        sam.seek_bam(wins[pipe.refused].m0, (const char *)pipe.refused_head.data(), pipe.refused_head.size());
        return false;
    }
    return true;
}

}  // namespace cli
