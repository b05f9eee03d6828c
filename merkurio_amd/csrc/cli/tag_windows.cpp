// tag_windows.cpp -- `merkurio tag` with the records resident on the device, in all four directions (r05; SURVEY.md §8 rows a11 / f-3;
// the reader loop, process_record and the writers of src/cmd_tag.rs:503-615, :387-497, :254-271).  A direction is one of two input
// sides followed by one of two output sides; the library's entry point in between (mk_tag_bam_window, mk_tag_sam_window,
// mk_tag_sam_bam_window, mk_tag_bam_sam_window) inflates or uploads, indexes the records, scans, tags and encodes on the device, so the
// text crosses the host boundary once in each direction at most, and what comes back goes to the file as it is.  All four share one driver:
// tag_windows cuts the windows, packs the reference names and makes a Worker<input, output, window struct> per handle; run_windows is
// the round-robin over the workers, the repeat of a call that asked for more room, the emit turn (results leave in window order; the
// writer thread writes window k - 1 meanwhile), the host turn of a refused window, error bookkeeping, counters and log rows.
//
// A WINDOW THE DEVICE REFUSES IS THE HOST LOOP'S, AND ONLY THAT WINDOW: when its emit turn comes, the reader is given the window's
// bounds and the host loop (tag_host.cpp: the code of --host-ingest) runs over them with the worker's own handle; its output, counters
// and log rows land where the window's would have, and the windows behind it stay on the device.  After kRefusedInARow = 4 refused
// windows in a row the last of them gets no turn: the reader is put at its first byte and the host loop keeps the rest of the file.
//
// MemberInput (BAM): a window is a run of BGZF members AS THEY ARE STORED, copied into page-locked memory (a mapped file is not a DMA
// source), behind a head: window k + 1 starts with the unfinished record window k ended with -- its TAIL, known right after k's record
// index (on_tail).  Two windows per device are in flight, each on a handle (and stream) of its own (--gpus N: consecutive windows on
// different devices), so k + 1's staging, upload and inflate run beside k's scan, tag and output.  A window the device refuses -- a
// record that fails the parser's checks, optional fields that do not parse, a kept record whose field of the tag's name is not a plain
// string, a damaged member -- is read by the host loop from the head it was given to the record that crosses its end (SamFile::seek_bam
// with an end member).  Window k + 1 never starts before its head is known: from on_tail, or, where window k was refused before its
// record index, from the bytes window k's host turn stopped in front of.  So a window behind a refused one always ran with its true
// head and stands.
//
// LineInput (plain SAM text): a window is a slice of the memory-mapped file cut at a line start (a '\n' can be found without reading
// the lines), staged through a page-locked buffer: no heads or tails, the windows are INDEPENDENT.  A refused window (a line with fewer
// than 10 fields, a kept record whose field of the tag's name is not a plain string) is [wins[k].first, wins[k + 1].first) of the
// mapping to the host loop (SamFile::seek_text with an end).
//
// MembersOutput (BAM, or nothing with -S on BAM input): the kept records come back as finished BGZF members in a buffer of the
// BamWriter's and go to BamWriter::put_members.  From lines they are encoded on the device against the @SQ names the writer's header
// was written from; a kept line that BamWriter::encode_record would refuse, or whose numbers are not plain ones, makes the window the
// host loop's.  TextOutput (SAM text / STDOUT, or nothing with -S on SAM input): the kept lines with their tag field appended come back
// in a page-locked buffer and go to the Sink.  From BAM they are formatted on the device with the reference names of the input's header;
// a kept record with a float that "%g" would write in exponent notation makes the window the host loop's.
#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <thread>
#include <type_traits>

#include "../../../include/merkurio_hip.h"
#include "commands.hpp"
#include "extract_common.hpp"
#include "io.hpp"

namespace cli {

namespace {

// file[lo, hi) -> dst on a few host threads (first touch of the mapping's pages included)
void copy_in(const uint8_t *file, uint64_t lo, uint64_t hi, uint8_t *dst) {
    const uint64_t n = hi - lo;
    const size_t T = std::max<size_t>(1, std::min<size_t>(std::max(1u, io_threads() / 2), (size_t)(n >> 22) + 1));
    run_threads(T, [&](size_t t) { memcpy(dst + n * t / T, file + lo + n * t / T, (size_t)(n * (t + 1) / T - n * t / T)); });
}

// what the workers share: whose turn it is to emit, and how the job ends early
constexpr size_t kRefusedInARow = 4;  // R: after so many refused windows in a row the rest of the file is the host loop's

struct Pipe {
    std::mutex mu;
    std::condition_variable cv;
    size_t emit_turn = 0;         // windows before this one have been emitted
    bool stop = false;            // the job ends here (an error) or goes to the host loop (`refused`): nothing further is emitted
    size_t refused = ~(size_t)0;  // the window the host loop takes the rest of the file over at (the R-th refused one in a row)
    std::string error;
    size_t n_device = 0, n_host = 0;  // windows the device emitted | the host loop took: in turns, and behind a hand-over
    size_t refused_in_a_row = 0;
    struct Left {
        size_t k;
        int rc;  // what the window returned
        uint32_t status;
    };
    std::vector<Left> left;  // the windows the device refused
    // BAM's head chain: window k + 1 starts with window k's tail, reported by the library as soon as it is known (on_tail)
    size_t heads_ready = 0;  // the head of window `heads_ready` is in `head` (windows before it have theirs already)
    std::vector<uint8_t> head;
    std::vector<uint8_t> refused_head;  // the head window `refused` was given
};

// One worker per handle: window k runs on worker k mod n_workers (with the handles of several devices in a row, consecutive windows
// go to different devices).  `make(id)` gives worker id its format's state W: W.w is the library's window struct (tag and keep rule
// filled in here), W.load(k) puts window k's input where the device reads it (false: the job has been stopped), W.call(...) runs the
// window, W.grow() makes the room for tail and output that a call asked for, W.write() hands the output on.  A window the device
// refuses waits for its turn like any other and then has the host loop run over its bounds (W.host_turn) where its output would have
// gone: the loop's bytes, counters, per-pattern counts and log rows land in window order, the workers behind go on.  The
// kRefusedInARow-th refused window in a row is not run but noted (W.refused, pipe.mu held) and ends the windows: the host loop takes
// the file from its first byte.  Results leave in window order, and after `stop` none do; a worker holds one finished window at most
// while it waits for its turn.  The first error is left in pipe.error.
template <class Make>
void run_windows(const TagArgs &a, Pipe &pipe, size_t n_win, size_t n_workers, const std::vector<TagHandle> &handles, Loggers &lg, const Patterns &pats,
                 const std::string &in_name, double (&t_dev)[8], const HostTurn &turn, Make make) {
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
            if (!err.empty()) {
                pipe.stop = true, pipe.error = err;
                pipe.cv.notify_all();
                return;
            }
            if (refused) {
                pipe.left.push_back({k, rc, status});
                if (++pipe.refused_in_a_row >= kRefusedInARow) {
                    pipe.stop = true, pipe.refused = k, pipe.n_host += n_win - k;
                    W.refused();
                    pipe.cv.notify_all();
                    return;
                }
                lk.unlock();
                // (only the worker whose turn it is gets here: the reader, the loggers and the output are its alone)
                std::string turn_err;
                try {
                    W.host_turn(k, [&] { turn(handles[id]); });
                } catch (const Error &e) {
                    turn_err = e.what()[0] ? e.what() : "error";
                }
                lk.lock();
                ++pipe.n_host;
                if (!turn_err.empty()) pipe.stop = true, pipe.error = turn_err;
                pipe.emit_turn = k + 1;
                pipe.cv.notify_all();
                if (pipe.stop) return;
                continue;
            }
            pipe.refused_in_a_row = 0;
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
            else ++pipe.n_device;
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
}

// ---- the input sides.  An input cuts the job's windows (cut), copies window k to where the device reads it (stage), fills the window
// struct's input fields (fill; false: the job has been stopped), says how much text the window holds for the output's room (text_bytes),
// places the tail (aim), follows a call (done: one that went well; grow: one that asked for more room; refused: one that ends the
// windows), gives the reader the bounds of a window that is the host loop's and runs it (host_turn) and puts the reader where the
// windows stopped (seek; k = the window of the hand-over, ~0: none)
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

// members [m0, m1) of the file: their table re-based to the first one's DEFLATE stream, and that byte range of the file
struct WindowMembers {
    size_t m0 = 0, m1 = 0;
    uint64_t file_lo = 0, file_hi = 0, text = 0;
    std::vector<mk_bgzf_member> mem;
};

// BGZF members with the head chain
struct MemberInput {
    static constexpr bool is_bam = true, corrupt_is_refused = true;  // (a damaged member)
    static constexpr const char *error = "Error during BAM record parsing: ";
    using Windows = std::vector<WindowMembers>;
    const Windows &wins;
    const uint8_t *file;
    Pipe &pipe;
    SamFile &sam;
    HostBuffer stage_buf;  // the window's members (page-locked)
    std::vector<uint8_t> tail = std::vector<uint8_t>(1u << 20), head;
    TailCtx tctx{};

    static const uint8_t *bytes(const WindowSource &src) { return src.file_bytes(); }
    // the windows of the rest of the file: runs of members of ~window_bytes of text (the same whatever the heads turn out to be); the
    // records behind the header that open() has inflated already are the first head -- a window of their own if no member follows
    static Windows cut(SamFile &sam, Pipe &pipe, uint64_t window_bytes) {
        const WindowSource &src = sam.source();
        uint64_t n_pending = 0;
        const char *pend = sam.bam_pending(&n_pending);
        pipe.head.assign(pend, pend + n_pending);
        const std::vector<mk_bgzf_member> &mem = src.bgzf_members();
        const size_t n_mem = mem.size();
        Windows wins;
        for (size_t m0 = src.next_member(); m0 < n_mem;) {
            WindowMembers W;
            W.m0 = m0, W.m1 = bgzf_run_end(mem, m0, n_mem, window_bytes);
            const mk_bgzf_member &last = mem[W.m1 - 1];
            W.file_lo = mem[m0].data_off, W.file_hi = last.data_off + last.data_len;
            W.text = last.out_off + last.isize - mem[m0].out_off;
            W.mem = bgzf_rebased(mem.data() + m0, W.m1 - m0, W.file_lo, mem[m0].out_off);
            m0 = W.m1;
            wins.push_back(std::move(W));
        }
        if (wins.empty() && !pipe.head.empty()) {
            WindowMembers W;
            W.m0 = W.m1 = n_mem;
            wins.push_back(std::move(W));
        }
        return wins;
    }
    static void seek(SamFile &sam, const Windows &wins, const Pipe &pipe, size_t k) {
        if (k != ~(size_t)0) sam.seek_bam(wins[k].m0, (const char *)pipe.refused_head.data(), pipe.refused_head.size());
    }

    uint64_t text_bytes(size_t k) const { return wins[k].text + (1u << 20); }  // (and a head)
    void stage(size_t k) {
        const WindowMembers &X = wins[k];
        if (X.mem.empty()) return;
        if (!stage_buf.grow(X.file_hi - X.file_lo, 1u << 20)) bail(std::string(error) + mk_last_error());
        copy_in(file, X.file_lo, X.file_hi, stage_buf.p);
    }
    template <class Win>
    bool fill(size_t k, Win &w) {
        const WindowMembers &X = wins[k];
        {
            std::unique_lock<std::mutex> lk(pipe.mu);
            pipe.cv.wait(lk, [&] { return pipe.stop || pipe.heads_ready >= k; });
            if (pipe.stop) return false;
            head = pipe.head;
        }
        tctx = TailCtx{&pipe, k};
        w.head = head.data(), w.n_head = head.size();
        w.bgzf = stage_buf.p, w.n_bgzf = X.file_hi - X.file_lo;
        w.members = X.mem.data(), w.n_members = X.mem.size();
        w.last = k + 1 == wins.size();
        w.on_tail = on_tail, w.on_tail_ctx = &tctx;
        return true;
    }
    template <class Win>
    void aim(Win &w) {
        w.tail = tail.data(), w.tail_cap = tail.size();
    }
    template <class Win>
    void done(const Win &w) {
        on_tail(&tctx, tail.data(), w.n_tail);  // (an empty window returns before the library reports it)
    }
    template <class Win>
    bool grow(const Win &w) {
        if (w.n_tail <= tail.size()) return false;
        tail.resize(w.n_tail + (1u << 20));
        return true;
    }
    void refused() { pipe.refused_head = head; }  // (the head the window was given, not the current one)
    // The head the window was given, then its members; the loop stops in front of the record that crosses the window's end.  That
    // record's first bytes are window k + 1's head: where the device got as far as its record index they are the tail it has
    // reported already (the same chain walked by the same rule: window k + 1 stands, and may be running), where it did not (a record
    // chain it could not prove, an unfinished record, a damaged member) window k + 1 has been waiting for them.  Either way no
    // window ever starts with a head that is not the true one, so none has to be run again.  (on_tail's `heads_ready != k` guard is
    // what makes the second publication a no-op: once the device's tail has moved heads_ready to k + 1, window k + 1 may already
    // have published window k + 2's head into pipe.head, and the bytes handed in here must not overwrite it.)
    template <class Run>
    void host_turn(size_t k, Run run) {
        sam.seek_bam(wins[k].m0, (const char *)head.data(), head.size(), wins[k].m1);
        run();
        uint64_t n_left = 0;
        const char *left = sam.bam_pending(&n_left);
        on_tail(&tctx, (const uint8_t *)left, n_left);
    }
};

// SAM text: windows cut at line starts have no heads or tails and are independent
struct LineInput {
    static constexpr bool is_bam = false, corrupt_is_refused = false;
    static constexpr const char *error = "Error during SAM record parsing: ";
    using Windows = std::vector<std::pair<uint64_t, uint64_t>>;
    const Windows &wins;
    const uint8_t *file;
    Pipe &pipe;
    SamFile &sam;
    HostBuffer stage_buf;  // the window's text (page-locked)
    uint8_t no_tail[8];

    static const uint8_t *bytes(const WindowSource &src) { return (const uint8_t *)src.text(); }
    // [b, e) per window, e = the first line start at or behind b + window_bytes
    static Windows cut(SamFile &sam, Pipe &, uint64_t window_bytes) {
        const uint8_t *file = bytes(sam.source());
        const uint64_t n_file = sam.source().text_size();
        Windows wins;
        for (uint64_t b = sam.text_cursor(); b < n_file;) {
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
    static void seek(SamFile &sam, const Windows &wins, const Pipe &, size_t k) { sam.seek_text(k != ~(size_t)0 ? wins[k].first : sam.source().text_size()); }

    uint64_t text_bytes(size_t k) const { return wins[k].second - wins[k].first; }
    void stage(size_t k) {
        if (!stage_buf.grow(text_bytes(k), 1u << 20)) bail(std::string(error) + mk_last_error());
        copy_in(file, wins[k].first, wins[k].second, stage_buf.p);
    }
    template <class Win>
    bool fill(size_t k, Win &w) {
        w.text = stage_buf.p, w.n_text = text_bytes(k);
        w.last = 1;  // (the window ends at a line end or at the end of the file: all of it is lines)
        return true;
    }
    template <class Win>
    void aim(Win &w) {
        w.tail = no_tail, w.tail_cap = sizeof(no_tail);
    }
    template <class Win>
    void done(const Win &) {}
    template <class Win>
    bool grow(const Win &) {
        return false;
    }
    void refused() {}
    template <class Run>
    void host_turn(size_t k, Run run) {
        sam.seek_text(wins[k].first, wins[k].second);
        run();
    }
};

// ---- the output sides.  An output makes room for what `text` bytes of window text may turn into (room: a guess -- a window that does
// not fit is done again with the size it asked for, grow), places its buffer (aim), follows a call that went well (done) and hands the
// output on (write).  `error` = the input side's prefix.
struct MembersOutput {
    BamWriter *bw;   // absent: -S
    HostBuffer out;  // the members the window turns into (the writer's, moved back to it)
    MembersOutput(BamWriter *bw_, bool, bool) : bw(bw_) {}
    // (BAM-shaped text deflates to a third, and a BAM record is shorter than its line)
    static uint64_t out_guess(uint64_t text) { return text / 3 + (4u << 20); }
    void take(uint64_t n) {
        out.reset();
        out = bw->take_raw_buffer(n);
    }
    void room(uint64_t text, const char *) {
        if (bw && out.cap < out_guess(text)) take(out_guess(text));
    }
    template <class Win>
    void aim(Win &w) {
        w.out = bw ? out.p : nullptr, w.out_cap = bw ? out.cap : 0;
    }
    template <class Win>
    void done(const Win &) {}
    template <class Win>
    bool grow(const Win &w, const char *) {
        if (!bw || w.out_len <= out.cap) return false;
        take(w.out_len);
        return true;
    }
    template <class Win>
    void write(const Win &w) {
        if (bw && w.out_len) bw->put_members(std::move(out), w.out_len);
    }
};

struct TextOutput {
    Sink *sink;  // absent: -S
    bool from_bam, all_kept;  // all_kept: neither -m nor -v
    HostBuffer out;    // the kept lines (page-locked)
    double ratio = 0;  // from BAM: line bytes per byte of window text of this worker's previous window (0: none yet)
    TextOutput(Sink *sink_, bool from_bam_, bool all_kept_) : sink(sink_), from_bam(from_bam_), all_kept(all_kept_) {}
    // From lines: a kept line grows by its tag field, a tenth of a 350-byte line per matched 31-mer.  From BAM the first guess comes from
    // the flags: with everything kept the lines take more than the window's text (SEQ doubles, the numbers grow), with -m or -v what the
    // k-mers select -- an eighth is a guess; after that the previous window's ratio and a quarter, which keeps a repeat the exception.
    uint64_t guess(uint64_t text) const {
        if (!from_bam) return text + text / 4 + (1u << 20);
        const double r = ratio > 0 ? ratio * 1.25 : all_kept ? 2.25 : 0.125;
        return (uint64_t)((double)text * r) + (1u << 20);
    }
    void room(uint64_t text, const char *error) {
        if (sink && out.cap < guess(text) && !out.grow(guess(text), 1u << 20)) bail(std::string(error) + mk_last_error());
    }
    template <class Win>
    void aim(Win &w) {
        w.out = sink ? out.p : nullptr, w.out_cap = sink ? out.cap : 0;
    }
    template <class Win>
    void done(const Win &w) {
        if (w.n_window) ratio = (double)w.out_len / (double)w.n_window;
    }
    template <class Win>
    bool grow(const Win &w, const char *error) {
        if (!sink || w.out_len <= out.cap) return false;
        if (!out.grow(w.out_len, 1u << 20)) bail(std::string(error) + mk_last_error());
        return true;
    }
    template <class Win>
    void write(const Win &w) {
        if (sink && w.out_len) sink->write((const char *)out.p, w.out_len);
    }
};

// ---- a direction: its window struct picks the library's entry point, which gets the reference names where the struct has them (the
// writer's @SQ names / the input header's: what RNAME and RNEXT are looked up in / printed from)
struct Refs {
    std::vector<uint8_t> ref_bytes;
    std::vector<uint64_t> ref_off = std::vector<uint64_t>(1, 0);
};
int call_window(mk_matcher *m, mk_codec *codec, const Refs &, mk_bam_window *w, int logging, mk_counters *c, uint32_t *counts, uint32_t *status) {
    return mk_tag_bam_window(m, codec, w, logging, c, counts, status);
}
int call_window(mk_matcher *m, mk_codec *, const Refs &, mk_sam_window *w, int logging, mk_counters *c, uint32_t *counts, uint32_t *status) {
    return mk_tag_sam_window(m, w, logging, c, counts, status);
}
int call_window(mk_matcher *m, mk_codec *codec, const Refs &R, mk_sam_bam_window *w, int logging, mk_counters *c, uint32_t *counts, uint32_t *status) {
    w->ref_names = R.ref_bytes.data(), w->ref_off = R.ref_off.data(), w->n_refs = R.ref_off.size() - 1;
    return mk_tag_sam_bam_window(m, codec, w, logging, c, counts, status);
}
int call_window(mk_matcher *m, mk_codec *codec, const Refs &R, mk_bam_sam_window *w, int logging, mk_counters *c, uint32_t *counts, uint32_t *status) {
    w->ref_names = R.ref_bytes.data(), w->ref_off = R.ref_off.data(), w->n_refs = R.ref_off.size() - 1;
    return mk_tag_bam_sam_window(m, codec, w, logging, c, counts, status);
}

// what run_windows asks of a worker, from an input and an output
template <class In, class Out, class Win>
struct Worker {
    In in;
    Out out;
    const Refs &refs;
    mk_matcher *m;
    mk_codec *codec;  // (none: SAM -> SAM)
    Win w{};
    static constexpr bool corrupt_is_refused = In::corrupt_is_refused;
    ~Worker() {
        if (codec && !g_process_is_ending) mk_codec_destroy(codec);
    }
    bool load(size_t k) {
        in.stage(k);
        out.room(in.text_bytes(k), In::error);
        return in.fill(k, w);
    }
    int call(int logging, mk_counters *wc, uint32_t *wcounts, uint32_t *status) {
        in.aim(w), out.aim(w);
        const int rc = call_window(m, codec, refs, &w, logging, wc, wcounts, status);
        if (rc == MK_OK && !*status) in.done(w), out.done(w);
        return rc;
    }
    bool grow() {
        const bool tail_grew = in.grow(w), out_grew = out.grow(w, In::error);
        return tail_grew || out_grew;
    }
    void refused() { in.refused(); }
    template <class Run>
    void host_turn(size_t k, Run run) {
        in.host_turn(k, run);
    }
    void write() { out.write(w); }
};

// the [timing] texts of a direction
struct Direction {
    const char *title;       // "N of M<title> windows on the device"
    const char *phases[8];   // what ms[0 ...] of its entry point are
    const char *left_to;     // who takes a refused window
    const char *reasons[4];  // status bits 1, 2, 4 (nullptr: not this direction's) | any other refusal
};
const Direction kBamBam = {"", {"upload", "inflate", "record index", "unpack + scan + sets", "tag + pack", "deflate", "download"}, "reader",
                           {"record chain", "optional fields", "existing tag", "unfinished record"}};
const Direction kSamSam = {" SAM text", {"upload", "line index + fields", "gather + scan + sets", "tag + emit", "download"}, "reader",
                           {"a line with too few fields", nullptr, nullptr, "existing tag"}};
const Direction kSamBam = {" SAM text -> BAM", {"upload", "line index + fields", "gather + scan + sets", "tag + encode", "deflate", "download"}, "loop",
                           {"a line with too few fields", "a record the device does not encode", nullptr, "existing tag"}};
const Direction kBamSam = {" BAM -> SAM text", {"upload", "inflate", "record index", "unpack + scan + sets", "tag + format", "download"}, "loop",
                           {"record chain", "a record the device does not format", "existing tag", "unfinished record"}};

// (the row's first number is the windows the DEVICE emitted -- a window's host turn is not one of them --, and the rows are printed
// before an error ends the job: a window whose turn bailed still has its `left to the host` row in front of the error message)
void report(const Direction &D, const Pipe &pipe, size_t n_win, size_t n_workers, const double (&t_dev)[8]) {
    std::string row;
    char buf[64];
    for (int i = 0; D.phases[i]; ++i) {
        snprintf(buf, sizeof(buf), "%s %.3f", D.phases[i], t_dev[i] / 1e3);
        row += (i ? ", " : "") + std::string(buf);
    }
    fprintf(stderr,
            "[timing] %llu of %llu%s windows on the device (%llu in flight): %s s (of these, growing device buffers: %.3f s); windows: %llu on the device, "
            "%llu on the host\n",
            (unsigned long long)pipe.n_device, (unsigned long long)n_win, D.title, (unsigned long long)n_workers, row.c_str(), t_dev[7] / 1e3,
            (unsigned long long)pipe.n_device, (unsigned long long)pipe.n_host);
    for (const Pipe::Left &x : pipe.left) {
        const char *why = x.rc == MK_E_CORRUPT ? "a damaged member" : D.reasons[3];
        for (int bit = 2; bit >= 0 && x.rc != MK_E_CORRUPT; --bit)
            if ((x.status >> bit & 1) && D.reasons[bit]) why = D.reasons[bit];
        fprintf(stderr, "[timing] window %llu left to the host %s (%s)%s\n", (unsigned long long)x.k, D.left_to, why,
                x.k == pipe.refused ? " with every window behind it" : "");
    }
}

// The driver of all four directions.  `target`: where the output side sends (nullptr: -S); names: the reference names the direction's
// entry point takes (nullptr: none); turn: the host loop over what the reader has been bounded to (a refused window).  false: the
// kRefusedInARow-th window in a row was not for the device and the reader stands at its first byte.
template <class In, class Out, class Win, class Target>
bool tag_windows(const Direction &D, const TagArgs &a, SamFile &sam, const std::vector<TagHandle> &handles, Loggers &lg, const Patterns &pats,
                 const std::string &in_name, Target *target, const std::vector<std::string> *names, uint64_t window_bytes, const HostTurn &turn) {
    const uint8_t *file = In::bytes(sam.source());
    Pipe pipe;
    const typename In::Windows wins = In::cut(sam, pipe, window_bytes);
    if (wins.empty()) return true;
    Refs refs;
    for (size_t i = 0; names && i < names->size(); ++i) {
        refs.ref_bytes.insert(refs.ref_bytes.end(), (*names)[i].begin(), (*names)[i].end());
        refs.ref_off.push_back(refs.ref_bytes.size());
    }
    refs.ref_bytes.push_back(0);  // (never empty: a pointer to hand over)
    const size_t n_win = wins.size();
    // (window k runs on handle k mod n_workers: with the handles of several devices in a row, consecutive windows go to different devices)
    const size_t n_workers = std::max<size_t>(1, std::min<size_t>(handles.size(), n_win));
    double t_dev[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    run_windows(a, pipe, n_win, n_workers, handles, lg, pats, in_name, t_dev, turn, [&](size_t id) {
        mk_codec *codec = nullptr;
        if (!std::is_same<Win, mk_sam_window>::value && mk_codec_create(handles[id].device, &codec) != MK_OK) bail(std::string(In::error) + mk_last_error());
        return Worker<In, Out, Win>{In{wins, file, pipe, sam}, Out(target, In::is_bam, !a.filter_matching && !a.invert_match), refs, handles[id].m, codec};
    });
    if (getenv("MERKURIO_TIMING")) report(D, pipe, n_win, n_workers, t_dev);
    if (!pipe.error.empty()) bail(pipe.error);
    In::seek(sam, wins, pipe, pipe.refused);
    return pipe.refused == ~(size_t)0;
}

}  // namespace

bool tag_bam_windows_on_device(const TagArgs &a, SamFile &sam, const std::vector<TagHandle> &handles, Loggers &lg, const Patterns &pats,
                               const std::string &in_name, BamWriter *bw, uint64_t window_bytes, const HostTurn &turn) {
    return tag_windows<MemberInput, MembersOutput, mk_bam_window>(kBamBam, a, sam, handles, lg, pats, in_name, bw, nullptr, window_bytes, turn);
}

bool tag_sam_windows_on_device(const TagArgs &a, SamFile &sam, const std::vector<TagHandle> &handles, Loggers &lg, const Patterns &pats,
                               const std::string &in_name, Sink *out_sink, uint64_t window_bytes, const HostTurn &turn) {
    return tag_windows<LineInput, TextOutput, mk_sam_window>(kSamSam, a, sam, handles, lg, pats, in_name, out_sink, nullptr, window_bytes, turn);
}

bool tag_sam_bam_windows_on_device(const TagArgs &a, SamFile &sam, const std::vector<TagHandle> &handles, Loggers &lg, const Patterns &pats,
                                   const std::string &in_name, BamWriter &bw, uint64_t window_bytes, const HostTurn &turn) {
    return tag_windows<LineInput, MembersOutput, mk_sam_bam_window>(kSamBam, a, sam, handles, lg, pats, in_name, &bw, &bw.ref_names, window_bytes, turn);
}

bool tag_bam_sam_windows_on_device(const TagArgs &a, SamFile &sam, const std::vector<TagHandle> &handles, Loggers &lg, const Patterns &pats,
                                   const std::string &in_name, Sink &out_sink, uint64_t window_bytes, const HostTurn &turn) {
    return tag_windows<MemberInput, TextOutput, mk_bam_sam_window>(kBamSam, a, sam, handles, lg, pats, in_name, &out_sink, &sam.ref_names, window_bytes, turn);
}

}  // namespace cli
