// extract_windows.cpp -- `merkurio extract` over text windows that are indexed on the device: prepare(), run()
// and the three loops of the pipeline, with its queues, the tail map and the end-of-job path.
//
// Everything the reference's loops read through needletail (src/cmd_extract.rs:281-282 single, :412-418 paired; records consumed
// at :321-328 and :463-468) goes to the GPU as raw text: one FASTQ or FASTA file or a pair of them, plain, gzip, bzip2 or bgzip'ed,
// on one device or dealt window by window to several.  Each input has one source of window bodies (extract_sources.hpp: host text,
// BGZF members, device text, gzip stream).  mk_extract_window does the rest: record index, sequences, scan, emission order, rows,
// counts, keep.
//
//   reader thread   bodies of window k + 1 from every input's source, then -- where windows depend on each other -- the tails of
//                   window k as its heads
//   device threads  window k on device k mod N: one call (extract_window_call.cpp); a window the device refuses (not plain 4-line
//                   FASTQ / FASTA, or too large for it) is parsed by the host reader's own code instead, which also words the
//                   reference's parse errors
//   main thread     results in window order: log rows (reference emission order), kept records (extract_write.cpp)
//
// Windows depend on each other when a window can end inside a record (BGZF members, device text: the host never sees the text) or when
// the two files of a pair hold different numbers of records per window (the leftovers of one are carried): then window k + 1 cannot
// start before window k has returned its tails, whatever device it runs on; a single plain input has no such chain and its windows
// run on their devices independently.
#include <fcntl.h>
#include <unistd.h>

#include <thread>

#include "extract_windows.hpp"

namespace cli {

using xw::kFirstWindow;
using Win = xw::Win;

void WindowExtract::Impl::reader_loop() {
    const size_t N = devs.size();
    for (uint64_t k = 0;; ++k) {
        std::unique_ptr<Win> W(new Win);
        W->k = k, W->dev = (int)(k % N);
        mk_matcher *m_ahead = ms.empty() ? nullptr : ms[W->dev];
        auto ask = [&](int i, bool first) {  // the next body of input i; first: no page-locked staging yet, a small window
            Side &S = W->side[i];
            const uint64_t full = src[i]->on_device() ? bgzf_target : (first ? std::min(plain_target, kFirstWindow) : plain_target);
            // (the previous window's leftovers count against this one: the two files of a pair then advance at the same rate)
            const uint64_t target = std::max<uint64_t>(1u << 16, full > last_head[i] ? full - last_head[i] : 0);
            S.from = src[i].get(), S.on_device = src[i]->on_device();
            src[i]->next(k, S, target, m_ahead);
        };
        if (open_mode && k > 0) {  // open windows finish out of order: no more than N + 2 of them ahead of the writer
            std::unique_lock<std::mutex> lk(gate.mu);
            gate.cv.wait(lk, [&] { return gate.failed || k < written + N + 2; });
            if (gate.failed) return;
            W->open = !open_off;
        }
        for (int i = 0; i < n_in; ++i) ask(i, k == 0);
        if (chained && k > 0 && !W->open) {  // the tails of window k - 1 are this window's heads
            std::unique_lock<std::mutex> lk(gate.mu);
            gate.cv.wait(lk, [&] { return gate.failed || tails.count(k - 1); });
            if (gate.failed) return;
            std::vector<std::vector<char>> t = std::move(tails[k - 1]);
            tails.erase(k - 1);
            lk.unlock();
            for (int i = 0; i < n_in; ++i) {
                W->side[i].head = std::move(t[i]);
                last_head[i] = W->side[i].head.size();
            }
        }
        {
            std::lock_guard<std::mutex> lk(gate.mu);
            if (gate.failed) return;
        }
        for (int i = 0; i < n_in; ++i)
            if (std::unique_ptr<xw::Source> next = src[i]->hand_back(W->side[i])) {  // the source changed kind: ask it once more
                last_head[i] = 0;
                retired.push_back(std::move(src[i]));
                src[i] = std::move(next);
                ask(i, true);
            }
        bool any = false;
        for (int i = 0; i < n_in; ++i) any = any || W->side[i].has_body() || !W->side[i].head.empty();
        if (!any) {
            std::lock_guard<std::mutex> lk(gate.mu);
            reader_done = true;
            n_windows = k;
            gate.cv.notify_all();
            return;
        }
        if (n_in == 2) {
            // one file has nothing left while the other still holds records: the reference notices at this point, after the common
            // part (src/cmd_extract.rs:465-468 file 2 ends first; :608-612 file 2 still has records)
            bool none[2];
            for (int i = 0; i < 2; ++i) none[i] = W->side[i].head.empty() && !W->side[i].has_body();
            if (none[0] != none[1]) {
                W->error = none[1] ? "Error during FASTQ record parsing of second file. Do the two input files contain the same number of records?"
                                   : "The two input files have a different number of records. Please provide valid paired-end read files.";
                // (what the other file still holds may be nothing but blank lines at its end: the host parser says)
                Side &S = W->side[none[0] ? 1 : 0];
                bool only_blank = S.grp.empty() && !S.n_dev_body;
                for (char ch : S.head) only_blank = only_blank && (ch == '\n' || ch == '\r');
                for (uint64_t q = 0; q < S.n_body && only_blank; ++q) only_blank = S.body[q] == '\n' || S.body[q] == '\r';
                if (only_blank) W->error.clear(), W->by_host = true;  // an empty window: nothing to do, the job goes on to its end
            }
        }
        const bool stop = !W->error.empty();
        std::lock_guard<std::mutex> lk(gate.mu);
        queue[W->dev].push_back(std::move(W));
        if (stop) reader_done = true, n_windows = k + 1;
        gate.cv.notify_all();
        if (stop) return;
    }
}

void WindowExtract::Impl::device_loop(size_t d) {
    mk_matcher *m = ms[d];
    for (;;) {
        std::unique_ptr<Win> W;
        {
            std::unique_lock<std::mutex> lk(gate.mu);
            // (--open-windows: the writer sends seams and re-runs until it has ended)
            gate.cv.wait(lk, [&] { return gate.failed || !queue[d].empty() || (reader_done && (!open_mode || writer_done)); });
            if (gate.failed) return;
            if (queue[d].empty()) return;  // (reader_done)
            W = std::move(queue[d].front());
            queue[d].pop_front();
        }
        const double t_call = PhaseTimer::now();
        if (W->error.empty() && !W->by_host) {
            // an error of this window (a malformed record, a damaged member) is raised when the writer reaches the window: the
            // reference has written everything in front of it by then
            try {
                device_window(*W, m, codecs.empty() ? nullptr : codecs[d]);
            } catch (const Error &e) {
                W->error = e.what()[0] ? e.what() : "error";
                for (int i = 0; i < n_in; ++i) W->side[i].out.tail.clear();
            }
        }
        if (gate.timing) {
            float ms4[4] = {0, 0, 0, 0};
            (void)mk_matcher_batch_times(m, ms4);
            fprintf(stderr, "[timing]   device %zu, window %llu: call %.1f ms (upload %.1f, device %.1f, download %.1f, host %.1f)%s\n", d,
                    (unsigned long long)W->k, (PhaseTimer::now() - t_call) * 1e3, ms4[0], ms4[1], ms4[2], ms4[3], W->by_host ? " [host parser]" : "");
        }
        std::lock_guard<std::mutex> lk(gate.mu);
        for (int i = 0; i < n_in; ++i) {  // (the text the writer needs has been copied out of the staging buffers: device and host windows alike)
            Side &S = W->side[i];
            if (S.from) S.from->window_left_device(S);
            S.body = nullptr, S.n_body = 0;
            std::vector<char>().swap(S.own);
            if (!chained) std::vector<char>().swap(S.head);
        }
        if (W->job) {  // a seam or a re-run: the writer waits for it
            job_done = std::move(W);
            gate.cv.notify_all();
            continue;
        }
        if (chained && !open_mode) {  // (--open-windows: a tail counts once its window is proved -- the writer publishes it)
            std::vector<std::vector<char>> t(2);
            for (int i = 0; i < n_in; ++i) t[i] = W->side[i].out.tail;  // (a copy: the window itself goes to the writer)
            tails[W->k] = std::move(t);
        }
        const uint64_t k = W->k;
        gate.n_done = std::max(gate.n_done, k + 1);
        done[k] = std::move(W);
        gate.cv.notify_all();
    }
}

// ---- `extract --open-windows`: what the writer does when it reaches an OPEN window, one that started at a BGZF member
// and found its own first record (mk_extract_window_open).  The text between the window in front and that record -- tail(k - 1) ++
// front(k) -- goes through a seam call, which also proves the found start: begun at a true record start it takes its whole text
// (status 0, n_used = n_window) if and only if the found start is a record start.  A disproved window is run again the
// chained way, head = tail(k - 1); after 4 of them in a row the reader chains the rest of the file.  Seams and re-runs run on the
// window's device thread (a matcher handle serves one call at a time): the writer queues them in front and waits.
// W to the front of its device's queue; -> W once its device thread is through with it.  NO OVERLAP is gained here: the writer issues a
// seam only when it reaches window k (not as soon as windows k - 1 and k are both done), one at a time, and the job lands behind
// whatever call that device thread has in flight -- on one device a seam can cost the writer up to one whole window call of waiting
std::unique_ptr<Win> WindowExtract::Impl::run_job(std::unique_ptr<Win> W) {
    W->job = true;
    std::unique_lock<std::mutex> lk(gate.mu);
    queue[W->dev].push_front(std::move(W));
    gate.cv.notify_all();
    gate.cv.wait(lk, [&] { return gate.failed || job_done; });
    if (!job_done) bail(gate.failure);
    return std::move(job_done);
}

// -> the window whose results stand for window k: W itself behind a seam that passed (the seam has been emitted), else its chained re-run
std::unique_ptr<Win> WindowExtract::Impl::settle_open_window(std::unique_ptr<Win> W, const std::vector<char> &prev_tail, int &disproved_in_a_row,
                                                             const std::function<void(Win &)> &emit) {
    ++n_open;
    bool proved = false;
    if (!W->refused) {
        std::unique_ptr<Win> seam(new Win);
        seam->k = W->k, seam->dev = W->dev, seam->probe = true;
        xw::Side &S = seam->side[0];
        S.head = prev_tail;
        S.own = W->front;
        S.body = S.own.data(), S.n_body = S.own.size();
        S.ends = true;
        ++n_seams;
        seam = run_job(std::move(seam));
        // (an error of the seam's own -- nothing but a failing device call -- disproves nothing: it is the job's error)
        if (!seam->error.empty()) bail(seam->error);
        proved = !seam->refused && seam->side[0].out.n_used == seam->side[0].out.n_window;
        if (proved) emit(*seam);
    }
    if (proved) {
        disproved_in_a_row = 0;
        return W;
    }
    // disproved: the same members once more, with the tail in front as their head; the first results are dropped, their counters with them
    ++n_reruns;
    if (++disproved_in_a_row >= 4) {
        std::lock_guard<std::mutex> lk(gate.mu);
        open_off = true;
    }
    std::unique_ptr<Win> R(new Win);
    R->k = W->k, R->dev = W->dev;
    xw::Side &S = R->side[0], &O = W->side[0];
    S.head = prev_tail;
    S.grp = O.grp, S.ends = O.ends, S.from = O.from, S.on_device = O.on_device;
    W.reset();
    R = run_job(std::move(R));
    if (!R->error.empty()) bail(R->error);
    return R;
}

WindowExtract::~WindowExtract() {
    if (!impl) return;
    for (int i = 0; i < 2; ++i)
        if (impl->in[i].fd >= 0) close(impl->in[i].fd);
    // (codec handles, like the page-locked buffers, are not released at the end of the run: that costs more than the process has left to live)
    if (!g_process_is_ending)
        for (mk_codec *c : impl->codecs) mk_codec_destroy(c);
    delete impl;
}

// the first byte of a bgzip'ed text that is not a line end: zlib on its first members, here
static int first_text_byte_of_bgzf(const WindowSource &ws, const std::string &path) {
    const std::vector<mk_bgzf_member> &mem = ws.bgzf_members();
    for (size_t g = 0; g < mem.size() && g < 64; ++g) {
        if (!mem[g].isize) continue;
        const mk_bgzf_member e = bgzf_rebased(&mem[g], 1, 0, mem[g].out_off)[0];
        std::vector<char> out(e.isize);
        inflate_bgzf_members_host(ws.file_bytes(), &e, 1, out.data(), path);
        for (char ch : out)
            if (ch != '\n' && ch != '\r') return (unsigned char)ch;
    }
    return -1;
}

bool WindowExtract::prepare(const ExtractArgs &a, const std::vector<int> &devs) {
    impl = new Impl;
    Impl &J = *impl;
    J.a = a;
    J.devs = devs;
    J.n_in = a.in_fastq_2 ? 2 : 1;
    J.in[0].path = a.in_fastx;
    if (a.in_fastq_2) J.in[1].path = *a.in_fastq_2;
    const bool logs = a.out_log || a.json_log;
    const uint64_t window_bytes = (uint64_t)a.window_mb << 20;
    // (windows of 128 MB: the copy into pinned memory of window k + 1 overlaps upload + scan of window k; page-locking a buffer costs
    // ~0.1 ms per MB, so the staging buffers stay small.  With logs every window also pays the ordering / row / count round trips:
    // fewer, larger windows)
    J.plain_target = std::min<uint64_t>(window_bytes, logs ? 256ull << 20 : 128ull << 20);
    J.whole_text = a.invert_match && logs;
    // (a launch of the inflate kernel lasts as long as its slowest member whatever it holds: few, large windows -- and when the text
    // stays on the device, --window-mb's reason, the host's memory, does not apply: 3 GiB unless the flag was given)
    J.bgzf_target = a.window_mb_given ? std::max<uint64_t>(1u << 16, std::min<uint64_t>(window_bytes, 3ull << 30))
                                      : (J.whole_text ? 1ull << 30 : 3ull << 30);
    if (J.n_in == 2) J.bgzf_target = std::max<uint64_t>(1u << 16, J.bgzf_target / 2);
    int kind[2] = {-1, -1};
    for (int i = 0; i < J.n_in; ++i) {
        xw::InputFile &I = J.in[i];
        I.s.open(I.path, !a.host_codec, !a.host_codec && a.device_zstd, !a.host_codec && a.device_xz);
        I.xz_spread = a.xz_spread, I.xz_text_cap = a.xz_text_cap;
        if (I.s.raw_is_deferred()) {
            // not inflated here: run() hands the file to the device once the HIP runtime is up.  What its records are is read from
            // the start of the first block's text (libbz2; libzstd for a .zst input under --device-zstd, liblzma for an .xz input under --device-xz); where that does not say (an
            // empty first stream, a damaged file), the library reads the whole file now, as under --host-codec, and words what is wrong with it
            std::vector<char> first;
            if ((I.s.raw_is_xz() ? xz_first_bytes : I.s.raw_is_zstd() ? zstd_first_bytes : bz2_first_bytes)(I.s.source().file_bytes(), I.s.source().file_size(), first, 1u << 16))
                for (char ch : first)
                    if (ch != '\n' && ch != '\r') {
                        kind[i] = (unsigned char)ch;
                        break;
                    }
            if (kind[i] != '@' && kind[i] != '>') kind[i] = -1, I.s.raw_settle();
        }
        if (J.members_input(i)) {
            kind[i] = first_text_byte_of_bgzf(I.s.source(), I.path);
        } else if (!I.s.raw_is_deferred()) {
            I.have_first = I.s.raw_fill(std::min(J.plain_target, kFirstWindow), &I.first_text, &I.first_n, &I.first_resume);
            if (I.have_first) kind[i] = I.s.raw_fastq() ? '@' : '>';
        }
        if (I.s.raw_is_plain()) I.fd = open(I.path.c_str(), O_RDONLY);
        J.src[i] = J.members_input(i) ? xw::members_source(I) : xw::host_text_source(I, i, J.gate);
    }
    for (int i = 0; i < J.n_in; ++i)
        if (kind[i] != '@' && kind[i] != '>') return false;  // empty, or not FASTA / FASTQ: the host reader words what it is
    if (J.n_in == 2 && kind[0] != kind[1]) return false;
    J.fastq = kind[0] == '@';
    // (a plain gzip input may become device text once the HIP runtime is up, run(): its windows then end anywhere too)
    J.chained = J.n_in == 2 || J.members_input(0) || (!a.host_codec && J.in[0].s.raw_is_gzip()) || J.in[0].s.raw_is_deferred();
    return true;
}

// a window's text, its sequences, its members and its tables all live on the device: keep it to a sixth of what is free there
void WindowExtract::Impl::bound_device_windows() {
    if (const uint64_t free_b = xw::device_free_bytes(devs[0]))
        bgzf_target = std::min<uint64_t>(bgzf_target, std::max<uint64_t>(64ull << 20, free_b / (6 * (uint64_t)n_in)));
}

// libbz2 inflates the file after all, whole, and the first window is read from its text
void WindowExtract::Impl::settle_bzip2(xw::InputFile &I) {
    I.s.raw_settle();
    I.have_first = I.s.raw_fill(std::min(plain_target, kFirstWindow), &I.first_text, &I.first_n, &I.first_resume);
}

// Once the HIP runtime is up: the inputs whose text the device can make become device sources (xw::take_on_device); handles on devs[0]
void WindowExtract::Impl::take_inputs_on_device() {
    // A streamed gzip file holds, per window, its compressed bytes, 12 to 48 16-bit symbols per compressed byte and two text buffers of 12
    // to 48 bytes per compressed byte: about 50 times the window at the usual ratio.  Two windows' worth per streamed file must fit into
    // half of what is free (the text windows' own buffers take a sixth per input), otherwise the window shrinks
    uint64_t gzip_window = a.gzip_window, n_streamed = 0;
    for (int i = 0; i < n_in; ++i)
        if (!a.host_codec && in[i].s.raw_is_gzip() && in[i].s.source().file_size() > gzip_window) ++n_streamed;
    if (const uint64_t free_b = n_streamed ? xw::device_free_bytes(devs[0]) : 0)
        while (gzip_window > (1u << 20) && n_streamed * 2 * 50 * gzip_window > free_b / 2) gzip_window /= 2;
    // A streamed bzip2 file holds, per window, its compressed bytes, 1.125 bytes per symbol in front of the run-length step and two text
    // buffers; at 8 bytes of text per compressed byte (FASTQ: 4 to 5) that is 1 + 1.125 * 8 + 2 * 8 = 26 times the window.  The pass
    // scratch (4.5 bytes per symbol of a block in flight) takes what is left and shrinks its passes when that is little.  The factor is
    // an estimate for FULL blocks and is not measured: the library reserves a block's room by its level's capacity, not by its symbols,
    // so many short streams at level 9 take far more per compressed byte -- there the library decodes the prefix of a window's blocks
    // that fits and leaves the rest to the next window, which keeps the bound whatever this factor is.  Same rule
    uint64_t bzip2_window = a.bzip2_window, n_bz_streamed = 0;
    for (int i = 0; i < n_in; ++i)
        if (bzip2_streamed(i)) ++n_bz_streamed;
    if (const uint64_t free_b = n_bz_streamed ? xw::device_free_bytes(devs[0]) : 0)
        while (bzip2_window > (1u << 20) && n_bz_streamed * 2 * 26 * bzip2_window > free_b / 2) bzip2_window /= 2;
    // The two bzip2 files of a pair that go up WHOLE go ONE AFTER THE OTHER: a one-shot call sizes its passes and accepts its text by the
    // memory that is free when it runs, so the second must find the first's text there already, not a sibling that is about to take the
    // same half.  A file the device does not take is libbz2's, whole, and the job goes on with host text
    // the same holds for the .zst files of a pair under --device-zstd (a larger one than --zstd-window is libzstd's, unless --zstd-stream)
    // and for the .xz files of a pair under --device-xz (a larger one than --xz-window is liblzma's, unless --xz-stream: then it is
    // streamed with window_bytes = 0 -- its windows are bounded by the library's text cap, which the spread rule wants large)
    // A streamed zstd file holds, per window, its compressed bytes, its literals and 12 bytes per sequence, two text buffers and 8
    // bytes of sources per text byte: at 5 bytes of text per compressed byte about 60 times the window.  An estimate, not measured;
    // the library bounds a window's text by its own cap whatever this factor is.  Same rule
    uint64_t zstd_window = a.zstd_window, n_zs_streamed = 0;
    for (int i = 0; i < n_in; ++i)
        if (zstd_streamed(i)) ++n_zs_streamed;
    if (const uint64_t free_b = n_zs_streamed ? xw::device_free_bytes(devs[0]) : 0)
        while (zstd_window > (1u << 20) && n_zs_streamed * 2 * 60 * zstd_window > free_b / 2) zstd_window /= 2;
    // The library's default text cap -- a sixth of the free memory, two text buffers and an upload in half of what is free -- is
    // chosen per codec: the two streamed .xz files of a pair begin side by side and would each see the same free memory, so the CLI
    // gives each its share of that default.  A cap the user set stands as given
    uint64_t n_xz_streamed = 0;
    for (int i = 0; i < n_in; ++i)
        if (xz_streamed(i)) ++n_xz_streamed;
    if (const uint64_t free_b = n_xz_streamed > 1 && !a.xz_text_cap ? xw::device_free_bytes(devs[0]) : 0)
        for (int i = 0; i < n_in; ++i)
            if (xz_streamed(i)) in[i].xz_text_cap = std::max<uint64_t>(free_b / 6 / n_xz_streamed, 1u << 20);
    for (int i = 0; i < n_in; ++i) {
        xw::InputFile &I = in[i];
        if (!I.s.raw_is_deferred() || bzip2_streamed(i) || zstd_streamed(i) || xz_streamed(i)) continue;
        if (std::unique_ptr<xw::Source> dev = xw::take_on_device(I, i, devs[0], I.s.raw_is_xz() ? a.xz_window : I.s.raw_is_zstd() ? a.zstd_window : a.bzip2_window, gate)) {  // (at or below the window: in one call)
            src[i] = std::move(dev);
            continue;
        }
        settle_bzip2(I);
    }
    run_threads((size_t)n_in, [&](size_t i) {  // (the two streamed files of a pair side by side: a handle and a stream each, sized by their windows)
        if (bzip2_streamed((int)i)) {
            if (std::unique_ptr<xw::Source> dev = xw::take_on_device(in[i], (int)i, devs[0], bzip2_window, gate)) src[i] = std::move(dev);
            else settle_bzip2(in[i]);
            return;
        }
        if (zstd_streamed((int)i)) {
            // (the stream is asked for by the file's size against --zstd-window as given; its windows may be smaller)
            in[i].zstd_stream = true;
            if (std::unique_ptr<xw::Source> dev = xw::take_on_device(in[i], (int)i, devs[0], zstd_window, gate)) src[i] = std::move(dev);
            else settle_bzip2(in[i]);
            return;
        }
        if (xz_streamed((int)i)) {
            in[i].xz_stream = true;
            if (std::unique_ptr<xw::Source> dev = xw::take_on_device(in[i], (int)i, devs[0], 0, gate)) src[i] = std::move(dev);
            else settle_bzip2(in[i]);
            return;
        }
        if (a.host_codec || !in[i].s.raw_is_gzip()) return;
        if (std::unique_ptr<xw::Source> dev = xw::take_on_device(in[i], (int)i, devs[0], gzip_window, gate)) src[i] = std::move(dev);
    });
}

void WindowExtract::run(const ExtractArgs &a, const Patterns &pats, Loggers &lg, const std::vector<mk_matcher *> &ms, const std::vector<int> &devs,
                        Sink &w1, Sink &w2, const std::string &name1, const std::string &name2, std::vector<mk_counters> &dev_c,
                        std::vector<std::vector<uint32_t>> &dev_counts, PhaseTimer &tm) {
    Impl &J = *impl;
    xw::Gate &G = J.gate;
    J.pats = &pats, J.lg = &lg, J.ms = ms;
    J.batch_bytes = (uint64_t)a.batch_mb << 20;
    const size_t N = devs.size();
    J.queue.resize(N);
    bool any_bgzf = false;
    for (int i = 0; i < J.n_in; ++i) any_bgzf = any_bgzf || J.members_input(i);
    const bool logs = a.out_log || a.json_log;
    J.z_members = (a.bgzf_output || a.zstd_output) && !a.host_codec && !a.host_ingest && !a.suppress_output && !(logs && a.invert_match);
    if (any_bgzf || J.z_members) {  // (a codec per device: BGZF input is inflated, -z / --zstd-output compressed where its window is)
        for (size_t d = 0; d < N; ++d) {
            mk_codec *c = nullptr;
            mk_check(mk_codec_create(devs[d], &c), "Error setting up the BGZF codec");
            J.codecs.push_back(c);
        }
    }
    J.open_mode = a.open_windows && J.n_in == 1 && J.members_input(0) && !a.bgzf_output && !a.zstd_output && !a.host_ingest;
    if (any_bgzf) J.bound_device_windows();
    J.take_inputs_on_device();
    bool any_dev_text = false;
    for (int i = 0; i < J.n_in; ++i) any_dev_text = any_dev_text || J.src[i]->on_device();
    if (any_dev_text && !any_bgzf) J.bound_device_windows();  // (with the text that was just made there counted)
    // (page-locking costs ~0.2 ms per MB: the N + 1 staging buffers of a host-text input are made on a thread of their own, beside the
    // first window -- which goes up from where it lies --, and handed to the reader as they appear)
    std::vector<std::thread> pin_threads;
    for (int i = 0; i < J.n_in; ++i)
        if (xw::PinPool *pool = J.src[i]->pins()) {
            pool->bufs.resize(N + 1);
            pin_threads.emplace_back([&J, pool] {
                try {
                    pool->make(J.gate, J.plain_target + (1u << 20));
                } catch (const Error &e) {
                    J.gate.fail_all(e.what());
                }
            });
        }
    std::vector<std::thread> th;
    auto guarded = [&](auto fn) {
        return [&J, fn] {
            try {
                fn();
            } catch (const Error &e) {
                J.gate.fail_all(e.what()[0] ? e.what() : "error");
            } catch (const std::exception &e) {
                J.gate.fail_all(std::string("Error: ") + e.what());
            }
        };
    };
    th.emplace_back(guarded([&J] { J.reader_loop(); }));
    for (size_t d = 0; d < N; ++d) th.emplace_back(guarded([&J, d] { J.device_loop(d); }));
    std::string writer_error;
    std::vector<char> prev_tail;  // --open-windows: the tail of the window in front, final
    int disproved_in_a_row = 0;
    try {
        for (uint64_t k = 0;; ++k) {
            std::unique_ptr<xw::Win> W;
            {
                std::unique_lock<std::mutex> lk(G.mu);
                G.cv.wait(lk, [&] { return G.failed || J.done.count(k) || (J.reader_done && k >= J.n_windows); });
                if (G.failed) break;
                if (!J.done.count(k)) break;  // every window is written
                W = std::move(J.done[k]);
                J.done.erase(k);
            }
            if (!W->error.empty()) bail(W->error);
            auto emit = [&](xw::Win &X) {
                tm.mark(X.by_host ? "window: host parser + scan" : "window: H2D + index + scan + D2H");
                add_counters(dev_c[X.dev], X.cb);
                add_counts(dev_counts[X.dev], X.cnt);
                J.write_window(X, w1, w2, name1, name2, tm);
                w1.window_done(), w2.window_done();
            };
            if (W->open) W = J.settle_open_window(std::move(W), prev_tail, disproved_in_a_row, emit);  // (the seam's records go out first)
            emit(*W);
            if (J.open_mode) {  // this window's tail is final: the seam behind it, or a chained window, may use it
                prev_tail = W->side[0].out.tail;
                std::lock_guard<std::mutex> lk(G.mu);
                J.tails.clear();
                J.tails[k] = std::vector<std::vector<char>>{prev_tail, {}};
                J.written = k + 1;
                G.cv.notify_all();
            }
        }
    } catch (const Error &e) {
        writer_error = e.what()[0] ? e.what() : "error";
        G.fail_all(writer_error);
    }
    {
        std::lock_guard<std::mutex> lk(G.mu);
        J.writer_done = true;
        G.cv.notify_all();
    }
    for (auto &t : th) t.join();
    for (auto &t : pin_threads) t.join();
    if (G.failed && G.discard_kept) {  // (the logs likewise: back to what they held before the first window)
        w1.discard(), w2.discard();
        if (lg.text.out) lg.text.out->rollback();
        if (lg.has_json) lg.json.out->rollback();
    }
    if (!writer_error.empty()) bail(writer_error);
    if (G.failed) bail(G.failure);
    if (G.timing && J.open_mode)
        fprintf(stderr, "[timing] extract --open-windows: %llu open windows, %llu seams, %llu re-runs\n", (unsigned long long)J.n_open,
                (unsigned long long)J.n_seams, (unsigned long long)J.n_reruns);
    if (G.timing && a.bgzf_output) {
        fprintf(stderr, "[timing] extract -z: %llu windows as members, %llu as text\n", (unsigned long long)J.z_member_windows,
                (unsigned long long)J.z_text_windows);
        if (J.z_member_windows + J.z_text_windows)
            fprintf(stderr, "[timing] extract -z on the windows' devices: written form %.1f ms, cut %.1f ms, deflate %.1f ms, download %.1f ms; %llu calls repeated for a larger buffer\n",
                    J.z_ms[0], J.z_ms[1], J.z_ms[2], J.z_ms[3], (unsigned long long)J.z_repeats.load());
    }
    // (--zstd-output: the library times the cut kernel with the deflate; the frames themselves are counted in the "zstd output" row)
    if (G.timing && a.zstd_output && J.z_member_windows + J.z_text_windows)
        fprintf(stderr, "[timing] extract --zstd-output on the windows' devices: %llu windows as frames, %llu as text; written form %.1f ms, cut + deflate %.1f ms, download %.1f ms; %llu calls repeated for a larger buffer\n",
                (unsigned long long)J.z_member_windows, (unsigned long long)J.z_text_windows, J.z_ms[0], J.z_ms[2], J.z_ms[3], (unsigned long long)J.z_repeats.load());
}

}  // namespace cli
