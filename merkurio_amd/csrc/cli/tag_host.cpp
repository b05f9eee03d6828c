// tag_host.cpp -- see tag_host.hpp
#include "tag_host.hpp"

#include <cstring>
#include <future>

namespace cli {

void TagHostLoop::emit(BatchOut &o) {  // (takes the batch's encoded records with it)
    if (lg.active)
        emit_log_rows(
            lg, pats, o.rows.data(), o.rows.size(),
            [&](const mk_row &r) {
                const auto &rec = sam.recs[r.rec];
                return std::pair<const char *, size_t>(sam.data + rec.off + (sam.is_bam ? 36 : 0), rec.name_len);
            },
            [&](const mk_row &) -> const std::string & { return in_name; });
    for (auto &b : o.bin) bw.put_encoded(std::move(b));  // moved, not copied: the pieces are joined on the device
    for (auto &t : o.txt) w.write(t);
    {  // the text buffers go back to the encoder threads (pages mapped: a fresh one costs a fault per 4 KiB)
        std::lock_guard<std::mutex> lk(txt_pool_mu);
        for (auto &t : o.txt)
            if (t.capacity() >= (1u << 20) && txt_pool.size() < 64) {
                t.clear();
                txt_pool.push_back(std::move(t));
            }
    }
}

// Inside a window, one batch = a slab of records whose sequences fill --batch-mb: gather (upper-case / un-nibble) -> mk_tag_records
// -> log rows -> tag + encode the kept records.  Only the input buffer and its record index are the window's; device buffers, hit
// rows and matched-pattern sets are per batch.
template <class OnBatch>
void TagHostLoop::scan_range(const TagHandle &h, TagBuffers &TB, size_t r0, size_t r1, size_t enc_threads, PhaseTimer &pt, OnBatch on_batch) {
    const uint64_t batch_bytes = (uint64_t)a.batch_mb << 20;
    const bool marks = devices.size() == 1;
    mk_matcher *mm = h.m;
    std::vector<uint8_t> &seq = TB.seq, &keep = TB.keep;
    std::vector<uint64_t> &off = TB.off, &foff = TB.foff;
    std::vector<uint32_t> &fpat = TB.fpat;
    std::vector<mk_row> &rows = TB.rows;
    for (size_t b0 = r0; b0 < r1;) {
        size_t b1 = b0;
        uint64_t bytes = 0;
        while (b1 < r1 && (bytes < batch_bytes || b1 == b0)) bytes += sam.recs[b1++].l_seq;
        const size_t nb = b1 - b0;
        sam.gather(b0, b1, seq, off);
        if (marks) pt.mark("  batch: gather");
        keep.assign(nb, 0);
        foff.assign(nb + 1, 0);
        uint64_t n_rows = 0;
        for (;;) {
            mk_counters cb;
            memset(&cb, 0, sizeof(cb));
            std::vector<uint32_t> cnt_b(h.pattern_counts->size(), 0);
            int rc = mk_tag_records(mm, seq.data(), off.data(), nb, lg.active, a.filter_matching, a.invert_match, keep.data(), rows.data(), rows.size(),
                                    &n_rows, &cb, cnt_b.data(), foff.data(), fpat.data(), fpat.size());
            if (rc == MK_E_CAPACITY && (n_rows > rows.size() || foff[nb] > fpat.size())) {
                rows.resize(std::max<uint64_t>(rows.size(), n_rows));
                fpat.resize(std::max<uint64_t>(fpat.size(), foff[nb]));
                continue;
            }
            mk_check(rc, "Error during matching");
            add_counters(*h.counters, cb);
            add_counts(*h.pattern_counts, cnt_b);
            break;
        }
        if (marks) pt.mark("  batch: mk_tag_records");
        BatchOut out;
        if (lg.active) {
            out.rows.assign(rows.begin(), rows.begin() + n_rows);
            for (auto &r : out.rows) r.rec += b0;
        }
        // tag + encode the kept records (src/cmd_tag.rs:457-497) on the host threads, in record order
        std::vector<size_t> kept;
        for (size_t k = 0; k < nb; ++k)
            if (keep[k]) kept.push_back(k);
        if (a.suppress_output) {  // the reference still validates existing tags of kept records
            for (size_t k : kept) {
                std::string existing;
                if (sam.find_tag(b0 + k, a.tag, &existing) == 2) bail("Invalid tag value format. Expected string value.");
            }
        } else {
            const size_t T = std::max<size_t>(1, std::min<size_t>(enc_threads, kept.size() / 4096 + 1));
            out.bin.resize(to_bam ? T : 0);
            out.txt.resize(to_bam ? 0 : T);
            run_threads(T, [&](size_t t) {
                std::vector<char> val(4096);
                std::string line;
                {  // one allocation for the slice's output instead of a doubling series of copies
                    size_t est = 0;
                    for (size_t i = kept.size() * t / T; i < kept.size() * (t + 1) / T; ++i) est += sam.recs[b0 + kept[i]].len + 24 + a.tag.size();
                    if (to_bam) {
                        out.bin[t] = bw.take_buffer();  // (one the writer thread has written out, if there is one)
                        out.bin[t].reserve(est);
                    } else {
                        {
                            std::lock_guard<std::mutex> lk(txt_pool_mu);
                            if (!txt_pool.empty()) {
                                out.txt[t] = std::move(txt_pool.back());
                                txt_pool.pop_back();
                            }
                        }
                        out.txt[t].reserve(est);
                    }
                }
                for (size_t i = kept.size() * t / T; i < kept.size() * (t + 1) / T; ++i) {
                    const size_t k = kept[i], g = b0 + k;
                    std::string existing;
                    const int has = sam.find_tag(g, a.tag, &existing);
                    if (has == 2) bail("Invalid tag value format. Expected string value.");
                    size_t need = 0;
                    for (;;) {
                        int rc = mk_tag_value(mm, fpat.data() + foff[k], foff[k + 1] - foff[k], has == 1 ? existing.c_str() : nullptr, val.data(), val.size(),
                                              &need);
                        if (rc == MK_E_CAPACITY) {
                            val.resize(need + 1);
                            continue;
                        }
                        mk_check(rc, "Error building tag value");
                        break;
                    }
                    if (to_bam && sam.is_bam) {
                        BamWriter::append_tagged_raw(sam.raw(g), sam.raw_len(g), a.tag, val.data(), need, out.bin[t]);
                    } else if (to_bam) {
                        line.clear();
                        sam.append_line(g, line);
                        line += '\t';
                        line += a.tag;
                        line += ":Z:";
                        line.append(val.data(), need);
                        bw.encode_record(line, out.bin[t]);
                    } else {
                        std::string &o = out.txt[t];
                        sam.append_line(g, o);
                        o += '\t';
                        o += a.tag;
                        o += ":Z:";
                        o.append(val.data(), need);
                        o += '\n';
                    }
                }
            });
        }
        if (marks) pt.mark("  batch: tag values + encode");
        on_batch(std::move(out));
        b0 = b1;
    }
}

void TagHostLoop::run(const TagHandle *turn) {
    const uint64_t window_bytes = (uint64_t)a.window_mb << 20;
    // (a window's turn runs on a worker thread between the caller's marks: it prints no rows of its own and leaves the job's timer alone)
    PhaseTimer quiet;
    quiet.on = false;
    PhaseTimer &t = turn ? quiet : tm;
    // (the first window is small: nothing can run beside its read; the later, large ones are read beside their predecessors)
    bool more_windows = sam.fill(std::min<uint64_t>(window_bytes, 128ull << 20));
    while (more_windows) {
        const size_t n = sam.recs.size();
        t.mark("window: read (inflate) + index");
        // the next window of a compressed input is inflated (device codec: the host threads are free for the batches
        // below) and indexed beside this one; an error in it is reported after this window was written
        std::future<void> next_window = std::async(std::launch::async, [&] { sam.prefetch(window_bytes); });
        try {
            if (turn || devices.size() == 1) {
                scan_range(turn ? *turn : devices[0], turn ? turn_bufs : dev_bufs[0], 0, n, io_threads(), t, [&](BatchOut &&o) {
                    emit(o);
                    t.mark("  batch: rows + write");
                });
            } else {
                // --gpus N: device d scans and tags a contiguous record range of the window
                auto outs = run_shards<std::vector<BatchOut>>(n, devices.size(), [&](size_t d, size_t lo, size_t hi, std::vector<BatchOut> &out) {
                    scan_range(devices[d], dev_bufs[d], lo, hi, std::max<size_t>(1, io_threads() / devices.size()), t,
                               [&](BatchOut &&o) { out.push_back(std::move(o)); });
                });
                t.mark("window: scan + tag on all devices");
                for (auto &v : outs)
                    for (auto &o : v) emit(o);
            }
        } catch (...) {
            next_window.wait();  // it works on sam
            throw;
        }
        t.mark("window done");
        next_window.get();
        more_windows = sam.fill(window_bytes);
    }
}

}  // namespace cli
