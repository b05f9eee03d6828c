// commands.cpp -- the `extract` and `tag` drivers of the C++ host program: everything around
// the hot path (argument semantics, record I/O, log / JSON emission, summaries), restated from
// src/cmd_extract.rs:143-717 and src/cmd_tag.rs:155-689.  All matching goes through the C ABI
// (mk_extract_single / mk_extract_paired / mk_tag_records): no text is searched on the host.
#include "commands.hpp"

#include <fcntl.h>
#include <unistd.h>

#include <future>
#include <memory>
#include <mutex>

#include <algorithm>
#include <cstring>
#include <ctime>

#include <hip/hip_runtime_api.h>

#include "../../../include/merkurio_hip.h"
#include "io.hpp"
#include "extract_common.hpp"
#include "tag_host.hpp"
#include "bgzf_out.hpp"

namespace cli {

static const char *kProgram = "merkurio";
static const char *kVersion = "1.0.0";  // crate version of the reference tree (Cargo.toml:3)

// The handles of a finished command.  The program that is about to end (main.cpp: every output is flushed and closed when
// run_extract / run_tag return, then the process leaves through _exit) does not free device memory, streams and
// communicators one by one first: with the HIP runtime's own exit handlers that teardown was 0.15 s of a 0.6 s run.
static void release_matchers(const std::vector<mk_matcher *> &ms) {
    if (g_process_is_ending) return;
    for (mk_matcher *x : ms) mk_matcher_destroy(x);
}

// How the emission order of the job's hit tuples was restored (order_hits.hip): calls per path over all handles.  The
// reference's JSON `meta_information` has a fixed key set (the fixture comparators check it), so this goes to stderr: in
// timing mode always, and as a note whenever the library merge sort (path 3, the slow fallback for batches that defeat both
// binnings) ran at all -- real data should tell whether it ever does.
static void report_order_paths(const std::vector<mk_matcher *> &ms) {
    uint64_t tot[4] = {0, 0, 0, 0};
    for (mk_matcher *m : ms) {
        uint64_t c4[4] = {0, 0, 0, 0};
        if (m && mk_matcher_order_stats(m, c4) == MK_OK)
            for (int k = 0; k < 4; ++k) tot[k] += c4[k];
    }
    if (getenv("MERKURIO_TIMING"))
        fprintf(stderr, "[timing] emission-order calls: %llu without work, %llu on record bins, %llu on whole-key bins, %llu library sort\n",
                (unsigned long long)tot[0], (unsigned long long)tot[1], (unsigned long long)tot[2], (unsigned long long)tot[3]);
    if (tot[3])
        fprintf(stderr, "Note: %llu of %llu emission-order calls fell back to the library merge sort (hit tuples that defeat both binnings)\n",
                (unsigned long long)tot[3], (unsigned long long)(tot[1] + tot[2] + tot[3]));
}

// helpers::parse_pattern_list (src/helpers.rs:76-133) through the library
static Patterns load_patterns(const CommonArgs &a) {
    std::vector<uint8_t> raw;
    std::vector<uint32_t> raw_off{0};
    if (a.kmer_file) {  // the file has priority (src/helpers.rs:85-89)
        if (is_directory(*a.kmer_file))
            bail("Problem parsing pattern list.: Problem reading k-mers from file: \"" + *a.kmer_file +
                 "\": K-mer file path '" + *a.kmer_file + "' is a directory, not a file.");
        FILE *f = fopen(a.kmer_file->c_str(), "rb");
        if (!f) bail("Problem parsing pattern list.: Problem reading k-mers from file: \"" + *a.kmer_file + "\": File not found.");
        std::string content;
        char buf[65536];
        size_t n;
        while ((n = fread(buf, 1, sizeof(buf), f)) > 0) content.append(buf, n);
        fclose(f);
        uint8_t *b = nullptr;
        uint32_t *o = nullptr, cnt = 0;
        if (mk_read_kmers_from_text((const uint8_t *)content.data(), content.size(), &b, &o, &cnt) != MK_OK)
            bail(std::string("Problem parsing pattern list.: Problem reading k-mers from file: \"") + *a.kmer_file + "\": " +
                 mk_last_error());
        raw.assign(b, b + o[cnt]);
        raw_off.assign(o, o + cnt + 1);
        mk_free(b);
        mk_free(o);
    } else {
        for (auto &s : a.kmer_seq) {
            raw.insert(raw.end(), s.begin(), s.end());
            raw_off.push_back((uint32_t)raw.size());
        }
    }
    uint8_t *b = nullptr;
    uint32_t *o = nullptr, cnt = 0;
    raw.push_back(0);
    if (mk_parse_pattern_list(raw.data(), raw_off.data(), (uint32_t)raw_off.size() - 1, a.reverse_complement, a.canonical,
                              a.lowercase, a.uppercase, &b, &o, &cnt) != MK_OK)
        bail(std::string("Problem parsing pattern list.: ") + mk_last_error());
    Patterns p;
    p.bytes.assign(b, b + o[cnt]);
    p.off.assign(o, o + cnt + 1);
    for (uint32_t i = 0; i < cnt; ++i) p.list.emplace_back((const char *)b + o[i], o[i + 1] - o[i]);
    mk_free(b);
    mk_free(o);
    return p;
}

static void open_loggers(const CommonArgs &a, Loggers &lg) {
    if (a.out_log) {
        lg.text.out.reset(new Sink());
        lg.text.out->open(*a.out_log);
        if (!lg.text.out->f) bail("Problem creating log file: " + *a.out_log);
    }
    if (a.json_log) {
        lg.json.out.reset(new Sink());
        lg.json.out->open(*a.json_log);
        if (!lg.json.out->f) bail("Error creating JSON log file: " + *a.json_log);
        lg.json.begin();
        lg.has_json = true;
    }
    lg.active = a.out_log || a.json_log;
}

// the scalars of src/cmd_extract.rs:285-290 / src/cmd_tag.rs:360-364 and pattern_hit_counts of every
// device, summed by the library's RCCL all-reduce (mk_reduce_counters): the job's only collective.
// The per-device vectors are host values by the time the job ends (the driver loops keep them per batch), so
// when RCCL cannot be bound or the collective fails the same sum is taken on the host, with a warning -- a
// job whose records and log rows are already written must not end without its summary.
static void reduce_device_counters(const std::vector<mk_matcher *> &ms, const std::vector<int> &devs,
                                   const std::vector<mk_counters> &cs, const std::vector<std::vector<uint32_t>> &counts,
                                   mk_counters &c, std::vector<uint32_t> &total_counts) {
    const size_t n_pat = total_counts.size(), len = n_pat + 8;
    std::vector<std::vector<uint64_t>> vec(ms.size(), std::vector<uint64_t>(len, 0));
    for (size_t d = 0; d < ms.size(); ++d) {
        std::vector<uint64_t> &v = vec[d];
        for (size_t k = 0; k < n_pat; ++k) v[k] = counts[d][k];
        v[n_pat + 0] = cs[d].nb_records_tot; v[n_pat + 1] = cs[d].nb_bases;
        v[n_pat + 2] = cs[d].nb_hits_tot[0]; v[n_pat + 3] = cs[d].nb_hits_tot[1];
        v[n_pat + 4] = cs[d].nb_records_hit[0]; v[n_pat + 5] = cs[d].nb_records_hit[1];
        v[n_pat + 6] = cs[d].nb_records_extracted;
    }
    std::vector<uint64_t> sum(len, 0);
    std::string why;
    bool reduced = false;
    if (mk_comm_available() != MK_OK) {
        why = mk_last_error();
    } else {
        std::vector<void *> dptr(ms.size(), nullptr);
        bool ok = true;
        for (size_t d = 0; d < ms.size() && ok; ++d) {
            ok = hipSetDevice(devs[d]) == hipSuccess && hipMalloc(&dptr[d], len * sizeof(uint64_t)) == hipSuccess &&
                 hipMemcpy(dptr[d], vec[d].data(), len * sizeof(uint64_t), hipMemcpyHostToDevice) == hipSuccess;
            if (!ok) why = "device buffer for the counter vector: " + std::string(hipGetErrorString(hipGetLastError()));
        }
        if (ok) {
            reduced = mk_reduce_counters(ms.data(), (int)ms.size(), dptr.data(), len, sum.data()) == MK_OK;
            if (!reduced) why = mk_last_error();
        }
        for (size_t d = 0; d < ms.size(); ++d)
            if (dptr[d]) {
                (void)hipSetDevice(devs[d]);
                (void)hipFree(dptr[d]);
            }
    }
    if (!reduced) {
        fprintf(stderr, "Warning: per-GPU counters summed on the host (RCCL reduction unavailable: %s)\n", why.c_str());
        std::fill(sum.begin(), sum.end(), 0);
        for (auto &v : vec)
            for (size_t k = 0; k < len; ++k) sum[k] += v[k];
    }
    for (size_t k = 0; k < n_pat; ++k) total_counts[k] = (uint32_t)sum[k];
    c.nb_records_tot = sum[n_pat + 0]; c.nb_bases = sum[n_pat + 1];
    c.nb_hits_tot[0] = sum[n_pat + 2]; c.nb_hits_tot[1] = sum[n_pat + 3];
    c.nb_records_hit[0] = sum[n_pat + 4]; c.nb_records_hit[1] = sum[n_pat + 5];
    c.nb_records_extracted = sum[n_pat + 6];
}

static mk_matcher *make_matcher(const CommonArgs &a, const Patterns &p, bool *use_ac, int device = -1) {
    // src/cmd_extract.rs:166-171: -I forces AC; otherwise auto unless -q / -a were given
    bool ac = a.aho_corasick;
    if (a.case_insensitive)
        ac = true;
    else if (!a.q_size && !a.aho_corasick)
        ac = mk_recommend_aho_corasick(p.list.size(), std::max_element(p.list.begin(), p.list.end(), [](auto &x, auto &y) {
                                                          return x.size() < y.size();
                                                      })->size()) != 0;
    *use_ac = ac;
    mk_matcher *m = nullptr;
    mk_check(mk_matcher_create(p.bytes.data(), p.off.data(), (uint32_t)p.list.size(), ac ? MK_ALGO_AC : MK_ALGO_BNDMQ,
                               a.q_size ? (uint32_t)*a.q_size : 0, a.case_insensitive ? MK_FLAG_ASCII_CASE_INSENSITIVE : 0,
                               device < 0 ? a.device : device, &m),
             "Error");
    return m;
}

// --gpus N: the N handles live on devices (--device + d) mod the number of visible GPUs, so that the
// multi-device path can be rehearsed on a box with fewer GPUs (several handles then share a device)
static std::vector<int> device_list(const CommonArgs &a) {
    // (one GPU: no device query here -- the first HIP call starts the runtime, 0.2 s, and belongs on the matcher thread)
    const int avail = a.gpus > 1 ? std::max(1, mk_device_count()) : 1;
    std::vector<int> devs;
    for (int d = 0; d < std::max(1, a.gpus); ++d) devs.push_back(a.gpus > 1 ? (a.device + d) % avail : a.device);
    return devs;
}

static std::vector<mk_matcher *> make_matchers(const CommonArgs &a, const Patterns &p, const std::vector<int> &devs, bool *use_ac) {
    std::vector<mk_matcher *> ms(devs.size(), nullptr);
    try {
        run_threads(devs.size(), [&](size_t d) {
            bool ac = false;
            ms[d] = make_matcher(a, p, &ac, devs[d]);
            if (d == 0) *use_ac = ac;
        });
    } catch (...) {
        for (mk_matcher *m : ms) mk_matcher_destroy(m);
        throw;
    }
    return ms;
}

static void write_summary(TextLogger &t, const Patterns &p, const std::vector<uint32_t> &counts, const mk_counters &c,
                          bool paired) {
    // src/cmd_extract.rs:616-670 / src/cmd_tag.rs:618-647
    size_t found = 0;
    for (uint32_t x : counts) found += x > 0;
    char buf[128];
    snprintf(buf, sizeof(buf), "#\n#Number of patterns found: %zu/%zu (%.2f %%)\n", found, counts.size(),
             (double)found / (double)counts.size() * 100.0);
    t.header(buf);
    t.header("#Pattern\tCount\n");
    for (size_t i = 0; i < counts.size(); ++i) t.header("#" + p.list[i] + "\t" + std::to_string(counts[i]) + "\n");
    t.header("#\n#Total number of records searched: " + std::to_string(c.nb_records_tot) + "\n");
    t.header("#Total number of characters searched: " + std::to_string(c.nb_bases) + "\n");
    t.header("#Total number of hits: " + std::to_string(c.nb_hits_tot[0] + c.nb_hits_tot[1]) + "\n");
    t.header("#Number of distinct records with a hit: " + std::to_string(c.nb_records_hit[0] + c.nb_records_hit[1]) + "\n");
    if (paired) {
        t.header("#\n#Total number of hits in file 1: " + std::to_string(c.nb_hits_tot[0]) + "\n");
        t.header("#Total number of hits in file 2: " + std::to_string(c.nb_hits_tot[1]) + "\n");
        t.header("#Number of distinct records with a hit in file 1: " + std::to_string(c.nb_records_hit[0]) + "\n");
        t.header("#Number of distinct records with a hit in file 2: " + std::to_string(c.nb_records_hit[1]) + "\n");
        t.header("#Total number of extracted records: " + std::to_string(c.nb_records_extracted) + "\n");
    }
    t.flush();
}

// The end of a job's logs: the text log's summary and the JSON log's meta information, pattern hit counts and summary statistics
// (src/cmd_extract.rs:673-714, src/cmd_tag.rs:650-686).  The subcommands differ in input_files' record files, tag's `tag` and
// extract's paired-end object.
static void finish_logs(Loggers &lg, const CommonArgs &a, const char *subcommand, const std::vector<std::string> &argv, bool use_ac,
                        const Patterns &pats, const std::vector<uint32_t> &counts, const mk_counters &c, bool paired, Json input_files,
                        const std::string *tag, const Json *paired_end) {
    if (lg.active) {
        lg.text.flush();
        write_summary(lg.text, pats, counts, c, paired);
    }
    if (!lg.has_json) return;
    Json command_line = Json::array();
    for (auto &s : argv) command_line.push(Json::string(s));
    input_files.set("kmer_file", a.kmer_file ? Json::string(*a.kmer_file) : Json::null());
    Json meta = Json::object();
    meta.set("program", Json::string(kProgram)).set("version", Json::string(kVersion));
    meta.set("timestamp", Json::string(timestamp_now())).set("subcommand", Json::string(subcommand));
    meta.set("command_line", command_line);
    meta.set("search_algorithm", Json::string(use_ac ? "Aho-Corasick" : "BNDMq"));
    meta.set("inverted_matching", Json::boolean(a.invert_match)).set("case_insensitive", Json::boolean(a.case_insensitive));
    meta.set("input_files", input_files);
    if (tag) meta.set("tag", Json::string(*tag));
    Json cj = Json::object();
    size_t found = 0;
    for (size_t k = 0; k < counts.size(); ++k) {
        cj.set(pats.list[k], Json::integer(counts[k]));
        found += counts[k] > 0;
    }
    Json sum = Json::object();
    sum.set("number_of_patterns_searched", Json::integer((long long)pats.list.size()));
    sum.set("number_of_patterns_found", Json::integer((long long)found));
    sum.set("number_of_records_searched", Json::integer((long long)c.nb_records_tot));
    sum.set("number_of_characters_searched", Json::integer((long long)c.nb_bases));
    sum.set("number_of_matches", Json::integer((long long)(c.nb_hits_tot[0] + c.nb_hits_tot[1])));
    sum.set("number_of_distinct_records_with_a_hit", Json::integer((long long)(c.nb_records_hit[0] + c.nb_records_hit[1])));
    lg.json.finalize(meta, cj, sum, paired_end);
}
static std::string join(const std::vector<std::string> &v) {
    std::string s;
    for (size_t i = 0; i < v.size(); ++i) s += (i ? " " : "") + v[i];
    return s;
}

static void write_log_header(TextLogger &t, const char *title, const std::vector<std::string> &argv, const std::string *tag,
                             size_t n_pat, bool invert) {
    t.header(std::string("#SeqKatcher ") + title + " log\n");  // literal of src/cmd_extract.rs:232
    t.header("#" + timestamp_now() + "\n");
    t.header(std::string("#Running ") + kProgram + " version " + kVersion + "\n");
    t.header("#Command line: " + join(argv) + "\n");
    if (tag) t.header("#Tag used for labeling records: " + *tag + "\n");
    t.header("#Searching for " + std::to_string(n_pat) + " pattern" + (n_pat > 1 ? "s" : "") + " " +
             (invert ? "(inverted matching)" : "") + "\n");
    t.header("#\n#File\tRecord\tPattern\tPosition (zero-based)\n");
    t.flush();
}

// ---- extract ------------------------------------------------------------------------------------
int run_extract(const ExtractArgs &a, const std::vector<std::string> &argv) {
    const std::string conflict = check_log_flag_conflict(a.out_log ? &*a.out_log : nullptr, a.json_log ? &*a.json_log : nullptr,
                                                         a.out_fastx ? &*a.out_fastx : nullptr, a.suppress_output);
    if (!conflict.empty()) bail(conflict);
    Patterns pats = load_patterns(a);
    if (is_directory(a.in_fastx)) bail("Record file path '" + a.in_fastx + "' is a directory, not a file.");
    if (a.in_fastq_2 && is_directory(*a.in_fastq_2)) bail("Second read file path '" + *a.in_fastq_2 + "' is a directory, not a file.");
    const std::string name1 = file_name(a.in_fastx), name2 = a.in_fastq_2 ? file_name(*a.in_fastq_2) : "";
    Loggers lg;
    open_loggers(a, lg);
    if (lg.active) write_log_header(lg.text, "extract", argv, nullptr, pats.list.size(), a.invert_match);
    // (what the logs hold before any input is read -- the text log's header, the JSON log's opening: Sink::rollback cuts them back to this)
    if (lg.text.out) lg.text.out->mark();
    if (lg.has_json) lg.json.out->mark();
    PhaseTimer tm;
    bool use_ac = false;
    // HIP initialisation + pattern-set compilation (0.1-0.3 s) runs beside the input parsing
    const std::vector<int> devs = device_list(a);
    std::future<std::vector<mk_matcher *>> fm = std::async(std::launch::async, [&] { return make_matchers(a, pats, devs, &use_ac); });

    // Default: everything `extract` reads goes to the device as windows of raw text (extract_windows.cpp: FASTQ or FASTA, one file or
    // a pair, plain / gzip / bgzip'ed, one GPU or several).  --host-ingest, and inputs that path does not take, are parsed here.
    WindowExtract wx;
    bool by_windows = false;
    // The host reader: the inputs are read a window at a time (--window-mb of text, decompressed if need be): the host holds
    // one window and its record index, like the reference, which streams records.
    FastxStream s1, s2;
    FastxFile &f1 = s1.view, &f2 = s2.view;
    const bool paired = (bool)a.in_fastq_2;
    const uint64_t window_bytes = (uint64_t)a.window_mb << 20;
    bool more1 = false, more2 = false;
    try {
        by_windows = !a.host_ingest && wx.prepare(a, devs);
        if (!by_windows) {
            s1.open(a.in_fastx);
            if (paired) s2.open(*a.in_fastq_2);
            more1 = s1.fill(window_bytes);
            if (paired) more2 = s2.fill(window_bytes);
        }
    } catch (...) {
        fm.get();  // a matcher error comes first, as in the serial order of the reference
        throw;
    }
    tm.mark("open + first window");
    const std::vector<mk_matcher *> ms = fm.get();
    mk_matcher *m = ms[0];
    // --gpus N: RCCL's communicators for the final counter reduction are set up beside the job (seconds, against a job of one)
    std::future<void> comm_ready;
    if (ms.size() > 1) comm_ready = std::async(std::launch::async, [&ms] { (void)mk_reduce_prepare(ms.data(), (int)ms.size()); });
    // from here on (the HIP runtime is up) the members of a bgzip'ed input are inflated by the device codec (mk_bgzf_inflate)
    if (!a.host_codec) set_bgzf_device(devs[0], a.device_codec_always);
    tm.mark("matcher create (HIP init), remainder");
    // writers: src/cmd_extract.rs:297-318, :420-460
    Sink w1, w2;
    if (a.out_fastx) {
        std::string p = with_extension(*a.out_fastx, identify_uncompressed_type(a.in_fastx));
        if (a.bgzf_output) p += ".gz";  // (-z; the reference never compresses: its name is the derived one)
        if (a.zstd_output) p += ".zst";
        if (paired) {
            w1.open(add_suffix_to_file_prefix(p, "_1"));
            w2.open(add_suffix_to_file_prefix(p, "_2"));
            if (!w1.f || !w2.f) bail("Error writing to paired-end file; no such directory: \"" + p + "\"");
        } else {
            w1.open(p);
            if (!w1.f) bail("Error writing to output file; no such directory: \"" + p + "\"");
        }
    } else {
        w1.open("STDOUT");
        if (paired) w2.open("STDOUT");
    }
    // -z: what the sinks are given leaves as BGZF members that end at record ends
    RecordGzip z1, z2;
    if (a.bgzf_output || a.zstd_output) {  // (--zstd-output: as zstd frames; what gathers here is compressed on the first device)
        z1.attach(w1, a.host_codec ? -1 : devs[0], a.zstd_output);
        if (paired) z2.attach(w2, a.host_codec ? -1 : devs[0], a.zstd_output);
    }

    mk_counters c;
    memset(&c, 0, sizeof(c));
    std::vector<uint32_t> counts(pats.list.size(), 0);
    const uint64_t batch_bytes = (uint64_t)a.batch_mb << 20;
    // what a batch's results turn into: log rows (reference emission order) and the kept records
    auto emit_rows = [&](size_t b0, const mk_row *rows, uint64_t n_rows) {
        emit_log_rows(
            lg, pats, rows, n_rows,
            [&](const mk_row &r) {
                const FastxFile &ff = r.file ? f2 : f1;
                const auto &rec = ff.recs[b0 + r.rec];
                return std::pair<const char *, size_t>(ff.data + rec.id_b, rec.id_e - rec.id_b);
            },
            [&](const mk_row &r) -> const std::string & { return r.file ? name2 : name1; });
    };
    auto emit_records = [&](size_t b0, const uint8_t *keep, uint64_t nb) {
        if (a.suppress_output) return;
        for (uint64_t k = 0; k < nb; ++k)
            if (keep[k]) {
                f1.write(b0 + k, w1);
                w1.end_record();
                if (paired) f2.write(b0 + k, w2), w2.end_record();
            }
        w1.window_done(), w2.window_done();
    };
    // Scans records [r0, r1) on matcher `mm` in double-buffered batches: while batch k is on the GPU
    // and its results are consumed, a second thread gathers the sequences of batch k + 1.
    // on_batch(first record, #records, keep, rows, #rows) is called in record order.
    // batch buffers of one device thread; they live as long as the job (a fresh 128 MB buffer costs its page
    // faults again: 30 ms per batch instead of 4)
    struct Batch {
        size_t b0 = 0, b1 = 0;
        std::vector<uint8_t> s1, s2;
        std::vector<uint64_t> o1, o2;
    };
    struct DevBuffers {
        Batch bufs[2];
        std::vector<uint8_t> keep;
        std::vector<mk_row> rows = std::vector<mk_row>(4096);
    };
    std::vector<DevBuffers> dev_bufs(ms.size());
    double call_ms[4] = {0, 0, 0, 0};  // MERKURIO_TIMING: phases inside mk_extract_single / _paired, summed (one device)
    auto scan_range = [&](mk_matcher *mm, DevBuffers &DB, size_t r0, size_t r1, mk_counters &cc, std::vector<uint32_t> &cnts, auto on_batch) {
        Batch(&bufs)[2] = DB.bufs;
        std::vector<uint8_t> &keep = DB.keep;
        std::vector<mk_row> &rows = DB.rows;
        auto fill = [&](Batch &b, size_t from) {
            size_t i = from;
            uint64_t bytes = 0;
            while (i < r1 && (bytes < batch_bytes || i == from)) {
                bytes += f1.raw_len(i) + (paired ? f2.raw_len(i) : 0);
                ++i;
            }
            b.b0 = from;
            b.b1 = i;
            f1.gather(from, i, b.s1, b.o1);
            if (paired) f2.gather(from, i, b.s2, b.o2);
        };
        int cur = 0;
        bufs[0].b0 = r1;
        if (r0 < r1) fill(bufs[0], r0);
        while (bufs[cur].b0 < r1) {
            Batch &B = bufs[cur];
            const size_t b0 = B.b0, i = B.b1;
            std::future<void> next;
            Batch &N = bufs[cur ^ 1];
            N.b0 = r1;  // "no further batch" unless filled below
            if (i < r1) next = std::async(std::launch::async, [&, i] { fill(N, i); });
            const uint64_t nb = i - b0;
            keep.assign(nb, 0);
            uint64_t n_rows = 0;
            try {
                for (;;) {
                    mk_counters cb;
                    memset(&cb, 0, sizeof(cb));
                    std::vector<uint32_t> cnt_b(cnts.size(), 0);
                    int rc = paired ? mk_extract_paired(mm, B.s1.data(), B.o1.data(), nb, B.s2.data(), B.o2.data(), nb, lg.active,
                                                        a.invert_match, keep.data(), rows.data(), rows.size(), &n_rows, &cb, cnt_b.data())
                                    : mk_extract_single(mm, B.s1.data(), B.o1.data(), nb, lg.active, a.invert_match, keep.data(),
                                                        rows.data(), rows.size(), &n_rows, &cb, cnt_b.data());
                    if (rc == MK_E_CAPACITY && n_rows > rows.size()) {
                        rows.resize(n_rows);
                        continue;
                    }
                    mk_check(rc, "Error during matching");
                    if (tm.on && ms.size() == 1) {  // where the call itself spent its time: upload / device / download / host loop
                        float ms4[4] = {0, 0, 0, 0};
                        if (mk_matcher_batch_times(mm, ms4) == MK_OK)
                            for (int k = 0; k < 4; ++k) call_ms[k] += ms4[k];
                    }
                    add_counters(cc, cb);
                    add_counts(cnts, cnt_b);
                    break;
                }
                on_batch(b0, nb, keep.data(), rows.data(), lg.active ? n_rows : 0);
            } catch (...) {
                if (next.valid()) next.wait();  // the gather thread still writes into this frame
                throw;
            }
            if (next.valid()) next.get();
            cur ^= 1;
        }
    };
    // per-device counters of a --gpus N job (summed once, at the end, by RCCL)
    std::vector<mk_counters> dev_c(ms.size());
    std::vector<std::vector<uint32_t>> dev_counts(ms.size(), std::vector<uint32_t>(counts.size(), 0));
    for (auto &x : dev_c) memset(&x, 0, sizeof(x));
    if (by_windows) {
        wx.run(a, pats, lg, ms, devs, w1, w2, name1, name2, dev_c, dev_counts, tm);
        if (ms.size() == 1) {
            c = dev_c[0];
            counts = dev_counts[0];
        }
    }
    while (more1 || more2) {
        if (paired && !more2)  // src/cmd_extract.rs:465-468: file 2 ends first
            bail("Error during FASTQ record parsing of second file. Do the two input files contain the same number of records?");
        if (paired && !more1)  // src/cmd_extract.rs:608-612: file 2 still has records
            bail("The two input files have a different number of records. Please provide valid paired-end read files.");
        // pairs are matched by ordinal: both windows advance by the same number of records
        const size_t n = paired ? std::min(f1.recs.size(), f2.recs.size()) : f1.recs.size();
        // the next window is inflated and indexed while this one is scanned
        s1.consume(n);
        if (paired) s2.consume(n);
        std::future<void> next_window = std::async(std::launch::async, [&] {
            s1.prefetch(window_bytes);
            if (paired) s2.prefetch(window_bytes);
        });
        try {
        if (ms.size() == 1) {
            scan_range(m, dev_bufs[0], 0, n, c, counts, [&](size_t b0, uint64_t nb, const uint8_t *keep, const mk_row *rows, uint64_t n_rows) {
                tm.mark("batch: gather + H2D + scan + D2H");
                emit_rows(b0, rows, n_rows);
                emit_records(b0, keep, nb);
                tm.mark("batch: rows + records out");
            });
        } else {
            // --gpus N: device d scans a contiguous record (pair) range of the window
            struct Shard {
                size_t r0 = 0, r1 = 0;
                std::vector<uint8_t> keep;
                std::vector<mk_row> rows;  // rec = index inside the shard
            };
            std::vector<Shard> shards = run_shards<Shard>(n, ms.size(), [&](size_t d, size_t lo, size_t hi, Shard &S) {
                S.r0 = lo, S.r1 = hi;
                S.keep.assign(hi - lo, 0);
                scan_range(ms[d], dev_bufs[d], lo, hi, dev_c[d], dev_counts[d],
                           [&](size_t b0, uint64_t nb, const uint8_t *keep, const mk_row *rows, uint64_t n_rows) {
                               memcpy(S.keep.data() + (b0 - lo), keep, nb);
                               for (uint64_t k = 0; k < n_rows; ++k) {
                                   mk_row r = rows[k];
                                   r.rec += b0 - lo;
                                   S.rows.push_back(r);
                               }
                           });
            });
            tm.mark("window: scan on all devices");
            for (auto &S : shards) {
                emit_rows(S.r0, S.rows.data(), S.rows.size());
                emit_records(S.r0, S.keep.data(), S.r1 - S.r0);
            }
        }
        } catch (...) {
            next_window.wait();  // it works on s1 / s2
            throw;
        }
        next_window.get();  // a malformed record in the next window is reported now, after this one was written
        more1 = s1.fill(window_bytes);
        if (paired) more2 = s2.fill(window_bytes);
        tm.mark("next window");
    }
    if (ms.size() > 1) {
        tm.mark("records done");
        comm_ready.get();
        reduce_device_counters(ms, devs, dev_c, dev_counts, c, counts);
        tm.mark("counter reduction (RCCL set-up began with the job)");
    }
    z1.finish(), z2.finish();
    w1.flush();
    w2.flush();
    tm.mark("log rows + write records");
    if (tm.on && a.bgzf_output)
        fprintf(stderr, "[timing] BGZF output (%s): %llu members written, cut %.1f ms, deflate %.1f ms, download %.1f ms\n", a.host_codec ? "zlib, host" : "device codec",
                (unsigned long long)(z1.members + z2.members), z1.cut_ms + z2.cut_ms, z1.deflate_ms + z2.deflate_ms, z1.download_ms + z2.download_ms);
    if (tm.on && a.zstd_output)
        fprintf(stderr, "[timing] zstd output (%s): %llu frames written, blocks raw %llu rle %llu compressed %llu, upload %.1f ms, cut + deflate %.1f ms, download %.1f ms (of the gathering path); %llu frames from the window path, %llu from the gathering path\n",
                a.host_codec ? "libzstd, host" : "device codec", (unsigned long long)(z1.members + z2.members), (unsigned long long)(z1.kinds[0] + z2.kinds[0]),
                (unsigned long long)(z1.kinds[1] + z2.kinds[1]), (unsigned long long)(z1.kinds[2] + z2.kinds[2]), z1.upload_ms + z2.upload_ms,
                z1.deflate_ms + z2.deflate_ms, z1.download_ms + z2.download_ms, (unsigned long long)(z1.window_members + z2.window_members),
                (unsigned long long)(z1.members + z2.members - z1.window_members - z2.window_members));
    if (tm.on && (call_ms[0] + call_ms[1] + call_ms[2] + call_ms[3]) > 0)
        fprintf(stderr, "[timing] inside the batch calls: upload %.3f s, device %.3f s, download %.3f s, host loop %.3f s\n", call_ms[0] * 1e-3,
                call_ms[1] * 1e-3, call_ms[2] * 1e-3, call_ms[3] * 1e-3);
    report_order_paths(ms);
    Json files = Json::object(), pe = Json::object();
    files.set("record_file_1", Json::string(name1)).set("record_file_2", paired ? Json::string(name2) : Json::null());
    pe.set("searching_paired_end_reads", Json::boolean(paired));
    pe.set("number_of_hits_in_file_1", Json::integer((long long)c.nb_hits_tot[0]));
    pe.set("number_of_hits_in_file_2", paired ? Json::integer((long long)c.nb_hits_tot[1]) : Json::null());
    pe.set("number_of_distinct_records_with_a_hit_in_file_1", Json::integer((long long)c.nb_records_hit[0]));
    pe.set("number_of_distinct_records_with_a_hit_in_file_2", paired ? Json::integer((long long)c.nb_records_hit[1]) : Json::null());
    pe.set("number_of_extracted_records", Json::integer((long long)c.nb_records_extracted));
    finish_logs(lg, a, "extract", argv, use_ac, pats, counts, c, paired, files, nullptr, &pe);
    release_matchers(ms);
    return 0;
}

// ---- tag ----------------------------------------------------------------------------------------
int run_tag(const TagArgs &a, const std::vector<std::string> &argv) {
    const std::string conflict = check_log_flag_conflict(a.out_log ? &*a.out_log : nullptr, a.json_log ? &*a.json_log : nullptr,
                                                         a.out_file ? &*a.out_file : nullptr, a.suppress_output);
    if (!conflict.empty()) bail(conflict);
    if (is_directory(a.in_file)) bail("Record file path '" + a.in_file + "' is a directory, not a file.");
    const std::string in_name = file_name(a.in_file);
    Patterns pats = load_patterns(a);
    if (a.threads < 1) bail("Number of threads must be at least 1.");
    if (a.threads_given) set_io_threads_cap((unsigned)a.threads);
    if (a.tag.size() != 2) bail("Tag must be exactly two characters long.");
    Loggers lg;
    open_loggers(a, lg);
    // extension logic: src/cmd_tag.rs:293-308
    const std::string in_ext = extension(a.in_file);
    if (in_ext.empty()) bail("Could not detect the file extension: \"" + a.in_file + "\"");
    std::string out_ext = "STDOUT";
    if (a.out_file) {
        out_ext = extension(*a.out_file);
        if (out_ext.empty()) out_ext = in_ext;
    }
    if (lg.active) write_log_header(lg.text, "tag", argv, &a.tag, pats.list.size(), a.invert_match);
    bool use_ac = false;
    PhaseTimer tm;
    const std::vector<int> devs = device_list(a);
    std::future<std::vector<mk_matcher *>> fm = std::async(std::launch::async, [&] { return make_matchers(a, pats, devs, &use_ac); });

    SamFile sam;
    try {
        if (a.device_codec_always && !a.host_codec) {  // (the header's members too: the HIP runtime has to be up first)
            fm.wait();
            set_bgzf_device(devs[0], true);
        }
        sam.open(a.in_file);  // "Input file must be a BAM or SAM file." for other extensions; header only
    } catch (...) {
        fm.get();  // a matcher error comes first, as in the serial order of the reference
        throw;
    }
    tm.mark("open + header");
    const std::vector<mk_matcher *> ms = fm.get();
    std::future<void> comm_ready;  // (--gpus N: RCCL's set-up beside the job, as in extract)
    if (ms.size() > 1) comm_ready = std::async(std::launch::async, [&ms] { (void)mk_reduce_prepare(ms.data(), (int)ms.size()); });
    // from here on (the HIP runtime is up) the BGZF members of a BAM window are inflated by the device codec (mk_bgzf_inflate)
    if (!a.host_codec) set_bgzf_device(devs[0], a.device_codec_always);
    tm.mark("matcher (HIP init), remainder");
    if (out_ext != "sam" && out_ext != "bam" && out_ext != "STDOUT") bail("Output file must be a BAM or SAM file.");
    Sink w;
    BamWriter bw;
    const bool to_bam = out_ext == "bam" && !a.suppress_output;
    // header + @PG line (src/cmd_tag.rs:509-514)
    const std::string out_header =
        sam.header + "@PG\tID:" + kProgram + "\tPN:" + kProgram + "\tCL:" + join(argv) + "\tVN:" + kVersion + "\n";
    if (to_bam && !a.host_codec) bw.use_device(devs[0]);  // members deflated by the device codec (mk_bgzf_deflate)
    if (to_bam) {  // BAM -> BAM passes raw records through: they keep the input's reference ids
        if (sam.is_bam)
            bw.open(with_extension(*a.out_file, out_ext), out_header, &sam.ref_names, &sam.ref_lens);
        else
            bw.open(with_extension(*a.out_file, out_ext), out_header);
    } else if (!a.suppress_output) {
        w.open(out_ext == "STDOUT" ? "STDOUT" : with_extension(*a.out_file, out_ext));
        if (!w.f) bail("Error writing SAM file: " + with_extension(*a.out_file, out_ext));
        w.write(out_header);
    }

    mk_counters c;
    memset(&c, 0, sizeof(c));
    std::vector<uint32_t> counts(pats.list.size(), 0);
    const uint64_t window_bytes = (uint64_t)a.window_mb << 20;
    // per-device counters of a --gpus N job (summed once, at the end, by RCCL)
    std::vector<mk_counters> dev_c(ms.size());
    std::vector<std::vector<uint32_t>> dev_counts(ms.size(), std::vector<uint32_t>(counts.size(), 0));
    for (auto &x : dev_c) memset(&x, 0, sizeof(x));
    // the host loop (tag_host.cpp): the whole input where no window path applies, the rest of it where one handed over, and single
    // windows the device refused in between (tag_windows.cpp)
    std::vector<TagHandle> host_handles;
    for (size_t d = 0; d < ms.size(); ++d)
        host_handles.push_back(TagHandle{ms[d], devs[d], ms.size() == 1 ? &c : &dev_c[d], ms.size() == 1 ? &counts : &dev_counts[d]});
    TagHostLoop host(a, sam, lg, pats, in_name, w, bw, to_bam, tm, host_handles);
    bool device_done = false;
    // BAM -> BAM (or no output at all): the records stay on the device between inflate and deflate
    // (tag_windows.cpp; two windows per device in flight, each on a handle of its own); false: a window was not for the device and the
    // loop below takes the input from there
    std::vector<mk_matcher *> seconds;
    const bool bam_windows = sam.bam_on_bgzf() && (to_bam || a.suppress_output) && !a.host_codec && !a.host_ingest;
    // BAM -> SAM text / STDOUT: the same windows, whose kept records come back as SAM lines formatted on the device
    // (tag_bam_sam_windows_on_device); --host-ingest keeps the host loop
    const bool bam_sam_windows = sam.bam_on_bgzf() && !to_bam && !a.suppress_output && !a.host_codec && !a.host_ingest;
    // SAM text -> SAM text / STDOUT (or no output at all) from a memory-mapped file: the lines stay on the device between the upload and
    // the download of the kept ones (tag_windows.cpp: tag_sam_windows_on_device; windows cut at line starts, independent of each other)
    // SAM text -> BAM goes the same way with the kept lines encoded as BAM records and deflated on the device (tag_sam_bam_windows_on_device)
    const bool sam_windows = sam.sam_on_mapping() && !a.host_ingest && !(to_bam && a.host_codec);
    if (bam_windows || bam_sam_windows || sam_windows) {
        if (to_bam) bw.use_device(devs[0]);
        // BAM: 240 MiB of text -- the tagged records of a window then fill one round of the deflate kernel's 4 096 resident waves, not one
        // and a bit.  SAM (to SAM and to BAM alike: the input side is the same): 64 MiB, the fastest of the 64 / 128 / 240 / 512 sweep (profiles/e2e_tag_sam_window.txt): the windows are
        // independent, so small ones cost nothing but launches, and their page-locked staging buffers stay small.
        // (an explicit --window-mb is honoured up to 2 GiB: a window's text, head included, has to stay below 4 GiB on the device)
        const uint64_t dev_window = a.window_mb_given ? std::min<uint64_t>(window_bytes, 2048ull << 20) : ((bam_windows || bam_sam_windows ? 240ull : 64ull) << 20);
        // (a SAM text that is one window needs no second handle; BAM windows are not known before their members are walked)
        const bool one_window = sam_windows && sam.source().text_size() - sam.text_cursor() <= dev_window;
        seconds.assign(ms.size(), nullptr);
        if (!one_window)
            run_threads(ms.size(), [&](size_t d) {
                bool ac2 = false;
                seconds[d] = make_matcher(a, pats, &ac2, devs[d]);
            });
        // window k runs on handle k mod 2N: devices in turn, and two windows per device in flight.  One device: the job's counters;
        // several: the per-device vectors that RCCL sums at the end
        std::vector<TagHandle> handles;
        for (int rep = 0; rep < (one_window ? 1 : 2); ++rep)
            for (size_t d = 0; d < ms.size(); ++d)
                handles.push_back(TagHandle{rep ? seconds[d] : ms[d], devs[d], ms.size() == 1 ? &c : &dev_c[d], ms.size() == 1 ? &counts : &dev_counts[d]});
        // (a window the device refuses is the host loop's, with the handle of the worker that had it)
        const HostTurn turn = [&](const TagHandle &h) { host.run(&h); };
        device_done = bam_windows       ? tag_bam_windows_on_device(a, sam, handles, lg, pats, in_name, to_bam ? &bw : nullptr, dev_window, turn)
                      : bam_sam_windows ? tag_bam_sam_windows_on_device(a, sam, handles, lg, pats, in_name, w, dev_window, turn)
                      : to_bam          ? tag_sam_bam_windows_on_device(a, sam, handles, lg, pats, in_name, bw, dev_window, turn)
                                        : tag_sam_windows_on_device(a, sam, handles, lg, pats, in_name, a.suppress_output ? nullptr : &w, dev_window, turn);
        tm.mark(device_done ? "windows on the device" : "windows on the device (the rest: host reader)");
    }
    if (!device_done) host.run();
    if (ms.size() > 1) {
        comm_ready.get();
        reduce_device_counters(ms, devs, dev_c, dev_counts, c, counts);
        tm.mark("counter reduction");
    }
    w.flush();
    bw.close();
    tm.mark("write");
    if (to_bam && getenv("MERKURIO_TIMING"))
        fprintf(stderr, "[timing] BGZF deflate on its own threads (%s): %.3f s\n", a.host_codec ? "zlib, host" : "device codec", bw.deflate_seconds);
    if (getenv("MERKURIO_TIMING") && bgzf_device_seconds() > 0)
        fprintf(stderr, "[timing] BGZF inflate calls of the device codec (inside the window reads): %.3f s\n", bgzf_device_seconds());
    report_order_paths(ms);
    Json files = Json::object();
    files.set("record_file_1", Json::string(in_name));
    finish_logs(lg, a, "tag", argv, use_ac, pats, counts, c, false, files, &a.tag, nullptr);
    release_matchers(ms);
    release_matchers(seconds);
    return 0;
}

}  // namespace cli
