// tag_host.hpp -- the host loop of `merkurio tag` (the reader loop, process_record and the writers of src/cmd_tag.rs:387-615): the input
// is read a window at a time through SamFile::fill, a window's records go to the matcher in batches (SamFile::gather ->
// mk_tag_records), the kept ones are tagged and written as SAM lines (SamFile::append_line), as BAM records encoded from those lines
// (BamWriter::encode_record) or as the raw records they came as (BamWriter::append_tagged_raw).  The loop runs FROM WHERE `sam`
// STANDS TO WHERE IT ENDS: the whole file (--host-ingest, --host-codec, inputs the device takes no windows of), the rest of a file
// (SamFile::seek_text / seek_bam without an end), or one window that the device refused (the same calls with an end: tag_windows.cpp).
#pragma once
#include <mutex>
#include <string>
#include <vector>

#include "extract_common.hpp"

namespace cli {

struct TagHostLoop {
    const TagArgs &a;
    SamFile &sam;
    Loggers &lg;
    const Patterns &pats;
    const std::string &in_name;
    Sink &w;        // SAM text output (open unless to_bam or -S)
    BamWriter &bw;  // BAM output (open if to_bam)
    bool to_bam;
    PhaseTimer &tm;
    // the job's matchers with where their records are counted: one (the job's counters), or one per device of a --gpus N job, which
    // shares a window's records among them (per-device counters, summed by the caller at the end)
    std::vector<TagHandle> devices;

    TagHostLoop(const TagArgs &a_, SamFile &sam_, Loggers &lg_, const Patterns &pats_, const std::string &in_name_, Sink &w_, BamWriter &bw_, bool to_bam_,
                PhaseTimer &tm_, std::vector<TagHandle> devices_)
        : a(a_), sam(sam_), lg(lg_), pats(pats_), in_name(in_name_), w(w_), bw(bw_), to_bam(to_bam_), tm(tm_), devices(std::move(devices_)),
          dev_bufs(devices.size()) {}
    // Every record from where `sam` stands to where it ends, in record order: log rows, then the kept records.  turn: not the job's
    // matchers but this handle alone, counted where it says (a window's turn inside tag_windows.cpp: the handle is the window's
    // worker's own, the other handles are busy with the windows behind; no [timing] rows).  Ends with bail() on the reference's errors.
    void run(const TagHandle *turn = nullptr);

   private:
    // The results of a batch: its log rows and the encoded output of its kept records, in record order.
    struct BatchOut {
        std::vector<mk_row> rows;               // rec = record index in the window
        std::vector<std::vector<uint8_t>> bin;  // BAM output: per-thread encoded records, in order
        std::vector<std::string> txt;           // SAM output
    };
    // scan buffers of one device thread, reused by every batch of every window
    struct TagBuffers {
        std::vector<uint8_t> seq, keep;
        std::vector<uint64_t> off, foff;
        std::vector<uint32_t> fpat = std::vector<uint32_t>(1024);
        std::vector<mk_row> rows = std::vector<mk_row>(4096);
    };
    std::vector<TagBuffers> dev_bufs;
    TagBuffers turn_bufs;
    std::mutex txt_pool_mu;
    std::vector<std::string> txt_pool;
    void emit(BatchOut &o);
    template <class OnBatch>
    void scan_range(const TagHandle &h, TagBuffers &TB, size_t r0, size_t r1, size_t enc_threads, PhaseTimer &pt, OnBatch on_batch);
};

}  // namespace cli
