// sam_in.hpp -- SAM / BAM input of the `merkurio` CLI.  Observable behaviour follows what the reference gets from bam 0.1.4
// (src/cmd_tag.rs:470-497,503-615).
#pragma once
#include "window_source.hpp"

namespace cli {

// A whole SAM or BAM input held as ONE buffer (mmap of the text / inflated BAM); records are
// index entries into it, nothing is copied or converted until it is needed: sequences are
// gathered (upper-cased / un-nibbled) straight into the concatenated scan buffer, SAM text of a
// BAM record is produced only for records that are written as text, and BAM -> BAM output passes
// the raw record through with the new tag appended (as the reference's bam crate does).
struct SamFile {
    std::string header;  // header text, every line '\n'-terminated
    const char *data = nullptr;  // the current window (whole text for a memory-mapped SAM)
    bool is_bam = false;
    std::vector<std::string> ref_names;  // BAM: reference dictionary of the binary header
    std::vector<uint32_t> ref_lens;
    struct Rec {
        uint64_t off;      // SAM: start of the text line; BAM: the record's block_size field
        uint32_t len;      // SAM: line length without line end; BAM: 4 + block_size
        uint32_t name_len; // QNAME length (SAM: at off; BAM: at off + 36)
        uint64_t seq_off;  // SAM: SEQ field text; BAM: packed 4-bit sequence
        uint32_t l_seq;    // bases ('*' -> 0)
    };
    std::vector<Rec> recs;
    // A window of records at a time (the bam crate's readers stream records, src/cmd_tag.rs:515,567):
    // open() (by extension: "sam" / "bam", src/cmd_tag.rs:503-615) reads the header and a BAM's reference
    // dictionary, every fill() replaces `recs` by the next records worth ~window_bytes of input; `data`
    // then points at that window.
    void open(const std::string &path);
    bool fill(uint64_t window_bytes);
    // (compressed input; a no-op otherwise) reads, inflates and indexes the window after the current one on the calling
    // thread -- meant for a second thread, beside the work on the current window, whose `data` / `recs` stay valid; the
    // next fill() hands the prepared window out.  An error of that window is thrown here.
    void prefetch(uint64_t window_bytes);
    std::string name(size_t i) const { return std::string(data + recs[i].off + (is_bam ? 36 : 0), recs[i].name_len); }
    // SEQ of records [b0, b1) as the matcher sees it (upper-case ASCII), concatenated (+1 pad byte)
    void gather(size_t b0, size_t b1, std::vector<uint8_t> &seq, std::vector<uint64_t> &off) const;
    // record i as one SAM text line (no line end) appended to out
    void append_line(size_t i, std::string &out) const;
    // BAM input: raw record bytes after the block_size field
    const uint8_t *raw(size_t i) const { return (const uint8_t *)data + recs[i].off + 4; }
    uint32_t raw_len(size_t i) const { return recs[i].len - 4; }
    // value of an existing `tag` field: 0 = absent, 1 = Z value in *val, 2 = present with a
    // non-string type (the reference bails: "Invalid tag value format...")
    int find_tag(size_t i, const std::string &tag, std::string *val) const;
    // BAM input for a caller that keeps the records on the device (run_tag: mk_tag_bam_window takes windows of members as they are
    // stored).  After open(): the file and its member table (source()), the bytes open() inflated behind the header but has not
    // turned into records (the first window's head), and the first member it has not touched.  seek_bam() hands the input back to
    // fill(): the records continue with head[0, n_head) followed by the text of member `member` onwards -- up to member `end_member`
    // where one is given: fill() then returns false in front of the record that crosses into it, which bam_pending() hands out
    // (the next window's head); an end at or behind the last member is the end of the file, where such a record is an error.
    bool bam_on_bgzf() const { return is_bam && src.is_bgzf(); }
    const WindowSource &source() const { return src; }
    const char *bam_pending(uint64_t *n) const {
        *n = buf_len > cursor ? buf_len - cursor : 0;
        return buf.data() + cursor;
    }
    void seek_bam(size_t member, const char *head, uint64_t n_head, size_t end_member = ~(size_t)0);
    // plain SAM text for a caller that keeps the lines on the device (run_tag: mk_tag_sam_window takes slices of the mapping): after
    // open(), text_cursor() = the first byte behind the header lines; seek_text() hands the input back to fill(): the records
    // continue at byte `offset` of the text (a line start) and, where `end` is given (a line start too), end in front of it.
    bool sam_on_mapping() const { return !is_bam && src.mapped() && src.is_file_mapping(); }
    uint64_t text_cursor() const { return cursor; }
    void seek_text(uint64_t offset, uint64_t end = ~0ull) {
        cursor = offset;
        text_end = end;
        recs.clear();
    }

   private:
    WindowSource src;
    std::vector<char> buf;  // compressed input: the window
    uint64_t buf_len = 0;
    uint64_t cursor = 0;    // mapped input: next unread byte; compressed: bytes of the window already turned into records
    uint64_t text_end = ~0ull;  // mapped input: seek_text()'s end
    bool bam_bounded = false;   // seek_bam() was given an end in front of the last member: an unfinished record there is no error
    const char *bytes() const { return src.mapped() ? src.text() : buf.data(); }
    uint64_t n_bytes() const { return src.mapped() ? src.text_size() : buf_len; }
    void drop_front(uint64_t k);
    bool next_window(std::vector<char> &b, uint64_t &bl, uint64_t &cur, std::vector<Rec> &rs, uint64_t window_bytes);
    std::vector<char> nbuf;  // the prefetched window
    uint64_t nbuf_len = 0, ncursor = 0;
    std::vector<Rec> nrecs;
    bool have_next = false, next_more = false;
};

}  // namespace cli
