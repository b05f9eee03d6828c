// fastx.hpp -- FASTA / FASTQ input of the `merkurio` CLI.  Observable behaviour follows what the reference gets from needletail 0.6.3
// (src/cmd_extract.rs:281,327-340,403).
#pragma once
#include "util.hpp"
#include "window_source.hpp"

namespace cli {

// the records of a text (a whole file or a window of one) as index entries into it
struct FastxFile {
    const char *data = nullptr;  // the text (FastxStream: the current window)
    uint64_t data_n = 0;         // bytes behind `data`
    bool fastq = false;
    struct Rec {
        uint64_t id_b, id_e;    // header line without the marker ('>' / '@') and line end
        uint64_t raw_b, raw_e;  // sequence as stored, inner line breaks included (FASTA) -- what write() emits
        uint64_t qual_b, qual_e;
    };
    std::vector<Rec> recs;
    std::string id(size_t i) const { return std::string(data + recs[i].id_b, recs[i].id_e - recs[i].id_b); }
    // record.seq(): newline-free sequence appended to `out`; returns num_bases()
    uint64_t append_seq(size_t i, std::vector<uint8_t> &out) const;
    // sequences of records [b0, b1) concatenated into seq (+1 pad byte) with offsets off[0..b1-b0];
    // FASTQ records are copied by several host threads
    void gather(size_t b0, size_t b1, std::vector<uint8_t> &seq, std::vector<uint64_t> &off) const;
    // number of sequence bytes of record i as stored (upper bound of num_bases)
    uint64_t raw_len(size_t i) const { return recs[i].raw_e - recs[i].raw_b; }
    // record.write(writer, None): FASTA keeps the original wrapping, FASTQ is 4 lines
    void write(size_t i, Sink &w) const;
    // appends the records of data[b, e) (b at a record start) to recs
    void parse_span(uint64_t b, uint64_t e);
    // the same for text that may end inside a record (partial_ok: more text follows data[0, data_n)): parsing stops in front of a
    // record that cannot be shown to end in it; returns where it stopped
    uint64_t parse_span_partial(uint64_t b, uint64_t e, bool partial_ok);
};

// A FASTA/FASTQ input read window by window (needletail's parse_fastx_file streams records:
// src/cmd_extract.rs:281,321), with the next window parsed (and inflated) while the current one is in use:
//     bool more = s.fill(W);
//     while (more) { n = s.view.recs.size(); s.consume(n); s.prefetch(W) on another thread;
//                    ...records [0, n) of s.view...; join; more = s.fill(W); }
struct FastxStream {
    FastxFile view;  // the current window: view.data / view.recs / view.fastq; all FastxFile accessors work on it
    void open(const std::string &path, bool defer_bzip2 = false, bool defer_zstd = false, bool defer_xz = false) { src.open(path, defer_bzip2, defer_zstd, defer_xz); }
    // Makes the next window current: every complete record among the unconsumed bytes plus up to
    // `window_bytes` new ones (parsed here unless prefetch() already did).  false: no record is left.
    bool fill(uint64_t window_bytes);
    // The first n records of the current window are all this window hands out; the next window starts
    // with record n.  The records stay valid until the next fill().
    void consume(size_t n);
    // Parses the window behind the consumed records into a spare index (and, for compressed input, a second
    // buffer); may run on another thread while `view` is being used.  Call after consume().
    void prefetch(uint64_t window_bytes);
    // RAW windows (extract_windows.cpp: a window's text goes to the GPU as it is and is indexed there, mk_extract_window): the
    // next ~window_bytes of text, from a record start to a record start, NOT parsed; FASTQ ('@' records) or FASTA ('>' records),
    // whichever the first record is.  false: no text is left, or it does not start like a record (nothing consumed).  The text
    // stays valid until the raw_fill() after next; raw_consume() accepts the window, without it the next fill() / raw_fill()
    // starts at the same place.  Use before any fill().
    bool raw_fill(uint64_t window_bytes, const char **text, uint64_t *n, uint64_t *resume);
    void raw_consume();
    // everything that is left of the input, as it is (after raw_fill() returned false: text that does not start like a record);
    // consumed.  false: nothing is left
    bool raw_rest(const char **text, uint64_t *n);
    // gzip input whose first text_bytes bytes something else has read (the device's gzip stream, up to where it handed the file back):
    // the reader inflates them too, from the front and at its own pace, and drops them; the next raw_fill() starts behind them, which
    // has to be a record start.  A raw_fill() that was not consumed is forgotten.  false: the text is shorter than that
    bool raw_skip(uint64_t text_bytes);
    // the raw windows are slices of a plain (memory-mapped) file: window = file[resume - n, resume)
    bool raw_is_plain() const { return src.mapped() && src.is_file_mapping(); }
    // after the first raw_fill(): the input is FASTQ ('@' records) or FASTA ('>' records)
    bool raw_fastq() const { return fastq; }
    // bgzip'ed input: the caller walks source()'s members itself and sends them to the device as they are
    bool raw_is_bgzf() const { return src.is_bgzf(); }
    bool raw_is_gzip() const { return src.is_gzip(); }
    // a bzip2 input opened with defer_bzip2 that nothing has read yet: source().file_bytes() is the file as stored
    bool raw_is_bzip2() const { return src.is_bzip2(); }
    // likewise a zstd input opened with defer_zstd; raw_is_deferred: any of the three
    bool raw_is_zstd() const { return src.is_zstd(); }
    // and an xz input opened with defer_xz
    bool raw_is_xz() const { return src.is_xz(); }
    bool raw_is_deferred() const { return src.is_bzip2() || src.is_zstd() || src.is_xz(); }
    void raw_settle() { src.settle(); }  // libbz2 / libzstd / liblzma inflates it now
    const WindowSource &source() const { return src; }

   private:
    WindowSource src;
    uint64_t cursor = 0;  // mapped text: first byte of the next window; compressed: offset of the unconsumed tail in bufs[cur]
    bool started = false, fastq = false;
    std::vector<char> bufs[2];  // compressed input: the current window lives in bufs[cur]
    uint64_t lens[2] = {0, 0};
    int cur = 0;
    bool have_spare = false;
    std::vector<FastxFile::Rec> spare_recs;
    const char *spare_data = nullptr;
    uint64_t spare_n = 0, spare_end = 0, cur_end = 0;  // *_end: where the records of a window end
    uint64_t raw_next = 0;  // raw windows: where the window handed out last ends
    void parse_window(const char *d, uint64_t n, uint64_t from, uint64_t stop, bool partial_ok);
    // c, the first byte of the text that is no line end, says once whether the input is FASTQ ('@') or FASTA ('>'); true: c starts a
    // record of the input's kind
    bool starts_record(char c) {
        if (!started && (c == '@' || c == '>')) fastq = c == '@', started = true;
        return started && c == (fastq ? '@' : '>');
    }
};

}  // namespace cli
