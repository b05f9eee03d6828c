// bam_out.hpp -- BAM output of the `merkurio` CLI: SAM text lines encoded as BAM records, the stream cut into BGZF members
#pragma once
#include <condition_variable>
#include <deque>
#include <exception>
#include <mutex>
#include <thread>

#include "host_mem.hpp"

namespace cli {

// one BGZF member of in[0, n) (n <= 65 280) by zlib at level 6: gzip header with the BC extra field, raw deflate, CRC-32, ISIZE
void bgzf_compress(const uint8_t *in, size_t n, std::vector<uint8_t> &out);
// BAM writer (BGZF): encodes SAM text lines against the header's @SQ dictionary.  Used for
// `tag -o out.bam` (src/cmd_tag.rs:254-271); output is checked by reading it back.
// The uncompressed stream is kept as the pieces it arrives in (the per-thread record buffers of a batch are moved in,
// not copied) and cut into 65 280-byte BGZF members when enough has gathered: on the device (use_device:
// mk_bgzf_deflate_pieces uploads the pieces back to back, the codec of merkurio_amd/csrc/codec/ does the rest) or, with
// --host-codec, by zlib on every host thread.  A flush runs on a thread of its own while the caller encodes the next
// batch; members reach the file in order.
struct BamWriter {
    FILE *f = nullptr;
    std::vector<std::vector<uint8_t>> pieces;  // bytes not handed to a flush yet, in stream order
    size_t pieces_bytes = 0;
    std::vector<std::string> ref_names;
    ~BamWriter();
    // reference dictionary from the @SQ lines of header_text, or (BAM -> BAM pass-through, where
    // records keep their reference ids) the input's own binary dictionary
    void open(const std::string &path, const std::string &header_text, const std::vector<std::string> *names = nullptr,
              const std::vector<uint32_t> *lens = nullptr);
    // members are deflated on this HIP device from now on (the handle is created by the first flush)
    void use_device(int device);
    // pass-through of a raw BAM record with one more Z tag appended (thread-safe, see encode_record)
    static void append_tagged_raw(const uint8_t *rec, uint32_t len, const std::string &tag, const char *val, size_t val_len,
                                  std::vector<uint8_t> &dst);
    void write_record(const std::string &sam_line);
    // block_size + record bytes of one SAM text line appended to dst (thread-safe: encoding is the
    // slow part of SAM -> BAM and runs on every host thread), then put_encoded() in record order
    void encode_record(const std::string &sam_line, std::vector<uint8_t> &dst) const;
    void put_encoded(std::vector<uint8_t> &&bytes);
    // complete BGZF members made elsewhere (mk_tag_bam_window: the tagged records deflated on the device), in buffer[0, used): what
    // has been put so far is closed with a member of its own, then these bytes follow it in the file as they are.  The buffer is the
    // writer's from the call on, whether it returns or throws: the caller's is empty afterwards.
    // (the buffer: page-locked memory the device writes into directly -- a fresh pageable buffer costs a page fault per 4 KiB inside
    // the copy, more than the copy itself --, handed back and forth between the caller and the writer thread)
    void put_members(HostBuffer &&buffer, size_t used);
    // a buffer of at least min_size bytes for such members: one the writer thread has written out, or a new one
    HostBuffer take_raw_buffer(size_t min_size);
    // an empty buffer for the next slice of encoded records: one the writer thread is done with (its pages are mapped
    // already: a fresh 16 MB vector costs 4 000 page faults), or a new one
    std::vector<uint8_t> take_buffer();
    void close();
    double deflate_seconds = 0;  // inside the flush threads (timing mode)
    size_t run_members = 1536;   // members per run handed to the writer thread (100 MB of text: two rounds of the deflate kernel's waves)

   private:
    struct Run : std::vector<std::vector<uint8_t>> {  // a run of whole members, as the pieces it arrived in
        bool raw = false;                               // the run IS members already (put_members) ...
        HostBuffer raw_buf;                             // ... in the first raw_used bytes of this buffer
        size_t raw_used = 0;
    };
    void put(const void *p, size_t n);
    void flush(bool all);
    void enqueue(Run &&run);  // to the writer thread (started here), behind at most kMaxQueuedRuns others; raises the writer thread's error
    void writer_loop();
    void compress_and_write(Run &run);
    int device_ = -1;  // < 0: zlib on the host threads
    void *codec_ = nullptr;
    std::vector<uint8_t> z_, flat_;  // the run being written: its members; its text in one piece (host codec only)
    // runs wait in a queue for the writer thread (a batch hands over several at once: with one flush in flight the
    // caller stood behind its own previous run); at most kMaxQueuedRuns of them, then the caller waits
    std::deque<Run> queue_;
    std::mutex mu_;
    std::condition_variable cv_;
    std::thread writer_;
    bool closing_ = false, busy_ = false;
    std::exception_ptr failed_;
    std::vector<std::vector<uint8_t>> free_;  // buffers of written runs (guarded by mu_)
    std::vector<HostBuffer> free_raw_;  // buffers of written raw runs (guarded by mu_)
};

}  // namespace cli
