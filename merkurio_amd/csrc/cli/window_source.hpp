// window_source.hpp -- the (decompressed) bytes of an input file, a window at a time
#pragma once
#include <algorithm>
#include <cstring>

#include "bgzf_in.hpp"
#include "file_bytes.hpp"

namespace cli {

// An input file as a sequence of (decompressed) bytes that is looked at through a sliding window, so that
// the host holds one window at a time, like the reference, which streams records.  Plain files are
// memory-mapped: the "window" is the whole mapping and costs nothing.  gzip is inflated incrementally
// (zlib streaming, concatenated members included), BGZF a group of members at a time on all host
// threads; bzip2 / xz / zstd inputs are inflated whole (their libraries are bound through dlopen without
// any block index) and then behave like plain text -- a bzip2 file opened with defer_bzip2 only when settle() is called.
struct WindowSource {
    // defer_bzip2: a bzip2 file is mapped as stored and NOT inflated (is_bzip2()): the caller may decode file_bytes() elsewhere
    // (extract's mk_bzip2_inflate_device path); settle() -- which every read of the text through FastxStream begins with -- inflates it
    // with libbz2 after all, and from then on it is plain text like any other inflated bzip2 input
    // defer_zstd: likewise for a zstd file (is_zstd(); extract's mk_zstd_inflate_device path under --device-zstd); settle(): libzstd
    // defer_xz: likewise for an xz file (is_xz(); extract's mk_xz_inflate_device path under --device-xz); settle(): liblzma
    void open(const std::string &path, bool defer_bzip2 = false, bool defer_zstd = false, bool defer_xz = false);
    bool is_bzip2() const { return kind == BZIP2; }
    bool is_zstd() const { return kind == ZSTD; }
    bool is_xz() const { return kind == XZ; }
    void settle();
    bool mapped() const { return kind == PLAIN; }  // text()/text_size() is the complete text
    bool is_file_mapping() const { return kind == PLAIN && src.map != nullptr; }  // (not an inflated bzip2 / xz / zstd copy)
    const char *text() const { return src.p; }
    uint64_t text_size() const { return src.n; }
    // compressed kinds: appends up to ~want more inflated bytes to dst[0,len) (some progress unless the
    // source is exhausted); false if it already was
    bool more_into(std::vector<char> &dst, uint64_t &len, uint64_t want);
    bool exhausted() const { return kind == PLAIN || src_eof; }
    const std::string &name() const { return path; }
    // BGZF: the file as stored and its member table (data_off absolute in the file, out_off the running text offset), for a caller
    // that inflates on the device (extract's mk_extract_fastq_bgzf path); seek_member() makes member i the next one more_into() inflates
    bool is_bgzf() const { return kind == BGZF; }
    bool is_gzip() const { return kind == GZIP; }  // one or more plain gzip members: file_bytes() is the file as stored (so it is for is_bzip2())
    const uint8_t *file_bytes() const { return (const uint8_t *)src.p; }
    uint64_t file_size() const { return src.n; }
    const std::vector<mk_bgzf_member> &bgzf_members() const { return members; }
    size_t n_bgzf_members() const { return members.size(); }
    // (end: more_into() stops in front of member `end`, as if the file ended there)
    void seek_member(size_t i, size_t end = ~(size_t)0) {
        src_pos = i;
        member_end = end;
        src_eof = i >= std::min(members.size(), member_end);
    }
    size_t next_member() const { return (size_t)src_pos; }  // BGZF: the first member more_into() has not inflated yet
    ~WindowSource();
    WindowSource() = default;
    WindowSource(const WindowSource &) = delete;
    WindowSource &operator=(const WindowSource &) = delete;

   private:
    enum Kind { PLAIN, GZIP, BGZF, BZIP2, ZSTD, XZ } kind = PLAIN;
    std::string path;
    FileBytes src;  // the file as stored (PLAIN: the text itself, or inflated bzip2 / xz / zstd)
    bool src_eof = false;
    void *zs = nullptr;    // GZIP: z_stream
    uint64_t src_pos = 0;  // GZIP: next compressed byte; BGZF: next member
    std::vector<mk_bgzf_member> members;
    size_t member_end = ~(size_t)0;  // BGZF: seek_member()'s end
};

// Readers of compressed input keep two buffers: the unconsumed tail from[cursor, from_len) of the current one opens the other, to[0, to_len)
inline void carry_tail(const std::vector<char> &from, uint64_t from_len, uint64_t cursor, std::vector<char> &to, uint64_t &to_len) {
    const uint64_t tail = from_len > cursor ? from_len - cursor : 0;
    if (to.size() < tail) to.resize(tail);
    if (tail) memcpy(to.data(), from.data() + cursor, tail);
    to_len = tail;
}

// text lines: the index of the '\n' that ends the line at b, or n; the line's end without a '\r'
inline uint64_t line_end(const char *d, uint64_t n, uint64_t b) {
    const void *p = memchr(d + b, '\n', n - b);
    return p ? (uint64_t)((const char *)p - d) : n;
}
inline uint64_t strip_cr(const char *d, uint64_t b, uint64_t e) { return (e > b && d[e - 1] == '\r') ? e - 1 : e; }

}  // namespace cli
