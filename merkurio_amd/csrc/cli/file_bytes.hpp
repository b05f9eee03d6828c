// file_bytes.hpp -- an input file's bytes in memory: the mapping of a regular file, or an inflated copy
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace cli {

struct FileBytes {
    const char *p = nullptr;
    uint64_t n = 0;
    std::vector<char> owned;  // an inflated copy
    void *map = nullptr;      // mmap path
    uint64_t map_len = 0;
    ~FileBytes();
    // maps the file read-only: p[0, n) is the file as stored.  false: not a regular file, an empty one, or one that cannot be mapped
    // (nothing changed); raises cli::Error if it cannot be opened.  No MAP_POPULATE: the inputs are read a window at a time; the
    // reader asks for each window ahead of its parse (FastxStream::prefetch, SamFile::fill), the kernel reads ahead sequentially
    bool map_file(const std::string &path);
    // these bytes take the mapping's place (the inflated text of a compressed file): the mapping, if any, is released
    void adopt(std::vector<char> &&bytes);
    FileBytes() = default;
    FileBytes(const FileBytes &) = delete;
    FileBytes &operator=(const FileBytes &) = delete;
};

// whole file into memory; transparently inflates gzip (magic 1f 8b; BGZF members in parallel) and,
// like needletail's `compression` feature, bzip2 / xz / zstd (decompress.cpp)
std::vector<char> read_file_maybe_gz(const std::string &path);
// bzip2 / xz / zstd by magic bytes through the system's runtime libraries (bound with dlopen):
// false = none of the three; raises cli::Error on corrupt input or a missing library
bool inflate_by_magic(const std::string &path, const unsigned char *data, size_t n, std::vector<char> &out);
// the first bytes of a bzip2 file's text, at most `want` of them, by libbz2 (the first block is decoded, no more): false if the library is
// missing or the file is damaged before that many bytes have come out (the whole-file call then words the error)
bool bz2_first_bytes(const unsigned char *data, size_t n, std::vector<char> &out, size_t want);
// likewise for a zstd file, by libzstd
bool zstd_first_bytes(const unsigned char *data, size_t n, std::vector<char> &out, size_t want);
// and for an xz file, by liblzma
bool xz_first_bytes(const unsigned char *data, size_t n, std::vector<char> &out, size_t want);

}  // namespace cli
