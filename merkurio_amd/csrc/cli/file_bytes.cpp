#include "file_bytes.hpp"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>

#include "bgzf_in.hpp"
#include "host_mem.hpp"

namespace cli {

FileBytes::~FileBytes() {
    if (map) munmap(map, map_len);
}

bool FileBytes::map_file(const std::string &path) {
    const int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) bail("No such file or directory: " + path);
    struct stat st;
    void *m = fstat(fd, &st) == 0 && S_ISREG(st.st_mode) && st.st_size > 0 ? mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0) : MAP_FAILED;
    close(fd);
    if (m == MAP_FAILED) return false;
    map = m, map_len = (uint64_t)st.st_size;
    p = (const char *)m, n = map_len;
    return true;
}

void FileBytes::adopt(std::vector<char> &&bytes) {
    if (map) munmap(map, map_len);
    map = nullptr, map_len = 0;
    owned = std::move(bytes);
    p = owned.data(), n = owned.size();
}

std::vector<char> read_file_maybe_gz(const std::string &path) {
    std::vector<char> out;
    {
        FileBytes fb;
        if (fb.map_file(path)) {
            if (inflate_by_magic(path, (const unsigned char *)fb.p, (size_t)fb.n, out)) return out;  // bzip2 / xz / zstd
            // BGZF (BAM, bgzip'ed FASTQ): independent <= 64 KiB members, inflated on every host thread
            std::vector<mk_bgzf_member> mem;
            if (fb.n >= 28 && bgzf_walk((const uint8_t *)fb.p, (size_t)fb.n, mem)) {
                const uint64_t total = mem.back().out_off + mem.back().isize;
                require_host_memory(total + total / 8, path);  // + record index
                out.resize(total);
                bgzf_inflate_range((const uint8_t *)fb.p, mem.data(), mem.size(), out.data(), path);
                return out;
            }
        }
    }
    // gzopen reads plain files transparently and walks concatenated gzip members
    gzFile g = gzopen(path.c_str(), "rb");
    if (!g) bail("Cannot open " + path);
    gzbuffer(g, 1 << 20);
    size_t cap = 1 << 22;
    out.resize(cap);
    size_t n = 0;
    for (;;) {
        if (n == cap) {
            require_host_memory(cap * 2, path);  // the buffer doubles: both copies exist for a moment
            cap *= 2;
            out.resize(cap);
        }
        int r = gzread(g, out.data() + n, (unsigned)std::min<size_t>(cap - n, 1u << 30));
        if (r < 0) {
            gzclose(g);
            bail("Error while decompressing " + path);
        }
        if (r == 0) break;
        n += (size_t)r;
    }
    gzclose(g);
    out.resize(n);
    return out;
}

}  // namespace cli
