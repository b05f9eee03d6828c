#include "window_source.hpp"

#include <sys/mman.h>
#include <zlib.h>

#include "host_mem.hpp"

namespace cli {

WindowSource::~WindowSource() {
    if (zs) {
        inflateEnd((z_stream *)zs);
        delete (z_stream *)zs;
    }
}

void WindowSource::settle() {
    if (kind != BZIP2 && kind != ZSTD && kind != XZ) return;
    std::vector<char> out;
    (void)inflate_by_magic(path, (const unsigned char *)src.p, (size_t)src.n, out);  // (raises on a damaged file)
    src.adopt(std::move(out));
    kind = PLAIN;
}

void WindowSource::open(const std::string &p, bool defer_bzip2, bool defer_zstd, bool defer_xz) {
    path = p;
    kind = PLAIN;
    if (!src.map_file(p)) {  // not a regular file with bytes in it: gzopen reads it whole (plain or gzip)
        src.adopt(read_file_maybe_gz(p));
        return;
    }
    const uint8_t *d = (const uint8_t *)src.p;
    if (defer_bzip2 && src.n >= 4 && !memcmp(d, "BZh", 3)) {
        kind = BZIP2;
    } else if (defer_zstd && src.n >= 4 && d[0] == 0x28 && d[1] == 0xB5 && d[2] == 0x2F && d[3] == 0xFD) {
        kind = ZSTD;
    } else if (defer_xz && src.n >= 6 && !memcmp(d, "\xfd" "7zXZ\0", 6)) {
        kind = XZ;
    } else if (src.n >= 2 && d[0] == 0x1f && d[1] == 0x8b) {
        if (bgzf_walk(d, (size_t)src.n, members)) {
            kind = BGZF;
            return;
        }
        members.clear();
        kind = GZIP;
        z_stream *z = new z_stream;
        memset(z, 0, sizeof(*z));
        if (inflateInit2(z, 15 + 32) != Z_OK) {  // gzip or zlib header, detected
            delete z;
            bail("Error while decompressing " + p);
        }
        zs = z;
    } else {
        (void)madvise(src.map, (size_t)src.map_len, MADV_SEQUENTIAL);
        // bzip2 / xz / zstd (needletail's `compression` feature, Cargo.toml:26): inflated whole, by magic
        std::vector<char> out;
        if (inflate_by_magic(p, d, (size_t)src.n, out)) src.adopt(std::move(out));
    }
}

bool WindowSource::more_into(std::vector<char> &buf, uint64_t &buf_len, uint64_t want) {
    if (kind == PLAIN || src_eof) return false;
    if (want < (1u << 16)) want = 1u << 16;
    require_host_memory(buf_len + want + (buf_len + want) / 8, path);
    if (kind == BGZF) {
        const size_t m0 = (size_t)src_pos, m1 = bgzf_run_end(members, m0, member_end, want);
        const uint64_t add = m1 > m0 ? members[m1 - 1].out_off + members[m1 - 1].isize - members[m0].out_off : 0;
        if (buf.size() < buf_len + add) buf.resize(buf_len + add);
        bgzf_inflate_range((const uint8_t *)src.p, members.data() + m0, m1 - m0, buf.data() + buf_len, path);
        buf_len += add;
        src_pos = m1;
        if (src_pos >= std::min(members.size(), member_end)) src_eof = true;
        return true;
    }
    // GZIP: zlib streaming over the mapped file, concatenated members included
    z_stream *z = (z_stream *)zs;
    if (buf.size() < buf_len + want) buf.resize(buf_len + want);
    uint64_t room = buf.size() - buf_len;
    while (room > 0 && !src_eof) {
        z->next_in = (Bytef *)const_cast<char *>(src.p + src_pos);
        const uInt in_piece = (uInt)std::min<uint64_t>(src.n - src_pos, 1u << 30);
        z->avail_in = in_piece;
        z->next_out = (Bytef *)buf.data() + buf_len;
        const uInt out_piece = (uInt)std::min<uint64_t>(room, 1u << 30);
        z->avail_out = out_piece;
        const int r = inflate(z, Z_NO_FLUSH);
        src_pos += in_piece - z->avail_in;
        buf_len += out_piece - z->avail_out;
        room -= out_piece - z->avail_out;
        if (r == Z_STREAM_END) {
            if (src_pos >= src.n) {
                src_eof = true;
            } else if (inflateReset(z) != Z_OK) {  // next member
                bail("Error while decompressing " + path);
            }
        } else if (r != Z_OK && r != Z_BUF_ERROR) {
            bail("Error while decompressing " + path);
        } else if (src_pos >= src.n && z->avail_out != 0) {
            bail("Error while decompressing " + path);  // the input ends inside a member
        }
    }
    return true;
}

}  // namespace cli
