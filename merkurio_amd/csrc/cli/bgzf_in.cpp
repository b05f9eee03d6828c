#include "bgzf_in.hpp"

#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <mutex>

#include "device_abi_weak.hpp"
#include "host_mem.hpp"

namespace cli {

bool bgzf_walk(const uint8_t *d, size_t n, std::vector<mk_bgzf_member> &mem) {
    size_t p = 0;
    uint64_t total = 0;
    while (p < n) {
        if (n - p < 18 || d[p] != 0x1f || d[p + 1] != 0x8b || d[p + 2] != 8 || !(d[p + 3] & 4)) return false;
        const size_t xlen = d[p + 10] | (size_t)d[p + 11] << 8;
        if (n - p < 12 + xlen + 8) return false;
        size_t bsize = 0;
        for (size_t x = p + 12; x + 4 <= p + 12 + xlen;) {  // extra subfields
            const size_t slen = d[x + 2] | (size_t)d[x + 3] << 8;
            if (d[x] == 'B' && d[x + 1] == 'C' && slen == 2 && x + 6 <= p + 12 + xlen) bsize = (d[x + 4] | (size_t)d[x + 5] << 8) + 1;
            x += 4 + slen;
        }
        if (bsize < 12 + xlen + 8 || (d[p + 3] & ~4) || n - p < bsize) return false;
        mk_bgzf_member b{p + 12 + xlen, total, (uint32_t)(bsize - (12 + xlen) - 8), 0, 0, 0};
        memcpy(&b.crc, d + p + bsize - 8, 4);
        memcpy(&b.isize, d + p + bsize - 4, 4);
        total += b.isize;
        mem.push_back(b);
        p += bsize;
    }
    return !mem.empty();
}

size_t bgzf_run_end(const std::vector<mk_bgzf_member> &m, size_t m0, size_t m_end, uint64_t want_text) {
    const size_t end = std::min(m.size(), m_end);
    size_t m1 = m0;
    uint64_t text = 0;
    while (m1 < end && (text < want_text || m1 == m0)) text += m[m1++].isize;
    return m1;
}

std::vector<mk_bgzf_member> bgzf_rebased(const mk_bgzf_member *m, size_t n, uint64_t file_lo, uint64_t text_base) {
    std::vector<mk_bgzf_member> run(m, m + n);
    for (mk_bgzf_member &b : run) b.data_off -= file_lo, b.out_off -= text_base;
    return run;
}

// The device codec for BGZF input (set_bgzf_device; merkurio_amd/csrc/codec/): one handle per process, created by the
// first window that is large enough to be worth a launch.  < 0: zlib on the host threads (--host-codec).
static int g_bgzf_device = -1;
static std::mutex g_bgzf_mu;
static mk_codec *g_bgzf_codec = nullptr;
static double g_bgzf_device_seconds = 0;
static size_t g_bgzf_device_min_members = 0;  // set below
double bgzf_device_seconds() { return g_bgzf_device_seconds; }
// A launch of the inflate kernel takes 35-60 ms whether it holds 64 members or 49 152 (one lane per member, bound by
// the latency of a lane's serial decode: profiles/r04_codec_kernels.txt); zlib on 16 host threads inflates ~4 GB/s.
// Below ~0.5 GB of text per call the host threads are done first (extract's 128 MB raw windows: 0.63-0.70 s on the
// host, 0.89-0.91 s through the device: profiles/r04_e2e_extract_bgzf.txt).
constexpr size_t kDeviceInflateMinMembers = 8192;
void set_bgzf_device(int device, bool always) {
    g_bgzf_device = mk_bgzf_inflate ? device : -1;
    g_bgzf_device_min_members = always ? 1 : kDeviceInflateMinMembers;
}

void bgzf_inflate_range(const uint8_t *d, const mk_bgzf_member *mem, size_t cnt, char *out, const std::string &path, bool may_use_device) {
    if (cnt == 0) return;
    const uint64_t base = mem[0].out_off;
    // (a device-side failure that is not about the data -- no memory for a third set of codec buffers next to the matcher's
    // and the BAM writer's, a lost device -- is no reason to give up on an input zlib can read: said once, then the host path)
    auto device_gave_up = [&](const char *what) {
        fprintf(stderr, "Warning: BGZF input is inflated on the host threads from here on (%s: %s)\n", what, mk_last_error());
        g_bgzf_device = -1;
    };
    if (may_use_device) {  // (the global is read and written under the mutex only)
        std::unique_lock<std::mutex> lock(g_bgzf_mu);
        if (g_bgzf_device >= 0 && cnt >= g_bgzf_device_min_members && !g_bgzf_codec && mk_codec_create(g_bgzf_device, &g_bgzf_codec) != MK_OK)
            device_gave_up("mk_codec_create");
        if (g_bgzf_device >= 0 && cnt >= g_bgzf_device_min_members) {
            const auto t0 = std::chrono::steady_clock::now();
            const uint64_t in_lo = mem[0].data_off;
            const std::vector<mk_bgzf_member> tab = bgzf_rebased(mem, cnt, in_lo, base);
            uint64_t text = 0, in_hi = 0;
            for (const mk_bgzf_member &b : tab) {
                text = std::max<uint64_t>(text, b.out_off + b.isize);
                in_hi = std::max<uint64_t>(in_hi, b.data_off + b.data_len);
            }
            uint64_t bad = 0;
            const int rc = mk_bgzf_inflate(g_bgzf_codec, d + in_lo, in_hi, tab.data(), cnt, (uint8_t *)out, text, &bad);
            if (rc == MK_E_CORRUPT) bail("Error while decompressing " + path);
            if (rc == MK_OK) {
                g_bgzf_device_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                return;
            }
            device_gave_up("mk_bgzf_inflate");
        }
    }
    const size_t T = std::max<size_t>(1, std::min<size_t>(io_threads(), cnt / 16 + 1));
    run_threads(T, [&](size_t t) {
        z_stream z;
        memset(&z, 0, sizeof(z));
        if (inflateInit2(&z, -15) != Z_OK) bail("Error while decompressing " + path);
        for (size_t i = cnt * t / T; i < cnt * (t + 1) / T; ++i) {
            const mk_bgzf_member &b = mem[i];
            inflateReset(&z);
            z.next_in = const_cast<Bytef *>(d + b.data_off);
            z.avail_in = (uInt)b.data_len;
            Bytef none = 0;  // (an empty member -- the end-of-file marker -- into an empty buffer: zlib refuses a NULL next_out)
            z.next_out = b.isize ? (Bytef *)out + (b.out_off - base) : &none;
            z.avail_out = b.isize;
            const int r = inflate(&z, Z_FINISH);
            if ((r != Z_STREAM_END && !(b.isize == 0 && r == Z_BUF_ERROR)) || z.avail_out != 0 ||
                (uint32_t)crc32(crc32(0, nullptr, 0), b.isize ? (const Bytef *)out + (b.out_off - base) : &none, b.isize) != b.crc) {
                inflateEnd(&z);
                bail("Error while decompressing " + path);
            }
        }
        inflateEnd(&z);
    });
}

void inflate_bgzf_members_host(const uint8_t *file, const mk_bgzf_member *members, size_t n, char *out, const std::string &path) {
    if (n) bgzf_inflate_range(file, members, n, out + members[0].out_off, path, false);  // (the host's own checker path: never the device codec)
}

}  // namespace cli
