// bgzf_host.cpp -- host side of the C ABI's BGZF writer and reader (include/merkurio_hip.h, mk_bgzf_*): chunking of a call into
// device-sized passes, the members that end at record ends, the BSIZE walk.  Kernels: bgzf_deflate.hip, bgzf_inflate.hip.  The handle
// and the staging copies: codec_host.cpp.
// Reference interface replaced: the BGZF reader / writer of `bam 0.1.4` as `merkurio tag` drives it
// (src/cmd_tag.rs:254-271 `BamWriter::build().write_header(..).from_path`, :503-506 `BamReader::from_path(.., threads)`)
// and needletail's gzip reader on bgzip'ed inputs (src/cmd_extract.rs:281).
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "../host_common.h"
#include "bgzf_cuts.hpp"
#include "codec_internal.h"
#include "codec_kernels.h"

using mkz::download;
using mkz::elapsed;
using mkz::now_ms;
using mkz::upload;

namespace {

// Members per device pass (mk_codec_set_pass_limits overrides).  Deflate deals its members from a counter to a resident
// grid of 16 waves per CU, so a pass only has to be large: 49 152 members = 3.2 GB of text (its 64 KiB slot per member is
// what bounds it).  Inflate is bound by the latency of its slowest lane, 25-60 ms per launch whatever it holds
// (profiles/r04_codec_kernels.txt): a pass takes as many members as the part holds streams, 3 GiB of text.
constexpr uint64_t kDeflateChunkBlocks = 49152;
constexpr uint64_t kInflateChunkText = 3ull << 30;

const uint8_t kEof[28] = {0x1f, 0x8b, 0x08, 0x04, 0, 0, 0, 0, 0, 0xff, 0x06, 0, 0x42, 0x43, 0x02, 0, 0x1b, 0, 0x03, 0, 0, 0, 0, 0, 0, 0, 0, 0};

}  // namespace

namespace mkz {

int deflate_pass(mk_codec *c, hipStream_t st, const uint8_t *d_text, uint64_t n_text, uint32_t bb, const unsigned long long *off, const uint32_t *len,
                 uint32_t blocks, void *d_packed, size_t packed_cap, void **d_members, uint64_t *total) {
    int rc;
    const uint32_t grid = deflate_grid(blocks, c->num_cus);
    if ((rc = mk::ensure_device(&c->d_crc, &c->crc_cap, blocks * 4ull)) || (rc = mk::ensure_device(&c->d_tokens, &c->tokens_cap, (uint64_t)grid * kTokensPerWave * 4)) ||
        (rc = mk::ensure_device(&c->d_slots, &c->slots_cap, (uint64_t)blocks * kSlotBytes)) || (rc = mk::ensure_device(&c->d_len, &c->len_cap, (blocks + 1) * 4ull)) ||
        (rc = mk::ensure_device(&c->d_off, &c->off_cap, (blocks + 2) * 8ull)))
        return rc;
    // (a stored member: its text + 31 bytes)
    const uint64_t bound = off ? std::min<uint64_t>((uint64_t)blocks * kMaxBlockBytes, n_text) + blocks * 31ull : mk_bgzf_deflate_bound(n_text, bb);
    if (packed_cap < bound) {
        if ((rc = mk::ensure_device(&c->d_out, &c->out_cap, bound))) return rc;
        d_packed = c->d_out;
    }
    uint64_t *d_total = (uint64_t *)c->d_off + blocks;
    if (off) {
        launch_crc_ranges(d_text, off, len, blocks, (uint32_t *)c->d_crc, st);
        launch_deflate_ranges(d_text, off, len, blocks, (const uint32_t *)c->d_crc, (uint32_t *)c->d_tokens, (uint8_t *)c->d_slots, (uint32_t *)c->d_len,
                              (uint32_t *)(d_total + 1), grid, st);
    } else {
        launch_crc(d_text, n_text, bb, blocks, (uint32_t *)c->d_crc, st);
        launch_deflate(d_text, n_text, bb, blocks, (const uint32_t *)c->d_crc, (uint32_t *)c->d_tokens, (uint8_t *)c->d_slots, (uint32_t *)c->d_len,
                       (uint32_t *)(d_total + 1), grid, st);
    }
    launch_pack((const uint8_t *)c->d_slots, (const uint32_t *)c->d_len, (uint64_t *)c->d_off, d_total, blocks, (uint8_t *)d_packed, st);
    *total = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(total, d_total, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return mk::fail(MK_E_HIP, "BGZF deflate on the device failed");
    *d_members = d_packed;
    return MK_OK;
}

// d_text[0, n_text) (kPad readable bytes behind it) whose records end at d_ends[0, n_ends) (device memory, non-decreasing, the last
// one = n_text) -> BGZF members that end at record ends (the cut rule of include/merkurio_hip.h), in passes of members
// (mk_codec_set_pass_limits).  *need = the bytes of all members, *n_members how many.  A pass's members are downloaded to out as long
// as everything so far has fitted out_cap: *need > out_cap means out holds only the passes in front of the one that did not fit (the
// caller reports MK_E_CAPACITY).  c->cut_ms: cut, deflate, download.  d_packed / packed_cap: as deflate_pass.  (Shared with
// mk_extract_window_members, extract_window.cpp: the ends are then the offsets scan of a window's written lengths.)
int deflate_ranges(mk_codec *c, hipStream_t st, const uint8_t *d_text, uint64_t n_text, const unsigned long long *d_ends, uint64_t n_ends, void *d_packed,
                   size_t packed_cap, uint8_t *out, uint64_t out_cap, uint64_t *need, uint64_t *n_members) {
    *need = 0, *n_members = 0;
    c->cut_ms[0] = c->cut_ms[1] = c->cut_ms[2] = 0, c->cut_members = 0;
    if (!n_text) return MK_OK;
    const uint64_t grid64 = (n_text + kCutGrid - 1) / kCutGrid;
    if (grid64 >= 0xFFFFFFFFull) return mk::fail(MK_E_UNSUPPORTED, "%llu output members", (unsigned long long)grid64);
    const uint32_t n_grid = (uint32_t)grid64;
    int rc;
    // the range table: count | off[n_grid] | len[n_grid]
    if ((rc = mk::ensure_device(&c->d_cut, &c->cut_cap, 16 + n_grid * 12ull))) return rc;
    uint32_t *d_count = (uint32_t *)c->d_cut;
    unsigned long long *d_off = (unsigned long long *)((uint8_t *)c->d_cut + 16);
    uint32_t *d_len = (uint32_t *)(d_off + n_grid);
    double t0 = now_ms();
    launch_cuts(d_ends, n_ends, n_text, n_grid, d_off, d_len, d_count, st);
    uint32_t members = 0;
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&members, d_count, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return mk::fail(MK_E_HIP, "the cut kernel failed");
    if (members > n_grid || members + 1 < n_grid) return mk::fail(MK_E_HIP, "the cut kernel reports %u members of %u grid points", members, n_grid);
    c->cut_ms[0] = (float)(now_ms() - t0);
    // passes of members; a pass's members are downloaded as long as everything so far has fitted
    const uint64_t pass = std::min<uint64_t>(c->deflate_pass_blocks ? c->deflate_pass_blocks : kDeflateChunkBlocks, 0x7FFFFFFFu);
    uint64_t written = 0;
    bool fits = true;
    for (uint64_t m0 = 0; m0 < members; m0 += pass) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(pass, members - m0);
        void *d_members = nullptr;
        uint64_t total = 0;
        t0 = now_ms();
        if ((rc = deflate_pass(c, st, d_text, n_text, 0, d_off + m0, d_len + m0, cnt, d_packed, packed_cap, &d_members, &total))) return rc;
        c->cut_ms[1] += (float)(now_ms() - t0);
        fits = fits && written + total <= out_cap;
        if (fits && total) {
            t0 = now_ms();
            if (hipMemcpyAsync(out + written, d_members, total, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
                return mk::fail(MK_E_HIP, "download of the members failed");
            c->cut_ms[2] += (float)(now_ms() - t0);
        }
        written += total;
    }
    *need = written, *n_members = members, c->cut_members = members;
    return MK_OK;
}

}  // namespace mkz

extern "C" {

int mk_bgzf_record_cuts(const uint64_t *rec_end, uint64_t n_rec, uint64_t *cut, uint64_t cap, uint64_t *n_cuts) {
    if (!n_cuts || (n_rec && !rec_end) || (cap && !cut)) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_record_cuts: NULL argument");
    *n_cuts = 0;
    for (uint64_t r = 1; r < n_rec; ++r)
        if (rec_end[r] < rec_end[r - 1]) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_record_cuts: record end %llu lies in front of the one before it", (unsigned long long)r);
    const uint64_t k = mkz::record_cuts(rec_end, n_rec, cut, cap);
    *n_cuts = k;
    if (k > cap) return mk::fail(MK_E_CAPACITY, "mk_bgzf_record_cuts: %llu cuts, room for %llu", (unsigned long long)k, (unsigned long long)cap);
    return MK_OK;
}

int mk_bgzf_deflate_records(mk_codec *c, const uint8_t *text, uint64_t n, const uint64_t *rec_end, uint64_t n_rec, uint8_t *out, uint64_t out_cap,
                            uint64_t *out_len, uint64_t *n_members) {
    MK_ABI_BEGIN
    if (!c || !out_len || !n_members || (n && (!text || !rec_end)) || (out_cap && !out)) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate_records: NULL argument");
    *out_len = 0, *n_members = 0;
    if ((n_rec ? rec_end[n_rec - 1] : 0) != n) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate_records: the last record does not end where the text does");
    for (uint64_t r = 1; r < n_rec; ++r)
        if (rec_end[r] < rec_end[r - 1]) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate_records: record end %llu lies in front of the one before it", (unsigned long long)r);
    std::lock_guard<std::mutex> lock(c->mu);
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    c->ms[0] = c->ms[1] = c->ms[2] = 0;
    if (!n) return MK_OK;
    int rc;
    if ((rc = mk::ensure_device(&c->d_in, &c->in_cap, n + mkz::kPad)) || (rc = mk::ensure_device(&c->d_ends, &c->ends_cap, n_rec * 8ull))) return rc;
    const double t_up = now_ms();
    if ((rc = upload(c, c->d_in, text, n)) || (rc = upload(c, c->d_ends, (const uint8_t *)rec_end, n_rec * 8ull))) return rc;
    MKC_HIP(hipMemsetAsync((uint8_t *)c->d_in + n, 0, mkz::kPad, c->stream), "hipMemsetAsync");
    MKC_HIP(hipStreamSynchronize(c->stream), "upload of the text");
    c->ms[0] = (float)(now_ms() - t_up);
    uint64_t need = 0;
    if ((rc = mkz::deflate_ranges(c, c->stream, (const uint8_t *)c->d_in, n, (const unsigned long long *)c->d_ends, n_rec, nullptr, 0, out, out_cap, &need, n_members)))
        return rc;
    c->ms[1] = c->cut_ms[0] + c->cut_ms[1], c->ms[2] = c->cut_ms[2];
    *out_len = need;
    if (need > out_cap) return mk::fail(MK_E_CAPACITY, "mk_bgzf_deflate_records: the members take %llu bytes, room for %llu", (unsigned long long)need, (unsigned long long)out_cap);
    return MK_OK;
    MK_ABI_END
}

uint64_t mk_bgzf_deflate_bound(uint64_t n, uint32_t block_bytes) {
    const uint64_t bb = block_bytes ? block_bytes : mkz::kMaxBlockBytes;
    const uint64_t blocks = (n + bb - 1) / bb;
    return n + blocks * 31;  // a stored member: 18 + 5 + text + 8
}

const uint8_t *mk_bgzf_eof(void) { return kEof; }

int mk_bgzf_deflate_pieces(mk_codec *c, const uint8_t *const *pieces, const uint64_t *sizes, uint64_t n_pieces, uint32_t block_bytes,
                           uint8_t *out, uint64_t out_cap, uint64_t *out_len) {
    MK_ABI_BEGIN
    if (!c || !out_len || (n_pieces && (!pieces || !sizes))) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate: NULL argument");
    uint64_t n = 0;
    for (uint64_t k = 0; k < n_pieces; ++k) {
        if (sizes[k] && !pieces[k]) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate: piece %llu is NULL", (unsigned long long)k);
        n += sizes[k];
    }
    if (n && !out) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate: NULL argument");
    const uint32_t bb = block_bytes ? block_bytes : mkz::kMaxBlockBytes;
    if (bb > mkz::kMaxBlockBytes) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate: block_bytes %u > %u", bb, mkz::kMaxBlockBytes);
    const uint64_t bound = mk_bgzf_deflate_bound(n, bb);
    *out_len = 0;
    if (out_cap < bound) {
        *out_len = bound;
        return mk::fail(MK_E_CAPACITY, "mk_bgzf_deflate: out_cap %llu < bound %llu", (unsigned long long)out_cap, (unsigned long long)bound);
    }
    std::lock_guard<std::mutex> lock(c->mu);
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    c->ms[0] = c->ms[1] = c->ms[2] = 0;
    const uint64_t chunk_bytes = (c->deflate_pass_blocks ? c->deflate_pass_blocks : kDeflateChunkBlocks) * bb;
    uint64_t written = 0;
    uint64_t piece = 0, piece_at = 0;  // where the text of the next device pass starts
    for (uint64_t at = 0; at < n; at += chunk_bytes) {
        const uint64_t cn = std::min<uint64_t>(chunk_bytes, n - at);
        const uint32_t blocks = (uint32_t)((cn + bb - 1) / bb);
        const uint32_t grid = mkz::deflate_grid(blocks, c->num_cus);
        int rc;
        if ((rc = mk::ensure_device(&c->d_in, &c->in_cap, cn + mkz::kPad)) || (rc = mk::ensure_device(&c->d_crc, &c->crc_cap, blocks * 4ull)) ||
            (rc = mk::ensure_device(&c->d_tokens, &c->tokens_cap, (uint64_t)grid * mkz::kTokensPerWave * 4)) ||
            (rc = mk::ensure_device(&c->d_slots, &c->slots_cap, (uint64_t)blocks * mkz::kSlotBytes)) ||
            (rc = mk::ensure_device(&c->d_len, &c->len_cap, blocks * 4ull)) || (rc = mk::ensure_device(&c->d_off, &c->off_cap, (blocks + 2) * 8ull)) ||
            (rc = mk::ensure_device(&c->d_out, &c->out_cap, mk_bgzf_deflate_bound(cn, bb))))
            return rc;
        uint64_t *d_total = (uint64_t *)c->d_off + blocks;
        const double t_up = now_ms();
        for (uint64_t done = 0; done < cn;) {  // the pieces land back to back: the concatenation exists on the device only
            while (piece_at == sizes[piece]) ++piece, piece_at = 0;
            const uint64_t k = std::min<uint64_t>(cn - done, sizes[piece] - piece_at);
            if ((rc = upload(c, (uint8_t *)c->d_in + done, pieces[piece] + piece_at, k))) return rc;
            done += k, piece_at += k;
        }
        MKC_HIP(hipMemsetAsync((uint8_t *)c->d_in + cn, 0, mkz::kPad, c->stream), "hipMemsetAsync");
        MKC_HIP(hipStreamSynchronize(c->stream), "upload of the text");
        c->ms[0] += (float)(now_ms() - t_up);
        MKC_HIP(hipEventRecord(c->ev[1], c->stream), "hipEventRecord");
        mkz::launch_crc((const uint8_t *)c->d_in, cn, bb, blocks, (uint32_t *)c->d_crc, c->stream);
        mkz::launch_deflate((const uint8_t *)c->d_in, cn, bb, blocks, (const uint32_t *)c->d_crc, (uint32_t *)c->d_tokens, (uint8_t *)c->d_slots,
                            (uint32_t *)c->d_len, (uint32_t *)(d_total + 1), grid, c->stream);
        mkz::launch_pack((const uint8_t *)c->d_slots, (const uint32_t *)c->d_len, (uint64_t *)c->d_off, d_total, blocks, (uint8_t *)c->d_out, c->stream);
        MKC_HIP(hipGetLastError(), "BGZF deflate kernels");
        MKC_HIP(hipEventRecord(c->ev[2], c->stream), "hipEventRecord");
        uint64_t total = 0;
        MKC_HIP(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, c->stream), "download of the size");
        MKC_HIP(hipStreamSynchronize(c->stream), "BGZF deflate");
        if (total > out_cap - written) return mk::fail(MK_E_CAPACITY, "mk_bgzf_deflate: members exceed the bound (internal error)");
        const double t_down = now_ms();
        if ((rc = download(c, out + written, c->d_out, total))) return rc;
        c->ms[1] += elapsed(c->ev[1], c->ev[2]), c->ms[2] += (float)(now_ms() - t_down);
        written += total;
    }
    *out_len = written;
    return MK_OK;
    MK_ABI_END
}

int mk_bgzf_deflate(mk_codec *c, const uint8_t *in, uint64_t n, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_len) {
    if (n && !in) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_deflate: NULL argument");
    return mk_bgzf_deflate_pieces(c, &in, &n, n ? 1 : 0, block_bytes, out, out_cap, out_len);
}

int mk_bgzf_members(const uint8_t *in, uint64_t n, mk_bgzf_member *members, uint64_t cap, uint64_t *n_members, uint64_t *consumed,
                    uint64_t *text_bytes) {
    if (!n_members || (n && !in)) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_members: NULL argument");
    uint64_t at = 0, k = 0, text = 0;
    while (n - at >= 18) {
        const uint8_t *h = in + at;
        if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || !(h[3] & 4)) return mk::fail(MK_E_CORRUPT, "not a BGZF member at byte %llu", (unsigned long long)at);
        const uint32_t xlen = h[10] | (uint32_t)h[11] << 8;
        if (n - at < 12 + (uint64_t)xlen) break;
        uint32_t bsize = 0;
        bool found = false;
        for (uint32_t x = 0; x + 4 <= xlen;) {  // the extra field's subfields: SI1 SI2 SLEN data
            const uint8_t *f = h + 12 + x;
            const uint32_t slen = f[2] | (uint32_t)f[3] << 8;
            if (f[0] == 'B' && f[1] == 'C' && slen == 2 && x + 6 <= xlen) bsize = f[4] | (uint32_t)f[5] << 8, found = true;
            x += 4 + slen;
        }
        if (!found) return mk::fail(MK_E_CORRUPT, "gzip member without a BC subfield at byte %llu", (unsigned long long)at);
        const uint64_t size = (uint64_t)bsize + 1;
        if (size < 12 + (uint64_t)xlen + 8) return mk::fail(MK_E_CORRUPT, "BGZF member with BSIZE %u at byte %llu", bsize, (unsigned long long)at);
        if (n - at < size) break;
        uint32_t crc, isize;
        memcpy(&crc, h + size - 8, 4), memcpy(&isize, h + size - 4, 4);
        if (isize > 65536) return mk::fail(MK_E_CORRUPT, "BGZF member with ISIZE %u at byte %llu", isize, (unsigned long long)at);
        // RFC 1952's optional fields between the extra field and the DEFLATE stream (bgzip sets none of them, a gzip member
        // that carries a BC subfield may): FNAME / FCOMMENT are zero-terminated, FHCRC is two bytes; reserved bits refuse
        uint64_t skip = 12 + (uint64_t)xlen;
        if (h[3] & 0xE0) return mk::fail(MK_E_UNSUPPORTED, "gzip member with reserved FLG bits (0x%02x) at byte %llu", h[3], (unsigned long long)at);
        for (int bit = 3; bit <= 4; ++bit)
            if (h[3] & (1 << bit)) {
                const void *z = skip < size - 8 ? memchr(h + skip, 0, (size_t)(size - 8 - skip)) : nullptr;
                if (!z) return mk::fail(MK_E_CORRUPT, "gzip member with an unterminated %s at byte %llu", bit == 3 ? "FNAME" : "FCOMMENT", (unsigned long long)at);
                skip = (uint64_t)((const uint8_t *)z - h) + 1;
            }
        if (h[3] & 2) skip += 2;
        if (skip + 8 > size) return mk::fail(MK_E_CORRUPT, "BGZF member whose header fields overrun BSIZE at byte %llu", (unsigned long long)at);
        if (members && k < cap) members[k] = mk_bgzf_member{at + skip, text, (uint32_t)(size - skip - 8), isize, crc, 0};
        ++k, text += isize, at += size;
    }
    *n_members = k;
    if (consumed) *consumed = at;
    if (text_bytes) *text_bytes = text;
    return MK_OK;
}

int mk_bgzf_inflate(mk_codec *c, const uint8_t *in, uint64_t n_in, const mk_bgzf_member *members, uint64_t n_members, uint8_t *out,
                    uint64_t out_cap, uint64_t *bad_member) {
    MK_ABI_BEGIN
    if (!c || (n_members && (!in || !members)) || (out_cap && !out)) return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_inflate: NULL argument");
    static_assert(sizeof(mk_bgzf_member) == sizeof(mkz::Member), "member layouts");
    if (bad_member) *bad_member = 0;
    for (uint64_t i = 0; i < n_members; ++i) {
        const mk_bgzf_member &m = members[i];
        if (m.data_off > n_in || m.data_len > n_in - m.data_off || m.isize > 65536 || m.out_off > out_cap || m.isize > out_cap - m.out_off) {
            if (bad_member) *bad_member = i;
            return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_inflate: member %llu lies outside its buffers", (unsigned long long)i);
        }
    }
    std::lock_guard<std::mutex> lock(c->mu);
    MKC_HIP(hipSetDevice(c->device), "hipSetDevice");
    c->ms[0] = c->ms[1] = c->ms[2] = 0;
    std::vector<mkz::Member> part;
    std::vector<int32_t> status;
    for (uint64_t m0 = 0; m0 < n_members;) {
        // a run of members whose compressed bytes and text are both contiguous enough to move in one piece each
        uint64_t m1 = m0, text = 0, in_lo = members[m0].data_off, in_hi = in_lo, out_lo = members[m0].out_off, out_hi = out_lo;
        const uint64_t pass_text = c->inflate_pass_text ? c->inflate_pass_text : kInflateChunkText;
        while (m1 < n_members && (m1 == m0 || text + members[m1].isize <= pass_text)) {
            const mk_bgzf_member &m = members[m1];
            in_lo = std::min(in_lo, m.data_off), in_hi = std::max(in_hi, m.data_off + m.data_len);
            out_lo = std::min(out_lo, m.out_off), out_hi = std::max(out_hi, m.out_off + m.isize);
            text += m.isize, ++m1;
        }
        if (out_hi - out_lo > 2 * kInflateChunkText || in_hi - in_lo > 2 * kInflateChunkText)
            return mk::fail(MK_E_INVALID_ARG, "mk_bgzf_inflate: members %llu.. are scattered over more than a device pass holds",
                            (unsigned long long)m0);
        const uint32_t cnt = (uint32_t)(m1 - m0);
        part.resize(cnt);
        for (uint32_t k = 0; k < cnt; ++k) {
            const mk_bgzf_member &m = members[m0 + k];
            part[k] = mkz::Member{m.data_off - in_lo, m.out_off - out_lo, m.data_len, m.isize, m.crc, 0};
        }
        const uint64_t cn = in_hi - in_lo, tn = out_hi - out_lo;
        int rc;
        if ((rc = mk::ensure_device(&c->d_in, &c->in_cap, cn + mkz::kPad)) || (rc = mk::ensure_device(&c->d_aux, &c->aux_cap, cnt * sizeof(mkz::Member))) ||
            (rc = mk::ensure_device(&c->d_out, &c->out_cap, tn + 16)) || (rc = mk::ensure_device(&c->d_len, &c->len_cap, cnt * 4ull)))
            return rc;
        const double t_up = now_ms();
        if ((rc = upload(c, c->d_in, in + in_lo, cn))) return rc;
        MKC_HIP(hipMemsetAsync((uint8_t *)c->d_in + cn, 0, mkz::kPad, c->stream), "hipMemsetAsync");
        MKC_HIP(hipMemcpyAsync(c->d_aux, part.data(), cnt * sizeof(mkz::Member), hipMemcpyHostToDevice, c->stream), "upload of the member table");
        MKC_HIP(hipStreamSynchronize(c->stream), "upload of the members");
        c->ms[0] += (float)(now_ms() - t_up);
        MKC_HIP(hipEventRecord(c->ev[1], c->stream), "hipEventRecord");
        mkz::launch_inflate((const uint8_t *)c->d_in, cn, (const mkz::Member *)c->d_aux, cnt, (uint8_t *)c->d_out, (int32_t *)c->d_len, c->num_cus, c->stream,
                            c->inflate_kernel);
        mkz::launch_crc_check((const uint8_t *)c->d_out, (const mkz::Member *)c->d_aux, cnt, (int32_t *)c->d_len, c->stream);
        MKC_HIP(hipGetLastError(), "BGZF inflate kernels");
        MKC_HIP(hipEventRecord(c->ev[2], c->stream), "hipEventRecord");
        status.resize(cnt);
        MKC_HIP(hipMemcpyAsync(status.data(), c->d_len, cnt * 4ull, hipMemcpyDeviceToHost, c->stream), "download of the status words");
        MKC_HIP(hipStreamSynchronize(c->stream), "BGZF inflate");
        // (a damaged member's text is not handed out: the status words first)
        bool all_ok = true;
        for (uint32_t k = 0; k < cnt && all_ok; ++k) all_ok = status[k] == 0;
        const double t_down = now_ms();
        if (all_ok && tn && (rc = download(c, out + out_lo, c->d_out, tn))) return rc;
        c->ms[1] += elapsed(c->ev[1], c->ev[2]), c->ms[2] += (float)(now_ms() - t_down);
        for (uint32_t k = 0; k < cnt; ++k)
            if (status[k]) {
                if (bad_member) *bad_member = m0 + k;
                if (status[k] > 0)  // the decoder was content (0), the checksum kernel raised its bit
                    return mk::fail(MK_E_CORRUPT, "BGZF member %llu: CRC-32 of the inflated text differs from the trailer's", (unsigned long long)(m0 + k));
                return mk::fail(MK_E_CORRUPT, "BGZF member %llu does not inflate to its ISIZE (decoder status %d)", (unsigned long long)(m0 + k), status[k]);
            }
        m0 = m1;
    }
    return MK_OK;
    MK_ABI_END
}

}  // extern "C"
