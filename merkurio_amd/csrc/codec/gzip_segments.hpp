// gzip_segments.hpp -- ONE DEFLATE stream decoded in parallel pieces (r05): the serial parts, shared by the kernels of
// gzip_inflate.hip and by the host harness (tests/helpers/gzip_harness.cpp) that checks them against zlib.
//
// What this replaces: needletail's gzip reader under `merkurio extract` (src/cmd_extract.rs:281-282) on the input it meets most --
// a FASTQ / FASTA compressed by plain gzip: ONE member, one DEFLATE stream of thousands of blocks, which zlib can only walk from the
// front (0.5 GB/s of text on one host thread, 2.6 s per 1.27 GB end to end in r04).  A BGZF file is cut into independent members; a gzip
// stream is not -- but its blocks can be FOUND, and decoded without knowing what came before (the scheme of pugz / rapidgzip,
// restated for a GPU):
//   1. block starts.  A dynamic block opens with a header that almost no bit position satisfies: HLIT / HDIST in range, a COMPLETE
//      code-length code, code lengths that decode to a complete literal / length code with an end-of-block codeword and a usable
//      distance code.  seg_header_plausible() tests one bit position with registers only (the header reader is the lane decoders' one,
//      dynamic_header() of inflate_serial.hpp, in its strict form without table memory).  Over 5.7 G bit positions of gzip -1 / -6
//      / -9 FASTQ streams and of random bytes it passed at the 22 000 block starts and at 3 other places; those give codes whose
//      first codewords are no symbols, or a block that ends after a handful of symbols in front of something that is no header -- so a
//      position that passes is looked at by decoding the first 2 048 symbols of its block dry (gzip_segments_wave.hpp; the first
//      version decoded the whole block, seg_confirm_block_start: a second decode of a quarter to all of the stream).  What PROVES
//      a start is step 2 -- the piece in front of it ends exactly there -- and a start that a piece runs over is dropped and the
//      pieces are decoded again.  The kernel tries 64 positions per wave and step, one wave per nominal chunk of the stream.
//   2. segments.  The stream is cut at the confirmed starts; inflate_segment() decodes [start, next start) into 16-bit symbols: a
//      value below 256 is a byte; a match that reaches back beyond the segment's start copies from a 32 768-element prefix that the
//      caller has filled with place-holders 0x8000 | k ("byte k of the 32 KiB in front of this segment") -- so every match is a plain
//      copy inside the segment's buffer, and place-holders travel through later matches like bytes do.
//   3. resolution.  Segment by segment, the last 32 KiB of resolved text become the next segment's context (sequential, 32 KiB per
//      step); then every symbol of every segment is translated in parallel and the text is checked against the member's CRC-32 / ISIZE.
//      A place-holder that stands for a byte in FRONT of the stream's first one (seg_before_stream) is a match that reaches too far
//      back, in its own piece or carried on by later matches: zlib refuses such a stream, and so does the translation.
// Anything that does not add up -- no block start found where one is needed, a segment that does not end exactly on the next start,
// a buffer that is too small for an unusually compressible stream, a wrong CRC -- makes the whole call report "not taken": the
// caller inflates that file with zlib, as before.  RFC 1951 / RFC 1952.
// A file of SEVERAL members is the same scheme over all of them at once (mk_gzip_members_inflate_device, codec_host.cpp): every
// member's first bit is a start that is known, a piece never reads behind its member's payload, the contexts restart at every member.
#pragma once
#include "inflate_serial.hpp"

namespace mkz {

constexpr uint32_t kSegPrefix = 32768;     // place-holder elements in front of a segment's output
constexpr uint16_t kSegUnknown = 0x8000u;  // | index into the 32 KiB in front of the segment
constexpr uint32_t kSegSlack = 16;         // elements a segment buffer holds behind its capacity (8-byte copy rounds overshoot)

// error codes (negative; >= 0 are fine)
constexpr int kSegDesync = -20, kSegOverflow = -21, kSegNoStart = -22, kSegEndsEarly = -23;

// What a piece that decoded cleanly says about its ends.  A piece in front of another start (bit_end) has met it exactly -- a final
// block on the way is a member that ends in front of where it is said to (kSegEndsEarly).  A member's last piece (bit_end = ~0) runs
// to the final block, which must end inside the last byte of the member's payload [.., lim): in front of it the member ends early
// (bytes between the stream and the trailer: zlib reads the trailer there), behind it the reader's bound has cut the piece short.
MKZ_HD int seg_end_status(uint64_t bit_end, uint64_t lim, uint64_t stop, bool fin) {
    if (bit_end != ~0ull) return fin ? kSegEndsEarly : stop != bit_end ? kSegDesync : 0;
    return !fin ? kSegDesync : stop + 8 <= lim * 8 ? kSegEndsEarly : 0;
}

// Element k of the context of a segment whose text starts at byte text_off of the whole text is byte text_off - 32 768 + k of it:
// how many elements at the context's front lie in front of the stream's first byte.  A symbol that is the place-holder of one of
// them is a distance "too far back" (RFC 1951 3.2.3: a distance never reaches beyond the beginning of the output stream).
MKZ_HD uint32_t seg_context_before_stream(uint64_t text_off) { return text_off < kSegPrefix ? kSegPrefix - (uint32_t)text_off : 0u; }
MKZ_HD bool seg_before_stream(uint16_t symbol, uint32_t before) { return (symbol & kSegUnknown) && (uint32_t)(symbol & 0x7fffu) < before; }

// ---- bit reader: straight from global memory, one dword ahead --------------------------------------------------------------------
// (the member names of LaneReader, inflate_serial.hpp: dynamic_header() runs over either)
struct SegReader {
    const uint8_t *in;
    uint64_t n_in;  // bytes of the stream; readable up to n_in + kStreamPad
    uint64_t pos;   // byte offset of the dword behind `ahead`
    uint64_t bitbuf;
    uint32_t bitcnt, ahead;

    MKZ_HD uint32_t load(uint64_t byte) const { return byte <= n_in + 8 ? load_le32(in + byte) : 0u; }
    MKZ_HD void need32() {
        if (bitcnt < 32) {
            bitbuf |= (uint64_t)ahead << bitcnt;
            bitcnt += 32;
            ahead = load(pos);  // (asked for one refill before it is needed)
            pos += 4;
        }
    }
    MKZ_HD void take(uint32_t n) { bitbuf >>= n, bitcnt -= n; }
    MKZ_HD uint64_t bitpos() const { return (pos - 4) * 8 - bitcnt; }  // bits consumed so far
    MKZ_HD bool ran_out() const { return bitpos() > n_in * 8; }
    MKZ_HD void seek(uint64_t bit) {
        pos = bit >> 3;
        bitbuf = 0, bitcnt = 0;
        ahead = load(pos);
        pos += 4;
        need32();
        take((uint32_t)bit & 7u);
    }
};

// The header of a block is read by dynamic_header() / fixed_tables() of inflate_serial.hpp, the lane decoder's own; with no table
// memory dynamic_header() is the strict test of a block start (seg_header_plausible below).
// The first two levels of that test on their own (the search kernel runs them on all positions / on the survivors, so that the lanes of
// a wave do the same work at the same time).  Level 1: BFINAL = 0, BTYPE = dynamic, HLIT / HDIST in range -- the 13 bits `v` at the
// position (1 in 9 passes).  Level 2: the code-length code is complete and not empty (~1 in 100 of those).
MKZ_HD bool seg_header_bits_plausible(uint32_t v) { return (v & 7u) == 4u && ((v >> 3) & 31u) <= 29u && ((v >> 8) & 31u) <= 29u; }
MKZ_HD bool seg_header_cl_plausible(const uint8_t *in, uint64_t n_in, uint64_t bit) {
    if (bit + 64 > n_in * 8) return false;
    SegReader r;
    r.in = in, r.n_in = n_in;
    r.seek(bit);
    if (!seg_header_bits_plausible((uint32_t)r.bitbuf)) return false;
    const uint32_t hclen = ((uint32_t)(r.bitbuf >> 13) & 15u) + 4;
    r.take(17);
    uint64_t cl = 0;
    for (uint32_t i = 0; i < hclen; ++i) {
        r.need32();
        cl |= (uint64_t)((uint32_t)r.bitbuf & 7u) << (3 * cl_order_at(i));
        r.take(3);
    }
    ClCode clc;
    return cl != 0 && cl_build(cl, clc) == 0;
}

// is `bit` the start of a non-final dynamic block, as far as its header says?  (registers only)
MKZ_HD bool seg_header_plausible(const uint8_t *in, uint64_t n_in, uint64_t bit) {
    if (bit + 64 > n_in * 8) return false;
    SegReader r;
    r.in = in, r.n_in = n_in;
    r.seek(bit);
    if (((uint32_t)r.bitbuf & 7u) != 4u) return false;  // BFINAL = 0, BTYPE = 10 (dynamic): bits 0 | 0 1 -> value 4
    r.take(3);
    return dynamic_header(r, nullptr) == 0;
}

// Decodes from bit0 (a block start).  Stops in front of the block that would start at bit_end (reaching it exactly is the proof
// that both ends are block starts), or behind the final block (*final_seen), or -- max_blocks > 0 -- after that many blocks.
// out: 16-bit symbols, out[-kSegPrefix .. -1] are the caller's place-holders; cap elements (+ kSegSlack writable).  out == nullptr:
// dry run (nothing is stored or copied: the bit stream alone is checked).  t: kLaneTableU16 16-bit words of table memory.
// Returns 0 or a negative code; *n_out = elements produced, *bit_stop = the bit position behind the last block decoded.
MKZ_HD int inflate_segment(const uint8_t *in, uint64_t n_in, uint64_t bit0, uint64_t bit_end, uint32_t max_blocks, uint16_t *out, uint64_t cap, uint16_t *t,
                           uint64_t *n_out, uint64_t *bit_stop, bool *final_seen) {
    SegReader r;
    r.in = in, r.n_in = n_in;
    r.seek(bit0);
    uint64_t op = 0;
    *final_seen = false;
    uint32_t blocks = 0;
    for (;;) {
        const uint64_t at = r.bitpos();
        if (at == bit_end || (max_blocks && blocks == max_blocks)) break;
        if (at > bit_end) {  // passed over bit_end: it is not a block start (*bit_stop: the block boundary behind it)
            *n_out = op, *bit_stop = at;
            return kSegDesync;
        }
        r.need32();
        if (r.ran_out()) return kInfTruncated;
        const uint32_t final_block = (uint32_t)r.bitbuf & 1u, type = ((uint32_t)r.bitbuf >> 1) & 3u;
        r.take(3);
        ++blocks;
        if (type == 3) return kInfBadBlockType;
        if (type == 0) {
            r.take(r.bitcnt & 7);
            r.need32();
            const uint32_t len = (uint32_t)r.bitbuf & 0xffffu, nlen = ((uint32_t)(r.bitbuf >> 16)) & 0xffffu;
            r.take(32);
            if ((len ^ nlen) != 0xffffu) return kInfBadStored;
            const uint64_t pos = r.bitpos() >> 3;  // (byte-aligned here)
            if (r.ran_out() || pos > n_in || len > n_in - pos) return kInfTruncated;
            if (len > cap - op) return kSegOverflow;
            if (out)
                for (uint32_t i = 0; i < len; ++i) out[op + i] = in[pos + i];
            op += len;
            r.seek((pos + len) * 8);
        } else {
            if (type == 1) {
                fixed_tables(t);
            } else {
                const int rc = dynamic_header(r, t);
                if (rc) return rc;
            }
            const uint16_t *ll_sorted = t + kOffLlSorted, *d_sorted = t + kOffDSorted, *ll_limit = t + kOffLlLimit, *ll_base = t + kOffLlBase,
                           *d_limit = t + kOffDLimit, *d_base = t + kOffDBase;
            for (;;) {
                r.need32();
                const uint32_t e = decode_codeword((uint32_t)r.bitbuf, ll_sorted, ll_limit, ll_base);
                r.take(e & 15u);
                const uint32_t sym = e >> 4;
                if (e == 0) return kInfBadSymbol;
                if (r.ran_out()) return kInfTruncated;
                if (sym < 256) {
                    if (op >= cap) return kSegOverflow;
                    if (out) out[op] = (uint16_t)sym;
                    ++op;
                    continue;
                }
                if (sym == 256) break;
                if (sym > 285) return kInfBadSymbol;
                const uint32_t idx = sym - 257;
                const uint32_t leb = length_extra_bits(idx);
                const uint32_t len = length_base(idx) + ((uint32_t)r.bitbuf & ((1u << leb) - 1));
                r.take(leb);
                r.need32();
                const uint32_t d = decode_codeword((uint32_t)r.bitbuf, d_sorted, d_limit, d_base);
                r.take(d & 15u);
                const uint32_t dsym = d >> 4;
                if (d == 0 || dsym > 29) return kInfBadSymbol;
                const uint32_t deb = distance_extra_bits(dsym);
                const uint32_t dist = distance_base(dsym) + ((uint32_t)r.bitbuf & ((1u << deb) - 1));
                r.take(deb);
                if (len > cap - op) return kSegOverflow;
                if (out) {
                    // the match as bytes of the 16-bit buffer: 2 len bytes from 2 dist bytes back (the place-holder prefix is
                    // ordinary memory: a match that reaches in front of the segment copies place-holders)
                    uint8_t *dst = reinterpret_cast<uint8_t *>(out + op);
                    const uint8_t *src = dst - 2 * (uint64_t)dist;
                    const uint32_t nb = 2 * len;
                    if (dist >= 4) {  // 8 bytes a round: a round never reads what it writes
                        for (uint32_t k = 0; k < nb; k += 8) store_le64(dst + k, load_le64(src + k));
                    } else {  // a period of 2, 4 or 6 bytes, spread over a register and stored a whole number of periods at a time
                        const uint64_t v0 = load_le64(src);
                        const uint32_t period = 2 * dist;
                        uint64_t pat = 0;
                        for (uint32_t j = 0; j < 8; ++j) pat |= ((v0 >> (8 * (j % period))) & 0xffull) << (8 * j);
                        const uint32_t step = 8 - 8 % period;
                        for (uint32_t k = 0; k < nb; k += step) store_le64(dst + k, pat);
                    }
                }
                op += len;
            }
            if (r.ran_out()) return kInfTruncated;
        }
        if (final_block) {
            *final_seen = true;
            break;
        }
    }
    *n_out = op;
    *bit_stop = r.bitpos();
    return 0;
}

// does a block header follow at `bit` (where a candidate's block has ended) that can be checked: a stored block whose LEN and its
// complement agree, or a plausible dynamic one?  (registers only)
MKZ_HD bool seg_next_header_plausible(const uint8_t *in, uint64_t n_in, uint64_t bit) {
    if (bit + 3 > n_in * 8) return false;
    SegReader r;
    r.in = in, r.n_in = n_in;
    r.seek(bit);
    const uint32_t type = ((uint32_t)r.bitbuf >> 1) & 3u;
    r.take(3);
    if (type == 2) return dynamic_header(r, nullptr) == 0;
    if (type == 0) {
        r.take(r.bitcnt & 7);
        r.need32();
        const uint32_t len = (uint32_t)r.bitbuf & 0xffffu, nlen = ((uint32_t)(r.bitbuf >> 16)) & 0xffffu;
        return (len ^ nlen) == 0xffffu;
    }
    return false;  // (a fixed block behind it proves nothing: such a start is passed over, the chunk joins its predecessor; type 3 is none)
}

// a plausible header at `bit`: is it a block start?  Its block decodes cleanly (dry) and another block header follows at once.
// The whole-block form: the host harness cuts its streams with it (and the search kernel's first version did); the kernel now
// decodes the first symbols only (wave_confirm_block_start, gzip_segments_wave.hpp).
MKZ_HD bool seg_confirm_block_start(const uint8_t *in, uint64_t n_in, uint64_t bit, uint16_t *t) {
    uint64_t n_out = 0, stop = 0;
    bool fin = false;
    if (inflate_segment(in, n_in, bit, ~0ull, 1, nullptr, ~0ull, t, &n_out, &stop, &fin) != 0) return false;
    if (n_out == 0 || fin) return false;  // (the block at a nominal cut is neither empty nor the last one)
    return seg_next_header_plausible(in, n_in, stop);
}

}  // namespace mkz
