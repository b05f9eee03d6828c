// codec_kernels.h -- launchers of the device BGZF codec (bgzf_deflate.hip, bgzf_inflate.hip), called by the host side
// of the C ABI's mk_codec entry points (codec_host.cpp).
//
// BGZF (SAM specification §4.1) = gzip members of at most 64 KiB, each a raw DEFLATE stream (RFC 1951) between an
// 18-byte header (with the member's size in a 'BC' extra field) and CRC-32 + ISIZE.  The reference reads and writes
// them through `bam 0.1.4` / flate2 on `tag`'s reader and writer threads (src/cmd_tag.rs:254-271,503-615) and reads
// bgzip'ed FASTA/FASTQ through needletail (src/cmd_extract.rs:281).  Members are independent: one wave (deflate) or
// one lane (inflate) per member.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bgzf_cuts.hpp"

namespace mkz {

constexpr uint32_t kSlotBytes = 65536;       // a member never exceeds 64 KiB (BSIZE is 16 bits)
constexpr uint32_t kMaxBlockBytes = 0xff00;  // input bytes per member (what htslib / the host writer use)
constexpr uint32_t kTokensPerWave = 65536;   // token scratch of one resident deflate wave (u32 each)
static_assert(kCutGrid + kCutReach == kMaxBlockBytes, "members that end at record ends hold kMaxBlockBytes at most (bgzf_cuts.hpp)");
constexpr uint32_t kCutBlocks = 8;           // the cut kernel's grid: at most this many blocks of 128 lanes, which stride over the grid points
constexpr uint32_t kPad = 128;               // readable bytes every input buffer needs behind its last byte (inflate_serial.hpp: kStreamPad)

// one member of an inflate call (the host walks the BSIZE chain and fills these)
struct Member {
    uint64_t data_off;  // raw DEFLATE stream inside the compressed buffer
    uint64_t out_off;   // where its text goes
    uint32_t data_len, isize, crc;
    uint32_t pad_;
};

// CRC-32 of every block_bytes-sized block of in[0, n) (the last one may be shorter) -> crc[b]
void launch_crc(const uint8_t *in, uint64_t n, uint32_t block_bytes, uint32_t n_blocks, uint32_t *crc, hipStream_t s);
// CRC-32 of in[off[b], off[b] + len[b]) -> crc[b], b < n_ranges (off, len: device memory)
void launch_crc_ranges(const uint8_t *in, const unsigned long long *off, const uint32_t *len, uint32_t n_ranges, uint32_t *crc, hipStream_t s);
// CRC-32 of the members' text out[out_off, out_off + isize) compared with Member::crc; status[i] |= 0x100 on a mismatch
void launch_crc_check(const uint8_t *out, const Member *members, uint32_t n_members, int32_t *status, hipStream_t s);

// Deflate: block b of in -> one complete BGZF member in slots[b * kSlotBytes ...], its size in slot_len[b].
// tokens: kTokensPerWave u32 per launched wave (deflate_grid(n_blocks) waves); `in` readable up to in + n + kPad.
uint32_t deflate_grid(uint32_t n_blocks, int num_cus);
// next_block: one u32 of device memory (the kernel's work counter; zeroed by the launcher)
void launch_deflate(const uint8_t *in, uint64_t n, uint32_t block_bytes, uint32_t n_blocks, const uint32_t *crc, uint32_t *tokens,
                    uint8_t *slots, uint32_t *slot_len, uint32_t *next_block, uint32_t grid, hipStream_t s);
// The same with member b = in[off[b], off[b] + len[b]) (off, len: device memory; len[b] <= kMaxBlockBytes): members that end where
// the caller's table says, not every block_bytes.  `in` readable up to kPad bytes behind the last range.
void launch_deflate_ranges(const uint8_t *in, const unsigned long long *off, const uint32_t *len, uint32_t n_blocks, const uint32_t *crc, uint32_t *tokens,
                           uint8_t *slots, uint32_t *slot_len, uint32_t *next_block, uint32_t grid, hipStream_t s);
// The range table of a text of n_text > 0 bytes whose records end at rec_end[0, n_rec) (device memory, non-decreasing, the last one =
// n_text) by the cut rule of include/merkurio_hip.h: n_grid = ceil(n_text / kCutGrid) grid points -> off / len[0, *n_members),
// *n_members = n_grid or n_grid - 1 (room for n_grid entries)
void launch_cuts(const unsigned long long *rec_end, uint64_t n_rec, uint64_t n_text, uint32_t n_grid, unsigned long long *off, uint32_t *len,
                 uint32_t *n_members, hipStream_t s);
// slot_len[0, n_blocks) -> slot_off (exclusive sums, u64) and *total; then the members back to back
void launch_pack(const uint8_t *slots, const uint32_t *slot_len, uint64_t *slot_off, uint64_t *total, uint32_t n_blocks, uint8_t *packed,
                 hipStream_t s);

// Inflate: member i of `in` -> out[out_off, out_off + isize); status[i] = 0 or an error code of inflate_serial.hpp.
// `in` readable up to in + n_in + kPad.
// (1 to 64 members per wave, by how many there are: inflate_lanes)
uint32_t inflate_lanes(uint32_t n_members, int num_cus);
// which: 3 / 4 = a wave per member with a ring of 8 / 16 KiB (measurement); 0 = by the number of members (up to kWaveMembersMax per CU-quarter... see bgzf_inflate.hip), 1 = one lane per member
// (bgzf_inflate.hip), 2 = one wave per member with the text in LDS (bgzf_inflate_wave.hip)
void launch_inflate(const uint8_t *in, uint64_t n_in, const Member *members, uint32_t n_members, uint8_t *out, int32_t *status, int num_cus,
                    hipStream_t s, int which = 0);
// ring_bytes: 32768 (all of a member's reach in LDS, 4 waves per CU), 16384 (7) or 8192 (12; far matches read flushed text back)
void launch_inflate_wave(const uint8_t *in, uint64_t n_in, const Member *members, uint32_t n_members, uint8_t *out, int32_t *status, hipStream_t s,
                         uint32_t ring_bytes = 32768);

// ---- a gzip file inflated in parallel pieces: one member, or a chain of them (gzip_inflate.hip, gzip_segments.hpp) ----
// starts[c] (c = 1 .. n_chunks - 1) = bit position of the first confirmed block start at or behind byte c * chunk_bytes, searched
// over search_bytes; ~0 = none
void launch_gzip_find(const uint8_t *in, uint64_t n_in, uint64_t chunk_bytes, uint32_t n_chunks, uint64_t search_bytes, unsigned long long *starts,
                      hipStream_t s);
// segment j = bits [seg_bits[j], seg_end[j]) of `in` (seg_end[j] = ~0: a member's last piece, to the final block), read no further than
// byte seg_lim[j] (the end of its member's payload) -> 16-bit symbols in sym[seg_off[j] + 32768 ...], at most seg_cap[j] of them;
// n_out[j], status[j]
void launch_gzip_segments(const uint8_t *in, const unsigned long long *seg_bits, const unsigned long long *seg_end, const unsigned long long *seg_lim,
                          const unsigned long long *seg_off, const unsigned long long *seg_cap, uint32_t n_seg, uint16_t *sym, unsigned long long *n_out,
                          int32_t *status, int num_cus, hipStream_t s, bool lane_per_segment = false);
// (the same with a wave per segment: gzip_segments_wave.hip; the place-holders must lie in front of every segment already)
void launch_gzip_segments_wave(const uint8_t *in, const unsigned long long *seg_bits, const unsigned long long *seg_end, const unsigned long long *seg_lim,
                               const unsigned long long *seg_off, const unsigned long long *seg_cap, uint32_t n_seg, uint16_t *sym, unsigned long long *n_out,
                               int32_t *status, hipStream_t s);
// contexts (n_seg x 32 KiB) and the text: text[text_off[j] ...] = segment j's bytes; *bad != 0: a symbol that is neither.  The chain of
// contexts restarts at every member: seg_first[j] = the first segment of segment j's member, max_member_segs = the most segments a member has
void launch_gzip_resolve(const uint16_t *sym, const unsigned long long *seg_off, const unsigned long long *n_out, const unsigned long long *text_off,
                         const uint32_t *seg_first, uint32_t n_seg, uint32_t max_member_segs, uint8_t *ctx, uint8_t *text, uint32_t *bad, hipStream_t s,
                         const uint8_t *carry = nullptr, uint32_t carry_len = 0);
// a window of a stream (mk_gzip_stream_next).  launch_gzip_resolve with carry != nullptr: segment 0 continues a member whose last 32 KiB
// of text in front of the window are carry[0, 32768) (carry_len of them real, at the buffer's end): its context, and what counts as
// "inside the stream" for the member's segments.  launch_gzip_carry: next = the last 32 KiB of (prev ++ text[0, n)), prev = nullptr: of
// text alone (zeros in front of it)
void launch_gzip_carry(const uint8_t *text, uint64_t n, const uint8_t *prev, uint8_t *next, hipStream_t s);

// ---- a .bz2 file, a wave per block (bzip2_inflate.hip, bzip2_serial.hpp, bzip2_stream.hpp) ----
// in[0, n) (zeros up to n_words dwords behind it) -> table[0, min(*count, cap)) = bit << 1 | kind of every block / end-of-stream magic, in no order
void launch_bz2_markers(const uint8_t *in, uint64_t n, uint64_t n_words, unsigned long long *table, uint32_t cap, uint32_t *count, int num_cus, hipStream_t s);
// blocks first .. first + count - 1 of the tables blk_bit / blk_level / blk_pre (device memory): header, symbols, inverse-BWT vector.
// Block b's bytes go to pre + blk_pre[b] (cap = its level's symbols rounded up to 128 bytes, then cap / 8 bytes for the walk's count
// bits), its selectors and vector to slot b - first of scratch (slot_bytes >= kBzSelBytes + 4 x cap); rep[b] = its Bz2Block
void launch_bz2_decode(const uint8_t *in, uint64_t n, uint64_t n_words, const unsigned long long *blk_bit, const uint32_t *blk_level, const unsigned long long *blk_pre,
                       uint8_t *pre, uint8_t *scratch, uint64_t slot_bytes, uint32_t first, uint32_t count, void *rep, hipStream_t s);
// the same blocks' vectors walked from origPtr: the bytes in front of the run-length step and their count bits to pre, text_len[b]
void launch_bz2_walk(const unsigned long long *blk_pre, const uint32_t *blk_level, uint8_t *pre, const uint8_t *scratch, uint64_t slot_bytes, uint32_t first,
                     uint32_t count, void *rep, unsigned long long *text_len, hipStream_t s);
// every block's text to text + text_off[b]; then bzip2's CRC-32 of it to crc[b]
void launch_bz2_expand(const unsigned long long *blk_pre, const uint32_t *blk_level, const uint8_t *pre, const void *rep, const unsigned long long *text_off,
                       uint8_t *text, uint32_t n_blocks, hipStream_t s);
void launch_bz2_crc(const uint8_t *text, const unsigned long long *text_off, const unsigned long long *text_len, uint32_t *crc, uint32_t n_blocks, hipStream_t s);

// ---- a .zst file, a wave per block (zstd_inflate.hip, zstd_serial.hpp, zstd_plan.hpp) ----
// blocks[0, n_blocks) (ZsBlock, device memory) of in[0, n) (zeros up to n_words dwords behind it): literals to lit, sequences to ll / ml /
// of at the blocks' slices, rep[b] = its ZsReport
void launch_zs_decode(const uint8_t *in, uint64_t n, uint64_t n_words, const void *blocks, uint32_t n_blocks, uint8_t *lit, uint32_t *ll, uint32_t *ml, uint32_t *of,
                      void *rep, hipStream_t s);
// the same blocks executed from start[b] (ZsStart): text, and per text byte kZsResolved or the position it copies from; status[b],
// *open_total += the bytes left as positions.  text[0, settled) is final (a stream's history; the one-shot call: 0): read as bytes
void launch_zs_execute(const uint8_t *in, const void *blocks, const void *start, const void *rep, uint32_t n_blocks, uint8_t *lit, uint32_t *ll, uint32_t *ml,
                       uint32_t *of, uint8_t *text, uint32_t *src, uint64_t settled, int32_t *status, unsigned long long *open_total, hipStream_t s);
// one round of pointer doubling over text[first, total): sources a -> b; *open_total += the bytes still open
void launch_zs_resolve(const uint32_t *a, uint32_t *b, uint8_t *text, uint64_t first, uint64_t total, unsigned long long *open_total, int num_cus, hipStream_t s);

// ---- an .xz file, a wave per block (xz_inflate.hip, lzma_serial.hpp, xz_plan.hpp) ----
// blocks[0, n_blocks) (XzBlock, device memory) of the file in `in` (zeros up to n_words dwords behind it): block b's text to
// text + its text_off, status[b] = 0 or the refusal.  lclp_room: the largest lc + lp the launch's LDS has room for.  order (device
// memory, may be null): workgroup i handles block order[i] (a stream's window: largest text first); null: block i
size_t xz_decode_lds_bytes(uint32_t lclp_room);
void launch_xz_decode(const uint8_t *in, uint64_t n_words, const void *blocks, const uint32_t *order, uint32_t n_blocks, uint8_t *text, uint32_t lclp_room,
                      int32_t *status, hipStream_t s);
// every decoded block's CRC-32 / CRC-64 against its stored check: check[b] = 0 or kLzCheck
void launch_xz_check(const uint8_t *in, const void *blocks, const uint32_t *order, uint32_t n_blocks, const uint8_t *text, const int32_t *status, int32_t *check,
                     hipStream_t s);

// ---- zstd frames written on the device, a wave per frame (zstd_deflate.hip, zstd_enc_serial.hpp) ----
constexpr uint32_t kZsDeflateSlotBytes = 131328;       // a frame never exceeds 16 bytes + 128 KiB of text (a Raw block)
constexpr uint32_t kZsDeflateLitBytes = 131136;        // literal scratch of one resident wave
constexpr uint32_t kZsDeflateSeqCap = 43712;           // sequences a block holds at most (128 KiB / the minimum match of 3), rounded up
constexpr uint64_t kZsDeflateWaveScratch = 1005376;    // literals + five u32 per sequence
uint32_t zstd_deflate_grid(uint32_t n_frames, int num_cus);
// the range table of the frames of a text (launch_cuts with kZsCutGrid / kZsCutReach)
void launch_zstd_cuts(const unsigned long long *rec_end, uint64_t n_rec, uint64_t n_text, uint32_t n_grid, unsigned long long *off, uint32_t *len,
                      uint32_t *n_frames, hipStream_t s);
// frame b = in[off[b], off[b] + len[b]) (len[b] <= 128 KiB) -> slots[b * kZsDeflateSlotBytes ...], slot_len[b]; kinds[0 .. 2] += Raw / RLE /
// Compressed blocks.  scratch: kZsDeflateWaveScratch bytes per launched wave; `in` readable up to kPad bytes behind the last range
void launch_zstd_deflate(const uint8_t *in, const unsigned long long *off, const uint32_t *len, uint32_t n_frames, uint8_t *scratch, uint8_t *slots,
                         uint32_t *slot_len, uint32_t *next_frame, uint32_t *kinds, uint32_t grid, hipStream_t s);
void launch_zstd_pack(const uint8_t *slots, const uint32_t *slot_len, uint64_t *slot_off, uint64_t *total, uint32_t n_frames, uint8_t *packed, hipStream_t s);

}  // namespace mkz
