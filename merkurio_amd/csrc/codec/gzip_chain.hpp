// gzip_chain.hpp -- the host's part of the proof that a gzip file was cut at real member and block starts (gzip_segments.hpp says how
// the pieces are decoded): header parsing and member guesses, the candidate members of an upload, the piece table, the walk over a
// round's status words, where a window ends, text offsets and ISIZE, the CRC-32 fold.  No HIP: gzip_host.cpp runs it between the
// launches of gzip_inflate.hip (the whole file at once, or a window of it), tests/helpers/gzip_chain_harness.cpp runs it on the CPU
// with the serial decoder in the device's place, under sanitizers, against zlib.  Both run the same round loop (gzip_prove).
#pragma once
#include <string.h>

#include <algorithm>
#include <iterator>
#include <vector>

#include "../../../include/merkurio_hip.h"
#include "gzip_segments.hpp"

namespace mkz {

constexpr uint64_t kGzMaxPieces = 65535;  // pieces of one round (a grid dimension): more is not taken

// RFC 1952: does a member's header parse at gz[b ...]?  -> the offset of the byte behind it (FEXTRA / FNAME / FCOMMENT / FHCRC
// walked), with room for a DEFLATE stream (2 bytes at least) and the 8 trailer bytes inside the file; 0 = no header here
inline uint64_t gzip_header_end(const uint8_t *gz, uint64_t n, uint64_t b) {
    if (n - b < 10 + 2 + 8 || gz[b] != 0x1f || gz[b + 1] != 0x8b || gz[b + 2] != 8 || (gz[b + 3] & 0xE0)) return 0;
    const uint8_t flg = gz[b + 3];
    uint64_t p = b + 10;
    if (flg & 4) {
        if (p + 2 > n) return 0;
        p += 2 + (gz[p] | (uint64_t)gz[p + 1] << 8);
    }
    for (int bit = 3; bit <= 4; ++bit)
        if (flg & (1 << bit)) {
            const void *z = p < n ? memchr(gz + p, 0, (size_t)(n - p)) : nullptr;
            if (!z) return 0;
            p = (uint64_t)((const uint8_t *)z - gz) + 1;
        }
    if (flg & 2) p += 2;
    return p <= n && n - p >= 2 + 8 ? p : 0;
}

// mk_gzip_member_guesses (include/merkurio_hip.h): every place of gz[0, n) where a header parses -> how many; table[0, min(cap, that))
inline uint64_t gzip_member_guesses(const uint8_t *gz, uint64_t n, mk_gzip_guess *table, uint64_t cap) {
    if (n < 20 || !gzip_header_end(gz, n, 0)) return 0;  // (not a gzip file: no guesses)
    uint64_t k = 0;
    auto trailer = [&](uint64_t member, uint64_t end) {  // the 8 bytes in front of `end` are what the member in front of it ends with
        if (table && member < cap) memcpy(&table[member].crc, gz + end - 8, 4), memcpy(&table[member].isize, gz + end - 4, 4);
    };
    for (uint64_t b = 0; n - b >= 20;) {
        const uint64_t p = gzip_header_end(gz, n, b);
        if (p && (b == 0 || b >= 8)) {  // (behind the first one: with the room of a trailer in front of it)
            if (k) trailer(k - 1, b);
            if (table && k < cap) table[k] = mk_gzip_guess{b, p, 0, 0};
            ++k;
        }
        const void *next = memchr(gz + b + 1, 0x1f, (size_t)(n - b - 1));  // (ID1: one byte in 256)
        if (!next) break;
        b = (uint64_t)((const uint8_t *)next - gz);
    }
    trailer(k - 1, n);
    return k;
}

// A candidate member of the uploaded bytes up[0, n_in): its DEFLATE stream starts at bit pay_bit.  closed: its trailer (CRC-32,
// ISIZE) lies at up[end ...] -- host memory, inside the upload or right behind it.  Open (the last candidate of a window that is not
// the file's last): the trailer lies behind the upload, the member goes on in the next window.  header: the byte of the upload where
// its header parses -- where the next window starts when the member stays open without a proved block start (0 for the member a
// window continues, and where nobody asks).
struct GzCandidate {
    uint64_t pay_bit, header, end;
    bool closed;
};

inline uint32_t gzip_trailer_word(const uint8_t *up, const GzCandidate &m, int word) {  // 0: CRC-32, 1: ISIZE
    uint32_t v;
    memcpy(&v, up + m.end + 4 * word, 4);
    return v;
}

// Nominal chunks of compressed bytes (a block of zlib's is 15-40 KiB of them).  A piece is decoded by one wave at that wave's pace
// (~13 MB/s of text), so what counts is the largest piece and how many rounds of the device's decoder slots (17 per CU) the pieces
// make.  Cuts every 16 KiB give every block its own piece (no piece can be smaller); up to a round and a half of them that is the
// fastest (61 MB of stream: 27 ms against 37); above, cuts every 64 KiB (pieces of ~2 blocks, a third of the search waves) are
// (245 MB: 63 ms against 67).  At most 32 768 chunks (the prefix kernel's grid; a stream of more than 2 GiB gets larger chunks).
// set: mk_codec_set_gzip_chunk, 0 = by the rule.
inline uint64_t gzip_chunk_bytes(uint64_t n_in, uint64_t set, int num_cus) {
    uint64_t chunk = set ? set : (n_in / (32u << 10) <= (uint64_t)num_cus * 17 * 3 / 2 ? 16u << 10 : 64u << 10);
    while (n_in / chunk > 32768) chunk *= 2;
    return chunk;
}

// what the search reports per chunk (starts[0] is never searched: bit 0 is known; ~0 = none) -> the found starts, increasing
inline std::vector<unsigned long long> gzip_found_starts(const std::vector<unsigned long long> &starts) {
    std::vector<unsigned long long> found;
    for (size_t k = 1; k < starts.size(); ++k)
        if (starts[k] != ~0ull && (found.empty() || starts[k] > found.back())) found.push_back(starts[k]);
    return found;
}

// The candidates of a whole file that goes up as it is (mk_gzip_members_inflate_device): every guess, closed by the one behind it
inline std::vector<GzCandidate> gzip_file_candidates(const std::vector<mk_gzip_guess> &guesses, uint64_t n) {
    std::vector<GzCandidate> mem(guesses.size());
    for (size_t k = 0; k < guesses.size(); ++k)
        mem[k] = GzCandidate{guesses[k].data_off * 8, guesses[k].header_off, (k + 1 < guesses.size() ? guesses[k + 1].header_off : n) - 8, true};
    return mem;
}

// The first ratio of the one-shot calls.  ISIZE says how much text there is in all -- below 4 GiB of it: the first guess per piece is
// half as much again as the stream's own ratio, which spares a 1.27 GB FASTQ two thirds of a 6 GB allocation; a stream of 4 GiB of
// text or more starts at 12.
inline uint64_t gzip_first_ratio(const uint8_t *up, uint64_t n_up, const std::vector<GzCandidate> &mem) {
    uint64_t said_text = 0;
    for (const GzCandidate &m : mem) said_text += gzip_trailer_word(up, m, 1);
    const uint64_t whole_ratio = n_up ? said_text / n_up + 1 : 1;
    return (n_up < (1ull << 29) && said_text > n_up) ? std::min<uint64_t>(12, whole_ratio + whole_ratio / 2 + 1) : 12;
}

// A window of a stream uploads its nominal size: `window` compressed bytes, doubled `grow` times, and a margin behind them (a trailer
// and the fixed part of the next header).  It may grow as long as it does not hold the rest of the file already, 24 times at most.
constexpr uint64_t kGzStreamMargin = 64;
inline uint64_t gzip_window_nominal(uint64_t window, uint32_t grow) { return (window << grow) + kGzStreamMargin; }
inline bool gzip_window_may_grow(uint64_t pos_bit, uint64_t window, uint32_t grow, uint64_t n_file) {
    return (pos_bit >> 3) + gzip_window_nominal(window, grow) < n_file && grow < 24;
}

// The candidates of the window that starts at bit pos_bit of gz[0, n) and uploads n_up bytes from byte pos_bit >> 3: the member the
// window continues (in_member) or the header it starts at, then every guess inside the upload.  Every candidate but the last is
// closed by the guess behind it; the last one is closed by the file's end (is_last) and open otherwise.
// -> 0: mem stands; 2: bytes behind the last member that are no member; 3: the header does not fit the upload, the window grows
inline int gzip_window_candidates(const uint8_t *gz, uint64_t n, const std::vector<mk_gzip_guess> &guesses, uint64_t pos_bit, bool in_member, uint64_t n_up,
                                  bool is_last, std::vector<GzCandidate> &mem) {
    const uint64_t base = pos_bit >> 3;
    mem.clear();
    if (in_member) {
        mem.push_back(GzCandidate{pos_bit - base * 8, 0, 0, false});
    } else {
        const uint64_t p = gzip_header_end(gz, n, base);
        if (!p) return 2;
        if (p + 2 > base + n_up) return 3;
        mem.push_back(GzCandidate{(p - base) * 8, 0, 0, false});
    }
    const uint64_t from = base + (mem[0].pay_bit >> 3);
    auto g = std::upper_bound(guesses.begin(), guesses.end(), from, [](uint64_t v, const mk_gzip_guess &x) { return v < x.header_off; });
    for (; g != guesses.end() && g->data_off + 2 <= base + n_up; ++g) {
        if (g->header_off < base + 8) continue;  // (no room for a trailer in front of it inside this upload)
        mem.back().end = g->header_off - base - 8, mem.back().closed = true;
        mem.push_back(GzCandidate{(g->data_off - base) * 8, g->header_off - base, 0, false});
    }
    if (is_last) mem.back().end = n_up - 8, mem.back().closed = true;
    return 0;
}

// The piece table of a round.  Every member's first bit is a start that is KNOWN; of the searched ones those inside its payload are
// kept (one in a header or a trailer is none).  An open member's pieces end at found starts only, and the last of those is the cut
// (cut_bit; ~0: it has none) -- no piece is decoded behind it.
struct GzPieces {
    std::vector<unsigned long long> tab;   // bits | end | lim | off | cap, J of each: what goes to the device in one copy
    std::vector<uint32_t> seg_first;       // piece -> first piece of its member; [J] = J (what the kernels compare the last one's with)
    std::vector<uint32_t> mem_first;       // member -> its first piece (M + 1)
    uint32_t J = 0;
    uint64_t elems = 0;                    // 16-bit symbols of all pieces' buffers
    unsigned long long cut_bit = ~0ull;
    const unsigned long long *bits() const { return tab.data(); }
    const unsigned long long *end() const { return tab.data() + J; }
    const unsigned long long *lim() const { return tab.data() + 2 * (size_t)J; }
    const unsigned long long *off() const { return tab.data() + 3 * (size_t)J; }
    const unsigned long long *cap() const { return tab.data() + 4 * (size_t)J; }
};

// Room per piece: `ratio` x its compressed bytes (FASTQ / FASTA / text: 3-6 x).  false: more than kGzMaxPieces pieces
inline bool gzip_piece_table(const std::vector<GzCandidate> &mem, const std::vector<unsigned long long> &found, uint64_t n_in, uint64_t ratio, GzPieces &P) {
    const size_t M = mem.size();
    std::vector<unsigned long long> bits, end, lim, at;
    P.mem_first.assign(M + 1, 0), P.seg_first.clear();
    P.cut_bit = ~0ull;
    size_t f = 0;
    for (size_t m = 0; m < M; ++m) {
        P.mem_first[m] = (uint32_t)bits.size();
        const unsigned long long b0 = mem[m].pay_bit, b1 = mem[m].closed ? mem[m].end * 8 : n_in * 8;
        at.assign(1, b0);
        while (f < found.size() && found[f] <= b0) ++f;
        for (; f < found.size() && found[f] < b1; ++f) at.push_back(found[f]);
        if (!mem[m].closed) {  // (the last start is where the window ends)
            if (at.size() > 1) P.cut_bit = at.back();
            at.pop_back();
        }
        for (size_t j = 0; j < at.size(); ++j) {
            bits.push_back(at[j]);
            end.push_back(j + 1 < at.size() ? at[j + 1] : mem[m].closed ? ~0ull : P.cut_bit);
            // (a guess inside the header in front of it leaves no room: such a member reads nothing and fails)
            lim.push_back(mem[m].closed ? std::max(mem[m].end, mem[m].pay_bit >> 3) : n_in);
            P.seg_first.push_back(P.mem_first[m]);
        }
    }
    if (bits.size() > kGzMaxPieces) return false;
    const uint32_t J = P.J = (uint32_t)bits.size();
    P.mem_first[M] = J;
    P.seg_first.push_back(J);
    P.tab.assign((size_t)J * 5, 0);
    std::copy(bits.begin(), bits.end(), P.tab.begin()), std::copy(end.begin(), end.end(), P.tab.begin() + J), std::copy(lim.begin(), lim.end(), P.tab.begin() + 2 * (size_t)J);
    unsigned long long *seg_off = P.tab.data() + (size_t)J * 3, *seg_cap = seg_off + J;
    P.elems = 0;
    for (uint32_t j = 0; j < J; ++j) {
        const uint64_t b0 = bits[j] >> 3, b1 = end[j] != ~0ull ? end[j] >> 3 : lim[j];
        seg_cap[j] = 65536 + ratio * (b1 - b0 + 1);
        seg_off[j] = P.elems;
        P.elems += kSegPrefix + seg_cap[j] + kSegSlack;
        P.elems = (P.elems + 7) & ~7ull;  // (16-byte aligned buffers)
    }
    return true;
}

// What a round says.  The counters of the rounds spent travel with the ratio: three drop rounds, three join rounds, 12 -> 48 once.
enum GzVerdict { kGzProved, kGzDropStarts, kGzJoinMembers, kGzMoreRoom, kGzNotTaken };
struct GzRounds {
    uint64_t ratio = 12;
    int drop_rounds = 0, join_rounds = 0;
    uint32_t repeated = 0;  // rounds beyond the first
};

// The walk over a round's status[] / n_out[].  Member by member from the first: a piece that ends on the next start proves that start;
// the first piece that runs over its end (kSegDesync, and n_out says at which block boundary it stands) disproves the found starts in
// front of that boundary (what lies behind is looked at next time).  A member whose pieces do not add up otherwise ends somewhere else
// than at the guess behind it: that guess goes, the member is joined with the next one.  What follows a dropped guess says nothing
// until a member decodes whole again (a real one: the walk goes on from there, `anchored`, so that false guesses in several members
// cost one round, not one each).  An open member has no last piece to judge, and every one of its pieces ends at a found start.
// Drops and joins are applied to found / mem here; kGzMoreRoom has set the ratio to 48.
inline GzVerdict gzip_judge(std::vector<GzCandidate> &mem, std::vector<unsigned long long> &found, const GzPieces &P, const int32_t *status,
                            const unsigned long long *n_out, uint64_t n_in, GzRounds &R) {
    const size_t M = mem.size();
    const unsigned long long *bits = P.bits();
    bool overflow = false, anchored = true;
    std::vector<char> join(M, 0);  // member m ends at no member start: it is joined with member m + 1
    std::vector<unsigned long long> gone;
    for (size_t m = 0; m < M; ++m) {
        if (m && join[m - 1]) continue;  // (it starts at the guess that has just gone)
        int32_t st = 0;
        uint32_t at = P.mem_first[m];
        bool over = false;
        for (; at < P.mem_first[m + 1] && st == 0; ++at) {
            if (status[at] == kSegOverflow) over = true;
            else st = status[at];
        }
        if (st == 0 && !over) {
            anchored = true;
            continue;
        }
        if (!anchored) continue;
        if (st == 0) {
            overflow = true;
        } else if (st == kSegDesync && (at < P.mem_first[m + 1] || !mem[m].closed)) {  // (not a closed member's last piece: that one ran to no start)
            // The starts that go: found x inside the member with from < x < stands_at.  In a closed member these are the pieces
            // bits[at ..] of the member below stands_at -- every piece behind the member's first IS a found start inside (b0, b1),
            // in increasing order, and bits[at - 1] = from -- which is how the one-shot call used to collect them; in an open member
            // the cut, which is no piece's first bit, is among them too.
            const unsigned long long from = bits[at - 1], stands_at = n_out[at - 1], b1 = mem[m].closed ? mem[m].end * 8 : n_in * 8;
            const size_t before = gone.size();
            for (unsigned long long x : found)
                if (x > from && x < stands_at && x < b1) gone.push_back(x);
            if (gone.size() == before) return kGzNotTaken;  // (nothing to drop: not what this is for)
        } else {
            if (m + 1 == M) return kGzNotTaken;  // (no guess to drop: a stream that does not decode, or ends elsewhere -- zlib will say what this file is)
            join[m] = 1, anchored = false;
        }
    }
    if (!gone.empty()) {
        if (++R.drop_rounds > 3) return kGzNotTaken;
        std::sort(gone.begin(), gone.end());  // (member by member they come in order already; set_difference depends on it)
        std::vector<unsigned long long> kept;
        std::set_difference(found.begin(), found.end(), gone.begin(), gone.end(), std::back_inserter(kept));
        found.swap(kept);
    }
    if (std::find(join.begin(), join.end(), 1) != join.end()) {
        if (++R.join_rounds > 3) return kGzNotTaken;
        std::vector<GzCandidate> left;
        for (size_t m = 0; m < M; ++m) {
            if (m && join[m - 1]) left.back().end = mem[m].end, left.back().closed = mem[m].closed;
            else left.push_back(mem[m]);
        }
        mem.swap(left);
        return kGzJoinMembers;
    }
    if (!gone.empty()) return kGzDropStarts;
    if (!overflow) return kGzProved;
    if (R.ratio == 48) return kGzNotTaken;
    R.ratio = 48;
    return kGzMoreRoom;
}

// The rounds: table, decode, walk, until the chain is proved or given up.  decode(P, n_out, status) decodes the J pieces of P into
// n_out[J] / status[J] (codes of gzip_segments.hpp) and returns false when it cannot (no room, a device error: the caller knows which).
// true: every member left decoded from its first bit to a final block that ends in its last payload byte (an open one: to the cut) --
// the chain zlib walks, since a DEFLATE stream decoded from a given bit has one end.  P / n_out are the last round's.  P.J == 0 (one
// open member without a found start) is "proved" with nothing decoded: gzip_window_end makes that window grow.
template <class Decode>
bool gzip_prove(std::vector<GzCandidate> &mem, std::vector<unsigned long long> &found, uint64_t n_in, GzRounds &R, GzPieces &P,
                std::vector<unsigned long long> &n_out, Decode &&decode) {
    std::vector<int32_t> status;
    for (;; ++R.repeated) {
        if (!gzip_piece_table(mem, found, n_in, R.ratio, P)) return false;
        n_out.assign(P.J, 0), status.assign(P.J, 0);
        if (!P.J) return true;
        if (!decode(P, n_out.data(), status.data())) return false;
        const GzVerdict v = gzip_judge(mem, found, P, status.data(), n_out.data(), n_in, R);
        if (v == kGzProved || v == kGzNotTaken) return v == kGzProved;
    }
}

// Where a proved window ends: behind the file's last member; at the open member's cut; at the open member's header when it has no
// proved start but closed members stand in front of it (it begins the next window, header first).
// -> 0 and *next_bit / *next_in_member; 3: no proved start to stop at, the window grows (2 where it cannot: the file's last window)
inline int gzip_window_end(const std::vector<GzCandidate> &mem, unsigned long long cut_bit, uint64_t pos_bit, bool in_member, uint64_t n_file, bool is_last,
                           uint64_t *next_bit, bool *next_in_member) {
    const uint64_t base = pos_bit >> 3;
    const GzCandidate &last = mem.back();
    if (last.closed) *next_bit = n_file * 8, *next_in_member = false;
    else if (cut_bit != ~0ull) *next_bit = base * 8 + cut_bit, *next_in_member = true;
    else if (mem.size() > 1) *next_bit = (base + last.header) * 8, *next_in_member = false;
    else *next_bit = pos_bit, *next_in_member = in_member;
    if (*next_bit <= pos_bit && !last.closed) return is_last ? 2 : 3;
    return 0;
}

// A closed member's text against its trailer's ISIZE.  whole (the one-shot calls: the member lies in the upload from its first bit):
// below 4 GiB and exactly as long.  Else (a window): modulo 2^32 (RFC 1952), `before` = what the member had in front of the window.
inline bool gzip_isize_agrees(uint64_t text_len, uint64_t before, uint32_t isize, bool whole) {
    if (whole) return !(text_len >> 32) && (uint32_t)text_len == isize;
    return (uint32_t)(text_len + before) == isize;
}

// where every piece's text goes (the members' texts back to back), how long every member's is
struct GzText {
    std::vector<unsigned long long> off;  // per piece (one element at least)
    std::vector<uint64_t> mem_text;
    uint64_t total = 0;
    uint32_t max_member_segs = 1;
    // the last member's text (an open one's: what the carry is made of); a member without a piece: the text's end
    uint64_t last_member_off(const GzPieces &P) const { return P.J && P.mem_first[mem_text.size() - 1] < P.J ? off[P.mem_first[mem_text.size() - 1]] : total; }
};
// false: a closed member's text is not as long as its trailer says.  open_len: of mem[0] in front of the window (0: it starts here)
inline bool gzip_text_offsets(const std::vector<GzCandidate> &mem, const GzPieces &P, const std::vector<unsigned long long> &n_out, const uint8_t *up, bool whole,
                              uint64_t open_len, GzText &T) {
    const size_t M = mem.size();
    T.off.assign(std::max<uint32_t>(P.J, 1), 0), T.mem_text.assign(M, 0);
    T.total = 0, T.max_member_segs = 1;
    for (size_t m = 0; m < M; ++m) {
        for (uint32_t j = P.mem_first[m]; j < P.mem_first[m + 1]; ++j) T.off[j] = T.total, T.total += n_out[j], T.mem_text[m] += n_out[j];
        if (mem[m].closed && !gzip_isize_agrees(T.mem_text[m], m == 0 ? open_len : 0, gzip_trailer_word(up, mem[m], 1), whole)) return false;
        T.max_member_segs = std::max(T.max_member_segs, P.mem_first[m + 1] - P.mem_first[m]);
    }
    return true;
}

// CRC-32 of every member's text: per block of at most block_bytes on the device (the BGZF writer's wave), the grid cut member by
// member, folded here: crc(A ++ B) = crc(A) * x^(8 |B|) mod P  ^  crc(B)
inline void gzip_crc_blocks(const GzPieces &P, const GzText &T, uint32_t block_bytes, std::vector<unsigned long long> &blk_off, std::vector<uint32_t> &blk_len) {
    blk_off.clear(), blk_len.clear();
    for (size_t m = 0; m < T.mem_text.size(); ++m)
        for (uint64_t at = 0; at < T.mem_text[m]; at += block_bytes)
            blk_off.push_back(T.off[P.mem_first[m]] + at), blk_len.push_back((uint32_t)std::min<uint64_t>(block_bytes, T.mem_text[m] - at));
}
// crcs[b] of the blocks above -> mem_crc[m], mem[0]'s folded onto open_crc (what it had in front of the window; 0: it starts here).
// false: a closed member's differs from its trailer's
inline bool gzip_crc_fold(const std::vector<GzCandidate> &mem, const GzText &T, const std::vector<uint32_t> &blk_len, const uint32_t *crcs, uint32_t block_bytes,
                          const uint8_t *up, uint32_t open_crc, std::vector<uint32_t> &mem_crc) {
    const uint32_t shift_full = crc_x_pow_bytes(block_bytes);
    mem_crc.assign(mem.size(), 0);
    size_t b = 0;
    for (size_t m = 0; m < mem.size(); ++m) {
        uint32_t crc = m == 0 ? open_crc : 0;
        for (uint64_t at = 0; at < T.mem_text[m]; at += block_bytes, ++b) crc = crc_mulmod(crc, blk_len[b] == block_bytes ? shift_full : crc_x_pow_bytes(blk_len[b])) ^ crcs[b];
        mem_crc[m] = crc;
        if (mem[m].closed && crc != gzip_trailer_word(up, mem[m], 0)) return false;
    }
    return true;
}

// what a stream carries from window to window
struct GzStreamPos {
    uint64_t pos_bit = 0;    // first bit of the next window
    bool in_member = false;  // pos_bit lies inside a member's DEFLATE stream (else: at a header, or at the file's end)
    uint32_t open_crc = 0;   // of the open member's text so far
    uint64_t open_len = 0;
    uint32_t carry_len = 0;  // real bytes at the end of the 32 KiB carried in front of pos_bit
};
// does the member that stays open behind this window continue the one the window continued (its carry then stands in front of the new one)?
inline bool gzip_window_continues(const GzStreamPos &at, size_t members, bool next_in_member) { return next_in_member && members == 1 && at.in_member; }
// the window stands: what the next one starts from.  t_open / crc_open: the text of the member that stays open, its CRC-32 so far
inline void gzip_window_stands(GzStreamPos &at, size_t members, uint64_t t_open, uint32_t crc_open, uint64_t next_bit, bool next_in_member) {
    if (next_in_member) {
        const bool continued = gzip_window_continues(at, members, next_in_member);
        at.carry_len = (uint32_t)std::min<uint64_t>(kSegPrefix, (continued ? at.carry_len : 0) + t_open);
        at.open_crc = crc_open;
        at.open_len = (continued ? at.open_len : 0) + t_open;
    } else {
        at.carry_len = 0, at.open_crc = 0, at.open_len = 0;
    }
    at.pos_bit = next_bit, at.in_member = next_in_member;
}

}  // namespace mkz
