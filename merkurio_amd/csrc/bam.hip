// bam.hip -- a window of inflated BAM text on the device (r05): the record chain becomes a
// record table, the 4-bit sequences become the ASCII text the matcher scans, and the kept records leave with their
// `km` tag appended -- what the reference's reader thread, record loop and writer do one record at a time
// (src/cmd_tag.rs:503-615 `for record in reader`, :387-497 process_record, bam 0.1.4's record layout = SAM
// specification §4.2) -- so that between inflate and deflate the records never visit the host.
//
// BAM records are a CHAIN: record k + 1 starts 4 + block_size bytes behind record k, which only a serial walk can
// follow.  The chain is cut into pieces of kPiece bytes of text:
//   mk_bam_find_kernel   a wave per piece looks for the first position at or behind the piece's first byte where four
//                        records in a row have consistent fixed fields (sizes that add up, a printable NUL-terminated
//                        name, reference ids and positions >= -1) -- a GUESS;
//   mk_bam_walk_kernel   a lane per piece walks from its start to the first record start at or behind the next piece's
//                        first byte (counting, then -- with the pieces' record counts summed -- writing the table);
// and the guesses are PROVED by the host from two small arrays: piece 0 starts at a record start by contract, and if
// every walk lands exactly on the next piece's start, every start is one (induction) and the table is the serial
// walk's.  A start that is not met is replaced by the landing and the walks run again (a false guess costs a round; no
// guess survives the check).  The walk applies the checks of the CLI's serial parser (cli/sam_in.cpp:
// parse_bam_records_serial); a record that fails them raises a status bit and the caller's host reader takes over, which
// also words the error.
#include <algorithm>

#include "bam_numbers.hpp"
#include "scan_kernel.h"
#include "tag_merge.hpp"

namespace mk {

constexpr uint32_t kBamNone = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t bam_ld32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
__device__ __forceinline__ uint32_t bam_ld16(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8; }
__device__ __forceinline__ void bam_st32(uint8_t *p, uint32_t v) { __builtin_memcpy(p, &v, 4); }
__device__ __forceinline__ void bam_st64(uint8_t *p, unsigned long long v) { __builtin_memcpy(p, &v, 8); }

// 4 + block_size if the bytes at p look like a record that lies inside text[0, n); 0: they do not; -1: they might, but the
// text ends first
__device__ __forceinline__ long long bam_plausible(const uint8_t *__restrict__ text, uint64_t n, uint64_t p) {
    if (n - p < 36) return -1;
    const uint8_t *r = text + p;
    const int32_t block = (int32_t)bam_ld32(r), ref = (int32_t)bam_ld32(r + 4), pos = (int32_t)bam_ld32(r + 8), l_seq = (int32_t)bam_ld32(r + 20),
                  nref = (int32_t)bam_ld32(r + 24), npos = (int32_t)bam_ld32(r + 28);
    if (block < 32 || block > (1 << 28) || ref < -1 || ref > (1 << 24) || pos < -1 || l_seq < 0 || nref < -1 || nref > (1 << 24) || npos < -1) return 0;
    const uint32_t l_name = r[12], n_cig = bam_ld16(r + 16);
    const uint64_t fixed = 32ull + l_name + 4ull * n_cig + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq;
    if (l_name == 0 || fixed > (uint64_t)block) return 0;
    if (n - p - 4 < (uint64_t)block) return -1;
    if (r[36 + l_name - 1] != 0) return 0;
    for (uint32_t k = 0; k + 1 < l_name; ++k)
        if (r[36 + k] < 33 || r[36 + k] > 126) return 0;
    return 4 + (long long)block;
}

// start[p] (p >= 1) = the first position in [p * piece, min((p + 1) * piece, n)) from which four plausible records follow each
// other (or fewer, if the chain reaches the end of the text), kBamNone if there is none; start[0] = 0.  One wave per piece.
__global__ __launch_bounds__(64) void mk_bam_find_kernel(const uint8_t *__restrict__ text, uint64_t n, uint32_t piece, uint32_t n_pieces,
                                                        uint32_t *__restrict__ start) {
    const uint32_t p = blockIdx.x;
    if (p >= n_pieces) return;
    if (p == 0) {
        if (threadIdx.x == 0) start[0] = 0;
        return;
    }
    const uint64_t b = (uint64_t)p * piece, e = min(b + piece, n);
    uint32_t found = kBamNone;
    for (uint64_t base = b; base < e; base += 64) {
        uint64_t q = base + threadIdx.x;
        bool ok = q < e;
        if (ok) {
            int k = 0;
            for (; k < 4; ++k) {
                const long long sz = bam_plausible(text, n, q);
                if (sz == 0) {
                    ok = false;
                    break;
                }
                if (sz < 0) {  // the text ends inside this record: nothing more can be checked
                    ok = k > 0;
                    break;
                }
                q += (uint64_t)sz;
                if (q == n) break;
            }
        }
        const unsigned long long mask = __ballot(ok);
        if (mask) {
            found = (uint32_t)(base + (uint64_t)__ffsll((long long)mask) - 1);
            break;
        }
    }
    if (threadIdx.x == 0) start[p] = found;
}

// One lane per piece: from start[p] along the chain to the first record start at or behind the next piece's first byte (the
// end of the whole records for the last piece) -> land[p], records passed -> count[p].  EMIT: the records' table entries at
// base[p] + k; checks as parse_bam_records_serial (st[0] |= 1: not a record), st[1] / st[2] = smallest / largest l_seq.
template <bool EMIT>
__global__ __launch_bounds__(64) void mk_bam_walk_kernel(const uint8_t *__restrict__ text, uint64_t n, uint32_t piece, uint32_t n_pieces,
                                                        const uint32_t *__restrict__ start, uint32_t *__restrict__ land, uint32_t *__restrict__ count,
                                                        const uint32_t *__restrict__ base, uint32_t *__restrict__ rec_off, uint32_t *__restrict__ rec_len,
                                                        uint32_t *__restrict__ seq_start, uint32_t *__restrict__ seq_len, uint32_t *__restrict__ st) {
    const uint32_t p = blockIdx.x * 64 + threadIdx.x;
    uint32_t mn = 0xFFFFFFFFu, mx = 0, bad = 0;
    if (p < n_pieces) {
        uint64_t pos = start[p];
        const uint64_t stop = p + 1 < n_pieces ? (uint64_t)(p + 1) * piece : n;
        uint32_t cnt = 0, unfinished = 0;
        const uint32_t k0 = EMIT ? base[p] : 0;
        if (pos != kBamNone) {
            while (pos < stop) {
                if (n - pos < 4) {  // an unfinished record: the window's tail
                    unfinished = pos < n;
                    break;
                }
                const uint8_t *r = text + pos;
                const int32_t block = (int32_t)bam_ld32(r);
                if (block < 32) {
                    bad = 1;
                    break;
                }
                if (n - pos - 4 < (uint64_t)block) {
                    unfinished = 1;
                    break;
                }
                const uint32_t l_name = r[12], n_cig = bam_ld16(r + 16);
                const int32_t l_seq = (int32_t)bam_ld32(r + 20);
                const uint64_t fixed = 32ull + l_name + 4ull * n_cig;
                if (l_seq < 0 || fixed + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq > (uint64_t)block) {
                    bad = 1;
                    break;
                }
                if (EMIT) {
                    rec_off[k0 + cnt] = (uint32_t)pos;
                    rec_len[k0 + cnt] = (uint32_t)block + 4;
                    seq_start[k0 + cnt] = (uint32_t)(pos + 4 + fixed);
                    seq_len[k0 + cnt] = (uint32_t)l_seq;
                    mn = min(mn, (uint32_t)l_seq), mx = max(mx, (uint32_t)l_seq);
                }
                ++cnt;
                pos += 4 + (uint64_t)block;
            }
        }
        if (!EMIT) {
            land[p] = (uint32_t)pos;
            count[p] = cnt | unfinished << 31;  // (bit 31: the walk ended at a record the text does not hold to its end)
        }
    }
    if (EMIT) {
        for (int o = 32; o > 0; o >>= 1) {
            mn = min(mn, (uint32_t)__shfl_down(mn, o));
            mx = max(mx, (uint32_t)__shfl_down(mx, o));
        }
        if (__ballot(bad != 0) && threadIdx.x == 0) atomicOr(&st[0], 1u);
        if (threadIdx.x == 0) {
            atomicMin(&st[1], mn);
            atomicMax(&st[2], mx);
        }
    }
}

// record i's packed sequence (two bases per byte, high nibble first, "=ACMGRSVTWYHKDBN") -> the ASCII the matcher sees
// (record.sequence().to_vec(), src/cmd_tag.rs:395) at seq[fixed_len ? i * fixed_len : off[i]]; 16 lanes per record, four packed
// bytes = eight bases per lane and step
__global__ __launch_bounds__(256) void mk_bam_unpack_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ seq_start,
                                                           const uint32_t *__restrict__ seq_len, const unsigned long long *__restrict__ off, uint32_t fixed_len,
                                                           uint64_t n_rec, uint8_t *__restrict__ seq) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    if (i >= n_rec) return;
    const uint32_t len = seq_len[i];
    const uint8_t *__restrict__ src = text + seq_start[i];
    uint8_t *__restrict__ dst = seq + (fixed_len ? i * (uint64_t)fixed_len : off[i]);
    const unsigned long long tab_lo = 0x565352474D43413Dull;  // bytes 0..7  = '=' 'A' 'C' 'M' 'G' 'R' 'S' 'V'
    const unsigned long long tab_hi = 0x4E42444B48595754ull;  // bytes 8..15 = 'T' 'W' 'Y' 'H' 'K' 'D' 'B' 'N'
    for (uint32_t b0 = 8 * sub; b0 < len; b0 += 128) {  // bases [b0, b0 + 8) = packed bytes [b0 / 2, b0 / 2 + 4)
        const uint32_t w = bam_ld32(src + (b0 >> 1));   // (may read up to three bytes of the qualities behind the sequence)
        unsigned long long out = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t byte = (w >> (8 * (k >> 1))) & 0xFFu;
            const uint32_t nib = (k & 1) ? (byte & 15u) : (byte >> 4);
            const unsigned long long c = ((nib < 8 ? tab_lo : tab_hi) >> (8 * (nib & 7))) & 0xFFull;
            out |= c << (8 * k);
        }
        if (b0 + 8 <= len) {
            bam_st64(dst + b0, out);
        } else {
            for (uint32_t k = 0; b0 + k < len; ++k) dst[b0 + k] = (uint8_t)(out >> (8 * k));
        }
    }
}

// ---- the keep rule and the value of the tag (plain or merged with an existing one): tag_merge.hpp (shared with sam.hip)

// Per record: keep or drop (src/cmd_tag.rs:457-467), and for a kept one the size of the record it leaves as --
// 4 + block_size + tag (2) + 'Z' + value + NUL, the value being its distinct matched patterns joined by ',' (:484-490; ascending
// pattern index = sort_unstable order of the sorted unique pattern list), merged with the record's existing Z value of that name if
// it has one (:470-485).  A kept record's optional fields are walked for that: fields that do not parse, a field of that name that is
// not a string (the reference refuses it), or a value that is not plain ASCII or very long set a status bit -- the caller's host
// path then does this window, where those rules live.
__global__ __launch_bounds__(256) void mk_bam_taglen_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ rec_off,
                                                           const uint32_t *__restrict__ rec_len, const uint32_t *__restrict__ seq_start,
                                                           const uint32_t *__restrict__ seq_len, const unsigned long long *__restrict__ found_off,
                                                           const uint32_t *__restrict__ found_pat, const uint32_t *__restrict__ pat_off, uint64_t n_rec,
                                                           const uint8_t *__restrict__ pat_bytes, uint32_t filter_matching, uint32_t invert, uint32_t tag0,
                                                           uint32_t tag1, uint8_t *__restrict__ keep, uint32_t *__restrict__ out_len,
                                                           uint32_t *__restrict__ ex_off, uint32_t *__restrict__ st) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bad = 0;
    if (i < n_rec) {
        const unsigned long long f0 = found_off[i], f1 = found_off[i + 1];
        const bool kept = tag_keeps(filter_matching, invert, f1 > f0);
        uint32_t len = 0, ex_at = 0, ex_n = 0;
        if (kept) {
            const uint32_t l = seq_len[i];
            uint64_t p = (uint64_t)seq_start[i] + (l + 1) / 2 + l;
            const uint64_t e = (uint64_t)rec_off[i] + rec_len[i];
            while (p < e) {
                if (e - p < 3) {
                    bad |= 2;
                    break;
                }
                const uint32_t t0 = text[p], t1 = text[p + 1], type = text[p + 2];
                const bool mine = t0 == tag0 && t1 == tag1 && ex_at == 0 && !(bad & 4);  // (record.tags().get(): the first field of that name)
                if (mine && type != 'Z') bad |= 4;  // the reference refuses it: the host path words that
                p += 3;
                if (type == 'A' || type == 'c' || type == 'C') {
                    p += 1;
                } else if (type == 's' || type == 'S') {
                    p += 2;
                } else if (type == 'i' || type == 'I' || type == 'f') {
                    p += 4;
                } else if (type == 'Z' || type == 'H') {
                    const uint64_t v0 = p;
                    uint32_t high = 0;
                    while (p < e && text[p]) high |= text[p], ++p;
                    if (mine && type == 'Z') {
                        // (not plain ASCII: the reference checks UTF-8 first -- the host path's business; so is a very long value)
                        if ((high & 0x80u) || p - v0 > kBamMergeBytes) bad |= 4;
                        else ex_at = (uint32_t)v0, ex_n = (uint32_t)(p - v0);
                    }
                    ++p;
                } else if (type == 'B') {
                    if (e - p < 5) {
                        bad |= 2;
                        break;
                    }
                    const uint32_t sub = text[p];
                    const int32_t cnt = (int32_t)bam_ld32(text + p + 1);
                    const uint64_t w = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
                    if (cnt < 0) {
                        bad |= 2;
                        break;
                    }
                    p += 5 + w * (uint64_t)cnt;
                } else {
                    bad |= 2;
                    break;
                }
            }
            if (p > e) bad |= 2;
            if (ex_n == 0) ex_at = 0;  // no tag of that name, or an empty value ("do nothing if tag is empty", :472-473)
            const uint32_t vlen = (ex_n && bad) ? 0u : tag_value_len(text + ex_at, ex_n, f0, f1, found_pat, pat_off, pat_bytes);
            len = rec_len[i] + 3 + vlen + 1;
        }
        keep[i] = kept ? 1 : 0;
        out_len[i] = len;
        ex_off[i] = ex_at;
    }
    if (__ballot(bad != 0)) {
        uint32_t all = bad;
        for (int o = 32; o > 0; o >>= 1) all |= (uint32_t)__shfl_down(all, o);
        if ((threadIdx.x & 63) == 0) atomicOr(&st[0], all);
    }
}

// the kept records with their tag appended, back to back at out + out_off[i] (record.tags_mut().push_string, src/cmd_tag.rs:488-490;
// the bytes BamWriter::append_tagged_raw of the CLI's host path produces); 16 lanes per record copy four bytes each and step
__global__ __launch_bounds__(256) void mk_bam_emit_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ rec_off,
                                                         const uint32_t *__restrict__ rec_len, const uint32_t *__restrict__ out_len,
                                                         const unsigned long long *__restrict__ out_off, const unsigned long long *__restrict__ found_off,
                                                         const uint32_t *__restrict__ found_pat, const uint8_t *__restrict__ pat_bytes,
                                                         const uint32_t *__restrict__ pat_off, const uint32_t *__restrict__ ex_off, uint64_t n_rec,
                                                         uint32_t tag0, uint32_t tag1, uint8_t *__restrict__ out) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    if (i >= n_rec) return;
    const uint32_t olen = out_len[i];
    if (!olen) return;
    const uint8_t *__restrict__ src = text + rec_off[i];
    uint8_t *__restrict__ dst = out + out_off[i];
    const uint32_t L = rec_len[i];
    uint32_t k = 4 + 4 * sub;
    for (; k + 4 <= L; k += 64) bam_st32(dst + k, bam_ld32(src + k));
    // (the last lane's step may leave up to three bytes: whoever's k is the first not to fit copies them)
    if (k < L && k + 4 > L)
        for (uint32_t j = k; j < L; ++j) dst[j] = src[j];
    if (sub == 0) {
        bam_st32(dst, olen - 4);
        uint8_t *t = dst + L;
        t[0] = (uint8_t)tag0, t[1] = (uint8_t)tag1, t[2] = 'Z';
        t += 3;
        const unsigned long long f0 = found_off[i], f1 = found_off[i + 1];
        const uint32_t ex_at = ex_off[i];  // (0: no existing value; else it ends at its NUL)
        uint32_t ex_n = 0;
        if (ex_at)
            while (text[ex_at + ex_n]) ++ex_n;
        *tag_value_put(t, text + ex_at, ex_n, f0, f1, found_pat, pat_off, pat_bytes) = 0;
    }
}

// ---- BAM record -> SAM line (mk_tag_bam_sam_window; the mirror of sam.hip's SAM -> BAM half): the bytes SamFile::append_line
// (cli/bam_text.cpp: bam_record_to_sam + aux_to_text) writes for the record, then TAB tag ":Z:" value "\n".  One walk, bam_sam_line<kWrite>,
// sizes a line (mk_bam_sam_len_kernel) and writes everything of it that is not SEQ / QUAL (mk_bam_sam_fields_kernel): the same code
// advances the same position in both, so the sizes of the first are the bytes of the second.  The walk is serial and short -- a few
// dozen bytes per record -- so it is one lane per record; SEQ and QUAL, three quarters of a line, are 16 lanes per record
// (mk_bam_sam_seq_kernel).  Numbers: bam_numbers.hpp.
struct BamRefs {  // the reference names of the BAM header: name i = bytes[off[i], off[i + 1])
    const uint8_t *bytes;
    const uint32_t *off;
    uint32_t n;
};

template <bool kWrite>
__device__ __forceinline__ void bam_sam_ref(BamText<kWrite> &t, const BamRefs &F, int32_t id) {
    if (id < 0 || (uint32_t)id >= F.n) {
        t.put('*');
        return;
    }
    const uint32_t a = F.off[id], b = F.off[id + 1];
    if (kWrite)
        for (uint32_t k = a; k < b; ++k) t.out[t.at + (k - a)] = F.bytes[k];
    t.at += b - a;
}

// one item of an integer type at p (type one of c C s S i I); the caller has checked that its bytes are there
template <bool kWrite>
__device__ __forceinline__ void bam_sam_item(BamText<kWrite> &t, const uint8_t *p, uint32_t type) {
    long long v;
    if (type == 'c') v = (int8_t)p[0];
    else if (type == 'C') v = p[0];
    else if (type == 's') v = (int16_t)bam_ld16(p);
    else if (type == 'S') v = bam_ld16(p);
    else if (type == 'i') v = (int32_t)bam_ld32(p);
    else v = bam_ld32(p);
    bam_put_int(t, v);
}

// The record at text + r0 (its block_size field; rlen = 4 + block_size, sizes checked by the record index) as a SAM line without its
// tag and line end, at t; SEQ and QUAL are left out -- *seq_at = where SEQ starts, QUAL one tab behind it -- except where they are "*".
// Returns the refusal bits: 2 = optional fields that do not parse (the host path words that), an `f` outside bam_numbers.hpp's rule,
// or POS / PNEXT = INT32_MAX (the host adds 1 in 32 bits, which is undefined: not imitated, the window is refused).
template <bool kWrite>
__device__ __forceinline__ uint32_t bam_sam_line(BamText<kWrite> &t, const uint8_t *__restrict__ text, uint64_t r0, uint32_t rlen, const BamRefs &F, uint32_t *seq_at) {
    const uint8_t *r = text + r0 + 4;
    const int32_t ref = (int32_t)bam_ld32(r), pos = (int32_t)bam_ld32(r + 4), l_seq = (int32_t)bam_ld32(r + 16), nref = (int32_t)bam_ld32(r + 20),
                  npos = (int32_t)bam_ld32(r + 24), tlen = (int32_t)bam_ld32(r + 28);
    const uint32_t l_name = r[8], mapq = r[9], n_cig = bam_ld16(r + 12), flag = bam_ld16(r + 14);
    uint32_t bad = (pos == 0x7FFFFFFF || npos == 0x7FFFFFFF) ? 2u : 0u;
    for (uint32_t k = 0; k + 1 < l_name; ++k) t.put(r[32 + k]);
    t.put('\t');
    bam_put_int(t, (long long)flag);
    t.put('\t');
    bam_sam_ref(t, F, ref);
    t.put('\t');
    bam_put_int(t, (long long)pos + 1);
    t.put('\t');
    bam_put_int(t, (long long)mapq);
    t.put('\t');
    const uint8_t *cg = r + 32 + l_name;
    if (n_cig == 0) t.put('*');
    for (uint32_t k = 0; k < n_cig; ++k) {
        const uint32_t v = bam_ld32(cg + 4 * k), op = v & 15u;
        bam_put_int(t, (long long)(v >> 4));
        // "MIDNSHP=" as the bytes of one constant, indexed by a shift; 'X', and '?' for a code the specification does not have
        t.put(op < 8 ? (uint32_t)(0x3D5048534E44494Dull >> (8 * op)) & 0xFFu : op == 8 ? 'X' : '?');
    }
    t.put('\t');
    if (nref < 0) t.put('*');
    else if (nref == ref) t.put('=');
    else bam_sam_ref(t, F, nref);
    t.put('\t');
    bam_put_int(t, (long long)npos + 1);
    t.put('\t');
    bam_put_int(t, (long long)tlen);
    t.put('\t');
    const uint8_t *sq = cg + 4 * (uint64_t)n_cig, *ql = sq + ((uint32_t)l_seq + 1) / 2;
    *seq_at = (uint32_t)t.at;
    if (l_seq == 0) t.put('*');
    else t.at += (uint32_t)l_seq;
    t.put('\t');
    if (l_seq == 0 || ql[0] == 0xFF) t.put('*');
    else t.at += (uint32_t)l_seq;
    // ---- the optional fields (aux_to_text)
    const uint8_t *p = ql + (uint32_t)l_seq, *e = text + r0 + rlen;
    while (p < e) {
        if (e - p < 3) return bad | 2;
        const uint32_t type = p[2];
        t.put('\t'), t.put(p[0]), t.put(p[1]), t.put(':');
        p += 3;
        if (type == 'A') {
            if (e - p < 1) return bad | 2;
            t.put('A'), t.put(':'), t.put(p[0]);
            p += 1;
        } else if (type == 'c' || type == 'C' || type == 's' || type == 'S' || type == 'i' || type == 'I') {
            const uint32_t w = (type == 'c' || type == 'C') ? 1 : (type == 's' || type == 'S') ? 2 : 4;
            if (e - p < w) return bad | 2;
            t.put('i'), t.put(':');
            bam_sam_item(t, p, type);
            p += w;
        } else if (type == 'f') {
            if (e - p < 4) return bad | 2;
            t.put('f'), t.put(':');
            if (!bam_put_float(t, bam_ld32(p))) bad |= 2;
            p += 4;
        } else if (type == 'Z' || type == 'H') {
            t.put(type), t.put(':');
            while (p < e && *p) t.put(*p++);
            if (p == e) return bad | 2;  // (no NUL: today's rule of mk_bam_taglen_kernel)
            ++p;
        } else if (type == 'B') {
            if (e - p < 5) return bad | 2;
            const uint32_t sub = p[0];
            const int32_t cnt = (int32_t)bam_ld32(p + 1);
            p += 5;
            const bool is_int = sub == 'c' || sub == 'C' || sub == 's' || sub == 'S' || sub == 'i' || sub == 'I';
            const uint32_t w = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            if (cnt < 0 || (cnt > 0 && !is_int && sub != 'f') || (uint64_t)(e - p) < (uint64_t)w * (uint32_t)cnt) return bad | 2;
            t.put('B'), t.put(':'), t.put(sub);
            for (int32_t k = 0; k < cnt; ++k, p += w) {
                t.put(',');
                if (is_int) bam_sam_item(t, p, sub);
                else if (!bam_put_float(t, bam_ld32(p))) bad |= 2;
            }
        } else {
            return bad | 2;
        }
    }
    return bad;
}

// Runs behind mk_bam_taglen_kernel (keep, ex_off, out_len = the record as BAM with its tag, refusal bits): a kept record's out_len
// becomes the length of its line with the tag -- the value's length is taken from the BAM length -- and seq_at where its SEQ goes
__global__ __launch_bounds__(256) void mk_bam_sam_len_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ rec_off,
                                                            const uint32_t *__restrict__ rec_len, const uint8_t *__restrict__ keep, uint64_t n_rec, BamRefs F,
                                                            uint32_t *__restrict__ out_len, uint32_t *__restrict__ seq_at, uint32_t *__restrict__ st) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bad = 0;
    if (i < n_rec && keep[i]) {
        BamText<false> t{nullptr, 0};
        uint32_t sa = 0;
        const uint32_t L = rec_len[i];
        bad = bam_sam_line<false>(t, text, rec_off[i], L, F, &sa);
        const uint64_t vlen = out_len[i] - L - 4;  // (out_len = L + tag (2) + 'Z' + value + NUL)
        const uint64_t len = t.at + 6 + vlen + 1;  // TAB tag ":Z:" value "\n"
        if (len > 0xFFFFFFFFull) bad |= 2;
        out_len[i] = (uint32_t)len;
        seq_at[i] = sa;
    }
    if (__ballot(bad != 0)) {
        uint32_t all = bad;
        for (int o = 32; o > 0; o >>= 1) all |= (uint32_t)__shfl_down(all, o);
        if ((threadIdx.x & 63) == 0) atomicOr(&st[0], all);
    }
}

// everything of a kept record's line that is not SEQ / QUAL, at out + out_off[i]; one lane per record
__global__ __launch_bounds__(256) void mk_bam_sam_fields_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ rec_off,
                                                               const uint32_t *__restrict__ rec_len, const uint32_t *__restrict__ out_len,
                                                               const unsigned long long *__restrict__ out_off, const unsigned long long *__restrict__ found_off,
                                                               const uint32_t *__restrict__ found_pat, const uint8_t *__restrict__ pat_bytes,
                                                               const uint32_t *__restrict__ pat_off, const uint32_t *__restrict__ ex_off, BamRefs F, uint64_t n_rec,
                                                               uint32_t tag0, uint32_t tag1, uint8_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec || !out_len[i]) return;
    BamText<true> t{out + out_off[i], 0};
    uint32_t sa;
    bam_sam_line<true>(t, text, rec_off[i], rec_len[i], F, &sa);
    t.put('\t'), t.put(tag0), t.put(tag1), t.put(':'), t.put('Z'), t.put(':');
    const uint32_t ex_at = ex_off[i];  // (0: no existing value; else it ends at its NUL)
    uint32_t ex_n = 0;
    if (ex_at)
        while (text[ex_at + ex_n]) ++ex_n;
    *tag_value_put(t.out + t.at, text + ex_at, ex_n, found_off[i], found_off[i + 1], found_pat, pat_off, pat_bytes) = '\n';
}

// SEQ and QUAL of the kept records; 16 lanes per record, per lane and step eight packed bytes -> 16 letters and 16 quality bytes + 33
// (per byte, as the host's (char)(q + 33): the low seven bits are added, the top bit is put back, so no carry crosses a byte)
__global__ __launch_bounds__(256) void mk_bam_sam_seq_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ seq_start,
                                                            const uint32_t *__restrict__ seq_len, const uint32_t *__restrict__ out_len,
                                                            const unsigned long long *__restrict__ out_off, const uint32_t *__restrict__ seq_at, uint64_t n_rec,
                                                            uint8_t *__restrict__ out) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    if (i >= n_rec || !out_len[i]) return;
    const uint32_t len = seq_len[i];
    if (!len) return;
    const uint8_t *__restrict__ src = text + seq_start[i];
    const uint8_t *__restrict__ ql = src + (len + 1) / 2;
    uint8_t *__restrict__ dst = out + out_off[i] + seq_at[i];
    uint8_t *__restrict__ qdst = dst + len + 1;
    const bool has_q = ql[0] != 0xFF;
    const unsigned long long tab_lo = 0x565352474D43413Dull;  // bytes 0..7  = '=' 'A' 'C' 'M' 'G' 'R' 'S' 'V'
    const unsigned long long tab_hi = 0x4E42444B48595754ull;  // bytes 8..15 = 'T' 'W' 'Y' 'H' 'K' 'D' 'B' 'N'
    for (uint32_t b0 = 16 * sub; b0 < len; b0 += 256) {  // bases [b0, b0 + 16) = packed bytes [b0 / 2, b0 / 2 + 8)
        if (b0 + 16 <= len) {
            unsigned long long w, v[2] = {0, 0};
            __builtin_memcpy(&w, src + (b0 >> 1), 8);
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t byte = (uint32_t)(w >> (8 * (k >> 1))) & 0xFFu;
                const uint32_t nib = (k & 1) ? (byte & 15u) : (byte >> 4);
                const unsigned long long c = ((nib < 8 ? tab_lo : tab_hi) >> (8 * (nib & 7))) & 0xFFull;
                v[k >> 3] |= c << (8 * (k & 7));
            }
            __builtin_memcpy(dst + b0, v, 16);
            if (has_q) {
                unsigned long long q[2];
                __builtin_memcpy(q, ql + b0, 16);
#pragma unroll
                for (int k = 0; k < 2; ++k) q[k] = ((q[k] & 0x7F7F7F7F7F7F7F7Full) + 0x2121212121212121ull) ^ (q[k] & 0x8080808080808080ull);
                __builtin_memcpy(qdst + b0, q, 16);
            }
        } else {  // (the last, shorter step of the record)
            for (uint32_t b = b0; b < len; ++b) {
                const uint32_t nib = (src[b >> 1] >> ((~b & 1u) << 2)) & 15u;
                dst[b] = (uint8_t)(((nib < 8 ? tab_lo : tab_hi) >> (8 * (nib & 7))) & 0xFFull);
                if (has_q) qdst[b] = (uint8_t)(ql[b] + 33u);
            }
        }
    }
}

// names (NUL included) of the records with a hit, for the log rows: name_len[i] = flags[i] ? l_read_name : 0 and where the name starts
__global__ __launch_bounds__(256) void mk_bam_names_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ rec_off,
                                                          const uint8_t *__restrict__ flags, uint64_t n_rec, uint32_t *__restrict__ name_start,
                                                          uint32_t *__restrict__ name_len) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec) return;
    name_start[i] = rec_off[i] + 36;
    name_len[i] = flags[i] ? (uint32_t)text[rec_off[i] + 12] : 0u;
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
void launch_bam_find(const uint8_t *d_text, uint64_t n, uint32_t piece, uint32_t n_pieces, uint32_t *d_start, hipStream_t st) {
    hipLaunchKernelGGL(mk_bam_find_kernel, dim3(n_pieces), dim3(64), 0, st, d_text, n, piece, n_pieces, d_start);
}
void launch_bam_walk_count(const uint8_t *d_text, uint64_t n, uint32_t piece, uint32_t n_pieces, const uint32_t *d_start, uint32_t *d_land,
                           uint32_t *d_count, hipStream_t st) {
    hipLaunchKernelGGL(mk_bam_walk_kernel<false>, dim3((n_pieces + 63) / 64), dim3(64), 0, st, d_text, n, piece, n_pieces, d_start, d_land, d_count,
                       (const uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr);
}
void launch_bam_walk_emit(const uint8_t *d_text, uint64_t n, uint32_t piece, uint32_t n_pieces, const uint32_t *d_start, const uint32_t *d_base,
                          uint32_t *d_rec_off, uint32_t *d_rec_len, uint32_t *d_seq_start, uint32_t *d_seq_len, uint32_t *d_st, hipStream_t st) {
    hipLaunchKernelGGL(mk_bam_walk_kernel<true>, dim3((n_pieces + 63) / 64), dim3(64), 0, st, d_text, n, piece, n_pieces, d_start, (uint32_t *)nullptr,
                       (uint32_t *)nullptr, d_base, d_rec_off, d_rec_len, d_seq_start, d_seq_len, d_st);
}
void launch_bam_unpack(const uint8_t *d_text, const uint32_t *d_seq_start, const uint32_t *d_seq_len, const unsigned long long *d_off, uint32_t fixed_len,
                       uint64_t n_rec, uint8_t *d_seq, hipStream_t st) {
    if (!n_rec) return;
    hipLaunchKernelGGL(mk_bam_unpack_kernel, dim3((unsigned)((n_rec * 16 + 255) / 256)), dim3(256), 0, st, d_text, d_seq_start, d_seq_len, d_off, fixed_len,
                       n_rec, d_seq);
}
void launch_bam_taglen(const uint8_t *d_text, const uint32_t *d_rec_off, const uint32_t *d_rec_len, const uint32_t *d_seq_start, const uint32_t *d_seq_len,
                       const unsigned long long *d_found_off, const uint32_t *d_found_pat, const uint32_t *d_pat_off, const uint8_t *d_pat_bytes, uint64_t n_rec,
                       uint32_t filter_matching, uint32_t invert, uint32_t tag0, uint32_t tag1, uint8_t *d_keep, uint32_t *d_out_len, uint32_t *d_ex_off,
                       uint32_t *d_st, hipStream_t st) {
    if (!n_rec) return;
    hipLaunchKernelGGL(mk_bam_taglen_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, d_text, d_rec_off, d_rec_len, d_seq_start, d_seq_len,
                       d_found_off, d_found_pat, d_pat_off, n_rec, d_pat_bytes, filter_matching, invert, tag0, tag1, d_keep, d_out_len, d_ex_off, d_st);
}
void launch_bam_emit(const uint8_t *d_text, const uint32_t *d_rec_off, const uint32_t *d_rec_len, const uint32_t *d_out_len, const unsigned long long *d_out_off,
                     const unsigned long long *d_found_off, const uint32_t *d_found_pat, const uint8_t *d_pat_bytes, const uint32_t *d_pat_off,
                     const uint32_t *d_ex_off, uint64_t n_rec, uint32_t tag0, uint32_t tag1, uint8_t *d_out, hipStream_t st) {
    if (!n_rec) return;
    hipLaunchKernelGGL(mk_bam_emit_kernel, dim3((unsigned)((n_rec * 16 + 255) / 256)), dim3(256), 0, st, d_text, d_rec_off, d_rec_len, d_out_len, d_out_off,
                       d_found_off, d_found_pat, d_pat_bytes, d_pat_off, d_ex_off, n_rec, tag0, tag1, d_out);
}
void launch_bam_sam_len(const uint8_t *d_text, const uint32_t *d_rec_off, const uint32_t *d_rec_len, const uint8_t *d_keep, uint64_t n_rec,
                        const uint8_t *d_ref_bytes, const uint32_t *d_ref_off, uint32_t n_refs, uint32_t *d_out_len, uint32_t *d_seq_at, uint32_t *d_st, hipStream_t st) {
    if (!n_rec) return;
    hipLaunchKernelGGL(mk_bam_sam_len_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, d_text, d_rec_off, d_rec_len, d_keep, n_rec,
                       BamRefs{d_ref_bytes, d_ref_off, n_refs}, d_out_len, d_seq_at, d_st);
}
void launch_bam_sam_emit(const uint8_t *d_text, const uint32_t *d_rec_off, const uint32_t *d_rec_len, const uint32_t *d_seq_start, const uint32_t *d_seq_len,
                         const uint32_t *d_out_len, const unsigned long long *d_out_off, const uint32_t *d_seq_at, const unsigned long long *d_found_off,
                         const uint32_t *d_found_pat, const uint8_t *d_pat_bytes, const uint32_t *d_pat_off, const uint32_t *d_ex_off, const uint8_t *d_ref_bytes,
                         const uint32_t *d_ref_off, uint32_t n_refs, uint64_t n_rec, uint32_t tag0, uint32_t tag1, uint8_t *d_out, hipStream_t st) {
    if (!n_rec) return;
    hipLaunchKernelGGL(mk_bam_sam_fields_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, d_text, d_rec_off, d_rec_len, d_out_len, d_out_off,
                       d_found_off, d_found_pat, d_pat_bytes, d_pat_off, d_ex_off, BamRefs{d_ref_bytes, d_ref_off, n_refs}, n_rec, tag0, tag1, d_out);
    hipLaunchKernelGGL(mk_bam_sam_seq_kernel, dim3((unsigned)((n_rec * 16 + 255) / 256)), dim3(256), 0, st, d_text, d_seq_start, d_seq_len, d_out_len, d_out_off,
                       d_seq_at, n_rec, d_out);
}
void launch_bam_names(const uint8_t *d_text, const uint32_t *d_rec_off, const uint8_t *d_flags, uint64_t n_rec, uint32_t *d_name_start, uint32_t *d_name_len,
                      hipStream_t st) {
    if (!n_rec) return;
    hipLaunchKernelGGL(mk_bam_names_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, d_text, d_rec_off, d_flags, n_rec, d_name_start,
                       d_name_len);
}

}  // namespace mk
