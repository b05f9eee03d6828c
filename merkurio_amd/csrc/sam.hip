// sam.hip -- a window of SAM text on the device: its lines become a record table, the SEQ fields become the text the matcher scans,
// and the kept lines leave with their `km` field appended -- what the reference's reader thread, record loop and text writer do
// one record at a time (src/cmd_tag.rs:559-612 `for record in reader`, :387-497 process_record) and what the CLI's host path does
// on its threads (cli/sam_in.cpp: parse_sam_text, SamFile::gather, SamFile::find_tag), which is the definition these kernels follow.
//
// The line table is ingest.hip's (one u32 per line start).  The text is then read three times -- fields, SEQ gather, emit -- and
// nothing else is large, so each pass gives a line to 16 lanes that take 16 (gather: 8) consecutive bytes each per step: a line
// of ~350 bytes is two steps of full-width loads, where a lane per line would put neighbouring lanes 350 bytes apart.  Lines and
// fields start anywhere: the loads and stores are unaligned ones.
//   mk_sam_fields_kernel   per line: record or not ('@' and empty lines are not), '\r' stripped, tabs 1, 9, 10 and 11 located from
//                          16-bit tab masks and a prefix sum over the 16 lanes -> QNAME length, SEQ, where the optional fields start
//   mk_sam_compact_kernel  the entries of the record lines moved to the front (only when some line is not a record)
//   mk_sam_gather_kernel   SEQ -> scan buffer, a-z upper-cased (eight bytes at a time)
//   mk_sam_taglen_kernel   keep / drop; of a kept record the first optional field of the tag's name, its value, the output length
//   mk_sam_emit_kernel     line TAB tag ":Z:" value '\n' at its place in the output
//   mk_sam_bam_len_kernel / _fields_kernel / _seq_kernel   SAM -> BAM: the kept lines as BAM records (the second half of this file)
// (the keep rule and the value itself are tag_merge.hpp's, shared with bam.hip; the host side of both is tag_windows.cpp: tag_scan / tag_keep)
// Every access is bounded by the line it belongs to: a load of 16 bytes starts inside the line and may run up to 15 bytes past its
// end, which the text buffer's padding (64 bytes behind the window, window_ingest.cpp: window_assemble) covers.
#include "scan_kernel.h"
#include "sam_numbers.hpp"
#include "tag_merge.hpp"

namespace mk {

constexpr uint32_t kSamNone = 0xFFFFFFFFu;

struct SamBytes16 {
    uint32_t w[4];
};
__device__ __forceinline__ SamBytes16 sam_ld128(const uint8_t *p) {
    SamBytes16 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
__device__ __forceinline__ void sam_st128(uint8_t *p, const SamBytes16 &v) { __builtin_memcpy(p, &v, 16); }

// bit k = byte k of the dword equals the byte replicated in c4 (exact: no borrow between bytes)
__device__ __forceinline__ uint32_t sam_eq4(uint32_t v, uint32_t c4) {
    const uint32_t x = v ^ c4;
    const uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
    const uint32_t m = (~(t | x | 0x7F7F7F7Fu)) >> 7;  // bit 0 / 8 / 16 / 24
    return (m * 0x01020408u) >> 24;                    // (the four bits meet in bits 24..27 without a carry)
}
// bit k = byte k of the 16 bytes is a tab; only bytes in front of `valid` (>= 1) count
__device__ __forceinline__ uint32_t sam_tab_mask(const SamBytes16 &v, uint32_t valid) {
    const uint32_t m = sam_eq4(v.w[0], 0x09090909u) | sam_eq4(v.w[1], 0x09090909u) << 4 | sam_eq4(v.w[2], 0x09090909u) << 8 | sam_eq4(v.w[3], 0x09090909u) << 12;
    return valid >= 16 ? m : m & ((1u << valid) - 1u);
}
__device__ __forceinline__ uint32_t sam_nth_bit(uint32_t mask, uint32_t k) {  // position of the k-th (0-based) set bit; it exists
    for (uint32_t j = 0; j < k; ++j) mask &= mask - 1;
    return (uint32_t)__ffs(mask) - 1u;
}
__device__ __forceinline__ uint32_t sam_min16(uint32_t v) {  // the smallest value of the 16 lanes of a line; every lane gets it
    for (int o = 8; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor(v, o, 16));
    return v;
}

__global__ __launch_bounds__(256) void mk_sam_fields_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ line_start, uint64_t n_lines,
                                                           uint32_t *__restrict__ is_rec, SamTables L, uint32_t *__restrict__ st) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    const bool live = i < n_lines;
    uint32_t s = 0, e = 0;
    if (live) {
        // line i is [s, e) without its '\n' (the entry behind the last line is n + 1: a last line without '\n' ends at n); a '\r'
        // in front of the '\n' belongs to the line end
        s = line_start[i], e = line_start[i + 1] - 1;
        if (e > s && text[e - 1] == '\r') --e;
    }
    const bool rec = live && e > s && text[s] != '@';
    uint32_t bad = 0, len = 0;
    if (rec) {  // (the same for the 16 lanes of a line, and so is the loop's trip count)
        uint32_t tabs = 0, p1 = kSamNone, p9 = kSamNone, p10 = kSamNone, p11 = kSamNone;
        for (uint32_t base = s; base < e && tabs < 11; base += 256) {
            const uint32_t c = base + 16 * sub;
            const uint32_t mask = c < e ? sam_tab_mask(sam_ld128(text + c), e - c) : 0u;
            const uint32_t cnt = __popc(mask);
            uint32_t incl = cnt;
            for (int o = 1; o < 16; o <<= 1) {
                const uint32_t u = __shfl_up(incl, o, 16);
                if ((int)sub >= o) incl += u;
            }
            const uint32_t before = tabs + incl - cnt;  // tabs of the line in front of this lane's bytes
            if (before < 1 && before + cnt >= 1) p1 = c + sam_nth_bit(mask, 0 - before);
            if (before < 9 && before + cnt >= 9) p9 = c + sam_nth_bit(mask, 8 - before);
            if (before < 10 && before + cnt >= 10) p10 = c + sam_nth_bit(mask, 9 - before);
            if (before < 11 && before + cnt >= 11) p11 = c + sam_nth_bit(mask, 10 - before);
            tabs += __shfl(incl, 15, 16);
        }
        p1 = sam_min16(p1), p9 = sam_min16(p9), p10 = sam_min16(p10), p11 = sam_min16(p11);
        if (sub == 0) {
            uint32_t name = 0, q0 = s, aux = e;
            if (tabs < 9) {  // fewer than 10 fields: the host reader words that
                bad = 1;
            } else {
                name = p1 - s;
                q0 = p9 + 1;
                const uint32_t q1 = tabs >= 10 ? p10 : e;
                len = q1 - q0;
                if (len == 1 && text[q0] == '*') len = 0;
                if (tabs >= 11) aux = p11 + 1;  // (else: no optional fields)
            }
            L.rec_start[i] = s, L.rec_len[i] = e - s, L.name_len[i] = name, L.seq_start[i] = q0, L.seq_len[i] = len, L.aux_start[i] = aux;
        }
    }
    if (live && sub == 0) is_rec[i] = rec ? 1u : 0u;
    // per-wave reductions, one atomic each (as mk_ingest_records_kernel)
    const bool counts = rec && sub == 0 && !bad;
    uint32_t mn = counts ? len : 0xFFFFFFFFu, mx = counts ? len : 0u;
    for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, (uint32_t)__shfl_down(mn, o));
        mx = max(mx, (uint32_t)__shfl_down(mx, o));
    }
    if (__ballot(bad != 0) && (threadIdx.x & 63) == 0) atomicOr(&st[0], 1u);
    if ((threadIdx.x & 63) == 0) {
        if (mn < __atomic_load_n(&st[1], __ATOMIC_RELAXED)) atomicMin(&st[1], mn);
        if (mx > __atomic_load_n(&st[2], __ATOMIC_RELAXED)) atomicMax(&st[2], mx);
    }
}

__global__ __launch_bounds__(256) void mk_sam_compact_kernel(const uint32_t *__restrict__ is_rec, const unsigned long long *__restrict__ rec_index, uint64_t n_lines,
                                                            SamTables L, SamTables R) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_lines || !is_rec[i]) return;
    const unsigned long long r = rec_index[i];
    R.rec_start[r] = L.rec_start[i], R.rec_len[r] = L.rec_len[i], R.name_len[r] = L.name_len[i];
    R.seq_start[r] = L.seq_start[i], R.seq_len[r] = L.seq_len[i], R.aux_start[r] = L.aux_start[i];
}

// the eight bytes of v with a-z upper-cased, every other byte as it is (bytes >= 0x80 included)
__device__ __forceinline__ unsigned long long sam_upper8(unsigned long long v) {
    const unsigned long long k7f = 0x7F7F7F7F7F7F7F7Full, k80 = 0x8080808080808080ull;
    const unsigned long long y = v & k7f;
    const unsigned long long ge_a = y + 0x1F1F1F1F1F1F1F1Full;  // bit 7: the low seven bits are >= 'a'
    const unsigned long long gt_z = y + 0x0505050505050505ull;  // bit 7: ... > 'z'
    const unsigned long long lower = ge_a & ~gt_z & ~v & k80;
    return v ^ (lower >> 2);
}

// SEQ of record i -> seq[fixed_len ? i * fixed_len : off[i]] as the matcher sees it (cli/sam_in.cpp: SamFile::gather); 16 lanes per record,
// eight bytes per lane and step
__global__ __launch_bounds__(256) void mk_sam_gather_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ seq_start,
                                                           const uint32_t *__restrict__ seq_len, const unsigned long long *__restrict__ off, uint32_t fixed_len,
                                                           uint64_t n_rec, uint8_t *__restrict__ seq) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    if (i >= n_rec) return;
    const uint32_t len = seq_len[i];
    const uint8_t *__restrict__ src = text + seq_start[i];
    uint8_t *__restrict__ dst = seq + (fixed_len ? i * (uint64_t)fixed_len : off[i]);
    for (uint32_t k = 8 * sub; k < len; k += 128) {
        if (k + 8 <= len) {
            unsigned long long v;
            __builtin_memcpy(&v, src + k, 8);
            v = sam_upper8(v);
            __builtin_memcpy(dst + k, &v, 8);
        } else {
            for (uint32_t j = k; j < len; ++j) {
                const uint8_t b = src[j];
                dst[j] = (b >= 'a' && b <= 'z') ? (uint8_t)(b & ~0x20u) : b;
            }
        }
    }
}

__global__ __launch_bounds__(256) void mk_sam_names_kernel(const uint32_t *__restrict__ name_len, const uint8_t *__restrict__ flags, uint64_t n_rec,
                                                          uint32_t *__restrict__ name_len_out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rec) name_len_out[i] = flags[i] ? name_len[i] + 1u : 0u;
}
__global__ __launch_bounds__(256) void mk_sam_name_ends_kernel(const uint32_t *__restrict__ name_len_out, const unsigned long long *__restrict__ name_off,
                                                              uint64_t n_rec, uint8_t *__restrict__ names) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_rec && name_len_out[i]) names[name_off[i] + name_len_out[i] - 1] = 0;
}

// Per record: keep or drop (src/cmd_tag.rs:457-467), and for a kept one the size of the line it leaves as -- line + TAB + tag + ":Z:"
// + value + '\n', the value being its distinct matched patterns joined by ',' (:484-490), merged with the record's existing value of
// that name if it has one (:470-485).  The optional fields of a kept record (fields 12 ...) are searched for the FIRST field of at
// least five bytes that starts with the tag and ':' (cli/sam_in.cpp: SamFile::find_tag): 16 lanes look at the tabs of 16 bytes each, a
// field starts behind every tab.  A field of that name that is not "Z:" (the reference refuses it) or whose value is not plain ASCII
// or very long sets status bit 4 -- the caller's host path then does this window.  ex_off[i] = where the value starts, 0 = none.
__global__ __launch_bounds__(256) void mk_sam_taglen_kernel(const uint8_t *__restrict__ text, SamTables R, const unsigned long long *__restrict__ found_off,
                                                           const uint32_t *__restrict__ found_pat, const uint32_t *__restrict__ pat_off, uint64_t n_rec,
                                                           const uint8_t *__restrict__ pat_bytes, uint32_t filter_matching, uint32_t invert, uint32_t tag0,
                                                           uint32_t tag1, uint8_t *__restrict__ keep, uint32_t *__restrict__ out_len,
                                                           uint32_t *__restrict__ ex_off, uint32_t *__restrict__ st) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    uint32_t bad = 0;
    if (i < n_rec) {
        const unsigned long long f0 = found_off[i], f1 = found_off[i + 1];
        const bool kept = tag_keeps(filter_matching, invert, f1 > f0);
        uint32_t len = 0, ex_at = 0, ex_n = 0;
        if (kept) {
            const uint32_t a = R.aux_start[i], e = R.rec_start[i] + R.rec_len[i];
            uint32_t first = kSamNone;
            // a field of at least five bytes at p that starts with the tag and ':'
            auto mine = [&](uint32_t p) {
                return e - p >= 5 && text[p] == tag0 && text[p + 1] == tag1 && text[p + 2] == ':' && text[p + 3] != '\t' && text[p + 4] != '\t';
            };
            if (a < e && sub == 0 && mine(a)) first = a;
            for (uint32_t base = a; base < e; base += 256) {
                const uint32_t c = base + 16 * sub;
                uint32_t mask = c < e ? sam_tab_mask(sam_ld128(text + c), e - c) : 0u;
                while (mask) {
                    const uint32_t p = c + (uint32_t)__ffs(mask);  // the byte behind the tab
                    mask &= mask - 1;
                    if (p < first && mine(p)) first = p;
                }
            }
            first = sam_min16(first);
            if (sub == 0) {
                if (first != kSamNone) {
                    if (text[first + 3] != 'Z' || text[first + 4] != ':') {
                        bad = 4;
                    } else {
                        uint32_t p = first + 5, high = 0;
                        while (p < e && text[p] != '\t') high |= text[p], ++p;
                        // (not plain ASCII: the reference checks UTF-8 first -- the host path's business; so is a very long value)
                        if ((high & 0x80u) || p - (first + 5) > kBamMergeBytes) bad = 4;
                        else ex_at = first + 5, ex_n = p - (first + 5);
                    }
                }
                if (ex_n == 0) ex_at = 0;  // no field of that name, or an empty value ("do nothing if tag is empty", :472-473)
                len = R.rec_len[i] + 6 + tag_value_len(text + ex_at, ex_n, f0, f1, found_pat, pat_off, pat_bytes) + 1;
            }
        }
        if (sub == 0) {
            keep[i] = kept ? 1 : 0;
            out_len[i] = len;
            ex_off[i] = ex_at;
        }
    }
    if (__ballot(bad != 0) && (threadIdx.x & 63) == 0) atomicOr(&st[0], 4u);
}

// the kept lines with their tag appended, back to back at out + out_off[i] (what the CLI's host path writes: SamFile::append_line,
// TAB, tag, ":Z:", value, '\n'); 16 lanes per record copy 16 bytes each and step
__global__ __launch_bounds__(256) void mk_sam_emit_kernel(const uint8_t *__restrict__ text, SamTables R, const uint32_t *__restrict__ out_len,
                                                         const unsigned long long *__restrict__ out_off, const unsigned long long *__restrict__ found_off,
                                                         const uint32_t *__restrict__ found_pat, const uint8_t *__restrict__ pat_bytes,
                                                         const uint32_t *__restrict__ pat_off, const uint32_t *__restrict__ ex_off, uint64_t n_rec,
                                                         uint32_t tag0, uint32_t tag1, uint8_t *__restrict__ out) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    if (i >= n_rec) return;
    const uint32_t olen = out_len[i];
    if (!olen) return;
    const uint32_t s = R.rec_start[i], L = R.rec_len[i];
    const uint8_t *__restrict__ src = text + s;
    uint8_t *__restrict__ dst = out + out_off[i];
    uint32_t k = 16 * sub;
    for (; k + 16 <= L; k += 256) sam_st128(dst + k, sam_ld128(src + k));
    // (the last step may leave up to 15 bytes: whoever's k is the first not to fit copies them)
    if (k < L)
        for (uint32_t j = k; j < L; ++j) dst[j] = src[j];
    if (sub == 0) {
        uint8_t *t = dst + L;
        t[0] = '\t', t[1] = (uint8_t)tag0, t[2] = (uint8_t)tag1, t[3] = ':', t[4] = 'Z', t[5] = ':';
        t += 6;
        const unsigned long long f0 = found_off[i], f1 = found_off[i + 1];
        const uint32_t ex_at = ex_off[i];  // (0: no existing value; else it ends at the next tab or with the line)
        uint32_t ex_n = 0;
        if (ex_at)
            while (ex_at + ex_n < s + L && text[ex_at + ex_n] != '\t') ++ex_n;
        *tag_value_put(t, text + ex_at, ex_n, f0, f1, found_pat, pat_off, pat_bytes) = '\n';
    }
}

// ---- SAM line -> BAM record (mk_tag_sam_bam_window): what the CLI's host path does with a kept line -- line TAB tag ":Z:" value handed
// to BamWriter::encode_record (cli/bam_out.cpp), which is the definition: the same bytes, or the window is refused (st[0] |= 1: a kept line
// with fewer than 11 fields; |= 2: a field that does not encode -- include/merkurio_hip.h lists them) and the host path does it.
// Two passes over the kept lines.  SEQ and QUAL, three quarters of a record, go across 16 lanes per line as above: 16 bases become 8
// bytes of nibbles, 16 quality bytes less 33 stay 16 bytes (mk_sam_bam_seq_kernel).  The short fields in front of SEQ, the CIGAR and the
// optional fields are a few dozen bytes whose meaning depends on the bytes before them: a serial walk, so those kernels give a line to
// ONE lane -- 64 walks per wave instead of 4 with 60 lanes idle.  Both passes walk them with the same code (kWrite = false: sizes and
// checks only), so the sizes of the first pass are the bytes of the second.
struct SamRefs {  // the reference dictionary: names back to back, n + 1 offsets, an open-addressing table of index + 1 (0 = free)
    const uint8_t *bytes;
    const uint32_t *off, *table;
    uint32_t table_mask;
};

// 4-bit codes of "=ACMGRSVTWYHKDBN" in either case, 15 for every other byte (the host's NibbleTable), from a table of the 32 letters
__device__ __forceinline__ uint32_t sam_nibble(uint32_t b) {
    // idx = letter & 31:        @ A B  C D  E F G H  I J K  L M N O | P Q R S T U V W X Y  Z
    const unsigned long long lo = 0xFF3FCFFB4FFD2E1Full, hi = 0xFFFFFFAF97F865FFull;
    const uint32_t u = b | 0x20u, idx = b & 31u;
    const uint32_t code = (uint32_t)((idx < 16 ? lo : hi) >> (4 * (idx & 15u))) & 15u;
    return (u >= 'a' && u <= 'z') ? code : (b == '=' ? 0u : 15u);
}
__device__ __forceinline__ uint32_t sam_sub33x4(uint32_t x) {  // every byte of x less 33, mod 256 (no borrow between bytes)
    const uint32_t y = 0x21212121u, h = 0x80808080u;
    return ((x | h) - y) ^ ((x ^ ~y) & h);
}
__device__ __forceinline__ uint32_t sam_next_tab(const uint8_t *__restrict__ text, uint32_t p, uint32_t e) {
    while (p < e && text[p] != '\t') ++p;
    return p;
}
template <class T>
__device__ __forceinline__ void sam_put(uint8_t *&t, T v) {
    __builtin_memcpy(t, &v, sizeof(T));
    t += sizeof(T);
}

// CIGAR [c, ce) -> its ops at t (kWrite); false: not a CIGAR the device takes
template <bool kWrite>
__device__ __forceinline__ bool sam_bam_cigar(const uint8_t *__restrict__ text, uint32_t c, uint32_t ce, uint8_t *t, uint32_t *n_ops, long long *ref_span) {
    uint32_t ops = 0;
    long long span = 0;
    if (!(ce - c == 1 && text[c] == '*')) {
        while (c < ce) {
            uint32_t d = c;
            while (d < ce && (uint32_t)text[d] - '0' <= 9u) ++d;
            uint32_t len = 0, op;
            if (d == ce || !sam_cigar_len(text + c, d - c, &len)) return false;
            switch (text[d]) {
            case 'M': op = 0; break;
            case 'I': op = 1; break;
            case 'D': op = 2; break;
            case 'N': op = 3; break;
            case 'S': op = 4; break;
            case 'H': op = 5; break;
            case 'P': op = 6; break;
            case '=': op = 7; break;
            case 'X': op = 8; break;
            default: return false;
            }
            if (kWrite) sam_put<uint32_t>(t, len << 4 | op);
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) span += len;
            ++ops;
            c = d + 1;
        }
    }
    *n_ops = ops, *ref_span = span;
    return ops <= 65535u;
}

// the optional fields [a, e) (a < e) -> their BAM form at t (kWrite); returns its size, *ok = false: a field the device does not take
template <bool kWrite>
__device__ __forceinline__ uint32_t sam_bam_opts(const uint8_t *__restrict__ text, uint32_t a, uint32_t e, uint8_t *t, bool *ok) {
    uint32_t size = 0;
    for (uint32_t p = a;;) {
        const uint32_t f = sam_next_tab(text, p, e);
        if (f - p < 5 || text[p + 2] != ':' || text[p + 4] != ':') return *ok = false, 0u;
        const uint32_t type = text[p + 3], v = p + 5, vn = f - v;
        if (kWrite) t[0] = text[p], t[1] = text[p + 1], t += 2;
        size += 3;  // (the tag and the type byte)
        long long x;
        float fl;
        if (type == 'A') {
            if (kWrite) *t++ = 'A', *t++ = vn ? text[v] : (uint8_t)0;
            size += 1;
        } else if (type == 'i') {  // the smallest type that holds the value
            if (!sam_int(text + v, vn, &x)) return *ok = false, 0u;
            const uint32_t w = x >= 0 ? (x <= 0xff ? 1u : x <= 0xffff ? 2u : 4u) : (x >= -128 ? 1u : x >= -32768 ? 2u : 4u);
            if (kWrite) {
                *t++ = x >= 0 ? (w == 1 ? 'C' : w == 2 ? 'S' : 'I') : (w == 1 ? 'c' : w == 2 ? 's' : 'i');
                const uint32_t u = (uint32_t)x;  // (the host's casts: the low bytes)
                for (uint32_t k = 0; k < w; ++k) *t++ = (uint8_t)(u >> (8 * k));
            }
            size += w;
        } else if (type == 'f') {
            if (!sam_float(text + v, vn, &fl)) return *ok = false, 0u;
            if (kWrite) *t++ = 'f', sam_put(t, fl);
            size += 4;
        } else if (type == 'Z' || type == 'H') {
            if (kWrite) {
                *t++ = (uint8_t)type;
                for (uint32_t k = 0; k < vn; ++k) *t++ = text[v + k];
                *t++ = 0;
            }
            size += vn + 1;
        } else if (type == 'B') {  // subtype, then ",item" as often as there are items
            if (vn == 0 || (vn > 1 && text[v + 1] != ',')) return *ok = false, 0u;
            const uint32_t sub = text[v];
            const uint32_t w = (sub == 'c' || sub == 'C') ? 1u : (sub == 's' || sub == 'S') ? 2u : (sub == 'i' || sub == 'I' || sub == 'f') ? 4u : 0u;
            if (!w) return *ok = false, 0u;
            uint8_t *cnt_at = nullptr;
            if (kWrite) *t++ = 'B', *t++ = (uint8_t)sub, cnt_at = t, t += 4;
            uint32_t cnt = 0;
            for (uint32_t q = v + 1; q < f;) {  // text[q] == ','
                const uint32_t ie = [&] {
                    uint32_t k = q + 1;
                    while (k < f && text[k] != ',') ++k;
                    return k;
                }();
                if (sub == 'f') {
                    if (!sam_float(text + q + 1, ie - q - 1, &fl)) return *ok = false, 0u;
                    if (kWrite) sam_put(t, fl);
                } else {
                    if (!sam_int(text + q + 1, ie - q - 1, &x)) return *ok = false, 0u;
                    if (kWrite) {
                        const uint32_t u = (uint32_t)x;
                        for (uint32_t k = 0; k < w; ++k) *t++ = (uint8_t)(u >> (8 * k));
                    }
                }
                ++cnt;
                q = ie;
            }
            if (kWrite) __builtin_memcpy(cnt_at, &cnt, 4);
            size += 1 + 4 + cnt * w;
        } else {
            return *ok = false, 0u;
        }
        if (f >= e) break;
        p = f + 1;  // (a tab at the end of the line: one more, empty, field -- refused above)
    }
    return size;
}

// where QUAL lies in a line of at least 11 fields; false: the line has 10
__device__ __forceinline__ bool sam_qual(const uint8_t *__restrict__ text, uint32_t q0, uint32_t l_seq, uint32_t aux, uint32_t e, uint32_t *qs, uint32_t *qe,
                                         bool *empty_field) {
    const uint32_t raw = l_seq ? l_seq : ((q0 < e && text[q0] == '*') ? 1u : 0u);  // SEQ as written: "*" has length 0 in the table
    if (q0 + raw >= e) return false;
    *qs = q0 + raw + 1;
    // aux == e: no twelfth field -- or an empty one behind a tab that ends the line (QUAL holds no tab: a tab at e - 1 is that one)
    *empty_field = aux == e && e > *qs && text[e - 1] == '\t';
    *qe = aux < e ? aux - 1 : (*empty_field ? e - 1 : e);
    return true;
}

__device__ __forceinline__ int sam_reg2bin(long long beg, long long end) {  // SAM specification 5.3, on the host's 64-bit values
    --end;
    if (beg >> 14 == end >> 14) return (int)(4681 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(585 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(73 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(9 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(1 + (beg >> 26));
    return 0;
}

// index of the name [p, p + n) in the dictionary (the first of equal names), -1: "*" or not in it
__device__ __forceinline__ int32_t sam_ref_id(const uint8_t *__restrict__ text, uint32_t p, uint32_t n, const SamRefs &F) {
    if ((n == 1 && text[p] == '*') || !F.table) return -1;
    for (uint32_t slot = sam_name_hash(text + p, n) & F.table_mask;; slot = (slot + 1) & F.table_mask) {
        const uint32_t id1 = F.table[slot];
        if (!id1) return -1;
        const uint32_t a = F.off[id1 - 1], b = F.off[id1];
        if (b - a != n) continue;
        uint32_t k = 0;
        while (k < n && F.bytes[a + k] == text[p + k]) ++k;
        if (k == n) return (int32_t)(id1 - 1);
    }
}

// Pass 1.  In: keep[i], out_len[i] = the length of the kept line as TEXT with its tag (mk_sam_taglen_kernel: line + 6 + value + 1).
// Out, for a kept record: out_len[i] = the size of its BAM record with block_size, n_cig[i] = its CIGAR ops; st[0] |= 1 / 2.
__global__ __launch_bounds__(256) void mk_sam_bam_len_kernel(const uint8_t *__restrict__ text, SamTables R, const uint8_t *__restrict__ keep, uint64_t n_rec,
                                                            uint32_t *__restrict__ out_len, uint32_t *__restrict__ n_cig, uint32_t *__restrict__ st) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t bad = 0;
    if (i < n_rec && keep[i]) {
        const uint32_t s = R.rec_start[i], e = s + R.rec_len[i], name = R.name_len[i], q0 = R.seq_start[i], l_seq = R.seq_len[i], aux = R.aux_start[i];
        const uint32_t vlen = out_len[i] - R.rec_len[i] - 7;
        uint32_t qs, qe, ops = 0, opt = 0;
        bool empty_field;
        if (!sam_qual(text, q0, l_seq, aux, e, &qs, &qe, &empty_field)) {
            bad = 1;
        } else {
            bool ok = !empty_field && name <= 254 && ((qe - qs == 1 && text[qs] == '*') || qe - qs == l_seq);
            // FLAG RNAME POS MAPQ CIGAR RNEXT PNEXT TLEN lie between the first tab and SEQ
            uint32_t b = s + name + 1;
            long long x, span;
            for (int fld = 1; fld <= 8 && ok; ++fld) {
                const uint32_t f = sam_next_tab(text, b, q0 - 1);
                if (fld == 5) ok = sam_bam_cigar<false>(text, b, f, nullptr, &ops, &span);
                else if (fld != 2 && fld != 6) ok = sam_int(text + b, f - b, &x);
                b = f + 1;
            }
            if (ok && aux < e) opt = sam_bam_opts<false>(text, aux, e, nullptr, &ok);
            if (!ok) bad = 2;
        }
        out_len[i] = 36 + name + 1 + 4 * ops + (l_seq + 1) / 2 + l_seq + opt + 3 + vlen + 1;
        n_cig[i] = ops;
    }
    const unsigned long long any1 = __ballot(bad == 1), any2 = __ballot(bad == 2);
    if ((any1 || any2) && (threadIdx.x & 63) == 0) atomicOr(&st[0], (any1 ? 1u : 0u) | (any2 ? 2u : 0u));
}

// Pass 2, the walked part: block_size, the fixed fields, the CIGAR, the optional fields and the tag at out + out_off[i], one lane per
// record (no window gets here with a bit of pass 1 set)
__global__ __launch_bounds__(256) void mk_sam_bam_fields_kernel(const uint8_t *__restrict__ text, SamTables R, const uint8_t *__restrict__ keep,
                                                               const uint32_t *__restrict__ out_len, const unsigned long long *__restrict__ out_off,
                                                               const uint32_t *__restrict__ n_cig, const unsigned long long *__restrict__ found_off,
                                                               const uint32_t *__restrict__ found_pat, const uint8_t *__restrict__ pat_bytes,
                                                               const uint32_t *__restrict__ pat_off, const uint32_t *__restrict__ ex_off, SamRefs F, uint64_t n_rec,
                                                               uint32_t tag0, uint32_t tag1, uint8_t *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_rec || !keep[i]) return;
    const uint32_t s = R.rec_start[i], e = s + R.rec_len[i], name = R.name_len[i], q0 = R.seq_start[i], l_seq = R.seq_len[i], aux = R.aux_start[i];
    const uint32_t ops = n_cig[i];
    uint8_t *__restrict__ dst = out + out_off[i];
    uint8_t *cig_at = dst + 36 + name + 1;
    dst[36 + name] = 0;
    long long flag = 0, pos1 = 0, mapq = 0, pnext = 0, tlen = 0, span = 0;
    uint32_t b = s + name + 1, f, n_ops;
    auto field = [&] { f = sam_next_tab(text, b, q0 - 1); };
    auto next = [&] { b = f + 1; };
    field(), sam_int(text + b, f - b, &flag), next();
    field();
    const int32_t rid = sam_ref_id(text, b, f - b, F);
    next();
    field(), sam_int(text + b, f - b, &pos1), next();
    field(), sam_int(text + b, f - b, &mapq), next();
    field(), sam_bam_cigar<true>(text, b, f, cig_at, &n_ops, &span), next();
    field();
    const int32_t next_rid = (f - b == 1 && text[b] == '=') ? rid : sam_ref_id(text, b, f - b, F);
    next();
    field(), sam_int(text + b, f - b, &pnext), next();
    field(), sam_int(text + b, f - b, &tlen);
    const int32_t pos = (int32_t)((uint32_t)pos1 - 1u), next_pos = (int32_t)((uint32_t)pnext - 1u);
    const uint32_t bin = (uint32_t)sam_reg2bin(pos, (long long)pos + (span ? span : 1)) & 0xFFFFu;
    uint8_t *t = dst;
    sam_put<uint32_t>(t, out_len[i] - 4);
    sam_put<int32_t>(t, rid);
    sam_put<int32_t>(t, pos);
    sam_put<uint32_t>(t, (name + 1) | ((uint32_t)mapq & 255u) << 8 | bin << 16);
    sam_put<uint32_t>(t, ops | ((uint32_t)flag & 0xFFFFu) << 16);
    sam_put<uint32_t>(t, l_seq);
    sam_put<int32_t>(t, next_rid);
    sam_put<int32_t>(t, next_pos);
    sam_put<int32_t>(t, (int32_t)(uint32_t)tlen);
    t = cig_at + 4 * ops + (l_seq + 1) / 2 + l_seq;
    bool ok = true;
    if (aux < e) t += sam_bam_opts<true>(text, aux, e, t, &ok);
    t[0] = (uint8_t)tag0, t[1] = (uint8_t)tag1, t[2] = 'Z';
    t += 3;
    const unsigned long long f0 = found_off[i], f1 = found_off[i + 1];
    const uint32_t ex_at = ex_off[i];  // (0: no existing value; else it ends at the next tab or with the line)
    uint32_t ex_n = 0;
    if (ex_at)
        while (ex_at + ex_n < e && text[ex_at + ex_n] != '\t') ++ex_n;
    *tag_value_put(t, text + ex_at, ex_n, f0, f1, found_pat, pat_off, pat_bytes) = 0;
}

// Pass 2, the wide part: read_name, SEQ as nibbles, QUAL less 33 (or 0xFF for "*"); 16 lanes per record, 16 text bytes per lane and step
__global__ __launch_bounds__(256) void mk_sam_bam_seq_kernel(const uint8_t *__restrict__ text, SamTables R, const uint8_t *__restrict__ keep,
                                                            const unsigned long long *__restrict__ out_off, const uint32_t *__restrict__ n_cig, uint64_t n_rec,
                                                            uint8_t *__restrict__ out) {
    const uint64_t i = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const uint32_t sub = threadIdx.x & 15u;
    if (i >= n_rec || !keep[i]) return;
    const uint32_t s = R.rec_start[i], e = s + R.rec_len[i], name = R.name_len[i], q0 = R.seq_start[i], l_seq = R.seq_len[i], aux = R.aux_start[i];
    uint8_t *__restrict__ dst = out + out_off[i];
    uint8_t *sq = dst + 36 + name + 1 + 4 * n_cig[i], *ql = sq + (l_seq + 1) / 2;
    for (uint32_t k = sub; k < name; k += 16) dst[36 + k] = text[s + k];
    if (!l_seq) return;
    uint32_t qs = 0, qe = 0;
    bool empty_field;
    sam_qual(text, q0, l_seq, aux, e, &qs, &qe, &empty_field);
    const bool no_qual = qe - qs == 1 && text[qs] == '*';
    for (uint32_t k = 16 * sub; k < l_seq; k += 256) {
        if (k + 16 <= l_seq) {
            SamBytes16 v = sam_ld128(text + q0 + k);
            uint32_t o[2];
            for (int w = 0; w < 4; ++w) {
                const uint32_t x = v.w[w];
                const uint32_t two = (sam_nibble(x & 255u) << 4 | sam_nibble((x >> 8) & 255u)) | (sam_nibble((x >> 16) & 255u) << 4 | sam_nibble(x >> 24)) << 8;
                if (w & 1) o[w >> 1] |= two << 16;
                else o[w >> 1] = two;
            }
            __builtin_memcpy(sq + k / 2, o, 8);
            if (no_qual) {
                v.w[0] = v.w[1] = v.w[2] = v.w[3] = 0xFFFFFFFFu;
            } else {
                v = sam_ld128(text + qs + k);
                for (int w = 0; w < 4; ++w) v.w[w] = sam_sub33x4(v.w[w]);
            }
            sam_st128(ql + k, v);
        } else {  // (the last bases; an odd length pads the low nibble with 0)
            for (uint32_t j = k; j < l_seq; j += 2)
                sq[j / 2] = (uint8_t)(sam_nibble(text[q0 + j]) << 4 | (j + 1 < l_seq ? sam_nibble(text[q0 + j + 1]) : 0u));
            for (uint32_t j = k; j < l_seq; ++j) ql[j] = no_qual ? (uint8_t)0xFF : (uint8_t)(text[qs + j] - 33u);
        }
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------------------
void launch_sam_fields(const uint8_t *d_text, const uint32_t *d_line_start, uint64_t n_lines, uint32_t *d_is_rec, const SamTables &L, uint32_t *d_st,
                       hipStream_t st) {
    if (!n_lines) return;
    hipLaunchKernelGGL(mk_sam_fields_kernel, dim3((unsigned)((n_lines * 16 + 255) / 256)), dim3(256), 0, st, d_text, d_line_start, n_lines, d_is_rec, L, d_st);
}
void launch_sam_compact(const uint32_t *d_is_rec, const unsigned long long *d_rec_index, uint64_t n_lines, const SamTables &L, const SamTables &R,
                        hipStream_t st) {
    if (!n_lines) return;
    hipLaunchKernelGGL(mk_sam_compact_kernel, dim3((unsigned)((n_lines + 255) / 256)), dim3(256), 0, st, d_is_rec, d_rec_index, n_lines, L, R);
}
void launch_sam_gather(const uint8_t *d_text, const uint32_t *d_seq_start, const uint32_t *d_seq_len, const unsigned long long *d_off, uint32_t fixed_len,
                       uint64_t n_rec, uint8_t *d_seq, hipStream_t st) {
    if (!n_rec) return;
    hipLaunchKernelGGL(mk_sam_gather_kernel, dim3((unsigned)((n_rec * 16 + 255) / 256)), dim3(256), 0, st, d_text, d_seq_start, d_seq_len, d_off, fixed_len,
                       n_rec, d_seq);
}
void launch_sam_names(const uint32_t *d_name_len, const uint8_t *d_flags, uint64_t n_rec, uint32_t *d_name_len_out, hipStream_t st) {
    if (!n_rec) return;
    hipLaunchKernelGGL(mk_sam_names_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, d_name_len, d_flags, n_rec, d_name_len_out);
}
void launch_sam_name_ends(const uint32_t *d_name_len_out, const unsigned long long *d_name_off, uint64_t n_rec, uint8_t *d_names, hipStream_t st) {
    if (!n_rec) return;
    hipLaunchKernelGGL(mk_sam_name_ends_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, d_name_len_out, d_name_off, n_rec, d_names);
}
void launch_sam_taglen(const uint8_t *d_text, const SamTables &R, const unsigned long long *d_found_off, const uint32_t *d_found_pat, const uint32_t *d_pat_off,
                       const uint8_t *d_pat_bytes, uint64_t n_rec, uint32_t filter_matching, uint32_t invert, uint32_t tag0, uint32_t tag1, uint8_t *d_keep,
                       uint32_t *d_out_len, uint32_t *d_ex_off, uint32_t *d_st, hipStream_t st) {
    if (!n_rec) return;
    hipLaunchKernelGGL(mk_sam_taglen_kernel, dim3((unsigned)((n_rec * 16 + 255) / 256)), dim3(256), 0, st, d_text, R, d_found_off, d_found_pat, d_pat_off, n_rec,
                       d_pat_bytes, filter_matching, invert, tag0, tag1, d_keep, d_out_len, d_ex_off, d_st);
}
void launch_sam_emit(const uint8_t *d_text, const SamTables &R, const uint32_t *d_out_len, const unsigned long long *d_out_off,
                     const unsigned long long *d_found_off, const uint32_t *d_found_pat, const uint8_t *d_pat_bytes, const uint32_t *d_pat_off,
                     const uint32_t *d_ex_off, uint64_t n_rec, uint32_t tag0, uint32_t tag1, uint8_t *d_out, hipStream_t st) {
    if (!n_rec) return;
    hipLaunchKernelGGL(mk_sam_emit_kernel, dim3((unsigned)((n_rec * 16 + 255) / 256)), dim3(256), 0, st, d_text, R, d_out_len, d_out_off, d_found_off,
                       d_found_pat, d_pat_bytes, d_pat_off, d_ex_off, n_rec, tag0, tag1, d_out);
}
void launch_sam_bam_len(const uint8_t *d_text, const SamTables &R, const uint8_t *d_keep, uint64_t n_rec, uint32_t *d_out_len, uint32_t *d_n_cig, uint32_t *d_st,
                        hipStream_t st) {
    if (!n_rec) return;
    hipLaunchKernelGGL(mk_sam_bam_len_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, d_text, R, d_keep, n_rec, d_out_len, d_n_cig, d_st);
}
void launch_sam_bam_encode(const uint8_t *d_text, const SamTables &R, const uint8_t *d_keep, const uint32_t *d_out_len, const unsigned long long *d_out_off,
                           const uint32_t *d_n_cig, const unsigned long long *d_found_off, const uint32_t *d_found_pat, const uint8_t *d_pat_bytes,
                           const uint32_t *d_pat_off, const uint32_t *d_ex_off, const uint8_t *d_ref_bytes, const uint32_t *d_ref_off, const uint32_t *d_ref_table,
                           uint32_t ref_table_mask, uint64_t n_rec, uint32_t tag0, uint32_t tag1, uint8_t *d_out, hipStream_t st) {
    if (!n_rec) return;
    hipLaunchKernelGGL(mk_sam_bam_fields_kernel, dim3((unsigned)((n_rec + 255) / 256)), dim3(256), 0, st, d_text, R, d_keep, d_out_len, d_out_off, d_n_cig,
                       d_found_off, d_found_pat, d_pat_bytes, d_pat_off, d_ex_off, SamRefs{d_ref_bytes, d_ref_off, d_ref_table, ref_table_mask}, n_rec, tag0, tag1,
                       d_out);
    hipLaunchKernelGGL(mk_sam_bam_seq_kernel, dim3((unsigned)((n_rec * 16 + 255) / 256)), dim3(256), 0, st, d_text, R, d_keep, d_out_off, d_n_cig, n_rec, d_out);
}

}  // namespace mk
