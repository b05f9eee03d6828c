// sam.hip -- a window of SAM text on the device: its lines become a record table, the SEQ fields become the text the matcher scans,
// and the kept lines leave with their `km` field appended -- what the reference's reader thread, record loop and text writer do
// one record at a time (src/cmd_tag.rs:559-612 `for record in reader`, :387-497 process_record) and what the CLI's host path does
// on its threads (cli/io.cpp: parse_sam_text, SamFile::gather, SamFile::find_tag), which is the definition these kernels follow.
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
// (the keep rule and the value itself are tag_merge.hpp's, shared with bam.hip; the host side of both is host_loops.cpp: tag_scan / tag_keep)
// Every access is bounded by the line it belongs to: a load of 16 bytes starts inside the line and may run up to 15 bytes past its
// end, which the text buffer's padding (64 bytes behind the window, host_loops.cpp: window_assemble) covers.
#include "scan_kernel.h"
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

// SEQ of record i -> seq[fixed_len ? i * fixed_len : off[i]] as the matcher sees it (cli/io.cpp: SamFile::gather); 16 lanes per record,
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
// least five bytes that starts with the tag and ':' (cli/io.cpp: SamFile::find_tag): 16 lanes look at the tabs of 16 bytes each, a
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

}  // namespace mk
