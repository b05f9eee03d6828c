/*
 * merkurio_hip.h -- C ABI of the MI355X-native multi-pattern matcher that replaces
 * MerKurio's pattern_matching hot path (BNDMq / Aho-Corasick) for `merkurio extract|tag`.
 *
 * The reference has no trait / plugin / FFI for this path: its drivers hold
 * `(Option<AhoCorasick>, Vec<(String, BNDMq)>)` (src/cmd_extract.rs:259, src/cmd_tag.rs:234)
 * and call the matcher once per record.  A GPU wants batches, so this ABI exposes the same
 * observable contract per *batch of records*; every entry point below names the reference
 * interface it replaces (paths relative to the reference repo).  A Rust host binds these
 * symbols with `extern "C"`.
 *
 * Conventions
 *  - plain pointers and sizes only; no C++/torch types cross the boundary;
 *  - every function returns 0 (MK_OK) or a negative MK_E_* code; mk_last_error() gives the
 *    text for the calling thread; nothing throws across the ABI (host allocation failures and
 *    hipErrorOutOfMemory come back as MK_E_NOMEM);
 *  - there is NO CPU fallback: without a usable HIP device creation fails with MK_E_HIP;
 *  - a matcher handle is bound to one HIP device and supports ONE scan in flight at a time
 *    (its tuple staging buffer, timing events and launch bookkeeping are per handle): enqueue
 *    the next scan of a handle on the same stream, or after the previous one has completed;
 *    distinct handles (one per GPU / per process / per stream) are independent;
 *  - nothing here reads environment variables: tuning goes through mk_matcher_options;
 *  - the caller owns every buffer it passes; the library copies patterns at create time;
 *  - every output that comes with a capacity: a call that needs more returns MK_E_CAPACITY, states the size it needs where the
 *    entry point says so, and writes nothing at or behind the capacity it was given (a capacity of 0 with a pointer is a
 *    capacity).  Such a call leaves the handle as a call that fits does: the next call's answer does not depend on it.  What
 *    a refused call leaves in its other outputs is said per call family below; where nothing is said it is unspecified, and
 *    counters / pattern_hit_counts, which are += updated, must be fresh for every attempt.
 */
#ifndef MERKURIO_HIP_H
#define MERKURIO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MK_ABI_VERSION 7

/* ---- error codes.  -1..-3 map 1:1 to PatternError (src/pattern_matching.rs:28-36) ---- */
#define MK_OK 0
#define MK_E_EMPTY_PATTERN (-1)    /* PatternError::EmptyPattern */
#define MK_E_INVALID_Q (-2)        /* PatternError::InvalidQGramLength(q) */
#define MK_E_PATTERN_TOO_LONG (-3) /* PatternError::PatternTooLong(len, 64) */
#define MK_E_NO_PATTERNS (-4)      /* "No k-mers found ..." (src/helpers.rs:128-130,158-160) */
#define MK_E_NOMEM (-5)
#define MK_E_PAIR_MISMATCH (-6) /* paired inputs differ in record count (src/cmd_extract.rs:465-468,608-612) */
#define MK_E_HIP (-7)           /* HIP runtime error / no device */
#define MK_E_CAPACITY (-8)      /* output buffer too small; required size is reported */
#define MK_E_INVALID_ARG (-9)
#define MK_E_UNSUPPORTED (-10)
#define MK_E_RCCL (-11) /* RCCL missing or a collective failed (counter reduction only) */
#define MK_E_CORRUPT (-12) /* a BGZF member that does not inflate to its ISIZE / CRC-32 (mk_bgzf_inflate) */

/* algorithm selector: what the reference's `-a` / `-q` / auto rule decides
 * (src/cmd_extract.rs:166-171, src/helpers.rs:203-211).  The device scan is the same for
 * both; the algorithm fixes the EMISSION ORDER and the pattern_hit_counts semantics. */
#define MK_ALGO_AUTO 0  /* AC iff case-insensitive, or n >= 14, or max_len > 64 */
#define MK_ALGO_AC 1    /* aho_corasick::AhoCorasick (DFA, overlapping search) */
#define MK_ALGO_BNDMQ 2 /* pattern_matching::BNDMq, one instance per pattern */

#define MK_FLAG_ASCII_CASE_INSENSITIVE 1u /* AhoCorasickBuilder::ascii_case_insensitive(true) */

/* scan modes = what the reference loops consume from the matcher */
#define MK_MODE_ANY 0  /* per-record "any hit" flag only  (find_match / first-hit break) */
#define MK_MODE_HITS 1 /* + every (record, pattern, start) in reference emission order */

typedef struct mk_matcher mk_matcher;

/* one occurrence: pattern `pat` (index into the sorted unique pattern list) starts at byte
 * `pos` (0-based) of record `rec`.  == (mat.pattern().as_usize(), mat.start()) of
 * src/cmd_extract.rs:341-342 and the `o` of BNDMq::find_iter (src/cmd_extract.rs:367).
 * Limits of this build: a single record shorter than 4 GiB (`pos` is 32 bits; a batch may hold
 * any number of bytes and records), at most 2^27 - 2 patterns and at most 2^26 exact-table entries
 * (patterns x sampling stride, the stride being 1..16 as mk_matcher_filter_info reports it):
 * larger sets fail at create time with MK_E_UNSUPPORTED. */
typedef struct {
    uint64_t rec;
    uint32_t pat;
    uint32_t pos;
} mk_hit;

/* one log row: mk_hit plus the file (mate) index; logger.log_fields arguments,
 * src/logger.rs:41 */
typedef struct {
    uint64_t rec;
    uint32_t pat;
    uint32_t pos;
    uint32_t file; /* 0 = file 1, 1 = file 2 */
    uint32_t _pad;
} mk_row;

/* the scalar counters of src/cmd_extract.rs:285-289 / src/cmd_tag.rs:360-363 */
typedef struct {
    uint64_t nb_records_tot;
    uint64_t nb_bases;
    uint64_t nb_hits_tot[2];
    uint64_t nb_records_hit[2];
    uint64_t nb_records_extracted;
} mk_counters;

/* ------------------------------------------------------------------------------------
 * Library / device
 * ---------------------------------------------------------------------------------- */
int mk_abi_version(void);
const char *mk_last_error(void);
/* number of visible HIP devices (0 if none); never fails */
int mk_device_count(void);

/* ------------------------------------------------------------------------------------
 * Pattern preparation (host side; defines the pattern index space)
 * ---------------------------------------------------------------------------------- */
/* helpers::read_kmers_from_file body, src/helpers.rs:152-156: content -> raw k-mer lines.
 * Outputs are malloc'd by the library; release with mk_free. */
int mk_read_kmers_from_text(const uint8_t *content, size_t len, uint8_t **out_bytes, uint32_t **out_off,
                            uint32_t *out_n);
/* helpers::parse_pattern_list, src/helpers.rs:76-133: case conversion, reverse-complement
 * extension (-r) or canonical form (-c), drop empty, sort_unstable, dedup. */
int mk_parse_pattern_list(const uint8_t *in_bytes, const uint32_t *in_off, uint32_t n_in, int reverse_complement,
                          int canonical, int lowercase, int uppercase, uint8_t **out_bytes, uint32_t **out_off,
                          uint32_t *out_n);
/* needletail Sequence::reverse_complement / sequence::canonical as used at
 * src/helpers.rs:103,117.  out must hold n bytes. */
void mk_reverse_complement(const uint8_t *in, size_t n, uint8_t *out);
void mk_canonical(const uint8_t *in, size_t n, uint8_t *out);
/* helpers::recommend_aho_corasick, src/helpers.rs:203-211 */
int mk_recommend_aho_corasick(size_t num_patterns, size_t max_len);
/* pattern_matching::tune_q_value, src/pattern_matching.rs:213-225 (0 for len >= 65) */
size_t mk_tune_q_value(size_t pattern_len);
/* pattern_preprocessing::generate_masks, src/pattern_preprocessing.rs:24-43 */
int mk_generate_masks(const uint8_t *pattern, size_t m, uint64_t masks[256], uint64_t *accept);
void mk_free(void *p);

/* ------------------------------------------------------------------------------------
 * Matcher construction
 * replaces: BNDMq::new per pattern (src/pattern_matching.rs:61-78, called at
 * src/cmd_extract.rs:267-276) and AhoCorasick::builder()...build() (src/cmd_extract.rs:260-265,
 * src/cmd_tag.rs:235-240).
 *
 * pat_bytes/pat_off: n_pat patterns, pattern i = pat_bytes[pat_off[i] .. pat_off[i+1]); the
 * list must already be the sorted unique list of parse_pattern_list (indices are reported
 * as given).  algo: MK_ALGO_*.  q: BNDMq q-gram length, 0 = tune_q_value per pattern;
 * ignored for AC.  q has no effect on results, but its validation errors are reproduced
 * (MK_E_INVALID_Q, MK_E_EMPTY_PATTERN, MK_E_PATTERN_TOO_LONG for BNDMq patterns > 64 B).
 * flags: MK_FLAG_* (case-insensitive forces AC like src/cmd_extract.rs:166-167).
 * device: HIP device ordinal.
 * ---------------------------------------------------------------------------------- */
int mk_matcher_create(const uint8_t *pat_bytes, const uint32_t *pat_off, uint32_t n_pat, uint32_t algo, uint32_t q,
                      uint32_t flags, int32_t device, mk_matcher **out);
/* Same, with explicit tuning / test options (NULL = defaults = mk_matcher_create).  Options never
 * change results, only the filter geometry the scan kernel runs with. */
typedef struct {
    uint32_t struct_size;         /* = sizeof(mk_matcher_options); lets the struct grow compatibly */
    uint32_t force_stride;        /* 0 = geometry rule; else sampling stride 1, 2, 4, 8 or 16 */
    uint32_t force_global_filter; /* 1 = level-1 filter in global memory even for small sets */
    uint32_t gbloom_log2_blocks;  /* 0 = rule; else log2 of the number of 64-bit blocks of a global filter */
    uint32_t tile_run;            /* 0 = rule; else R in 1..8: a scan wave's long tiles are 32 R - 1 KiB + a 1 KiB halo (mk_scan_tile_geometry).
                                   * A test hook.  On a text so short that the grid is not full (fewer 31 KiB tiles than 16 waves per compute
                                   * unit), a forced R > 1 launches only as many workgroups (of 16 waves) as the text has long tiles for,
                                   * at least one, so that the forced length is what runs; on any longer text of less than one round of
                                   * long tiles the grid stays full and all of it runs in 31 KiB tiles.  R is shortened where the device's wave
                                   * count times the tile length would exceed 1 GiB (mk_matcher_scan_geometry reports what ran). */
    uint32_t gbloom_kib;          /* 0 = rule; else size of a global filter in KiB (any size, overrides gbloom_log2_blocks) */
    /* length classes (ABI 4).  A set whose shortest pattern is much shorter than the rest is split by length: the
     * short patterns get their own stride and q-gram table next to the main filter (one pass, one kernel). */
    uint32_t length_classes;      /* 0 = rule (split where the cost model says it pays); 1 = never split; 2 = split */
    uint32_t force_split_len;     /* 0 = rule; else patterns shorter than this form the short class */
    uint32_t force_stride2;       /* 0 = rule; else stride of the short class: 1, 2, 4 or 8 */
    uint32_t force_q2;            /* 0 = rule; else q-gram length of the short class, 1..8 (clamped to what its shortest pattern admits) */
} mk_matcher_options;
int mk_matcher_create_ex(const uint8_t *pat_bytes, const uint32_t *pat_off, uint32_t n_pat, uint32_t algo, uint32_t q,
                         uint32_t flags, int32_t device, const mk_matcher_options *options, mk_matcher **out);
/* The filter geometry mk_matcher_create_ex would choose for patterns of these lengths, without creating anything (host
 * only, no device needed) -- this library's counterpart of what AhoCorasick::builder()...build() decides about its
 * automaton from the pattern list (src/cmd_extract.rs:260-265), which scans any list at one speed: main-class q-gram length and stride, whether the level-1 filter fits LDS, and the length
 * classes (see mk_matcher_class_info).  Any output pointer may be NULL. */
int mk_plan_geometry(const uint32_t *pat_len, uint32_t n_pat, const mk_matcher_options *options, uint32_t *q_gram, uint32_t *stride,
                     uint32_t *in_lds, uint32_t *split_len, uint32_t *n_short, uint32_t *q_gram2, uint32_t *stride2);
void mk_matcher_destroy(mk_matcher *m);
/* MK_ALGO_AC or MK_ALGO_BNDMQ after the auto rule was applied */
uint32_t mk_matcher_algo(const mk_matcher *m);
uint32_t mk_matcher_num_patterns(const mk_matcher *m);
/* filter geometry chosen at create time: q-gram length, sampling stride, table entries */
int mk_matcher_filter_info(const mk_matcher *m, uint32_t *q_gram, uint32_t *stride, uint64_t *entries,
                           uint64_t *table_bytes);
/* length classes chosen at create time: *split_len = 0 (one class: mk_matcher_filter_info describes it) or the
 * length below which a pattern belongs to the short class, the number of such patterns, and the short class's
 * q-gram length and stride (mk_matcher_filter_info then describes the main class; `entries` counts both) */
int mk_matcher_class_info(const mk_matcher *m, uint32_t *split_len, uint32_t *n_short, uint32_t *q_gram2, uint32_t *stride2);
/* where the level-1 filter lives: *in_lds = 1 (128 KiB image staged in LDS by every workgroup)
 * or 0 (large pattern sets: blocks in global memory, L2 / Infinity-Cache resident), and its size */
int mk_matcher_filter_mode(const mk_matcher *m, uint32_t *in_lds, uint64_t *filter_bytes);

/* ------------------------------------------------------------------------------------
 * Batched scan, host buffers
 * replaces, for a whole batch of records: BNDMq::find_match / find_iter / find_all
 * (src/pattern_matching.rs:128-153) and AhoCorasick::find_overlapping_iter
 * (src/cmd_extract.rs:332,480,507; src/cmd_tag.rs:393-396).
 *
 * record i = seq_bytes[seq_off[i] .. seq_off[i+1]) (newline-free sequence bytes exactly as
 * needletail's record.seq() / bam's record.sequence() hand them to the matcher).
 * rec_flags[i] = 1 iff any pattern occurs in record i.
 * MK_MODE_HITS: hits[0..*n_hits) = every occurrence, in the reference's emission order for
 * the matcher's algorithm: AC: record, end ascending, start ascending, pattern ascending;
 * BNDMq: record, pattern ascending, start ascending.
 * If more than hits_cap occurrences exist: returns MK_E_CAPACITY, *n_hits = required
 * count, rec_flags valid, hits content unspecified (nothing at or behind hits_cap is written).  Never truncates silently.
 * ---------------------------------------------------------------------------------- */
int mk_scan_batch(mk_matcher *m, const uint8_t *seq_bytes, const uint64_t *seq_off, uint64_t n_rec, uint32_t mode,
                  uint8_t *rec_flags, mk_hit *hits, uint64_t hits_cap, uint64_t *n_hits);

/* ------------------------------------------------------------------------------------
 * Batched scan, device-resident buffers (the kernel boundary; asynchronous)
 *
 * All pointers are device pointers on the matcher's device.  d_seq must be 16-byte aligned and
 * d_seq_off[0] must be 0 (offsets relative to d_seq);
 * d_rec_flags 4-byte aligned with its allocation padded to a multiple of 4 bytes.
 * The call enqueues on `stream` (a hipStream_t, NULL = default stream): clear of
 * d_rec_flags[0..n_rec) and of *d_n_hits, then the scan kernel (and, behind it, a small kernel that sets
 * the flag bytes of the records the scan has listed).  d_hits may be NULL in
 * MK_MODE_ANY.  Hits are written UNORDERED (order them with mk_order_hits_device, or with
 * mk_order_hits after copying back); in MK_MODE_HITS *d_n_hits counts every occurrence even beyond hits_cap (0 in MK_MODE_ANY).
 * d_counters (may be NULL): uint64[n_pat + MK_NUM_SUMMARY] accumulated (+=) by the scan:
 *   [0, n_pat)            occurrences per pattern (the AC meaning of pattern_hit_counts,
 *                         src/cmd_extract.rs:353).  MK_MODE_HITS only, counted from the stored tuples
 *                         (all of them unless *d_n_hits exceeds hits_cap); MK_MODE_ANY leaves these
 *                         entries untouched -- the reference's no-logging path counts nothing either
 *   [n_pat + MK_SUM_*]    see below; they do not depend on hits_cap: MK_SUM_HITS counts every occurrence, as *d_n_hits does
 *                         (nb_hits_tot counts hits, not log rows), also beyond hits_cap
 * More than hits_cap occurrences is not an error of this call (it only enqueues): d_hits[0, hits_cap) then holds hits_cap
 * distinct occurrences, nothing at or behind d_hits[hits_cap] is written, the flags are valid, and the caller sees it from
 * *d_n_hits > hits_cap.
 * It is the vector a multi-GPU host sums across ranks (RCCL allReduce) at the end of a job.
 * ---------------------------------------------------------------------------------- */
#define MK_NUM_SUMMARY 8
#define MK_SUM_HITS 0        /* nb_hits_tot */
#define MK_SUM_RECORDS_HIT 1 /* nb_records_hit */
#define MK_SUM_RECORDS 2     /* nb_records_tot */
#define MK_SUM_BASES 3       /* nb_bases */
#define MK_SUM_CANDIDATES 4  /* filter positives sent to verification (diagnostic) */

int mk_scan_device(mk_matcher *m, const void *d_seq, uint64_t n_bytes, const void *d_seq_off, uint64_t n_rec,
                   uint32_t mode, void *d_rec_flags, void *d_hits, uint64_t hits_cap, void *d_n_hits,
                   void *d_counters, void *stream);

/* mk_scan_device only enqueues, so what a kernel finds wrong with its input comes back later: waits for `stream`,
 * then returns MK_E_UNSUPPORTED if the handle's LAST MK_MODE_HITS scan met an occurrence 4 GiB or more into its
 * record (mk_hit.pos cannot hold it; the flags of that scan are valid, its tuples are not), else MK_OK.
 * mk_order_hits_device makes the same check at its own round trip (from two tuples up: fewer need no ordering and are
 * not checked there); mk_scan_batch refuses such a record before it scans.  The condition is cleared by the call that
 * reports it and by the next MK_MODE_HITS scan on the handle. */
int mk_matcher_check_device(mk_matcher *m, void *stream);

/* Performance hint for mk_scan_device (never changes results): how many of 1000 records the caller
 * expects to contain a pattern.  Dense text (>= 145, or >= 95 when tuples are written) is streamed with cacheable loads, because the
 * exact verification re-reads every hit window; sparse text with non-temporal loads.  mk_scan_batch
 * and the driver-loop entry points maintain the value themselves from the batch they have just scanned. */
int mk_matcher_hint_hit_density(mk_matcher *m, uint32_t records_hit_per_1000);

/* Fixed-length batches (not a hint -- a statement about the data): with record_length > 0 every following
 * mk_scan_device on this handle takes record i to be d_seq[i * record_length, (i + 1) * record_length):
 * n_bytes must equal n_rec * record_length (else MK_E_INVALID_ARG) and d_seq_off is NOT read (it may be NULL --
 * 8 bytes per record the caller need not build).  The record of a verified occurrence is then computed instead
 * of looked up: one random memory transaction fewer per occurrence.  0 (the default) returns to offsets.
 * mk_scan_batch and the driver-loop entry points check their host offsets and do this by themselves. */
int mk_matcher_set_fixed_record_length(mk_matcher *m, uint32_t record_length);

/* Second hint for mk_scan_device: do the records of the batches differ in length (trimmed reads)?  With
 * equal_lengths == 0 every scan first builds a coarse record index (one entry per 64 KiB of text) for the
 * record lookup of verified occurrences; with 1 (the default) the index of a record is estimated from its
 * position, which is exact for equal lengths and merely slower otherwise.  mk_scan_batch decides by itself. */
int mk_matcher_hint_record_lengths(mk_matcher *m, int equal_lengths);

/* Sort hits (host memory) into the reference's emission order for this matcher:
 * Aho-Corasick find_overlapping_iter (src/cmd_extract.rs:332, src/cmd_tag.rs:393-396) per record end
 * ascending, longer pattern first, pattern id; BNDMq driver loop (src/cmd_extract.rs:365-384) per record
 * pattern-major, positions ascending. */
int mk_order_hits(const mk_matcher *m, mk_hit *hits, uint64_t n_hits);
/* The same order for tuples still on the device (d_hits as written by mk_scan_device, n_hits <= hits_cap of
 * them, 16-byte aligned), sorted in place on `stream` by hand-written kernels: tuples are counted into bins of
 * consecutive records, stored into their bin as 8-byte keys and each bin is sorted in LDS -- two passes over the
 * tuples and one over the keys (order_hits.hip).  The call waits ONCE for the stream (32 bytes of histogram
 * statistics fix the key layout; the caller has just read n_hits the same way) and returns with the rest enqueued.
 * Bins use the record count of the handle's last mk_scan_device; tuples of another batch are still ordered
 * correctly.  Batches that defeat the binning (a bin above 16384 tuples after re-binning on the top bits of the whole
 * record / end / pattern key,
 * more than 2^32 - 1 tuples, or record / end / pattern fields that do not fit 64 bits together) are ordered by a
 * library merge sort instead.  mk_scan_batch uses this by itself.  The scratch buffer (8 bytes per tuple) lives in
 * the handle (growing it synchronises the device; one call in flight per handle). */
int mk_order_hits_device(mk_matcher *m, void *d_hits, uint64_t n_hits, void *stream);
/* what the last mk_order_hits_device on this handle did: *path = 0 nothing (fewer than two tuples), 1 bins of
 * consecutive records, 2 bins on the top bits of the whole (record, end, pattern) key, 3 library merge sort; the number of
 * bins and the largest bin (paths 1 and 2) */
int mk_matcher_order_info(const mk_matcher *m, uint32_t *path, uint32_t *n_bins, uint32_t *max_bin);
/* (v6) how often each of those paths ran over the handle's life, driver-loop calls included: calls[p] for p = 0..3.  A host
 * program can tell from calls[3] whether its data ever sent the ordering to the library sort. */
int mk_matcher_order_stats(const mk_matcher *m, uint64_t calls[4]);

/* name of the scan kernel variant the last mk_scan_device on this handle launched, and its
 * launch geometry (for profiling / roofline bookkeeping) */
const char *mk_matcher_kernel_name(const mk_matcher *m);
int mk_matcher_launch_info(const mk_matcher *m, uint32_t *grid_blocks, uint32_t *block_threads, uint32_t *lds_bytes);
/* How a scan launch cuts its text into wave tiles (host arithmetic only, no device needed).  Tile i belongs to scan
 * wave i mod n_waves.  Tiles [0, n_long_tiles) are long_tile_bytes long and lie back to back from byte 0: a whole
 * number of rounds (n_long_tiles is a multiple of n_waves).  Tiles [n_long_tiles, n_long_tiles + n_short_tiles) follow
 * them, short_tile_bytes each (15 .. 31 KiB, the length that loads the busiest wave least): less than one round of long tiles.  [tail_start, n_bytes) is scanned with guarded loads,
 * one 1 KiB chunk per wave.  A tile is fetched with *_tile_loads loads of 1 KiB, one more than it has KiB: the last
 * one is the next tile's first KiB, so the scan streams n_bytes + 1 KiB per tile.  tile_run = R in 1..8: long tiles of
 * 32 R - 1 KiB; R = 1 is one region of 31 KiB tiles (n_long_tiles = 0); 0 = the R that a scan picks by itself for this
 * text and these waves (returned in tile_run). */
typedef struct {
    uint64_t n_waves;
    uint64_t n_long_tiles, long_tile_bytes;
    uint64_t n_short_tiles, short_tile_bytes;
    uint64_t tail_start;
    uint32_t long_tile_loads, short_tile_loads;
    uint32_t tile_run;
    uint32_t reserved;
} mk_tile_geometry;
int mk_scan_tile_geometry(uint64_t n_bytes, uint64_t n_waves, uint32_t tile_run, mk_tile_geometry *out);
/* the geometry of the last mk_scan_device on this handle (tile_run: the R its rule picked, or the forced one) */
int mk_matcher_scan_geometry(const mk_matcher *m, mk_tile_geometry *out);
/* Per-launch kernel timing with hipEvents recorded on the launch stream immediately before
 * and after the scan kernel (not around the buffer clears).  enable_timing(slots) keeps the
 * last `slots` launches; kernel_times() waits for them, returns their durations in ms
 * (oldest first) and resets the window.  slots == 0 disables. */
int mk_matcher_enable_timing(mk_matcher *m, uint32_t slots);
int mk_matcher_kernel_times(mk_matcher *m, float *ms, uint32_t cap, uint32_t *n_out);

/* ------------------------------------------------------------------------------------
 * Driver-loop semantics on batches (host buffers)
 * These restate what the reference's record loops do with the matcher's answers, so that
 * counters, log rows and keep/drop decisions are bit-identical.
 * ---------------------------------------------------------------------------------- */
/* extract, single file: loop body src/cmd_extract.rs:321-406.
 * logging == 0: only keep[] and nb_records_extracted are produced (like the reference).
 * rows (may be NULL when logging == 0) receives the log rows in emission order; on overflow
 * returns MK_E_CAPACITY with *n_rows = required.  pattern_hit_counts[n_pat] is += updated.
 * A call of this family (mk_extract_single / _paired, mk_tag_records, mk_extract_fastq_text / _bgzf, mk_extract_window) that
 * returns MK_E_CAPACITY for its rows, found_pat or kept text has done all its work: keep is valid, counters and
 * pattern_hit_counts have been added to (pass fresh ones with the next attempt), rows[0, rows_cap) are the first rows. */
int mk_extract_single(mk_matcher *m, const uint8_t *seq, const uint64_t *off, uint64_t n_rec, int logging,
                      int invert, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows,
                      mk_counters *counters, uint32_t *pattern_hit_counts);
/* extract, paired: loop body src/cmd_extract.rs:463-612.  keep[i] applies to pair i. */
int mk_extract_paired(mk_matcher *m, const uint8_t *seq1, const uint64_t *off1, uint64_t n_rec1,
                      const uint8_t *seq2, const uint64_t *off2, uint64_t n_rec2, int logging, int invert,
                      uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *counters,
                      uint32_t *pattern_hit_counts);
/* tag: process_record matching + set logic, src/cmd_tag.rs:387-467.
 * found_off[n_rec+1] / found_pat: CSR of the distinct matched pattern indices per record,
 * ascending (= kmers_found after sort_unstable + dedup, src/cmd_tag.rs:484-485, before the
 * merge with a pre-existing tag value).  On found_cap overflow: MK_E_CAPACITY, found_off[n_rec]
 * = required.  One call states both needs, *n_rows and found_off[n_rec], whichever was too small. */
int mk_tag_records(mk_matcher *m, const uint8_t *seq, const uint64_t *off, uint64_t n_rec, int logging,
                   int filter_matching, int invert, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows,
                   mk_counters *counters, uint32_t *pattern_hit_counts, uint64_t *found_off, uint32_t *found_pat,
                   uint64_t found_cap);
/* extract, single FASTQ file, from the window's RAW TEXT (replaces needletail's record parsing for
 * this loop, src/cmd_extract.rs:281-282,321-328): text[0, n_text) starts at a record start and ends behind a whole
 * record (n_text < 4 GiB).  The bytes are uploaded as they are (fastest from memory of mk_host_alloc), the records are
 * indexed and their sequence lines gathered on the device, then the loop body of mk_extract_single runs.
 * Outputs: *n_rec records; rec_start[i] = offset of record i's '@' (rec_start[n_rec] = n_text; room for rec_cap + 1);
 * keep / rows / counters / pattern_hit_counts as mk_extract_single (row.rec indexes the window's records).
 * Only plain 4-line FASTQ is taken ('@' line, sequence, '+' line, quality of the same length; LF or CRLF; no blank
 * lines).  Anything else sets *status = 1 and produces nothing: the caller parses that window with its own reader
 * (which also words the reference's parse errors).  More than rec_cap records: MK_E_CAPACITY, *n_rec = required. */
int mk_extract_fastq_text(mk_matcher *m, const uint8_t *text, uint64_t n_text, int logging, int invert, uint64_t rec_cap,
                          uint64_t *n_rec, uint64_t *rec_start, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows,
                          mk_counters *counters, uint32_t *pattern_hit_counts, uint32_t *status);
/* Optional overlap for a host that walks a file window by window: starts the upload of the NEXT window (page-locked
 * memory) on a stream of its own and returns; the mk_extract_fastq_text call that is then given the same pointer and
 * size finds its text on the device already.  May be called from another host thread while a call on the handle is in
 * progress, but must have returned before the call that consumes it starts; any other window simply uploads itself. */
int mk_upload_text_ahead(mk_matcher *m, const uint8_t *text, uint64_t n_text);
/* page-locked host memory for buffers that are uploaded (text windows, record batches): the DMA engines read it
 * directly, pageable memory is staged through a bounce buffer by one runtime thread.  Release with mk_host_free. */
int mk_host_alloc(size_t bytes, void **out);
void mk_host_free(void *p);
/* Where the last mk_extract_single / mk_tag_records call on this handle spent its time, in milliseconds:
 * ms[0] upload of the records (host -> device), ms[1] device work (scan, emission order, log rows, per-pattern
 * counts, per-record pattern sets -- all kernels), ms[2] download of the results, ms[3] host loops (flags -> keep,
 * adding counts).  Both calls run on the device from end to end; the host only copies and decides keep. */
int mk_matcher_batch_times(const mk_matcher *m, float ms[4]);

/* tag value, src/cmd_tag.rs:470-490: found patterns merged with an existing tag value
 * (split on ','), sort_unstable, dedup, join(",").  Writes a NUL-terminated string into
 * out (cap bytes); returns MK_E_CAPACITY with *out_len = required (excl. NUL) if too small. */
int mk_tag_value(const mk_matcher *m, const uint32_t *found_pat, uint64_t n_found, const char *existing, char *out,
                 size_t cap, size_t *out_len);

/* ------------------------------------------------------------------------------------
 * Synthetic workload generator (device; used by bench.py and the full-size parity tests)
 * Fills d_seq[0..n_rec*read_len) with uniform ACGT from a counter-based generator
 * (value at byte i depends only on (seed, i)), writes d_seq_off[i] = i*read_len, and plants
 * pattern (i * 2654435761 mod n_pat) of the matcher at a hashed offset in every record i
 * with hash(seed, i) % plant_every == 0 (plant_every == 0: none).
 * mk_synth_reads_host produces the identical bytes on the CPU for record range [rec0, rec0+n).
 * ---------------------------------------------------------------------------------- */
int mk_synth_reads_device(mk_matcher *m, uint64_t seed, uint64_t n_rec, uint32_t read_len, uint32_t plant_every,
                          void *d_seq, void *d_seq_off, void *stream);
int mk_synth_reads_host(const mk_matcher *m, uint64_t seed, uint64_t rec0, uint64_t n_rec, uint32_t read_len,
                        uint32_t plant_every, uint8_t *seq, uint64_t *seq_off);
/* records [rec0, rec0 + n_rec) of the same synthetic job (a rank's shard of a strong-scaled run):
 * d_seq_off is relative to the shard; rec0 * read_len must be a multiple of 32 */
int mk_synth_reads_device_range(mk_matcher *m, uint64_t seed, uint64_t rec0, uint64_t n_rec, uint32_t read_len,
                                uint32_t plant_every, void *d_seq, void *d_seq_off, void *stream);

/* ------------------------------------------------------------------------------------
 * Multi-GPU: the counter reduction (the path's only collective)
 * Records shard across GPUs with no data-path exchange; at the end of a job the per-GPU
 * vectors uint64[n_pat + MK_NUM_SUMMARY] (pattern_hit_counts | the scalars of
 * src/cmd_extract.rs:285-290, src/cmd_tag.rs:360-364) are summed with RCCL ncclAllReduce
 * over xGMI.  librccl is bound at run time; without it these calls return MK_E_RCCL.
 *
 * One process, one handle per GPU:  mk_reduce_counters(handles, n, vectors, len, host_sum)
 * sums d_counters[0..n) element-wise IN PLACE (every vector holds the sum on return) and
 * copies it to host_sum (may be NULL).  d_counters[i] is a device pointer on handles[i]'s
 * device.  Handles that share a device are added on that device first; the all-reduce runs
 * over the distinct devices.  Blocking: waits for all work enqueued on those devices.
 * Failure is total: if ncclCommInitAll fails nothing is cached; if the grouped all-reduce fails the communicators
 * of that device list are destroyed and the next call creates them again (MK_E_RCCL either way; the vectors of
 * handles that share a device may already hold their device-local sum).
 *
 * One process per GPU:  rank 0 calls mk_comm_unique_id and hands the id bytes to the other
 * ranks (file, MPI, torch.distributed, ...); every rank calls mk_comm_init (collective), then
 * mk_comm_reduce_counters enqueues the in-place all-reduce on `stream`.
 * ---------------------------------------------------------------------------------- */
#define MK_COMM_ID_BYTES 128
int mk_reduce_counters(mk_matcher *const *per_gpu, int n, void *const *d_counters, size_t len, uint64_t *host_sum);
/* (v6) creates the communicators mk_reduce_counters will use for these handles' devices and keeps them -- RCCL's set-up takes
 * seconds, the reduction itself microseconds: call it from a thread of its own when the job starts.  Nothing is synchronised,
 * nothing reduced; mk_reduce_counters works without it. */
int mk_reduce_prepare(mk_matcher *const *per_gpu, int n);
/* MK_OK if librccl could be bound in this process (ranks other than 0 can check before the collective init) */
int mk_comm_available(void);
int mk_comm_unique_id(uint8_t id[MK_COMM_ID_BYTES]);
int mk_comm_init(mk_matcher *m, const uint8_t id[MK_COMM_ID_BYTES], int rank, int n_ranks);
int mk_comm_reduce_counters(mk_matcher *m, void *d_counters, size_t len, void *stream);
/* ranks of the handle's communicator as RCCL reports them (ncclCommCount) */
int mk_comm_size(const mk_matcher *m, int *n_ranks);
int mk_comm_destroy(mk_matcher *m);

/* -------------------------------------------------------------------------------------
 * BGZF codec on the device (v5) -- the (de)compression either side of the hot path for BAM and bgzip'ed FASTA/FASTQ.
 * Replaces what the reference gets from `bam 0.1.4` / flate2 on `tag`'s reader and writer threads
 * (src/cmd_tag.rs:254-271 writer, :503-615 reader + record loop) and from needletail's gzip reader
 * (src/cmd_extract.rs:281): BGZF (SAM specification 4.1) is a series of independent gzip members of at most 64 KiB,
 * so members map to waves (deflate) and lanes (inflate).  A handle owns a stream and its device buffers, is bound to
 * one device and serialises its calls; independent of any mk_matcher.
 *
 * mk_bgzf_deflate: in[0, n) -> ceil(n / block_bytes) complete members back to back in out (block_bytes <= 65280;
 * 0 = 65280, what htslib writes).  The members inflate to `in` exactly, with correct CRC-32 / ISIZE / BSIZE; their
 * compressed bytes are this library's own parse (not zlib's).  No EOF marker is appended (mk_bgzf_eof gives its 28
 * bytes).  out_cap >= mk_bgzf_deflate_bound(n, block_bytes), else MK_E_CAPACITY with *out_len = that bound.
 *
 * mk_bgzf_inflate: the n_members members the caller found in in[0, n_in) by walking the BSIZE chain -> their text at
 * out + out_off.  Every member is checked: stream errors, ISIZE and CRC-32 (on the device).  A damaged member:
 * MK_E_CORRUPT, *bad_member = the first one, its status word in mk_last_error().  The call overwrites the span of out
 * its members cover (min out_off .. max out_off + isize: gaps between members included), nothing outside it.
 * Bytes inside data_len behind the stream's final block are left unread, as zlib leaves them (unused_data): the text is given.
 * --------------------------------------------------------------------------------------- */
typedef struct mk_codec mk_codec;
typedef struct mk_bgzf_member {
    uint64_t data_off; /* first byte of the raw DEFLATE stream (member start + 12 + XLEN) */
    uint64_t out_off;  /* where the member's text goes */
    uint32_t data_len; /* BSIZE + 1 - XLEN - 20 */
    uint32_t isize;    /* the trailer's ISIZE (<= 65536) */
    uint32_t crc;      /* the trailer's CRC-32 */
    uint32_t reserved;
} mk_bgzf_member;
int mk_codec_create(int device, mk_codec **out);
void mk_codec_destroy(mk_codec *c);
uint64_t mk_bgzf_deflate_bound(uint64_t n, uint32_t block_bytes);
int mk_bgzf_deflate(mk_codec *c, const uint8_t *in, uint64_t n, uint32_t block_bytes, uint8_t *out, uint64_t out_cap, uint64_t *out_len);
/* the same for text that lies in several pieces (a writer's per-thread record buffers): the members are those of the
 * pieces' concatenation, which exists on the device only -- the host never copies the pieces together */
int mk_bgzf_deflate_pieces(mk_codec *c, const uint8_t *const *pieces, const uint64_t *sizes, uint64_t n_pieces, uint32_t block_bytes,
                           uint8_t *out, uint64_t out_cap, uint64_t *out_len);
int mk_bgzf_inflate(mk_codec *c, const uint8_t *in, uint64_t n_in, const mk_bgzf_member *members, uint64_t n_members, uint8_t *out,
                    uint64_t out_cap, uint64_t *bad_member);
/* mk_extract_fastq_text for a window of a bgzip'ed FASTQ: the members are uploaded as they are (a fifth of the text) and
 * inflated on the device STRAIGHT INTO the text buffer the ingest kernels read -- the text is never uploaded.  The window's
 * text = head[0, n_head) (the unfinished record the previous window ended with) followed by the members' text
 * (members[i].out_off = running sum of ISIZE from 0).  [0, io->n_used) of it are whole 4-line records and are what is indexed
 * and scanned, exactly as mk_extract_fastq_text does (same outputs, same *status = 1 for text that is not plain FASTQ: the
 * caller's own reader then takes the window); the rest, [io->n_used, io->n_text), is the next call's head.  What comes back
 * of the text is the caller's choice (mk_window_text):
 *   io->text != NULL: all of it, text[0, n_text) (text_cap >= n_head + sum of ISIZE, else MK_E_CAPACITY);
 *   io->text == NULL: only io->tail[0, n_tail) = the next head, and io->kept[0, n_kept_bytes) = the text of the KEPT records
 *     (keep[r] != 0), gathered on the device, back to back in record order -- record r's text is the next
 *     rec_start[r + 1] - rec_start[r] bytes of it.  (With logging AND invert the rows name records that are not kept: use
 *     the whole-text mode then.)  kept_cap too small: MK_E_CAPACITY with n_kept_bytes = the need; the last whole record must
 *     end within the window's last MiB, else *status = 1.
 * last != 0: no text follows, a final line without a line end counts, an unfinished record is a refusal (*status = 1).
 * A damaged member: MK_E_CORRUPT.  The codec handle lends its device buffers and must be on the matcher's device.
 * (The reference gets these records from needletail's gzip reader, src/cmd_extract.rs:281-282,321-328.) */
typedef struct mk_window_text {
    uint8_t *text;     /* in: whole-text mode buffer or NULL */
    uint64_t text_cap;
    uint8_t *tail;     /* in (text == NULL): the unfinished record at the window's end goes here */
    uint64_t tail_cap;
    uint8_t *kept;     /* in (text == NULL): the kept records' text goes here */
    uint64_t kept_cap;
    uint64_t n_text, n_used, n_tail, n_kept_bytes; /* out */
} mk_window_text;
int mk_extract_fastq_bgzf(mk_matcher *m, mk_codec *codec, const uint8_t *head, uint64_t n_head, const uint8_t *bgzf, uint64_t n_bgzf,
                          const mk_bgzf_member *members, uint64_t n_members, int last, mk_window_text *io, int logging, int invert,
                          uint64_t rec_cap, uint64_t *n_rec, uint64_t *rec_start, uint8_t *keep, mk_row *rows, uint64_t rows_cap,
                          uint64_t *n_rows, mk_counters *c, uint32_t *pattern_hit_counts, uint32_t *status);
/* -------------------------------------------------------------------------------------
 * Text windows of one or two input files (v6) -- the general form of mk_extract_fastq_text / mk_extract_fastq_bgzf: FASTQ or
 * FASTA, one input (the loop of src/cmd_extract.rs:321-406) or two (paired: :463-612), plain text or BGZF members, with heads.
 * Replaces needletail's parse_fastx_file + record.seq() for these loops (src/cmd_extract.rs:281-282, 412-418, 321-328, 463-468).
 *
 * A source's window text = head[0, n_head) ++ body, the body being text[0, n_text) (uploaded; fastest from mk_host_alloc memory;
 * mk_upload_text_ahead of the same pointer and size beforehand overlaps the copy with the previous window) or the text of
 * members[0, n_members) of bgzf[0, n_bgzf) (inflated on the device, never uploaded; needs `codec` on the matcher's device), or
 * device_text[0, n_device_text) (text that is on the device already: a gzip file inflated there by mk_gzip_inflate_device).  The
 * window starts at a record start.  ends_at_record != 0: its end is a record end (the end of the input, or a place the caller
 * chose); == 0: it may end anywhere -- the unfinished record stays behind as the tail.  The head is how a caller hands the
 * previous window's tail back in.
 * The records are indexed on the device: FASTQ -- '@' line, sequence, '+' line, quality of the same length, LF or CRLF, no blank
 * lines; FASTA -- '>' header lines, every other line sequence, which reaches the matcher without its '\n' / '\r' bytes
 * (record.seq(); a hit may span a line break: tests/fixtures/extract/fixed-width.log:8).  Anything else sets *status = 1 and
 * produces nothing: the caller's own reader takes that window (and words the reference's parse errors).
 * *n_rec = the records (two sources: PAIRS, record i of one with record i of the other) the call has processed = the smallest
 * number of whole records any source holds; per source: n_rec_seen = whole records it held, rec_start[0 .. *n_rec] = their offsets
 * in the window text (rec_start[*n_rec] = n_used, the bytes the processed records take), n_tail = n_window - n_used.  Outputs
 * keep / rows / counters / pattern_hit_counts: as mk_extract_single, resp. mk_extract_paired (row.rec = index in the window,
 * row.file = source).  What comes back of the text is the caller's choice, per source:
 *   tail (tail_cap):  the text behind the processed records, the next window's head     (MK_E_CAPACITY: n_tail = the need)
 *   kept (kept_cap):  the text of the KEPT records back to back, record r's being rec_start[r + 1] - rec_start[r] bytes -- for
 *                     callers that do not hold the text themselves (BGZF bodies)          (MK_E_CAPACITY: n_kept_bytes = the need)
 *   all  (all_cap):   the whole window text (logging with invert: rows name records that are not kept)
 * A damaged BGZF member: MK_E_CORRUPT.  More than rec_cap records: MK_E_CAPACITY with *n_rec = the need.
 * A call reports the first thing that does not fit, in this order: rec_cap (nothing is scanned, nothing else stated); per source
 * tail, then all; kept (of every source at once); rows (*n_rows is stated only by a call whose texts all fit).  A caller that grows what
 * the call names and calls again with fresh counters is done after at most one call per output.
 * --------------------------------------------------------------------------------------- */
#define MK_TEXT_FASTQ 0
#define MK_TEXT_FASTA 1
typedef struct mk_window_source {
    /* in */
    const uint8_t *head;
    uint64_t n_head;
    const uint8_t *text;
    uint64_t n_text;
    const uint8_t *bgzf;
    uint64_t n_bgzf;
    const mk_bgzf_member *members; /* out_off = running sum of ISIZE from 0 */
    uint64_t n_members;
    const void *device_text; /* body that already lies on the matcher's device (a range of mk_gzip_text_device's text), or NULL */
    uint64_t n_device_text;
    uint32_t ends_at_record;
    uint32_t reserved;
    uint64_t *rec_start; /* room for rec_cap + 1, or NULL */
    uint8_t *tail;
    uint64_t tail_cap;
    uint8_t *kept;
    uint64_t kept_cap;
    uint8_t *all;
    uint64_t all_cap;
    /* out */
    uint64_t n_window, n_used, n_tail, n_kept_bytes, n_rec_seen;
} mk_window_source;
int mk_extract_window(mk_matcher *m, mk_codec *codec, uint32_t format, uint32_t n_sources, mk_window_source *sources, int logging, int invert,
                      uint64_t rec_cap, uint64_t *n_rec, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *counters,
                      uint32_t *pattern_hit_counts, uint32_t *status);

/* -------------------------------------------------------------------------------------
 * A text window that may START ANYWHERE (v7 addition) -- mk_extract_window for a window whose first byte may lie inside a record: a
 * range of BGZF members that begins at a member boundary, a slice of a plain file.  The call finds a record start itself, hands back
 * the text in front of it and processes the records from there; windows of one file can then run side by side, on any device, and
 * the text between two of them -- the tail of window k - 1 ++ the front of window k -- goes through one small mk_extract_window call.
 * Same arguments, outputs and body as mk_extract_window, plus `fronts` (one mk_window_front: n_sources must be 1 -- mate i of one
 * file of a pair has no index in the other -- and n_head 0; anything else is MK_E_INVALID_ARG, raised before any device use).
 *
 * THE START RULE, on the lines of the window text (line 0 begins at byte 0, a '\n' ends a line; a line is COMPLETE when the text
 * holds its '\n'):
 *   FASTQ  the smallest line j >= 1 such that the record shape holds at j AND at j + 4, all eight lines complete.  The shape at j is
 *          mk_extract_window's: line j begins with '@' and holds at least three bytes with its '\n'; line j + 2 begins with '+';
 *          lines j + 1 and j + 3 have one length, a '\r' in front of the '\n' counted as part of the line end.
 *   FASTA  the smallest line j >= 1 whose first byte is '>' (a line that begins inside the text; it need not be complete).
 * Line 0 is never taken: whether byte 0 follows a line end is not known to the call.
 * out: front[0, n_front) = the text in front of line j; the records are indexed from byte n_front on as by mk_extract_window, and
 *      rec_start[] (rec_start[0] = n_front), n_used and n_tail stay offsets in the WHOLE window text.
 * *status = 2: no start was found (fewer than nine complete lines, one record longer than the window, an empty window): nothing is
 *      produced, n_front = n_window and `front` is not written.  *status = 1: as mk_extract_window, n_front is stated.
 * front_cap too small: MK_E_CAPACITY with n_front = the need; in the order of "the first thing that does not fit" it stands behind
 *      rec_cap and in front of tail.
 *
 * THE FOUND START IS A GUESS, and the caller proves it.  A FASTA start is always true: every line that begins with '>' begins a
 * record.  A FASTQ quality line may begin with '@', and texts exist in which the shape holds twice at lines that begin no record.
 * The proof is the seam call: mk_extract_window on tail(k - 1) ++ front(k) with ends_at_record = 1.  By induction tail(k - 1)
 * begins at a true record start (window 0 begins the file; a window that begins at a true start counts whole records, so what it
 * leaves behind begins at one).  In a well-formed file every record is four lines, so the lines from that true start to the found
 * start are a multiple of four, every group of which has the shape, if and only if the found start is a record start: the seam call
 * returns *status = 0 and n_used = n_window exactly then.  Anything else (status != 0, n_used != n_window, or status 2 from the open
 * call) disproves the guess; the caller then runs window k the chained way, head = tail(k - 1), and drops the open call's results.
 * A file that is not well formed fails the seam or the window behind it and ends up on the same chained path, which words the error.
 * --------------------------------------------------------------------------------------- */
typedef struct mk_window_front {
    uint8_t *front;     /* in: where the text in front of the found start goes */
    uint64_t front_cap;
    uint64_t n_front;   /* out */
} mk_window_front;
int mk_extract_window_open(mk_matcher *m, mk_codec *codec, uint32_t format, uint32_t n_sources, mk_window_source *sources, int logging, int invert,
                           uint64_t rec_cap, uint64_t *n_rec, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *counters,
                           uint32_t *pattern_hit_counts, uint32_t *status, mk_window_front *fronts);

/* -------------------------------------------------------------------------------------
 * BGZF members that end at record ends (v7 addition) -- the output side of `extract -z`: the kept records are deflated on the
 * device, and every member is a FASTQ / FASTA fragment that parses on its own, so a reader that splits its work at member boundaries needs
 * no head / tail chain.  (mk_bgzf_deflate cuts its text every block_bytes: a record may straddle two members.  The reference writes
 * plain text only: src/cmd_extract.rs:297-318.)
 *
 * THE CUT RULE.  A text of T bytes whose records end at e[0] <= e[1] <= ... <= e[n-1] = T.  G = 49152 (the grid step), L = 65280 (the
 * most text a member holds).  For k = 1 .. ceil(T / G) - 1, x = k * G: e* = the smallest record end >= x; snap(x) = e* if
 * e* < x + (L - G), else x (a raw cut inside a record longer than L - G = 16128 bytes: a chromosome).  The cuts are 0, the distinct
 * snap(k * G) in increasing order, and T; member i is the text between cut i and cut i + 1.  Consecutive cuts are more than 0 and at
 * most L bytes apart; a grid point costs one binary search, no walk over the records; T = 0 gives one cut (0) and no member.  Since
 * snap(x) lies in [x, x + (L - G)) and L - G <= G, two grid points never snap to the same place: the only cut that can coincide with
 * another is the last grid point's with T.  A text that starts and ends at record ends gives members that do: concatenated outputs
 * of several calls stay record-aligned.
 *
 * mk_bgzf_record_cuts (host code, no device): the rule -> cut[0, *n_cuts), at most ceil(T / G) + 1 of them.  rec_end must not
 * decrease (MK_E_INVALID_ARG); cap too small: MK_E_CAPACITY with *n_cuts = the need.
 * mk_bgzf_deflate_records: text[0, n) with rec_end[n_rec - 1] = n -> the members of the rule back to back in out, cut and deflated
 * on the device (the cut kernel is checked against mk_bgzf_record_cuts by the tests).  *out_len = their bytes, *n_members how many;
 * out_cap too small: MK_E_CAPACITY with *out_len = the exact need; out then holds nothing of use (the members of the device passes
 * that still fitted may have been written to it).  No EOF member is appended.  Honours
 * mk_codec_set_pass_limits (deflate_members).
 * mk_codec_cut_times: members and milliseconds (cut kernel; CRC-32 + deflate + pack; download) of the handle's last
 * mk_bgzf_deflate_records -- mk_codec_times reports the first two as one number, a caller that weighs the cut kernel against the deflate
 * launch (`extract -z` under MERKURIO_TIMING) needs them apart.
 * --------------------------------------------------------------------------------------- */
#define MK_BGZF_CUT_GRID 49152u
#define MK_BGZF_MEMBER_TEXT_MAX 65280u
int mk_bgzf_record_cuts(const uint64_t *rec_end, uint64_t n_rec, uint64_t *cut, uint64_t cap, uint64_t *n_cuts);
int mk_bgzf_deflate_records(mk_codec *c, const uint8_t *text, uint64_t n, const uint64_t *rec_end, uint64_t n_rec, uint8_t *out, uint64_t out_cap,
                            uint64_t *out_len, uint64_t *n_members);
int mk_codec_cut_times(const mk_codec *c, uint64_t *n_members, float ms[3]);

/* -------------------------------------------------------------------------------------
 * A window's kept records as BGZF members (v7 addition) -- mk_extract_window whose kept records leave the device deflated: they
 * are packed in their WRITTEN form on the device, cut by the rule above and deflated where they lie; only the members come down.
 * Same arguments and outputs as mk_extract_window, plus one mk_window_members per source (paired: each source has members of its
 * own).  Both entry points share one body.  `codec` is required and must be on the matcher's device (MK_E_INVALID_ARG); a source's
 * `kept` buffer belongs to mk_extract_window (MK_E_INVALID_ARG here); logging with invert is MK_E_INVALID_ARG, because rows then
 * name records that are not kept (use mk_extract_window's `all`).
 *
 * THE WRITTEN FORM.  The writer re-emits a kept record's lines (the reference's record.write(_, None), src/cmd_extract.rs:297-318),
 * it does not copy its stored bytes.  eol = the line end of the record's HEADER line, "\r\n" or "\n".
 *   FASTQ  '@' id eol sequence eol '+' eol quality eol     -- id, sequence, quality: the lines without their line ends; the '+'
 *          line loses whatever it repeats; a last record without a line end gains one.  Every record the index accepts is written.
 *   FASTA  the record's bytes up to its final line end, then eol -- the final line end becomes the header's kind, a last record
 *          without one gains it; inner line ends stay as stored.  A kept FASTA record that this does not describe (no sequence
 *          line, blank lines or a lone '\r' at its end) makes the call refuse member output for the window: *status = 2, every
 *          mk_window_members reports 0 bytes (of two sources, the buffers of the one in front of the refusing one may have been
 *          written to; nothing in them is of use), and the caller calls mk_extract_window for that window (with fresh counters).
 * The record ends of the written text are the cut rule's e[]: every member starts at a record start, unless a record is longer
 * than 16128 bytes.  No EOF member is written.  Nothing kept: 0 members, 0 bytes.
 *
 * in:  members / members_cap   where the members go, back to back
 *      ids / ids_cap / id_end  with logging: the ids of the kept records (header lines without marker and line end) back to back
 *                              in record order, id_end[q] = where the q-th kept record's id ends (room for rec_cap entries); the
 *                              log rows then need no text.  May be NULL / 0 without logging.
 *      text_below              > 0: a source whose written text is shorter than this many bytes comes back as that TEXT in
 *                              `members` (as_text = 1, n_members = 0) -- for a caller that gathers small windows with their
 *                              neighbours before it compresses.  0: always members.
 * out: n_member_bytes (bytes in `members`: of the members, or of the text when as_text), n_members, n_written (bytes of the
 *      written text), n_kept (records), n_id_bytes, as_text, written_ms (the two written-form kernels, select + gather, by stream
 *      events; mk_codec_cut_times reports the cut, deflate and download of the codec handle's last such call, summed over sources).
 * members_cap too small: MK_E_CAPACITY with n_member_bytes = the exact need; ids_cap too small: MK_E_CAPACITY with n_id_bytes = the
 * need.  In mk_extract_window's order of "the first thing that does not fit" these two stand where `kept` stands: after tail and
 * all, of every source at once, before rows.
 * --------------------------------------------------------------------------------------- */
typedef struct mk_window_members {
    /* in */
    uint8_t *members;
    uint64_t members_cap;
    uint8_t *ids;
    uint64_t ids_cap;
    uint64_t *id_end;
    uint64_t text_below;
    /* out */
    uint64_t n_member_bytes, n_members, n_written, n_kept, n_id_bytes;
    uint32_t as_text;
    float written_ms;
} mk_window_members;
int mk_extract_window_members(mk_matcher *m, mk_codec *codec, uint32_t format, uint32_t n_sources, mk_window_source *sources,
                              mk_window_members *members, int logging, int invert, uint64_t rec_cap, uint64_t *n_rec, uint8_t *keep, mk_row *rows,
                              uint64_t rows_cap, uint64_t *n_rows, mk_counters *counters, uint32_t *pattern_hit_counts, uint32_t *status);

/* -------------------------------------------------------------------------------------
 * A window's kept records as zstd frames (v7 addition) -- the output side of `extract --zstd-output`: mk_extract_window_members with the
 * other codec.  Same arguments and outputs, the same mk_window_members per source (paired: each source has frames of its own), the same
 * body: only the step that turns the packed written text into compressed bytes differs.  In the struct, `members` holds the FRAMES back
 * to back, n_member_bytes their bytes and n_members how many there are.
 *
 * The frames are those of mk_zstd_deflate_records (below) applied to the window's written text (THE WRITTEN FORM, above) with the
 * written record ends: cut by the rule of mk_zstd_record_cuts -- grid MK_ZSTD_CUT_GRID = 114688, at most MK_ZSTD_FRAME_TEXT_MAX = 131072
 * bytes of text per frame, so every frame starts at a record start unless a record is longer than 16384 bytes --, each a
 * self-contained frame of one block with a content checksum, byte for byte what that call makes of the same text and ends.  Cuts start
 * again with every window and every source.  Nothing kept: 0 frames, 0 bytes (the empty frame that makes an empty job's output a
 * valid .zst is the caller's business).
 *
 * text_below, ids / ids_cap / id_end, n_written, n_kept, as_text and written_ms: as for members.  *status = 2 for a kept FASTA record
 * that the written form does not describe: every mk_window_members reports 0 bytes, as for members.  members_cap too small:
 * MK_E_CAPACITY with n_member_bytes = the exact need; ids_cap too small: MK_E_CAPACITY with n_id_bytes = the need; both stand where they
 * stand for members in the order of "the first thing that does not fit".
 * MK_E_INVALID_ARG: no codec; a codec on another device than the matcher's; a source with a `kept` buffer; logging with invert; a
 * codec handle with an open stream (mk_gzip_stream_*, mk_bzip2_stream_*, mk_zstd_stream_*, mk_xz_stream_*), as for
 * mk_zstd_deflate_records.
 * mk_zstd_deflate_info reports, for the codec handle's last such call, the frames, the block kinds and the milliseconds SUMMED over the
 * sources (ms[0], upload, is 0: nothing goes up) -- what mk_codec_cut_times is for members.
 * --------------------------------------------------------------------------------------- */
int mk_extract_window_frames(mk_matcher *m, mk_codec *codec, uint32_t format, uint32_t n_sources, mk_window_source *sources,
                             mk_window_members *frames, int logging, int invert, uint64_t rec_cap, uint64_t *n_rec, uint8_t *keep, mk_row *rows,
                             uint64_t rows_cap, uint64_t *n_rows, mk_counters *counters, uint32_t *pattern_hit_counts, uint32_t *status);

/* -------------------------------------------------------------------------------------
 * A gzip file inflated in parallel on the device (v6: one member; v7: a chain of members) -- a .fastq.gz / .fasta.gz as plain gzip (or pigz, or zlib) writes it: ONE
 * DEFLATE stream of thousands of blocks, which zlib can only walk from the front.  Replaces needletail's gzip reader under
 * `merkurio extract` (src/cmd_extract.rs:281-282) for such files.  The stream is cut where block starts can be FOUND (a dynamic
 * block's header is a pattern almost no bit position satisfies; a candidate is confirmed by decoding its block and meeting another
 * header behind it), the pieces are decoded side by side into 16-bit symbols -- bytes, or place-holders for the text in front of the
 * piece that a match reached into --, the place-holders are resolved piece by piece, and the text is checked against the member's
 * CRC-32 and ISIZE (merkurio_amd/csrc/codec/gzip_segments.hpp).
 * gz[0, n) = the whole member.  *taken = 1: the text lies on the codec's device, *text_bytes long, until the next call or
 * mk_gzip_text_release; read it with mk_gzip_text_read (host copy of a range) or hand windows of it to mk_extract_window
 * (mk_window_source::device_text).  *taken = 0: not a file for this path -- several members (mk_gzip_members_inflate_device takes
 * those), a stream that ends in front of its trailer, a stream without findable block starts
 * where they are needed, a piece that does not meet its neighbour, an unusually compressible stream the buffers do not hold, a
 * CRC-32 / ISIZE that does not match --: nothing is reported as an error, the caller inflates the file with zlib (which then also
 * words what is wrong with a damaged one).
 * --------------------------------------------------------------------------------------- */
int mk_gzip_inflate_device(mk_codec *c, const uint8_t *gz, uint64_t n, uint64_t *text_bytes, uint32_t *taken);
int mk_gzip_text_read(mk_codec *c, uint64_t offset, uint8_t *out, uint64_t len);
const void *mk_gzip_text_device(const mk_codec *c, uint64_t *text_bytes);
int mk_gzip_text_release(mk_codec *c);
/* pieces of the last mk_gzip_inflate_device / mk_gzip_members_inflate_device and its phases in milliseconds: upload, block search,
 * pieces, resolution, CRC-32 */
int mk_gzip_info(const mk_codec *c, uint32_t *segments, float ms[5]);

/* (v7) A .bz2 file decoded on the device, one wave per block (merkurio_amd/csrc/codec/bzip2_inflate.hip, bzip2_serial.hpp) -- what
 * `merkurio extract` reads through needletail's bzip2 reader (src/cmd_extract.rs:281).  bz[0, n) is the whole file, which may hold
 * several streams (pbzip2 output, `cat a.bz2 b.bz2`).  Every bit offset is tested on the device for the block magic 0x314159265359
 * and the end-of-stream magic 0x177245385090; the host walks the sorted hits: "BZh" + level at byte 0, the first magic at bit 32,
 * every block decoded from its magic must END exactly on the next magic of the table (the proof of a guessed start), behind an end
 * magic and the stream's CRC comes padding to the byte, then the file's end or another "BZh" + level.  A block: header, code tables,
 * Huffman symbols + zero runs + move-to-front on one wave, the inverse BWT vector by a counting sort across the wave, the walk of
 * the vector on one lane, lengths, an offsets scan, the text written at each block's offset, bzip2's CRC-32 (polynomial 0x04c11db7,
 * first bit on top) of every block in 64 folded pieces, the stream CRC folded on the host.  Blocks are decoded in passes whose
 * scratch (4.5 bytes per symbol) is bounded: by the free memory, or by mk_codec_set_bzip2_pass_blocks (test hook; 0 = default;
 * results do not depend on it).
 * *taken = 1 only when proved blocks and streams cover bz[0, n) with nothing left over and every block and stream CRC agrees: the
 * text of all streams then lies back to back where mk_gzip_inflate_device leaves its text (mk_gzip_text_read / _device / _release,
 * mk_window_source::device_text), *n_blocks says how many blocks it came from (an empty stream: 0 blocks, 0 bytes).  *taken = 0
 * (MK_OK, nothing else touched) means the caller runs libbz2, which also words the error: a `randomised` block, origPtr >= the
 * block's symbols, nGroups outside 2..6, nSelectors 0 or above 18 002, a selector >= nGroups, a code length outside 1..20, a code
 * under which a symbol does not decode (libbz2's own test of a code), more symbols than level x 100 000, a block that ends inside a
 * run, data that ends early, a table of magics that does not chain, trailing bytes, a wrong CRC, text plus scratch beyond half of
 * the free device memory, any device error.  With a gzip or bzip2 stream open on the handle: MK_E_INVALID_ARG.  Everything here is
 * sized by the file; a larger file: mk_bzip2_stream_*.
 * mk_bzip2_info: blocks of the last call and its phases in milliseconds: upload, marker search, block decode (symbols + vector),
 * text (walk + expansion), CRC. */
int mk_bzip2_inflate_device(mk_codec *c, const uint8_t *bz, uint64_t n, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_blocks);
int mk_bzip2_info(const mk_codec *c, uint32_t *blocks, float ms[5]);
int mk_codec_set_bzip2_pass_blocks(mk_codec *c, uint64_t blocks);

/* (an addition to v7; `merkurio extract --device-zstd`) A .zst file decoded on the device, one wave per block (merkurio_amd/csrc/codec/zstd_inflate.hip, zstd_serial.hpp,
 * zstd_plan.hpp) -- what `merkurio extract` reads through needletail's zstd reader (src/cmd_extract.rs:281).  zs[0, n) is the whole
 * file: Zstandard frames (RFC 8878) and skippable frames back to back.  The host walks the frame headers and every block header, and
 * of a compressed block the literals and sequences headers; it names, for every table a block repeats, the bytes that describe it.
 * Then, a wave per block: the Huffman and FSE tables built in LDS and the literals and sequences decoded; two scans on the host (text
 * offsets, the three repeat offsets in front of every block, composed from each block's symbolic effect on them); the text written,
 * a match that reaches in front of its block leaving the text position it copies from; rounds of pointer doubling over those
 * positions, at most log2(blocks) + 2; and per frame that carries one the content checksum, XXH64 on the host over the text as it
 * is downloaded.
 * *taken = 1 only when frames, skippable ones included, cover zs[0, n) with nothing left over, every size agrees and every checksum
 * agrees: the text of all frames then lies back to back where mk_gzip_inflate_device leaves its text (mk_gzip_text_read / _device /
 * _release, mk_window_source::device_text), *n_blocks says how many blocks it came from (an empty frame: 0 blocks, 0 bytes).
 * *taken = 0 (MK_OK, nothing else touched) means the caller runs libzstd, which also words the error: a legacy or unknown magic, a
 * reserved bit in the frame header descriptor, a dictionary id other than 0, a window above 2^27 bytes, a block above min(window,
 * 128 KiB), a compressed block under 3 bytes or of 128 KiB and more, the Reserved block type, Huffman weights that do not sum to a power of two or need more than 11 bits, an FSE description
 * whose probabilities do not add up or whose accuracy log is out of range, Repeat or treeless with nothing to repeat, a bitstream
 * that does not end exactly at its first bit, more literals asked for than there are, an offset of zero, in front of the frame's first
 * byte or beyond the window, a block that regenerates more than 128 KiB, a content size or checksum that disagrees, trailing bytes that
 * start no frame, data that ends early, 4 GiB of text and more, more rounds than the cap, text plus scratch (8 bytes per text byte)
 * beyond half of the free device memory, any device error.  With a gzip or bzip2 stream open on the handle: MK_E_INVALID_ARG.
 * Everything here is sized by the file.
 * mk_zstd_info: blocks, frames and resolution rounds of the last call and its phases in milliseconds: upload, tables + entropy
 * decode, scans, execution, cross-block rounds, checksum. */
int mk_zstd_inflate_device(mk_codec *c, const uint8_t *zs, uint64_t n, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_blocks);
int mk_zstd_info(const mk_codec *c, uint32_t *blocks, uint32_t *frames, uint32_t *rounds, float ms[6]);

/* (an addition to v7; `merkurio extract --device-xz`) An .xz file decoded on the device, one wave per block (merkurio_amd/csrc/codec/xz_inflate.hip,
 * lzma_serial.hpp, xz_plan.hpp) -- what `merkurio extract` reads through needletail's xz reader (src/cmd_extract.rs:279-281).  xz[0, n)
 * is the whole file: streams (xz file format 1.0.4) and Stream Padding back to back.  The host walks it from its end: every stream's
 * footer, Index and header, then every Block Header; the Index states each block's stored size and text size, so every block's place
 * in the file and in the text is known before a bit is decoded.  Then, a wave per block: its LZMA2 chunks decoded to the block's
 * place in the text, the probabilities in LDS; and a wave per block for the stream's check, CRC-32 or CRC-64 (None costs nothing).
 * *taken = 1 only when streams and padding cover xz[0, n), every header, Index and footer is well-formed with its CRC-32 right, every
 * block's 0x00 control byte sits exactly at its stored end, its text has exactly the Index's length and its check matches: the text
 * of all blocks then lies back to back where mk_gzip_inflate_device leaves its text (mk_gzip_text_read / _device / _release,
 * mk_window_source::device_text), *n_blocks says how many blocks it came from (an empty stream: 0 blocks, 0 bytes).
 * *taken = 0 (MK_OK, nothing else touched) means the caller runs liblzma, which also words the error; mk_xz_info's status names why
 * (negative, as uint32_t; the codes are xz_plan.hpp's and lzma_serial.hpp's): every malformation of the container (magic, a CRC-32,
 * a non-minimal multi-byte integer, non-zero padding, sizes in a Block Header or the Backward Size that disagree with the Index,
 * trailing bytes, data that ends early) and of a block (a control byte 0x03-0x7F, a first chunk without dictionary reset, an LZMA
 * chunk without properties, lc + lp > 4, a first range-coder byte other than 0, a chunk whose stored bytes are not consumed exactly
 * or whose final code is not 0, text past a chunk's or the block's size, a distance in front of the block's first byte or beyond
 * the dictionary size, the end-of-payload marker, a check that does not match); and what is valid but not this path's: the SHA-256
 * check and reserved check ids, any filter chain other than one LZMA2 (BCJ, delta), a dictionary above 1.5 GiB, more than 2^20
 * blocks, text beyond half of the free device memory, any device error -- and a file whose LARGEST BLOCK's text times the spread K
 * exceeds its whole text: a block is one wave's serial decode, so a file of one huge block is liblzma's.  K defaults to 107
 * (ceil(2 x liblzma's rate on one host thread / one wave's rate), measured: profiles/e2e_unxz.txt); mk_codec_set_xz_spread sets it (0 = the default, 1 = every file is tried).  With a gzip, bzip2,
 * zstd or xz stream open on the handle: MK_E_INVALID_ARG.  Opt-in everywhere: nothing is claimed about speed.
 * mk_xz_info: blocks, streams and status of the last call, the text bytes of the file's largest block, and the phases in
 * milliseconds: upload, decode, check, the whole call. */
int mk_xz_inflate_device(mk_codec *c, const uint8_t *xz, uint64_t n, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_blocks);
int mk_xz_info(const mk_codec *c, uint32_t *blocks, uint32_t *streams, uint32_t *status, uint64_t *largest_block_text, float ms[4]);
int mk_codec_set_xz_spread(mk_codec *c, uint32_t spread);

/* (an addition to v7; `merkurio extract --xz-stream`) An .xz file of ANY size, decoded on the device window by window: nothing on the
 * device is sized by the file.  The contract is mk_zstd_stream_*'s.
 * mk_xz_stream_begin: xz[0, n) = the whole file (the caller's -- the mapped file -- until _end).  The container walk of
 * mk_xz_inflate_device runs once over it (footers, Indexes, stream headers, Block Headers: one header per block, no compressed
 * payload is read), and because the Index states every block's stored size and text size, ALL windows are planned here, before a bit
 * is decoded (merkurio_amd/csrc/codec/xz_chain.hpp).  The plan is greedy and deterministic: a window is the longest run of consecutive
 * blocks from the cursor whose text is at most the text cap T and whose compressed span -- from the first block's Block Header to
 * the end of the last block's check -- is at most window_bytes (0 = no bound on the span: bounded by the text cap only); one block at
 * the least, also where that block alone exceeds window_bytes.  A window may run across stream boundaries, Stream Padding and streams
 * of other check kinds; a stream without blocks makes no window and counts as closed with the blocks in front of it.  Blocks need
 * nothing from each other: no history and no table crosses a seam.
 * *taken = 0 (MK_OK, no stream is open; mk_xz_stream_info's status names why): everything mk_xz_inflate_device's walk refuses, under
 * the same codes; a block whose text alone exceeds T (kXzBlockOverCap, -33); the spread rule, generalised: K x the sum over the
 * windows of (that window's largest block's text) must not exceed the whole text (kXzSpread) -- a window costs as long as its
 * slowest block, so many small windows cost more than one large one, and with one window this is mk_xz_inflate_device's rule; K is
 * mk_codec_set_xz_spread's.  The rule ignores that a window may hold more blocks than the device has resident waves (a known
 * approximation, as in the one-shot call).  With 24 MiB blocks and K = 107 a window must hold about 2.5 GiB of text, which is why
 * window_bytes = 0 sets no bound of its own.  T is chosen from the free device memory: a sixth of it, so that two text buffers of T
 * and the largest window's upload and tables fit in half of what is free (checked against the plan: kXzTooLarge otherwise).  That
 * default is an UNMEASURED choice (profiles/e2e_unxz_windows.txt).  mk_codec_set_xz_text_cap sets T (test hook; 0 = default; results
 * do not depend on it).
 * mk_xz_stream_next uploads only the window's compressed span, walks the chunk headers of the window's blocks (the launch's LDS is
 * sized by this window's lc + lp), and launches the two kernels of mk_xz_inflate_device over the window's blocks, largest text first.
 * *state = 0: a window of text was produced, *text_bytes long (0 is possible: blocks without text): it is what mk_gzip_text_device /
 *             mk_gzip_text_read refer to, in one of two text buffers -- window w stays valid until the call that produces w + 2;
 *          1: end of file: every block of every window was proved as in the one-shot call -- the control byte 0x00 at the stored
 *             end, the Index's text length, the check; no text in this call;
 *          2: handed back (MK_OK): stats.status names the first block of this window that failed, or kXzTooLarge (no room), or
 *             kXzDevice (any device error).  No text comes from this window and nothing after it.  The windows delivered before it
 *             are a prefix of liblzma's text, in whole blocks: the caller's liblzma reads from the front and skips stats.text_bytes.
 * mk_xz_stream_end closes the stream and frees what it held (the two text buffers included).  mk_xz_stream_info takes the codec's
 * lock; without an open stream: the last stream's figures, a refusal at _begin included.  While an xz stream is open every one-shot
 * call and every other *_stream_begin return MK_E_INVALID_ARG -- and mk_xz_stream_begin does while another stream is --, and
 * mk_gzip_text_release ends the stream as mk_xz_stream_end does.  Opt-in everywhere: nothing is claimed about speed. */
typedef struct mk_xz_stream_stats {
    uint64_t windows;            /* windows of text produced */
    uint64_t streams;            /* streams whose blocks have all been delivered (all of them at state 1) */
    uint64_t blocks;             /* blocks delivered */
    uint64_t consumed_bytes;     /* compressed bytes in front of the next window (the file's size behind the last) */
    uint64_t text_bytes;         /* text bytes delivered so far */
    uint64_t planned_windows;    /* windows of the plan made at _begin */
    uint64_t largest_block_text; /* text bytes of the file's largest block */
    uint64_t peak_device_bytes;  /* most device memory the stream has held */
    int32_t status;              /* 0, or why _begin refused / a window was handed back (xz_plan.hpp, lzma_serial.hpp, xz_chain.hpp) */
    uint32_t reserved;
    float ms[4];                 /* summed over the windows: upload, decode, check, the whole of the calls */
} mk_xz_stream_stats;
int mk_xz_stream_begin(mk_codec *c, const uint8_t *xz, uint64_t n, uint64_t window_bytes, uint32_t *taken);
int mk_xz_stream_next(mk_codec *c, uint64_t *text_bytes, uint32_t *state);
int mk_xz_stream_info(const mk_codec *c, mk_xz_stream_stats *out);
int mk_xz_stream_end(mk_codec *c);
int mk_codec_set_xz_text_cap(mk_codec *c, uint64_t text_bytes);

/* (v7) The kept records of `extract` as a .zst file, compressed on the device (zstd_deflate.hip, a wave per frame): what
 * mk_bgzf_deflate_records is for BGZF.  The text is cut by the rule of mk_bgzf_record_cuts with two other constants: a cut is looked for at
 * every multiple of MK_ZSTD_CUT_GRID among the record ends of the next MK_ZSTD_FRAME_TEXT_MAX - MK_ZSTD_CUT_GRID bytes, so only a longer
 * record is cut inside.  Every piece becomes one frame that decodes on its own: magic, descriptor 0xA4 (Single_Segment,
 * Content_Checksum, 4-byte Frame_Content_Size), ONE block with Last_Block set, the low 32 bits of XXH64 (seed 0) of its text -- 16 bytes
 * plus the block.  The block is RLE where all bytes are equal, Raw where the compressed form is not smaller than the text, Compressed
 * otherwise.  Fixed choices of the writer: no match reaches in front of its block and there is no dictionary; offsets are always coded
 * as offset + 3 (no repeat-offset codes); literals are RLE for one distinct byte, Huffman-coded under a tree of direct 4-bit weights
 * (code lengths <= 11; one stream below 1024 literals, four from there on), and Raw where that does not shrink them or a byte above 128
 * occurs (FSE-coded weights are not written); each sequence table is RLE where one code occurs, else the cheaper of Predefined and
 * FSE_Compressed by an estimate from its histogram.  Any conforming decoder reads the frames; no ratio is promised.
 * mk_zstd_record_cuts (host code, no device): the rule -> cut[0, *n_cuts); the contract of mk_bgzf_record_cuts.
 * mk_zstd_deflate_bound: the bytes the frames of n bytes of text take at most.
 * mk_zstd_deflate_records: the contract of mk_bgzf_deflate_records -- rec_end[n_rec - 1] == n and non-decreasing ends, else
 * MK_E_INVALID_ARG; MK_E_CAPACITY with the exact need in *out_len; n == 0 writes nothing (0 frames); passes of
 * mk_codec_set_pass_limits' deflate_blocks frames; MK_E_INVALID_ARG while a stream is open on the handle.
 * mk_zstd_deflate_info: of the last such call (or the last mk_extract_window_frames with this handle: summed over its sources), the
 * frames, how many blocks were Raw / RLE / Compressed, and milliseconds of upload, cut + deflate + pack, download. */
#define MK_ZSTD_CUT_GRID 114688u
#define MK_ZSTD_FRAME_TEXT_MAX 131072u
int mk_zstd_record_cuts(const uint64_t *rec_end, uint64_t n_rec, uint64_t *cut, uint64_t cap, uint64_t *n_cuts);
uint64_t mk_zstd_deflate_bound(uint64_t n);   /* n + 16 * (n / MK_ZSTD_CUT_GRID + 2) */
int mk_zstd_deflate_records(mk_codec *c, const uint8_t *text, uint64_t n, const uint64_t *rec_end, uint64_t n_rec,
                            uint8_t *out, uint64_t out_cap, uint64_t *out_len, uint64_t *n_frames);
int mk_zstd_deflate_info(const mk_codec *c, uint64_t *n_frames, uint32_t kinds[3] /* raw, rle, compressed blocks */, float ms[3]);

/* (v7) A .bz2 file of ANY size, decoded on the device window by window: nothing on the device is sized by the file.  The contract is
 * mk_gzip_stream_*'s (below).  mk_bzip2_stream_begin: bz[0, n) = the whole file (the caller's -- the mapped file -- until _end);
 * window_bytes = compressed bytes per window (0 = 256 MiB, an unmeasured choice: profiles/e2e_bunzip2_windows.txt).  *taken = 0: no
 * "BZh1-9" at byte 0, no stream is open.  mk_bzip2_stream_next uploads the compressed bytes from the byte that holds the previous
 * cut's bit up to window_bytes further on, searches them for the two magics, walks the hits into blocks and stream ends, decodes
 * every block whose closing magic lies inside the upload (in passes, mk_codec_set_bzip2_pass_blocks applies), proves each (status
 * 0, it ends exactly on the next magic), walks, expands and CRC-checks them.  The cut is the LAST magic of the window -- proved, not
 * guessed --; the bytes behind it go up again with the next window.  An end-of-stream magic is consumed only when its 32 CRC bits,
 * the padding to the byte and either the file's end or the next "BZh" + level + first magic lie inside the upload; otherwise it is
 * the cut.  Blocks need nothing of each other: carried between windows are the next bit, whether a stream is open, its level, its
 * CRC folded so far, and the totals.  A window with fewer than two magics (a block longer than the window) is doubled and tried again
 * as long as the file has more bytes and the device the room (windows_grown).  Text is not bounded by compressed bytes (a block may
 * expand to 46 MB): the text buffers are sized by the blocks' text lengths once those are known and grow within half of the free
 * memory; a window whose text does not fit is delivered as SEVERAL text windows, each a prefix of whole blocks, at least one (the
 * bytes in front of the run-length step stay on the device for the rest).  mk_codec_set_bzip2_text_cap bounds a text window's bytes
 * (test hook; 0 = by the free memory; results do not depend on it).
 * *state = 0: a window of text was produced, *text_bytes long (0 for a window of empty streams): it is what mk_gzip_text_device /
 *             mk_gzip_text_read refer to, in one of two text buffers -- text window w stays valid until the call that produces w + 2;
 *          1: end of file: every block CRC and every stream's folded CRC agree; no text in this call;
 *          2: handed back (MK_OK): no text in this call and the stream produces nothing more -- a table that does not chain, a block
 *             that does not end on its magic, a status of the decoder (mk_bzip2_inflate_device lists them), a wrong block or stream
 *             CRC, bytes behind the last stream, data that ends early, more than 2^20 magics in a window, no room, any device error.
 *             The whole blocks in front of the fault are delivered first (state 0), so the text delivered before state 2 is a prefix
 *             of what libbz2 gives before it refuses: the caller's libbz2 reads the file from the front and skips stats.text_bytes.
 * mk_bzip2_stream_end closes the stream and frees what it held (the two text buffers included).  mk_bzip2_stream_info takes the
 * codec's lock and may be called beside mk_bzip2_stream_next; without an open stream: the last stream's figures.  While a bzip2
 * stream is open the one-shot gzip and bzip2 calls and mk_gzip_stream_begin return MK_E_INVALID_ARG -- and mk_bzip2_stream_begin
 * does while a gzip stream is --, and mk_gzip_text_release ends the stream as mk_bzip2_stream_end does. */
typedef struct mk_bzip2_stream_stats {
    uint64_t windows;           /* windows of text produced */
    uint64_t streams;           /* streams closed: their folded CRC agrees */
    uint64_t blocks;            /* blocks delivered: proved, their CRC agrees */
    uint64_t consumed_bytes;    /* compressed bytes in front of the next window's first bit */
    uint64_t text_bytes;        /* text bytes delivered so far */
    uint64_t windows_grown;     /* doublings of a window that held no whole block */
    uint64_t peak_device_bytes; /* most device memory the stream has held */
    float ms[5];                /* summed over the windows: upload, marker search, block decode, text (walk + expansion), CRC */
    uint32_t reserved;
} mk_bzip2_stream_stats;
int mk_bzip2_stream_begin(mk_codec *c, const uint8_t *bz, uint64_t n, uint64_t window_bytes, uint32_t *taken);
int mk_bzip2_stream_next(mk_codec *c, uint64_t *text_bytes, uint32_t *state);
int mk_bzip2_stream_info(const mk_codec *c, mk_bzip2_stream_stats *out);
int mk_bzip2_stream_end(mk_codec *c);
int mk_codec_set_bzip2_text_cap(mk_codec *c, uint64_t text_bytes);

/* (an addition to v7; `merkurio extract --zstd-stream`) A .zst file of ANY size, decoded on the device window by window: nothing on
 * the device is sized by the file, and a frame may hold 4 GiB of text or more.  The contract is mk_bzip2_stream_*'s.
 * mk_zstd_stream_begin: zs[0, n) = the whole file (the caller's -- the mapped file -- until _end); window_bytes = compressed bytes per
 * window (0 = 256 MiB, an unmeasured choice: profiles/e2e_unzstd_windows.txt).  *taken = 0: no frame or skippable-frame magic at byte
 * 0, no stream is open.  Every block header states its block's compressed size, so mk_zstd_stream_next walks on from where the window
 * before stopped (merkurio_amd/csrc/codec/zstd_chain.hpp, zstd_plan.hpp) and stops behind the first block at which the compressed
 * bytes taken reach window_bytes, or at which another block of 128 KiB beside the carried history would exceed the text cap, or the
 * file ends -- one block at the least; no start is guessed and no window grows.  A frame's 4 checksum bytes go with its last block.
 * The text cap is chosen from the free device memory, below 4 GiB minus the largest history (an unmeasured choice);
 * mk_codec_set_zstd_text_cap sets it (test hook; 0 = default; results do not depend on it).  Carried from window to window: whether a
 * frame is open, its window, content size, checksum flag and text so far (64 bits), the running XXH64 state, the three repeat
 * offsets behind the last block, a copy of the bytes that describe the tree and the three sequence tables in force (128 bytes each at
 * the most, laid in front of the next window's compressed bytes so that a block which repeats one builds it as it builds its own),
 * and the history: the last H = min(frame window, frame text so far) bytes of text, copied on the device to the front of the next
 * window's text buffer.  The execute step reads a match source inside the history as a byte; only sources inside the window wait
 * for the rounds of resolution, at most log2(blocks of the window) + 2.  The content checksum is XXH64 on the host over each
 * window's new text as it is downloaded, compared when the frame's last block has been decoded; a content size likewise, in 64 bits.
 * *state = 0: a window of text was produced, *text_bytes long (its NEW text, without the history; 0 for a window of empty frames):
 *             it is what mk_gzip_text_device / mk_gzip_text_read refer to, in one of two text buffers -- window w stays valid until
 *             the call that produces w + 2;
 *          1: end of file: every frame's size and checksum agree; no text in this call;
 *          2: handed back (MK_OK): no text in this call and the stream produces nothing more -- whatever mk_zstd_inflate_device
 *             lists, met in this window, a carried description above 128 bytes, no room, any device error.  The windows delivered
 *             before it are a prefix of what libzstd writes before it refuses: the caller's libzstd reads the file from the front
 *             and skips stats.text_bytes.
 * mk_zstd_stream_end closes the stream and frees what it held (the two text buffers included).  mk_zstd_stream_info takes the codec's
 * lock; without an open stream: the last stream's figures.  While a zstd stream is open the one-shot gzip, bzip2 and zstd calls and
 * mk_gzip_stream_begin / mk_bzip2_stream_begin return MK_E_INVALID_ARG -- and mk_zstd_stream_begin does while another stream is --,
 * and mk_gzip_text_release ends the stream as mk_zstd_stream_end does. */
typedef struct mk_zstd_stream_stats {
    uint64_t windows;           /* windows of text produced */
    uint64_t frames;            /* frames closed: content size and checksum agree */
    uint64_t blocks;            /* blocks delivered */
    uint64_t consumed_bytes;    /* compressed bytes in front of the next window */
    uint64_t text_bytes;        /* text bytes delivered so far */
    uint64_t rounds;            /* cross-block resolution rounds, summed over the windows */
    uint64_t max_history;       /* the largest history carried into a window, bytes */
    uint64_t peak_device_bytes; /* most device memory the stream has held */
    float ms[6];                /* summed over the windows, mk_zstd_info's phases: upload, tables + entropy decode, scans, execution
                                   (the history's copy included), cross-block rounds, checksum */
} mk_zstd_stream_stats;
int mk_zstd_stream_begin(mk_codec *c, const uint8_t *zs, uint64_t n, uint64_t window_bytes, uint32_t *taken);
int mk_zstd_stream_next(mk_codec *c, uint64_t *text_bytes, uint32_t *state);
int mk_zstd_stream_info(const mk_codec *c, mk_zstd_stream_stats *out);
int mk_zstd_stream_end(mk_codec *c);
int mk_codec_set_zstd_text_cap(mk_codec *c, uint64_t text_bytes);

/* (v7) A gzip file of SEVERAL members -- `cat a.gz b.gz`, a member per tile or per block without BGZF's BC field.  A member carries no
 * compressed size: where it ends is known once it is decoded.  So the starts are guessed on the host and proved on the device.
 * mk_gzip_member_guesses (host code, no device needed) reports every offset at which an RFC 1952 header parses inside gz[0, n): ID1
 * ID2 CM = 1f 8b 08, reserved FLG bits clear, FEXTRA / FNAME / FCOMMENT / FHCRC walked, at least 2 bytes of stream and 8 of trailer
 * behind it (and, behind offset 0, 8 bytes in front of it).  Offset 0 must be one, otherwise there are no guesses.  A guess is not a
 * member: the three bytes and the flag test pass at a handful of places per GB of compressed data.  crc / isize are read from the 8
 * bytes in front of the NEXT guess (the file's end for the last one).  *n_guesses = how many there are; table[0, min(cap, that)) is
 * written (table may be NULL).
 * mk_gzip_members_inflate_device: the whole file goes up, all candidate members are cut into pieces and decoded in ONE batch of
 * launches, the 32 KiB context chain restarts at every member.  Member 0 starts at byte 0; a guess is PROVED a member start when the
 * member in front of it decodes from its first bit to a final block that ends in the last byte in front of the trailer there, with
 * that trailer's CRC-32 and ISIZE.  A candidate that does not is joined with the next one (its end was no member start) and the
 * pieces are decoded again, four rounds in all.  *taken = 1 only when proved members cover gz[0, n) with nothing left over -- the
 * chain zlib walks; the text of all members lies back to back where mk_gzip_inflate_device leaves its text (mk_gzip_text_read /
 * _device / _release), *n_members says how many were proved.  *taken = 0 (MK_OK, nothing else touched): trailing bytes, a member of
 * 4 GiB of text or more, more than 65 535 pieces, and everything mk_gzip_inflate_device hands back. */
typedef struct mk_gzip_guess {
    uint64_t header_off; /* where the header parses */
    uint64_t data_off;   /* the first byte behind it: the member's DEFLATE stream, if this is a member */
    uint32_t crc, isize; /* of the 8 bytes in front of the next guess */
} mk_gzip_guess;
int mk_gzip_member_guesses(const uint8_t *gz, uint64_t n, mk_gzip_guess *table, uint64_t cap, uint64_t *n_guesses);
int mk_gzip_members_inflate_device(mk_codec *c, const uint8_t *gz, uint64_t n, uint64_t *text_bytes, uint32_t *taken, uint64_t *n_members);

/* (v7) A gzip file of ANY size, inflated on the device window by window: nothing on the device is sized by the file, a member may hold
 * 4 GiB of text or more.  mk_gzip_stream_begin: gz[0, n) = the whole file (the caller's -- the mapped file -- until _end);
 * window_bytes = compressed bytes per window (0 = 256 MiB).  mk_gzip_member_guesses runs once over the file.  *taken = 0: not a gzip
 * file, no stream is open.  mk_gzip_stream_next uploads the compressed bytes from the previous cut up to window_bytes further on,
 * searches block starts in them, decodes the pieces and stops at the LAST start that the piece in front of it lands on exactly -- a
 * cut that is proved, not guessed; the bytes behind it go up again with the next window.  The window's first bit is a known start,
 * the 32 KiB of text in front of it are carried on the device from window to window (two buffers), the CRC-32 of a member that is
 * open across windows is folded (mk_crc32_combine) and its length kept in 64 bits and compared with ISIZE modulo 2^32 (RFC 1952).
 * Member starts inside a window are the guesses there, proved by the join / drop rounds of mk_gzip_members_inflate_device; a member
 * whose trailer lies behind the upload stays open.  A window without a proved start (a huge stored block, a tiny window) is doubled
 * and tried again as long as the device has the room.  At most 65 535 pieces per window.
 * *state = 0: a window of text was produced, *text_bytes long: it is what mk_gzip_text_device / mk_gzip_text_read refer to, in one
 *             of two text buffers -- window w's text stays valid until the call that produces window w + 2;
 *          1: end of file: every member is proved, its CRC-32 and ISIZE agree; no text in this call;
 *          2: handed back (MK_OK): this window produced nothing and the stream produces nothing more -- a desync the rounds do not
 *             cure, an overflow at ratio 48, a distance in front of a member's first byte, a wrong CRC-32 or ISIZE, bytes behind the
 *             last member, no room on the device, any device error.  The text delivered before it is what zlib gives for those bytes;
 *             the caller's zlib takes the file from the front and skips stats.text_bytes.
 * mk_gzip_stream_end closes the stream and frees what it held (the two text buffers included); the one-shot calls work as before.
 * mk_gzip_stream_info may be called from another thread beside mk_gzip_stream_next (it takes the codec's lock, so it waits for the
 * window in progress); without an open stream it is MK_OK with the last stream's figures, zeros if there was none.  While a stream is
 * open the one-shot calls (mk_gzip_inflate_device, mk_gzip_members_inflate_device, mk_bzip2_inflate_device) and
 * mk_bzip2_stream_begin return MK_E_INVALID_ARG, and mk_gzip_text_release
 * ends the stream as mk_gzip_stream_end does.  A window drops at most three false member starts (three drop rounds): a window with
 * four or more header look-alikes that are no member starts -- planted in a stored block, say -- is handed back (state 2).
 * mk_crc32_combine (host code, no device): the CRC-32 of A ++ B from crc_a = CRC-32(A), crc_b = CRC-32(B) and len_b = |B|. */
typedef struct mk_gzip_stream_stats {
    uint64_t windows;           /* windows of text produced */
    uint64_t members;           /* members proved (decoded to their final block, CRC-32 and ISIZE agree) */
    uint64_t consumed_bytes;    /* compressed bytes in front of the next window's first bit */
    uint64_t text_bytes;        /* text bytes delivered so far */
    uint64_t windows_grown;     /* doublings of a window that had no proved start */
    uint64_t rounds_repeated;   /* decodes of a window's pieces beyond the first (dropped starts, joined members, ratio 48) */
    uint64_t peak_device_bytes; /* most device memory the stream has held */
    float ms[5];                /* summed over the windows: upload, block search, pieces, resolution, CRC-32 */
    uint32_t reserved;
} mk_gzip_stream_stats;
int mk_gzip_stream_begin(mk_codec *c, const uint8_t *gz, uint64_t n, uint64_t window_bytes, uint32_t *taken);
int mk_gzip_stream_next(mk_codec *c, uint64_t *text_bytes, uint32_t *state);
int mk_gzip_stream_info(const mk_codec *c, mk_gzip_stream_stats *out);
int mk_gzip_stream_end(mk_codec *c);
uint32_t mk_crc32_combine(uint32_t crc_a, uint32_t crc_b, uint64_t len_b);

/* -------------------------------------------------------------------------------------
 * `tag` on a window of a BAM file with the records RESIDENT ON THE DEVICE (v7) -- the reader loop, process_record and the writer
 * of src/cmd_tag.rs:503-615, :387-497, :254-271 for BAM -> BAM: only compressed members cross the host boundary, in both directions.
 *
 * The window's text = head[0, n_head) (the unfinished record the previous window ended with; the first window starts behind the
 * BAM header) ++ the text of members[0, n_members) of bgzf[0, n_bgzf) (out_off = running sum of ISIZE from 0), inflated on the
 * device and checked (CRC-32, ISIZE: MK_E_CORRUPT).  On the device: the records' block_size chain is indexed (pieces whose starts
 * are guessed and then proved by every piece's walk landing on the next piece's start: the table is the serial walk's), the 4-bit
 * sequences become the upper-case ASCII record.sequence() hands the matcher (:395), the scan, the emission order and the per-record
 * pattern sets run as in mk_tag_records, a record is kept by the rule of :457-467, and every kept record leaves as
 * block_size' | record | tag 'Z' value NUL -- the value being its distinct matched patterns, ascending, joined by ',' (:484-490),
 * merged with the items of the record's existing Z field of that name if it has one (:470-485; the old field stays)
 * -- packed back to back and deflated into BGZF members of block_bytes of text (0 = 65280; the last one shorter) in out[0, out_len).
 * The members inflate to exactly the bytes the CLI's host path writes for these records.
 * Outputs: n_window (bytes of text), n_rec whole records covering n_used bytes, tail[0, n_tail) = the text behind them (the next
 * window's head; tail_cap too small: MK_E_CAPACITY, n_tail = the need), n_kept, out_text_bytes (bytes of the kept records as
 * written), out_len (out_cap too small: MK_E_CAPACITY, out_len = the need).  out == NULL: nothing is written (`tag -s`).
 * A call that returns MK_E_CAPACITY (tail, then rows and names together, then out) has counted nothing: counters and
 * pattern_hit_counts are added to when the window is done.
 * logging != 0 (the reference's -l / -j): counters and pattern_hit_counts as mk_tag_records, rows[0, n_rows) in emission order
 * (row.rec = index in the window) and, per row, row_name[r] = offset of the record's NUL-terminated name in names[0, n_names_bytes)
 * (logger.log_fields' record.name(), :412); too small a rows / names buffer: MK_E_CAPACITY with n_rows / n_names_bytes = the need.
 * *status != 0: this window is not for the device and NOTHING was produced -- the caller's host reader takes it from the window's
 * first byte (and words the reference's errors): 1 = a record that fails the parser's checks or a chain that could not be proved,
 * 2 = optional fields that do not parse, 4 = a kept record whose field of the tag's name is not a string (the reference refuses it,
 * :482) or holds a value that is not plain ASCII or longer than 2 KiB, 8 = last != 0 and the text ends inside a record.
 * ms[]: milliseconds of upload, inflate, index, unpack + scan + sets, tag + emit, deflate, download; ms[7]: of these, growing device buffers.
 * --------------------------------------------------------------------------------------- */
typedef struct mk_bam_window {
    /* in */
    const uint8_t *head;
    uint64_t n_head;
    const uint8_t *bgzf;
    uint64_t n_bgzf;
    const mk_bgzf_member *members;
    uint64_t n_members;
    uint32_t last; /* no text follows this window */
    uint32_t filter_matching, invert;
    uint8_t tag[2];
    uint8_t reserved[2];
    uint32_t block_bytes;
    uint8_t *tail;
    uint64_t tail_cap;
    uint8_t *out;
    uint64_t out_cap;
    mk_row *rows;
    uint64_t rows_cap;
    uint64_t *row_name; /* room for rows_cap entries */
    uint8_t *names;
    uint64_t names_cap;
    /* optional: called from inside the call as soon as tail[0, n_tail) is known -- right after the record index, before the scan --
     * so that a caller with a second handle can start the next window (whose head this is) beside the rest of this one.  Not called
     * when the window is refused by the index (*status 1 or 8) or fails before that point. */
    void (*on_tail)(void *ctx, const uint8_t *tail, uint64_t n_tail);
    void *on_tail_ctx;
    /* out */
    uint64_t n_window, n_used, n_tail, n_rec, n_kept, out_text_bytes, out_len, n_rows, n_names_bytes;
    float ms[8];
} mk_bam_window;
int mk_tag_bam_window(mk_matcher *m, mk_codec *codec, mk_bam_window *w, int logging, mk_counters *counters, uint32_t *pattern_hit_counts,
                      uint32_t *status);
/* Tuning / test hook: bytes of text per piece of the record-chain index (0 = the default, 65536).  Results do not depend on it. */
int mk_matcher_set_bam_piece(mk_matcher *m, uint32_t piece_bytes);

/* -------------------------------------------------------------------------------------
 * `tag` on a window of SAM TEXT with the lines resident on the device (an addition to v7; kernels: sam.hip) -- the reader loop,
 * process_record and the text writer of src/cmd_tag.rs:559-612, :387-497 for SAM -> SAM or no output.  No codec: nothing is inflated
 * or deflated.
 *
 * The window's text = head[0, n_head) (the unfinished line the previous window ended with; may be empty) ++ text[0, n_text), uploaded
 * as it is (fastest from mk_host_alloc memory); together below 4 GiB (32-bit offsets; larger: MK_E_UNSUPPORTED).  On the device:
 * lines are split at '\n', one trailing '\r' is not part of a line; empty lines and lines that start with '@' are not records and
 * produce nothing.  A record line has at least 10 tab-separated fields; QNAME = the bytes before the first tab, SEQ = field 10 (a
 * SEQ that is exactly "*" has length 0); the matcher sees SEQ with a-z upper-cased and every other byte as it is.  Scan, emission
 * order, counters, pattern_hit_counts, rows, row_name and names (QNAME, NUL-terminated) as in mk_tag_bam_window; keep rule
 * :457-467.  Of a KEPT record the optional fields (fields 12 ...) are searched for the first one that is at least 5 bytes long and
 * starts with the tag's two bytes and ':': its type must be "Z:", its value is the rest of the field (an empty value counts as no
 * tag).  A kept record leaves as  line (without "\r" / "\n") TAB tag ":Z:" value "\n",  value = mk_tag_value's string, packed back
 * to back in record order in out[0, out_len); out_cap too small: MK_E_CAPACITY with out_len = the need and nothing counted (the
 * counters are added when the window is done).  out == NULL && out_cap == 0: nothing is written (`tag -S`), the checks still run.
 * n_used = bytes up to and including the last '\n' (last != 0: the whole window -- a final line without '\n' is a line); tail[0,
 * n_tail) = the rest, the next window's head.  A caller that cuts its input at line starts has empty heads and tails: its windows
 * are independent and may run on different handles at the same time.
 * *status != 0: this window is not for the device and NOTHING was produced -- the caller's host reader takes it from the window's
 * first byte (and words the reference's errors): 1 = a record line with fewer than 10 fields, 4 = a kept record whose field of the
 * tag's name is not "Z:", or whose value is not plain ASCII or longer than 2 KiB.  Records that are dropped are not looked at.
 * ms[]: milliseconds of [0] upload, [1] line index + fields, [2] gather + scan + sets, [3] tag + emit, [4] download; ms[7]: of
 * these, growing device buffers.
 * --------------------------------------------------------------------------------------- */
typedef struct mk_sam_window {
    /* in */
    const uint8_t *head;
    uint64_t n_head;
    const uint8_t *text;
    uint64_t n_text;
    uint32_t last; /* no text follows this window */
    uint32_t filter_matching, invert;
    uint8_t tag[2];
    uint8_t reserved[2];
    uint8_t *tail;
    uint64_t tail_cap;
    uint8_t *out;
    uint64_t out_cap;
    mk_row *rows;
    uint64_t rows_cap;
    uint64_t *row_name; /* room for rows_cap entries */
    uint8_t *names;
    uint64_t names_cap;
    /* out */
    uint64_t n_window, n_used, n_tail, n_rec, n_kept, out_len, n_rows, n_names_bytes;
    float ms[8];
} mk_sam_window;
int mk_tag_sam_window(mk_matcher *m, mk_sam_window *w, int logging, mk_counters *counters, uint32_t *pattern_hit_counts, uint32_t *status);

/* -------------------------------------------------------------------------------------
 * `tag` on a window of SAM TEXT whose kept records leave as BAM (an addition to v7; kernels: sam.hip) -- SAM -> BAM: the window,
 * its lines, the scan, the keep rule, the tag's value, rows, names, counters, tail and n_used are mk_tag_sam_window's; what leaves is
 * mk_tag_bam_window's: every kept record as  block_size | BAM record,  back to back in record order (out_text_bytes of them),
 * deflated into BGZF members of block_bytes of text (0 = 65280) in out[0, out_len).  The members inflate to exactly the bytes the
 * CLI's host path writes for these records: it appends TAB tag ":Z:" value to the line and encodes the line (cli/bam_out.cpp:
 * BamWriter::encode_record), which is the definition.  Restated:
 *   refID / next_refID: the index of RNAME / RNEXT among the n_refs reference names ref_names[ref_off[i], ref_off[i + 1]) (the @SQ
 *     lines' SN, in the order of the BAM header; of equal names the first), -1 for "*" or a name not among them; RNEXT "=" = refID.
 *   pos, next_pos = POS - 1, PNEXT - 1; mapq, flag, tlen = the low 8 / 16 / 32 bits of MAPQ, FLAG, TLEN;
 *   bin = reg2bin(pos, pos + (the reference bases of the CIGAR, or 1 without any)) on signed 64-bit values (POS 0: 4680);
 *   l_read_name = QNAME + NUL; CIGAR "*" = no ops, else len << 4 | op of "MIDNSHP=X"; SEQ "*" = l_seq 0, else two bases per byte from
 *   "=ACMGRSVTWYHKDBN" in either case (any other byte: 15; an odd length pads with 0); QUAL "*" = l_seq bytes 0xFF, else each byte - 33;
 *   optional fields TAG:TYPE:VALUE in line order, then the tag:  A = one byte (none: 0);  i = the smallest of C S I (>= 0) or c s i
 *   (< 0) that holds the value;  f = a float;  Z / H = the bytes and NUL;  B = subtype, count, items ("B:c,1,2").
 * The device converts plain numbers only (sam_numbers.hpp): an integer is [+-] and 1-18 digits, a CIGAR length 1-9 digits, a float
 * [+-]digits[.digits][e[+-]digits] whose digits without the point are an integer below 2^24 and whose net power of ten is within
 * +-10 (one exactly rounded double operation, then one rounding to float: strtof's value).
 * *status != 0: this window is not for the device and NOTHING was produced or counted -- the caller's host path takes it from the
 * window's first byte (and words the errors).  Bits: 1 = a record line with fewer than 10 fields, or a KEPT line with fewer than 11;
 * 2 = a kept record that does not encode as above: QNAME longer than 254 bytes; a CIGAR with a byte that is no op, a length that is
 * not 1-9 digits, or more than 65 535 ops; QUAL of another length than SEQ; FLAG, POS, MAPQ, PNEXT, TLEN, an `i` value or an integer
 * item that is not a plain integer; an `f` value or item outside the float rule (inf, nan, hex, long digit strings, large exponents);
 * an optional field shorter than 5 bytes or without its two colons (an empty field behind a final tab included); an unknown type; a B
 * field without a subtype, with an unknown one, or whose items do not each follow a ','; 4 = as in mk_tag_sam_window.  Records that
 * are dropped are not looked at.
 * MK_E_CAPACITY (tail, then rows and names together, then out; the need in n_tail / n_rows + n_names_bytes / out_len) has counted
 * nothing.  out == NULL && out_cap == 0: nothing is encoded or written, the checks still run (out_text_bytes is set, out_len 0).
 * ms[]: milliseconds of [0] upload, [1] line index + fields, [2] gather + scan + sets, [3] tag + encode, [4] deflate, [5] download;
 * ms[7]: of these, growing device buffers.
 * --------------------------------------------------------------------------------------- */
typedef struct mk_sam_bam_window {
    /* in */
    const uint8_t *head;
    uint64_t n_head;
    const uint8_t *text;
    uint64_t n_text;
    uint32_t last; /* no text follows this window */
    uint32_t filter_matching, invert;
    uint8_t tag[2];
    uint8_t reserved[2];
    const uint8_t *ref_names; /* the reference names, back to back */
    const uint64_t *ref_off;  /* n_refs + 1 ascending offsets into ref_names */
    uint64_t n_refs;
    uint32_t block_bytes;
    uint32_t reserved2;
    uint8_t *tail;
    uint64_t tail_cap;
    uint8_t *out;
    uint64_t out_cap;
    mk_row *rows;
    uint64_t rows_cap;
    uint64_t *row_name; /* room for rows_cap entries */
    uint8_t *names;
    uint64_t names_cap;
    /* out */
    uint64_t n_window, n_used, n_tail, n_rec, n_kept, out_text_bytes, out_len, n_rows, n_names_bytes;
    float ms[8];
} mk_sam_bam_window;
int mk_tag_sam_bam_window(mk_matcher *m, mk_codec *codec, mk_sam_bam_window *w, int logging, mk_counters *counters, uint32_t *pattern_hit_counts,
                          uint32_t *status);

/* -------------------------------------------------------------------------------------
 * `tag` on a window of a BAM file whose kept records leave as SAM TEXT (an addition to v7; kernels: bam.hip) -- BAM -> SAM / STDOUT:
 * the window, its members, head and tail, on_tail, the record index, the scan, the keep rule, the tag's value, rows, names and counters
 * are mk_tag_bam_window's; what leaves is mk_tag_sam_window's: every kept record as  line TAB tag ":Z:" value "\n",  back to back in
 * record order in out[0, out_len) -- only these lines are downloaded.  The line is what the CLI's host path writes for the record
 * (cli/sam_in.cpp: SamFile::append_line), which is the definition.  Restated, tab-separated:
 *   QNAME: read_name without its NUL;  FLAG, MAPQ: decimal;
 *   RNAME: reference name refID -- ref_names[ref_off[i], ref_off[i + 1]), the names of the BAM header in its order -- when
 *     0 <= refID < n_refs, else "*";  RNEXT: "*" when next_refID < 0, "=" when it equals refID, its name when it is < n_refs, else "*";
 *   POS, PNEXT: the field + 1;  TLEN: signed decimal;
 *   CIGAR: "*" without ops, else per op its length and its letter of "MIDNSHP=X" (an op code of 9 or more prints '?');
 *   SEQ: "*" when l_seq is 0, else "=ACMGRSVTWYHKDBN"[nibble], high nibble first;
 *   QUAL: "*" when l_seq is 0 or the first byte is 0xFF, else each byte + 33 (modulo 256);
 *   the optional fields in record order as TAG:TYPE:VALUE:  A = the byte;  c C s S i I = "i:" and the decimal value;  f = "f:" and
 *     "%g" of the float;  Z / H = the bytes up to the NUL;  B = "B:", the subtype, then ",item" per item;
 *   then the tag -- an existing field of that name stays where it is, the merged value is appended, as on every other path.
 * Integers are plain decimal.  A float is formatted only where "%g" can be computed exactly in 64-bit integers (bam_numbers.hpp): +-0,
 * and the finite values that, rounded to six significant digits, have a decimal exponent of -4 ... 5 ("%g"'s fixed notation).
 * *status != 0: this window is not for the device and NOTHING was produced or counted -- the caller's host path takes it from the
 * window's first byte (and words the errors).  Bits 1, 4 and 8 as in mk_tag_bam_window;  2 = a kept record whose optional fields do
 * not parse (an unknown B subtype with items included), or with an `f` value / item outside the float rule (exponent notation, inf,
 * nan, subnormals), or with POS or PNEXT = 2^31 - 1 (the host path adds 1 in 32 bits).  Records that are dropped are not looked at.
 * MK_E_CAPACITY (tail, then rows and names together, then out; the need in n_tail / n_rows + n_names_bytes / out_len) has counted
 * nothing.  out == NULL && out_cap == 0: nothing is formatted or written (out_len 0), the checks still run.
 * ms[]: milliseconds of [0] upload, [1] inflate, [2] record index, [3] unpack + scan + sets, [4] tag + format, [5] download; ms[7]: of
 * these, growing device buffers.
 * --------------------------------------------------------------------------------------- */
typedef struct mk_bam_sam_window {
    /* in */
    const uint8_t *head;
    uint64_t n_head;
    const uint8_t *bgzf;
    uint64_t n_bgzf;
    const mk_bgzf_member *members;
    uint64_t n_members;
    uint32_t last; /* no text follows this window */
    uint32_t filter_matching, invert;
    uint8_t tag[2];
    uint8_t reserved[2];
    const uint8_t *ref_names; /* the reference names, back to back */
    const uint64_t *ref_off;  /* n_refs + 1 ascending offsets into ref_names */
    uint64_t n_refs;
    uint8_t *tail;
    uint64_t tail_cap;
    uint8_t *out;
    uint64_t out_cap;
    mk_row *rows;
    uint64_t rows_cap;
    uint64_t *row_name; /* room for rows_cap entries */
    uint8_t *names;
    uint64_t names_cap;
    void (*on_tail)(void *ctx, const uint8_t *tail, uint64_t n_tail); /* as in mk_bam_window */
    void *on_tail_ctx;
    /* out */
    uint64_t n_window, n_used, n_tail, n_rec, n_kept, out_len, n_rows, n_names_bytes;
    float ms[8];
} mk_bam_sam_window;
int mk_tag_bam_sam_window(mk_matcher *m, mk_codec *codec, mk_bam_sam_window *w, int logging, mk_counters *counters, uint32_t *pattern_hit_counts,
                          uint32_t *status);

/* walks the BSIZE chain of in[0, n): fills members[0, cap) (out_off = running sum of ISIZE), *n_members = how many there are,
 * *consumed = bytes of whole members, *text_bytes = sum of ISIZE.  MK_E_CORRUPT where a header is not BGZF; a trailing
 * partial member is not an error (*consumed < n).  Host code, no device. */
int mk_bgzf_members(const uint8_t *in, uint64_t n, mk_bgzf_member *members, uint64_t cap, uint64_t *n_members, uint64_t *consumed,
                    uint64_t *text_bytes);
/* the 28-byte empty member that ends a BGZF file */
const uint8_t *mk_bgzf_eof(void);
/* Tuning / test hook: a call is cut into device passes of at most `deflate_members` members (default 49 152 = 3.2 GB of
 * text) / `inflate_text_bytes` of text (default 3 GiB); 0 keeps the default.  Results do not depend on it. */
int mk_codec_set_pass_limits(mk_codec *c, uint64_t deflate_members, uint64_t inflate_text_bytes);
/* (v6) Tuning / test hook: which inflate kernel the handle's calls use -- 0 (default) by the number of members in the call,
 * 1 one lane per member (many members in flight, each slow), 2 one wave per member with the member's recent text in LDS (few in
 * flight, each fast), 3 / 4 / 5 / 6 the same with only the most recent 8 / 16 / 4 / 2 KiB of the member's text in LDS (12 / 7 / 19 / 25 waves per
 * CU instead of 4; matches that reach further read the text back from device memory).  mk_gzip_inflate_device gives a piece of
 * the stream to a wave, with 1 to a lane.  Results do not depend on it. */
int mk_codec_set_inflate_kernel(mk_codec *c, int which);
/* (v7) Tuning / test hook of mk_gzip_inflate_device: the nominal distance between two cuts of the stream, in compressed bytes -- a
 * power of two, 4 KiB ... 1 MiB; 0 (default): by the size of the stream (16 KiB up to ~200 MB of it, 64 KiB above).  A piece starts at the first DEFLATE block found behind a cut.  Results do not depend on it. */
int mk_codec_set_gzip_chunk(mk_codec *c, uint64_t chunk_bytes);
/* milliseconds of the handle's last call: [0] upload, [1] kernels, [2] download */
int mk_codec_times(const mk_codec *c, float ms[3]);

#ifdef __cplusplus
}
#endif
#endif
