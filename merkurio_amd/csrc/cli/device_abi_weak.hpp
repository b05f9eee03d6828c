// device_abi_weak.hpp -- the device codec and page-locked memory, reached through weak references: the reader / writer harnesses of the
// CPU tests compile the readers without libmerkurio_hip.so (they never select a device: set_bgzf_device / BamWriter::use_device;
// HostBuffer takes malloc's memory there), the CLI links it.  Included by the .cpp files that make these calls, by nothing else.
#pragma once
#include "../../../include/merkurio_hip.h"

extern "C" {
__attribute__((weak)) int mk_codec_create(int device, mk_codec **out);
__attribute__((weak)) void mk_codec_destroy(mk_codec *c);
__attribute__((weak)) uint64_t mk_bgzf_deflate_bound(uint64_t n, uint32_t block_bytes);
__attribute__((weak)) int mk_bgzf_deflate_pieces(mk_codec *c, const uint8_t *const *pieces, const uint64_t *sizes, uint64_t n_pieces, uint32_t block_bytes,
                                                 uint8_t *out, uint64_t out_cap, uint64_t *out_len);
__attribute__((weak)) int mk_bgzf_inflate(mk_codec *c, const uint8_t *in, uint64_t n_in, const mk_bgzf_member *members, uint64_t n_members, uint8_t *out,
                                          uint64_t out_cap, uint64_t *bad_member);
__attribute__((weak)) const char *mk_last_error(void);
__attribute__((weak)) int mk_host_alloc(size_t bytes, void **out);
__attribute__((weak)) void mk_host_free(void *p);
// (extract_window_call.cpp: reached by `extract --zstd-output` on the window path only, which needs a codec handle)
__attribute__((weak)) int mk_extract_window_frames(mk_matcher *m, mk_codec *codec, uint32_t format, uint32_t n_sources, mk_window_source *sources,
                                                   mk_window_members *frames, int logging, int invert, uint64_t rec_cap, uint64_t *n_rec, uint8_t *keep,
                                                   mk_row *rows, uint64_t rows_cap, uint64_t *n_rows, mk_counters *counters, uint32_t *pattern_hit_counts,
                                                   uint32_t *status);
// (an open window of `extract`: the window's first record start is found on the device)
__attribute__((weak)) int mk_extract_window_open(mk_matcher *m, mk_codec *codec, uint32_t format, uint32_t n_sources, mk_window_source *sources, int logging,
                                                 int invert, uint64_t rec_cap, uint64_t *n_rec, uint8_t *keep, mk_row *rows, uint64_t rows_cap, uint64_t *n_rows,
                                                 mk_counters *counters, uint32_t *pattern_hit_counts, uint32_t *status, mk_window_front *fronts);
__attribute__((weak)) int mk_zstd_deflate_info(const mk_codec *c, uint64_t *n_frames, uint32_t kinds[3], float ms[3]);
}
