"""ctypes binding of libmerkurio_hip.so (include/merkurio_hip.h) and a thin Python mirror of the
reference's matcher surface, so tests read like the reference's own tests:

    BNDMq(pattern, q).find_iter(text) / find_all / find_match   src/pattern_matching.rs:61-153
    AhoCorasick(patterns, ascii_case_insensitive).find_overlapping_iter(text)
                                                                 src/cmd_extract.rs:260-265,332
    parse_pattern_list / read_kmers_from_file / recommend_aho_corasick / tune_q_value /
    generate_masks                                               src/helpers.rs, pattern_*.rs
    Matcher(...).extract_single / extract_paired / tag_records   the record loops of cmd_*.rs

Everything that searches text runs in the gfx950 kernels; there is no CPU fallback here: if
the library or a GPU is missing, construction raises.
"""
import collections
import ctypes as C
import time
import importlib.util
import os

import numpy as np

from . import build as _build

MK_OK = 0
MK_E_EMPTY_PATTERN = -1
MK_E_INVALID_Q = -2
MK_E_PATTERN_TOO_LONG = -3
MK_E_NO_PATTERNS = -4
MK_E_NOMEM = -5
MK_E_PAIR_MISMATCH = -6
MK_E_HIP = -7
MK_E_CAPACITY = -8
MK_E_INVALID_ARG = -9
MK_E_UNSUPPORTED = -10
MK_E_RCCL = -11
MK_E_CORRUPT = -12
MK_COMM_ID_BYTES = 128

MK_ALGO_AUTO, MK_ALGO_AC, MK_ALGO_BNDMQ = 0, 1, 2
MK_FLAG_ASCII_CASE_INSENSITIVE = 1
MK_MODE_ANY, MK_MODE_HITS = 0, 1
MK_NUM_SUMMARY = 8
MK_SUM_HITS, MK_SUM_RECORDS_HIT, MK_SUM_RECORDS, MK_SUM_BASES, MK_SUM_CANDIDATES = 0, 1, 2, 3, 4

HIT_DTYPE = np.dtype([("rec", "<u8"), ("pat", "<u4"), ("pos", "<u4")])
ROW_DTYPE = np.dtype([("rec", "<u8"), ("pat", "<u4"), ("pos", "<u4"), ("file", "<u4"), ("_pad", "<u4")])

EXPORTS = [
    "mk_abi_version", "mk_last_error", "mk_device_count", "mk_read_kmers_from_text", "mk_parse_pattern_list",
    "mk_reverse_complement", "mk_canonical", "mk_recommend_aho_corasick", "mk_tune_q_value", "mk_generate_masks",
    "mk_free", "mk_matcher_create", "mk_matcher_create_ex", "mk_plan_geometry", "mk_matcher_destroy", "mk_matcher_algo", "mk_matcher_num_patterns",
    "mk_matcher_filter_info", "mk_matcher_class_info", "mk_matcher_filter_mode", "mk_scan_batch", "mk_scan_device", "mk_order_hits", "mk_order_hits_device", "mk_matcher_order_info", "mk_matcher_order_stats", "mk_matcher_kernel_name",
    "mk_matcher_launch_info", "mk_scan_tile_geometry", "mk_matcher_scan_geometry", "mk_matcher_enable_timing", "mk_matcher_kernel_times", "mk_matcher_hint_hit_density", "mk_matcher_hint_record_lengths", "mk_matcher_set_fixed_record_length", "mk_matcher_check_device",
    "mk_extract_single", "mk_extract_fastq_text", "mk_upload_text_ahead", "mk_host_alloc", "mk_host_free", "mk_extract_paired", "mk_tag_records", "mk_tag_value", "mk_matcher_batch_times", "mk_synth_reads_device",
    "mk_synth_reads_host", "mk_synth_reads_device_range", "mk_reduce_counters", "mk_reduce_prepare", "mk_comm_available", "mk_comm_unique_id", "mk_comm_init",
    "mk_comm_reduce_counters", "mk_comm_size", "mk_comm_destroy",
    "mk_codec_create", "mk_codec_destroy", "mk_bgzf_deflate_bound", "mk_bgzf_deflate", "mk_bgzf_deflate_pieces", "mk_bgzf_inflate", "mk_bgzf_members", "mk_bgzf_eof",
    "mk_codec_times", "mk_codec_set_pass_limits", "mk_codec_set_inflate_kernel", "mk_codec_set_gzip_chunk", "mk_gzip_inflate_device", "mk_gzip_member_guesses", "mk_gzip_members_inflate_device", "mk_gzip_text_read", "mk_gzip_text_device", "mk_gzip_text_release", "mk_gzip_info", "mk_bzip2_inflate_device", "mk_bzip2_info", "mk_zstd_inflate_device", "mk_zstd_info", "mk_xz_inflate_device", "mk_xz_info", "mk_codec_set_xz_spread", "mk_zstd_record_cuts", "mk_zstd_deflate_bound", "mk_zstd_deflate_records", "mk_zstd_deflate_info", "mk_codec_set_bzip2_pass_blocks",
    "mk_bzip2_stream_begin", "mk_bzip2_stream_next", "mk_bzip2_stream_info", "mk_bzip2_stream_end", "mk_codec_set_bzip2_text_cap",
    "mk_zstd_stream_begin", "mk_zstd_stream_next", "mk_zstd_stream_info", "mk_zstd_stream_end", "mk_codec_set_zstd_text_cap",
    "mk_xz_stream_begin", "mk_xz_stream_next", "mk_xz_stream_info", "mk_xz_stream_end", "mk_codec_set_xz_text_cap",
    "mk_gzip_stream_begin", "mk_gzip_stream_next", "mk_gzip_stream_info", "mk_gzip_stream_end", "mk_crc32_combine", "mk_extract_fastq_bgzf", "mk_extract_window",
    "mk_bgzf_record_cuts", "mk_bgzf_deflate_records", "mk_codec_cut_times", "mk_extract_window_members", "mk_extract_window_frames", "mk_extract_window_open",
    "mk_tag_bam_window", "mk_matcher_set_bam_piece", "mk_tag_sam_window", "mk_tag_sam_bam_window", "mk_tag_bam_sam_window",
]


class MerkurioError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[{code}] {msg}")
        self.code = code


class PatternError(MerkurioError):
    """src/pattern_matching.rs:28-36"""
    KINDS = {MK_E_EMPTY_PATTERN: "EmptyPattern", MK_E_INVALID_Q: "InvalidQGramLength",
             MK_E_PATTERN_TOO_LONG: "PatternTooLong"}

    @property
    def kind(self):
        return self.KINDS.get(self.code, "?")


class GzipStreamStats(C.Structure):
    """mk_gzip_stream_stats"""
    _fields_ = [("windows", C.c_uint64), ("members", C.c_uint64), ("consumed_bytes", C.c_uint64), ("text_bytes", C.c_uint64),
                ("windows_grown", C.c_uint64), ("rounds_repeated", C.c_uint64), ("peak_device_bytes", C.c_uint64), ("ms", C.c_float * 5),
                ("reserved", C.c_uint32)]


class Bzip2StreamStats(C.Structure):
    """mk_bzip2_stream_stats"""
    _fields_ = [("windows", C.c_uint64), ("streams", C.c_uint64), ("blocks", C.c_uint64), ("consumed_bytes", C.c_uint64), ("text_bytes", C.c_uint64),
                ("windows_grown", C.c_uint64), ("peak_device_bytes", C.c_uint64), ("ms", C.c_float * 5), ("reserved", C.c_uint32)]


class ZstdStreamStats(C.Structure):
    """mk_zstd_stream_stats"""
    _fields_ = [("windows", C.c_uint64), ("frames", C.c_uint64), ("blocks", C.c_uint64), ("consumed_bytes", C.c_uint64), ("text_bytes", C.c_uint64),
                ("rounds", C.c_uint64), ("max_history", C.c_uint64), ("peak_device_bytes", C.c_uint64), ("ms", C.c_float * 6)]


class XzStreamStats(C.Structure):
    """mk_xz_stream_stats"""
    _fields_ = [("windows", C.c_uint64), ("streams", C.c_uint64), ("blocks", C.c_uint64), ("consumed_bytes", C.c_uint64), ("text_bytes", C.c_uint64),
                ("planned_windows", C.c_uint64), ("largest_block_text", C.c_uint64), ("peak_device_bytes", C.c_uint64), ("status", C.c_int32),
                ("reserved", C.c_uint32), ("ms", C.c_float * 4)]


class MatcherOptions(C.Structure):
    """mk_matcher_options (include/merkurio_hip.h): tuning / test hooks of mk_matcher_create_ex"""
    _fields_ = [("struct_size", C.c_uint32), ("force_stride", C.c_uint32), ("force_global_filter", C.c_uint32),
                ("gbloom_log2_blocks", C.c_uint32), ("tile_run", C.c_uint32), ("gbloom_kib", C.c_uint32),
                ("length_classes", C.c_uint32), ("force_split_len", C.c_uint32), ("force_stride2", C.c_uint32),
                ("force_q2", C.c_uint32)]

    def __init__(self, force_stride=0, force_global_filter=False, gbloom_log2_blocks=0, tile_run=0, gbloom_kib=0,
                 length_classes=0, force_split_len=0, force_stride2=0, force_q2=0, force_single_class=False):
        super().__init__(C.sizeof(MatcherOptions), int(force_stride), int(bool(force_global_filter)),
                         int(gbloom_log2_blocks), int(tile_run), int(gbloom_kib),
                         1 if force_single_class else int(length_classes), int(force_split_len), int(force_stride2), int(force_q2))


class TileGeometry(C.Structure):
    """mk_tile_geometry (include/merkurio_hip.h): how a scan launch cuts its text into wave tiles"""
    _fields_ = [("n_waves", C.c_uint64), ("n_long_tiles", C.c_uint64), ("long_tile_bytes", C.c_uint64), ("n_short_tiles", C.c_uint64),
                ("short_tile_bytes", C.c_uint64), ("tail_start", C.c_uint64), ("long_tile_loads", C.c_uint32),
                ("short_tile_loads", C.c_uint32), ("tile_run", C.c_uint32), ("reserved", C.c_uint32)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_ if k != "reserved"}


class WindowText(C.Structure):
    """mk_window_text (include/merkurio_hip.h): what mk_extract_fastq_bgzf hands back of a window's text"""
    _fields_ = [("text", C.c_void_p), ("text_cap", C.c_uint64), ("tail", C.c_void_p), ("tail_cap", C.c_uint64), ("kept", C.c_void_p),
                ("kept_cap", C.c_uint64), ("n_text", C.c_uint64), ("n_used", C.c_uint64), ("n_tail", C.c_uint64), ("n_kept_bytes", C.c_uint64)]


class WindowSource(C.Structure):
    """mk_window_source (include/merkurio_hip.h, v6): one input file's part of a window handed to mk_extract_window"""
    _fields_ = [("head", C.c_void_p), ("n_head", C.c_uint64), ("text", C.c_void_p), ("n_text", C.c_uint64), ("bgzf", C.c_void_p),
                ("n_bgzf", C.c_uint64), ("members", C.c_void_p), ("n_members", C.c_uint64), ("device_text", C.c_void_p), ("n_device_text", C.c_uint64), ("ends_at_record", C.c_uint32),
                ("reserved", C.c_uint32), ("rec_start", C.c_void_p), ("tail", C.c_void_p), ("tail_cap", C.c_uint64), ("kept", C.c_void_p),
                ("kept_cap", C.c_uint64), ("all", C.c_void_p), ("all_cap", C.c_uint64), ("n_window", C.c_uint64), ("n_used", C.c_uint64),
                ("n_tail", C.c_uint64), ("n_kept_bytes", C.c_uint64), ("n_rec_seen", C.c_uint64)]


class WindowMembers(C.Structure):
    """mk_window_members (include/merkurio_hip.h, v7): where one source's kept records go as BGZF members (mk_extract_window_members)"""
    _fields_ = [("members", C.c_void_p), ("members_cap", C.c_uint64), ("ids", C.c_void_p), ("ids_cap", C.c_uint64), ("id_end", C.c_void_p),
                ("text_below", C.c_uint64), ("n_member_bytes", C.c_uint64), ("n_members", C.c_uint64), ("n_written", C.c_uint64),
                ("n_kept", C.c_uint64), ("n_id_bytes", C.c_uint64), ("as_text", C.c_uint32), ("written_ms", C.c_float)]


class WindowFront(C.Structure):
    """mk_window_front (include/merkurio_hip.h, v7): where the text in front of an open window's found start goes (mk_extract_window_open)"""
    _fields_ = [("front", C.c_void_p), ("front_cap", C.c_uint64), ("n_front", C.c_uint64)]


MK_TEXT_FASTQ, MK_TEXT_FASTA = 0, 1
BGZF_CUT_GRID, BGZF_MEMBER_TEXT_MAX = 49152, 65280  # the cut rule of include/merkurio_hip.h


class BamWindow(C.Structure):
    """mk_bam_window (include/merkurio_hip.h, v7): a window of a BAM file handed to mk_tag_bam_window"""
    _fields_ = [("head", C.c_void_p), ("n_head", C.c_uint64), ("bgzf", C.c_void_p), ("n_bgzf", C.c_uint64), ("members", C.c_void_p), ("n_members", C.c_uint64),
                ("last", C.c_uint32), ("filter_matching", C.c_uint32), ("invert", C.c_uint32), ("tag", C.c_uint8 * 2), ("reserved", C.c_uint8 * 2),
                ("block_bytes", C.c_uint32), ("tail", C.c_void_p), ("tail_cap", C.c_uint64), ("out", C.c_void_p), ("out_cap", C.c_uint64),
                ("rows", C.c_void_p), ("rows_cap", C.c_uint64), ("row_name", C.c_void_p), ("names", C.c_void_p), ("names_cap", C.c_uint64),
                ("on_tail", C.c_void_p), ("on_tail_ctx", C.c_void_p),
                ("n_window", C.c_uint64), ("n_used", C.c_uint64), ("n_tail", C.c_uint64), ("n_rec", C.c_uint64), ("n_kept", C.c_uint64),
                ("out_text_bytes", C.c_uint64), ("out_len", C.c_uint64), ("n_rows", C.c_uint64), ("n_names_bytes", C.c_uint64), ("ms", C.c_float * 8)]


class SamWindow(C.Structure):
    """mk_sam_window (include/merkurio_hip.h, v7): a window of SAM text handed to mk_tag_sam_window"""
    _fields_ = [("head", C.c_void_p), ("n_head", C.c_uint64), ("text", C.c_void_p), ("n_text", C.c_uint64),
                ("last", C.c_uint32), ("filter_matching", C.c_uint32), ("invert", C.c_uint32), ("tag", C.c_uint8 * 2), ("reserved", C.c_uint8 * 2),
                ("tail", C.c_void_p), ("tail_cap", C.c_uint64), ("out", C.c_void_p), ("out_cap", C.c_uint64),
                ("rows", C.c_void_p), ("rows_cap", C.c_uint64), ("row_name", C.c_void_p), ("names", C.c_void_p), ("names_cap", C.c_uint64),
                ("n_window", C.c_uint64), ("n_used", C.c_uint64), ("n_tail", C.c_uint64), ("n_rec", C.c_uint64), ("n_kept", C.c_uint64),
                ("out_len", C.c_uint64), ("n_rows", C.c_uint64), ("n_names_bytes", C.c_uint64), ("ms", C.c_float * 8)]


class SamBamWindow(C.Structure):
    """mk_sam_bam_window (include/merkurio_hip.h, v7): a window of SAM text handed to mk_tag_sam_bam_window"""
    _fields_ = [("head", C.c_void_p), ("n_head", C.c_uint64), ("text", C.c_void_p), ("n_text", C.c_uint64),
                ("last", C.c_uint32), ("filter_matching", C.c_uint32), ("invert", C.c_uint32), ("tag", C.c_uint8 * 2), ("reserved", C.c_uint8 * 2),
                ("ref_names", C.c_void_p), ("ref_off", C.c_void_p), ("n_refs", C.c_uint64), ("block_bytes", C.c_uint32), ("reserved2", C.c_uint32),
                ("tail", C.c_void_p), ("tail_cap", C.c_uint64), ("out", C.c_void_p), ("out_cap", C.c_uint64),
                ("rows", C.c_void_p), ("rows_cap", C.c_uint64), ("row_name", C.c_void_p), ("names", C.c_void_p), ("names_cap", C.c_uint64),
                ("n_window", C.c_uint64), ("n_used", C.c_uint64), ("n_tail", C.c_uint64), ("n_rec", C.c_uint64), ("n_kept", C.c_uint64),
                ("out_text_bytes", C.c_uint64), ("out_len", C.c_uint64), ("n_rows", C.c_uint64), ("n_names_bytes", C.c_uint64), ("ms", C.c_float * 8)]


class BamSamWindow(C.Structure):
    """mk_bam_sam_window (include/merkurio_hip.h, v7): a window of a BAM file handed to mk_tag_bam_sam_window"""
    _fields_ = [("head", C.c_void_p), ("n_head", C.c_uint64), ("bgzf", C.c_void_p), ("n_bgzf", C.c_uint64), ("members", C.c_void_p), ("n_members", C.c_uint64),
                ("last", C.c_uint32), ("filter_matching", C.c_uint32), ("invert", C.c_uint32), ("tag", C.c_uint8 * 2), ("reserved", C.c_uint8 * 2),
                ("ref_names", C.c_void_p), ("ref_off", C.c_void_p), ("n_refs", C.c_uint64),
                ("tail", C.c_void_p), ("tail_cap", C.c_uint64), ("out", C.c_void_p), ("out_cap", C.c_uint64),
                ("rows", C.c_void_p), ("rows_cap", C.c_uint64), ("row_name", C.c_void_p), ("names", C.c_void_p), ("names_cap", C.c_uint64),
                ("on_tail", C.c_void_p), ("on_tail_ctx", C.c_void_p),
                ("n_window", C.c_uint64), ("n_used", C.c_uint64), ("n_tail", C.c_uint64), ("n_rec", C.c_uint64), ("n_kept", C.c_uint64),
                ("out_len", C.c_uint64), ("n_rows", C.c_uint64), ("n_names_bytes", C.c_uint64), ("ms", C.c_float * 8)]


class Counters(C.Structure):
    _fields_ = [("nb_records_tot", C.c_uint64), ("nb_bases", C.c_uint64), ("nb_hits_tot", C.c_uint64 * 2),
                ("nb_records_hit", C.c_uint64 * 2), ("nb_records_extracted", C.c_uint64)]

    def as_dict(self, counts):
        return {"records": self.nb_records_tot, "bases": self.nb_bases,
                "hits": (self.nb_hits_tot[0], self.nb_hits_tot[1]),
                "records_hit": (self.nb_records_hit[0], self.nb_records_hit[1]),
                "extracted": self.nb_records_extracted, "pattern_hit_counts": counts.tolist()}


_lib = None


def lib_path():
    return _build.LIB_PATH


def _bind_to_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch wheels bundle their own libamdhip64.so (same soname,
    libamdhip64.so.7, as /opt/rocm's); two runtimes in one process each try to own the GPU and the
    second one finds none.  If PyTorch is installed, load ITS runtime first so that
    libmerkurio_hip.so's DT_NEEDED binds to it and a later `import torch` shares it.  A host
    without PyTorch (the C++ CLI, a Rust host) uses the system runtime.
    Set MERKURIO_SYSTEM_HIP=1 to skip."""
    if os.environ.get("MERKURIO_SYSTEM_HIP") == "1":
        return None
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if not spec or not spec.submodule_search_locations:
        return None
    path = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if not os.path.exists(path):
        return None
    return C.CDLL(path, mode=C.RTLD_GLOBAL)


def load(build_if_missing=True):
    """Loads the shared library (building it in-tree with hipcc first if needed)."""
    global _lib
    if _lib is not None:
        return _lib
    _bind_to_torch_hip_runtime()
    path = os.environ.get("MERKURIO_LIB_PATH") or _build.LIB_PATH  # override: A/B runs against another build
    if path == _build.LIB_PATH and build_if_missing and (
            not os.path.exists(path) or os.environ.get("MERKURIO_REBUILD") == "1"):
        _build.build_lib()  # a present library is used as is (the driver's build() step keeps it fresh)
    if not os.path.exists(path):
        raise MerkurioError(MK_E_HIP, f"{path} is missing: run `python -m merkurio_amd.build`")
    L = C.CDLL(path)
    L.mk_last_error.restype = C.c_char_p
    L.mk_matcher_kernel_name.restype = C.c_char_p
    L.mk_matcher_kernel_name.argtypes = [C.c_void_p]
    L.mk_tune_q_value.restype = C.c_size_t
    L.mk_tune_q_value.argtypes = [C.c_size_t]
    L.mk_recommend_aho_corasick.argtypes = [C.c_size_t, C.c_size_t]
    L.mk_free.argtypes = [C.c_void_p]
    L.mk_matcher_destroy.argtypes = [C.c_void_p]
    L.mk_matcher_algo.argtypes = [C.c_void_p]
    L.mk_matcher_algo.restype = C.c_uint32
    L.mk_matcher_num_patterns.argtypes = [C.c_void_p]
    L.mk_matcher_num_patterns.restype = C.c_uint32
    L.mk_matcher_create.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32,
                                    C.POINTER(C.c_void_p)]
    L.mk_matcher_create_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32,
                                       C.POINTER(MatcherOptions), C.POINTER(C.c_void_p)]
    L.mk_synth_reads_device_range.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                              C.c_void_p, C.c_void_p, C.c_void_p]
    L.mk_reduce_counters.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_size_t, C.c_void_p]
    L.mk_reduce_prepare.argtypes = [C.POINTER(C.c_void_p), C.c_int]
    L.mk_comm_unique_id.argtypes = [C.c_void_p]
    L.mk_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.mk_comm_reduce_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.mk_comm_destroy.argtypes = [C.c_void_p]
    L.mk_comm_size.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    L.mk_scan_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                C.c_uint64, C.POINTER(C.c_uint64)]
    L.mk_scan_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p,
                                 C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mk_order_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.mk_order_hits_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    L.mk_matcher_order_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.mk_matcher_launch_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.mk_scan_tile_geometry.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(TileGeometry)]
    L.mk_matcher_scan_geometry.argtypes = [C.c_void_p, C.POINTER(TileGeometry)]
    L.mk_matcher_enable_timing.argtypes = [C.c_void_p, C.c_uint32]
    L.mk_matcher_hint_hit_density.argtypes = [C.c_void_p, C.c_uint32]
    L.mk_matcher_hint_record_lengths.argtypes = [C.c_void_p, C.c_int]
    L.mk_matcher_set_fixed_record_length.argtypes = [C.c_void_p, C.c_uint32]
    L.mk_matcher_check_device.argtypes = [C.c_void_p, C.c_void_p]
    L.mk_matcher_batch_times.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mk_matcher_kernel_times.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
    L.mk_matcher_filter_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.mk_matcher_filter_mode.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.mk_plan_geometry.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(MatcherOptions)] + [C.POINTER(C.c_uint32)] * 7
    L.mk_matcher_class_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint32)]
    L.mk_extract_single.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_void_p,
                                    C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Counters), C.c_void_p]
    L.mk_extract_fastq_text.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Counters), C.c_void_p,
                                        C.POINTER(C.c_uint32)]
    L.mk_upload_text_ahead.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
    L.mk_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    L.mk_host_free.argtypes = [C.c_void_p]
    L.mk_host_free.restype = None
    L.mk_codec_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    L.mk_codec_destroy.argtypes = [C.c_void_p]
    L.mk_codec_destroy.restype = None
    L.mk_bgzf_deflate_bound.argtypes = [C.c_uint64, C.c_uint32]
    L.mk_bgzf_deflate_bound.restype = C.c_uint64
    L.mk_bgzf_deflate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mk_bgzf_deflate_pieces.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mk_bgzf_inflate.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mk_bgzf_members.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_uint64)]
    L.mk_bgzf_eof.restype = C.POINTER(C.c_uint8 * 28)
    L.mk_codec_times.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mk_codec_set_pass_limits.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64]
    L.mk_codec_set_gzip_chunk.argtypes = [C.c_void_p, C.c_uint64]
    L.mk_codec_set_inflate_kernel.argtypes = [C.c_void_p, C.c_int]
    L.mk_gzip_inflate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.mk_gzip_member_guesses.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mk_gzip_members_inflate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.mk_gzip_text_read.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
    L.mk_gzip_text_device.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mk_gzip_text_device.restype = C.c_void_p
    L.mk_gzip_text_release.argtypes = [C.c_void_p]
    L.mk_gzip_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    L.mk_bzip2_inflate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.mk_bzip2_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    L.mk_zstd_inflate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.mk_zstd_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    L.mk_xz_inflate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.mk_xz_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    L.mk_codec_set_xz_spread.argtypes = [C.c_void_p, C.c_uint32]
    L.mk_codec_set_bzip2_pass_blocks.argtypes = [C.c_void_p, C.c_uint64]
    L.mk_bzip2_stream_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
    L.mk_bzip2_stream_next.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.mk_bzip2_stream_info.argtypes = [C.c_void_p, C.POINTER(Bzip2StreamStats)]
    L.mk_bzip2_stream_end.argtypes = [C.c_void_p]
    L.mk_codec_set_bzip2_text_cap.argtypes = [C.c_void_p, C.c_uint64]
    L.mk_zstd_record_cuts.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mk_zstd_deflate_bound.argtypes = [C.c_uint64]
    L.mk_zstd_deflate_bound.restype = C.c_uint64
    L.mk_zstd_deflate_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64)]
    L.mk_zstd_deflate_info.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]
    L.mk_zstd_stream_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
    L.mk_zstd_stream_next.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.mk_zstd_stream_info.argtypes = [C.c_void_p, C.POINTER(ZstdStreamStats)]
    L.mk_zstd_stream_end.argtypes = [C.c_void_p]
    L.mk_codec_set_zstd_text_cap.argtypes = [C.c_void_p, C.c_uint64]
    L.mk_xz_stream_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
    L.mk_xz_stream_next.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.mk_xz_stream_info.argtypes = [C.c_void_p, C.POINTER(XzStreamStats)]
    L.mk_xz_stream_end.argtypes = [C.c_void_p]
    L.mk_codec_set_xz_text_cap.argtypes = [C.c_void_p, C.c_uint64]
    L.mk_gzip_stream_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32)]
    L.mk_gzip_stream_next.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.mk_gzip_stream_info.argtypes = [C.c_void_p, C.POINTER(GzipStreamStats)]
    L.mk_gzip_stream_end.argtypes = [C.c_void_p]
    L.mk_crc32_combine.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
    L.mk_crc32_combine.restype = C.c_uint32
    L.mk_extract_fastq_bgzf.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int,
                                        C.POINTER(WindowText), C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Counters), C.c_void_p, C.POINTER(C.c_uint32)]
    L.mk_extract_window.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_int, C.c_uint64, C.POINTER(C.c_uint64),
                                    C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.POINTER(C.c_uint32)]
    L.mk_extract_window_open.argtypes = L.mk_extract_window.argtypes + [C.c_void_p]  # (the same arguments, then the mk_window_front)
    L.mk_bgzf_record_cuts.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.mk_extract_window_members.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_uint64,
                                            C.POINTER(C.c_uint64), C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Counters),
                                            C.c_void_p, C.POINTER(C.c_uint32)]
    L.mk_extract_window_frames.argtypes = L.mk_extract_window_members.argtypes  # (the same arguments: zstd frames where members are)
    L.mk_bgzf_deflate_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64)]
    L.mk_codec_cut_times.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_float)]
    L.mk_matcher_order_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
    L.mk_tag_bam_window.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BamWindow), C.c_int, C.POINTER(Counters), C.c_void_p, C.POINTER(C.c_uint32)]
    L.mk_matcher_set_bam_piece.argtypes = [C.c_void_p, C.c_uint32]
    L.mk_tag_sam_window.argtypes = [C.c_void_p, C.POINTER(SamWindow), C.c_int, C.POINTER(Counters), C.c_void_p, C.POINTER(C.c_uint32)]
    L.mk_tag_sam_bam_window.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(SamBamWindow), C.c_int, C.POINTER(Counters), C.c_void_p, C.POINTER(C.c_uint32)]
    L.mk_tag_bam_sam_window.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(BamSamWindow), C.c_int, C.POINTER(Counters), C.c_void_p, C.POINTER(C.c_uint32)]
    L.mk_extract_paired.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                    C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                    C.POINTER(Counters), C.c_void_p]
    L.mk_tag_records.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(Counters), C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_uint64]
    L.mk_tag_value.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_char_p, C.c_size_t,
                               C.POINTER(C.c_size_t)]
    L.mk_synth_reads_device.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
    L.mk_synth_reads_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32,
                                      C.c_void_p, C.c_void_p]
    L.mk_read_kmers_from_text.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_uint32)]
    L.mk_parse_pattern_list.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint32)]
    L.mk_reverse_complement.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.mk_canonical.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p]
    L.mk_generate_masks.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint64)]
    _lib = L
    return L


def _check(rc):
    if rc == MK_OK:
        return
    msg = load().mk_last_error().decode(errors="replace")
    if rc in PatternError.KINDS:
        raise PatternError(rc, msg)
    raise MerkurioError(rc, msg)


def device_count():
    return load().mk_device_count()


# ------------------------------------------------------------------ packing helpers
def pack_list(items):
    items = [bytes(x) for x in items]
    off = np.zeros(len(items) + 1, dtype=np.uint32)
    if items:
        off[1:] = np.cumsum([len(x) for x in items])
    data = np.frombuffer(b"".join(items) + b"\0", dtype=np.uint8).copy()
    return data, off


def pack_records(seqs):
    seqs = [bytes(x) for x in seqs]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        off[1:] = np.cumsum([len(x) for x in seqs], dtype=np.uint64)
    data = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8).copy()
    return data, off


def _take_list(pb, po, n):
    L = load()
    off = np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_uint32)), shape=(n.value + 1,)).copy()
    total = int(off[-1])
    data = C.string_at(pb, total) if total else b""
    L.mk_free(pb)
    L.mk_free(po)
    return [data[off[i]:off[i + 1]] for i in range(n.value)]


# ------------------------------------------------------------------ pattern preparation
def read_kmers_from_text(content: bytes):
    """helpers::read_kmers_from_file body (src/helpers.rs:152-156)"""
    pb, po, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
    buf = np.frombuffer(bytes(content) + b"\0", dtype=np.uint8)
    _check(load().mk_read_kmers_from_text(buf.ctypes.data, len(content), C.byref(pb), C.byref(po), C.byref(n)))
    return _take_list(pb, po, n)


def read_kmers_from_file(path):
    with open(path, "rb") as f:
        return read_kmers_from_text(f.read())


def parse_pattern_list(kmer_file=None, kmer_seq=None, reverse_complement=False, canonical=False, lowercase=False,
                       uppercase=False):
    """helpers::parse_pattern_list (src/helpers.rs:76-133); the file has priority over kmer_seq"""
    if kmer_file is not None:
        raw = read_kmers_from_file(kmer_file)
    elif kmer_seq is not None:
        raw = [s.encode() if isinstance(s, str) else bytes(s) for s in kmer_seq]
    else:
        raise MerkurioError(MK_E_NO_PATTERNS, "No k-mer sequence provided.")
    data, off = pack_list(raw)
    pb, po, n = C.c_void_p(), C.c_void_p(), C.c_uint32()
    _check(load().mk_parse_pattern_list(data.ctypes.data, off.ctypes.data, len(raw), int(reverse_complement),
                                        int(canonical), int(lowercase), int(uppercase), C.byref(pb), C.byref(po),
                                        C.byref(n)))
    return _take_list(pb, po, n)


def reverse_complement(s: bytes) -> bytes:
    src = np.frombuffer(bytes(s) + b"\0", dtype=np.uint8)
    out = np.zeros(len(s) + 1, dtype=np.uint8)
    load().mk_reverse_complement(src.ctypes.data, len(s), out.ctypes.data)
    return out[:len(s)].tobytes()


def canonical(s: bytes) -> bytes:
    src = np.frombuffer(bytes(s) + b"\0", dtype=np.uint8)
    out = np.zeros(len(s) + 1, dtype=np.uint8)
    load().mk_canonical(src.ctypes.data, len(s), out.ctypes.data)
    return out[:len(s)].tobytes()


def recommend_aho_corasick(pattern_list) -> bool:
    return bool(load().mk_recommend_aho_corasick(len(pattern_list), max(len(p) for p in pattern_list)))


def tune_q_value(pattern) -> int:
    q = load().mk_tune_q_value(len(pattern))
    if q == 0:
        raise MerkurioError(MK_E_PATTERN_TOO_LONG, "Pattern length is too long for BNDMq.")
    return q


def generate_masks(pattern: bytes):
    src = np.frombuffer(bytes(pattern) + b"\0", dtype=np.uint8)
    masks = np.zeros(256, dtype=np.uint64)
    accept = C.c_uint64()
    _check(load().mk_generate_masks(src.ctypes.data, len(pattern), masks.ctypes.data, C.byref(accept)))
    return masks.tolist(), accept.value


def plan_geometry(lengths, options=None):
    """mk_plan_geometry: the filter geometry / length classes a matcher for patterns of these lengths would get"""
    lens = np.ascontiguousarray(lengths, dtype=np.uint32)
    opt = None if options is None else (options if isinstance(options, MatcherOptions) else MatcherOptions(**options))
    v = [C.c_uint32() for _ in range(7)]
    _check(load().mk_plan_geometry(lens.ctypes.data, len(lens), None if opt is None else C.byref(opt), *[C.byref(x) for x in v]))
    keys = ("q_gram", "stride", "in_lds", "split_len", "n_short", "q_gram2", "stride2")
    return dict(zip(keys, (x.value for x in v)))


def scan_tile_geometry(n_bytes, n_waves, tile_run):
    """mk_scan_tile_geometry: the two tile regions and the tail of a scan of n_bytes by n_waves waves (host arithmetic)"""
    g = TileGeometry()
    _check(load().mk_scan_tile_geometry(int(n_bytes), int(n_waves), int(tile_run), C.byref(g)))
    return g.as_dict()


# ------------------------------------------------------------------ matcher handle
class Matcher:
    """The matcher bundle the reference drivers hold (src/cmd_extract.rs:259): construction
    applies the reference's algorithm-selection rule; scans run on the GPU."""

    def __init__(self, patterns, algo=MK_ALGO_AUTO, q=0, case_insensitive=False, device=0, options=None):
        """options: None or a MatcherOptions / dict(force_stride=..., force_global_filter=...,
        gbloom_log2_blocks=...) -> mk_matcher_create_ex"""
        self.patterns = [p.encode() if isinstance(p, str) else bytes(p) for p in patterns]
        data, off = pack_list(self.patterns)
        self._h = C.c_void_p()
        flags = MK_FLAG_ASCII_CASE_INSENSITIVE if case_insensitive else 0
        if options is None:
            _check(load().mk_matcher_create(data.ctypes.data, off.ctypes.data, len(self.patterns), algo, q, flags,
                                            device, C.byref(self._h)))
        else:
            opt = options if isinstance(options, MatcherOptions) else MatcherOptions(**options)
            _check(load().mk_matcher_create_ex(data.ctypes.data, off.ctypes.data, len(self.patterns), algo, q, flags,
                                               device, C.byref(opt), C.byref(self._h)))
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            load().mk_matcher_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: the module globals are already gone
            pass

    @property
    def handle(self):
        return self._h

    @property
    def algo(self):
        return load().mk_matcher_algo(self._h)

    @property
    def use_ac(self):
        return self.algo == MK_ALGO_AC

    @property
    def kernel_name(self):
        return load().mk_matcher_kernel_name(self._h).decode()

    def launch_info(self):
        g, b, l = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(load().mk_matcher_launch_info(self._h, C.byref(g), C.byref(b), C.byref(l)))
        return {"grid_blocks": g.value, "block_threads": b.value, "lds_bytes": l.value}

    def scan_geometry(self):
        """tile geometry of the last mk_scan_device on this handle (mk_tile_geometry as a dict)"""
        g = TileGeometry()
        _check(load().mk_matcher_scan_geometry(self._h, C.byref(g)))
        return g.as_dict()

    def batch_times_ms(self):
        """upload / device / download / host milliseconds of the last extract_single / tag_records call"""
        ms = (C.c_float * 4)()
        _check(load().mk_matcher_batch_times(self._h, ms))
        return {"upload": ms[0], "device": ms[1], "download": ms[2], "host": ms[3]}

    def order_info(self):
        """what the last mk_order_hits_device did: path 0 nothing, 1 record bins, 2 (record, end) bins, 3 library sort"""
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(load().mk_matcher_order_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"path": a.value, "bins": b.value, "max_bin": c.value}

    def enable_timing(self, slots):
        _check(load().mk_matcher_enable_timing(self._h, slots))
        self._timing_slots = slots

    def kernel_times_ms(self):
        """durations of the retained scan-kernel launches (hipEvents on the launch stream)"""
        cap = max(1, getattr(self, "_timing_slots", 0))
        ms = np.zeros(cap, dtype=np.float32)
        n = C.c_uint32()
        _check(load().mk_matcher_kernel_times(self._h, ms.ctypes.data, cap, C.byref(n)))
        return ms[:n.value].tolist()

    def filter_info(self):
        q, s, e, tb = C.c_uint32(), C.c_uint32(), C.c_uint64(), C.c_uint64()
        _check(load().mk_matcher_filter_info(self._h, C.byref(q), C.byref(s), C.byref(e), C.byref(tb)))
        return {"q_gram": q.value, "stride": s.value, "entries": e.value, "table_bytes": tb.value}

    def class_info(self):
        """length classes (matcher.cpp: plan_classes): split_len 0 = one class"""
        a, b, c, d = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(load().mk_matcher_class_info(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"split_len": a.value, "n_short": b.value, "q_gram2": c.value, "stride2": d.value}

    def filter_mode(self):
        lds, fb = C.c_uint32(), C.c_uint64()
        _check(load().mk_matcher_filter_mode(self._h, C.byref(lds), C.byref(fb)))
        return {"in_lds": bool(lds.value), "filter_bytes": fb.value}

    def hint_hit_density(self, records_hit_per_1000):
        """performance hint for the next scan (never changes results): picks the load flavour of the kernel"""
        _check(load().mk_matcher_hint_hit_density(self._h, int(records_hit_per_1000)))

    # ---- batched scan, host buffers
    def scan(self, seqs, mode=MK_MODE_HITS, hits_cap=None):
        """-> (flags: np.bool_[n], hits: structured array in reference emission order)"""
        data, off = pack_records(seqs)
        return self.scan_packed(data, off, mode, hits_cap)

    def scan_packed(self, data, off, mode=MK_MODE_HITS, hits_cap=None):
        n = len(off) - 1
        flags = np.zeros(max(1, n), dtype=np.uint8)
        nh = C.c_uint64()
        cap = 1024 if hits_cap is None else hits_cap
        while True:
            hits = np.zeros(max(1, cap), dtype=HIT_DTYPE)
            rc = load().mk_scan_batch(self._h, data.ctypes.data, off.ctypes.data, n, mode, flags.ctypes.data,
                                      hits.ctypes.data, cap, C.byref(nh))
            if rc == MK_E_CAPACITY and hits_cap is None:
                cap = nh.value
                continue
            _check(rc)
            return flags[:n].astype(bool), hits[:nh.value]

    # ---- driver loops
    def _rows(self, call):
        cap = 4096
        while True:
            rows = np.zeros(cap, dtype=ROW_DTYPE)
            n_rows = C.c_uint64()
            rc = call(rows, cap, n_rows)
            if rc == MK_E_CAPACITY and n_rows.value > cap:
                cap = n_rows.value
                continue
            _check(rc)
            r = rows[:n_rows.value]
            return [(int(f), int(rec), int(p), int(pos)) for f, rec, p, pos in zip(r["file"], r["rec"], r["pat"], r["pos"])]

    def extract_single(self, seqs, logging=True, invert=False):
        data, off = pack_records(seqs)
        n = len(seqs)
        keep = np.zeros(max(1, n), dtype=np.uint8)
        res = {}

        def call(rows, cap, n_rows):
            res["c"], res["counts"] = Counters(), np.zeros(len(self.patterns), dtype=np.uint32)
            return load().mk_extract_single(self._h, data.ctypes.data, off.ctypes.data, n, int(logging), int(invert),
                                            keep.ctypes.data, rows.ctypes.data, cap, C.byref(n_rows),
                                            C.byref(res["c"]), res["counts"].ctypes.data)
        rows = self._rows(call)
        return keep[:n].astype(bool).tolist(), rows, res["c"].as_dict(res["counts"])

    def extract_fastq_text(self, text: bytes, logging=True, invert=False):
        """mk_extract_fastq_text: raw 4-line FASTQ text -> (status, rec_start list (n + 1), keep, rows, counters);
        status 1 = not plain FASTQ, the caller's own reader must take the window"""
        buf = np.frombuffer(text, dtype=np.uint8)
        cap = max(1, text.count(b"\n") // 4 + 2)
        n_rec, status = C.c_uint64(), C.c_uint32()
        rec_start = np.zeros(cap + 1, dtype=np.uint64)
        keep = np.zeros(cap, dtype=np.uint8)
        cnt = Counters()
        counts = np.zeros(len(self.patterns), dtype=np.uint32)
        rows = np.zeros(4096, dtype=ROW_DTYPE)
        n_rows = C.c_uint64()
        while True:
            c2, k2 = Counters(), np.zeros(len(self.patterns), dtype=np.uint32)
            rc = load().mk_extract_fastq_text(self._h, buf.ctypes.data if len(buf) else None, len(buf), int(logging), int(invert), cap,
                                              C.byref(n_rec), rec_start.ctypes.data, keep.ctypes.data, rows.ctypes.data, len(rows),
                                              C.byref(n_rows), C.byref(c2), k2.ctypes.data, C.byref(status))
            if rc == MK_E_CAPACITY and n_rows.value > len(rows):
                rows = np.zeros(n_rows.value, dtype=ROW_DTYPE)
                continue
            _check(rc)
            cnt, counts = c2, k2
            break
        n = n_rec.value
        out_rows = [(int(r["file"]), int(r["rec"]), int(r["pat"]), int(r["pos"])) for r in rows[:n_rows.value]] if logging else []
        return status.value, rec_start[:n + 1].tolist(), [bool(k) for k in keep[:n]], out_rows, cnt.as_dict(counts)

    def extract_fastq_bgzf(self, codec, head: bytes, blob: bytes, members, last, logging=True, invert=False, whole_text=True):
        """mk_extract_fastq_bgzf: head + the text of `members` (entries of bgzf_members(blob), out_off re-based to 0) ->
        (status, text, n_used, rec_start, keep, rows, counters); the members are inflated into the ingest buffer on the device.
        whole_text=False: `text` is a pair (tail, kept) -- the unfinished record at the window's end and the kept records' text"""
        mem = members.copy()
        if len(mem):
            mem["out_off"] -= mem["out_off"][0]
        n_text = len(head) + int(mem["isize"].sum()) if len(mem) else len(head)
        hb, bb = np.frombuffer(head, dtype=np.uint8), np.frombuffer(blob, dtype=np.uint8)
        text = np.zeros(max(1, n_text), dtype=np.uint8)
        tail = np.zeros(1 << 20, dtype=np.uint8)
        io = WindowText()
        if whole_text:
            io.text, io.text_cap = text.ctypes.data, n_text
        else:
            io.tail, io.tail_cap, io.kept, io.kept_cap = tail.ctypes.data, tail.size, text.ctypes.data, 64
        cap = max(1, n_text // 8 + 2)
        n_rec, status = C.c_uint64(), C.c_uint32()
        rec_start = np.zeros(cap + 1, dtype=np.uint64)
        keep = np.zeros(cap, dtype=np.uint8)
        rows = np.zeros(4096, dtype=ROW_DTYPE)
        n_rows = C.c_uint64()
        while True:
            c2, k2 = Counters(), np.zeros(len(self.patterns), dtype=np.uint32)
            rc = load().mk_extract_fastq_bgzf(self._h, codec._h, hb.ctypes.data if len(hb) else None, len(hb), bb.ctypes.data if len(bb) else None,
                                              len(bb), mem.ctypes.data if len(mem) else None, len(mem), int(bool(last)), C.byref(io), int(logging),
                                              int(invert), cap, C.byref(n_rec), rec_start.ctypes.data, keep.ctypes.data, rows.ctypes.data,
                                              len(rows), C.byref(n_rows), C.byref(c2), k2.ctypes.data, C.byref(status))
            if rc == MK_E_CAPACITY and n_rows.value > len(rows):
                rows = np.zeros(n_rows.value, dtype=ROW_DTYPE)
                continue
            if rc == MK_E_CAPACITY and not whole_text and io.n_kept_bytes > io.kept_cap:  # (the first call states the need: the retry path)
                io.kept_cap = io.n_kept_bytes
                continue
            _check(rc)
            break
        n = n_rec.value
        out_rows = [(int(r["file"]), int(r["rec"]), int(r["pat"]), int(r["pos"])) for r in rows[:n_rows.value]] if logging else []
        out_text = text[:io.n_text].tobytes() if whole_text else (tail[:io.n_tail].tobytes(), text[:io.n_kept_bytes].tobytes())
        return (status.value, out_text, io.n_used, rec_start[:n + 1].tolist(), [bool(k) for k in keep[:n]], out_rows, c2.as_dict(k2))

    @staticmethod
    def _window_sources(sources):
        """the mk_window_source array of extract_window's source dicts -> (array, what keeps its buffers alive, the longest window text)"""
        arr = (WindowSource * len(sources))()
        hold = []
        bound = 0
        for k, sd in enumerate(sources):
            S = arr[k]
            head = np.frombuffer(sd.get("head", b""), dtype=np.uint8)
            hold.append(head)
            S.head, S.n_head = (head.ctypes.data if head.size else None), head.size
            n_body = 0
            if "members" in sd:
                mem = sd["members"].copy()
                if len(mem):
                    mem["out_off"] -= mem["out_off"][0]
                blob = np.frombuffer(sd["blob"], dtype=np.uint8)
                hold += [mem, blob]
                S.bgzf, S.n_bgzf = (blob.ctypes.data if blob.size else None), blob.size
                S.members, S.n_members = (mem.ctypes.data if len(mem) else None), len(mem)
                n_body = int(mem["isize"].sum()) if len(mem) else 0
            elif "device_text" in sd:  # (pointer, bytes): a range of a text that lies on the device (mk_gzip_text_device)
                S.device_text, S.n_device_text = sd["device_text"]
                n_body = S.n_device_text
            else:
                text = np.frombuffer(sd.get("text", b""), dtype=np.uint8)
                hold.append(text)
                S.text, S.n_text = (text.ctypes.data if text.size else None), text.size
                n_body = text.size
            S.ends_at_record = int(bool(sd.get("ends_at_record", True)))
            bound = max(bound, head.size + n_body)
        return arr, hold, bound

    def extract_window(self, sources, fmt=MK_TEXT_FASTQ, logging=True, invert=False, codec=None, want=("tail",)):
        """mk_extract_window.  sources: one dict per input file (one = single, two = paired) with keys
             head (bytes, default b""), text (bytes) OR blob + members (bgzf_members entries), ends_at_record (bool)
        want: which texts come back per source, any of "tail", "kept", "all".
        -> dict(status, n_rec, keep, rows, counters, sources=[dict(n_window, n_used, n_rec_seen, rec_start, tail, kept, all)])"""
        return self._extract_window_text(sources, fmt, logging, invert, codec, want, None)

    def extract_window_open(self, sources, fmt=MK_TEXT_FASTQ, logging=True, invert=False, codec=None, want=("tail",), front_cap=None):
        """mk_extract_window_open: extract_window on ONE source without a head whose text may begin anywhere -- the call finds the first
        record start (the start rule of include/merkurio_hip.h) and processes the records from there.  front_cap: None = grow the
        buffer to what the call names and ask again; a number = taken as it is (MK_E_CAPACITY is raised, the error's n_front = the need).
        -> extract_window's dict plus n_front and front (bytes: the text in front of the found start; b"" when status is 2, where
           n_front = n_window).  rec_start, n_used and the tail's place stay offsets in the whole window text."""
        return self._extract_window_text(sources, fmt, logging, invert, codec, want, 64 if front_cap is None else ("fixed", int(front_cap)))

    def _extract_window_text(self, sources, fmt, logging, invert, codec, want, front):
        L = load()
        n_src = len(sources)
        arr, hold, bound = self._window_sources(sources)
        cap = max(1, bound // (2 if fmt == MK_TEXT_FASTA else 8) + 2)
        bufs = []
        for k in range(n_src):
            S = arr[k]
            b = {"rec_start": np.zeros(cap + 1, dtype=np.uint64), "tail": np.zeros(64, dtype=np.uint8), "kept": np.zeros(64, dtype=np.uint8),
                 "all": np.zeros(max(1, bound), dtype=np.uint8)}
            bufs.append(b)
            S.rec_start = b["rec_start"].ctypes.data
            if "tail" in want:
                S.tail, S.tail_cap = b["tail"].ctypes.data, b["tail"].size
            if "kept" in want:
                S.kept, S.kept_cap = b["kept"].ctypes.data, b["kept"].size
            if "all" in want:
                S.all, S.all_cap = b["all"].ctypes.data, b["all"].size
        n_rec, status, n_rows = C.c_uint64(), C.c_uint32(), C.c_uint64()
        keep = np.zeros(cap, dtype=np.uint8)
        rows = np.zeros(4096, dtype=ROW_DTYPE)
        F, front_buf, front_grows = WindowFront(), None, False
        if front is not None:
            front_grows = not isinstance(front, tuple)
            front_buf = np.zeros(max(1, front if front_grows else front[1]), dtype=np.uint8)
            F.front, F.front_cap = front_buf.ctypes.data, (front_buf.size if front_grows else front[1])
        for _ in range(8):
            c2, k2 = Counters(), np.zeros(len(self.patterns), dtype=np.uint32)
            args = (self._h, codec._h if codec else None, fmt, n_src, arr, int(logging), int(invert), cap, C.byref(n_rec),
                    keep.ctypes.data, rows.ctypes.data, len(rows), C.byref(n_rows), C.byref(c2), k2.ctypes.data, C.byref(status))
            rc = L.mk_extract_window(*args) if front is None else L.mk_extract_window_open(*args, C.addressof(F))
            if rc == MK_E_CAPACITY:  # the call states every need: grow what was too small and ask again
                grown = False
                if front is not None and F.n_front > F.front_cap:
                    if not front_grows:
                        err = MerkurioError(rc, L.mk_last_error().decode())
                        err.n_front = F.n_front
                        raise err
                    front_buf = np.zeros(F.n_front, dtype=np.uint8)
                    F.front, F.front_cap = front_buf.ctypes.data, front_buf.size
                    grown = True
                if n_rows.value > len(rows):
                    rows = np.zeros(n_rows.value, dtype=ROW_DTYPE)
                    grown = True
                for k in range(n_src):
                    S, b = arr[k], bufs[k]
                    if "tail" in want and S.n_tail > S.tail_cap:
                        b["tail"] = np.zeros(S.n_tail, dtype=np.uint8)
                        S.tail, S.tail_cap = b["tail"].ctypes.data, b["tail"].size
                        grown = True
                    if "kept" in want and S.n_kept_bytes > S.kept_cap:
                        b["kept"] = np.zeros(S.n_kept_bytes, dtype=np.uint8)
                        S.kept, S.kept_cap = b["kept"].ctypes.data, b["kept"].size
                        grown = True
                if grown:
                    continue
            _check(rc)
            break
        n = n_rec.value
        out = {"status": status.value, "n_rec": n, "keep": [bool(x) for x in keep[:n]],
               "rows": [(int(r["file"]), int(r["rec"]), int(r["pat"]), int(r["pos"])) for r in rows[:n_rows.value]] if logging else [],
               "counters": c2.as_dict(k2), "sources": []}
        if front is not None:
            out["n_front"] = F.n_front
            out["front"] = front_buf[:F.n_front].tobytes() if status.value != 2 else b""
        for k in range(n_src):
            S, b = arr[k], bufs[k]
            out["sources"].append({"n_window": S.n_window, "n_used": S.n_used, "n_rec_seen": S.n_rec_seen,
                                   "rec_start": b["rec_start"][:n + 1].tolist() if not status.value else [],
                                   "tail": b["tail"][:S.n_tail].tobytes() if "tail" in want else None,
                                   "kept": b["kept"][:S.n_kept_bytes].tobytes() if "kept" in want else None,
                                   "all": b["all"][:S.n_window].tobytes() if "all" in want else None})
        return out

    def extract_window_members(self, sources, codec, fmt=MK_TEXT_FASTQ, logging=False, invert=False, text_below=0, caps=None):
        """mk_extract_window_members: mk_extract_window whose kept records come back as BGZF members of their written form, one
        stream per source.  sources: as extract_window.  caps: None = grow what the call names and ask again; else
        dict(members=..., ids=...) taken as they are (MK_E_CAPACITY is raised).
        -> extract_window's dict (sources: n_window, n_used, n_rec_seen, rec_start, tail) plus per source
           members (bytes: the members, or the text when as_text), n_members, n_written, n_kept, as_text, ids (bytes), id_end (list),
           written_ms"""
        return self._extract_window_packed(load().mk_extract_window_members, sources, codec, fmt, logging, invert, text_below, caps)

    def extract_window_frames(self, sources, codec, fmt=MK_TEXT_FASTQ, logging=False, invert=False, text_below=0, caps=None):
        """mk_extract_window_frames: the same call with zstd frames where the members are (the frames of Codec.zstd_records on the
        written text and its record ends).  Arguments and the dictionary as extract_window_members: `members` holds the frames back to
        back, n_members is how many there are; Codec.zstd_records_info reports the call's frames, block kinds and milliseconds."""
        return self._extract_window_packed(load().mk_extract_window_frames, sources, codec, fmt, logging, invert, text_below, caps)

    def _extract_window_packed(self, entry, sources, codec, fmt, logging, invert, text_below, caps):
        n_src = len(sources)
        arr, hold, bound = self._window_sources(sources)
        cap = max(1, bound // (2 if fmt == MK_TEXT_FASTA else 8) + 2)
        mem = (WindowMembers * n_src)()
        bufs = []
        for k in range(n_src):
            b = {"rec_start": np.zeros(cap + 1, dtype=np.uint64), "tail": np.zeros(max(64, bound), dtype=np.uint8),
                 "members": np.zeros((caps or {}).get("members", 65536), dtype=np.uint8), "ids": np.zeros((caps or {}).get("ids", 4096), dtype=np.uint8),
                 "id_end": np.zeros(cap, dtype=np.uint64)}
            bufs.append(b)
            arr[k].rec_start = b["rec_start"].ctypes.data
            arr[k].tail, arr[k].tail_cap = b["tail"].ctypes.data, b["tail"].size
            M = mem[k]
            M.members, M.members_cap = (b["members"].ctypes.data if b["members"].size else None), b["members"].size
            M.ids, M.ids_cap = (b["ids"].ctypes.data if b["ids"].size else None), b["ids"].size
            M.id_end, M.text_below = b["id_end"].ctypes.data, int(text_below)
        n_rec, status, n_rows = C.c_uint64(), C.c_uint32(), C.c_uint64()
        keep = np.zeros(cap, dtype=np.uint8)
        rows = np.zeros(4096, dtype=ROW_DTYPE)
        for _ in range(8):
            c2, k2 = Counters(), np.zeros(len(self.patterns), dtype=np.uint32)
            rc = entry(self._h, codec._h if codec else None, fmt, n_src, arr, mem, int(logging), int(invert), cap, C.byref(n_rec),
                       keep.ctypes.data, rows.ctypes.data, len(rows), C.byref(n_rows), C.byref(c2), k2.ctypes.data, C.byref(status))
            if rc == MK_E_CAPACITY and caps is None:
                grown = False
                if n_rows.value > len(rows):
                    rows = np.zeros(n_rows.value, dtype=ROW_DTYPE)
                    grown = True
                for k in range(n_src):
                    M, b = mem[k], bufs[k]
                    if M.n_member_bytes > M.members_cap:
                        b["members"] = np.zeros(M.n_member_bytes, dtype=np.uint8)
                        M.members, M.members_cap = b["members"].ctypes.data, b["members"].size
                        grown = True
                    if M.n_id_bytes > M.ids_cap:
                        b["ids"] = np.zeros(M.n_id_bytes, dtype=np.uint8)
                        M.ids, M.ids_cap = b["ids"].ctypes.data, b["ids"].size
                        grown = True
                if grown:
                    continue
            _check(rc)
            break
        n = n_rec.value
        out = {"status": status.value, "n_rec": n, "keep": [bool(x) for x in keep[:n]],
               "rows": [(int(r["file"]), int(r["rec"]), int(r["pat"]), int(r["pos"])) for r in rows[:n_rows.value]] if logging else [],
               "counters": c2.as_dict(k2), "sources": []}
        for k in range(n_src):
            S, M, b = arr[k], mem[k], bufs[k]
            out["sources"].append({"n_window": S.n_window, "n_used": S.n_used, "n_rec_seen": S.n_rec_seen,
                                   "rec_start": b["rec_start"][:n + 1].tolist() if not status.value else [],
                                   "tail": b["tail"][:S.n_tail].tobytes(), "members": b["members"][:M.n_member_bytes].tobytes(),
                                   "n_members": M.n_members, "n_written": M.n_written, "n_kept": M.n_kept, "as_text": bool(M.as_text),
                                   "ids": b["ids"][:M.n_id_bytes].tobytes(), "id_end": b["id_end"][:M.n_kept].tolist() if logging else [],
                                   "written_ms": float(M.written_ms)})
        return out

    def extract_paired(self, seqs1, seqs2, logging=True, invert=False):
        d1, o1 = pack_records(seqs1)
        d2, o2 = pack_records(seqs2)
        n = len(seqs1)
        keep = np.zeros(max(1, n), dtype=np.uint8)
        res = {}

        def call(rows, cap, n_rows):
            res["c"], res["counts"] = Counters(), np.zeros(len(self.patterns), dtype=np.uint32)
            return load().mk_extract_paired(self._h, d1.ctypes.data, o1.ctypes.data, len(seqs1), d2.ctypes.data,
                                            o2.ctypes.data, len(seqs2), int(logging), int(invert), keep.ctypes.data,
                                            rows.ctypes.data, cap, C.byref(n_rows), C.byref(res["c"]),
                                            res["counts"].ctypes.data)
        rows = self._rows(call)
        return keep[:n].astype(bool).tolist(), rows, res["c"].as_dict(res["counts"])

    def tag_records(self, seqs, logging=True, filter_matching=False, invert=False):
        data, off = pack_records(seqs)
        n = len(seqs)
        keep = np.zeros(max(1, n), dtype=np.uint8)
        foff = np.zeros(n + 1, dtype=np.uint64)
        res = {"fcap": 4096}

        def call(rows, cap, n_rows):
            while True:
                res["c"], res["counts"] = Counters(), np.zeros(len(self.patterns), dtype=np.uint32)
                res["fpat"] = np.zeros(res["fcap"], dtype=np.uint32)
                rc = load().mk_tag_records(self._h, data.ctypes.data, off.ctypes.data, n, int(logging),
                                           int(filter_matching), int(invert), keep.ctypes.data, rows.ctypes.data, cap,
                                           C.byref(n_rows), C.byref(res["c"]), res["counts"].ctypes.data,
                                           foff.ctypes.data, res["fpat"].ctypes.data, res["fcap"])
                if rc == MK_E_CAPACITY and int(foff[n]) > res["fcap"]:
                    res["fcap"] = int(foff[n])
                    continue
                return rc
        rows = self._rows(call)
        found = [res["fpat"][int(foff[i]):int(foff[i + 1])].tolist() for i in range(n)]
        return keep[:n].astype(bool).tolist(), rows, res["c"].as_dict(res["counts"]), found

    def _tag_window(self, w, fn, handles, n_text, logging, write, out_cap=None, guard=0):
        """What the four tag_*_window wrappers share.  w: the window struct with its input fields set; fn(*handles, w, ...): its entry
        point.  Gives the call a tail of n_text bytes, an output buffer (write) and rows / names, and repeats a call that asks for more
        room -- but not for more output than a given out_cap: that call's MK_E_CAPACITY comes back as rc, with `guard` bytes of 0xA5
        behind the buffer as they are afterwards.  -> (the result keys all four have, rc, guard)"""
        tail = np.zeros(max(64, n_text), dtype=np.uint8)
        w.tail, w.tail_cap = tail.ctypes.data, tail.size
        fixed = out_cap is not None
        cap = out_cap if fixed else 1 << 16
        out = np.full(max(1, cap + guard), 0xA5, dtype=np.uint8)
        rows = np.zeros(4096, dtype=ROW_DTYPE)
        row_name = np.zeros(4096, dtype=np.uint64)
        names = np.zeros(1 << 16, dtype=np.uint8)
        status = C.c_uint32()
        while True:
            if write:
                w.out, w.out_cap = out.ctypes.data, cap
            w.rows, w.rows_cap, w.row_name, w.names, w.names_cap = rows.ctypes.data, len(rows), row_name.ctypes.data, names.ctypes.data, names.size
            c2, k2 = Counters(), np.zeros(len(self.patterns), dtype=np.uint32)
            rc = fn(*handles, C.byref(w), int(logging), C.byref(c2), k2.ctypes.data, C.byref(status))
            if rc == MK_E_CAPACITY and (w.n_rows > len(rows) or w.n_names_bytes > names.size or (w.out_len > cap and not fixed)):
                if w.n_rows > len(rows):
                    rows, row_name = np.zeros(w.n_rows, dtype=ROW_DTYPE), np.zeros(w.n_rows, dtype=np.uint64)
                if w.n_names_bytes > names.size:
                    names = np.zeros(w.n_names_bytes, dtype=np.uint8)
                if w.out_len > cap and not fixed:
                    cap = w.out_len
                    out = np.full(cap + guard, 0xA5, dtype=np.uint8)
                continue
            if not (fixed and rc == MK_E_CAPACITY):
                _check(rc)
            break
        nb = names[:w.n_names_bytes].tobytes()
        out_rows = []
        if logging and status.value == 0 and rc == MK_OK:
            for k in range(w.n_rows):
                a = int(row_name[k])
                out_rows.append((nb[a:nb.index(b"\0", a)], int(rows[k]["rec"]), int(rows[k]["pat"]), int(rows[k]["pos"])))
        res = dict(status=status.value, n_window=w.n_window, n_used=w.n_used, n_rec=w.n_rec, n_kept=w.n_kept, tail=tail[:w.n_tail].tobytes(),
                   out=out[:min(w.out_len, cap)].tobytes() if rc == MK_OK else b"", rows=out_rows, counters=c2.as_dict(k2), ms=list(w.ms))
        return res, rc, out[cap:cap + guard].tobytes()

    # The input fields of a window struct, by what the struct has.  Each returns the arrays the struct points into: they must outlive the call.
    def _window_common(self, w, head, last, tag, filter_matching, invert):
        hb = np.frombuffer(head, dtype=np.uint8)
        w.head, w.n_head = (hb.ctypes.data if len(hb) else None), len(hb)
        w.last, w.filter_matching, w.invert = int(bool(last)), int(bool(filter_matching)), int(bool(invert))
        w.tag[0], w.tag[1] = tag[0], tag[1]
        return [hb]

    def _window_members(self, w, blob, members, piece_bytes):
        """`members` re-based to the first one's text -> (the arrays, bytes of text)"""
        mem = members.copy()
        if len(mem):
            mem["out_off"] -= mem["out_off"][0]
        bb = np.frombuffer(blob, dtype=np.uint8)
        _check(load().mk_matcher_set_bam_piece(self._h, piece_bytes))
        w.bgzf, w.n_bgzf = (bb.ctypes.data if len(bb) else None), len(bb)
        w.members, w.n_members = (mem.ctypes.data if len(mem) else None), len(mem)
        return [mem, bb], int(mem["isize"].sum()) if len(mem) else 0

    def _window_text(self, w, text):
        tb = np.frombuffer(text, dtype=np.uint8)
        w.text, w.n_text = (tb.ctypes.data if len(tb) else None), len(tb)
        return [tb], len(tb)

    def _window_refs(self, w, refs):
        ref_bytes = np.frombuffer(b"".join(refs) + b"\0", dtype=np.uint8)
        ref_off = np.zeros(len(refs) + 1, dtype=np.uint64)
        ref_off[1:] = np.cumsum([len(r) for r in refs], dtype=np.uint64)
        w.ref_names, w.ref_off, w.n_refs = ref_bytes.ctypes.data, ref_off.ctypes.data, len(refs)
        return [ref_bytes, ref_off]

    def tag_bam_window(self, codec, head: bytes, blob: bytes, members, last, tag=b"km", logging=True, filter_matching=False, invert=False,
                       write=True, block_bytes=0, piece_bytes=0):
        """mk_tag_bam_window: head + the text of `members` (entries of bgzf_members(blob), out_off re-based to 0) as BAM records ->
        dict(status, n_window, n_used, n_rec, n_kept, tail, out (BGZF members of the tagged kept records), out_text_bytes, rows
        [(name, rec, pat, pos)], counters, ms)"""
        w = BamWindow()
        hold = self._window_common(w, head, last, tag, filter_matching, invert)
        held, n_body = self._window_members(w, blob, members, piece_bytes)
        w.block_bytes = block_bytes
        res, _, _ = self._tag_window(w, load().mk_tag_bam_window, (self._h, codec._h), len(head) + n_body, logging, write)
        return dict(res, out_text_bytes=w.out_text_bytes)

    def tag_sam_window(self, head: bytes, text: bytes, last, tag=b"km", logging=True, filter_matching=False, invert=False, write=True):
        """mk_tag_sam_window: head + text as SAM lines -> dict(status, n_window, n_used, n_rec, n_kept, tail, out (the kept lines with
        their tag field appended), rows [(name, rec, pat, pos)], counters, ms)"""
        w = SamWindow()
        hold = self._window_common(w, head, last, tag, filter_matching, invert)
        held, n_body = self._window_text(w, text)
        res, _, _ = self._tag_window(w, load().mk_tag_sam_window, (self._h,), len(head) + n_body, logging, write)
        return dict(res, out=res["out"] if write else b"")

    def tag_sam_bam_window(self, codec, head: bytes, text: bytes, last, refs=(), tag=b"km", logging=True, filter_matching=False, invert=False,
                           write=True, block_bytes=0):
        """mk_tag_sam_bam_window: head + text as SAM lines, `refs` = the reference names (bytes) in header order -> dict(status, n_window,
        n_used, n_rec, n_kept, tail, out (BGZF members of the kept lines as tagged BAM records), out_text_bytes, rows [(name, rec, pat,
        pos)], counters, ms)"""
        w = SamBamWindow()
        hold = self._window_common(w, head, last, tag, filter_matching, invert) + self._window_refs(w, refs)
        held, n_body = self._window_text(w, text)
        w.block_bytes = block_bytes
        res, _, _ = self._tag_window(w, load().mk_tag_sam_bam_window, (self._h, codec._h), len(head) + n_body, logging, write)
        return dict(res, out=res["out"] if write else b"", out_text_bytes=w.out_text_bytes)

    def tag_bam_sam_window(self, codec, head: bytes, blob: bytes, members, last, refs=(), tag=b"km", logging=True, filter_matching=False, invert=False,
                           write=True, piece_bytes=0, out_cap=None, guard=0):
        """mk_tag_bam_sam_window: head + the text of `members` (entries of bgzf_members(blob), out_off re-based to 0) as BAM records, `refs`
        = the reference names (bytes) in header order -> dict(status, rc, n_window, n_used, n_rec, n_kept, tail, out (the kept records as SAM
        lines with their tag field appended), out_len, rows [(name, rec, pat, pos)], counters, ms).  out_cap: the output buffer is exactly
        that large and a call that asks for more is NOT repeated (rc = MK_E_CAPACITY is returned); `guard` bytes of 0xA5 lie behind it and
        come back as `guard`."""
        w = BamSamWindow()
        hold = self._window_common(w, head, last, tag, filter_matching, invert) + self._window_refs(w, refs)
        held, n_body = self._window_members(w, blob, members, piece_bytes)
        res, rc, guard_bytes = self._tag_window(w, load().mk_tag_bam_sam_window, (self._h, codec._h), len(head) + n_body, logging, write, out_cap, guard)
        return dict(res, rc=rc, out=res["out"] if write else b"", out_len=w.out_len, guard=guard_bytes)

    def tag_value(self, found, existing=None) -> bytes:
        arr = np.asarray(list(found) + [0], dtype=np.uint32)
        cap = 256
        while True:
            out = C.create_string_buffer(cap)
            n = C.c_size_t()
            rc = load().mk_tag_value(self._h, arr.ctypes.data, len(found), existing, out, cap, C.byref(n))
            if rc == MK_E_CAPACITY:
                cap = n.value + 1
                continue
            _check(rc)
            return out.value


def reduce_counters(matchers, d_counter_ptrs, length):
    """mk_reduce_counters: in-place RCCL all-reduce (sum) of one device counter vector per handle
    (single process, one handle per GPU; handles sharing a device are pre-summed there).
    d_counter_ptrs: device addresses (ints).  Returns the sum as a numpy uint64 array."""
    n = len(matchers)
    hs = (C.c_void_p * n)(*[m.handle for m in matchers])
    ps = (C.c_void_p * n)(*[C.c_void_p(int(p)) for p in d_counter_ptrs])
    out = np.zeros(length, dtype=np.uint64)
    _check(load().mk_reduce_counters(hs, n, ps, length, out.ctypes.data))
    return out


# ------------------------------------------------------------------ reference-shaped single matchers
class BNDMq:
    """pattern_matching::BNDMq (src/pattern_matching.rs:42-153): one pattern, q-gram length q.
    q is validated like the reference and has no effect on results."""

    def __init__(self, pattern: bytes, q: int, device=0):
        if len(pattern) == 0:
            raise PatternError(MK_E_EMPTY_PATTERN, "Pattern is empty.")
        if q == 0:
            raise PatternError(MK_E_INVALID_Q, "Invalid q-gram length: 0. Must be between 1 and pattern length.")
        self._m = Matcher([pattern], MK_ALGO_BNDMQ, q, False, device)

    def find_all(self, text: bytes):
        _, hits = self._m.scan([text], MK_MODE_HITS)
        return hits["pos"].tolist()

    def find_iter(self, text: bytes):
        return iter(self.find_all(text))

    def find_match(self, text: bytes) -> bool:
        flags, _ = self._m.scan([text], MK_MODE_ANY)
        return bool(flags[0])


class AhoCorasick:
    """AhoCorasick::builder().kind(DFA).ascii_case_insensitive(ci).build(patterns) with the
    overlapping iterator (src/cmd_extract.rs:260-265,332)."""

    def __init__(self, patterns, ascii_case_insensitive=False, device=0):
        self._m = Matcher(patterns, MK_ALGO_AC, 0, ascii_case_insensitive, device)

    def find_overlapping_iter(self, text: bytes):
        """yields (pattern_index, start) in the crate's emission order"""
        _, hits = self._m.scan([text], MK_MODE_HITS)
        return iter(list(zip(hits["pat"].tolist(), hits["pos"].tolist())))

    def is_match(self, text: bytes) -> bool:
        flags, _ = self._m.scan([text], MK_MODE_ANY)
        return bool(flags[0])


# ---- BGZF codec (include/merkurio_hip.h v5; the reference's `bam` reader / writer, src/cmd_tag.rs:254-271,503-506) ----
MEMBER_DTYPE = np.dtype([("data_off", "<u8"), ("out_off", "<u8"), ("data_len", "<u4"), ("isize", "<u4"), ("crc", "<u4"), ("reserved", "<u4")])


def bgzf_members(data):
    """mk_bgzf_members: the member table of a BGZF byte string (host code) -> (members, consumed bytes, text bytes)"""
    L = load()
    buf = np.frombuffer(data, dtype=np.uint8)
    n, used, text = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _check(L.mk_bgzf_members(buf.ctypes.data if buf.size else None, buf.size, None, 0, C.byref(n), C.byref(used), C.byref(text)))
    mem = np.zeros(n.value, dtype=MEMBER_DTYPE)
    _check(L.mk_bgzf_members(buf.ctypes.data if buf.size else None, buf.size, mem.ctypes.data, mem.size, C.byref(n), C.byref(used), C.byref(text)))
    return mem, used.value, text.value


GUESS_DTYPE = np.dtype([("header_off", "<u8"), ("data_off", "<u8"), ("crc", "<u4"), ("isize", "<u4")])


def gzip_member_guesses(data):
    """mk_gzip_member_guesses: every offset of a gzip byte string at which an RFC 1952 header parses (host code) -> table of
    header_off, data_off and the crc / isize in front of the next guess.  Guesses, not members: the device proves them"""
    L = load()
    buf = np.frombuffer(data, dtype=np.uint8)
    n = C.c_uint64(0)
    _check(L.mk_gzip_member_guesses(buf.ctypes.data if buf.size else None, buf.size, None, 0, C.byref(n)))
    table = np.zeros(n.value, dtype=GUESS_DTYPE)
    _check(L.mk_gzip_member_guesses(buf.ctypes.data if buf.size else None, buf.size, table.ctypes.data if table.size else None, table.size, C.byref(n)))
    return table


def bgzf_eof():
    return bytes(load().mk_bgzf_eof().contents)


ZSTD_CUT_GRID, ZSTD_FRAME_TEXT_MAX = 114688, 131072


def zstd_record_cuts(rec_end):
    """mk_zstd_record_cuts (host code): where the zstd frames of a text end whose records end at rec_end -- the rule of
    bgzf_record_cuts with MK_ZSTD_CUT_GRID and MK_ZSTD_FRAME_TEXT_MAX -> the cuts, from 0 to the text's end"""
    L = load()
    ends = np.ascontiguousarray(rec_end, dtype=np.uint64)
    total = int(ends[-1]) if ends.size else 0
    cut = np.empty(total // ZSTD_CUT_GRID + 3, dtype=np.uint64)
    n = C.c_uint64(0)
    _check(L.mk_zstd_record_cuts(ends.ctypes.data if ends.size else None, ends.size, cut.ctypes.data, cut.size, C.byref(n)))
    return cut[:n.value].copy()


def bgzf_record_cuts(rec_end):
    """mk_bgzf_record_cuts (host code): where the members of a text end whose records end at rec_end -- the cut rule of
    include/merkurio_hip.h -> uint64 array, first 0, last rec_end[-1] (no records: [0])"""
    L = load()
    ends = np.ascontiguousarray(rec_end, dtype=np.uint64)
    total = int(ends[-1]) if ends.size else 0
    cut = np.zeros((total + BGZF_CUT_GRID - 1) // BGZF_CUT_GRID + 1, dtype=np.uint64)
    n = C.c_uint64(0)
    _check(L.mk_bgzf_record_cuts(ends.ctypes.data if ends.size else None, ends.size, cut.ctypes.data, cut.size, C.byref(n)))
    return cut[:n.value].copy()


def _stats_dict(st):
    """a mk_*_stream_stats as a dict, its times rounded"""
    out = {k: getattr(st, k) for k, _ in st._fields_ if k not in ("ms", "reserved")}
    out["ms"] = tuple(round(x, 2) for x in st.ms)
    return out


# what Codec._stream is told of a format: its four entries, its stats struct, the setter of its text cap (or None), and whether
# mk_*_stream_info names a refusal at _begin (then stream_stats is set for a file that was not taken, too)
_StreamCalls = collections.namedtuple("_StreamCalls", "begin next info end stats set_text_cap refusal_in_stats")


def _stream_calls(fmt, stats, set_text_cap=None, refusal_in_stats=False):
    return _StreamCalls(*("mk_%s_stream_%s" % (fmt, e) for e in ("begin", "next", "info", "end")), stats, set_text_cap, refusal_in_stats)


_GZIP_STREAM = _stream_calls("gzip", GzipStreamStats)
_BZIP2_STREAM = _stream_calls("bzip2", Bzip2StreamStats)
_ZSTD_STREAM = _stream_calls("zstd", ZstdStreamStats, "mk_codec_set_zstd_text_cap")
_XZ_STREAM = _stream_calls("xz", XzStreamStats, "mk_codec_set_xz_text_cap", True)


class Codec:
    """mk_codec: BGZF members deflated / inflated by the gfx950 kernels (no CPU path: without a device creation raises)"""

    def __init__(self, device=0):
        self._h = None
        self._L = load()
        h = C.c_void_p()
        _check(self._L.mk_codec_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if self._h:
            self._L.mk_codec_destroy(self._h)
            self._h = None

    __del__ = close

    def deflate(self, data, block_bytes=0):
        src = np.frombuffer(data, dtype=np.uint8)
        out = np.empty(self._L.mk_bgzf_deflate_bound(src.size, block_bytes), dtype=np.uint8)
        n = C.c_uint64(0)
        t0 = time.perf_counter()
        rc = self._L.mk_bgzf_deflate(self._h, src.ctypes.data if src.size else None, src.size, block_bytes,
                                     out.ctypes.data if out.size else None, out.size, C.byref(n))
        self.last_call_s = time.perf_counter() - t0  # (the C call alone: not this wrapper's buffer and bytes-object copies)
        _check(rc)
        return out[:n.value].tobytes()

    def deflate_pieces(self, pieces, block_bytes=0):
        """mk_bgzf_deflate_pieces: the members of b"".join(pieces), which is never formed on the host"""
        arrs = [np.frombuffer(p, dtype=np.uint8) for p in pieces]
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data if a.size else None for a in arrs])
        sizes = (C.c_uint64 * len(arrs))(*[a.size for a in arrs])
        total = sum(a.size for a in arrs)
        out = np.empty(self._L.mk_bgzf_deflate_bound(total, block_bytes), dtype=np.uint8)
        n = C.c_uint64(0)
        _check(self._L.mk_bgzf_deflate_pieces(self._h, ptrs, sizes, len(arrs), block_bytes, out.ctypes.data if out.size else None, out.size,
                                              C.byref(n)))
        return out[:n.value].tobytes()

    def deflate_records(self, text, rec_end, out_cap=None):
        """mk_bgzf_deflate_records: BGZF members of `text` that end at record ends (rec_end[-1] == len(text)), cut and deflated on the
        device.  out_cap (tests): the output buffer's size; too small raises MK_E_CAPACITY with self.last_need = the exact need.
        self.last_members = how many members there are"""
        src = np.frombuffer(text, dtype=np.uint8)
        ends = np.ascontiguousarray(rec_end, dtype=np.uint64)
        if out_cap is None:
            out_cap = src.size + 31 * ((src.size + BGZF_CUT_GRID - 1) // BGZF_CUT_GRID)  # every member stored
        out = np.empty(out_cap, dtype=np.uint8)
        n, members = C.c_uint64(0), C.c_uint64(0)
        t0 = time.perf_counter()
        rc = self._L.mk_bgzf_deflate_records(self._h, src.ctypes.data if src.size else None, src.size, ends.ctypes.data if ends.size else None, ends.size,
                                             out.ctypes.data if out.size else None, out.size, C.byref(n), C.byref(members))
        self.last_call_s = time.perf_counter() - t0
        self.last_need, self.last_members = n.value, members.value
        _check(rc)
        return out[:n.value].tobytes()

    def zstd_records(self, text, rec_end, out_cap=None):
        """mk_zstd_deflate_records: zstd frames of `text` that end at record ends (rec_end[-1] == len(text)), cut and compressed on the
        device, one frame per cut.  out_cap (tests): the output buffer's size; too small raises MK_E_CAPACITY with self.last_need = the
        exact need.  self.last_frames = how many frames there are"""
        src = np.frombuffer(text, dtype=np.uint8)
        ends = np.ascontiguousarray(rec_end, dtype=np.uint64)
        if out_cap is None:
            out_cap = self._L.mk_zstd_deflate_bound(src.size)
        out = np.empty(out_cap, dtype=np.uint8)
        n, frames = C.c_uint64(0), C.c_uint64(0)
        rc = self._L.mk_zstd_deflate_records(self._h, src.ctypes.data if src.size else None, src.size, ends.ctypes.data if ends.size else None, ends.size,
                                             out.ctypes.data if out.size else None, out.size, C.byref(n), C.byref(frames))
        self.last_need, self.last_frames = n.value, frames.value
        _check(rc)
        return out[:n.value].tobytes()

    zstd_record_cuts = staticmethod(lambda rec_end: zstd_record_cuts(rec_end))

    def zstd_records_info(self):
        """mk_zstd_deflate_info: (frames, (raw, rle, compressed) blocks, ms of upload / cut + deflate + pack / download) of the last zstd_records"""
        n, kinds, ms = C.c_uint64(0), (C.c_uint32 * 3)(), (C.c_float * 3)()
        _check(self._L.mk_zstd_deflate_info(self._h, C.byref(n), kinds, ms))
        return n.value, tuple(kinds), tuple(ms)

    def cut_times(self):
        """members and ms (cut kernel, CRC-32 + deflate + pack, download) of the last deflate_records call"""
        n, ms = C.c_uint64(0), (C.c_float * 3)()
        _check(self._L.mk_codec_cut_times(self._h, C.byref(n), ms))
        return n.value, tuple(ms)

    def inflate(self, data, members=None, text_bytes=None):
        if members is None:
            members, used, text_bytes = bgzf_members(data)
            if used != len(data):
                raise MerkurioError(MK_E_CORRUPT, "trailing bytes behind the last whole BGZF member")
        src = np.frombuffer(data, dtype=np.uint8)
        out = np.empty(text_bytes, dtype=np.uint8)
        bad = C.c_uint64(0)
        t0 = time.perf_counter()
        rc = self._L.mk_bgzf_inflate(self._h, src.ctypes.data if src.size else None, src.size, members.ctypes.data if members.size else None,
                                     members.size, out.ctypes.data if out.size else None, out.size, C.byref(bad))
        self.last_call_s = time.perf_counter() - t0  # (the C call alone, first touch of the fresh output buffer included)
        _check(rc)
        return out.tobytes()

    def gunzip(self, gz):
        """mk_gzip_inflate_device + mk_gzip_text_read: one gzip member inflated in parallel pieces -> bytes, or None when the device
        did not take the file (the caller's zlib does then).  self.gzip_info = (pieces, ms of upload / search / pieces / resolution / CRC)"""
        src = np.frombuffer(gz, dtype=np.uint8)
        n, taken = C.c_uint64(0), C.c_uint32(0)
        t0 = time.perf_counter()
        _check(self._L.mk_gzip_inflate_device(self._h, src.ctypes.data if src.size else None, src.size, C.byref(n), C.byref(taken)))
        self.last_call_s = time.perf_counter() - t0
        seg, ms = C.c_uint32(0), (C.c_float * 5)()
        _check(self._L.mk_gzip_info(self._h, C.byref(seg), ms))
        self.gzip_info = (seg.value, tuple(round(x, 2) for x in ms))
        if not taken.value:
            return None
        out = np.empty(n.value, dtype=np.uint8)
        t0 = time.perf_counter()
        _check(self._L.mk_gzip_text_read(self._h, 0, out.ctypes.data if out.size else None, out.size))
        self.last_read_s = time.perf_counter() - t0
        return out.tobytes()

    def bunzip2(self, data):
        """mk_bzip2_inflate_device + mk_gzip_text_read: a .bz2 file of one or more streams decoded on the device, a wave per block ->
        (taken, text, n_blocks); taken = False (text None): the device handed the file back and the caller's libbz2 decodes it"""
        src = np.frombuffer(data, dtype=np.uint8)
        n, taken, blocks = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        t0 = time.perf_counter()
        _check(self._L.mk_bzip2_inflate_device(self._h, src.ctypes.data if src.size else None, src.size, C.byref(n), C.byref(taken), C.byref(blocks)))
        self.last_call_s = time.perf_counter() - t0
        if not taken.value:
            return False, None, 0
        out = np.empty(n.value, dtype=np.uint8)
        _check(self._L.mk_gzip_text_read(self._h, 0, out.ctypes.data if out.size else None, out.size))
        return True, out.tobytes(), blocks.value

    def bunzip2_info(self):
        """mk_bzip2_info: (blocks of the last bunzip2, ms of upload / marker search / block decode / text / CRC)"""
        blocks, ms = C.c_uint32(0), (C.c_float * 5)()
        _check(self._L.mk_bzip2_info(self._h, C.byref(blocks), ms))
        return blocks.value, tuple(round(x, 3) for x in ms)

    def unzstd(self, data):
        """mk_zstd_inflate_device + mk_gzip_text_read: a .zst file of one or more frames decoded on the device, a wave per block ->
        (taken, text, n_blocks); taken = False (text None): the device handed the file back and the caller's libzstd decodes it"""
        src = np.frombuffer(data, dtype=np.uint8)
        n, taken, blocks = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        t0 = time.perf_counter()
        _check(self._L.mk_zstd_inflate_device(self._h, src.ctypes.data if src.size else None, src.size, C.byref(n), C.byref(taken), C.byref(blocks)))
        self.last_call_s = time.perf_counter() - t0
        if not taken.value:
            return False, None, 0
        out = np.empty(n.value, dtype=np.uint8)
        _check(self._L.mk_gzip_text_read(self._h, 0, out.ctypes.data if out.size else None, out.size))
        return True, out.tobytes(), blocks.value

    def unzstd_info(self):
        """mk_zstd_info: (blocks, frames, resolution rounds of the last unzstd, ms of upload / tables + entropy decode / scans /
        execution / cross-block rounds / checksum)"""
        blocks, frames, rounds, ms = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), (C.c_float * 6)()
        _check(self._L.mk_zstd_info(self._h, C.byref(blocks), C.byref(frames), C.byref(rounds), ms))
        return blocks.value, frames.value, rounds.value, tuple(round(x, 3) for x in ms)

    def unxz(self, data):
        """mk_xz_inflate_device + mk_gzip_text_read: an .xz file of one or more streams decoded on the device, a wave per block ->
        (taken, text, n_blocks); taken = False (text None): the device handed the file back (unxz_info()[2] says why) and the
        caller's liblzma decodes it"""
        src = np.frombuffer(data, dtype=np.uint8)
        n, taken, blocks = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        t0 = time.perf_counter()
        _check(self._L.mk_xz_inflate_device(self._h, src.ctypes.data if src.size else None, src.size, C.byref(n), C.byref(taken), C.byref(blocks)))
        self.last_call_s = time.perf_counter() - t0
        if not taken.value:
            return False, None, 0
        out = np.empty(n.value, dtype=np.uint8)
        _check(self._L.mk_gzip_text_read(self._h, 0, out.ctypes.data if out.size else None, out.size))
        return True, out.tobytes(), blocks.value

    def unxz_info(self):
        """mk_xz_info: (blocks, streams, status, text bytes of the largest block of the last unxz, ms of upload / decode / check /
        the whole call); status 0 = taken, else the refusal's code (xz_plan.hpp, lzma_serial.hpp)"""
        blocks, streams, status, largest, ms = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0), (C.c_float * 4)()
        _check(self._L.mk_xz_info(self._h, C.byref(blocks), C.byref(streams), C.byref(status), C.byref(largest), ms))
        return blocks.value, streams.value, C.c_int32(status.value).value, largest.value, tuple(round(x, 3) for x in ms)

    def set_xz_spread(self, spread):
        """mk_codec_set_xz_spread: an .xz file is taken only when its largest block's text x spread <= its whole text; 0 = the default"""
        _check(self._L.mk_codec_set_xz_spread(self._h, spread))

    def set_bzip2_pass_blocks(self, blocks):
        """blocks per device pass of bunzip2 (mk_codec_set_bzip2_pass_blocks); 0 = by the free memory"""
        _check(self._L.mk_codec_set_bzip2_pass_blocks(self._h, blocks))

    def set_bzip2_text_cap(self, text_bytes):
        """bytes per text window of bunzip2_stream (mk_codec_set_bzip2_text_cap); 0 = by the free memory"""
        _check(self._L.mk_codec_set_bzip2_text_cap(self._h, text_bytes))

    def bunzip2_stream(self, blob, window=0):
        """mk_bzip2_stream_begin / _next / _end: a .bz2 file of any size decoded window by window (`window` compressed bytes each, 0 =
        the default) -> a generator of the text windows.  self.stream_state = 1 when it ends at the file's end (every block and
        stream CRC agrees), 2 when the device handed the file back (what was yielded before is a prefix of libbz2's text; nothing
        was, for a file without "BZh1-9" in front); self.stream_stats = mk_bzip2_stream_info of the stream as it ended (a dict)"""
        return self._stream(_BZIP2_STREAM, blob, window)

    def unzstd_stream_info(self):
        """mk_zstd_stream_info as a dict: of the open stream, or what the last one left"""
        return self._stream_info(_ZSTD_STREAM)

    def unzstd_stream(self, blob, window_bytes=0, text_cap=0):
        """mk_zstd_stream_begin / _next / _end: a .zst file of any size decoded window by window (`window_bytes` compressed bytes
        each, 0 = the default; text_cap: mk_codec_set_zstd_text_cap for this stream, 0 = by the free memory) -> a generator of the
        windows' texts.  self.stream_state = 1 when it ends at the file's end (every frame's size and checksum agrees), 2 when the
        device handed the file back (what was yielded before is a prefix of libzstd's text; nothing was, for a file that starts
        with no frame); self.stream_stats = unzstd_stream_info() of the stream as it ended, self.stream_windows = that dict behind
        every call of _next (a list)"""
        return self._stream(_ZSTD_STREAM, blob, window_bytes, text_cap)

    def unxz_stream_info(self):
        """mk_xz_stream_info as a dict: of the open stream, or what the last one left (a refusal at _begin included: its status)"""
        return self._stream_info(_XZ_STREAM)

    def unxz_stream(self, blob, window_bytes=0, text_cap=0):
        """mk_xz_stream_begin / _next / _end: an .xz file of any size decoded window by window (`window_bytes`: a bound on a window's
        compressed span, 0 = none; text_cap: mk_codec_set_xz_text_cap for this stream, 0 = by the free memory) -> a generator of the
        windows' texts.  self.stream_state = 1 when it ends at the file's end (every block proved), 2 when the device handed the file
        back (what was yielded before is a prefix of liblzma's text in whole blocks; nothing was, for a file refused at _begin);
        self.stream_stats = unxz_stream_info() of the stream as it ended (its status names a refusal),
        self.stream_windows = that dict behind every call of _next (a list)"""
        return self._stream(_XZ_STREAM, blob, window_bytes, text_cap)

    def gunzip_members(self, gz):
        """mk_gzip_members_inflate_device + mk_gzip_text_read: a gzip file of one or more members, all of them inflated in one batch of
        parallel pieces -> (text of all members, how many members were proved), or None when the device did not take the file"""
        src = np.frombuffer(gz, dtype=np.uint8)
        n, taken, members = C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        t0 = time.perf_counter()
        _check(self._L.mk_gzip_members_inflate_device(self._h, src.ctypes.data if src.size else None, src.size, C.byref(n), C.byref(taken), C.byref(members)))
        self.last_call_s = time.perf_counter() - t0
        seg, ms = C.c_uint32(0), (C.c_float * 5)()
        _check(self._L.mk_gzip_info(self._h, C.byref(seg), ms))
        self.gzip_info = (seg.value, tuple(round(x, 2) for x in ms))
        if not taken.value:
            return None
        out = np.empty(n.value, dtype=np.uint8)
        _check(self._L.mk_gzip_text_read(self._h, 0, out.ctypes.data if out.size else None, out.size))
        return out.tobytes(), members.value

    def gunzip_stream(self, blob, window=0):
        """mk_gzip_stream_begin / _next / _end: a gzip file of any size inflated window by window (`window` compressed bytes each, 0 =
        the default) -> a generator of the windows' texts.  self.stream_state = 1 when it ends at the file's end (every member proved),
        2 when the device handed the file back (what was yielded before is zlib's prefix; nothing was, for a file that is not gzip);
        self.stream_stats = mk_gzip_stream_info of the stream as it ended (a dict)"""
        return self._stream(_GZIP_STREAM, blob, window)

    def _stream_info(self, calls):
        st = calls.stats()
        _check(getattr(self._L, calls.info)(self._h, C.byref(st)))
        return _stats_dict(st)

    def _stream(self, calls, blob, window, text_cap=None):
        """The generator behind gunzip_stream, bunzip2_stream, unzstd_stream and unxz_stream: `calls` names the format's _begin / _next /
        _info / _end, its stats struct and (or None) the setter of the text cap, which the stream takes when it begins"""
        src = np.frombuffer(blob, dtype=np.uint8)
        taken = C.c_uint32(0)
        self.stream_state, self.stream_stats, self.stream_windows = 2, None, []
        if calls.set_text_cap:
            _check(getattr(self._L, calls.set_text_cap)(self._h, text_cap))
        try:
            _check(getattr(self._L, calls.begin)(self._h, src.ctypes.data if src.size else None, src.size, window, C.byref(taken)))
        finally:
            if calls.set_text_cap:
                _check(getattr(self._L, calls.set_text_cap)(self._h, 0))  # (the stream took it when it began)
        if calls.refusal_in_stats:
            self.stream_stats = self._stream_info(calls)
        if not taken.value:
            return
        try:
            n, state = C.c_uint64(0), C.c_uint32(0)
            while True:
                _check(getattr(self._L, calls.next)(self._h, C.byref(n), C.byref(state)))
                self.stream_stats = self._stream_info(calls)
                self.stream_windows.append(self.stream_stats)
                self.stream_state = state.value
                if state.value != 0:
                    return
                out = np.empty(n.value, dtype=np.uint8)
                _check(self._L.mk_gzip_text_read(self._h, 0, out.ctypes.data if out.size else None, out.size))
                yield out.tobytes()
        finally:
            _check(getattr(self._L, calls.end)(self._h))

    def set_inflate_kernel(self, which=0):
        """0 = chosen per call, 1 = a lane per member, 2 = a wave per member (mk_codec_set_inflate_kernel)"""
        _check(self._L.mk_codec_set_inflate_kernel(self._h, which))

    def set_gzip_chunk(self, chunk_bytes=0):
        """nominal distance between two cuts of a gzip stream (mk_codec_set_gzip_chunk); 0 = by the stream's size"""
        _check(self._L.mk_codec_set_gzip_chunk(self._h, chunk_bytes))

    def set_pass_limits(self, deflate_members=0, inflate_text_bytes=0):
        _check(self._L.mk_codec_set_pass_limits(self._h, deflate_members, inflate_text_bytes))

    def times(self):
        ms = (C.c_float * 3)()
        _check(self._L.mk_codec_times(self._h, ms))
        return tuple(ms)
