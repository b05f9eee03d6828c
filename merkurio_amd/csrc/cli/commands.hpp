// commands.hpp -- argument structs of the two subcommands (clap structs of
// src/cmd_extract.rs:32-141 and src/cmd_tag.rs:29-150) and their drivers.
#pragma once
#include <optional>
#include <string>
#include <vector>

#include "util.hpp"

namespace cli {

struct CommonArgs {
    std::vector<std::string> kmer_seq;     // -s
    std::optional<std::string> kmer_file;  // -f
    bool reverse_complement = false;       // -r
    bool canonical = false;                // -c
    std::optional<std::string> out_log;    // -l [path]   ("STDOUT" when given without a value)
    std::optional<std::string> json_log;   // -j [path]
    bool suppress_output = false;          // -S
    bool invert_match = false;             // -v
    bool case_insensitive = false;         // -I
    bool lowercase = false;                // -L
    bool uppercase = false;                // -U
    std::optional<size_t> q_size;          // -q
    bool aho_corasick = false;             // -a
    // opt-in extras of this build (defaults reproduce the reference behaviour)
    int device = 0;       // --device
    int gpus = 1;         // --gpus N: records sharded over N devices, outputs in device order, counters reduced with RCCL
    int window_mb = 1024;  // --window-mb: text (decompressed) read, indexed and held per window of an extract input
    int batch_mb = 128;  // --batch-mb: sequence bytes per GPU batch (tools/batch_mb.sh: 128-256 MB is fastest end to end)
    bool host_codec = false;   // --host-codec: BGZF members are deflated / inflated by zlib on the host threads instead of the device codec
    bool device_codec_always = false;  // --device-codec-always: BGZF input goes through the device codec however few members a call holds (tests: the
                                       // reference's own small BAM / bgzip'ed fixtures through mk_bgzf_inflate)
    bool window_mb_given = false;      // --window-mb was on the command line (its default does not bind the paths that keep the text on the device)
    bool host_ingest = false;  // --host-ingest: extract parses its records on the host threads even where the device could index them; tag keeps the r04 path
                               // (BAM records indexed and tagged on the host threads) where BAM -> BAM would keep them on the device
};

// (the sweep of DESIGN.md §5.9, for -z: inside the parent build's range at 1 % kept, ahead of it from 20 %.  For --zstd-output the same
// value is an UNMEASURED choice: 64-73 frames per launch, on a kernel that keeps 8 waves per CU)
constexpr uint64_t kZMembersFrom = 8ull << 20;

constexpr uint64_t kGzipWindow = 256ull << 20;  // (an unmeasured choice: README, "Gunzip window by window")
constexpr uint64_t kXzWindow = 256ull << 20;     // (an unmeasured choice, the zstd and bzip2 value: profiles/e2e_unxz.txt)
constexpr uint64_t kZstdWindow = 256ull << 20;   // (an unmeasured choice, like its siblings: profiles/e2e_unzstd.txt)
constexpr uint64_t kBzip2Window = 256ull << 20;  // (an unmeasured choice: README, "Bunzip2 window by window"; profiles/e2e_bunzip2_windows.txt)

struct ExtractArgs : CommonArgs {
    std::string in_fastx;                   // -i / -1
    std::optional<std::string> in_fastq_2;  // -2
    std::optional<std::string> out_fastx;   // -o
    bool bgzf_output = false;               // -z: the kept records are written as BGZF members that end at record ends (output name + ".gz")
    bool zstd_output = false;               // --zstd-output: the kept records are written as zstd frames that end at record ends (output name + ".zst")
    // --z-members-from: with -z or --zstd-output on the window path, a window whose written kept records take this many bytes or more is
    // cut and compressed where it lies and comes down as members (mk_extract_window_members) or frames (mk_extract_window_frames); a
    // smaller one comes down as text and gathers with its neighbours
    uint64_t z_members_from = kZMembersFrom;
    // --gzip-window: a plain gzip input of more compressed bytes than this is inflated on the device window by window (mk_gzip_stream_*),
    // a smaller one in one piece (mk_gzip_inflate_device / mk_gzip_members_inflate_device)
    uint64_t gzip_window = kGzipWindow;
    // --bzip2-window: likewise for a .bz2 input (mk_bzip2_stream_*; a smaller one: mk_bzip2_inflate_device)
    uint64_t bzip2_window = kBzip2Window;
    // --device-zstd: a .zst input of at most --zstd-window compressed bytes is decoded on the device in one call
    // (mk_zstd_inflate_device); a larger one, and every .zst input without the flag, is libzstd's.  Opt-in: the path has not been timed
    bool device_zstd = false;
    // --zstd-stream (implies --device-zstd): a larger .zst input is decoded window by window (mk_zstd_stream_*), each window of
    // about --zstd-window compressed bytes.  Opt-in like its sibling: not timed
    bool zstd_stream = false;
    uint64_t zstd_window = kZstdWindow;
    // --device-xz: an .xz input of at most --xz-window compressed bytes is decoded on the device in one call (mk_xz_inflate_device),
    // when its largest block's text x --xz-spread <= its whole text (0 = the library's default, 107: profiles/e2e_unxz.txt); a larger one, one
    // the rule or the call hands back, and every .xz input without the flag, is liblzma's.  Opt-in: the path has not been timed
    bool device_xz = false;
    uint64_t xz_window = kXzWindow;
    uint32_t xz_spread = 0;
    // --xz-stream (implies --device-xz): a larger .xz input is decoded window by window (mk_xz_stream_*), windows of whole blocks
    // bounded by --xz-text-cap bytes of text (0 = the library's default, by the free device memory).  Opt-in like its sibling: not timed
    bool xz_stream = false;
    // --open-windows: the windows of ONE bgzip'ed input with plain-text output start at member boundaries and find their own first
    // record (mk_extract_window_open); the text between two windows goes through a seam call that also proves the found start
    bool open_windows = false;
    uint64_t xz_text_cap = 0;
};

struct TagArgs : CommonArgs {
    std::string in_file;                  // -i
    std::optional<std::string> out_file;  // -o
    std::string tag = "km";               // -t
    int threads = 1;                      // -p
    bool threads_given = false;           // -p on the command line: caps the codec threads (default: all cores)
    bool filter_matching = false;         // -m
};

int run_extract(const ExtractArgs &a, const std::vector<std::string> &argv);
int run_tag(const TagArgs &a, const std::vector<std::string> &argv);

}  // namespace cli
