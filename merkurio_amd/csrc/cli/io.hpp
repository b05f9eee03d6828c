// io.hpp -- record readers/writers of the `merkurio` CLI (host side, either side of the hot
// path), one header per subject.  Observable behaviour follows what the reference gets from its crates
// (SURVEY.md §5): needletail 0.6.3 for FASTA/FASTQ (src/cmd_extract.rs:281,327-340,403) and
// bam 0.1.4 for SAM/BAM (src/cmd_tag.rs:470-497,503-615).
#pragma once
#include "host_mem.hpp"       // host threads, page-locked buffers, the host-memory check
#include "file_bytes.hpp"     // a file's bytes: mapping or inflated copy; bzip2 / xz / zstd by magic
#include "bgzf_in.hpp"        // BGZF member table, runs of members, their inflate (device codec or host threads)
#include "window_source.hpp"  // the decompressed bytes of an input, a window at a time
#include "fastx.hpp"          // FASTA / FASTQ records and windows
#include "sam_in.hpp"         // SAM / BAM records and windows
#include "bam_text.hpp"       // a BAM record as a SAM text line
#include "bam_out.hpp"        // BamWriter, SAM line -> BAM record, BGZF members by zlib
